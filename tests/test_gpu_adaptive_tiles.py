"""Adaptive rounds and the a-trous filter on row-tiled frames (DESIGN.md §18 "Row tiles", §19).

The invariant: a pixel's stream depends only on (seed, x, y), the adaptive criterion is per 8x8
tile, and tiling.partition_rows deals whole 8-row blocks in ascending order, so every 8x8 tile of a
rank's context is a tile of the monolithic frame with the same pixels (the partial last block
too).  A row-tiled adaptive render, gathered with its moments and filtered, therefore equals one
context's render_adaptive and filter_frame bit for bit: accumulator, normals, moments, noise map,
filtered rgb and variance, and the tiles' pass counts sum to the one context's.  Every context
here sits on device 0 (a device may repeat, as in tests/test_gpu_devices.py).
"""
import os
import re
import subprocess

import filter_model as fm
import numpy as np
import pytest

from cpppathtracer_amd import CptError, Renderer, camera_get_copy, multigpu, scenes, tiling
from cpppathtracer_amd._lib import CPT_ERR_STATE, CPT_RENDER_AUX, CPT_TRAVERSAL_ORDERED

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 1234
CASES = {
    # tests/test_gpu_filter.py's PARITY: S4, 64 x 64, depth 8, batch 4, 8..32 spp, rel_error 0.1
    "parity": dict(scene=scenes.scene_s4, W=64, H=64, depth=8, batch=4, min_spp=8, max_spp=32, t=0.1,
                   flags=CPT_RENDER_AUX),
    # tests/test_gpu_adaptive.py's partial_tiles_20x12: S1000 n = 40, ordered walk, 8..16 spp, 0.05
    "partial": dict(scene=lambda: scenes.scene_s1000(n=40), W=20, H=12, depth=8, batch=4, min_spp=8, max_spp=16, t=0.05,
                    flags=CPT_RENDER_AUX | CPT_TRAVERSAL_ORDERED),
}
_cache = {}


def _setup(r, sky, case, rows=None):
    c = CASES[case]
    r.set_scene(c["scene"]())
    r.set_env(sky)
    r.set_frame(c["W"], c["H"], rows)
    r.init_rng(SEED)
    return camera_get_copy(scenes.camera_for(c["W"], c["H"]))


def _args(case, cam):
    c = CASES[case]
    return (cam, c["min_spp"], c["max_spp"], c["batch"], c["t"], c["depth"]), dict(flags=c["flags"])


def _state(r):
    """Everything an adaptive render leaves that the gather carries."""
    normal, depth = r.read_aux()
    return dict(accum=r.read_accum(), normal=normal, depth=depth, moments=r.read_moments(), noise=r.read_noise())


def _filtered(r):
    r.filter_frame()
    rgb, var = r.read_filtered()
    return dict(rgb=rgb, var=var)


def _same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        fm.assert_same_bits(got[k], want[k], f"{what}: {k}")


def _reference(gpu, sky, case):
    """One context's render_adaptive and filter_frame of the case, computed once and shared (read only)."""
    if case not in _cache:
        cam = _setup(gpu, sky, case)
        a, kw = _args(case, cam)
        info = gpu.render_adaptive(*a, **kw)
        ref = dict(info=info, state=_state(gpu), rng=gpu.read_rng())
        ref["filtered"] = _filtered(gpu)
        for v in list(ref["state"].values()) + list(ref["filtered"].values()) + [ref["rng"]]:
            v.flags.writeable = False
        _cache[case] = ref
    return _cache[case]


class _Tiled:
    """`world` tile contexts of the case's partition_rows (or the ranks in `only`) and a frame context."""

    def __init__(self, sky, case, world, only=None, staged=False):
        c = CASES[case]
        self.case, self.tiles, self.frame = case, [], None
        try:
            for rank in (range(world) if only is None else only):
                t = Renderer(0)
                self.tiles.append(t)
                self.cam = _setup(t, sky, case, tiling.partition_rows(c["H"], world, rank))
            self.frame = Renderer(0)
            self.frame.set_frame(c["W"], c["H"])
            if staged:
                self.frame.set_debug_gather(True)
        except Exception:
            self.close()
            raise

    def render(self):
        a, kw = _args(self.case, self.cam)
        return multigpu.render_adaptive_tiled(self.frame, self.tiles, *a, **kw)

    def close(self):
        for r in self.tiles + ([self.frame] if self.frame else []):
            r.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _assert_stitched_equals_one_context(gpu, sky, case, world, staged=False):
    c = CASES[case]
    ref = _reference(gpu, sky, case)
    with _Tiled(sky, case, world, staged=staged) as t:
        per_tile = t.render()
        assert [t.frame.last_gather_mode(s) for s in t.tiles] == ["staged" if staged else "same_device"] * world
        state = _state(t.frame)
        _same(state, ref["state"], f"{case} world {world}")
        info = t.frame.adaptive_info()
        assert info["rounds"] == 0 and info["passes_done"] == 0     # a gathered result: an empty round record
        filtered = _filtered(t.frame)
        _same(filtered, ref["filtered"], f"{case} world {world} filtered")
    want = fm.run(state["accum"], state["moments"], state["normal"], c["W"], c["H"])
    fm.assert_same_bits(filtered["rgb"], want[0], "filter model rgb")
    fm.assert_same_bits(filtered["var"], want[1], "filter model variance")
    assert sum(p for _, p in per_tile) == ref["info"]["passes_done"]
    assert max(r for r, _ in per_tile) == ref["info"]["rounds"]
    return ref


@pytest.mark.parametrize("world", [2, 3])
def test_stitched_equals_one_context(gpu, sky, world):
    ref = _assert_stitched_equals_one_context(gpu, sky, "parity", world)
    k = ref["state"]["moments"][2]
    assert len(set(k.tolist())) >= 3 and (k >= 2).all()             # tiles stop at different rounds


def test_partial_tiles(gpu, sky):
    """20 x 12 at world 2: rank 1 owns the 4-row partial block, and the tiles are 4 pixels wide at the right edge."""
    assert tiling.partition_rows(12, 2, 1).tolist() == [8, 9, 10, 11]
    ref = _assert_stitched_equals_one_context(gpu, sky, "partial", 2)
    assert len(set(ref["state"]["moments"][2].tolist())) == 2       # rounds 3 and 4


def test_staged_branch(gpu, sky):
    _assert_stitched_equals_one_context(gpu, sky, "parity", 2, staged=True)


def test_uncovered_rows(gpu, sky):
    """Rank 0 of 2 alone into a fresh frame: rank 1's rows are pixels before their second batch."""
    c = CASES["parity"]
    W, H = c["W"], c["H"]
    ref = _reference(gpu, sky, "parity")
    with _Tiled(sky, "parity", 2, only=[0]) as t:
        t.render()
        state = _state(t.frame)
        filtered = _filtered(t.frame)
    mine = np.zeros(H, dtype=bool)
    mine[tiling.partition_rows(H, 2, 0)] = True
    px = np.repeat(mine, W)
    assert px.any() and (~px).any()
    for k in ("accum", "normal", "depth", "noise"):
        fm.assert_same_bits(state[k][px], ref["state"][k][px], f"rank 0's rows: {k}")
    fm.assert_same_bits(state["moments"][:, px], ref["state"]["moments"][:, px], "rank 0's rows: moments")
    assert (state["moments"][:3][:, ~px].view(np.uint32) == 0).all()
    assert np.isposinf(state["noise"][~px]).all() and np.isposinf(state["moments"][3][~px]).all()
    assert (state["accum"][~px] == 0).all()
    want = fm.run(state["accum"], state["moments"], state["normal"], W, H)
    fm.assert_same_bits(filtered["rgb"], want[0], "filter model rgb")
    fm.assert_same_bits(filtered["var"], want[1], "filter model variance")


def test_split_calls_equal_render_adaptive(gpu, sky):
    ref = _reference(gpu, sky, "parity")
    with Renderer(0) as r:
        cam = _setup(r, sky, "parity")
        a, kw = _args("parity", cam)
        r.adaptive_begin(*a, **kw)
        seen = []
        while True:
            seen.append(r.adaptive_step())
            if seen[-1] == 0:
                break
        info = r.adaptive_info()
        _same(_state(r), ref["state"], "begin + step")
        np.testing.assert_array_equal(r.read_rng(), ref["rng"])
        _same(_filtered(r), ref["filtered"], "begin + step filtered")
    np.testing.assert_array_equal(info["active_tiles"], ref["info"]["active_tiles"])
    assert info["rounds"] == ref["info"]["rounds"] and info["passes_done"] == ref["info"]["passes_done"]
    # each step but the last returns the tiles of the round it queued
    assert seen == ref["info"]["active_tiles"][1:].tolist() + [0]


def test_step_order_does_not_matter(sky):
    """Two tile contexts stepped A, B, A, B ... equal the same two stepped A to its end, then B."""
    results = []
    for interleaved in (True, False):
        with _Tiled(sky, "parity", 2) as t:
            a, kw = _args("parity", t.cam)
            for r in t.tiles:
                r.adaptive_begin(*a, **kw)
            if interleaved:
                left = list(t.tiles)
                while left:
                    left = [r for r in left if r.adaptive_step() > 0]
            else:
                for r in t.tiles:
                    while r.adaptive_step() > 0:
                        pass
            results.append([dict(_state(r), rng=r.read_rng(), active=r.adaptive_info()["active_tiles"]) for r in t.tiles])
    for rank, (x, y) in enumerate(zip(*results)):
        _same(x, y, f"rank {rank}")


def test_pending_state_codes(gpu, sky):
    def status(fn, *args, **kw):
        with pytest.raises(CptError) as e:
            fn(*args, **kw)
        return e.value.status

    c = CASES["parity"]
    with Renderer(0) as r, Renderer(0) as frame:
        cam = _setup(r, sky, "parity", tiling.partition_rows(c["H"], 2, 0))
        frame.set_frame(c["W"], c["H"])
        a, kw = _args("parity", cam)
        assert status(r.adaptive_step) == CPT_ERR_STATE              # nothing pending
        r.adaptive_begin(*a, **kw)
        assert status(r.render, cam, 1, c["depth"]) == CPT_ERR_STATE
        assert status(r.render_adaptive, *a, **kw) == CPT_ERR_STATE
        assert status(r.adaptive_begin, *a, **kw) == CPT_ERR_STATE
        assert status(r.set_frame, c["W"], c["H"]) == CPT_ERR_STATE
        assert status(frame.gather_rows, r) == CPT_ERR_STATE
        assert status(r.read_noise) == CPT_ERR_STATE                 # no adaptive result yet
        while r.adaptive_step() > 0:                                 # the refused calls changed nothing
            pass
        assert status(r.adaptive_step) == CPT_ERR_STATE
        frame.gather_rows(r)
        ref = _reference(gpu, sky, "parity")
        px = np.repeat(np.isin(np.arange(c["H"]), tiling.partition_rows(c["H"], 2, 0)), c["W"])
        fm.assert_same_bits(frame.read_accum()[px], ref["state"]["accum"][px], "after the refused calls")
        fm.assert_same_bits(frame.read_moments()[:, px], ref["state"]["moments"][:, px], "after the refused calls")
        # and a plain render works again
        r.render(cam, 1, c["depth"], sync=True)
        assert (r.read_accum()[:, 3] == 1).all()
    # a pending context is destroyed without being stepped
    r = Renderer(0)
    cam = _setup(r, sky, "parity")
    r.adaptive_begin(*_args("parity", cam)[0], **_args("parity", cam)[1])
    r.close()


def test_plain_gather_leaves_the_moments_alone(sky):
    c = CASES["parity"]
    with _Tiled(sky, "parity", 2) as t:
        for r in t.tiles:
            r.render(t.cam, 2, c["depth"], aux=True)
        for r in t.tiles:
            t.frame.gather_rows(r)
        assert (t.frame.read_accum()[:, 3] == 2).all()
        with pytest.raises(CptError) as e:
            t.frame.read_moments()
        assert e.value.status == CPT_ERR_STATE
        with pytest.raises(CptError) as e:
            t.frame.filter_frame()
        assert e.value.status == CPT_ERR_STATE


def test_cpp_api_devices(tmp_path):
    """cpt_headless --adaptive --filter with --devices 2 writes the one-device PFM, byte for byte."""
    from cpppathtracer_amd import build
    exe = build.build_examples()
    out = {}
    for n in (1, 2):
        pfm = tmp_path / f"d{n}.pfm"
        r = subprocess.run([exe, "--scene", "s4", "--width", "64", "--height", "48", "--depth", "8", "--spp", "32",
                            "--min-spp", "8", "--batch", "4", "--adaptive", "0.1", "--filter", "--pfm", str(pfm),
                            "--devices", str(n)], cwd=REPO, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert f"on {n} device context(s)" in r.stdout and "filtered: 5 levels" in r.stdout, r.stdout
        m = re.search(r"adaptive: .*: (\d+) rounds, passes_done (\d+) ", r.stdout)
        assert m, r.stdout
        out[n] = (pfm.read_bytes(), int(m.group(1)), int(m.group(2)))
    assert len(out[1][0]) > 64 * 48 * 12
    assert out[2][0] == out[1][0]
    assert out[2][1:] == out[1][1:]
    assert 0 < out[1][2] < 64 * 48 * 32                              # tiles did stop early
