"""cpt_render_adaptive against the oracle, bit for bit (DESIGN.md §Adaptive sampling).

The invariant: after an adaptive render every pixel's accumulator (rgb sums and count) and RNG
state are those of a plain render of that pixel's own number of passes.  The oracle renders every
pixel for every round; tests/adaptive_model.py decides each 8x8 tile's stop round with the numpy
restatement of the criterion and takes each pixel from that round.  Each test asserts on the model,
before any GPU call, that its tiles do stop at different rounds.
"""
import ctypes

import adaptive_model as am
import numpy as np
import pytest

from cpppathtracer_amd import CptError, Renderer, _lib, camera_get_copy, scenes
from cpppathtracer_amd._lib import (CPT_PATH_WAVEFRONT, CPT_RENDER_ACCUMULATE, CPT_RENDER_AUX, CPT_SCHEDULE_COST,
                                    CPT_SCHEDULE_PREVIOUS, CPT_TRAVERSAL_ORDERED)

pytestmark = pytest.mark.gpu

SEED = 1234
# Case 2 (S4, 64 x 64, depth 8, batch 4, 8..32 spp): at this rel_error the oracle's model stops 12
# tiles at round 2 (the first eligible one), 31 at rounds 3..6 and 21 at round 8 (found on the CPU).
PARITY = dict(W=64, H=64, depth=8, batch=4, min_spp=8, max_spp=32, t=0.1)
_cache = {}


def _frame(gpu, sky, objs, W, H, rows):
    rows = np.arange(H, dtype=np.int32) if rows is None else np.asarray(rows, dtype=np.int32)
    cam = camera_get_copy(scenes.camera_for(W, H))
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H, rows)
    gpu.init_rng(SEED)
    return cam, rows


def _model(oracle_mod, sky, objs, cam, W, rows, depth, batch, min_spp, max_spp, t, aux=False, before=0):
    """The model of an adaptive render after `before` plain passes (with CPT_RENDER_ACCUMULATE)."""
    rng = oracle_mod.init_rng(SEED, W, rows, threads=8)
    acc0 = None
    if before:
        acc0 = oracle_mod.render(objs, cam, sky, rows, before, depth, rng, threads=8)[0]
    snaps = am.oracle_rounds(oracle_mod, objs, cam, sky, rows, batch, max_spp // batch, depth, rng, acc0=acc0, aux=aux)
    return am.run(snaps, W, rows.size, batch, min_spp, max_spp, np.float32(t), acc0=acc0)


def _parity_model(oracle_mod, sky):
    """Case 2's model, computed once and shared (read only)."""
    if "parity" not in _cache:
        p = PARITY
        cam = camera_get_copy(scenes.camera_for(p["W"], p["H"]))
        m = _model(oracle_mod, sky, scenes.scene_s4(), cam, p["W"], np.arange(p["H"], dtype=np.int32), p["depth"],
                   p["batch"], p["min_spp"], p["max_spp"], p["t"], aux=True)
        first, last = p["min_spp"] // p["batch"], p["max_spp"] // p["batch"]
        assert (m["stop"] == first).any() and (m["stop"] == last).any()
        assert ((m["stop"] > first) & (m["stop"] < last)).any()
        _cache["parity"] = m
    return _cache["parity"]


def _assert_state(gpu, info, m, noise=True):
    np.testing.assert_array_equal(info["active_tiles"], m["active"])
    assert info["rounds"] == len(m["active"]) and info["passes_done"] == m["passes_done"]
    np.testing.assert_array_equal(gpu.read_rng(), m["rng"])
    np.testing.assert_array_equal(gpu.read_accum().view(np.uint32), m["accum"].view(np.uint32))
    if noise:
        np.testing.assert_array_equal(gpu.read_noise().view(np.uint32), m["noise"].view(np.uint32))


def test_min_equals_max_is_a_plain_render(gpu, sky):
    W = H = 64
    objs = scenes.scene_s4()
    cam, _ = _frame(gpu, sky, objs, W, H, None)
    info = gpu.render_adaptive(cam, 32, 32, 8, 0.05, 8)
    assert info["rounds"] == 4 and info["passes_done"] == W * H * 32
    np.testing.assert_array_equal(info["active_tiles"], [64, 64, 64, 64])
    acc, rng = gpu.read_accum(), gpu.read_rng()
    assert np.isfinite(gpu.read_noise()).all()
    with Renderer(0) as other:
        cam2, _ = _frame(other, sky, objs, W, H, None)
        other.render(cam2, 32, 8, sync=True)
        np.testing.assert_array_equal(rng, other.read_rng())
        np.testing.assert_array_equal(acc.view(np.uint32), other.read_accum().view(np.uint32))
    assert (acc[:, 3] == 32).all()


def test_parity_with_the_model(gpu, oracle_mod, sky):
    p = PARITY
    m = _parity_model(oracle_mod, sky)
    cam, _ = _frame(gpu, sky, scenes.scene_s4(), p["W"], p["H"], None)
    info = gpu.render_adaptive(cam, p["min_spp"], p["max_spp"], p["batch"], p["t"], p["depth"], flags=CPT_RENDER_AUX)
    _assert_state(gpu, info, m)
    normal, depth = gpu.read_aux()
    np.testing.assert_array_equal(normal.view(np.uint32), m["normal"].view(np.uint32))
    assert (depth == np.float32(1e30)).all()
    counts = gpu.read_accum()[:, 3]
    np.testing.assert_array_equal(counts, (m["stop"][am.tile_of_pixel(p["W"], p["H"])] * p["batch"]).astype(np.float32))


# Case 3: S1000 with 40 objects, CPT_TRAVERSAL_ORDERED, depth 8, batch 4, 8..16 spp; at rel_error 0.05
# the oracle's model stops some tiles of each frame at round 3 and runs the others to round 4.
SHAPES = {
    "partial_tiles_20x12": dict(W=20, H=12, rows=None),
    "row_list_64": dict(W=64, H=48, rows=list(range(0, 4)) + list(range(8, 12)) + list(range(40, 48))),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(gpu, oracle_mod, sky, name):
    s = SHAPES[name]
    W, H = s["W"], s["H"]
    rows = np.arange(H, dtype=np.int32) if s["rows"] is None else np.asarray(s["rows"], dtype=np.int32)
    objs = scenes.scene_s1000(n=40)
    cam = camera_get_copy(scenes.camera_for(W, H))
    m = _model(oracle_mod, sky, objs, cam, W, rows, 8, 4, 8, 16, 0.05)
    assert (m["stop"] == 3).any() and (m["stop"] == 4).any()   # tiles stop at different rounds
    if name == "partial_tiles_20x12":
        assert len(m["stop"]) == 6 and W % 8 and H % 8
    cam, rows = _frame(gpu, sky, objs, W, H, s["rows"])
    info = gpu.render_adaptive(cam, 8, 16, 4, 0.05, 8, flags=CPT_TRAVERSAL_ORDERED)
    _assert_state(gpu, info, m)


@pytest.mark.parametrize("how", ["cost_ordered", "one_workgroup_of_two"])
def test_tile_order_does_not_matter(gpu, oracle_mod, sky, how):
    """The stable compaction of the cost schedule's heaviest-first order, and a grid capped at two
    workgroups (lanes take several pixels in turn): the same state and per-round counts as case 2."""
    p = PARITY
    m = _parity_model(oracle_mod, sky)
    cam, _ = _frame(gpu, sky, scenes.scene_s4(), p["W"], p["H"], None)
    flags = CPT_SCHEDULE_COST | CPT_TRAVERSAL_ORDERED if how == "cost_ordered" else 0
    if how != "cost_ordered":
        gpu.set_debug_grid(2, 0)
    try:
        info = gpu.render_adaptive(cam, p["min_spp"], p["max_spp"], p["batch"], p["t"], p["depth"], flags=flags)
    finally:
        gpu.set_debug_grid(0, 0)
    _assert_state(gpu, info, m)


def test_accumulate_starts_from_the_current_accumulator(gpu, oracle_mod, sky):
    W = H = 64
    objs = scenes.scene_s4()
    cam = camera_get_copy(scenes.camera_for(W, H))
    m = _model(oracle_mod, sky, objs, cam, W, np.arange(H, dtype=np.int32), 8, 4, 8, 24, 0.1, before=8)
    assert len(set(m["stop"].tolist())) >= 2
    cam, _ = _frame(gpu, sky, objs, W, H, None)
    gpu.render(cam, 8, 8, sync=True)
    info = gpu.render_adaptive(cam, 8, 24, 4, 0.1, 8, flags=CPT_RENDER_ACCUMULATE)
    _assert_state(gpu, info, m)
    assert (gpu.read_accum()[:, 3] >= 16).all()


def test_status_codes(gpu, oracle_mod, sky):
    INVALID, STATE, UNSUPPORTED = 1, 5, 6
    W, H, depth = 40, 24, 8
    objs = scenes.scene_s4()
    cam, rows = _frame(gpu, sky, objs, W, H, None)

    def status(*args, **kw):
        with pytest.raises(CptError) as e:
            gpu.render_adaptive(cam, *args, **kw)
        return e.value.status

    with pytest.raises(CptError) as e:
        gpu.read_noise()   # no adaptive render since set_frame
    assert e.value.status == STATE
    L = _lib.load()
    assert L.cpt_adaptive_info(gpu._ctx, None, None, 0, None) == STATE
    #              min max batch rel depth
    assert status(8, 32, 0, 0.1, depth) == INVALID      # batch >= 1
    assert status(8, 32, -4, 0.1, depth) == INVALID
    assert status(10, 32, 4, 0.1, depth) == INVALID     # min_spp not a multiple
    assert status(8, 30, 4, 0.1, depth) == INVALID      # max_spp not a multiple
    assert status(16, 8, 4, 0.1, depth) == INVALID      # min_spp > max_spp
    assert status(0, 8, 4, 0.1, depth) == INVALID       # batch <= min_spp
    assert status(4, 8, 4, 0.1, depth) == INVALID       # min_spp >= 2 batch unless min == max
    assert status(8, 32, 4, -0.1, depth) == INVALID     # rel_error >= 0
    assert status(8, 32, 4, float("nan"), depth) == INVALID
    assert status(8, 32, 4, 0.1, 33) == INVALID
    assert status(8, 32, 4, 0.1, depth, flags=CPT_PATH_WAVEFRONT) == UNSUPPORTED
    assert status(8, 32, 4, 0.1, depth, flags=CPT_SCHEDULE_PREVIOUS) == UNSUPPORTED
    with Renderer(0) as fresh:
        with pytest.raises(CptError) as e:
            fresh.render_adaptive(cam, 8, 32, 4, 0.1, depth)
        assert e.value.status == STATE                  # no scene
        fresh.set_scene(objs)
        with pytest.raises(CptError) as e:
            fresh.render_adaptive(cam, 8, 32, 4, 0.1, depth)
        assert e.value.status == STATE                  # no frame
        fresh.set_frame(W, H)
        with pytest.raises(CptError) as e:
            fresh.render_adaptive(cam, 8, 32, 4, 0.1, depth)
        assert e.value.status == STATE                  # no RNG
    # the failed calls left the context as it was: a plain render still matches the oracle
    gpu.render(cam, 4, depth, sync=True)
    rng = oracle_mod.init_rng(SEED, W, rows, threads=8)
    o_acc = oracle_mod.render(objs, cam, sky, rows, 4, depth, rng, threads=8)[0]
    np.testing.assert_array_equal(gpu.read_rng(), rng)
    np.testing.assert_array_equal(gpu.read_accum().view(np.uint32), o_acc.view(np.uint32))
    # min_spp == max_spp == batch is allowed (one round); then the read-outs and their capacities
    info = gpu.render_adaptive(cam, 4, 4, 4, 0.1, depth)
    assert info["rounds"] == 1 and info["passes_done"] == W * H * 4
    assert np.isinf(gpu.read_noise()).all()             # one batch mean: no estimate yet
    small = np.zeros(W * H - 1, dtype=np.float32)
    assert L.cpt_read_noise(gpu._ctx, ctypes.c_void_p(small.ctypes.data), small.size) == INVALID
    gpu.set_frame(W, H)
    with pytest.raises(CptError) as e:
        gpu.read_noise()                                # released with the frame
    assert e.value.status == STATE
