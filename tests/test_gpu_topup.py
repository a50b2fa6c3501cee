"""cpt_render_to_count on the GPU: every pixel topped up to a pass count, held bit
for bit to tests/topup_model.py (per-deficit oracle renders) in the accumulator, the RNG planes and,
with CPT_RENDER_AUX, the normals and depths; the plan's order and totals against the model's; what
the call must leave alone, its error codes and its place in the stream's order; and the point of it:
after a reprojection the same budget lowers the error of the disoccluded pixels more than a uniform
accumulating render does.
"""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import reproject_model as rm
import test_gpu_async_order as ao
import test_gpu_parity as tp
import topup_model as tu
import tracked_reproject_model as tm

from cpppathtracer_amd import CptError, Renderer, camera_get_copy, scenes
from cpppathtracer_amd._lib import (CPT_ERR_INVALID_ARG, CPT_ERR_STATE, CPT_ERR_UNSUPPORTED, CPT_PATH_WAVEFRONT,
                                    CPT_RENDER_ACCUMULATE, CPT_SCHEDULE_CONSOLIDATE, CPT_SCHEDULE_COST, CPT_SCHEDULE_PREVIOUS,
                                    CPT_TILE_ORDER_TOPUP, CPT_TRAVERSAL_ORDERED, CPT_TRAVERSAL_PLAIN_LEAVES)
from cpppathtracer_amd.tiling import tile_grid

pytestmark = pytest.mark.gpu

WALKS = {"reference": 0, "plain": CPT_TRAVERSAL_ORDERED | CPT_TRAVERSAL_PLAIN_LEAVES, "wide": CPT_TRAVERSAL_ORDERED}
DEPTH, TARGET, SEED = 8, 16, scenes.DEFAULT_SEED
shared = ao.shared   # the ordering test's workload (a module fixture of test_gpu_async_order.py)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


SCENES = {"s4cyl": tm.scene, "s1000": scenes.scene_s1000, "hyb": lambda: scenes.scene_s1000(n=3000), "chain": tp._chain_scene}
PLANES = {"checkerboard": lambda W, n, t: tu.checkerboard(W, n, t), "drawn": lambda W, n, t: tu.drawn_counts(W, n, t),
          "done": lambda W, n, t: np.resize(np.array([t, t + 1, 2.0 ** 24, np.inf, np.nan, -1, -np.inf, t + 0.5], dtype=np.float32), W * n)}
_cache = {}


def _case(oracle_mod, sky, scene, W, H, plane, target=TARGET, depth=DEPTH, rows=None):
    """The starting state and the model's expected frame of one case, computed once: NaN-filled
    normals and depths of 7, so a pixel the call must not write shows a write of any value."""
    key = (scene, W, H, plane, target, depth, None if rows is None else tuple(rows))
    if key not in _cache:
        r = np.arange(H, dtype=np.int32) if rows is None else np.asarray(rows, dtype=np.int32)
        npix = r.size * W
        objs = SCENES[scene]()
        cam = camera_get_copy(scenes.camera_for(W, H))
        rng0 = oracle_mod.init_rng(SEED, W, r, threads=8)
        acc0 = tu.with_counts(np.zeros((npix, 4), np.float32), PLANES[plane](W, r.size, target))
        normal0, depth0 = np.full((npix, 3), np.nan, np.float32), np.full(npix, 7.0, np.float32)
        acc, rng, normal, dep, p = tu.expected(oracle_mod, objs, cam, sky, r, depth, target, rng0, acc0, normal0, depth0)
        assert len(p["values"]) <= 6
        _cache[key] = SimpleNamespace(objs=objs, cam=cam, rows=rows, W=W, H=H, target=target, depth=depth, rng0=rng0, acc0=acc0,
                                      normal0=normal0, depth0=depth0, accum=acc, rng=rng, normal=normal, dep=dep, plan=p)
    return _cache[key]


def _start(gpu, sky, c, aux=True):
    gpu.set_scene(c.objs)
    gpu.set_env(sky)
    gpu.set_frame(c.W, c.H, c.rows)
    gpu.init_rng(SEED)
    np.testing.assert_array_equal(gpu.read_rng(), c.rng0)
    gpu.write_accum(c.acc0)
    if aux:
        gpu.write_aux(c.normal0, c.depth0)


def _assert_frame(gpu, c, aux=True, what=""):
    np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(c.accum), err_msg=what + " accumulator")
    np.testing.assert_array_equal(gpu.read_rng(), c.rng, err_msg=what + " RNG planes")
    if aux:
        n, d = gpu.read_aux()
        np.testing.assert_array_equal(_bits(n), _bits(c.normal), err_msg=what + " normals")
        np.testing.assert_array_equal(_bits(d), _bits(c.dep), err_msg=what + " depths")
    info = gpu.topup_info()
    assert info == {k: c.plan[k] for k in ("tiles", "pixels", "passes")}, what
    np.testing.assert_array_equal(gpu.debug_tile_order(CPT_TILE_ORDER_TOPUP), c.plan["order"], err_msg=what + " order")


def _run(gpu, oracle_mod, sky, scene, W, H, plane, walk, aux=True, **kw):
    c = _case(oracle_mod, sky, scene, W, H, plane, **kw)
    _start(gpu, sky, c, aux)
    gpu.render_to_count(c.cam, c.target, c.depth, aux=aux, sync=True, flags=WALKS[walk])
    _assert_frame(gpu, c, aux, f"{scene} {W}x{H} {plane} {walk}")
    return c


# ------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("plane", ["checkerboard", "drawn"])
@pytest.mark.parametrize("wh", [(64, 48), (67, 41)], ids=lambda wh: "%dx%d" % wh)
def test_topup_equals_the_model(gpu, oracle_mod, sky, wh, plane, walk):
    """A checkerboard of tiles at 0 and at the target, and per-pixel counts drawn from {0, 1, 5,
    12, target, target + 3}, under the three walks, with aux: accumulator, RNG planes, normals,
    depths, the plan's totals and its order."""
    c = _run(gpu, oracle_mod, sky, "s4cyl", *wh, plane, walk)
    done = c.plan["d"] == 0
    assert done.any() and not done.all()
    n, _ = gpu.read_aux()
    assert np.isnan(n[done]).all() and not np.isnan(n[~done]).any()   # untouched / written


def test_topup_without_aux(gpu, oracle_mod, sky):
    _run(gpu, oracle_mod, sky, "s4cyl", 67, 41, "drawn", "wide", aux=False)


@pytest.mark.parametrize("walk", ["reference", "wide"])
def test_topup_s1000(gpu, oracle_mod, sky, walk):
    _run(gpu, oracle_mod, sky, "s1000", 64, 36, "drawn", walk, target=8)
    assert 0 < gpu.walk_info()["n_wide"] <= tp.LDS_TREE_NODES


def test_topup_beyond_the_lds_image(gpu, oracle_mod, sky):
    """The HYB kernels (a 4-wide tree larger than the LDS image)."""
    _run(gpu, oracle_mod, sky, "hyb", 64, 36, "drawn", "wide", target=8)
    assert gpu.walk_info()["n_wide"] > tp.LDS_TREE_NODES


def test_topup_binary_fallback(gpu, oracle_mod, sky):
    """A tree too deep for the 4-wide walk: the kernels of 256 lanes under the ordered flag."""
    _run(gpu, oracle_mod, sky, "chain", 48, 32, "drawn", "wide", target=8)
    assert gpu.walk_info()["n_wide"] == 0


@pytest.mark.parametrize("grid", [(1, 64), (2, 64), (1, 4)], ids=lambda g: "%dwg_%dlanes" % g)
@pytest.mark.parametrize("walk", ["reference", "wide"])
def test_topup_capped_grid(gpu, oracle_mod, sky, walk, grid):
    """cpt_set_debug_grid at 1 and 2 workgroups and at 4 taking lanes per wave: lanes refill, and
    chains of different lengths share a wave (64 x 48: 3072 pixels on at most 2048 lanes)."""
    assert 64 * 48 > grid[0] * 16 * grid[1]
    gpu.set_debug_grid(*grid)
    try:
        _run(gpu, oracle_mod, sky, "s4cyl", 64, 48, "drawn", walk)
    finally:
        gpu.set_debug_grid(0, 0)


def test_topup_on_a_row_tiled_context(gpu, oracle_mod, sky):
    rows = [5, 2, 40, 41, 42, 43, 44, 45, 46, 47, 0]
    _run(gpu, oracle_mod, sky, "s4cyl", 64, 48, "drawn", "wide", rows=rows)


@pytest.mark.parametrize("walk", ["reference", "wide"])
def test_nothing_owed_nothing_written(gpu, oracle_mod, sky, walk):
    """Every count at or past the target, or no count at all (NaN, inf, negative): topup_info
    gives zeros and the accumulator, the RNG planes and the NaN-filled normals keep their bits."""
    c = _run(gpu, oracle_mod, sky, "s4cyl", 67, 41, "done", walk)
    assert c.plan["tiles"] == 0 and gpu.topup_info() == {"tiles": 0, "pixels": 0, "passes": 0}
    np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(c.acc0))
    np.testing.assert_array_equal(gpu.read_rng(), c.rng0)
    n, d = gpu.read_aux()
    assert np.isnan(n).all() and (d == 7.0).all()
    assert gpu.debug_tile_order(CPT_TILE_ORDER_TOPUP).size == 0


@pytest.mark.parametrize("wh", [(1, 1), (16, 16)], ids=lambda wh: "%dx%d" % wh)
def test_all_counts_zero_is_a_plain_render(gpu, sky, wh):
    W, H = wh
    cam = camera_get_copy(scenes.camera_for(W, H))
    gpu.set_scene(tm.scene())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED)
    gpu.render(cam, TARGET, DEPTH, aux=True, sync=True, ordered=True)
    want = gpu.read_accum(), gpu.read_rng(), *gpu.read_aux()
    gpu.init_rng(SEED)
    gpu.clear_accum()
    gpu.render_to_count(cam, TARGET, DEPTH, aux=True, sync=True, flags=CPT_TRAVERSAL_ORDERED | CPT_RENDER_ACCUMULATE)
    got = gpu.read_accum(), gpu.read_rng(), *gpu.read_aux()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert gpu.topup_info() == {"tiles": math.prod(tile_grid(W, H)), "pixels": W * H, "passes": W * H * TARGET}


def test_reprojected_accumulator(gpu, oracle_mod, sky):
    """A real reprojected accumulator from the sideways camera pair (4 passes of history, so at most
    five distinct deficits to a target of 8)."""
    W, H, target = 64, 48, 8
    c0, c1 = (camera_get_copy(c) for c in rm.camera_pairs(W, H)["sideways"])
    objs = tm.scene()
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED)
    gpu.render(c0, 4, DEPTH, sync=True, ordered=True)
    gpu.reproject_accum(c0, c1, max_history=4, flags=CPT_TRAVERSAL_ORDERED)
    acc0, rng0 = gpu.read_accum(), gpu.read_rng()
    assert 0.05 <= (acc0[:, 3] == 0).mean() and 0.25 <= (acc0[:, 3] == 4).mean()
    acc, rng, _, _, p = tu.expected(oracle_mod, objs, c1, sky, np.arange(H), DEPTH, target, rng0, acc0)
    assert len(p["values"]) <= 5
    gpu.render_to_count(c1, target, DEPTH, sync=True, flags=CPT_TRAVERSAL_ORDERED)
    np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(acc))
    np.testing.assert_array_equal(gpu.read_rng(), rng)
    assert gpu.topup_info() == {k: p[k] for k in ("tiles", "pixels", "passes")}
    assert (gpu.read_accum()[:, 3] >= target).all()


# ---------------------------------------------------------------------------------- the plan
def test_plan_order_and_totals_at_153_tiles(gpu, sky):
    """136 x 72 (153 tiles, more than one wave of tiles): the plan's active prefix equals the
    model's stable order, topup_info its totals; with CPT_RENDER_STATS at depth 1 (one segment per
    pass) the stats' segment count is the sum of the deficits."""
    W, H, target = 136, 72, 12
    counts = tu.graded_counts(W, H, target)   # several keys, many ties, tile columns without a deficit
    p = tu.plan(counts, W, H, target)
    assert math.prod(tile_grid(W, H)) == 153 and 64 < p["tiles"] < 153 and len(set(p["keys"].tolist())) >= 4
    cam = camera_get_copy(scenes.camera_for(W, H))
    gpu.set_scene(scenes.scene_s4())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED)
    gpu.write_accum(tu.with_counts(np.zeros((W * H, 4), np.float32), counts))
    gpu.reset_stats()
    gpu.render_to_count(cam, target, 1, stats=True, flags=CPT_TRAVERSAL_ORDERED)
    np.testing.assert_array_equal(gpu.debug_tile_order(CPT_TILE_ORDER_TOPUP), p["order"])
    assert gpu.topup_info() == {k: p[k] for k in ("tiles", "pixels", "passes")}
    st = gpu.stats()
    assert st["segments"] == p["passes"] == st["hits"] + st["misses"]
    got = gpu.read_accum()[:, 3]
    np.testing.assert_array_equal(got, np.where(p["d"] > 0, np.float32(target), counts))


# ------------------------------------------------------------------------------------ errors
def _raises(status, call):
    with pytest.raises(CptError) as e:
        call()
    assert e.value.status == status, e.value


def test_errors_write_nothing(gpu, sky):
    W, H = 64, 48
    cam = camera_get_copy(scenes.camera_for(W, H))
    small = camera_get_copy(scenes.camera_for(16, 16))
    acc0 = tu.with_counts(np.zeros((W * H, 4), np.float32), tu.drawn_counts(W, H, TARGET))
    r = Renderer(0)
    try:
        _raises(CPT_ERR_STATE, lambda: r.render_to_count(cam, TARGET, DEPTH))   # no scene
        _raises(CPT_ERR_STATE, r.topup_info)
        r.set_scene(scenes.scene_s4())
        _raises(CPT_ERR_STATE, lambda: r.render_to_count(cam, TARGET, DEPTH))   # no frame
        r.set_frame(W, H)
        r.write_accum(acc0)
        _raises(CPT_ERR_STATE, lambda: r.render_to_count(cam, TARGET, DEPTH))   # no RNG states
        _raises(CPT_ERR_STATE, r.topup_info)
        _raises(CPT_ERR_STATE, lambda: r.debug_tile_order(CPT_TILE_ORDER_TOPUP))
        np.testing.assert_array_equal(_bits(r.read_accum()), _bits(acc0))
    finally:
        r.close()

    gpu.set_scene(scenes.scene_s4())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED)
    gpu.write_accum(acc0)
    rng0 = gpu.read_rng()
    L, ctx = gpu._L, gpu._ctx
    pc = ctypes.c_void_p(np.ascontiguousarray(cam).ctypes.data)
    assert L.cpt_render_to_count(None, pc, TARGET, DEPTH, 0) == CPT_ERR_INVALID_ARG
    cases = [(CPT_ERR_INVALID_ARG, lambda: gpu._check(L.cpt_render_to_count(ctx, None, TARGET, DEPTH, 0)))]
    cases += [(CPT_ERR_INVALID_ARG, lambda t=t: gpu.render_to_count(cam, t, DEPTH)) for t in (0, -1, (1 << 20) + 1)]
    cases += [(CPT_ERR_INVALID_ARG, lambda d=d: gpu.render_to_count(cam, TARGET, d)) for d in (-1, 33)]
    cases += [(CPT_ERR_INVALID_ARG, lambda: gpu.render_to_count(small, TARGET, DEPTH))]
    cases += [(CPT_ERR_UNSUPPORTED, lambda f=f: gpu.render_to_count(cam, TARGET, DEPTH, flags=f | CPT_TRAVERSAL_ORDERED))
              for f in (CPT_PATH_WAVEFRONT, CPT_SCHEDULE_PREVIOUS, CPT_SCHEDULE_COST, CPT_SCHEDULE_CONSOLIDATE)]
    for status, call in cases:
        _raises(status, call)
        np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(acc0))
        np.testing.assert_array_equal(gpu.read_rng(), rng0)
    _raises(CPT_ERR_STATE, gpu.topup_info)   # none of the failed calls planned anything
    # an adaptive render pending
    gpu.adaptive_begin(cam, 4, 8, 2, 0.0, 4, flags=CPT_TRAVERSAL_ORDERED | CPT_RENDER_ACCUMULATE)
    _raises(CPT_ERR_STATE, lambda: gpu.render_to_count(cam, TARGET, DEPTH))
    while gpu.adaptive_step():
        pass
    gpu.render_to_count(cam, 1 << 20, 0, sync=True)   # the largest target, at depth 0: RayGen's draws alone
    assert (gpu.read_accum()[:, 3] >= 1 << 20).all()
    info = gpu.topup_info()
    assert info["pixels"] == W * H and info["tiles"] == 48
    # topup_info's outputs may each be NULL; a new frame forgets the plan
    gpu._check(L.cpt_topup_info(ctx, None, None, None))
    gpu.set_frame(W, H)
    _raises(CPT_ERR_STATE, gpu.topup_info)


def test_topup_leaves_the_rest_of_the_frame_alone(gpu, sky):
    """Like a plain render: the adaptive result's moments, the display state, the G-buffer and the
    captured reprojection history stay as they were."""
    W, H = 64, 48
    cam = camera_get_copy(scenes.camera_for(W, H))
    gpu.set_scene(tm.scene())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED)
    gpu.render_adaptive(cam, 4, 8, 2, 0.1, DEPTH, flags=CPT_TRAVERSAL_ORDERED | 0x2)
    gpu.denoise_mix_history()
    gpu.history_capture(cam, CPT_TRAVERSAL_ORDERED)

    def state():
        g = gpu.read_gbuffer()
        return [gpu.read_moments(), gpu.read_mix(), gpu.read_display_count(), g["id"], g["t"], g["normal"], g["albedo"]]
    before, acc = state(), gpu.read_accum()
    gpu.render_to_count(cam, 12, DEPTH, sync=True, flags=CPT_TRAVERSAL_ORDERED)
    for a, b in zip(before, state()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert gpu.history_info()[0]
    assert (gpu.read_accum()[:, 3] == 12).all() and (acc[:, 3] < 12).all()


# ---------------------------------------------------------------------------------- ordering
def _topup_then_read(r, e):
    r.render_to_count(e.cam, ao.SPP + 64, ao.DEPTH, flags=ao.WALK)
    return r.read_accum()   # unsynchronised: the read orders itself behind the top-up


ORDER_CASE = ao.Case("render_to_count-read", _topup_then_read, ao.IMAGE, rerecords=True)


def test_topup_behind_a_render_in_flight(shared):
    """cpt_render_to_count queued behind an unsynchronised cpt_render, and an unsynchronised read
    behind it, give the bytes of the sequence synchronised after every call."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    want, _, first = ao._run(ORDER_CASE, shared, twin=True)
    got, (t_launch, t_call, _), _ = ao._run(ORDER_CASE, shared, twin=False)
    ao.assert_overlap(ORDER_CASE.name, t_launch, t_call, first[2])
    ao._assert_same_bits(got, want)
    assert (want["accum"].view(np.float32).reshape(-1, 4)[:, 3] == ao.SPP + 64).all()


# ----------------------------------------------------------------------------------- C++ API
def test_headless_orbit_fill_equals_the_python_sequence(gpu, sky, tmp_path):
    """cpt_headless --orbit 3 --reproject --fill 16 (PathTracer::Reproject, then RenderToCount, between
    the frames of a small orbit) writes the PFM the same calls give through the Python wrapper."""
    import subprocess

    from cpppathtracer_amd import build
    from test_gpu_reproject import orbit_cameras
    W, H, SPP, N, FILL = 48, 32, 2, 3, 16
    out = tmp_path / "orbit.pfm"
    r = subprocess.run([build.build_examples(), "--scene", "s4", "--width", str(W), "--height", str(H), "--spp", str(SPP),
                        "--depth", "4", "--seed", str(SEED), "--orbit", str(N), "--reproject", "--fill", str(FILL), "--pfm", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF"
        assert tuple(int(v) for v in f.readline().split()) == (W, H)
        assert float(f.readline()) < 0
        pfm = np.frombuffer(f.read(), dtype="<f4").reshape(H, W, 3)[::-1].reshape(-1, 3)
    cams = orbit_cameras(W, H, N)
    gpu.set_scene(scenes.scene_s4())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED)
    spent = 0
    for k, cam in enumerate(cams):
        if k == 0:
            gpu.render(cam, SPP, 4, aux=True, sync=True, ordered=True)
            continue
        gpu.reproject_accum(cams[k - 1], cam, flags=CPT_TRAVERSAL_ORDERED)
        gpu.render_to_count(cam, FILL, 4, aux=True, sync=True, flags=CPT_TRAVERSAL_ORDERED)
        spent += gpu.topup_info()["passes"]
    acc = gpu.read_accum()
    assert (acc[:, 3] >= FILL).all() and 0 < spent < 2 * FILL * W * H   # the second fill found history to keep
    want = (acc[:, :3] / acc[:, 3:4]).astype(np.float32)
    np.testing.assert_array_equal(_bits(pfm), _bits(want))
    bad = subprocess.run([build.build_examples(), "--scene", "s4", "--fill", "8"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--fill" in bad.stderr


# -------------------------------------------------------------------------------- end to end
E2E_STEP = (8.0, 0.0, -8.0)   # the camera's sideways step (origin and look-at point), world units


def e2e_cameras(W, H):
    """The scenes' camera as the reference's MotionalCamera makes it (lens_radius 0.0005, as
    test_gpu_reproject.py's pair) and the same camera a step to the side.  On the CPU (the G-buffer
    model and cpt_reproject_host) this step leaves 7.3% of the 64 x 48 frame at count 0 and reuses
    92.7% at 32 passes; a step of 4 leaves 3.2%, one of 12 11.6% (tools/topup_ab.py --rehearsal)."""
    from cpppathtracer_amd.scenes import CAMERA_LOOK_AT as AT, CAMERA_ORIGIN as O
    from cpppathtracer_amd.types import make_camera
    move = lambda p: tuple(a + b for a, b in zip(p, E2E_STEP))
    return (camera_get_copy(make_camera(W, H, origin=O, look_at=AT)),
            camera_get_copy(make_camera(W, H, origin=move(O), look_at=move(AT))))


@pytest.fixture(scope="module")
def e2e(gpu, sky):
    """S4 + cylinder, 64x48, depth 8, 32 passes, reprojected to a sideways camera.  Arm A:
    render_to_count(32), B passes.  Arm B: from the same RNG states, ceil(B / npix) passes for
    every pixel.  Truth: 1024 passes at the new camera."""
    W, H = 64, 48
    c0, c1 = e2e_cameras(W, H)
    kw = dict(ordered=True)
    gpu.set_scene(tm.scene())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED + 1)
    gpu.render(c1, 1024, DEPTH, sync=True, **kw)
    truth = gpu.read_accum()
    truth = truth[:, :3].astype(np.float64) / truth[:, 3:4]
    gpu.init_rng(SEED)
    gpu.render(c0, 32, DEPTH, sync=True, **kw)
    gpu.reproject_accum(c0, c1, flags=CPT_TRAVERSAL_ORDERED)
    states, hist = gpu.read_rng(), gpu.read_accum()
    gpu.render_to_count(c1, 32, DEPTH, sync=True, flags=CPT_TRAVERSAL_ORDERED)
    topped, budget = gpu.read_accum(), gpu.topup_info()["passes"]
    uniform_spp = -(-budget // (W * H))
    gpu.write_rng(states)
    gpu.write_accum(hist)
    gpu.render(c1, uniform_spp, DEPTH, accumulate=True, sync=True, **kw)
    uniform = gpu.read_accum()

    def err(accum):
        mean = accum[:, :3] / accum[:, 3:4]
        return ((mean.astype(np.float64) - truth) ** 2).mean(axis=1)
    a, b = err(topped), err(uniform)
    empty, reused = hist[:, 3] == 0, hist[:, 3] == 32
    print(f"top-up: {budget} passes; uniform: {uniform_spp} per pixel = {uniform_spp * W * H} passes; "
          f"{empty.mean():.4f} of the frame at count 0, {reused.mean():.4f} reused at 32")
    print(f"count-0 pixels: top-up MSE {a[empty].mean():.6g}, uniform MSE {b[empty].mean():.6g}")
    print(f"frame: top-up MSE {a.mean():.6g}, uniform MSE {b.mean():.6g}")
    return SimpleNamespace(a=a, b=b, empty=empty, reused=reused, budget=budget, uniform_spp=uniform_spp, npix=W * H,
                           topped=topped)


def test_topup_beats_uniform_on_disocclusions(e2e):
    """At least 5% of the pixels start at count 0 and at least 50% are reused; the uniform arm's
    budget is never below the top-up's; over the pixels the reprojection left at count 0 the
    top-up's MSE to the truth is below the uniform render's: 0.000321612 against 0.00298287 in the CPU
    rehearsal (tools/topup_ab.py --rehearsal --steps 8).  The rehearsal also has the frame-wide MSE
    at 0.00107365 against 0.00114809 for this pair, so that is asserted too."""
    e = e2e
    assert e.empty.mean() >= 0.05 and e.reused.mean() >= 0.5
    assert e.uniform_spp * e.npix >= e.budget > 0
    assert (e.topped[:, 3] >= 32).all()
    assert e.a[e.empty].mean() < e.b[e.empty].mean()
    assert e.a.mean() <= e.b.mean()
