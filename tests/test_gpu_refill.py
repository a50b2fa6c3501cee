"""The megakernel's lane refill, held to the oracle bit for bit on frames the scalar oracle affords.

launch_mk sizes the persistent grid to min(ceil(tiles * 64 / block), resident workgroups), so on
the other GPU test files' frames (at most 96 x 54) every lane takes at most one pixel: a lane's
second take, the batched draw's bookkeeping across rounds, ids outside the frame, the long chains'
taper, the static first take's offset, the pilot's per-pixel subtraction and a consolidating
keeper that takes hand-overs and fresh pixels in one render never run there.  Here
Renderer.set_debug_grid (TEST HOOK cpt_set_debug_grid) caps the grid at 1 or 2 workgroups, or lets
only 4 lanes of a wave take pixels, and the same scenes, corpora and assertions run again: the
other files' test functions themselves where the frame they use is large enough, the same helpers
on a larger frame where it is not.

Every test states its precondition through `capped`: with `lanes` = max_workgroups x 16 waves x
lanes_per_wave (the LDS walk's workgroup; the kernels without the LDS image have 4 waves, a
quarter of that),
  * strict:  tiles x 64 >= 2 x lanes, and more pixels than lanes;
  * strict=False, the frames the plan lists at fewer than two ids per lane (40 x 40 and 48 x 32 at
    1 workgroup, the frames of 2048 .. 4095 ids at 2): more pixels than lanes, which is what
    forces some lane to take a second pixel (pigeonhole).
"""
import math
from contextlib import contextmanager

import numpy as np
import pytest
import scene_fuzz as sf
import test_gpu_edit_fuzz as te
import test_gpu_fuzz_parity as fz
import test_gpu_parity as tp
from test_gpu_parity import _check_stats, _kw, _run_both

from cpppathtracer_amd import CptError, camera_get_copy, scenes
from cpppathtracer_amd.tiling import tile_grid

pytestmark = pytest.mark.gpu

MK5 = ["megakernel", "megakernel:ordered", "megakernel:plain", "megakernel:ordered+timed",
       "megakernel:ordered+timed+cons"]
MK7 = MK5 + ["megakernel+timed", "megakernel:ordered+cons"]
assert set(MK7) <= set(tp.PATHS)


@contextmanager
def capped(gpu, W, n_rows, max_workgroups, lanes_per_wave=64, strict=True):
    """set_debug_grid(max_workgroups, lanes_per_wave) for the block, reset to 0, 0 after it (the
    `gpu` fixture is session-wide), and the precondition that a render of a W x n_rows frame under
    it cannot finish without a lane taking a second pixel."""
    lanes = max_workgroups * 16 * lanes_per_wave
    ids = math.prod(tile_grid(W, n_rows)) * 64
    assert W * n_rows > lanes, (W, n_rows, lanes)
    if strict:
        assert ids >= 2 * lanes, (ids, lanes)
    gpu.set_debug_grid(max_workgroups, lanes_per_wave)
    try:
        yield
    finally:
        gpu.set_debug_grid(0, 0)


def _bitexact(gpu, oracle_mod, sky, objs, W, H, spp, depth, path, **kw):
    """test_gpu_parity.py::test_render_bitexact's assertions (NaN-free demo scenes)."""
    (ga, gr, gs, gx), (oa, orng, os_, ox) = _run_both(gpu, oracle_mod, sky, objs, W, H, spp, depth, path=path, **kw)
    np.testing.assert_array_equal(gr, orng)
    _check_stats(gs, os_, path)
    np.testing.assert_array_equal(ga.view(np.uint32), oa.view(np.uint32))
    assert np.isfinite(ga).all() and (ga[:, 3] == spp).all()
    return gx, ox


# ------------------------------------------------------------------------------ the hook
def test_hook_arguments(gpu):
    for bad in ((-1, 0), (0, -1), (0, 65), (-3, 65)):
        with pytest.raises(CptError) as e:
            gpu.set_debug_grid(*bad)
        assert e.value.status == 1   # CPT_ERR_INVALID_ARG
    gpu.set_debug_grid(3, 64)
    gpu.set_debug_grid(1, 1)
    gpu.set_debug_grid()


# ----------------------------------------------------- (a) full-width waves, 1 and 2 workgroups
def _wgs(W, H):
    """(max_workgroups, strict) a W x H frame runs at: 1 and 2; 2 only with more pixels than 2048
    lanes; strict where it has two ids per lane."""
    ids = math.prod(tile_grid(W, H)) * 64
    return [(wg, ids >= 2048 * wg) for wg in (1, 2) if W * H > 1024 * wg]


def test_frames_of_the_demo_cases_run_where_planned():
    got = {(W, H): _wgs(W, H) for _, W, H, _, _ in tp.CASES}
    assert got == {(64, 64): [(1, True), (2, True)], (67, 33): [(1, True), (2, False)],
                   (64, 48): [(1, True), (2, False)], (40, 40): [(1, False)],
                   (64, 36): [(1, True), (2, False)], (96, 54): [(1, True), (2, True)]}
    assert 67 * 33 < 9 * 5 * 64   # the frame whose ids fall outside the image


@pytest.mark.parametrize("path", MK7)
@pytest.mark.parametrize("name,W,H,spp,depth,wg,strict",
                         [c + w for c in tp.CASES for w in _wgs(c[1], c[2])])
def test_render_bitexact_capped(gpu, oracle_mod, sky, name, W, H, spp, depth, wg, strict, path):
    with capped(gpu, W, H, wg, strict=strict):
        _bitexact(gpu, oracle_mod, sky, scenes.SCENES[name](), W, H, spp, depth, path)


@pytest.mark.parametrize("path", MK5)
@pytest.mark.parametrize("wg,strict", _wgs(64, 40))
def test_exact_ties_capped(gpu, oracle_mod, sky, wg, strict, path):
    with capped(gpu, 64, 40, wg, strict=strict):
        tp.test_exact_ties_between_primitives(gpu, oracle_mod, sky, path)


@pytest.mark.parametrize("path", MK5)
@pytest.mark.parametrize("wg,strict", _wgs(64, 40))
def test_mixed_large_capped(gpu, oracle_mod, sky, wg, strict, path):
    """Zero direction components in the 4-wide walk, in lanes on their second and third pixel."""
    (seed,) = sf.MIXED_LARGE_SEEDS
    cam = sf.mixed_large(seed)[1]
    assert (int(cam["width"]), int(cam["height"])) == (64, 40)
    with capped(gpu, 64, 40, wg, strict=strict):
        fz.test_mixed_large_wide_walk_axis_aligned(gpu, oracle_mod, sky, seed, path)


@pytest.mark.parametrize("path", ["megakernel:ordered", "megakernel:ordered+timed", "megakernel:ordered+timed+cons"])
@pytest.mark.parametrize("wg,strict", _wgs(64, 36))
def test_wide_walk_beyond_lds_image_capped(gpu, oracle_mod, sky, wg, strict, path):
    """The HYB kernel refilling (3000 primitives, 64 x 36), with its proof that wide nodes were
    read from global memory."""
    with capped(gpu, 64, 36, wg, strict=strict):
        tp.test_wide_walk_beyond_lds_image(gpu, oracle_mod, sky, path)


@pytest.mark.parametrize("path", MK5)
def test_deep_tree_fallback_capped(gpu, oracle_mod, sky, path):
    """The binary-walk fallback (no 4-wide tree: the kernels of 256 lanes), 48 x 32, 1 workgroup."""
    objs = tp._chain_scene()
    gpu.set_scene(objs)
    assert gpu.walk_info()["n_wide"] == 0
    with capped(gpu, 48, 32, 1, strict=False):
        _bitexact(gpu, oracle_mod, sky, objs, 48, 32, 2, 8, path)


@pytest.mark.parametrize("path", MK5)
@pytest.mark.parametrize("wg,strict", _wgs(64, 40))
def test_update_object_refit_capped(gpu, oracle_mod, sky, wg, strict, path):
    with capped(gpu, 64, 40, wg, strict=strict):
        tp._update_object_refit(gpu, oracle_mod, sky, path, 64, 40)


@pytest.mark.parametrize("path", MK5)
@pytest.mark.parametrize("wg,strict", _wgs(64, 40))
def test_render_aux_capped(gpu, oracle_mod, sky, wg, strict, path):
    """The first-hit normal of a lane's second pixel (its reset on a take), and the normal's slot
    in a hand-over under "+cons"."""
    with capped(gpu, 64, 40, wg, strict=strict):
        (gn, gd), (on, od) = _bitexact(gpu, oracle_mod, sky, scenes.scene_s4(), 64, 40, 2, 8, path, aux=True)
    np.testing.assert_array_equal(gn.view(np.uint32), on.view(np.uint32))
    np.testing.assert_array_equal(gd, od)
    assert (gd == np.float32(1e30)).all()


LONG = dict(W=72, H=40, spp=64, depth=8, seed=77)


@pytest.mark.parametrize("path", ["megakernel:ordered", "megakernel:ordered+cons", "megakernel:ordered+timed",
                                  "megakernel:ordered+timed+cons"])
@pytest.mark.parametrize("wg,strict", _wgs(72, 40))
def test_long_chains_capped(gpu, oracle_mod, sky, wg, strict, path):
    """64 passes per pixel, 2880 ids on 1024 / 2048 lanes (2.8 / 1.4 pixels per lane): the taper
    (spp >= 64: the counter re-read, the shrinking range) with the grid's lanes below the ids; with
    the cost schedule ("+timed") the static first take and the offset of every later take; with
    "+cons" keepers that take hand-overs and fresh pixels in one render.  The schedules: "tiles"
    and "cost", each with and without consolidation."""
    W, H = LONG["W"], LONG["H"]
    assert math.prod(tile_grid(W, H)) * 64 == 2880 > 1024 * wg
    kw = _kw(path)
    assert kw["ordered"] is True and kw.get("schedule", "tiles") == ("cost" if "timed" in path else "tiles")
    assert bool(kw.get("consolidate")) == ("cons" in path)
    objs = scenes.scene_s1000(n=200)
    gpu.set_scene(objs)
    assert gpu.walk_info()["n_wide"] > 0   # the LDS kernels: consolidation and the static first take
    with capped(gpu, W, H, wg, strict=strict):
        _bitexact(gpu, oracle_mod, sky, objs, W, H, LONG["spp"], LONG["depth"], path, seed=LONG["seed"])


@pytest.mark.parametrize("ordered", [True, False])
def test_previous_pass_schedule_capped(gpu, oracle_mod, sky, ordered):
    with capped(gpu, 72, 40, 1):
        tp.test_previous_pass_schedule(gpu, oracle_mod, sky, ordered)


# ------------------------------------------------- (b) narrow waves on the small fuzz corpus
def _narrow(gpu, cam):
    """set_debug_grid(1, 4): 64 pixel slots at most (16 with the kernels of 256 lanes)."""
    return capped(gpu, int(cam["width"]), int(cam["height"]), 1, 4)


@pytest.mark.parametrize("path", MK5)
@pytest.mark.parametrize("seed", sf.MIXED_SEEDS)
def test_mixed_narrow(gpu, oracle_mod, sky, seed, path):
    with _narrow(gpu, sf.mixed(seed)[1]):
        fz.test_mixed(gpu, oracle_mod, sky, seed, path)


@pytest.mark.parametrize("path", MK5)
@pytest.mark.parametrize("seed", sf.AXIS_SEEDS)
def test_axis_aligned_narrow(gpu, oracle_mod, sky, seed, path):
    with _narrow(gpu, sf.axis_aligned(seed)[1]):
        fz.test_axis_aligned(gpu, oracle_mod, sky, seed, path)


@pytest.mark.parametrize("path", MK5)
@pytest.mark.parametrize("seed", sf.INSIDE_SEEDS)
def test_inside_narrow(gpu, oracle_mod, sky, seed, path):
    with _narrow(gpu, sf.inside(seed)[1]):
        fz.test_inside(gpu, oracle_mod, sky, seed, path)


@pytest.mark.parametrize("path", MK5)
@pytest.mark.parametrize("name", list(fz.EDGE_MATERIALS))
def test_edge_materials_narrow(gpu, oracle_mod, sky, name, path):
    with _narrow(gpu, fz.EDGE_MATERIALS[name][1]):
        fz.test_edge_materials(gpu, oracle_mod, sky, name, path)


@pytest.mark.parametrize("path", MK5)
@pytest.mark.parametrize("name", list(fz.EDGE_GEOMETRY))
def test_edge_geometry_narrow(gpu, oracle_mod, sky, name, path):
    with _narrow(gpu, fz.EDGE_GEOMETRY[name][1]):
        fz.test_edge_geometry(gpu, oracle_mod, sky, name, path)


@pytest.mark.parametrize("path", ["megakernel", "megakernel:ordered"])
@pytest.mark.parametrize("name", list(fz.DEGENERATE))
def test_degenerate_camera_narrow(gpu, oracle_mod, sky, name, path):
    """Every primary ray non-finite (the FAST = false walk), 16 x 8: with its segment count."""
    with _narrow(gpu, fz.DEGENERATE[name][1]):
        fz.test_degenerate_camera(gpu, oracle_mod, sky, name, path)


@pytest.mark.parametrize("path", ["megakernel:ordered", "megakernel:ordered+timed+cons"])
@pytest.mark.parametrize("name", te.NAMES)
def test_edit_sequences_narrow(gpu, oracle_mod, sky, name, path):
    """test_gpu_edit_fuzz.py's frame-by-frame comparison against oracle.render_edited."""
    with _narrow(gpu, te.SEQ[name][2]):
        te.test_sequence_parity(gpu, oracle_mod, sky, name, path)


# ------------------------------------------------------ (c) the pilot's per-pixel subtraction
# The PROBE kernel's cost of a pixel is the lane's running counters minus their value when the
# lane took the pixel (work_at_take): zero for a lane's first pixel, so only a capped grid tests it.
GRIDS = [(1, 64), (2, 64), (1, 4)]
_PILOT_MIXED_SEED = max(sf.MIXED_SEEDS, key=lambda s: int(sf.mixed(s)[1]["width"]) * int(sf.mixed(s)[1]["height"]))


def _pilot_frames():
    W, H = 72, 40
    yield "s1000_200", scenes.scene_s1000(n=200), scenes.camera_for(W, H)
    yield "mixed", *sf.mixed(_PILOT_MIXED_SEED)
    yield "edge_material", *fz.EDGE_MATERIALS["smooth_neg1_metal"]


PILOT_FRAMES = {name: (objs, cam) for name, objs, cam in _pilot_frames()}


def _pilot_setup(gpu, sky, frame):
    objs, cam = PILOT_FRAMES[frame]
    cam = camera_get_copy(cam)
    W, H = int(cam["width"]), int(cam["height"])
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(31)
    return cam, W, H


def _pilot_costs(gpu, cam, W, H, passes, depth, ordered):
    """tile_costs uncapped and under every grid of GRIDS; the RNG states stay what they were."""
    rng0 = gpu.read_rng()
    out = {None: gpu.tile_costs(cam, passes, depth, ordered=ordered)}
    refilled = 0
    for wg, lpw in GRIDS:
        lanes = wg * 16 * lpw
        # (1, 4) refills on every frame; the full-width grids where the frame has the pixels
        strict = math.prod(tile_grid(W, H)) * 64 >= 2 * lanes and W * H > lanes
        assert strict or lpw == 64
        refilled += strict
        gpu.set_debug_grid(wg, lpw)
        try:
            out[(wg, lpw)] = gpu.tile_costs(cam, passes, depth, ordered=ordered)
        finally:
            gpu.set_debug_grid(0, 0)
    assert refilled >= 1
    np.testing.assert_array_equal(gpu.read_rng(), rng0)
    return out


@pytest.mark.parametrize("ordered", [False, "plain"])
@pytest.mark.parametrize("passes", [2, 5])
@pytest.mark.parametrize("frame", list(PILOT_FRAMES))
def test_pilot_costs_do_not_depend_on_the_grid(gpu, sky, frame, passes, ordered):
    """The reference walk and the plain ordered walk test each leaf where the ray meets it, so a
    pixel's segments + node visits + primitive tests depend on its own rays only: each tile's cost
    (its heaviest pixel's work) is the same however many pixels the lane ran before."""
    cam, W, H = _pilot_setup(gpu, sky, frame)
    if frame == "s1000_200":
        assert math.prod(tile_grid(W, H)) * 64 >= 2 * 1024   # refills at (1, 64) too
    out = _pilot_costs(gpu, cam, W, H, passes, 8, ordered)
    assert (out[None] > 0).all()
    for grid in GRIDS:
        np.testing.assert_array_equal(out[grid], out[None], err_msg=str(grid))


@pytest.mark.parametrize("passes", [2, 5])
@pytest.mark.parametrize("frame", list(PILOT_FRAMES))
def test_pilot_costs_wide_walk_same_zero_tiles(gpu, sky, frame, passes):
    """The default 4-wide walk tests a lane's parked leaf when its wave's leaf round fires and
    culls with the limit of the lane's last round, so a pixel's node and primitive counts depend
    on its wave-mates: the capped costs need not equal the uncapped ones.  They
    agree on which tiles cost nothing (none: every tile of these frames holds a pixel, and a pixel
    costs at least one segment per pass)."""
    cam, W, H = _pilot_setup(gpu, sky, frame)
    out = _pilot_costs(gpu, cam, W, H, passes, 8, True)
    assert (out[None] >= passes).all()
    for grid in GRIDS:
        np.testing.assert_array_equal(out[grid] == 0, out[None] == 0, err_msg=str(grid))


@pytest.mark.parametrize("ordered", [False, "plain"])
def test_pilot_cost_is_the_pixels_counted_work(gpu, sky, ordered):
    """The cost's definition: a one-pixel frame's only tile costs exactly the segments + nodes +
    prims a counting render of the same passes from the same RNG state reports.  (Tiles group eight
    context rows, so only a frame of one row and one column has one pixel per tile; a tile's cost is
    its pixels' maximum, not their sum.)  With the test above this pins the capped costs too."""
    objs = scenes.scene_s1000(n=200)
    H, passes, depth = 24, 3, 8
    cam = camera_get_copy(scenes.camera_for(1, H))
    gpu.set_scene(objs)
    gpu.set_env(sky)
    total = 0
    for row in range(0, H, 5):
        gpu.set_frame(1, H, [row])
        gpu.init_rng(9)
        cost = gpu.tile_costs(cam, passes, depth, ordered=ordered)
        assert cost.shape == (1, 1)
        gpu.reset_stats()
        gpu.render(cam, passes, depth, stats=True, sync=True, ordered=ordered)
        st = gpu.stats()
        assert st["segments"] >= passes
        assert int(cost[0, 0]) == st["segments"] + st["nodes"] + st["prims"], row
        total += int(cost[0, 0])
    assert total > 0
