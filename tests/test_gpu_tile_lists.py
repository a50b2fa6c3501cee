"""The device-built tile lists, read back with cpt_debug_read_tile_order and held to a model at the
sizes where their kernels have more than one wave of them (DESIGN.md §18 "The tile lists").

k_compact_order (cpt_adaptive.hip) places a kept tile by three offsets: its rank within its wave
(ballot + mbcnt), the kept counts of the waves before it in its chunk of 1024 (`before`, LDS) and
the running count of the chunks before (`base`).  The other adaptive tests have at most 64 tiles:
one wave of one chunk.  Here

  132 x 68    17 x 9  =  153 tiles   three waves (64, 64, 25), one chunk: `before`, s_px[1..2]
  268 x 252   34 x 32 = 1088 tiles   two chunks (1024, 64): `base`, the barrier between chunks
  1920 x 1080         = 32400 tiles  32 chunks (the feature's own workload), without the oracle

and both small frames have partial tiles at the right and bottom edges.  Before every step of the
render the pending round's list must equal the model's exactly and in order; after the last step
the whole state must (accumulator, RNG, noise map, round record, passes_done, which is the list's
pixel sum).  Each test asserts on the model, before the GPU call it guards, that its inputs reach
the code it is about.  Of the wave-offset precondition ("kept tiles in at least 4 waves of chunk
0") the 153-tile frame can only give its 3 waves, so there it is "in every wave"; the 1088-tile
frame gives 16.

The oracle's rounds of the 1088-tile frame (S4, 268 x 252, 6 rounds of 4 passes, depth 8) take
0.4 to 0.5 s with 8 threads, those of the 153-tile frame (S1000 n = 40) 0.2 s; `adaptive_model.run`
0.03 s. The full-size model's snapshots are plain GPU renders (tests/test_gpu_fullsize.py holds
those to the oracle); the same four rounds from the oracle take 34 s and give the same rounds.

The sorts (cpt_schedule.hip): the cost schedule's order must be the stable descending sort of the
pilot's costs, the previous-pass order that of each tile's RNG draws; nothing else in the suite
reads an order back (the render-parity tests only prove a permutation).
"""
import ctypes
import math

import adaptive_model as am
import numpy as np
import pytest
from test_gpu_adaptive import _assert_state

from cpppathtracer_amd import CptError, Renderer, _lib, camera_get_copy, scenes, types
from cpppathtracer_amd._lib import CPT_SCHEDULE_COST, CPT_TRAVERSAL_ORDERED
from cpppathtracer_amd.tiling import tile_grid

pytestmark = pytest.mark.gpu

SEED = 1234
INVALID, STATE = 1, 5
CHUNK, WAVE = 1024, 64   # k_compact_order: COMPACT_BLOCK, the wavefront
EMPTY = np.zeros(0, dtype=types.OBJECT_DTYPE)
_cache = {}


def _frame(gpu, sky, objs, W, H, seed=SEED):
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(seed)
    return camera_get_copy(scenes.camera_for(W, H))


def _n_tiles(W, H):
    return math.prod(tile_grid(W, H))


def _stable_descending(keys):
    return np.argsort(-np.asarray(keys).astype(np.int64), kind="stable").astype(np.uint32)


def _raw_read(gpu, which, capacity, size):
    """cpt_debug_read_tile_order into a buffer of `size` sentinels: (status, buffer, *n)."""
    buf = np.full(size, 0xDEADBEEF, dtype=np.uint32)
    n = ctypes.c_size_t(0)
    st = _lib.load().cpt_debug_read_tile_order(gpu._ctx, which, ctypes.c_void_p(buf.ctypes.data), capacity, ctypes.byref(n))
    return st, buf, n.value


def _status(gpu, which):
    with pytest.raises(CptError) as e:
        gpu.debug_tile_order(which)
    return e.value.status


# ---------------------------------------------------------------------------------------------
# 2a. Compaction across waves and chunks, against the oracle's model.  Batch 4, 8..24 spp, depth 8,
# rel_error 0.05 (found on the CPU): the model's rounds render
#   132 x 68, S1000 n = 40:   153,  153,  152,  128,  41,   9 tiles
#   268 x 252, S4:           1088, 1088, 1087, 1051, 936, 852 tiles
# so the compaction after round 3 keeps 128 of 152 (per wave 56, 55, 17) resp. 1051 of 1087 (992
# below position 1024, not a multiple of 64, and 59 above), and the one after round 4 runs on a list
# already shortened to 128 (> 64) resp. 1051 (> 1024) entries.
# ---------------------------------------------------------------------------------------------
ADAPT = dict(batch=4, min_spp=8, max_spp=24, depth=8, t=0.05)
FRAMES = {
    "three_waves_132x68": dict(W=132, H=68, scene=lambda: scenes.scene_s1000(n=40)),
    "two_chunks_268x252": dict(W=268, H=252, scene=scenes.scene_s4),
}


def _compactions(m):
    """(round, kept flag per position) of the compaction after each round, in raster order: the
    list of round r is the tiles that stop at r or later, and it keeps those that stop later."""
    for r in range(1, len(m["active"]) + 1):
        ids = np.nonzero(m["stop"] >= r)[0]
        yield r, m["stop"][ids] > r


def _reaches_the_offsets(kept, n_tiles):
    """Does this compaction need `before` (and, with more than one chunk, `base`) to be right?"""
    c0 = kept[:CHUNK]
    per_wave = [int(c0[i:i + WAVE].sum()) for i in range(0, c0.size, WAVE)]
    waves_wanted = min(4, (n_tiles + WAVE - 1) // WAVE)
    ok = sum(c > 0 for c in per_wave) >= waves_wanted and len(set(per_wave)) > 1
    if n_tiles > CHUNK:
        below = int(c0.sum())
        ok = ok and kept[CHUNK:].any() and 0 < below < c0.size and below % WAVE != 0
    return ok


def _model_2a(oracle_mod, sky, name):
    """The frame's model, computed once and shared (read only), with its preconditions asserted."""
    if name not in _cache:
        f, a = FRAMES[name], ADAPT
        W, H = f["W"], f["H"]
        assert W % 8 and H % 8   # partial tiles at the right and bottom edges
        cam = camera_get_copy(scenes.camera_for(W, H))
        rows = np.arange(H, dtype=np.int32)
        rng = oracle_mod.init_rng(SEED, W, rows, threads=8)
        snaps = am.oracle_rounds(oracle_mod, f["scene"](), cam, sky, rows, a["batch"], a["max_spp"] // a["batch"],
                                 a["depth"], rng)
        m = am.run(snaps, W, H, a["batch"], a["min_spp"], a["max_spp"], np.float32(a["t"]))
        n = _n_tiles(W, H)
        assert len(m["stop"]) == n and n == (153 if name.startswith("three") else 1088)
        last = a["max_spp"] // a["batch"]
        mixed = [(r, kept) for r, kept in _compactions(m)
                 if r * a["batch"] >= a["min_spp"] and r < last and kept.any() and not kept.all()]
        first = [r for r, kept in mixed if _reaches_the_offsets(kept, n)]
        assert first, "no compaction with kept tiles spread unevenly over the waves (and both chunks)"
        # a later compaction of a list that is already shorter than the frame's, and still longer
        # than one wave (one chunk on the large frame: S4 at this rel_error allows that)
        longer_than = CHUNK if n > CHUNK else WAVE
        assert any(r > first[0] and longer_than < kept.size < n for r, kept in mixed)
        for v in (m["stop"], m["active"], m["accum"], m["rng"], m["noise"]):
            v.flags.writeable = False
        _cache[name] = m
    return _cache[name]


def _drive(gpu, cam, m, a, flags):
    """begin / step with the pending round's list read, and held to the model's, before every step."""
    gpu.adaptive_begin(cam, a["min_spp"], a["max_spp"], a["batch"], a["t"], a["depth"], flags=flags)
    pending = [True]
    try:
        _drive_pending(gpu, m, flags, pending)
    finally:
        # a failed assert must not leave the session's context with a render pending
        while pending[0] and gpu.adaptive_step():
            pass


def _drive_pending(gpu, m, flags, pending):
    n = len(m["stop"])
    if flags & CPT_SCHEDULE_COST:
        order0 = gpu.debug_tile_order(0)
        np.testing.assert_array_equal(np.sort(order0), np.arange(n, dtype=np.uint32))
    else:
        assert _status(gpu, 0) == STATE   # no pilot has run on this frame
        order0 = np.arange(n, dtype=np.uint32)
    # a capacity below the list's length, another `which`: refused, nothing written, nothing changed
    st, buf, length = _raw_read(gpu, 2, n - 1, n)
    assert st == INVALID and length == n and (buf == 0xDEADBEEF).all()
    for which in (-1, 3):
        st, buf, _ = _raw_read(gpu, which, n, n)
        assert st == INVALID and (buf == 0xDEADBEEF).all()
    for r in range(1, len(m["active"]) + 1):
        want = order0[m["stop"][order0] >= r]
        assert want.size == m["active"][r - 1]
        np.testing.assert_array_equal(gpu.debug_tile_order(2), want, err_msg=f"the list of round {r}")
        pending[0] = False   # a step that raises ends the render itself
        active = gpu.adaptive_step()
        pending[0] = active > 0
        assert active == (m["active"][r] if r < len(m["active"]) else 0), f"tiles kept after round {r}"


@pytest.mark.parametrize("order", ["raster", "cost_ordered"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_compaction_across_waves_and_chunks(gpu, oracle_mod, sky, name, order):
    """Every round's list equals the model's, in raster order (the active ids ascending) and under
    CPT_SCHEDULE_COST | CPT_TRAVERSAL_ORDERED (the pilot's order with the stopped tiles struck out:
    the compaction is stable); then the state is cpt_render_adaptive's, and the probe has left the
    render as it was.  The preconditions are asserted for the raster lists: where the kept tiles
    sit in a cost-ordered list depends on the pilot."""
    f, a = FRAMES[name], ADAPT
    m = _model_2a(oracle_mod, sky, name)
    cam = _frame(gpu, sky, f["scene"](), f["W"], f["H"])
    assert _status(gpu, 2) == STATE   # nothing pending yet
    flags = CPT_SCHEDULE_COST | CPT_TRAVERSAL_ORDERED if order == "cost_ordered" else 0
    _drive(gpu, cam, m, a, flags)
    _assert_state(gpu, gpu.adaptive_info(), m)
    assert _status(gpu, 2) == STATE   # the render has ended
    st, buf, _ = _raw_read(gpu, 2, len(m["stop"]), len(m["stop"]))
    assert st == STATE and (buf == 0xDEADBEEF).all()


# ---------------------------------------------------------------------------------------------
# 2b. The workload's size: 32 400 tiles, 32 chunks.
# ---------------------------------------------------------------------------------------------
def test_fullsize_compaction_against_plain_renders(gpu, sky):
    """1920 x 1080, S1000, ordered walk, batch 4, 8..16 spp, depth 8, rel_error 0.2.  The model's
    snapshots are plain renders of 4, 8, 12 and 16 passes on a second context; the lists of all
    rounds, the final state and passes_done must be the model's.  (With the oracle's snapshots the
    model renders 32400, 32400, 28330, 26376 tiles, stopping 4070 tiles at round 2 and 1954 at
    round 3, and the tiles kept after round 2 lie in all 32 chunks.)"""
    W, H = 1920, 1080
    a = dict(batch=4, min_spp=8, max_spp=16, depth=8, t=0.2)
    objs = scenes.scene_s1000()
    snaps = []
    with Renderer(0) as other:
        cam = _frame(other, sky, objs, W, H)
        for k in range(a["max_spp"] // a["batch"]):
            other.render(cam, a["batch"], a["depth"], ordered=True, accumulate=k > 0, sync=True)
            snaps.append((other.read_accum(), other.read_rng(), None))
    m = am.run(snaps, W, H, a["batch"], a["min_spp"], a["max_spp"], np.float32(a["t"]))
    assert len(m["stop"]) == 32400
    assert len(set(m["stop"].tolist())) >= 2   # tiles stop at different rounds
    # round 2 is the first eligible one: its list is every tile, a tile's position is its id
    assert m["active"][1] == 32400
    assert len(set((np.nonzero(m["stop"] > 2)[0] // CHUNK).tolist())) >= 16
    cam = _frame(gpu, sky, objs, W, H)
    _drive(gpu, cam, m, a, CPT_TRAVERSAL_ORDERED)
    _assert_state(gpu, gpu.adaptive_info(), m)
    gpu.set_frame(8, 8)   # release the full-size frame's buffers


# ---------------------------------------------------------------------------------------------
# 2c. The cost schedule's sort.
# ---------------------------------------------------------------------------------------------
def _assert_stable_descending(order, cost):
    n = cost.size
    np.testing.assert_array_equal(np.sort(order), np.arange(n, dtype=np.uint32))   # a permutation
    c = cost[order].astype(np.int64)
    assert (np.diff(c) <= 0).all(), "cost[order] is not heaviest first"
    assert (np.diff(order.astype(np.int64))[np.diff(c) == 0] > 0).all(), "equal costs: the ids do not ascend"
    np.testing.assert_array_equal(order, _stable_descending(cost))


PILOT_MAX, PILOT_DIV = 16, 128   # cpt_capi_render.cpp cost_pilot_passes


@pytest.mark.parametrize("W,H", [(8, 8), (20, 12), (132, 68), (268, 252)])
def test_cost_order_is_the_stable_sort_of_the_pilot_costs(gpu, sky, W, H):
    """cpt_tile_costs runs the whole pilot, so its costs and order 0 come from one run; then a
    CPT_SCHEDULE_COST render of 256 passes (a pilot of 2) leaves the order of its own pilot's costs,
    which a second context gives from the same RNG state (the pilot writes nothing back).  The plain
    ordered walk: its costs depend on a pixel's own rays only (tests/test_gpu_refill.py), so two
    pilots from one state agree."""
    objs = scenes.scene_s1000(n=40)
    n = _n_tiles(W, H)
    cam = _frame(gpu, sky, objs, W, H)
    assert _status(gpu, 0) == STATE   # no pilot has run on this frame
    cost = gpu.tile_costs(cam, 4, 8, ordered="plain").reshape(-1)
    assert cost.size == n
    if n >= 153:
        assert len(np.unique(cost)) >= 8
    order = gpu.debug_tile_order(0)
    _assert_stable_descending(order, cost)
    spp = 256
    passes = min(PILOT_MAX, max(1, spp // PILOT_DIV))
    assert passes == 2
    gpu.render(cam, spp, 8, ordered="plain", schedule="cost", sync=True)
    order2 = gpu.debug_tile_order(0)
    with Renderer(0) as other:
        _frame(other, sky, objs, W, H)
        cost2 = other.tile_costs(cam, passes, 8, ordered="plain").reshape(-1)
    assert (cost2 != cost).any()   # another pilot: the first order would not do
    _assert_stable_descending(order2, cost2)
    st, buf, length = _raw_read(gpu, 0, n - 1, n)
    assert st == INVALID and length == n and (buf == 0xDEADBEEF).all()


def test_cost_order_of_equal_costs_is_the_identity(gpu, sky):
    """The empty scene: every tile's heaviest pixel does the same work, the partial tiles' too, and
    the stable sort leaves k_iota's ids as they are."""
    W, H = 132, 68
    cam = _frame(gpu, sky, EMPTY, W, H)
    cost = gpu.tile_costs(cam, 4, 8).reshape(-1)
    assert cost.size == 153 and (cost == cost[0]).all()
    np.testing.assert_array_equal(gpu.debug_tile_order(0), np.arange(153, dtype=np.uint32))


# ---------------------------------------------------------------------------------------------
# 2d. The previous-pass order.
# ---------------------------------------------------------------------------------------------
WEYL = 362437
WEYL_INV = pow(WEYL, -1, 1 << 32)


def _draw_keys(d0, d1, W, H):
    """k_tile_draws: each tile's sum, over its pixels inside the frame, of the draws since d0
    (every draw adds WEYL to the plane), saturated at 2^32 - 1; and the pixels in each sum."""
    draws = ((d1.astype(np.uint64) - d0.astype(np.uint64)) % (1 << 32) * np.uint64(WEYL_INV)) % (1 << 32)
    tile = am.tile_of_pixel(W, H)
    keys = np.zeros(_n_tiles(W, H), dtype=np.uint64)
    np.add.at(keys, tile, draws.astype(np.uint64))
    return np.minimum(keys, (1 << 32) - 1), np.bincount(tile, minlength=keys.size)


@pytest.mark.parametrize("W,H", [(20, 12), (132, 68)])
def test_previous_order_is_the_stable_sort_of_the_draws(gpu, sky, W, H):
    """One CPT_SCHEDULE_PREVIOUS render of a fresh frame leaves the tiles by descending draws of
    that render (the Weyl plane before and after), ids ascending among equals.  cpt_init_rng
    replaces the streams the order was measured on: no order is held until the next such render
    rebuilds it (before this test existed the old order stayed valid across a re-seed)."""
    assert (WEYL * WEYL_INV) % (1 << 32) == 1
    objs = scenes.scene_s1000(n=40)
    ty, tx = tile_grid(W, H)
    cam = _frame(gpu, sky, objs, W, H)
    assert _status(gpu, 1) == STATE   # no such render yet
    for seed in (SEED, 77):
        if seed != SEED:
            gpu.init_rng(seed)
            assert _status(gpu, 1) == STATE   # not the order of the streams just replaced
        d0 = gpu.read_rng()[5]
        gpu.render(cam, 2, 8, ordered=True, schedule="previous", sync=True)
        d1 = gpu.read_rng()[5]
        keys, pixels = _draw_keys(d0, d1, W, H)
        partial = (np.arange(tx * ty) % tx == tx - 1) | (np.arange(tx * ty) // tx == ty - 1)
        assert W % 8 and H % 8 and (pixels[partial] < 64).all() and (pixels[~partial] == 64).all()
        assert pixels.sum() == W * H and len(np.unique(keys)) >= 4
        got = gpu.debug_tile_order(1)
        np.testing.assert_array_equal(got, _stable_descending(keys), err_msg=f"seed {seed}")
    st, buf, length = _raw_read(gpu, 1, tx * ty - 1, tx * ty)
    assert st == INVALID and length == tx * ty and (buf == 0xDEADBEEF).all()
