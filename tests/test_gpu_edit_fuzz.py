"""The device refit (cpt_update_objects -> k_refit_leaves / k_refit_nodes) over the edit sequences
of edit_fuzz.py, within ONE context per sequence: set_scene, set_env and set_frame once, then for
every frame update_objects, init_rng, render -- the use the refit exists for -- and never a
set_scene in between.  Everything is bit-exact, against the oracle's refit
(oracle.render_edited) or against the library's own fresh upload of the same scene:

* sequence parity: every frame's accumulator bits, RNG end states and counters are the oracle's;
* round trip: after the sequence and `inverse`, the render equals a fresh set_scene(objs) one in
  image, RNG and the whole stats dict -- the 4-wide walk's own node / primitive counts included,
  which no oracle comparison covers: a box left too large costs visits and fails nothing else;
* path independence: the sequence equals a fresh scene plus the one batch `net(...)`;
* host tree: after every frame cpt_scene_bvh_export is edit_fuzz.refit_reference bit for bit;
* device bytes: the node memory itself (Renderer.read_nodes: reference order, eight octant orders,
  4-wide image, leaf array) after the round trip and after `net`, against a fresh upload;
* an update queued behind a render in flight, and the argument checks.

test_edit_fuzz.py checks on the CPU that the sequences are what they are meant to be."""
import time

import edit_fuzz as ef
import numpy as np
import pytest
from test_gpu_async_order import SPP as ASYNC_SPP
from test_gpu_async_order import assert_overlap
from test_gpu_fuzz_parity import SHORT_PATHS
from test_gpu_parity import _check_stats, _kw, _timed

from cpppathtracer_amd import CptError, camera_get_copy
from cpppathtracer_amd.types import OBJECT_DTYPE

pytestmark = pytest.mark.gpu

SEQ = ef.sequences()
NAMES = list(SEQ)
REFIT_ONLY = ef.refit_only()
SEED = 5
_ORACLE = {}


def _oracle(oracle_mod, sky, name, f, path, spp=None):
    """The oracle's (accum, rng, stats) after frames[:f + 1] (f = -1: the scene as built); for an
    ordered path the stats carry the diagnostic walk's under "walk", as _check_stats expects.  The
    renders do not depend on the path, so they are made once.  spp: the passes, when they are not
    the family's (ef.PARAMS)."""
    acc, rng, st, walk = _oracle_renders(oracle_mod, sky, name, f, spp)
    return acc, rng, (dict(st, walk=walk) if _kw(path)["ordered"] else dict(st))


def _oracle_renders(oracle_mod, sky, name, f, spp=None):
    if (name, f, spp) in _ORACLE:
        return _ORACLE[(name, f, spp)]
    family, objs, cam, frames = SEQ[name]
    depth = ef.PARAMS[family][1]
    spp = spp or ef.PARAMS[family][0]
    cam = camera_get_copy(cam)
    W, H = int(cam["width"]), int(cam["height"])
    rows = np.arange(H, dtype=np.int32)
    edits = ef.flat(frames[:f + 1])
    out = []
    for walk in (False, True):
        rng = oracle_mod.init_rng(SEED, W, rows, threads=8)
        oracle_mod.set_walk(walk)
        try:
            acc, st = oracle_mod.render_edited(objs, edits, cam, sky, rows, spp, depth, rng, threads=8)
            if walk:
                st["fallbacks"] = oracle_mod.last_fallbacks()
        finally:
            oracle_mod.set_walk(False)
        out.append((acc, rng, st))
    np.testing.assert_array_equal(out[1][0].view(np.uint32), out[0][0].view(np.uint32))
    np.testing.assert_array_equal(out[1][1], out[0][1])
    key = (name, f, None if spp == ef.PARAMS[family][0] else spp)
    _ORACLE[key] = (out[0][0], out[0][1], out[0][2], out[1][2])
    return _ORACLE[key]


def _setup(gpu, sky, name):
    family, objs, cam, _ = SEQ[name]
    cam = camera_get_copy(cam)
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(int(cam["width"]), int(cam["height"]))
    return (cam,) + ef.PARAMS[family]


def _render(gpu, view, path):
    cam, spp, depth = view
    gpu.init_rng(SEED)
    gpu.reset_stats()
    stats = not _timed(path)
    gpu.render(cam, spp, depth, stats=stats, sync=True, **_kw(path))
    gs = gpu.stats() if stats else None
    if stats and _kw(path)["ordered"]:
        gs["fallbacks"] = gpu.raw_counters()[5]
    return gpu.read_accum(), gpu.read_rng(), gs


def _calls(f, batch):
    """One batch call on even frames, one call per edit on odd frames."""
    return [batch] if f % 2 == 0 else [[e] for e in batch]


def _update(gpu, batch):
    gpu.update_objects([i for i, _ in batch], np.array([o for _, o in batch], dtype=OBJECT_DTYPE))


def _play(gpu, name, view=None, path=None):
    """Every frame of the sequence; with `view`, a render after each (as an animation does)."""
    if view is not None:
        gpu.init_rng(SEED)
    for f, batch in enumerate(SEQ[name][3]):
        for call in _calls(f, batch):
            _update(gpu, call)
        if view is not None:
            cam, spp, depth = view
            gpu.render(cam, spp, depth, sync=True, **_kw(path))


def _rebuild_from(name):
    """The first frame whose calls make the library rebuild its walk tree (a platform flip, or the
    material table crossing its compaction threshold); len(frames) when none does."""
    _, objs, _, frames = SEQ[name]
    cur, calls = objs.copy(), []
    for f, batch in enumerate(frames):
        calls += _calls(f, batch)
        for i, o in batch:
            if (int(cur[i]["type"]) == 1) != (int(o["type"]) == 1):
                return f
            cur[i] = o
        if ef.material_table(objs, calls)[1]:
            return f
    return len(frames)


def _assert_same_render(a, b, path):
    """Image bits, RNG end states and the whole stats dict (the wide walk's own nodes / prims
    too) of two renders of what should be the same device scene.

    wavefront:ordered is compared without `nodes` and `prims`: they are not a function of the
    scene there.  The wavefront's queues take their slots from one atomicAdd per wave
    (cpt_wavefront.hip wave_append), so from the second bounce on the rays that share a wave depend
    on timing, and the parked-leaf rounds count per wave (cpt.h, CPT_TRAVERSAL_PLAIN_LEAVES).  On one
    MI355X, 8 wavefront:ordered renders of one unchanged scene gave 5 distinct (nodes, prims) pairs on
    mixed_edits-102 (14995 .. 15017 nodes, 17206 .. 17222 prims) and 8 on mixed_large_edits-400 (25162
    .. 25173 nodes), with the same image, RNG states and segments every time; the megakernel, whose
    waves are its 8 x 8 tiles, gave one pair.  With the counts compared, 11 of the 36 wavefront:ordered
    cases here failed by such amounts in either direction, on node memory that test_device_bytes
    shows to be byte-identical.  What the counts were to show on the wavefront -- no copy of a box
    left too large in the 4-wide image or the leaf array -- test_device_bytes shows on the bytes
    themselves, which every path reads."""
    sa, sb = a[2], b[2]
    if sa is not None and path.split("+")[0] == "wavefront:ordered":
        sa, sb = ({k: v for k, v in s.items() if k not in ("nodes", "prims")} for s in (sa, sb))
    np.testing.assert_array_equal(a[1], b[1])
    assert sa == sb
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


# ---------------------------------------------------------------------- sequence parity
@pytest.mark.parametrize("path", SHORT_PATHS)
@pytest.mark.parametrize("name", NAMES)
def test_sequence_parity(gpu, oracle_mod, sky, name, path):
    """Every frame of every sequence against oracle.render_edited(objs, edits so far).  From the
    frame that makes the library rebuild its walk tree (flip_last, compaction) the walk's node
    counts are no longer compared; segments, hits and misses still are."""
    family, objs, _, frames = SEQ[name]
    view = _setup(gpu, sky, name)
    rebuilt = _rebuild_from(name)
    assert (rebuilt < len(frames)) == (family in ("flip_last", "compaction"))
    n_mats = gpu.material_count()
    for f, batch in enumerate(frames):
        for call in _calls(f, batch):
            _update(gpu, call)
        ga, gr, gs = _render(gpu, view, path)
        oa, orng, os_ = _oracle(oracle_mod, sky, name, f, path)
        np.testing.assert_array_equal(gr, orng, err_msg=f"frame {f}")
        if f < rebuilt:
            _check_stats(gs, os_, path)
        elif gs is not None:
            for k in ("segments", "hits", "misses"):
                assert gs[k] == os_[k], (f, k)
        np.testing.assert_array_equal(ga.view(np.uint32), oa.view(np.uint32), err_msg=f"frame {f}")
    if family == "compaction":   # 80 materials went in; the table was compacted on the way
        assert gpu.material_count() < n_mats + len(ef.flat(frames))
    elif family in ef.REFIT_ONLY:
        assert gpu.material_count() == len(ef.material_table(objs, frames)[0])


# --------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("path", SHORT_PATHS)
@pytest.mark.parametrize("name", REFIT_ONLY)
def test_round_trip(gpu, sky, name, path):
    """The sequence (a render after every frame), then `inverse`: the render equals that of a
    fresh set_scene(objs) in image, RNG end states and every counter."""
    _, objs, _, frames = SEQ[name]
    view = _setup(gpu, sky, name)
    _play(gpu, name, view, path)
    _update(gpu, ef.inverse(objs, frames))
    back = _render(gpu, view, path)
    gpu.set_scene(objs)
    _assert_same_render(back, _render(gpu, view, path), path)


# -------------------------------------------------------------------- path independence
@pytest.mark.parametrize("path", SHORT_PATHS)
@pytest.mark.parametrize("name", REFIT_ONLY)
def test_path_independence(gpu, sky, name, path):
    """The whole sequence equals a fresh set_scene(objs) plus the single batch net(...): a box a
    grow-then-shrink left too large would show up here as a node count."""
    _, objs, _, frames = SEQ[name]
    view = _setup(gpu, sky, name)
    _play(gpu, name, view, path)
    seq = _render(gpu, view, path)
    gpu.set_scene(objs)
    _update(gpu, ef.net(objs, frames))
    _assert_same_render(seq, _render(gpu, view, path), path)


# ---------------------------------------------------------------------------- host tree
@pytest.mark.parametrize("name", NAMES)
def test_host_tree_is_the_independent_refit(gpu, name):
    """After every frame cpt_scene_bvh_export's boxes are edit_fuzz.refit_reference's, bit for bit
    (-0 and the platforms' 5e30 included), and the links are those of the build."""
    _, objs, _, frames = SEQ[name]
    gpu.set_scene(objs)
    boxes0, links0 = gpu.bvh_export()
    np.testing.assert_array_equal(boxes0.view(np.uint32), ef.refit_reference(boxes0, links0, objs).view(np.uint32))
    for f, (batch, state) in enumerate(zip(frames, ef.states(objs, frames))):
        for call in _calls(f, batch):
            _update(gpu, call)
        boxes, links = gpu.bvh_export()
        np.testing.assert_array_equal(links, links0, err_msg=f"frame {f}")
        np.testing.assert_array_equal(boxes.view(np.uint32), ef.refit_reference(boxes0, links0, state).view(np.uint32),
                                      err_msg=f"frame {f}")


# ------------------------------------------------------------------------- device bytes
def _regions(info, n_bytes):
    """(name, first byte, end byte, bytes per node) of the parts of the device's node memory."""
    nb, nw, nwide = info["n_bvh"], info["n_walk"], info["n_wide"]
    regs = [("reference order", 0, 32 * nb, 32)]
    regs += [(f"octant {o} order", 32 * (nb + o * nw), 32 * (nb + (o + 1) * nw), 32) for o in range(8)]
    end = 32 * (nb + 8 * nw)
    if nwide > 0:
        leaves = end + 32 * ((7 * nwide + 1) // 2)
        regs += [("4-wide image", end, leaves, 112), ("leaf array", leaves, n_bytes, 32)]
        assert leaves < n_bytes
        end = n_bytes
    assert end == n_bytes, (info, n_bytes)
    return regs


def _assert_same_bytes(got, want, info, what):
    assert got.size == want.size, what
    diff = np.flatnonzero(got != want)
    if diff.size:
        b = int(diff[0])
        for region, lo, hi, stride in _regions(info, got.size):
            if lo <= b < hi:
                raise AssertionError(f"{what}: {diff.size} bytes differ, the first in the {region}, node "
                                     f"{(b - lo) // stride}, byte {(b - lo) % stride} of it")
        raise AssertionError(f"{what}: byte {b} differs, outside every region")


@pytest.mark.parametrize("name", REFIT_ONLY)
def test_device_bytes(gpu, name):
    """The device's node memory after the sequence + inverse equals a fresh upload's, and after the
    sequence equals a fresh upload's + net(...): every one of a box's up to 11 copies, whether or
    not a ray of these small frames passes through it."""
    _, objs, _, frames = SEQ[name]
    gpu.set_scene(objs)
    info = gpu.walk_info()
    _play(gpu, name)
    seq = gpu.read_nodes()
    _update(gpu, ef.inverse(objs, frames))
    back = gpu.read_nodes()
    gpu.set_scene(objs)
    assert gpu.walk_info() == info
    fresh = gpu.read_nodes()
    _regions(info, fresh.size)
    assert name != "mixed_large_edits-400" or info["n_wide"] > 0
    _assert_same_bytes(back, fresh, info, "sequence + inverse against a fresh upload")
    _update(gpu, ef.net(objs, frames))
    _assert_same_bytes(seq, gpu.read_nodes(), info, "sequence against a fresh upload + net")
    assert (seq != fresh).any()   # the edits did reach the device


# ----------------------------------------------------------------------- in-flight render
@pytest.mark.parametrize("name", [n for n in NAMES if SEQ[n][0] == "all_dirty"])
def test_update_behind_a_render_in_flight(gpu, oracle_mod, sky, name):
    """render(sync=False), then at once an update that dirties every leaf: the accumulator is the
    oracle's image of the scene BEFORE the edit, and the next render its image after.  With the
    passes and the overlap condition of test_gpu_async_order.py: at least three quarters of the
    render were still ahead when the update began."""
    path = "megakernel:ordered"
    cam, _, depth = _setup(gpu, sky, name)
    view = cam, ASYNC_SPP, depth
    gpu.init_rng(SEED)
    gpu.synchronize()
    t_launch = time.perf_counter()
    gpu.render(cam, ASYNC_SPP, depth, sync=False, consolidate=False, **_kw(path))
    t_call = time.perf_counter()
    _update(gpu, SEQ[name][3][0])
    acc, rng = gpu.read_accum(), gpu.read_rng()
    assert_overlap(name, t_launch, t_call, gpu.last_render_ms())
    oa, orng, _ = _oracle(oracle_mod, sky, name, -1, path, ASYNC_SPP)
    np.testing.assert_array_equal(rng, orng)
    np.testing.assert_array_equal(acc.view(np.uint32), oa.view(np.uint32))
    ga, gr, gs = _render(gpu, view, path)
    oa, orng, os_ = _oracle(oracle_mod, sky, name, 0, path, ASYNC_SPP)
    np.testing.assert_array_equal(gr, orng)
    _check_stats(gs, os_, path)
    np.testing.assert_array_equal(ga.view(np.uint32), oa.view(np.uint32))


# ------------------------------------------------------------------------ bad arguments
def test_empty_batch_and_bad_index_change_nothing(gpu, sky):
    """An empty batch is OK and changes nothing.  An out-of-range index in the middle of a batch
    is CPT_ERR_INVALID_ARG, and the range check runs before any write: the objects before it in the
    batch are not applied -- same host tree, same device bytes, same render."""
    name, path = "tiny_trees-3_prims_floor", "megakernel:ordered"
    _, objs, _, frames = SEQ[name]
    view = _setup(gpu, sky, name)
    _update(gpu, frames[0])
    before = _render(gpu, view, path)
    boxes, links = gpu.bvh_export()
    nodes, n_mats = gpu.read_nodes(), gpu.material_count()
    gpu.update_objects(np.zeros(0, np.int32), np.zeros(0, dtype=objs.dtype))
    _assert_same_render(before, _render(gpu, view, path), path)
    good = frames[-1]
    assert len(good) == 3
    for bad in (len(objs), -1):
        with pytest.raises(CptError) as e:
            gpu.update_objects([good[0][0], bad, good[2][0]], np.array([o for _, o in good], dtype=objs.dtype))
        assert e.value.status == 1   # CPT_ERR_INVALID_ARG
        b2, l2 = gpu.bvh_export()
        np.testing.assert_array_equal(b2.view(np.uint32), boxes.view(np.uint32))
        np.testing.assert_array_equal(l2, links)
        assert gpu.material_count() == n_mats
        np.testing.assert_array_equal(gpu.read_nodes(), nodes)
        _assert_same_render(before, _render(gpu, view, path), path)
