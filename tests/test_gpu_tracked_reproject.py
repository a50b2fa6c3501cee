"""Tracked reprojection on the GPU: the tracked kernels against
cpt_reproject_tracked_host / cpt_reproject_display_tracked_host bit for bit (themselves held to the
numpy restatement by tests/test_tracked_reproject_model.py), the equivalence with the untracked
calls when nothing was edited, the renewed history, what the calls leave alone, their error codes
and stream order, and the point of it all: after an object moved, the tracked history is closer to
the truth than a restart and than the stale history.
"""
import ctypes
from types import SimpleNamespace

import gbuffer_model as gm
import numpy as np
import pytest
import reproject_model as rm
import test_gpu_async_order as ao
import tracked_reproject_model as tm

from cpppathtracer_amd import CptError, Renderer, camera_get_copy, scenes
from cpppathtracer_amd._lib import CPT_RENDER_AUX, CPT_TRAVERSAL_ORDERED, CPT_TRAVERSAL_PLAIN_LEAVES
from cpppathtracer_amd.renderer import object_motion_host, reproject_display_tracked_host, reproject_tracked_host
from cpppathtracer_amd.types import MOTION_DROP, MOTION_SAME, PLATFORM

pytestmark = pytest.mark.gpu

WALKS = {"reference": 0, "ordered": CPT_TRAVERSAL_ORDERED, "plain": CPT_TRAVERSAL_ORDERED | CPT_TRAVERSAL_PLAIN_LEAVES}
INVALID, STATE = 1, 5
DEPTH = 4
shared = ao.shared   # the ordering tests' workload (a module fixture of test_gpu_async_order.py)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _full(a, npix):
    """The display band's rows padded to the frame's: the rows below hold zeros on the device."""
    out = np.zeros((npix,) + a.shape[1:], dtype=np.float32)
    out[:a.shape[0]] = a
    return out


def _changed(old, new):
    idx = [k for k in range(len(old)) if old[k].tobytes() != new[k].tobytes()]
    kinds = object_motion_host(old, new)["kind"]
    return [k for k in idx if kinds[k] != MOTION_SAME]


def _display_passes(gpu, cam, n=3):
    for _ in range(n):
        gpu.render(cam, 1, DEPTH, aux=True, sync=True, ordered=True)
        gpu.denoise_mix_history()


def _parity(gpu, sky, old, new, pair, walks, rebuild=False, settings=(tm.MAX_HISTORY, tm.PLANE_TOL)):
    """Per walk: the old scene, a few real display passes and a written-in accumulator at the first
    camera, history_capture, the edit, then each tracked call against its host function on the
    device's own G-buffer planes.  Returns the last accumulator and the new frame's ids."""
    c0, c1 = camera_get_copy(pair[0]), camera_get_copy(pair[1])
    W, H = int(c0["width"]), int(c0["height"])
    He = 16 * (H // 16)
    d0, d1 = gm.camera_rays(c0)[1], gm.camera_rays(c1)[1]
    idx = _changed(old, new)
    motion = object_motion_host(old, new)
    mh, tol = settings
    got = g1 = None
    for walk in walks:
        flags = WALKS[walk]
        gpu.set_scene(old)
        gpu.set_env(sky)
        gpu.set_frame(W, H)
        gpu.init_rng(scenes.DEFAULT_SEED)
        if He:
            _display_passes(gpu, c0)
        gpu.history_capture(c0, flags)
        g0 = gpu.read_gbuffer()
        hist = rm.history(g0["id"], W, H)
        gpu.write_accum(hist)
        gpu.update_objects(idx, new[idx], rebuild=rebuild)
        # the accumulator
        gpu.reproject_accum_tracked(c1, mh, tol, flags)
        got, g1 = gpu.read_accum(), gpu.read_gbuffer()
        want = reproject_tracked_host(c0, c1, d0, d1, g0["id"], g0["t"], g1["id"], g1["t"], g1["normal"], hist, motion, mh, tol)
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=walk)
        ms3 = gpu.last_reproject_ms(split=True)
        assert ms3[0] == 0.0 and ms3[1] > 0.0 and ms3[2] > 0.0 and gpu.last_reproject_ms() > 0.0
        valid, cam = gpu.history_info()
        assert valid and cam.tobytes() == np.ascontiguousarray(c1).tobytes()
        if not He:
            continue
        # the display state, from the same capture: put the history back first
        gpu.update_objects(idx, old[idx], rebuild=rebuild)
        gpu.history_capture(c0, flags)
        gpu.update_objects(idx, new[idx], rebuild=rebuild)
        mean, cnt = gpu.read_mix(), gpu.read_display_count()
        assert (cnt > 0).any()
        want_m, want_n = reproject_display_tracked_host(c0, c1, d0, d1, g0["id"], g0["t"], g1["id"], g1["t"], g1["normal"],
                                                        _full(mean, W * H), _full(cnt, W * H), motion, mh, tol)
        gpu.reproject_display_tracked(c1, mh, tol, flags)
        np.testing.assert_array_equal(_bits(gpu.read_display_count()), _bits(want_n[:He * W]), err_msg=walk)
        np.testing.assert_array_equal(_bits(gpu.read_mix()), _bits(want_m[:He * W]), err_msg=walk)
        assert not want_n[He * W:].any()
    return got, g1["id"]


# ------------------------------------------------------------------- kernel = host function
@pytest.mark.parametrize("edit", sorted(tm.edits()))
@pytest.mark.parametrize("wh", [(64, 48), (67, 41)], ids=lambda wh: "%dx%d" % wh)
def test_kernels_equal_the_host_functions(gpu, sky, wh, edit):
    old, new, pair, edited = tm.edits()[edit]
    got, ids = _parity(gpu, sky, old, new, rm.camera_pairs(*wh)[pair], WALKS)
    reused = (got[:, 3] > 0).mean()
    assert 0.05 <= reused <= 0.95, reused
    if edit in tm.DROPPED:
        mine = ids == tm.DROPPED[edit]
        assert mine.any() and (got[mine] == 0).all()
    elif edit != "zero_radius_old":
        assert all((got[ids == k, 3] > 0).any() for k in edited)


@pytest.mark.parametrize("max_history,plane_tol", tm.SETTINGS)
def test_kernels_equal_the_host_functions_at_other_settings(gpu, sky, max_history, plane_tol):
    old, new, pair, _ = tm.edits()["two_sideways"]
    _parity(gpu, sky, old, new, rm.camera_pairs(64, 48)[pair], ["ordered"], settings=(max_history, plane_tol))


def _s1000_moved(n_moved=50, seed=5):
    """scene_s1000 with 50 random objects (never the floor) translated and resized a little."""
    old = scenes.scene_s1000(n=1000)
    new = np.array(old, copy=True)
    rng = np.random.default_rng(seed)
    for k in rng.choice(np.arange(1, len(old)), size=n_moved, replace=False):
        new[k]["center"] = np.asarray(old[k]["center"], np.float32) + rng.uniform(-3, 3, 3).astype(np.float32)
        new[k]["radius"] = np.float32(old[k]["radius"]) * np.float32(rng.uniform(0.8, 1.25))
    return old, new


def test_kernels_equal_the_host_functions_on_s1000_with_50_objects_moved(gpu, sky):
    """Many ids per wave: the motion-table gather."""
    old, new = _s1000_moved()
    cam0 = gm.fixtures()["s1000_96x64"][1]
    c1 = cam0.copy()
    c1["origin"] = np.asarray(cam0["origin"], np.float32) + np.array([6.0, 2.0, -6.0], np.float32)
    c1["look_at"] = np.asarray(cam0["look_at"], np.float32) + np.array([3.0, 0.0, -3.0], np.float32)
    got, ids = _parity(gpu, sky, old, new, (cam0, c1), ["ordered"])
    moved = np.isin(ids, _changed(old, new))
    assert moved.sum() >= 20 and (got[moved, 3] > 0).any()
    assert 0.05 <= (got[:, 3] > 0).mean() <= 0.95


def test_kernels_equal_the_host_functions_after_a_rebuild(gpu, sky):
    """cpt_update_objects_rebuild keeps the captured history: with a sphere that became a platform
    (the edit that forces a rebuild; its record is DROP) the cylinder moved in the same batch is
    followed."""
    old, new, pair, _ = tm.edits()["cylinder_all"]
    new = tm._edit(new, tm.MIRROR, type=PLATFORM, y_pos=-5.0)   # under the floor: the sphere is gone from view
    assert object_motion_host(old, new)["kind"][tm.MIRROR] == MOTION_DROP
    got, ids = _parity(gpu, sky, old, new, rm.camera_pairs(64, 48)[pair], ["ordered"], rebuild=True)
    assert not (ids == tm.MIRROR).any()
    assert (got[ids == tm.CYL, 3] > 0).any()


# ----------------------------------------------------------------- no edit: the untracked calls
@pytest.mark.parametrize("pair", ["sideways", "look_at", "identical"])
@pytest.mark.parametrize("wh", [(64, 48), (67, 41)], ids=lambda wh: "%dx%d" % wh)
def test_without_an_edit_the_tracked_calls_are_the_untracked_ones(gpu, sky, wh, pair):
    W, H = wh
    c0, c1 = (camera_get_copy(c) for c in rm.camera_pairs(W, H)[pair])
    flags = CPT_TRAVERSAL_ORDERED
    gpu.set_scene(tm.scene())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    out = {}
    for arm in ("tracked", "untracked"):
        gpu.init_rng(scenes.DEFAULT_SEED)
        gpu.reset_display() if out else None
        gpu.clear_accum()
        gpu.render(c0, 3, DEPTH, sync=True, ordered=True)
        _display_passes(gpu, c0)
        if arm == "tracked":
            gpu.history_capture(c0, flags)
            gpu.reproject_accum_tracked(c1, flags=flags)
            acc, g = gpu.read_accum(), gpu.read_gbuffer()
            gpu.history_capture(c0, flags)
            gpu.reproject_display_tracked(c1, flags=flags)
        else:
            gpu.reproject_accum(c0, c1, flags=flags)
            acc, g = gpu.read_accum(), gpu.read_gbuffer()
            gpu.reproject_display(c0, c1, flags=flags)
        out[arm] = [acc, *(g[k] for k in sorted(g)), gpu.read_mix(), gpu.read_display_count(),
                    *(gpu.read_gbuffer()[k] for k in sorted(g))]
    for a, b in zip(out["tracked"], out["untracked"]):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    if pair != "identical":
        assert 0.05 <= (out["tracked"][0][:, 3] > 0).mean() < 1.0


def test_an_untracked_call_drops_the_captured_history(gpu, sky):
    """cpt_reproject_accum and cpt_reproject_display trace their `from` into the history's planes:
    the capture is gone (history_info), a tracked call behind them is CPT_ERR_STATE and writes
    nothing, and capturing again gives the tracked call its result back."""
    W, H = 64, 48
    c0, c1 = (camera_get_copy(c) for c in rm.camera_pairs(W, H)["sideways"])
    c2 = camera_get_copy(rm.camera_pairs(W, H)["dolly_in"][1])
    d1, d2 = gm.camera_rays(c1)[1], gm.camera_rays(c2)[1]
    flags = CPT_TRAVERSAL_ORDERED
    gpu.set_scene(tm.scene())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED)
    _display_passes(gpu, c0, 1)
    for untracked in (gpu.reproject_accum, gpu.reproject_display):
        gpu.history_capture(c0, flags)
        assert gpu.history_info()[0]
        untracked(c0, c1, flags=flags)      # the history planes now hold c0's G-buffer by this call's doing
        assert gpu.history_info() == (False, None)
        acc, mix, cnt, g1 = gpu.read_accum(), gpu.read_mix(), gpu.read_display_count(), gpu.read_gbuffer()
        for tracked in (gpu.reproject_accum_tracked, gpu.reproject_display_tracked):
            _raises(STATE, lambda: tracked(c2, flags=flags))
        for a, b in zip((acc, mix, cnt, *g1.values()), (gpu.read_accum(), gpu.read_mix(), gpu.read_display_count(),
                                                        *gpu.read_gbuffer().values())):
            np.testing.assert_array_equal(_bits(a), _bits(b))
    # a new capture at the camera the accumulator now stands at, and the tracked call is right again
    hist = rm.history(g1["id"], W, H)
    gpu.write_accum(hist)
    gpu.history_capture(c1, flags)
    gpu.reproject_accum_tracked(c2, flags=flags)
    g2 = gpu.read_gbuffer()
    want = reproject_tracked_host(c1, c2, d1, d2, g1["id"], g1["t"], g2["id"], g2["t"], g2["normal"], hist, None)
    np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(want))


# ------------------------------------------------------------------------------------- chain
def test_a_chain_of_tracked_calls_renews_the_history(gpu, sky):
    """capture at C0, tracked to C1, an edit, tracked to C2: the host function applied twice, the
    second time from C1's planes and the objects as they were at the first call."""
    W, H = 64, 48
    pairs = rm.camera_pairs(W, H)
    c0, c1 = (camera_get_copy(c) for c in pairs["sideways"])
    c2 = camera_get_copy(pairs["dolly_in"][1])
    d0, d1, d2 = (gm.camera_rays(c)[1] for c in (c0, c1, c2))
    old, new, _, _ = tm.edits()["two_sideways"]
    idx = _changed(old, new)
    flags = CPT_TRAVERSAL_ORDERED
    gpu.set_scene(old)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.history_capture(c0, flags)
    g0 = gpu.read_gbuffer()
    hist = rm.history(g0["id"], W, H)
    gpu.write_accum(hist)
    gpu.reproject_accum_tracked(c1, flags=flags)
    middle = gpu.last_reproject_ms(split=True)
    assert middle[0] == 0.0 and middle[1] > 0.0
    g1, a1 = gpu.read_gbuffer(), gpu.read_accum()
    want1 = reproject_tracked_host(c0, c1, d0, d1, g0["id"], g0["t"], g1["id"], g1["t"], g1["normal"], hist, None)
    np.testing.assert_array_equal(_bits(a1), _bits(want1))
    gpu.update_objects(idx, new[idx])
    gpu.reproject_accum_tracked(c2, flags=flags)
    g2, a2 = gpu.read_gbuffer(), gpu.read_accum()
    want2 = reproject_tracked_host(c1, c2, d1, d2, g1["id"], g1["t"], g2["id"], g2["t"], g2["normal"], want1,
                                   object_motion_host(old, new))
    np.testing.assert_array_equal(_bits(a2), _bits(want2))
    assert 0.05 <= (a2[:, 3] > 0).mean() < 1.0
    # and a third call with no further edit needs no table: the snapshot is the edited scene
    gpu.reproject_accum_tracked(c1, flags=flags)
    g3 = gpu.read_gbuffer()
    want3 = reproject_tracked_host(c2, c1, d2, d1, g2["id"], g2["t"], g3["id"], g3["t"], g3["normal"], want2, None)
    np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(want3))


# ------------------------------------------------------------------------------ side effects
def test_tracked_calls_leave_the_rest_of_the_frame_alone(gpu, sky):
    W, H = 64, 48
    c0, c1 = (camera_get_copy(c) for c in rm.camera_pairs(W, H)["sideways"])
    old, new, _, _ = tm.edits()["sphere_moved"]
    idx = _changed(old, new)
    flags = CPT_TRAVERSAL_ORDERED
    gpu.set_scene(old)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED)
    gpu.render_adaptive(c0, 8, 32, 4, 0.1, 8, flags=CPT_RENDER_AUX | CPT_TRAVERSAL_ORDERED)
    gpu.filter_frame()
    gpu.denoise_mix_history()

    def rest():
        return [gpu.read_rng(), *gpu.read_aux(), *gpu.read_filtered()]
    before, accum, mix, cnt, moments = rest(), gpu.read_accum(), gpu.read_mix(), gpu.read_display_count(), gpu.read_moments()
    # the capture writes the G-buffer and the history, nothing else
    gpu.history_capture(c0, flags)
    for a, b in zip(before + [accum, mix, cnt, moments], rest() + [gpu.read_accum(), gpu.read_mix(), gpu.read_display_count(),
                                                                  gpu.read_moments()]):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    gpu.update_objects(idx, new[idx])
    # the display variant: the accumulator and the moments stay
    gpu.reproject_display_tracked(c1, flags=flags)
    for a, b in zip(before + [accum, moments], rest() + [gpu.read_accum(), gpu.read_moments()]):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert gpu.read_mix().tobytes() != mix.tobytes()
    mix, cnt = gpu.read_mix(), gpu.read_display_count()
    # the accumulator variant: the display state stays, the adaptive result goes
    gpu.reproject_accum_tracked(c0, flags=flags)
    for a, b in zip(before + [mix, cnt], rest() + [gpu.read_mix(), gpu.read_display_count()]):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert gpu.read_accum().tobytes() != accum.tobytes()
    for call in (gpu.read_noise, gpu.read_moments, gpu.filter_frame):
        _raises(STATE, call)


# ------------------------------------------------------------------------------------ errors
def _raises(status, call):
    with pytest.raises(CptError) as e:
        call()
    assert e.value.status == status, e.value


def test_errors_write_nothing(gpu, sky):
    W, H = 64, 48
    c0, c1 = (camera_get_copy(c) for c in rm.camera_pairs(W, H)["sideways"])
    small = camera_get_copy(rm.camera_pairs(16, 16)["sideways"][1])
    hist = np.random.default_rng(3).random((W * H, 4), dtype=np.float32) + np.float32(1.0)
    objs = tm.scene()
    calls = lambda r: (lambda **kw: r.reproject_accum_tracked(c1, **kw), lambda **kw: r.reproject_display_tracked(c1, **kw))

    r = Renderer(0)
    try:
        _raises(STATE, lambda: r.history_capture(c0))               # no scene, no frame
        r.set_frame(W, H)
        _raises(STATE, lambda: r.history_capture(c0))               # no scene
        assert r.history_info() == (False, None)
    finally:
        r.close()

    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED)
    gpu.write_accum(hist)

    def unchanged():
        np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(hist))
    # no capture
    assert gpu.history_info() == (False, None)
    _raises(STATE, lambda: gpu.reproject_accum_tracked(c1))
    unchanged()
    _raises(STATE, gpu.read_gbuffer)
    # the display variant without a display pass, with and without a capture
    _raises(STATE, lambda: gpu.reproject_display_tracked(c1))
    gpu.history_capture(c0)
    assert gpu.history_info()[0]
    _raises(STATE, lambda: gpu.reproject_display_tracked(c1))
    # a capture dropped by set_scene and by set_frame
    gpu.set_scene(objs)
    assert not gpu.history_info()[0]
    _raises(STATE, lambda: gpu.reproject_accum_tracked(c1))
    unchanged()
    gpu.history_capture(c0)
    gpu.set_frame(W, H)
    assert not gpu.history_info()[0]
    gpu.init_rng(scenes.DEFAULT_SEED)
    gpu.write_accum(hist)
    _raises(STATE, lambda: gpu.reproject_accum_tracked(c1))
    unchanged()

    # bad arguments, with a capture and a display pass in place
    gpu.render(c0, 1, DEPTH, aux=True, sync=True, ordered=True)
    gpu.denoise_mix_history()
    gpu.write_accum(hist)
    gpu.history_capture(c0)
    g0 = gpu.read_gbuffer()
    mix, cnt = gpu.read_mix(), gpu.read_display_count()
    L, ctx = gpu._L, gpu._ctx
    bad = [lambda: gpu._check(L.cpt_history_capture(ctx, None, 0)), lambda: gpu.history_capture(small),
           lambda: gpu.history_capture(c0, flags=CPT_RENDER_AUX)]
    for fn, call in zip((L.cpt_reproject_accum_tracked, L.cpt_reproject_display_tracked), calls(gpu)):
        bad += [lambda fn=fn: gpu._check(fn(ctx, None, 32, ctypes.c_float(1e-2), 0)),
                lambda fn=fn: gpu._check(fn(ctx, ctypes.c_void_p(np.ascontiguousarray(small).ctypes.data), 32, ctypes.c_float(1e-2), 0)),
                lambda call=call: call(max_history=0), lambda call=call: call(max_history=-3),
                lambda call=call: call(plane_tol=-1e-3), lambda call=call: call(plane_tol=float("nan")),
                lambda call=call: call(plane_tol=float("inf")), lambda call=call: call(flags=CPT_RENDER_AUX),
                lambda call=call: call(flags=CPT_TRAVERSAL_ORDERED | 0x1)]
    for call in bad:
        _raises(INVALID, call)
        unchanged()
        np.testing.assert_array_equal(_bits(gpu.read_mix()), _bits(mix))
        np.testing.assert_array_equal(_bits(gpu.read_display_count()), _bits(cnt))
        after = gpu.read_gbuffer()   # still the capture's
        assert all(after[k].tobytes() == g0[k].tobytes() for k in g0)
        valid, cam = gpu.history_info()
        assert valid and cam.tobytes() == np.ascontiguousarray(c0).tobytes()

    # an adaptive render pending
    gpu.adaptive_begin(c0, 4, 8, 2, 0.0, 4, flags=CPT_TRAVERSAL_ORDERED)
    for call in (lambda: gpu.history_capture(c0), *calls(gpu)):
        _raises(STATE, call)
    while gpu.adaptive_step():
        pass
    # the display holds a band
    gpu.denoise_mix_band(1, 0, 16)
    _raises(STATE, lambda: gpu.reproject_display_tracked(c1))
    gpu.reproject_accum_tracked(c1)   # and the accumulator variant works
    gpu.synchronize()

    # frames that are not full
    for rows in ([5, 2, 40], list(range(24))):
        gpu.set_frame(W, H, rows)
        part = hist[:len(rows) * W]
        gpu.write_accum(part)
        for call in (lambda: gpu.history_capture(c0), *calls(gpu)):
            _raises(STATE, call)
        np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(part))


# ---------------------------------------------------------------------------------- ordering
def _second_camera():
    c = scenes.camera_for(ao.W, ao.H)
    c["origin"] = np.asarray(c["origin"], np.float32) + np.array([5.0, 0.0, -5.0], np.float32)
    return camera_get_copy(c)


def _capture_tracked_render(r, e):
    r.history_capture(e.cam, flags=ao.WALK)
    r.reproject_accum_tracked(e.cam2, flags=ao.WALK)
    r.render(e.cam2, 32, ao.DEPTH, accumulate=True, **ao.KW)


def _capture_and_edit(r, e):
    """Before the render in flight: the capture, then twenty objects moved (cpt_update_objects waits,
    so the edit cannot itself stand behind a render)."""
    r.history_capture(e.cam, flags=ao.WALK)
    moved = np.array(e.objs[1:21], copy=True)
    moved["center"][:, 0] += np.float32(1.5)
    r.update_objects(np.arange(1, 21), moved)


def _tracked_render(r, e):
    r.reproject_accum_tracked(e.cam2, flags=ao.WALK)
    r.render(e.cam2, 32, ao.DEPTH, accumulate=True, **ao.KW)


ORDER_CASES = [
    ao.Case("capture-tracked-render", _capture_tracked_render, ao.IMAGE + ("gbuffer",), rerecords=True),
    # an edited call: the motion table's upload, its event and the planes' ping-pong are in the queue
    ao.Case("edit-tracked-render", _tracked_render, ao.IMAGE + ("gbuffer",), before=_capture_and_edit, rerecords=True,
            pinned=False),
]


@pytest.mark.parametrize("case", ORDER_CASES, ids=lambda c: c.name)
def test_tracked_reproject_behind_a_render_in_flight(shared, case):
    """cpt_history_capture and cpt_reproject_accum_tracked queued behind an unsynchronised
    cpt_render, and a cpt_render queued behind them, give the bytes of the sequence synchronised
    after every call; so does a tracked call that uploads a motion table."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    e = SimpleNamespace(**vars(shared), cam2=_second_camera())
    want, _, first = ao._run(case, e, twin=True)
    got, (t_launch, t_call, _), _ = ao._run(case, e, twin=False)
    ao.assert_overlap(case.name, t_launch, t_call, first[2])
    ao._assert_same_bits(got, want)
    reused = (want["accum"].view(np.float32).reshape(-1, 4)[:, 3] > 32).mean()
    assert reused >= 0.25, "the reprojection kept no history: a vacuous case"


# -------------------------------------------------------------------------------- end to end
E2E_MOVE = (4.0, 0.0, 6.0)   # the Metal sphere's translation, world units


@pytest.fixture(scope="module")
def e2e(gpu, sky):
    """S4 + cylinder, 64x48, depth 8.  32 passes, then the Metal sphere moves, then 4 passes, three
    ways from the same RNG states: tracked (capture, edit, reproject_accum_tracked), restart (clear)
    and stale (reproject_accum(cam, cam) after the edit: today's only alternative to clearing).
    Truth: 1024 passes of the edited scene.  Per pixel: the squared error of each mean (averaged
    over rgb), the ids before and after."""
    from test_gpu_reproject import e2e_cameras
    W, H, D8 = 64, 48, 8
    cam = e2e_cameras(W, H)[0]
    old = tm.scene()
    c = np.asarray(old[tm.METAL]["center"], np.float32)
    new = tm._edit(old, tm.METAL, center=tuple(c + np.asarray(E2E_MOVE, np.float32)))
    flags = CPT_TRAVERSAL_ORDERED
    kw = dict(ordered=True, sync=True)
    gpu.set_scene(new)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED + 1)
    gpu.render(cam, 1024, D8, **kw)
    truth = gpu.read_accum()
    truth = truth[:, :3].astype(np.float64) / truth[:, 3:4]
    gpu.update_objects([tm.METAL], old[[tm.METAL]])
    gpu.init_rng(scenes.DEFAULT_SEED)
    gpu.clear_accum()
    gpu.render(cam, 32, D8, **kw)
    a32, states = gpu.read_accum(), gpu.read_rng()
    gpu.history_capture(cam, flags)
    id0 = gpu.read_gbuffer()["id"]
    gpu.update_objects([tm.METAL], new[[tm.METAL]])
    arms = {}
    gpu.reproject_accum_tracked(cam, flags=flags)
    id1 = gpu.read_gbuffer()["id"]
    gpu.render(cam, 4, D8, accumulate=True, **kw)
    arms["tracked"] = gpu.read_accum()
    gpu.write_rng(states)
    gpu.clear_accum()
    gpu.render(cam, 4, D8, accumulate=True, **kw)
    arms["restart"] = gpu.read_accum()
    gpu.write_rng(states)
    gpu.write_accum(a32)
    gpu.reproject_accum(cam, cam, flags=flags)
    gpu.render(cam, 4, D8, accumulate=True, **kw)
    arms["stale"] = gpu.read_accum()

    def err(accum):
        mean = accum[:, :3] / accum[:, 3:4]
        return ((mean.astype(np.float64) - truth) ** 2).mean(axis=1)
    errs = {k: err(v) for k, v in arms.items()}
    union = (id0 == tm.METAL) | (id1 == tm.METAL)
    # the floor away from both footprints: not within two pixels of either
    near = union.reshape(H, W).copy()
    for _ in range(2):
        grown = near.copy()
        grown[1:] |= near[:-1]
        grown[:-1] |= near[1:]
        grown[:, 1:] |= near[:, :-1]
        grown[:, :-1] |= near[:, 1:]
        near = grown
    far_floor = (id0 == tm.FLOOR) & (id1 == tm.FLOOR) & ~near.reshape(-1)
    for name, m in (("frame", np.ones(W * H, bool)), ("union of the sphere's footprints", union), ("floor away from them", far_floor)):
        print("%s: %d pixels, MSE tracked %.6g, restart %.6g, stale %.6g" %
              (name, m.sum(), *(errs[k][m].mean() for k in ("tracked", "restart", "stale"))))
    return arms, errs, union, far_floor


def test_tracked_history_beats_restart_and_stale(e2e):
    """Whole frame: tracked MSE below the restart's.  Union of the sphere's old and new footprints:
    tracked MSE below the stale history's.  Floor away from both footprints: tracked and stale are
    the same bits (both keep the pixel's own history).  The fixture prints the device's figures
    (DESIGN.md §23)."""
    arms, errs, union, far_floor = e2e
    assert union.sum() >= 100 and far_floor.sum() >= 1000
    assert errs["tracked"].mean() < errs["restart"].mean()
    assert errs["tracked"][union].mean() < errs["stale"][union].mean()
    np.testing.assert_array_equal(_bits(arms["tracked"][far_floor]), _bits(arms["stale"][far_floor]))
    assert (arms["tracked"][far_floor, 3] == 36).all()


# ----------------------------------------------------------------------------------- C++ API
LOOP_STEP = 6.0   # --animate-step of the loop tests: more than a pixel of the 48x32 frame (4.7 world units)


def _headless(tmp_path, name, *args, kind="--bgra"):
    import subprocess
    from cpppathtracer_amd import build
    out = tmp_path / name
    r = subprocess.run([build.build_examples(), "--scene", "s4", "--width", "48", "--height", "32", "--depth", "4", "--seed",
                        str(scenes.DEFAULT_SEED), *args, kind, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def _loop_in_python(gpu, sky, mode, N=2, K=2, A=2, step=LOOP_STEP):
    """The DispatchRay loop of cpt_headless --orbit N --spp K --animate A --display-reproject `mode`
    through the Python wrapper: K passes at each of N orbit cameras (a Refresh after each move), then
    A frames of K passes at the last camera with object 1 moved by +step in x before each.  `on`:
    reproject_display after a Refresh, nothing after an edit (the stale mean goes on).  `edits`:
    reproject_display_tracked after either, the history captured before the first of them."""
    from test_gpu_reproject import orbit_cameras
    W, H = 48, 32
    cams = orbit_cameras(W, H, N)
    objs = scenes.scene_s4()
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED)
    want, captured = None, False
    for f in range(N + A):
        cam = cams[min(f, N - 1)]
        for p in range(K):
            if f and p == 0:
                if mode == "edits" and not captured:
                    gpu.history_capture(cams[f - 1], CPT_TRAVERSAL_ORDERED)
                    captured = True
                if f >= N:
                    objs[1]["center"][0] += np.float32(step)
                    gpu.update_objects([1], objs[[1]])
                if mode == "edits":
                    gpu.reproject_display_tracked(cam, flags=CPT_TRAVERSAL_ORDERED)
                elif f < N:
                    gpu.reproject_display(cams[f - 1], cam, flags=CPT_TRAVERSAL_ORDERED)
            gpu.render(cam, 1, 4, aux=True, sync=True, ordered=True, schedule="previous")
            want = gpu.denoise_mix(2) if (f, p) == (0, 0) else gpu.denoise_mix_history()
    return want, gpu.read_display_count()


def test_headless_loop_through_edits_equals_the_python_sequence(gpu, sky, tmp_path):
    """SetDisplayReprojection(on, 32, 1e-2, through_edits = true): the loop's last BGRA8 frame after
    a camera move and two object edits is the Python sequence's, byte for byte; the edited passes
    kept history (counts above the passes since the last edit) and restarted where there is none
    (the sphere moves by more than a pixel per frame)."""
    got = np.fromfile(_headless(tmp_path, "edits.bgra", "--orbit", "2", "--spp", "2", "--animate", "2", "--animate-step", str(LOOP_STEP),
                                "--display-reproject", "edits"),
                      dtype=np.uint8)
    want, cnt = _loop_in_python(gpu, sky, "edits")
    # history kept through the edits, and restarted where the moved sphere uncovered the floor
    assert (cnt > 2).mean() > 0.5 and (cnt == 2).any()
    assert got.tobytes() == want.tobytes()


def test_headless_loop_with_through_edits_off_is_todays(gpu, sky, tmp_path):
    """through_edits off (the default) through the same edited scene: today's loop, which moves the
    mean after a Refresh only and lets it run on, stale, through an edit; and not the frames of
    through_edits on."""
    args = ("--orbit", "2", "--spp", "2", "--animate", "2", "--animate-step", str(LOOP_STEP), "--display-reproject")
    on = np.fromfile(_headless(tmp_path, "on.bgra", *args, "on"), dtype=np.uint8)
    edits = np.fromfile(_headless(tmp_path, "edits.bgra", *args, "edits"), dtype=np.uint8)
    want, cnt = _loop_in_python(gpu, sky, "on")
    assert (cnt == 9).mean() > 0.5   # no pass restarted anything after the edits
    assert on.tobytes() == want.tobytes()
    assert on.tobytes() != edits.tobytes()


def test_headless_animate_reproject_equals_the_python_sequence(gpu, sky, tmp_path):
    """cpt_headless --animate 2 --reproject (PathTracer::CaptureHistory, then ReprojectTracked after
    each frame's UpdateObjects, the frames added to one accumulator) writes the PFM the same calls
    give through the Python wrapper, bit for bit."""
    from test_gpu_reproject import orbit_cameras
    W, H, SPP = 48, 32, 2
    out = _headless(tmp_path, "animate.pfm", "--spp", str(SPP), "--animate", "2", "--reproject", kind="--pfm")
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF"
        assert tuple(int(v) for v in f.readline().split()) == (W, H)
        assert float(f.readline()) < 0
        pfm = np.frombuffer(f.read(), dtype="<f4").reshape(H, W, 3)[::-1].reshape(-1, 3)
    cam = orbit_cameras(W, H, 1)[0]
    objs = scenes.scene_s4()
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED)
    gpu.render(cam, SPP, 4, sync=True, ordered=True)
    gpu.history_capture(cam, CPT_TRAVERSAL_ORDERED)
    for _ in range(2):
        objs[1]["center"][0] += np.float32(0.75)
        gpu.update_objects([1], objs[[1]])
        gpu.reproject_accum_tracked(cam, flags=CPT_TRAVERSAL_ORDERED)
        gpu.render(cam, SPP, 4, accumulate=True, sync=True, ordered=True)
    acc = gpu.read_accum()
    assert (acc[:, 3] == 3 * SPP).mean() > 0.5   # history kept through both edits (the moves are below a pixel)
    want = (acc[:, :3] / acc[:, 3:4]).astype(np.float32)
    np.testing.assert_array_equal(_bits(pfm), _bits(want))
