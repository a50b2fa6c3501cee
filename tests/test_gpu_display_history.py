"""The display's per-pixel history on the GPU: cpt_denoise_mix_history against
cpt_denoise_mix bit for bit, the switch between the two, cpt_reproject_display's kernel against
cpt_reproject_display_host (itself held to the numpy restatement by test_display_history_model.py),
what the call must leave alone, its error codes, its place in the stream's order, the DispatchRay
loop with PathTracer::SetDisplayReprojection, and the point of it all: after a camera step the
reprojected running mean is closer to the truth than a restarted one at equal new passes.
"""
import ctypes
import subprocess
from types import SimpleNamespace

import gbuffer_model as gm
import numpy as np
import pytest
import reproject_model as rm
import test_gpu_async_order as ao
import test_gpu_reproject as tr

from cpppathtracer_amd import CptError, Renderer, camera_get_copy, scenes
from cpppathtracer_amd._lib import CPT_RENDER_AUX, CPT_TRAVERSAL_ORDERED

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 5
DEPTH = 8
shared = ao.shared   # the ordering tests' workload (a module fixture of test_gpu_async_order.py)
_bits = tr._bits


def _region(W, H):
    """(W', H', mask over the H' x W rows the display band holds)."""
    We, He = 16 * (W // 16), 16 * (H // 16)
    return We, He, np.tile(np.arange(W) < We, He)


def _setup(r, W, H, sky, objs=None, seed=scenes.DEFAULT_SEED):
    r.set_scene(scenes.scene_s4() if objs is None else objs)
    r.set_env(sky)
    r.set_frame(W, H)
    r.init_rng(seed)


def _pass(r, cam, **kw):
    """One display pass's render: a fresh sample per pixel with the first-hit normals."""
    r.render(cam, 1, DEPTH, aux=True, sync=True, ordered=True, **kw)


@pytest.fixture(scope="module")
def twin():
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    r = Renderer(0)
    yield r
    r.close()


# --------------------------------------------------------------------------- Mix equivalence
@pytest.mark.parametrize("wh", [(64, 48), (80, 32), (67, 41), (16, 16), (1920, 304)], ids=lambda wh: "%dx%d" % wh)
def test_history_passes_equal_the_global_index_passes(gpu, twin, sky, wh):
    """From a reset display, k calls of denoise_mix_history give the mix plane and the BGRA bytes of
    denoise_mix(1..k), after every pass; the counts are k inside W' x H' and 0 outside.  80x32: two
    60-column strips; 67x41: unaligned; 1920x304: a block owns 19 rows, three super-steps of 8 waves,
    where the ring wraps.  Pass 3 writes a pinned host frame."""
    import torch
    W, H = wh
    We, He, inside = _region(W, H)
    cam = camera_get_copy(scenes.camera_for(W, H))
    for r in (gpu, twin):
        _setup(r, W, H, sky)
    pinned = torch.full((H, W, 4), 0xAB, dtype=torch.uint8).pin_memory().numpy()
    for k in range(1, 6):
        for r in (gpu, twin):
            _pass(r, cam)
        got = gpu.denoise_mix_history(out=pinned if k == 3 else None)
        want = twin.denoise_mix(k)
        assert got.tobytes() == want.tobytes(), f"pass {k}: BGRA"
        np.testing.assert_array_equal(_bits(gpu.read_mix()), _bits(twin.read_mix()), err_msg=f"pass {k}: mix")
        cnt = gpu.read_display_count()
        assert cnt.shape == (He * W,)
        assert (cnt[inside] == k).all() and (cnt[~inside] == 0).all(), f"pass {k}: counts"
        np.testing.assert_array_equal(twin.read_display_count(), cnt)   # the stale plane reads as the fill leaves it
    assert want.any()


def test_switching_between_the_two_kinds_of_pass(gpu, twin, sky):
    """denoise_mix(1..3) then denoise_mix_history equals denoise_mix(1..4), and back again; the
    counts read as the recorded index in between; reset_display zeroes mean and counts."""
    W, H = 67, 41
    We, He, inside = _region(W, H)
    cam = camera_get_copy(scenes.camera_for(W, H))
    for r in (gpu, twin):
        _setup(r, W, H, sky)

    def both(k, history):
        for r in (gpu, twin):
            _pass(r, cam)
        got = gpu.denoise_mix_history() if history else gpu.denoise_mix(k)
        want = twin.denoise_mix(k)
        assert got.tobytes() == want.tobytes(), k
        np.testing.assert_array_equal(_bits(gpu.read_mix()), _bits(twin.read_mix()), err_msg=str(k))
    for k in (1, 2, 3):
        both(k, False)
    cnt = gpu.read_display_count()
    assert (cnt[inside] == 3).all() and (cnt[~inside] == 0).all()
    both(4, True)
    both(5, True)
    both(6, False)
    both(7, True)
    cnt = gpu.read_display_count()
    assert (cnt[inside] == 7).all() and (cnt[~inside] == 0).all()
    gpu.reset_display()
    assert not gpu.read_display_count().any() and not gpu.read_mix().any()
    twin.reset_display()
    both(1, True)
    assert (gpu.read_display_count()[inside] == 1).all()


# ------------------------------------------------------------------- kernel = host function
def _full(a, npix):
    """The band's rows (H' of them) padded to the frame's: the rows below hold zeros on the device."""
    out = np.zeros((npix,) + a.shape[1:], dtype=np.float32)
    out[:a.shape[0]] = a
    return out


def _display_parity(gpu, sky, objs, pair, walks):
    """Real passes at the first camera, holes made by reprojecting there and back, one more pass;
    then reproject_display against cpt_reproject_display_host on the device's own G-buffer planes
    and the display state read back before the call."""
    from cpppathtracer_amd.renderer import reproject_display_host
    c0, c1 = camera_get_copy(pair[0]), camera_get_copy(pair[1])
    W, H = int(c0["width"]), int(c0["height"])
    We, He, inside = _region(W, H)
    _setup(gpu, W, H, sky, objs)
    d0, d1 = gm.camera_rays(c0)[1], gm.camera_rays(c1)[1]
    reused = None
    for walk in walks:
        flags = tr.WALKS[walk]
        gpu.reset_display()
        for _ in range(3):
            _pass(gpu, c0)
            gpu.denoise_mix_history()
        gpu.reproject_display(c0, c1, flags=flags)
        gpu.reproject_display(c1, c0, flags=flags)
        _pass(gpu, c0)
        gpu.denoise_mix_history()
        mean, cnt = gpu.read_mix(), gpu.read_display_count()
        assert (cnt[~inside] == 0).all() and (cnt[inside] >= 1).all()
        assert (cnt == 1).any() and (cnt > 1).any(), "no holes in the written-in state: a weaker case"
        g0, g1 = tr._gbuffer(gpu, c0, flags), tr._gbuffer(gpu, c1, flags)
        want_m, want_n = reproject_display_host(c0, c1, d0, d1, g0["id"], g0["t"], g1["id"], g1["t"], g1["normal"],
                                                _full(mean, W * H), _full(cnt, W * H))
        assert not want_n[He * W:].any() and not want_m[He * W:].any()
        gpu.reproject_display(c0, c1, flags=flags)
        np.testing.assert_array_equal(_bits(gpu.read_display_count()), _bits(want_n[:He * W]), err_msg=walk)
        np.testing.assert_array_equal(_bits(gpu.read_mix()), _bits(want_m[:He * W]), err_msg=walk)
        after = gpu.read_gbuffer()
        for k in g1:
            np.testing.assert_array_equal(_bits(after[k]), _bits(g1[k]), err_msg=f"{walk}: read_gbuffer {k} is not the new camera's")
        assert gpu.last_reproject_ms() > 0.0 and len(gpu.last_reproject_ms(split=True)) == 3
        reused = (want_n[:He * W][inside] > 0).mean()
        # neither an all-zero nor an all-reused frame.  Every pixel of this state holds samples (the
        # synthetic state of the CPU tests has empty blocks; this one only single-sample holes), so
        # what is rejected is disocclusions and the frame's new border alone: 1% of the region, 20
        # pixels of the smallest one, is asked for
        assert 0.05 <= reused <= 0.99, reused
    return reused


@pytest.mark.parametrize("wh", [(64, 48), (67, 41)], ids=lambda wh: "%dx%d" % wh)
def test_kernel_equals_the_host_function(gpu, sky, wh):
    _display_parity(gpu, sky, scenes.scene_s4(), rm.camera_pairs(*wh)["sideways"], tr.WALKS)


def test_kernel_equals_the_host_function_on_s1000(gpu, sky):
    objs, cam0, _ = gm.fixtures()["s1000_96x64"]
    _display_parity(gpu, sky, objs, tr._nudged(cam0), ["ordered"])
    assert 0 < gpu.walk_info()["n_wide"] <= 512


def test_identical_cameras_leave_the_display_state(gpu, sky):
    W, H = 64, 48
    cam = camera_get_copy(scenes.camera_for(W, H))
    _setup(gpu, W, H, sky)
    for _ in range(3):
        _pass(gpu, cam)
        gpu.denoise_mix_history()
    mean, cnt = gpu.read_mix(), gpu.read_display_count()
    gpu.reproject_display(cam, cam, flags=CPT_TRAVERSAL_ORDERED)
    np.testing.assert_array_equal(_bits(gpu.read_mix()), _bits(mean))
    np.testing.assert_array_equal(_bits(gpu.read_display_count()), _bits(cnt))


# ------------------------------------------------------------------------------ side effects
def _bgra_on_device(gpu, nbytes):
    import torch
    buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    gpu.copy_bgra_device(buf.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def test_reproject_display_leaves_the_rest_of_the_frame_alone(gpu, sky):
    """After an adaptive render, filter_frame and display passes: the call changes the display's mean
    and counts and the G-buffer, and none of the accumulator, the RNG planes, the aux buffers, the
    moments, the filtered planes and the BGRA frame."""
    W, H = 64, 48
    c0, c1 = (camera_get_copy(c) for c in rm.camera_pairs(W, H)["sideways"])
    _setup(gpu, W, H, sky)
    gpu.render_adaptive(c0, 8, 32, 4, 0.1, 8, flags=CPT_RENDER_AUX | CPT_TRAVERSAL_ORDERED)
    gpu.filter_frame()
    gpu.denoise_mix_history()
    gpu.denoise_mix_history()

    def state():
        return [gpu.read_accum(), gpu.read_rng(), *gpu.read_aux(), gpu.read_moments(), *gpu.read_filtered(),
                _bgra_on_device(gpu, 48 * W * 4)]
    before, mean, cnt = state(), gpu.read_mix(), gpu.read_display_count()
    assert before[-1].any()
    want = tr._gbuffer(gpu, c1, CPT_TRAVERSAL_ORDERED)
    gpu.gbuffer(c0, CPT_TRAVERSAL_ORDERED)
    gpu.reproject_display(c0, c1, flags=CPT_TRAVERSAL_ORDERED)
    for a, b in zip(before, state()):
        np.testing.assert_array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b)
    got = gpu.read_gbuffer()
    for k in want:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=k)
    assert gpu.read_mix().tobytes() != mean.tobytes() and gpu.read_display_count().tobytes() != cnt.tobytes()
    gpu.read_noise()   # the adaptive result is still there


# ------------------------------------------------------------------------------------ errors
def test_errors_leave_the_display_state(gpu, sky):
    W, H = 64, 48
    c0, c1 = (camera_get_copy(c) for c in rm.camera_pairs(W, H)["sideways"])
    small = camera_get_copy(rm.camera_pairs(16, 16)["sideways"][1])
    r = Renderer(0)
    try:
        tr._raises(STATE, lambda: r.reproject_display(c0, c1))          # no scene, no frame
        r.set_frame(W, H)
        tr._raises(STATE, lambda: r.reproject_display(c0, c1))          # no scene
    finally:
        r.close()
    _setup(gpu, W, H, sky)
    for rows in ([5, 2, 40], list(range(24))):                            # frames that are not full
        gpu.set_frame(W, H, rows)
        tr._raises(STATE, lambda: gpu.reproject_display(c0, c1))
    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED)
    _pass(gpu, c0)
    tr._raises(STATE, lambda: gpu.reproject_display(c0, c1))            # no display pass yet
    tr._raises(STATE, gpu.read_gbuffer)                                   # ... and nothing was traced

    def state():
        return gpu.read_mix(), gpu.read_display_count(), gpu.display_band()
    gpu.denoise_mix_band(1, 0, 16)
    before = state()
    tr._raises(STATE, lambda: gpu.reproject_display(c0, c1))            # the display holds a band
    for a, b in zip(before, state()):
        np.testing.assert_array_equal(a, b)
    gpu.denoise_mix_history()
    _pass(gpu, c0)
    gpu.denoise_mix_history()
    before = state()
    assert (before[1] == 2).all()
    L, ctx = gpu._L, gpu._ctx
    p0, p1 = (ctypes.c_void_p(np.ascontiguousarray(c).ctypes.data) for c in (c0, c1))
    bad = [
        lambda: gpu._check(L.cpt_reproject_display(ctx, None, p1, 32, ctypes.c_float(1e-2), 0)),
        lambda: gpu._check(L.cpt_reproject_display(ctx, p0, None, 32, ctypes.c_float(1e-2), 0)),
        lambda: gpu.reproject_display(small, c1),
        lambda: gpu.reproject_display(c0, small),
        lambda: gpu.reproject_display(c0, c1, max_history=0),
        lambda: gpu.reproject_display(c0, c1, max_history=-3),
        lambda: gpu.reproject_display(c0, c1, plane_tol=-1e-3),
        lambda: gpu.reproject_display(c0, c1, plane_tol=float("nan")),
        lambda: gpu.reproject_display(c0, c1, plane_tol=float("inf")),
        lambda: gpu.reproject_display(c0, c1, flags=CPT_RENDER_AUX),
        lambda: gpu.reproject_display(c0, c1, flags=CPT_TRAVERSAL_ORDERED | 0x1),
    ]
    for call in bad:
        tr._raises(INVALID, call)
        for a, b in zip(before, state()):
            np.testing.assert_array_equal(_bits(a) if isinstance(a, np.ndarray) else a, _bits(b) if isinstance(b, np.ndarray) else b)
    tr._raises(STATE, gpu.read_gbuffer)   # none of the failed calls traced anything
    gpu.adaptive_begin(c0, 4, 8, 2, 0.0, 4, flags=CPT_TRAVERSAL_ORDERED)
    tr._raises(STATE, lambda: gpu.reproject_display(c0, c1))            # an adaptive render pending
    while gpu.adaptive_step():
        pass
    for a, b in zip(before, state()):
        np.testing.assert_array_equal(a, b)
    gpu.reproject_display(c0, c1)   # and works once it has ended
    gpu.synchronize()
    assert gpu.read_display_count().tobytes() != before[1].tobytes()


# ---------------------------------------------------------------------------------- ordering
def _display_twice(r, e):
    for _ in range(2):
        r.render(e.cam, 1, ao.DEPTH, aux=True, sync=True, **ao.KW)
        r.denoise_mix_history()
    r.init_rng(ao.SEED)


def _reproject_then_display(r, e):
    r.reproject_display(e.cam, e.cam2, flags=ao.WALK)
    return r.denoise_mix_history(), r.read_display_count()


def test_reproject_display_behind_a_render_in_flight(shared):
    """cpt_reproject_display queued behind an unsynchronised cpt_render, and a display pass queued
    behind it, give the bytes of the sequence synchronised after every call."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    case = ao.Case("reproject_display-denoise_mix_history", _reproject_then_display, ao.IMAGE + ("aux", "mix", "gbuffer"),
                   render=ao.AUX, before=_display_twice)
    e = SimpleNamespace(**vars(shared), cam2=tr._second_camera())
    want, _, _ = ao._run(case, e, twin=True)
    got, (t_launch, t_call, render_ms), _ = ao._run(case, e, twin=False)
    ao.assert_overlap(case.name, t_launch, t_call, render_ms)
    ao._assert_same_bits(got, want)
    cnt = want["call.1"]
    assert (cnt == 3).mean() >= 0.25 and (cnt == 1).any(), "the reprojection kept no history, or all of it: a vacuous case"


# -------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def e2e(gpu, sky):
    """S4, 64x48, depth 8, the reference's default lens.  32 display passes at C0, the display state
    reprojected to C1 (a sideways step of (4, 0, -4)), 4 passes there, against a restart: 4 passes at
    C1 from the same RNG states.  Truth: the mean of 1024 display passes at C1.  Per pixel of
    W' x H' (here the frame): the squared error of both means (averaged over rgb) and the object."""
    W, H = 64, 48
    c0, c1 = tr.e2e_cameras(W, H)

    def passes(cam, n):
        for _ in range(n):
            _pass(gpu, cam)
            gpu.denoise_mix_history(host=False)
    _setup(gpu, W, H, sky, seed=scenes.DEFAULT_SEED + 1)
    passes(c1, 1024)
    truth = gpu.read_mix().astype(np.float64)
    assert (gpu.read_display_count() == 1024).all()
    gpu.init_rng(scenes.DEFAULT_SEED)
    gpu.reset_display()
    passes(c0, 32)
    states = gpu.read_rng()
    gpu.reproject_display(c0, c1, flags=CPT_TRAVERSAL_ORDERED)
    ids = gpu.read_gbuffer()["id"]
    reused = gpu.read_display_count() > 0
    passes(c1, 4)
    reprojected, cnt = gpu.read_mix(), gpu.read_display_count()
    assert (cnt[reused] == 36).all() and (cnt[~reused] == 4).all() and 0.5 <= reused.mean() < 1.0
    gpu.write_rng(states)
    gpu.reset_display()
    passes(c1, 4)
    restart = gpu.read_mix()
    assert (gpu.read_display_count() == 4).all()
    a = ((reprojected.astype(np.float64) - truth) ** 2).mean(axis=1)
    b = ((restart.astype(np.float64) - truth) ** 2).mean(axis=1)
    for k in range(4):
        m = ids == k
        print(f"object {k}: {int(m.sum())} pixels, reprojected MSE {a[m].mean():.6g}, restart MSE {b[m].mean():.6g}")
    print(f"frame: reprojected MSE {a.mean():.6g}, restart MSE {b.mean():.6g}, ratio {a.mean() / b.mean():.4f}; "
          f"floor ratio {a[ids == 0].mean() / b[ids == 0].mean():.4f}; {reused.mean():.3f} of the frame reused")
    return a, b, ids


def test_reprojected_display_beats_a_restart(e2e):
    """The frame's MSE to the truth with the reprojected history is strictly below the restart's
    (DESIGN.md §22 records the measured ratio; none is fixed here)."""
    a, b, _ = e2e
    assert a.mean() < b.mean()


def test_reprojected_floor_beats_a_restart(e2e):
    a, b, ids = e2e
    floor = ids == 0
    assert floor.mean() > 0.5 and a[floor].mean() < b[floor].mean()


# ----------------------------------------------------------------------------------- C++ API
def _headless(tmp_path, name, *args):
    from cpppathtracer_amd import build
    out = tmp_path / name
    r = subprocess.run([build.build_examples(), "--scene", "s4", "--width", "48", "--height", "32", "--depth", "4", "--seed",
                        str(scenes.DEFAULT_SEED), *args, "--bgra", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(out, dtype=np.uint8)


def test_headless_display_orbit_equals_the_python_sequence(gpu, sky, tmp_path):
    """cpt_headless --orbit 3 --spp 2 --display-reproject on (DispatchRay with
    PathTracer::SetDisplayReprojection, a Refresh after every move) writes the BGRA8 frame the same
    calls give through the Python wrapper, byte for byte: the loop's first pass at the camera's index
    2, history passes after it, reproject_display before the first pass of each new camera."""
    W, H, N, K = 48, 32, 3, 2
    got = _headless(tmp_path, "orbit.bgra", "--orbit", str(N), "--spp", str(K), "--display-reproject", "on")
    cams = tr.orbit_cameras(W, H, N)
    gpu.set_scene(scenes.scene_s4())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED)
    want = None
    for k, cam in enumerate(cams):
        for p in range(K):
            if k and p == 0:
                gpu.reproject_display(cams[k - 1], cam, flags=CPT_TRAVERSAL_ORDERED)
            gpu.render(cam, 1, 4, aux=True, sync=True, ordered=True, schedule="previous")
            want = gpu.denoise_mix(2) if (k, p) == (0, 0) else gpu.denoise_mix_history()
    cnt = gpu.read_display_count()
    assert (cnt == 2 * N + 1).mean() > 0.5 and (cnt == K).any()   # history kept, and restarted where there is none
    assert got.tobytes() == want.tobytes()


def test_headless_loop_without_display_reprojection_is_todays(tmp_path):
    """SetDisplayReprojection(false) is the loop as it was: the frames of --dispatch 4.  A still
    camera with it on gives the same running mean, byte for byte."""
    today = _headless(tmp_path, "dispatch.bgra", "--dispatch", "4")
    off = _headless(tmp_path, "off.bgra", "--orbit", "1", "--spp", "4", "--display-reproject", "off")
    on = _headless(tmp_path, "on.bgra", "--orbit", "1", "--spp", "4", "--display-reproject", "on")
    assert today.any()
    assert off.tobytes() == today.tobytes()
    assert on.tobytes() == today.tobytes()
