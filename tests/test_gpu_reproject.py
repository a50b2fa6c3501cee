"""cpt_reproject_accum on the GPU: the kernel against cpt_reproject_host bit for bit
(itself held to the numpy restatement by tests/test_reproject_model.py), what the call must leave
alone, its error codes, its place in the stream's order, and the point of it all: after a camera
step the reprojected frame is closer to the truth than a restart at equal new passes.
"""
import ctypes
import subprocess
from types import SimpleNamespace

import gbuffer_model as gm
import numpy as np
import pytest
import reproject_model as rm
import test_gpu_async_order as ao

from cpppathtracer_amd import CptError, Renderer, camera_get_copy, scenes
from cpppathtracer_amd._lib import CPT_RENDER_AUX, CPT_TRAVERSAL_ORDERED, CPT_TRAVERSAL_PLAIN_LEAVES
from cpppathtracer_amd.renderer import reproject_host

pytestmark = pytest.mark.gpu

WALKS = {"reference": 0, "ordered": CPT_TRAVERSAL_ORDERED, "plain": CPT_TRAVERSAL_ORDERED | CPT_TRAVERSAL_PLAIN_LEAVES}
INVALID, STATE = 1, 5
shared = ao.shared   # the ordering tests' workload (a module fixture of test_gpu_async_order.py)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gbuffer(gpu, cam, flags):
    gpu.gbuffer(cam, flags)
    return gpu.read_gbuffer()


def _parity(gpu, objs, pair, walks, max_history=rm.MAX_HISTORY, plane_tol=rm.PLANE_TOL):
    """write_accum(history), reproject_accum, read_accum against cpt_reproject_host on the device's
    own G-buffer planes at both cameras; returns the last result."""
    c0, c1 = camera_get_copy(pair[0]), camera_get_copy(pair[1])
    W, H = int(c0["width"]), int(c0["height"])
    gpu.set_scene(objs)
    gpu.set_env(None)
    gpu.set_frame(W, H)
    d0, d1 = gm.camera_rays(c0)[1], gm.camera_rays(c1)[1]
    got = None
    for walk in walks:
        flags = WALKS[walk]
        g0, g1 = _gbuffer(gpu, c0, flags), _gbuffer(gpu, c1, flags)
        hist = rm.history(g0["id"], W, H)
        want = reproject_host(c0, c1, d0, d1, g0["id"], g0["t"], g1["id"], g1["t"], g1["normal"], hist, max_history, plane_tol)
        gpu.write_accum(hist)
        gpu.reproject_accum(c0, c1, max_history, plane_tol, flags)
        got = gpu.read_accum()
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=walk)
        after = gpu.read_gbuffer()
        for k in g1:
            np.testing.assert_array_equal(_bits(after[k]), _bits(g1[k]), err_msg=f"{walk}: read_gbuffer {k} is not the new camera's")
        assert gpu.last_reproject_ms() > 0.0 and len(gpu.last_reproject_ms(split=True)) == 3
    return got


@pytest.mark.parametrize("pair", sorted(rm.camera_pairs(1, 1)))
@pytest.mark.parametrize("wh", rm.FRAMES, ids=lambda wh: "%dx%d" % wh)
def test_kernel_equals_the_host_function(gpu, wh, pair):
    got = _parity(gpu, scenes.scene_s4(), rm.camera_pairs(*wh)[pair], WALKS)
    if pair == "away":
        assert (got == 0).all()
    elif wh != (1, 1):
        reused = (got[:, 3] > 0).mean()
        assert 0.05 <= reused <= 0.95, reused   # neither an all-zero nor an all-reused frame


def _nudged(cam0):
    """A fixture's camera and a nearby one: a step of the origin, half of it for the look-at point."""
    c1 = cam0.copy()
    c1["origin"] = (np.asarray(cam0["origin"], np.float32) + np.array([6.0, 2.0, -6.0], np.float32))
    c1["look_at"] = (np.asarray(cam0["look_at"], np.float32) + np.array([3.0, 0.0, -3.0], np.float32))
    return cam0, c1


@pytest.mark.parametrize("name", ["s1000_96x64", "fuzz_hyb_48x32"])
def test_kernel_equals_the_host_function_on_large_scenes(gpu, name):
    """S1000 (the wide walk on its LDS image) and a fuzz scene whose 4-wide tree outgrows the image,
    under the ordered walk."""
    objs, cam0, _ = gm.fixtures()[name]
    got = _parity(gpu, objs, _nudged(cam0), ["ordered"])
    n_wide = gpu.walk_info()["n_wide"]
    assert n_wide > 512 if name == "fuzz_hyb_48x32" else 0 < n_wide <= 512
    reused = (got[:, 3] > 0).mean()
    assert 0.05 <= reused <= 0.95, reused


@pytest.mark.parametrize("max_history,plane_tol", [(1, 0.0), (8, 1e-3), (128, 1e-1)])
def test_kernel_equals_the_host_function_at_other_settings(gpu, max_history, plane_tol):
    _parity(gpu, scenes.scene_s4(), rm.camera_pairs(64, 48)["sideways"], ["ordered"], max_history, plane_tol)


# ------------------------------------------------------------------------------ side effects
def test_reproject_leaves_the_rest_of_the_frame_alone(gpu, sky):
    """After an adaptive render, filter_frame and a display pass: the call changes the accumulator
    and the G-buffer, and none of the RNG planes, the aux buffers, the Mix buffer and the filtered
    planes; it drops the adaptive result."""
    W, H = 64, 48
    c0, c1 = (camera_get_copy(c) for c in rm.camera_pairs(W, H)["sideways"])
    gpu.set_scene(scenes.scene_s4())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED)
    gpu.render_adaptive(c0, 8, 32, 4, 0.1, 8, flags=CPT_RENDER_AUX | CPT_TRAVERSAL_ORDERED)
    gpu.filter_frame()
    gpu.denoise_mix(1)

    def state():
        return [gpu.read_rng(), *gpu.read_aux(), gpu.read_mix(), *gpu.read_filtered()]
    before, accum = state(), gpu.read_accum()
    gpu.read_noise()
    want = _gbuffer(gpu, c1, CPT_TRAVERSAL_ORDERED)
    gpu.gbuffer(c0, CPT_TRAVERSAL_ORDERED)
    gpu.reproject_accum(c0, c1, flags=CPT_TRAVERSAL_ORDERED)
    for a, b in zip(before, state()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    got = gpu.read_gbuffer()
    for k in want:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=k)
    assert gpu.read_accum().tobytes() != accum.tobytes()
    for call in (gpu.read_noise, gpu.read_moments, gpu.filter_frame):
        with pytest.raises(CptError) as e:
            call()
        assert e.value.status == STATE
    # the next adaptive render brings a result back
    gpu.render_adaptive(c1, 8, 16, 4, 0.1, 8, flags=CPT_RENDER_AUX | CPT_TRAVERSAL_ORDERED)
    gpu.read_noise()


# ------------------------------------------------------------------------------------ errors
def _raises(status, call):
    with pytest.raises(CptError) as e:
        call()
    assert e.value.status == status, e.value


def test_errors_write_nothing(gpu):
    W, H = 64, 48
    c0, c1 = (camera_get_copy(c) for c in rm.camera_pairs(W, H)["sideways"])
    small = camera_get_copy(rm.camera_pairs(16, 16)["sideways"][1])
    hist = np.random.default_rng(3).random((W * H, 4), dtype=np.float32) + np.float32(1.0)

    # no scene, no frame: fresh contexts
    r = Renderer(0)
    try:
        _raises(STATE, lambda: r.reproject_accum(c0, c1))          # neither
        r.set_frame(W, H)
        r.write_accum(hist)
        _raises(STATE, lambda: r.reproject_accum(c0, c1))          # no scene
        np.testing.assert_array_equal(_bits(r.read_accum()), _bits(hist))
    finally:
        r.close()
    r = Renderer(0)
    try:
        r.set_scene(scenes.scene_s4())
        _raises(STATE, lambda: r.reproject_accum(c0, c1))          # no frame
    finally:
        r.close()

    gpu.set_scene(scenes.scene_s4())
    gpu.set_env(None)
    # frames that are not full: a row list, and a leading run of rows
    for rows in ([5, 2, 40], list(range(24))):
        gpu.set_frame(W, H, rows)
        part = hist[:len(rows) * W]
        gpu.write_accum(part)
        _raises(STATE, lambda: gpu.reproject_accum(c0, c1))
        np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(part))

    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED)
    gpu.write_accum(hist)
    L, ctx = gpu._L, gpu._ctx
    p0, p1 = (ctypes.c_void_p(np.ascontiguousarray(c).ctypes.data) for c in (c0, c1))
    bad = [
        lambda: gpu._check(L.cpt_reproject_accum(ctx, None, p1, 32, ctypes.c_float(1e-2), 0)),
        lambda: gpu._check(L.cpt_reproject_accum(ctx, p0, None, 32, ctypes.c_float(1e-2), 0)),
        lambda: gpu.reproject_accum(small, c1),
        lambda: gpu.reproject_accum(c0, small),
        lambda: gpu.reproject_accum(c0, c1, max_history=0),
        lambda: gpu.reproject_accum(c0, c1, max_history=-3),
        lambda: gpu.reproject_accum(c0, c1, plane_tol=-1e-3),
        lambda: gpu.reproject_accum(c0, c1, plane_tol=float("nan")),
        lambda: gpu.reproject_accum(c0, c1, plane_tol=float("inf")),
        lambda: gpu.reproject_accum(c0, c1, flags=CPT_RENDER_AUX),
        lambda: gpu.reproject_accum(c0, c1, flags=CPT_TRAVERSAL_ORDERED | 0x1),
    ]
    for call in bad:
        _raises(INVALID, call)
        np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(hist))
    _raises(STATE, gpu.read_gbuffer)   # none of the failed calls traced anything

    # an adaptive render pending
    gpu.write_accum(hist)
    gpu.adaptive_begin(c0, 4, 8, 2, 0.0, 4, flags=CPT_TRAVERSAL_ORDERED)
    _raises(STATE, lambda: gpu.reproject_accum(c0, c1))
    while gpu.adaptive_step():
        pass
    gpu.reproject_accum(c0, c1)   # and works once it has ended
    gpu.synchronize()


# -------------------------------------------------------------------------------- end to end
E2E_STEP = (4.0, 0.0, -4.0)   # the camera's sideways step (origin and look-at point), world units


def e2e_cameras(W, H):
    """The scenes' camera as the reference's MotionalCamera makes it (lens_radius 0.0005) and the
    same camera a step to the side.  Not a pinhole: at lens_radius 0 every pass of a pixel shoots
    the same first ray, and where that ray's mirror bounce starts inside the sphere by rounding
    (BOUNCE_RAY_TMIN is 2e-5) the pixel is black in every pass; which pixels those are changes
    with the camera, so no history, kept or reprojected, says anything about them."""
    from cpppathtracer_amd.scenes import CAMERA_LOOK_AT as AT, CAMERA_ORIGIN as O
    from cpppathtracer_amd.types import make_camera
    move = lambda p: tuple(a + b for a, b in zip(p, E2E_STEP))
    return (camera_get_copy(make_camera(W, H, origin=O, look_at=AT)),
            camera_get_copy(make_camera(W, H, origin=move(O), look_at=move(AT))))


@pytest.fixture(scope="module")
def e2e(gpu, sky):
    """S4, 64x48, depth 8.  32 spp at C0, reprojected to a nearby C1, plus 4 spp there, against a
    restart: 4 spp at C1 from the same RNG states.  Truth: 1024 spp at C1.  Per pixel: the squared
    error of both means (averaged over rgb) and the object the pixel sees."""
    W, H, DEPTH = 64, 48, 8
    c0, c1 = e2e_cameras(W, H)
    kw = dict(ordered=True)
    gpu.set_scene(scenes.scene_s4())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(scenes.DEFAULT_SEED + 1)
    gpu.render(c1, 1024, DEPTH, sync=True, **kw)
    truth = gpu.read_accum()
    truth = truth[:, :3].astype(np.float64) / truth[:, 3:4]
    gpu.init_rng(scenes.DEFAULT_SEED)
    gpu.render(c0, 32, DEPTH, sync=True, **kw)
    states = gpu.read_rng()
    gpu.reproject_accum(c0, c1, flags=CPT_TRAVERSAL_ORDERED)
    ids = gpu.read_gbuffer()["id"]
    reused = gpu.read_accum()[:, 3] > 0
    gpu.render(c1, 4, DEPTH, accumulate=True, sync=True, **kw)
    reprojected = gpu.read_accum()
    gpu.write_rng(states)
    gpu.clear_accum()
    gpu.render(c1, 4, DEPTH, accumulate=True, sync=True, **kw)
    restart = gpu.read_accum()
    assert (restart[:, 3] == 4).all() and (reprojected[:, 3] >= 4).all()
    assert (reprojected[reused, 3] == 36).all() and 0.5 <= reused.mean() < 1.0

    def err(accum):
        mean = accum[:, :3] / accum[:, 3:4]
        return ((mean.astype(np.float64) - truth) ** 2).mean(axis=1)
    a, b = err(reprojected), err(restart)
    for k in range(4):
        m = ids == k
        print(f"object {k}: {int(m.sum())} pixels, reprojected MSE {a[m].mean():.6g}, restart MSE {b[m].mean():.6g}")
    print(f"frame: reprojected MSE {a.mean():.6g}, restart MSE {b.mean():.6g}, ratio {a.mean() / b.mean():.4f}; "
          f"{reused.mean():.3f} of the frame reused")
    return a, b, ids


def test_reprojected_frame_beats_a_restart(e2e):
    """The whole frame's MSE to the truth, reprojected, is strictly below the restart's.  On the
    CPU (oracle + cpt_reproject_host) the ratio is 0.15 to 0.20 at sideways steps from 0.02 to 8
    world units, 0.17 at this one; the fixture prints the device's figures."""
    a, b, _ = e2e
    assert a.mean() < b.mean()


def test_reprojected_objects_each_beat_a_restart(e2e):
    """And so is the MSE over the pixels of each of S4's four objects, the glass, metal and mirror
    spheres included."""
    a, b, ids = e2e
    for k in range(4):
        assert (ids == k).sum() >= 50 and a[ids == k].mean() < b[ids == k].mean(), k


def test_reprojected_diffuse_surfaces_beat_a_restart(e2e):
    """The same comparison on the pixels that see the diffuse floor, where outgoing radiance does
    not depend on the view: 36 passes of history against 4 must at least halve the MSE."""
    a, b, ids = e2e
    floor = ids == 0
    assert floor.mean() > 0.5
    assert a[floor].mean() < 0.5 * b[floor].mean()


# ---------------------------------------------------------------------------------- ordering
def _second_camera():
    c = scenes.camera_for(ao.W, ao.H)
    c["origin"] = np.asarray(c["origin"], np.float32) + np.array([5.0, 0.0, -5.0], np.float32)
    return camera_get_copy(c)


def _reproject_then_render(stream_of=None):
    def call(r, e):
        if stream_of:
            r.set_stream(stream_of(e))
        r.reproject_accum(e.cam, e.cam2, flags=ao.WALK)
        r.render(e.cam2, 32, ao.DEPTH, accumulate=True, **ao.KW)
    return call


ORDER_CASES = [
    ao.Case("reproject-render", _reproject_then_render(), ao.IMAGE + ("gbuffer",), rerecords=True),
    ao.Case("reproject-render-after-set_stream", _reproject_then_render(lambda e: e.ts.cuda_stream), ao.IMAGE + ("gbuffer",),
            before=ao._stream, rerecords=True),
    ao.Case("reproject-render-back-on-own-stream", _reproject_then_render(lambda e: None), ao.IMAGE + ("gbuffer",),
            before=ao._on_stream, rerecords=True),
]


@pytest.mark.parametrize("case", ORDER_CASES, ids=lambda c: c.name)
def test_reproject_behind_a_render_in_flight(shared, case):
    """cpt_reproject_accum queued behind an unsynchronised cpt_render, and a cpt_render queued behind
    it, give the bytes of the sequence synchronised after every call; also across cpt_set_stream."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    e = SimpleNamespace(**vars(shared), cam2=_second_camera())
    want, _, first = ao._run(case, e, twin=True)
    got, (t_launch, t_call, _), _ = ao._run(case, e, twin=False)
    ao.assert_overlap(case.name, t_launch, t_call, first[2])
    ao._assert_same_bits(got, want)
    reused = (want["accum"].view(np.float32).reshape(-1, 4)[:, 3] > 32).mean()
    assert reused >= 0.25, "the reprojection kept no history: a vacuous case"


# ----------------------------------------------------------------------------------- C++ API
def test_headless_orbit_equals_the_python_sequence(gpu, sky, tmp_path):
    """cpt_headless --orbit 3 --reproject (PathTracer::Reproject between the frames of a small orbit)
    writes the PFM the same calls give through the Python wrapper, bit for bit."""
    from cpppathtracer_amd import build
    W, H, SPP, DEPTH, N = 48, 32, 2, 4, 3
    out = tmp_path / "orbit.pfm"
    r = subprocess.run([build.build_examples(), "--scene", "s4", "--width", str(W), "--height", str(H), "--spp", str(SPP),
                        "--depth", str(DEPTH), "--seed", str(scenes.DEFAULT_SEED), "--orbit", str(N), "--reproject", "--pfm", str(out)],
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
    gpu.init_rng(scenes.DEFAULT_SEED)
    for k, cam in enumerate(cams):
        if k:
            gpu.reproject_accum(cams[k - 1], cam, flags=CPT_TRAVERSAL_ORDERED)
        gpu.render(cam, SPP, DEPTH, accumulate=k > 0, sync=True, ordered=True)
    acc = gpu.read_accum()
    assert (acc[:, 3] > SPP).mean() > 0.5
    want = (acc[:, :3] / acc[:, 3:4]).astype(np.float32)
    np.testing.assert_array_equal(_bits(pfm), _bits(want))


def orbit_cameras(W, H, n):
    """The headless driver's orbit: one degree per frame about the vertical axis through the look-at
    point, the offset turned in float32 as the driver writes it."""
    from cpppathtracer_amd.scenes import CAMERA_LOOK_AT as AT, CAMERA_ORIGIN as O
    from cpppathtracer_amd.types import make_camera
    F = np.float32
    c, s = F(0.99984770), F(0.01745241)
    dx, dz = F(O[0]) - F(AT[0]), F(O[2]) - F(AT[2])
    cams = []
    for k in range(n):
        if k:
            dx, dz = c * dx + s * dz, c * dz - s * dx
        cams.append(camera_get_copy(make_camera(W, H, origin=(F(AT[0]) + dx, F(O[1]), F(AT[2]) + dz), look_at=AT)))
    return cams
