"""cpt_filter_frame_spatial on the GPU: the filter for frames without moments, held
bit for bit in rgb and variance to the host hooks (which tests/test_filter_spatial_model.py holds to
the numpy restatement); cpt_write_gbuffer's round trip; what the call must leave alone, its error
codes and its place in the stream's order; the C++ API's path through the headless example; and the
point of it: a reprojected, topped-up frame leaves with a lower error than it came with.
"""
import subprocess
from types import SimpleNamespace

import filter_model as fm
import filter_spatial_model as sm
import numpy as np
import pytest
import test_filter_spatial_model as host
import test_gpu_async_order as ao
import tracked_reproject_model as tm

from cpppathtracer_amd import CptError, Renderer, camera_get_copy, scenes
from cpppathtracer_amd._lib import CPT_ERR_INVALID_ARG, CPT_ERR_STATE, CPT_RENDER_AUX, CPT_TRAVERSAL_ORDERED

pytestmark = pytest.mark.gpu

DEPTH, SEED = 8, scenes.DEFAULT_SEED
WALK = CPT_TRAVERSAL_ORDERED
D = sm.DEFAULTS
shared = ao.shared   # the ordering test's workload (a module fixture of test_gpu_async_order.py)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _assert_filtered(gpu, accum, ids, normal, W, H, levels, sigma_l, sharp, what=""):
    want_rgb, want_var = host.host_run(accum, ids, normal, W, H, levels, sigma_l, sharp)
    rgb, var = gpu.read_filtered()
    fm.assert_same_bits(rgb, want_rgb, f"{what} levels {levels} rgb")
    fm.assert_same_bits(var, want_var, f"{what} levels {levels} variance")
    return want_rgb, want_var


def _raises(status, call):
    with pytest.raises(CptError) as e:
        call()
    assert e.value.status == status, e.value


# ------------------------------------------------------------------------------ the checkpoint
def test_write_gbuffer_round_trips_every_plane(gpu):
    W, H = 67, 9
    rs = np.random.RandomState(4)
    gpu.set_frame(W, H)
    _raises(CPT_ERR_STATE, gpu.read_gbuffer)                 # set_frame dropped the G-buffer
    ids = rs.randint(-1, 50, W * H).astype(np.int32)
    gpu.write_gbuffer(id=ids)                                # the other planes: never written, zero
    g = gpu.read_gbuffer()
    np.testing.assert_array_equal(g["id"], ids)
    assert not g["t"].any() and not g["normal"].any() and not g["albedo"].any()
    planes = dict(t=rs.rand(W * H).astype(np.float32), normal=rs.standard_normal((W * H, 3)).astype(np.float32),
                  albedo=rs.rand(W * H, 3).astype(np.float32))
    planes["t"][:4] = [np.inf, 1e30, -0.0, np.nan]
    gpu.write_gbuffer(**planes)                              # id = None: left as it is
    g = gpu.read_gbuffer()
    np.testing.assert_array_equal(g["id"], ids)
    for k, v in planes.items():
        np.testing.assert_array_equal(_bits(g[k]), _bits(v), err_msg=k)
    # too few pixels: nothing written
    L = gpu._L
    import ctypes
    other = np.zeros(W * H, dtype=np.int32)
    assert L.cpt_write_gbuffer(gpu._ctx, ctypes.c_void_p(other.ctypes.data), None, None, None, W * H - 1) == CPT_ERR_INVALID_ARG
    np.testing.assert_array_equal(gpu.read_gbuffer()["id"], ids)


# ----------------------------------------------------------------------- parity: synthetic states
@pytest.mark.parametrize("kind", sm.ID_KINDS)
@pytest.mark.parametrize("wh", sm.SHAPES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_synthetic_states_equal_the_host_hooks(gpu, wh, kind):
    """States pushed in with write_accum / write_gbuffer, invalid pixels among them.  Level 0 is the
    prepare kernel alone, 1 and 2 the LDS variants, 3 and 5 reach the global-memory variant."""
    W, H = wh
    accum, normal = sm.synthetic_state(W, H, seed=200 + W, nan_normal=(kind == "miss"))
    ids = sm.id_plane(W, H, kind)
    gpu.set_frame(W, H)
    gpu.write_accum(accum)
    gpu.write_gbuffer(id=ids, normal=normal)
    for levels, sigma_l, sharp in ((0, 2.0, 3), (1, 2.0, 3), (2, 2.0, 3), (3, 2.0, 3), (5, 2.0, 3), (5, 1.0, 7), (2, 0.0, 0)):
        gpu.filter_frame_spatial(levels=levels, sigma_l=sigma_l, normal_sharpness_log2=sharp)
        _assert_filtered(gpu, accum, ids, normal, W, H, levels, sigma_l, sharp, kind)
    assert gpu.last_filter_ms() > 0.0


# --------------------------------------------------------------------------- parity: real frames
def _frame(gpu, sky, W, H, objs):
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED)


def _check_frame(gpu, W, H, what):
    """The device's result against the host hooks on the planes read back, at the defaults and at
    five levels."""
    accum, g = gpu.read_accum(), gpu.read_gbuffer()
    for levels in (D["levels"], 5):
        gpu.filter_frame_spatial(levels=levels)
        rgb, _ = _assert_filtered(gpu, accum, g["id"], g["normal"], W, H, levels, D["sigma_l"], D["sharpness"], what)
    with np.errstate(all="ignore"):
        mean = accum[:, :3] / accum[:, 3:4]
    assert (rgb != mean).any() and len(set(g["id"].tolist())) >= 3
    return accum, g


@pytest.mark.parametrize("wh", [(64, 48), (67, 41)], ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_real_frames_equal_the_host_hooks(gpu, sky, wh):
    """S4 + cylinder at 8 passes with cpt_gbuffer; the same after reproject_accum to a moved camera
    and render_to_count(32) with no cpt_gbuffer in between (the reprojection left the new camera's);
    the same after reproject_accum_tracked across one sphere move."""
    from test_gpu_topup import e2e_cameras
    W, H = wh
    c0, c1 = e2e_cameras(W, H)
    old, new, _, edited = tm.edits()["sphere_moved"]
    _frame(gpu, sky, W, H, old)
    gpu.render(c0, 8, DEPTH, sync=True, ordered=True)
    gpu.gbuffer(c0, WALK)
    _check_frame(gpu, W, H, "plain render")
    gpu.reproject_accum(c0, c1, flags=WALK)
    gpu.render_to_count(c1, 32, DEPTH, sync=True, flags=WALK)
    accum, _ = _check_frame(gpu, W, H, "reprojected and topped up")
    assert (accum[:, 3] >= 32).all()
    gpu.history_capture(c1, WALK)
    idx = np.asarray(edited, dtype=np.int32)
    gpu.update_objects(idx, new[idx])
    gpu.reproject_accum_tracked(c1, flags=WALK)
    accum, _ = _check_frame(gpu, W, H, "tracked")
    assert (accum[:, 3] == 0).any()                       # the move uncovered pixels: they stay zero
    rgb, var = gpu.read_filtered()
    assert not rgb[accum[:, 3] == 0].any() and not var[accum[:, 3] == 0].any()


# -------------------------------------------------------------------------------- side effects
def test_the_call_leaves_the_rest_of_the_frame_alone(gpu, sky):
    """Accumulator, RNG planes, aux, moments, G-buffer, display state, reprojection history and top-up
    plan are bit-identical after the call; a later cpt_filter_frame on the adaptive frame gives its
    own result; a later adaptive render is what it is without the call."""
    W, H = 64, 48
    cam = camera_get_copy(scenes.camera_for(W, H))

    def start():
        _frame(gpu, sky, W, H, tm.scene())
        gpu.render_adaptive(cam, 4, 8, 2, 0.1, DEPTH, flags=WALK | CPT_RENDER_AUX)
        gpu.render_to_count(cam, 8, DEPTH, aux=True, sync=True, flags=WALK)
    start()
    plain = gpu.read_accum(), gpu.read_rng()
    again = gpu.render_adaptive(cam, 4, 8, 2, 0.1, DEPTH, flags=WALK | CPT_RENDER_AUX)
    want_next = gpu.read_accum(), gpu.read_rng(), gpu.read_moments(), again["active_tiles"]
    start()
    np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(plain[0]))
    gpu.denoise_mix_history()
    gpu.history_capture(cam, WALK)
    gpu.filter_frame()
    moments_filtered = gpu.read_filtered()

    def state():
        g = gpu.read_gbuffer()
        n, d = gpu.read_aux()
        info = gpu.topup_info()
        return [gpu.read_accum(), gpu.read_rng(), n, d, gpu.read_moments(), gpu.read_mix(), gpu.read_display_count(),
                g["id"], g["t"], g["normal"], g["albedo"], np.array([info["tiles"], info["pixels"], info["passes"]]),
                np.array([int(gpu.history_info()[0])])]
    before = state()
    gpu.filter_frame_spatial()
    spatial = gpu.read_filtered()
    for k, (a, b) in enumerate(zip(before, state())):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"state {k}")
    assert (spatial[0] != moments_filtered[0]).any()
    gpu.filter_frame()
    for a, b in zip(gpu.read_filtered(), moments_filtered):
        fm.assert_same_bits(a, b, "cpt_filter_frame after the spatial call")
    got = gpu.render_adaptive(cam, 4, 8, 2, 0.1, DEPTH, flags=WALK | CPT_RENDER_AUX)
    for a, b in zip((gpu.read_accum(), gpu.read_rng(), gpu.read_moments(), got["active_tiles"]), want_next):
        np.testing.assert_array_equal(_bits(a), _bits(b))


def test_the_reprojection_history_survives_the_call(gpu, sky):
    """The captured history (its id and distance planes, its camera, its objects) is what a tracked
    reprojection reads: the same edit and reproject_accum_tracked after a filter call give the
    accumulator, the G-buffer and the renewed history of the sequence without the call."""
    from test_gpu_topup import e2e_cameras
    W, H = 64, 48
    c0, c1 = e2e_cameras(W, H)
    old, new, _, edited = tm.edits()["sphere_moved"]
    idx = np.asarray(edited, dtype=np.int32)

    def run(with_filter):
        _frame(gpu, sky, W, H, old)
        gpu.render(c0, 8, DEPTH, sync=True, ordered=True)
        gpu.history_capture(c0, WALK)                        # leaves c0's G-buffer on the frame as well
        if with_filter:
            gpu.filter_frame_spatial()
            assert np.isfinite(gpu.read_filtered()[0]).all()
        before = gpu.history_info()
        gpu.update_objects(idx, new[idx])
        gpu.reproject_accum_tracked(c1, flags=WALK)
        g = gpu.read_gbuffer()
        return [gpu.read_accum(), g["id"], g["t"], g["normal"], g["albedo"], np.frombuffer(before[1].tobytes(), dtype=np.uint8),
                np.frombuffer(gpu.history_info()[1].tobytes(), dtype=np.uint8)]
    want, got = run(False), run(True)
    assert (want[0][:, 3] > 0).any() and (want[0][:, 3] == 0).any()
    for k, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"state {k}")


# -------------------------------------------------------------------------------------- errors
def test_errors_write_nothing(gpu, sky):
    W, H = 20, 12
    accum, normal = sm.synthetic_state(W, H, seed=77)
    ids = sm.id_plane(W, H, "vstripes")
    # no G-buffer is valid: on an adaptive frame that cpt_filter_frame has filtered, whose result stays
    cam = camera_get_copy(scenes.camera_for(W, H))
    _frame(gpu, sky, W, H, scenes.scene_s4())
    gpu.render_adaptive(cam, 4, 8, 2, 0.1, 4, flags=WALK | CPT_RENDER_AUX)
    gpu.filter_frame()
    by_moments = gpu.read_filtered()
    _raises(CPT_ERR_STATE, gpu.filter_frame_spatial)
    for a, b in zip(gpu.read_filtered(), by_moments):
        fm.assert_same_bits(a, b, "cpt_filter_frame's result after the refused call")
    gpu.set_frame(W, H)
    gpu.write_accum(accum)
    _raises(CPT_ERR_STATE, gpu.filter_frame_spatial)                     # nor here, with no result yet
    gpu.write_gbuffer(id=ids, normal=normal)
    gpu.filter_frame_spatial(levels=2)
    kept = gpu.read_filtered()

    def still_there():
        for a, b in zip(gpu.read_filtered(), kept):
            fm.assert_same_bits(a, b, "the earlier result")
    for bad in (dict(levels=-1), dict(levels=9), dict(sigma_l=-1.0), dict(sigma_l=float("nan")), dict(sigma_l=float("inf")),
                dict(normal_sharpness_log2=-1), dict(normal_sharpness_log2=11)):
        _raises(CPT_ERR_INVALID_ARG, lambda: gpu.filter_frame_spatial(**bad))
        still_there()
    # an adaptive render pending
    gpu.set_scene(scenes.scene_s4())
    gpu.set_env(sky)
    gpu.init_rng(SEED)
    gpu.adaptive_begin(cam, 4, 8, 2, 0.1, 4, flags=WALK)
    _raises(CPT_ERR_STATE, gpu.filter_frame_spatial)
    while gpu.adaptive_step():
        pass
    still_there()
    # a row list / a frame that is not full; no frame
    with Renderer(0) as r:
        _raises(CPT_ERR_STATE, r.filter_frame_spatial)                   # no frame
        _raises(CPT_ERR_STATE, r.write_gbuffer)
        r.set_frame(W, H, rows=np.arange(0, H, 2, dtype=np.int32))
        r.write_gbuffer(id=np.zeros(W * (H // 2), dtype=np.int32))
        _raises(CPT_ERR_STATE, r.filter_frame_spatial)
        r.set_frame(W, H, rows=np.arange(H, dtype=np.int32)[::-1].copy())
        r.write_gbuffer(id=ids)
        _raises(CPT_ERR_STATE, r.filter_frame_spatial)
        _raises(CPT_ERR_STATE, r.read_filtered)


# ------------------------------------------------------------------------------------ ordering
def _filter_then_read(r, e):
    r.filter_frame_spatial()
    return r.read_filtered()   # unsynchronised: the read orders itself behind the filter


ORDER_CASE = ao.Case("render-filter_frame_spatial", _filter_then_read, ao.IMAGE + ("filtered", "gbuffer"),
                     before=lambda r, e: r.gbuffer(e.cam, ao.WALK))


def test_filter_behind_a_render_in_flight(shared):
    """cpt_filter_frame_spatial queued behind an unsynchronised cpt_render reads the accumulator that
    render leaves: the bytes of the sequence synchronised after every call."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    want, _, first = ao._run(ORDER_CASE, shared, twin=True)
    got, (t_launch, t_call, render_ms), _ = ao._run(ORDER_CASE, shared, twin=False)
    ao.assert_overlap(ORDER_CASE.name, t_launch, t_call, render_ms)
    ao._assert_same_bits(got, want)
    acc = first[0]
    assert (want["filtered.0"].reshape(-1, 3) != (acc[:, :3] / acc[:, 3:4])).any()


# ----------------------------------------------------------------------------------- C++ API
def _read_pfm(path, W, H):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        assert tuple(int(v) for v in f.readline().split()) == (W, H)
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), dtype="<f4").reshape(H, W, 3)[::-1].reshape(-1, 3)


def test_headless_filter_spatial_equals_the_python_sequence(gpu, sky, tmp_path):
    """cpt_headless --orbit 3 --reproject --fill 16 --filter-spatial (PathTracer::FilterRadianceSpatial
    after the last frame: the reprojection left that camera's G-buffer) writes the PFM the same calls
    give through the Python wrapper; with plain --spp the G-buffer is traced first."""
    from cpppathtracer_amd import build
    from test_gpu_reproject import orbit_cameras
    W, H, SPP, N, FILL = 48, 32, 2, 3, 16
    exe = build.build_examples()
    common = ["--scene", "s4", "--width", str(W), "--height", str(H), "--spp", str(SPP), "--depth", "4", "--seed", str(SEED)]
    out = tmp_path / "orbit.pfm"
    r = subprocess.run([exe, *common, "--orbit", str(N), "--reproject", "--fill", str(FILL), "--filter-spatial", "--pfm", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    cams = orbit_cameras(W, H, N)
    _frame(gpu, sky, W, H, scenes.scene_s4())
    for k, cam in enumerate(cams):
        if k == 0:
            gpu.render(cam, SPP, 4, aux=True, sync=True, ordered=True)
            continue
        gpu.reproject_accum(cams[k - 1], cam, flags=WALK)
        gpu.render_to_count(cam, FILL, 4, aux=True, sync=True, flags=WALK)
    gpu.filter_frame_spatial()
    want, _ = gpu.read_filtered()
    acc = gpu.read_accum()
    assert (want != acc[:, :3] / acc[:, 3:4]).any()
    np.testing.assert_array_equal(_bits(_read_pfm(out, W, H)), _bits(want))
    # plain --spp, five levels
    out = tmp_path / "plain.pfm"
    r = subprocess.run([exe, *common, "--filter-spatial", "5", "--pfm", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    _frame(gpu, sky, W, H, scenes.scene_s4())
    gpu.render(cams[0], SPP, 4, aux=True, sync=True, ordered=True)
    gpu.gbuffer(cams[0], WALK)
    gpu.filter_frame_spatial(levels=5)
    np.testing.assert_array_equal(_bits(_read_pfm(out, W, H)), _bits(gpu.read_filtered()[0]))
    # ReadGBuffer at a turned camera between two filter calls: the context's G-buffer is then the turned
    # camera's, and the second call must trace the render's camera again, not filter with the wrong one
    aside = tmp_path / "aside.pfm"
    r = subprocess.run([exe, *common, "--filter-spatial", "5", "--look-aside", "--pfm", str(aside)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "looked aside" in r.stdout, r.stdout + r.stderr
    np.testing.assert_array_equal(_bits(_read_pfm(aside, W, H)), _bits(gpu.read_filtered()[0]))
    gpu.gbuffer(cams[1], WALK)                               # what the wrong G-buffer would give differs
    gpu.filter_frame_spatial(levels=5)
    assert (gpu.read_filtered()[0] != _read_pfm(aside, W, H)).any()
    bad = subprocess.run([exe, "--scene", "s4", "--adaptive", "0.1", "--filter-spatial"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--filter-spatial" in bad.stderr


# -------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def e2e(gpu, sky):
    """§24's case: S4 + cylinder, 64x48, depth 8, 32 passes at C0, reprojected to C1 (8 units
    sideways), topped up to 32, filtered at the defaults.  Truth: 1024 passes at C1."""
    from test_gpu_topup import e2e_cameras
    W, H = 64, 48
    c0, c1 = e2e_cameras(W, H)
    _frame(gpu, sky, W, H, tm.scene())
    gpu.init_rng(SEED + 1)
    gpu.render(c1, 1024, DEPTH, sync=True, ordered=True)
    truth = gpu.read_accum()
    truth = truth[:, :3].astype(np.float64) / truth[:, 3:4]
    gpu.init_rng(SEED)
    gpu.render(c0, 32, DEPTH, sync=True, ordered=True)
    gpu.reproject_accum(c0, c1, flags=WALK)
    gpu.render_to_count(c1, 32, DEPTH, sync=True, flags=WALK)
    gpu.filter_frame_spatial()
    acc, ids = gpu.read_accum(), gpu.read_gbuffer()["id"]
    rgb, _ = gpu.read_filtered()
    err = lambda img: ((img.astype(np.float64) - truth) ** 2).mean(axis=1)
    a, b = err(acc[:, :3] / acc[:, 3:4]), err(rgb)
    print(f"frame: unfiltered MSE {a.mean():.6g}, filtered MSE {b.mean():.6g}")
    for obj in sorted(set(ids.tolist())):
        m = ids == obj
        print(f"{'miss (sky)' if obj < 0 else 'object %d' % obj} ({int(m.sum())} pixels): unfiltered MSE {a[m].mean():.6g}, "
              f"filtered MSE {b[m].mean():.6g}")
    return SimpleNamespace(a=a, b=b, ids=ids)


def test_the_defaults_lower_the_error_of_a_topped_up_frame(e2e):
    """Over the frame and over the floor's pixels alone the filtered mean image is nearer the truth
    than the unfiltered one.  The CPU rehearsal (tools/filter_spatial_ab.py --rehearsal) has the frame
    at 0.00107365 unfiltered against 0.00062394 filtered and the floor (object 0) at 0.000370296
    against 0.000229248; every object improves there, so each is asserted too."""
    e = e2e
    floor = e.ids == tm.FLOOR
    assert floor.sum() > 1000
    assert e.b.mean() < e.a.mean()
    assert e.b[floor].mean() < e.a[floor].mean()
    for obj in sorted(set(e.ids.tolist())):
        m = e.ids == obj
        assert e.b[m].mean() < e.a[m].mean(), obj
