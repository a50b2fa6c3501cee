"""cpt_meter_exposure and cpt_present on the GPU: the BGRA8 bytes, the meter's 257
words and the exposure's bits held to the host hooks (which tests/test_present_model.py holds to the
numpy restatement) for every tone curve and transfer, on full frames, row lists and filter results;
a meter, a present and a meter chained with no host wait; what the calls must leave alone, their
error codes and their place in the stream's order; and the C++ API through the headless example.
"""
import itertools
import subprocess

import numpy as np
import present_model as pm
import pytest
import test_gpu_async_order as ao
import tracked_reproject_model as tm

from cpppathtracer_amd import CptError, Renderer, camera_get_copy, present, scenes
from cpppathtracer_amd._lib import CPT_ERR_INVALID_ARG, CPT_ERR_STATE, CPT_RENDER_AUX, CPT_TRAVERSAL_ORDERED

pytestmark = pytest.mark.gpu

F = np.float32
DEPTH, SEED = 8, scenes.DEFAULT_SEED
WALK = CPT_TRAVERSAL_ORDERED
WHITE = 2.5
COMBOS = list(itertools.product(pm.TONES, pm.TRANSFERS))
shared = ao.shared   # the ordering test's workload (a module fixture of test_gpu_async_order.py)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _raises(status, call):
    with pytest.raises(CptError) as e:
        call()
    assert e.value.status == status, e.value


def _assert_presents(gpu, src, source, e, what):
    """Every tone x transfer of the context's source at its exposure `e` against cpt_present_host."""
    for tone, transfer in COMBOS:
        got = present.present(gpu, source, tone, WHITE, transfer).reshape(-1, 4)
        want = present.present_host(src, e, source, tone, WHITE, transfer)
        np.testing.assert_array_equal(got, want, err_msg=f"{what}: {source}, {tone}, {transfer}")
        np.testing.assert_array_equal(present.read_present(gpu).reshape(-1, 4), want)


def _assert_meters(gpu, src, source, what):
    """Two meters in a row from exposure 1 against cpt_meter_host; returns the exposure they leave."""
    present.set_exposure(gpu, 1.0)
    e = F(1.0)
    for key, permille, adapt in ((0.18, 500, 1.0), (0.5, 900, 0.25)):
        present.meter_exposure(gpu, source, key, permille, adapt)
        e, want_hist = present.meter_host(src, e, source, key, permille, adapt)
        got_e, got_hist = present.read_exposure(gpu)
        np.testing.assert_array_equal(got_hist, want_hist, err_msg=f"{what}: {source}")
        assert _bits(got_e) == _bits(e), (what, source, got_e, e)
    return e


# ----------------------------------------------------------------------- parity: synthetic states
@pytest.mark.parametrize("wh", pm.SHAPES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_synthetic_states_equal_the_host_hooks(gpu, wh):
    """Accumulators pushed in with write_accum on a full frame and on a row list (every other row,
    then the last), unsourced pixels and every special value among them; and the result of a
    one-level spatial filter of the full frame as the filtered source."""
    W, H = wh
    rows = np.unique(np.r_[np.arange(0, H, 2), H - 1]).astype(np.int32)
    for kind, n_rows in (("full", H), ("rows", len(rows))):
        accum = pm.synthetic_accum(W * n_rows, seed=300 + W + n_rows)
        gpu.set_frame(W, H, rows=None if kind == "full" else rows)
        e0, hist0 = present.read_exposure(gpu)
        assert e0 == F(1.0) and not hist0.any()                # a new frame: exposure 1, no meter yet
        gpu.write_accum(accum)
        _assert_presents(gpu, accum, "accum", 1.0, kind)
        e = _assert_meters(gpu, accum, "accum", kind)
        assert np.isfinite(e) and e > 0 and e != F(1.0)
        _assert_presents(gpu, accum, "accum", e, f"{kind}, metered")
        present.set_exposure(gpu, 0.37)
        assert present.read_exposure(gpu)[0] == F(0.37)
        _assert_presents(gpu, accum, "accum", 0.37, f"{kind}, set")
        assert present.last_present_ms(gpu) > 0.0
        if kind == "rows":
            _raises(CPT_ERR_STATE, lambda: present.present(gpu, "filtered"))
            continue
        rs = np.random.RandomState(W)
        normal = rs.standard_normal((W * H, 3)).astype(F)
        gpu.write_gbuffer(id=np.zeros(W * H, dtype=np.int32), normal=normal)
        gpu.filter_frame_spatial(levels=1)
        rgb, _ = gpu.read_filtered()
        _assert_presents(gpu, rgb, "filtered", 0.37, "filter result")
        e = _assert_meters(gpu, rgb, "filtered", "filter result")
        _assert_presents(gpu, rgb, "filtered", e, "filter result, metered")


# --------------------------------------------------------------------------- parity: a real frame
def _frame(gpu, sky, W, H, objs):
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED)


def test_a_real_frame_plain_and_filtered(gpu, sky):
    """S4 + cylinder at 64x48, 32 passes: the accumulator, and the frame after filter_frame_spatial."""
    W, H = 64, 48
    cam = camera_get_copy(scenes.camera_for(W, H))
    _frame(gpu, sky, W, H, tm.scene())
    gpu.render(cam, 32, DEPTH, sync=True, ordered=True)
    accum = gpu.read_accum()
    e = _assert_meters(gpu, accum, "accum", "render")
    _assert_presents(gpu, accum, "accum", e, "render")
    frame = present.present(gpu, "accum", "aces", WHITE, "srgb")
    assert frame.shape == (H, W, 4) and (frame[..., 3] == 255).all() and len(np.unique(frame[..., :3])) > 64
    gpu.gbuffer(cam, WALK)
    gpu.filter_frame_spatial()
    rgb, _ = gpu.read_filtered()
    e = _assert_meters(gpu, rgb, "filtered", "filtered render")
    _assert_presents(gpu, rgb, "filtered", e, "filtered render")
    assert (present.present(gpu, "filtered", "aces", WHITE, "srgb") != frame).any()


# ------------------------------------------------------------------ a chain with no host wait
def test_meter_present_meter_without_host_synchronisation(gpu):
    """meter, present (device only), meter again, queued back to back: the present sees the first
    meter's exposure and the second meter starts from it, with no read in between."""
    W, H = 130, 70
    accum = pm.synthetic_accum(W * H, seed=9)
    gpu.set_frame(W, H)
    gpu.write_accum(accum)
    present.set_exposure(gpu, 3.0)
    present.meter_exposure(gpu, "accum", 0.18, 500, 0.5)
    present.present(gpu, "accum", "reinhard", WHITE, "srgb", host=False)
    present.meter_exposure(gpu, "accum", 0.4, 250, 0.5)
    e1, _ = present.meter_host(accum, 3.0, "accum", 0.18, 500, 0.5)
    e2, hist2 = present.meter_host(accum, e1, "accum", 0.4, 250, 0.5)
    assert _bits(e1) != _bits(e2) != _bits(F(3.0))
    np.testing.assert_array_equal(present.read_present(gpu).reshape(-1, 4),
                                  present.present_host(accum, e1, "accum", "reinhard", WHITE, "srgb"))
    got_e, got_hist = present.read_exposure(gpu)
    assert _bits(got_e) == _bits(e2)
    np.testing.assert_array_equal(got_hist, hist2)


# -------------------------------------------------------------------------------- side effects
def test_the_calls_leave_the_rest_of_the_frame_alone(gpu, sky):
    """Accumulator, RNG planes, aux, moments, G-buffer, filter planes, the display's mix, counts and
    BGRA, the top-up plan and the reprojection history are bit-identical after set_exposure, both
    meters and both presents; a later render continues as without them."""
    W, H = 64, 48
    cam = camera_get_copy(scenes.camera_for(W, H))

    def start():
        _frame(gpu, sky, W, H, tm.scene())
        gpu.render_adaptive(cam, 4, 8, 2, 0.1, DEPTH, flags=WALK | CPT_RENDER_AUX)
        gpu.render_to_count(cam, 8, DEPTH, aux=True, sync=True, flags=WALK)
    start()
    gpu.render(cam, 2, DEPTH, accumulate=True, sync=True, ordered=True)
    want_next = gpu.read_accum(), gpu.read_rng()
    start()
    display = gpu.denoise_mix_history().copy()
    gpu.history_capture(cam, WALK)
    gpu.filter_frame_spatial()

    def state():
        g = gpu.read_gbuffer()
        n, d = gpu.read_aux()
        info = gpu.topup_info()
        rgb, var = gpu.read_filtered()
        bgra = np.zeros(16 * (H // 16) * W * 4, dtype=np.uint8)
        import torch
        buf = torch.zeros(bgra.size, dtype=torch.uint8, device="cuda")
        gpu.copy_bgra_device(buf.data_ptr(), bgra.size, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return [gpu.read_accum(), gpu.read_rng(), n, d, gpu.read_moments(), gpu.read_mix(), gpu.read_display_count(),
                buf.cpu().numpy(), g["id"], g["t"], g["normal"], g["albedo"], rgb, var,
                np.array([info["tiles"], info["pixels"], info["passes"]]), np.array([int(gpu.history_info()[0])]),
                np.frombuffer(gpu.history_info()[1].tobytes(), dtype=np.uint8)]
    before = state()
    assert (before[7].reshape(-1, W, 4) == display[:16 * (H // 16)]).all()
    present.set_exposure(gpu, 2.0)
    for source in ("accum", "filtered"):
        present.meter_exposure(gpu, source)
        frame = present.present(gpu, source)
        assert len(np.unique(frame[..., :3])) > 64
    for k, (a, b) in enumerate(zip(before, state())):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"state {k}")
    gpu.render(cam, 2, DEPTH, accumulate=True, sync=True, ordered=True)
    for a, b in zip((gpu.read_accum(), gpu.read_rng()), want_next):
        np.testing.assert_array_equal(_bits(a), _bits(b))


# -------------------------------------------------------------------------------------- errors
def test_errors_write_nothing(gpu, sky):
    W, H = 20, 12
    accum = pm.synthetic_accum(W * H, seed=77)
    with Renderer(0) as r:                                       # no frame
        for call in (lambda: present.set_exposure(r, 1.0), lambda: present.meter_exposure(r), lambda: present.read_exposure(r),
                     lambda: present.present(r), lambda: present.read_present(r), lambda: present.last_present_ms(r)):
            _raises(CPT_ERR_STATE, call)
    gpu.set_frame(W, H)
    gpu.write_accum(accum)
    _raises(CPT_ERR_STATE, lambda: present.read_present(gpu))    # nothing presented yet
    _raises(CPT_ERR_STATE, lambda: present.present(gpu, "filtered"))          # no filter result
    _raises(CPT_ERR_STATE, lambda: present.meter_exposure(gpu, "filtered"))
    _raises(CPT_ERR_STATE, lambda: present.read_present(gpu))
    present.set_exposure(gpu, 0.75)
    present.meter_exposure(gpu, "accum", 0.18, 500, 0.5)
    kept_frame = present.present(gpu, "accum", "aces", WHITE, "srgb")
    kept_e, kept_hist = present.read_exposure(gpu)

    def still_there():
        e, hist = present.read_exposure(gpu)
        assert _bits(e) == _bits(kept_e)
        np.testing.assert_array_equal(hist, kept_hist)
        np.testing.assert_array_equal(present.read_present(gpu), kept_frame)
    for bad in (dict(source=2), dict(source=-1), dict(tone=3), dict(tone=-1), dict(transfer=2), dict(white=0.0), dict(white=-2.0),
                dict(white=float("nan"))):
        _raises(CPT_ERR_INVALID_ARG, lambda: present.present(gpu, **bad))
        still_there()
    for bad in (dict(source=2), dict(key=0.0), dict(key=-1.0), dict(key=float("inf")), dict(key=float("nan")), dict(permille=-1),
                dict(permille=1001), dict(adapt=-0.5), dict(adapt=1.25), dict(adapt=float("nan"))):
        _raises(CPT_ERR_INVALID_ARG, lambda: present.meter_exposure(gpu, **bad))
        still_there()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _raises(CPT_ERR_INVALID_ARG, lambda: present.set_exposure(gpu, bad))
        still_there()
    _raises(CPT_ERR_STATE, lambda: present.present(gpu, "filtered"))
    still_there()
    # an adaptive render pending
    cam = camera_get_copy(scenes.camera_for(W, H))
    gpu.set_scene(scenes.scene_s4())
    gpu.set_env(sky)
    gpu.init_rng(SEED)
    gpu.adaptive_begin(cam, 4, 8, 2, 0.1, 4, flags=WALK)
    for call in (lambda: present.present(gpu), lambda: present.meter_exposure(gpu), lambda: present.set_exposure(gpu, 2.0)):
        _raises(CPT_ERR_STATE, call)
    while gpu.adaptive_step():
        pass
    still_there()


# ------------------------------------------------------------------------------------ ordering
def _meter_present_read(r, e):
    # (the module's functions call the library directly: the twin's wait after every call is made here)
    wait = r.synchronize if isinstance(r, ao.Synced) else (lambda: None)
    present.meter_exposure(r, "accum", 0.18, 500, 1.0)
    wait()
    present.present(r, "accum", "aces", WHITE, "srgb", host=False)
    wait()
    return present.read_present(r), present.read_exposure(r)   # the reads order themselves behind both


ORDER_CASE = ao.Case("render-meter_exposure-present", _meter_present_read, ao.IMAGE)


def test_meter_and_present_behind_a_render_in_flight(shared):
    """cpt_meter_exposure and cpt_present queued behind an unsynchronised cpt_render read the
    accumulator that render leaves: the bytes of the sequence synchronised after every call, which
    are the host hooks' on the finished accumulator."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    want, _, first = ao._run(ORDER_CASE, shared, twin=True)
    got, (t_launch, t_call, render_ms), _ = ao._run(ORDER_CASE, shared, twin=False)
    ao.assert_overlap(ORDER_CASE.name, t_launch, t_call, render_ms)
    ao._assert_same_bits(got, want)
    e, hist = present.meter_host(first[0], 1.0, "accum", 0.18, 500, 1.0)
    assert _bits(got["call.1.0"])[0] == _bits(e) and hist[:256].sum() > 0
    np.testing.assert_array_equal(got["call.1.1"], hist)
    np.testing.assert_array_equal(got["call.0"].reshape(-1, 4), present.present_host(first[0], e, "accum", "aces", WHITE, "srgb"))


# ----------------------------------------------------------------------------------- C++ API
def test_headless_present_equals_the_python_sequence(gpu, sky, tmp_path):
    """cpt_headless --present (PathTracer::MeterExposure / SetExposure / Present) writes the BGRA8
    frame the same calls give through the Python module: with plain --spp, and after --orbit 3
    --reproject --fill 16 --filter-spatial from the filter's result; with --display-reproject it is
    a usage error, and with two devices' tiles Present returns false."""
    from cpppathtracer_amd import build
    from test_gpu_reproject import orbit_cameras
    W, H, SPP, N, FILL = 48, 32, 2, 3, 16
    exe = build.build_examples()
    common = ["--scene", "s4", "--width", str(W), "--height", str(H), "--spp", str(SPP), "--depth", "4", "--seed", str(SEED)]

    def run(*args):
        out = tmp_path / "frame.bgra"
        r = subprocess.run([exe, *common, *args, "--bgra", str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(out, dtype=np.uint8).reshape(H, W, 4)
    cams = orbit_cameras(W, H, N)
    # plain --spp: metered, ACES, sRGB; a set exposure, Reinhard (the API's white, 4), linear
    _frame(gpu, sky, W, H, scenes.scene_s4())
    gpu.render(cams[0], SPP, 4, aux=True, sync=True, ordered=True)
    present.meter_exposure(gpu)
    want = present.present(gpu, "accum", "aces", 4.0, "srgb")
    assert len(np.unique(want[..., :3])) > 32
    np.testing.assert_array_equal(run("--present", "aces", "--exposure", "auto"), want)
    present.set_exposure(gpu, 0.5)
    np.testing.assert_array_equal(run("--present", "reinhard", "--exposure", "0.5", "--linear"),
                                  present.present(gpu, "accum", "reinhard", 4.0, "linear"))
    np.testing.assert_array_equal(run("--present", "clamp"), present.present_host(gpu.read_accum(), 1.0, "accum", "clamp", 4.0, "srgb")
                                  .reshape(H, W, 4))
    # the orbit, reprojected, topped up and filtered: the filter's result is presented
    _frame(gpu, sky, W, H, scenes.scene_s4())
    for k, cam in enumerate(cams):
        if k == 0:
            gpu.render(cam, SPP, 4, aux=True, sync=True, ordered=True)
            continue
        gpu.reproject_accum(cams[k - 1], cam, flags=WALK)
        gpu.render_to_count(cam, FILL, 4, aux=True, sync=True, flags=WALK)
    gpu.filter_frame_spatial()
    present.meter_exposure(gpu, "filtered")
    want = present.present(gpu, "filtered", "aces", 4.0, "srgb")
    got = run("--orbit", str(N), "--reproject", "--fill", str(FILL), "--filter-spatial", "--present", "aces", "--exposure", "auto")
    np.testing.assert_array_equal(got, want)
    assert (want != present.present(gpu, "accum", "aces", 4.0, "srgb")).any()
    # refusals
    bad = subprocess.run([exe, *common, "--orbit", "2", "--display-reproject", "on", "--present", "aces", "--bgra",
                          str(tmp_path / "no.bgra")], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--present" in bad.stderr and not (tmp_path / "no.bgra").exists()
    two = subprocess.run([exe, *common, "--devices", "2", "--present", "aces", "--bgra", str(tmp_path / "no.bgra")],
                         capture_output=True, text=True, timeout=300)
    assert two.returncode == 1 and "Present: Present: not available with SetDevices(n > 1)" in two.stderr, two.stdout + two.stderr
    assert not (tmp_path / "no.bgra").exists()
