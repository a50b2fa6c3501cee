"""cpt_bloom and cpt_present_bloom on the device against the host hooks on the same
header (which tests/test_bloom_model.py holds to the numpy restatement): every level of the pyramid
bit for bit and the presented bytes, on synthetic accumulators and filter results at every frame
shape and level count (640x360 for several workgroups of interior tiles and eight launched levels);
on a real frame; queued with no host wait; behind a render in flight; and through the example.
The calls' side effects, their errors (which write nothing) and the recorded contract of
cpt_bloom_capi.cpp's messages (tests/golden/capi_contract_bloom.json).
"""
import ctypes
import itertools
import json
import os
import subprocess

import bloom_model as bm
import numpy as np
import present_model as pm
import pytest
import test_gpu_async_order as ao
import tracked_reproject_model as tm

from cpppathtracer_amd import CptError, Renderer, antialias, bloom, camera_get_copy, present, scenes
from cpppathtracer_amd._lib import CPT_ERR_INVALID_ARG, CPT_ERR_STATE, CPT_RENDER_AUX, CPT_TRAVERSAL_ORDERED
from cpppathtracer_amd.types import OBJECT_DTYPE

pytestmark = pytest.mark.gpu

F = np.float32
DEPTH, SEED = 8, scenes.DEFAULT_SEED
WALK = CPT_TRAVERSAL_ORDERED
WHITE = 2.5
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_contract_bloom.json")
shared = ao.shared   # the ordering test's workload (a module fixture of test_gpu_async_order.py)
ALL_CURVES = list(itertools.product(pm.TONES, pm.TRANSFERS))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _raises(status, call):
    with pytest.raises(CptError) as e:
        call()
    assert e.value.status == status, e.value


def _cam(W, H):
    return camera_get_copy(scenes.camera_for(W, H))


def _assert_bloom(gpu, W, H, src, source, e, thr, L, what, curves=ALL_CURVES, intensity=0.3):
    """build() then every level against cpt_bloom_host, then the bytes against cpt_present_bloom_host."""
    bloom.build(gpu, source, thr, L)
    for l in range(1, L + 1):
        np.testing.assert_array_equal(_bits(bloom.read_level(gpu, l)), _bits(bloom.bloom_host(W, H, src, e, source, thr, L, l)),
                                      err_msg=f"{what}: U_{l} of {L}")
    for tone, transfer in curves:
        got = bloom.present_bloom(gpu, source, tone, WHITE, transfer, intensity)
        want = bloom.present_bloom_host(W, H, src, e, source, thr, L, intensity, tone, WHITE, transfer)
        np.testing.assert_array_equal(got, want, err_msg=f"{what}: {source}, {tone}, {transfer}, {L} levels")
        np.testing.assert_array_equal(present.read_present(gpu), want)
    return want


# ----------------------------------------------------------------------- parity: synthetic states
@pytest.mark.parametrize("L", bm.LEVELS)
@pytest.mark.parametrize("wh", bm.SHAPES + [(640, 360)], ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_synthetic_states_equal_the_host_hooks(gpu, wh, L):
    """Accumulators pushed in with write_accum, at a set and at a metered exposure, and the result
    of a one-level spatial filter as the second source."""
    W, H = wh
    large = W * H > 20000
    curves = [("aces", "srgb"), ("clamp", "linear")] if large else ALL_CURVES
    gpu.set_scene(tm.scene())
    gpu.set_frame(W, H)
    accum = pm.synthetic_accum(W * H, seed=500 + W + H)
    if large:   # a few highlights far above the rest, so that the coarse levels carry light across tiles
        accum[:: 9973, :3] *= F(4096)
    gpu.write_accum(accum)
    present.set_exposure(gpu, 0.37)
    _assert_bloom(gpu, W, H, accum, "accum", 0.37, 1.0, L, "set exposure", curves)
    assert bloom.last_bloom_ms(gpu) > 0.0
    present.meter_exposure(gpu)
    e, _ = present.read_exposure(gpu)
    frame = _assert_bloom(gpu, W, H, accum, "accum", e, 0.5, L, "metered", curves)
    if W * H >= 100:
        assert (frame != present.present(gpu, "accum", curves[-1][0], WHITE, curves[-1][1])).any()   # and the glow is seen
    rs = np.random.RandomState(W)
    gpu.write_gbuffer(id=np.zeros(W * H, dtype=np.int32), normal=rs.standard_normal((W * H, 3)).astype(F))
    gpu.filter_frame_spatial(levels=1)
    rgb, _ = gpu.read_filtered()
    _assert_bloom(gpu, W, H, rgb, "filtered", e, 0.5, L, "filter result", curves[:2])
    # the pyramid is the build's: presenting the other source keeps the glow of the filtered one
    got = bloom.present_bloom(gpu, "accum", "clamp", WHITE, "linear", 0.0)
    np.testing.assert_array_equal(got, present.present(gpu, "accum", "clamp", WHITE, "linear"))


def test_a_constant_plane_on_the_device(gpu):
    """The definition's identity through the kernels: U_l = (L - l + 1) v at every texel."""
    v = F(0.375)
    gpu.set_scene(tm.scene())
    for (W, H), L in (((65, 3), 8), ((130, 70), 5), ((640, 360), 8)):
        gpu.set_frame(W, H)
        gpu.write_accum(np.tile(np.array([v * 4, v * 4, v * 4, 4], dtype=F), (W * H, 1)))
        bloom.build(gpu, "accum", 0.0, L)
        for l in range(1, L + 1):
            assert (bloom.read_level(gpu, l) == F(L - l + 1) * v).all(), (W, H, L, l)


# --------------------------------------------------------------------------- parity: a real frame
def _frame(gpu, sky, W, H, objs):
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED)


def test_a_real_frame_plain_and_filtered(gpu, sky):
    """S4 + cylinder at 64x48, 32 passes: the accumulator, and the frame after filter_frame_spatial,
    at a metered exposure.  The meter brings the median luminance to 0.18 (within an eighth of an
    octave), so a threshold of 0.1 lets half the frame's pixels through: the glow is no vacuous case."""
    W, H = 64, 48
    cam = _cam(W, H)
    _frame(gpu, sky, W, H, tm.scene())
    gpu.render(cam, 32, DEPTH, sync=True, ordered=True)
    accum = gpu.read_accum()
    present.meter_exposure(gpu)
    e, _ = present.read_exposure(gpu)
    frame = _assert_bloom(gpu, W, H, accum, "accum", e, 0.1, 5, "render")
    assert (frame != present.present(gpu, "accum", ALL_CURVES[-1][0], WHITE, ALL_CURVES[-1][1])).any()
    gpu.gbuffer(cam, WALK)
    gpu.filter_frame_spatial()
    rgb, _ = gpu.read_filtered()
    _assert_bloom(gpu, W, H, rgb, "filtered", e, 0.1, 5, "filtered render")


def test_meter_bloom_present_without_host_synchronisation(gpu):
    """The three calls queued with no host wait between them: the bytes of the host sequence at
    the exposure the meter left."""
    W, H = 130, 70
    gpu.set_scene(tm.scene())
    gpu.set_frame(W, H)
    accum = pm.synthetic_accum(W * H, seed=91)
    gpu.write_accum(accum)
    present.meter_exposure(gpu, "accum", 0.18, 500, 1.0)
    bloom.build(gpu, "accum", 0.7, 6)
    bloom.present_bloom(gpu, "accum", "aces", WHITE, "srgb", 0.4, host=False)
    got = present.read_present(gpu)
    e, _ = pm.meter(accum, 1.0, pm.ACCUM)
    assert present.read_exposure(gpu)[0] == e
    np.testing.assert_array_equal(got, bloom.present_bloom_host(W, H, accum, e, "accum", 0.7, 6, 0.4, "aces", WHITE, "srgb"))


# -------------------------------------------------------------------------------- side effects
def test_the_calls_leave_the_rest_of_the_frame_alone(gpu, sky):
    """Accumulator, RNG planes, aux, moments, G-buffer, coverage, filter planes, the display's mix,
    counts and BGRA, the exposure and its histogram, the top-up plan and the reprojection history are
    bit-identical after both calls (only the pyramid and the present plane change); a later render
    continues as without them."""
    W, H = 64, 48
    cam = _cam(W, H)

    def start():
        _frame(gpu, sky, W, H, tm.scene())
        gpu.render_adaptive(cam, 4, 8, 2, 0.1, DEPTH, flags=WALK | CPT_RENDER_AUX)
        gpu.render_to_count(cam, 8, DEPTH, aux=True, sync=True, flags=WALK)
    start()
    gpu.render(cam, 2, DEPTH, accumulate=True, sync=True, ordered=True)
    want_next = gpu.read_accum(), gpu.read_rng()
    start()
    gpu.denoise_mix_history()
    gpu.history_capture(cam, WALK)
    antialias.coverage(gpu, cam, 4, 0.9, WALK)
    gpu.filter_frame_spatial()
    present.meter_exposure(gpu, "accum", 0.18, 500, 0.5)

    def state():
        g = gpu.read_gbuffer()
        n, d = gpu.read_aux()
        info = gpu.topup_info()
        rgb, var = gpu.read_filtered()
        e, hist = present.read_exposure(gpu)
        counts, flags = antialias.read_coverage(gpu)
        import torch
        nbytes = 16 * (H // 16) * W * 4
        buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        gpu.copy_bgra_device(buf.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return [gpu.read_accum(), gpu.read_rng(), n, d, gpu.read_moments(), gpu.read_mix(), gpu.read_display_count(),
                buf.cpu().numpy(), g["id"], g["t"], g["normal"], g["albedo"], counts, flags, rgb, var, np.array([e], dtype=F), hist,
                np.array([info["tiles"], info["pixels"], info["passes"]]), np.array([int(gpu.history_info()[0])]),
                np.frombuffer(gpu.history_info()[1].tobytes(), dtype=np.uint8)]
    before = state()
    for source in ("accum", "filtered"):
        bloom.build(gpu, source, 0.5, 8)
        frame = bloom.present_bloom(gpu, source)
        assert len(np.unique(frame[..., :3])) > 64
    for k, (a, b) in enumerate(zip(before, state())):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"state {k}")
    gpu.render(cam, 2, DEPTH, accumulate=True, sync=True, ordered=True)
    for a, b in zip((gpu.read_accum(), gpu.read_rng()), want_next):
        np.testing.assert_array_equal(_bits(a), _bits(b))


# -------------------------------------------------------------------------------------- errors
def test_errors_write_nothing(gpu, sky):
    W, H = 20, 12
    cam = _cam(W, H)
    nan, inf = float("nan"), float("inf")
    with Renderer(0) as r:                                       # no frame
        for call in (lambda: bloom.build(r), lambda: bloom.present_bloom(r), lambda: bloom.read_level(r, 1), lambda: bloom.last_bloom_ms(r)):
            _raises(CPT_ERR_STATE, call)
    gpu.set_scene(tm.scene())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.write_accum(pm.synthetic_accum(W * H, seed=78))
    _raises(CPT_ERR_STATE, lambda: bloom.read_level(gpu, 1))     # no pyramid yet
    _raises(CPT_ERR_STATE, lambda: bloom.present_bloom(gpu))
    _raises(CPT_ERR_STATE, lambda: bloom.build(gpu, "filtered"))   # no filter result
    _raises(CPT_ERR_STATE, lambda: bloom.present_bloom(gpu))     # and the refused build left no pyramid
    bloom.build(gpu, "accum", 0.5, 3)
    kept_levels = [bloom.read_level(gpu, l) for l in (1, 2, 3)]
    kept_frame = bloom.present_bloom(gpu, "accum", "aces", WHITE, "srgb", 0.5)
    kept_e = present.read_exposure(gpu)

    def still_there():
        for l, want in zip((1, 2, 3), kept_levels):
            np.testing.assert_array_equal(_bits(bloom.read_level(gpu, l)), _bits(want))
        _raises(CPT_ERR_INVALID_ARG, lambda: bloom.read_level(gpu, 4))   # still three levels
        np.testing.assert_array_equal(present.read_present(gpu), kept_frame)
        for a, b in zip(present.read_exposure(gpu), kept_e):
            np.testing.assert_array_equal(_bits(a), _bits(b))
    for bad in (dict(source=2), dict(source=-1), dict(levels=0), dict(levels=9), dict(levels=-3), dict(threshold=-0.5), dict(threshold=nan),
                dict(threshold=inf), dict(threshold=-inf)):
        _raises(CPT_ERR_INVALID_ARG, lambda: bloom.build(gpu, **{**dict(levels=5, threshold=0.1), **bad}))
        still_there()
    _raises(CPT_ERR_STATE, lambda: bloom.build(gpu, "filtered", 0.1, 5))
    still_there()
    for bad in (dict(source=2), dict(tone=3), dict(transfer=2), dict(white=0.0), dict(white=nan), dict(intensity=-1.0), dict(intensity=nan),
                dict(intensity=inf)):
        _raises(CPT_ERR_INVALID_ARG, lambda: bloom.present_bloom(gpu, **bad))
        still_there()
    _raises(CPT_ERR_STATE, lambda: bloom.present_bloom(gpu, "filtered"))
    _raises(CPT_ERR_INVALID_ARG, lambda: bloom.read_level(gpu, 0))
    still_there()
    # an adaptive render pending
    gpu.init_rng(SEED)
    gpu.adaptive_begin(cam, 4, 8, 2, 0.1, 4, flags=WALK)
    for call in (lambda: bloom.build(gpu, "accum", 0.1, 5), lambda: bloom.present_bloom(gpu)):
        _raises(CPT_ERR_STATE, call)
    while gpu.adaptive_step():
        pass
    for l, want in zip((1, 2, 3), kept_levels):
        np.testing.assert_array_equal(_bits(bloom.read_level(gpu, l)), _bits(want))
    # a row list: bloom needs the whole frame, and a new frame drops the old pyramid
    gpu.set_frame(W, H, rows=np.array([5, 2, 9], dtype=np.int32))
    _raises(CPT_ERR_STATE, lambda: bloom.build(gpu))
    _raises(CPT_ERR_STATE, lambda: bloom.present_bloom(gpu))
    _raises(CPT_ERR_STATE, lambda: bloom.read_level(gpu, 1))


def test_the_recorded_contract(gpu):
    """tests/golden/capi_contract_bloom.json replayed on the library itself (not through the
    binding): every step's status and cpt_last_error text."""
    from cpppathtracer_amd import _lib
    from cpppathtracer_amd.types import CAMERA_DTYPE
    L = _lib.load()
    with open(FIXTURE) as fh:
        recorded = {s[0]: (s[1], s[2]) for s in json.load(fh)}
    W = H = 16
    cam = np.array(_cam(W, H), dtype=CAMERA_DTYPE)
    objs = np.ascontiguousarray(scenes.scene_s3(), dtype=OBJECT_DTYPE)
    f32 = np.zeros(3 * W * H, dtype=F)
    ms = ctypes.c_float(0.0)
    fl = ctypes.c_float
    P = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    played = {}

    def step(c, what, status):
        text = L.cpt_last_error(c)
        played[what] = (status, (text.decode() if isinstance(text, bytes) else text) if status else "")
    c = ctypes.c_void_p()
    assert L.cpt_create(0, ctypes.byref(c)) == 0
    step(c, "new context: cpt_bloom, source 2", L.cpt_bloom(c, 2, fl(1.0), 6))
    step(c, "new context: cpt_bloom, levels 0", L.cpt_bloom(c, 0, fl(1.0), 0))
    step(c, "new context: cpt_bloom, levels 9", L.cpt_bloom(c, 0, fl(1.0), 9))
    step(c, "new context: cpt_bloom, threshold -0.5", L.cpt_bloom(c, 0, fl(-0.5), 6))
    step(c, "new context: cpt_bloom, threshold NaN", L.cpt_bloom(c, 0, fl(float("nan")), 6))
    step(c, "new context: cpt_bloom, threshold infinite", L.cpt_bloom(c, 0, fl(float("inf")), 6))
    step(c, "new context: cpt_bloom, no frame", L.cpt_bloom(c, 0, fl(1.0), 6))
    step(c, "new context: cpt_present_bloom, no frame", L.cpt_present_bloom(c, 0, 0, fl(4.0), 1, fl(0.25), None))
    step(c, "new context: cpt_read_bloom, no frame", L.cpt_read_bloom(c, 1, P(f32), W * H))
    step(c, "new context: cpt_last_bloom_ms, nothing yet", L.cpt_last_bloom_ms(c, ctypes.byref(ms)))
    assert L.cpt_set_frame(c, W, H, None, 0) == 0
    step(c, "frame: cpt_present_bloom, no pyramid", L.cpt_present_bloom(c, 0, 0, fl(4.0), 1, fl(0.25), None))
    step(c, "frame: cpt_read_bloom, no pyramid", L.cpt_read_bloom(c, 1, P(f32), W * H))
    step(c, "frame: cpt_bloom, filtered without a filter result", L.cpt_bloom(c, 1, fl(1.0), 6))
    step(c, "frame: cpt_bloom, valid", L.cpt_bloom(c, 0, fl(1.0), 3))
    step(c, "frame: cpt_read_bloom, level 0", L.cpt_read_bloom(c, 0, P(f32), W * H))
    step(c, "frame: cpt_read_bloom, level 4 of 3", L.cpt_read_bloom(c, 4, P(f32), W * H))
    step(c, "frame: cpt_read_bloom, capacity one short", L.cpt_read_bloom(c, 1, P(f32), 63))
    step(c, "frame: cpt_read_bloom, valid", L.cpt_read_bloom(c, 1, P(f32), 64))
    step(c, "frame: cpt_present_bloom, source 2", L.cpt_present_bloom(c, 2, 0, fl(4.0), 1, fl(0.25), None))
    step(c, "frame: cpt_present_bloom, intensity -1", L.cpt_present_bloom(c, 0, 0, fl(4.0), 1, fl(-1.0), None))
    step(c, "frame: cpt_present_bloom, intensity NaN", L.cpt_present_bloom(c, 0, 0, fl(4.0), 1, fl(float("nan")), None))
    step(c, "frame: cpt_present_bloom, filtered without a filter result", L.cpt_present_bloom(c, 1, 0, fl(4.0), 1, fl(0.25), None))
    step(c, "frame: cpt_present_bloom, valid", L.cpt_present_bloom(c, 0, 0, fl(4.0), 1, fl(0.25), None))
    step(c, "frame: cpt_last_bloom_ms, valid", L.cpt_last_bloom_ms(c, ctypes.byref(ms)))
    rows = np.arange(4, 12, dtype=np.int32)
    assert L.cpt_set_frame(c, W, H, P(rows), len(rows)) == 0
    step(c, "rows 4..11 of 16: cpt_bloom", L.cpt_bloom(c, 0, fl(1.0), 6))
    step(c, "rows 4..11 of 16: cpt_present_bloom", L.cpt_present_bloom(c, 0, 0, fl(4.0), 1, fl(0.25), None))
    rows = np.arange(H - 1, -1, -1, dtype=np.int32)
    assert L.cpt_set_frame(c, W, H, P(rows), len(rows)) == 0
    step(c, "rows reversed: cpt_bloom", L.cpt_bloom(c, 0, fl(1.0), 6))
    assert L.cpt_destroy(c) == 0
    with Renderer(0) as r:
        r.set_scene(objs)
        r.set_frame(W, H)
        r.init_rng(SEED)
        r.adaptive_begin(cam, 4, 8, 2, 0.1, 1)
        step(r._ctx, "adaptive render pending: cpt_bloom", L.cpt_bloom(r._ctx, 0, fl(1.0), 6))
        step(r._ctx, "adaptive render pending: cpt_present_bloom", L.cpt_present_bloom(r._ctx, 0, 0, fl(4.0), 1, fl(0.25), None))
        while r.adaptive_step():
            pass
    assert list(played) == list(recorded)
    for what in recorded:
        assert played[what] == recorded[what], what


# ------------------------------------------------------------------------------------ ordering
def _bloom_present_read(r, e):
    # (the module's functions call the library directly: the twin's wait after every call is made here)
    wait = r.synchronize if isinstance(r, ao.Synced) else (lambda: None)
    present.meter_exposure(r)
    wait()
    bloom.build(r, "accum", 0.1, 6)   # below the metered median of 0.18: light passes
    wait()
    bloom.present_bloom(r, "accum", "aces", WHITE, "srgb", 0.5, host=False)
    wait()
    return present.read_present(r), bloom.read_level(r, 1), bloom.read_level(r, 6)   # the reads order themselves behind the calls


ORDER_CASE = ao.Case("render-meter-bloom-present_bloom", _bloom_present_read, ao.IMAGE)


def test_bloom_and_present_bloom_behind_a_render_in_flight(shared):
    """cpt_meter_exposure, cpt_bloom and cpt_present_bloom queued behind an unsynchronised
    cpt_render read the accumulator that render leaves: the bytes of the sequence synchronised after
    every call, which are the host hook's on the finished accumulator."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    want, _, first = ao._run(ORDER_CASE, shared, twin=True)
    got, (t_launch, t_call, render_ms), _ = ao._run(ORDER_CASE, shared, twin=False)
    ao.assert_overlap(ORDER_CASE.name, t_launch, t_call, render_ms)
    ao._assert_same_bits(got, want)
    e, _ = pm.meter(first[0], 1.0, pm.ACCUM)
    np.testing.assert_array_equal(got["call.0"], bloom.present_bloom_host(ao.W, ao.H, first[0], e, "accum", 0.1, 6, 0.5, "aces", WHITE, "srgb"))
    assert got["call.2"].any()


# ----------------------------------------------------------------------------------- C++ API
def test_headless_bloom_equals_the_python_sequence(gpu, sky, tmp_path):
    """cpt_headless --present aces --exposure auto --bloom 0.1,5,0.4 (PathTracer::BuildBloom /
    PresentBloom) writes the frame the same calls give through the Python module; --bloom without
    --present, with --aa and with a bad level count are usage errors."""
    from cpppathtracer_amd import build
    W, H, SPP = 48, 32, 2
    exe = build.build_examples()
    common = ["--scene", "s4", "--width", str(W), "--height", str(H), "--spp", str(SPP), "--depth", "4", "--seed", str(SEED)]
    out = tmp_path / "frame.bgra"
    r = subprocess.run([exe, *common, "--present", "aces", "--exposure", "auto", "--bloom", "0.1,5,0.4", "--bgra", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, dtype=np.uint8).reshape(H, W, 4)
    cam = _cam(W, H)
    _frame(gpu, sky, W, H, scenes.scene_s4())
    gpu.render(cam, SPP, 4, aux=True, sync=True, ordered=True)
    present.meter_exposure(gpu)
    bloom.build(gpu, "accum", 0.1, 5)
    want = bloom.present_bloom(gpu, "accum", "aces", 4.0, "srgb", 0.4)
    np.testing.assert_array_equal(got, want)
    assert (want != present.present(gpu, "accum", "aces", 4.0, "srgb")).any()
    no = tmp_path / "no.bgra"
    for args in (["--bloom", "0.5"], ["--present", "aces", "--aa", "4", "--bloom", "0.5"], ["--present", "aces", "--bloom", "0.5,9"],
                 ["--present", "aces", "--bloom", "-1"], ["--present", "aces", "--bloom", "0.5,3,0.2,7"]):
        bad = subprocess.run([exe, *common, *args, "--bgra", str(no)], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and "--bloom" in bad.stderr and not no.exists(), args
