"""cpt_aa_coverage and cpt_present_aa on the GPU: the coverage words held bit for bit
to cpt_aa_coverage_host fed with the device's G-buffer and with sub-sample hits obtained another way
(cpt_trace_rays on cpt_aa_rays_host's rays), for frames from 1x1 up, both sample counts, the three
walks and edge lists that are empty, shorter than a wave's pixel group and longer than a workgroup's
share; the presented bytes held to cpt_present_aa_host (which tests/test_antialias_model.py holds to
the numpy restatement) and, on flat colours, to the exact supersample; what the calls must leave
alone, their errors, their place in the stream's order and the recorded contract of their messages;
and the C++ API through the headless example.
"""
import ctypes
import itertools
import json
import os
import subprocess

import antialias_model as am
import numpy as np
import present_model as pm
import pytest
import test_gpu_async_order as ao
import tracked_reproject_model as tm

from cpppathtracer_amd import CptError, Renderer, antialias, camera_get_copy, present, scenes
from cpppathtracer_amd._lib import (CPT_ERR_INVALID_ARG, CPT_ERR_STATE, CPT_RENDER_AUX, CPT_TRAVERSAL_ORDERED,
                                    CPT_TRAVERSAL_PLAIN_LEAVES)
from cpppathtracer_amd.types import DIFFUSE, OBJECT_DTYPE, PLATFORM, SPHERE, make_material, make_object

pytestmark = pytest.mark.gpu

F = np.float32
DEPTH, SEED = 8, scenes.DEFAULT_SEED
WALK = CPT_TRAVERSAL_ORDERED
WHITE = 2.5
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_contract_antialias.json")
shared = ao.shared   # the ordering test's workload (a module fixture of test_gpu_async_order.py)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _raises(status, call):
    with pytest.raises(CptError) as e:
        call()
    assert e.value.status == status, e.value


def _cam(W, H):
    return camera_get_copy(scenes.camera_for(W, H))


def _sub_hits(r, cam, W, H, S, walk, pixels):
    """The first hits of the S x S sub-samples of `pixels` (flat indices) through cpt_trace_rays on
    cpt_aa_rays_host's rays: (sub_id [npix, S^2], sub_normal [npix, S^2, 3]), zeros elsewhere."""
    s2 = S * S
    sub_id = np.zeros((W * H, s2), dtype=np.int32)
    sub_n = np.zeros((W * H, s2, 3), dtype=F)
    pixels = np.asarray(pixels, dtype=np.int64)
    if len(pixels):
        O = np.zeros((len(pixels), s2, 3), dtype=F)
        D = np.zeros_like(O)
        for n, p in enumerate(pixels):
            O[n], D[n] = antialias.rays_host(cam, W, H, S, int(p % W), int(p // W))
        hit = r.trace_rays(O.reshape(-1, 3), D.reshape(-1, 3), flags=walk)
        sub_id[pixels] = hit["id"].reshape(-1, s2)
        sub_n[pixels] = hit["normal"].reshape(-1, s2, 3)
    return sub_id, sub_n


def _expected_coverage(r, cam, W, H, S, cos, walk):
    """cpt_aa_coverage_host on the context's G-buffer (the one the call under test left) and the
    independently traced sub-sample hits of its edge pixels: (counts, flags, sub_id)."""
    g = r.read_gbuffer()
    blank_id, blank_n = np.zeros((W * H, S * S), dtype=np.int32), np.zeros((W * H, S * S, 3), dtype=F)
    _, flags = antialias.coverage_host(W, H, S, cos, g["id"], g["normal"], blank_id, blank_n)   # the edge bit needs no hits
    edge = np.flatnonzero(flags.reshape(-1) & am.EDGE)
    sub_id, sub_n = _sub_hits(r, cam, W, H, S, walk, edge)
    counts, flags = antialias.coverage_host(W, H, S, cos, g["id"], g["normal"], sub_id, sub_n)
    return counts, flags, sub_id


def _assert_coverage(r, cam, W, H, cos, walk, what):
    """Both sample counts; returns the numbers of edge pixels seen."""
    edges = []
    for S in (2, 4):
        antialias.coverage(r, cam, S, cos, walk)
        counts, flags = antialias.read_coverage(r)
        want_counts, want_flags, _ = _expected_coverage(r, cam, W, H, S, cos, walk)
        np.testing.assert_array_equal(flags, want_flags, err_msg=f"{what}: flags, S = {S}")
        np.testing.assert_array_equal(counts, want_counts, err_msg=f"{what}: counts, S = {S}")
        assert (counts.sum(axis=2) == S * S).all()
        assert antialias.last_aa_ms(r) > 0.0
        edges.append(int((flags & am.EDGE).astype(bool).sum()))
    assert edges[0] == edges[1]
    return edges[0]


# ------------------------------------------------------------------------------ coverage: scenes
def _one_small_sphere():
    return np.array([make_object(SPHERE, make_material(DIFFUSE, kd=(0.5, 0.5, 0.5)), center=(0.0, 10.0, 0.0), radius=4.0)],
                    dtype=OBJECT_DTYPE)


def _floor_only():
    s4 = scenes.scene_s4()
    floor = s4[[int(o["type"]) == PLATFORM for o in s4]]
    assert len(floor) == 1
    return floor


SMALL = [(1, 1), (2, 2), (3, 5), (63, 2), (65, 3)]
WALKS = {"reference": 0, "ordered": CPT_TRAVERSAL_ORDERED, "plain": CPT_TRAVERSAL_ORDERED | CPT_TRAVERSAL_PLAIN_LEAVES}


@pytest.mark.parametrize("walk", WALKS)
def test_coverage_equals_the_host_hook_on_every_frame_size(gpu, walk):
    """S4 + cylinder at the small frames (every border case) and at 64x48; both crease thresholds."""
    gpu.set_scene(tm.scene())
    seen = 0
    for W, H in SMALL + [(64, 48)]:
        gpu.set_frame(W, H)
        for cos in (0.9, -1.0):
            seen += _assert_coverage(gpu, _cam(W, H), W, H, cos, WALKS[walk], f"s4+cylinder {W}x{H} cos {cos}")
    assert seen > 300


@pytest.mark.parametrize("walk", ["reference", "ordered"])
def test_coverage_with_an_empty_and_a_short_edge_list(gpu, walk):
    """Sky only and floor only have no edge pixel (nothing is traced, every word is all on itself);
    one small sphere gives fewer edge pixels than a wave holds."""
    W, H = 64, 48
    cam = _cam(W, H)
    for name, objs in (("sky", np.zeros(0, dtype=OBJECT_DTYPE)), ("floor", _floor_only())):
        gpu.set_scene(objs)
        gpu.set_frame(W, H)
        assert _assert_coverage(gpu, cam, W, H, 0.9, WALKS[walk], name) == 0
        counts, flags = antialias.read_coverage(gpu)
        assert not flags.any() and (counts[..., am.SELF] == 16).all()
    gpu.set_scene(_one_small_sphere())
    for W, H in ((20, 14), (130, 70)):
        gpu.set_frame(W, H)
        n = _assert_coverage(gpu, _cam(W, H), W, H, 0.9, WALKS[walk], f"one sphere {W}x{H}")
        assert 0 < n < 16 if (W, H) == (20, 14) else n > 16   # S = 2: a wave holds 16 pixels


def test_coverage_with_a_long_edge_list_and_a_capped_grid(gpu):
    """S1000 at 130x70: thousands of edge pixels.  With the persistent grid capped at one workgroup
    (cpt_set_debug_grid) every lane takes many sub-samples in turn; the words are the same."""
    W, H = 130, 70
    cam = _cam(W, H)
    gpu.set_scene(scenes.scene_s1000())
    gpu.set_frame(W, H)
    n = _assert_coverage(gpu, cam, W, H, 0.9, WALK, "s1000 130x70")
    assert n * 16 > 4 * 1024      # more than one workgroup's share of sub-samples, several times over
    want = antialias.read_coverage(gpu)
    try:
        gpu.set_debug_grid(1, 0)
        antialias.coverage(gpu, cam, 4, 0.9, WALK)
        got = antialias.read_coverage(gpu)
    finally:
        gpu.set_debug_grid(0, 0)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    _assert_coverage(gpu, cam, W, H, 0.9, 0, "s1000 130x70, reference walk")


def test_coverage_on_a_tree_larger_than_the_lds_image(gpu):
    """The scene of the G-buffer's HYB fixture (2600 primitives: the 4-wide tree's lower part is read
    from global memory), at its camera."""
    import gbuffer_model as gm
    objs, cam, _ = gm.fixtures()["fuzz_hyb_48x32"]
    W, H = 48, 32
    gpu.set_scene(objs)
    gpu.set_frame(W, H)
    assert _assert_coverage(gpu, camera_get_copy(cam), W, H, 0.9, WALK, "hyb") > 100


def test_coverage_after_an_object_edit_equals_a_fresh_context(gpu):
    W, H = 64, 48
    cam = _cam(W, H)
    objs = tm.scene()
    gpu.set_scene(objs)
    gpu.set_frame(W, H)
    antialias.coverage(gpu, cam, 4, 0.9, WALK)
    before = antialias.read_coverage(gpu)
    moved = np.array(objs, copy=True)
    moved[tm.CYL]["center"] = np.asarray((-20.0, 12.0, 30.0), dtype=F)
    gpu.update_objects([tm.CYL], moved[[tm.CYL]])
    antialias.coverage(gpu, cam, 4, 0.9, WALK)
    after = antialias.read_coverage(gpu)
    assert (after[0] != before[0]).any()
    with Renderer(0) as fresh:
        fresh.set_scene(moved)
        fresh.set_frame(W, H)
        antialias.coverage(fresh, cam, 4, 0.9, WALK)
        want = antialias.read_coverage(fresh)
    np.testing.assert_array_equal(after[0], want[0])
    np.testing.assert_array_equal(after[1], want[1])


# ------------------------------------------------------------------------- flat colours, exactly
@pytest.fixture(scope="module")
def flat(gpu):
    """S4 + cylinder at 64x48 with normal_cos = -1 and an accumulator of count 1 whose colour is a
    palette entry per object id (every component a multiple of 1/8): the frame is noise-free, and
    the mean of a pixel's sub-samples' colours, the exact S x S supersample, is an exact float."""
    W, H, S = am.FLAT_W, am.FLAT_H, 4   # the frame test_antialias_model.py checks the 5% condition on, without a GPU
    cam = _cam(W, H)
    gpu.set_scene(tm.scene())
    gpu.set_frame(W, H)
    antialias.coverage(gpu, cam, S, am.FLAT_COS, WALK)
    counts, flags = antialias.read_coverage(gpu)
    g = gpu.read_gbuffer()
    palette = np.array([[1, 0.125, 0.25], [0, 0.5, 1], [0.875, 0.75, 0], [0.25, 1, 0.375], [0.625, 0, 0.875], [0.125, 0.25, 0.5]],
                       dtype=F)   # objects 0..4, then the sky (id -1)
    sub_id, _ = _sub_hits(gpu, cam, W, H, S, WALK, np.arange(W * H))
    exact = palette[sub_id].sum(axis=1, dtype=F) / F(S * S)     # exact sums of multiples of 1/8
    accum = np.concatenate([palette[g["id"]], np.ones((W * H, 1), dtype=F)], axis=1).astype(F)
    gpu.write_accum(accum)
    want = (F(255.99) * exact).astype(np.int32).astype(np.uint8)[:, ::-1]   # B, G, R
    aa = antialias.present_aa(gpu, "accum", "clamp", WHITE, "linear").reshape(-1, 4)
    plain = present.present(gpu, "accum", "clamp", WHITE, "linear").reshape(-1, 4)
    return dict(flags=flags.reshape(-1), counts=counts, want=want, aa=aa, plain=plain)


def test_flat_colours_present_the_exact_supersample(flat):
    edge = (flat["flags"] & am.EDGE) != 0
    unmatched = (flat["flags"] & am.UNMATCHED) != 0
    print(f"edge pixels {edge.sum()}, unmatched {unmatched.sum()}")
    assert edge.sum() > 200 and unmatched.sum() <= am.FLAT_UNMATCHED_SHARE * edge.sum()
    np.testing.assert_array_equal(flat["aa"][~unmatched, :3], flat["want"][~unmatched])
    assert (flat["aa"][:, 3] == 255).all()
    np.testing.assert_array_equal(flat["aa"][~edge], flat["plain"][~edge])


def test_flat_colours_squared_error_is_lower_than_without(flat):
    want = flat["want"].astype(np.float64)
    sse_aa = ((flat["aa"][:, :3] - want) ** 2).sum()
    sse_plain = ((flat["plain"][:, :3] - want) ** 2).sum()
    print(f"summed squared error against the supersample: antialiased {sse_aa:.0f}, plain {sse_plain:.0f}")
    assert sse_aa < sse_plain


# --------------------------------------------------------------------- bytes equal to the host hook
def _frame(gpu, sky, W, H, objs):
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(SEED)


def _assert_presents(gpu, W, H, S, src, source, counts, e, what):
    self_only = counts[..., am.SELF] == S * S
    for tone, transfer in itertools.product(pm.TONES, pm.TRANSFERS):
        got = antialias.present_aa(gpu, source, tone, WHITE, transfer)
        want = antialias.present_aa_host(W, H, S, src, counts, e, source, tone, WHITE, transfer)
        np.testing.assert_array_equal(got, want, err_msg=f"{what}: {source}, {tone}, {transfer}")
        np.testing.assert_array_equal(present.read_present(gpu), want)
        plain = present.present(gpu, source, tone, WHITE, transfer)
        np.testing.assert_array_equal(got[self_only], plain[self_only])
        assert (got[~self_only] != plain[~self_only]).any()


def test_a_real_frame_plain_and_filtered(gpu, sky):
    """S4 + cylinder at 64x48, 32 passes: the accumulator, and the frame after filter_frame_spatial
    (which reads the G-buffer the coverage call left), at a metered exposure."""
    W, H = 64, 48
    cam = _cam(W, H)
    _frame(gpu, sky, W, H, tm.scene())
    gpu.render(cam, 32, DEPTH, sync=True, ordered=True)
    accum = gpu.read_accum()
    for S in (2, 4):
        antialias.coverage(gpu, cam, S, 0.9, WALK)
        counts, _ = antialias.read_coverage(gpu)
        present.set_exposure(gpu, 1.0)
        _assert_presents(gpu, W, H, S, accum, "accum", counts, 1.0, f"render, S = {S}")
    present.meter_exposure(gpu)
    e, _ = present.read_exposure(gpu)
    _assert_presents(gpu, W, H, 4, accum, "accum", counts, e, "render, metered")
    gpu.filter_frame_spatial()
    rgb, _ = gpu.read_filtered()
    _assert_presents(gpu, W, H, 4, rgb, "filtered", counts, e, "filtered render")


def test_odd_frames_present_to_the_host_hooks_bytes(gpu):
    """Frames whose pixel count is no multiple of four (the kernel's tail) and of one row or column."""
    gpu.set_scene(tm.scene())
    for W, H in SMALL + [(130, 70)]:
        gpu.set_frame(W, H)
        accum = pm.synthetic_accum(W * H, seed=W + H)
        gpu.write_accum(accum)
        antialias.coverage(gpu, _cam(W, H), 4, 0.9, WALK)
        counts, _ = antialias.read_coverage(gpu)
        for tone, transfer in (("aces", "srgb"), ("clamp", "linear")):
            np.testing.assert_array_equal(antialias.present_aa(gpu, "accum", tone, WHITE, transfer),
                                          antialias.present_aa_host(W, H, 4, accum, counts, 1.0, "accum", tone, WHITE, transfer),
                                          err_msg=f"{W}x{H} {tone} {transfer}")


# -------------------------------------------------------------------------------- side effects
def test_the_calls_leave_the_rest_of_the_frame_alone(gpu, sky):
    """Accumulator, RNG planes, aux, moments, filter planes, the display's mix, counts and BGRA, the
    exposure and its histogram, the top-up plan and the reprojection history are bit-identical after
    both calls (only the G-buffer and the present plane change); a later render continues as
    without them."""
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
    gpu.filter_frame_spatial()
    present.meter_exposure(gpu, "accum", 0.18, 500, 0.5)

    def state():
        n, d = gpu.read_aux()
        info = gpu.topup_info()
        rgb, var = gpu.read_filtered()
        e, hist = present.read_exposure(gpu)
        bgra = np.zeros(16 * (H // 16) * W * 4, dtype=np.uint8)
        import torch
        buf = torch.zeros(bgra.size, dtype=torch.uint8, device="cuda")
        gpu.copy_bgra_device(buf.data_ptr(), bgra.size, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return [gpu.read_accum(), gpu.read_rng(), n, d, gpu.read_moments(), gpu.read_mix(), gpu.read_display_count(),
                buf.cpu().numpy(), rgb, var, np.array([e], dtype=F), hist,
                np.array([info["tiles"], info["pixels"], info["passes"]]), np.array([int(gpu.history_info()[0])]),
                np.frombuffer(gpu.history_info()[1].tobytes(), dtype=np.uint8)]
    before = state()
    for source in ("accum", "filtered"):
        antialias.coverage(gpu, cam, 4, 0.9, WALK)
        frame = antialias.present_aa(gpu, source)
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
    with Renderer(0) as r:                                       # no scene, no frame
        for call in (lambda: antialias.coverage(r, cam), lambda: antialias.read_coverage(r), lambda: antialias.present_aa(r),
                     lambda: antialias.last_aa_ms(r)):
            _raises(CPT_ERR_STATE, call)
    gpu.set_scene(tm.scene())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.write_accum(pm.synthetic_accum(W * H, seed=78))
    _raises(CPT_ERR_STATE, lambda: antialias.read_coverage(gpu))   # no coverage yet
    _raises(CPT_ERR_STATE, lambda: antialias.present_aa(gpu))
    antialias.coverage(gpu, cam, 2, 0.9, WALK)
    kept_cov = antialias.read_coverage(gpu)
    kept_frame = antialias.present_aa(gpu, "accum", "aces", WHITE, "srgb")
    kept_g = gpu.read_gbuffer()

    def still_there():
        for a, b in zip(antialias.read_coverage(gpu), kept_cov):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(present.read_present(gpu), kept_frame)
        g = gpu.read_gbuffer()
        for k in kept_g:
            np.testing.assert_array_equal(_bits(g[k]), _bits(kept_g[k]))
    other = camera_get_copy(scenes.make_camera(W, H, origin=(90.0, 60.0, -40.0), look_at=(0.0, 0.0, 0.0)))   # a G-buffer there would differ
    for bad in (dict(samples=3), dict(samples=0), dict(samples=8), dict(normal_cos=1.5), dict(normal_cos=-1.25),
                dict(normal_cos=float("nan")), dict(flags=0x1), dict(flags=WALK | 0x8)):
        _raises(CPT_ERR_INVALID_ARG, lambda: antialias.coverage(gpu, other, **bad))
        still_there()
    _raises(CPT_ERR_INVALID_ARG, lambda: antialias.coverage(gpu, _cam(W + 1, H)))
    still_there()
    for bad in (dict(source=2), dict(source=-1), dict(tone=3), dict(transfer=2), dict(white=0.0), dict(white=float("nan"))):
        _raises(CPT_ERR_INVALID_ARG, lambda: antialias.present_aa(gpu, **bad))
        still_there()
    _raises(CPT_ERR_STATE, lambda: antialias.present_aa(gpu, "filtered"))   # no filter result
    still_there()
    # an adaptive render pending
    gpu.init_rng(SEED)
    gpu.adaptive_begin(cam, 4, 8, 2, 0.1, 4, flags=WALK)
    for call in (lambda: antialias.coverage(gpu, other), lambda: antialias.present_aa(gpu)):
        _raises(CPT_ERR_STATE, call)
    while gpu.adaptive_step():
        pass
    still_there()
    # a row list: the coverage needs the whole frame, and a new frame drops the old coverage
    gpu.set_frame(W, H, rows=np.array([5, 2, 9], dtype=np.int32))
    _raises(CPT_ERR_STATE, lambda: antialias.coverage(gpu, cam))
    _raises(CPT_ERR_STATE, lambda: antialias.present_aa(gpu))
    _raises(CPT_ERR_STATE, lambda: antialias.read_coverage(gpu))


def test_the_recorded_contract(gpu):
    """tests/golden/capi_contract_antialias.json replayed on the library itself (not through the
    binding): every step's status and cpt_last_error text."""
    from cpppathtracer_amd import _lib
    from cpppathtracer_amd.types import CAMERA_DTYPE
    L = _lib.load()
    with open(FIXTURE) as fh:
        recorded = {s[0]: (s[1], s[2]) for s in json.load(fh)}
    W = H = 16
    cam, cam8 = (np.array(_cam(w, w), dtype=CAMERA_DTYPE) for w in (16, 8))
    objs = np.ascontiguousarray(scenes.scene_s3(), dtype=OBJECT_DTYPE)
    u8 = np.zeros(16 * W * H, dtype=np.uint8)
    ms = ctypes.c_float(0.0)
    fl = ctypes.c_float
    P = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    played = {}

    def ctx():
        c = ctypes.c_void_p()
        assert L.cpt_create(0, ctypes.byref(c)) == 0
        return c

    def step(c, what, status):
        text = L.cpt_last_error(c)
        played[what] = (status, (text.decode() if isinstance(text, bytes) else text) if status else "")
    c = ctx()
    step(c, "new context: cpt_aa_coverage, NULL camera", L.cpt_aa_coverage(c, None, 0, 4, fl(0.5)))
    step(c, "new context: cpt_aa_coverage, samples 3", L.cpt_aa_coverage(c, P(cam), 0, 3, fl(0.5)))
    step(c, "new context: cpt_aa_coverage, normal_cos 1.5", L.cpt_aa_coverage(c, P(cam), 0, 4, fl(1.5)))
    step(c, "new context: cpt_aa_coverage, normal_cos NaN", L.cpt_aa_coverage(c, P(cam), 0, 4, fl(float("nan"))))
    step(c, "new context: cpt_aa_coverage, a stray flag", L.cpt_aa_coverage(c, P(cam), 0x1, 4, fl(0.5)))
    step(c, "new context: cpt_aa_coverage, no scene", L.cpt_aa_coverage(c, P(cam), 0, 4, fl(0.5)))
    step(c, "new context: cpt_read_aa_coverage, no frame", L.cpt_read_aa_coverage(c, P(u8), P(u8), W * H))
    step(c, "new context: cpt_present_aa, no frame", L.cpt_present_aa(c, 0, 0, fl(4.0), 1, None))
    step(c, "new context: cpt_last_aa_ms, nothing yet", L.cpt_last_aa_ms(c, ctypes.byref(ms)))
    assert L.cpt_set_scene(c, P(objs), len(objs)) == 0
    step(c, "scene only: cpt_aa_coverage, no frame", L.cpt_aa_coverage(c, P(cam), 0, 4, fl(0.5)))
    assert L.cpt_set_frame(c, W, H, None, 0) == 0
    step(c, "scene and frame: cpt_aa_coverage, camera of another size", L.cpt_aa_coverage(c, P(cam8), 0, 4, fl(0.5)))
    step(c, "scene and frame: cpt_read_aa_coverage, no coverage", L.cpt_read_aa_coverage(c, P(u8), P(u8), W * H))
    step(c, "scene and frame: cpt_present_aa, no coverage", L.cpt_present_aa(c, 0, 0, fl(4.0), 1, None))
    step(c, "scene and frame: cpt_present_aa, source 2", L.cpt_present_aa(c, 2, 0, fl(4.0), 1, None))
    step(c, "scene and frame: cpt_aa_coverage, valid", L.cpt_aa_coverage(c, P(cam), 0, 4, fl(0.5)))
    step(c, "scene and frame: cpt_read_aa_coverage, capacity one short", L.cpt_read_aa_coverage(c, P(u8), P(u8), W * H - 1))
    step(c, "scene and frame: cpt_present_aa, filtered without a filter result", L.cpt_present_aa(c, 1, 0, fl(4.0), 1, None))
    step(c, "scene and frame: cpt_present_aa, valid", L.cpt_present_aa(c, 0, 0, fl(4.0), 1, None))
    step(c, "scene and frame: cpt_last_aa_ms, valid", L.cpt_last_aa_ms(c, ctypes.byref(ms)))
    rows = np.arange(4, 12, dtype=np.int32)
    assert L.cpt_set_frame(c, W, H, P(rows), len(rows)) == 0
    step(c, "rows 4..11 of 16: cpt_aa_coverage", L.cpt_aa_coverage(c, P(cam), 0, 4, fl(0.5)))
    step(c, "rows 4..11 of 16: cpt_present_aa", L.cpt_present_aa(c, 0, 0, fl(4.0), 1, None))
    assert L.cpt_destroy(c) == 0
    with Renderer(0) as r:
        r.set_scene(objs)
        r.set_frame(W, H)
        r.init_rng(SEED)
        r.adaptive_begin(cam, 4, 8, 2, 0.1, 1)
        step(r._ctx, "adaptive render pending: cpt_aa_coverage", L.cpt_aa_coverage(r._ctx, P(cam), 0, 4, fl(0.5)))
        step(r._ctx, "adaptive render pending: cpt_present_aa", L.cpt_present_aa(r._ctx, 0, 0, fl(4.0), 1, None))
        while r.adaptive_step():
            pass
    assert list(played) == list(recorded)
    for what in recorded:
        assert played[what] == recorded[what], what


# ------------------------------------------------------------------------------------ ordering
def _coverage_present_read(r, e):
    # (the module's functions call the library directly: the twin's wait after every call is made here)
    wait = r.synchronize if isinstance(r, ao.Synced) else (lambda: None)
    antialias.coverage(r, e.cam, 4, 0.9, WALK)
    wait()
    antialias.present_aa(r, "accum", "aces", WHITE, "srgb", host=False)
    wait()
    return present.read_present(r), antialias.read_coverage(r)   # the reads order themselves behind both


# the module's workload shows one object at its camera (no edge pixel: the CPU model says so), so the
# case renders the whole S1000 instead, which has edges in 1795 of its 2560 pixels
ORDER_CASE = ao.Case("render-aa_coverage-present_aa", _coverage_present_read, ao.IMAGE,
                     before=lambda r, e: r.set_scene(scenes.scene_s1000()), pinned=False)


def test_coverage_and_present_aa_behind_a_render_in_flight(shared):
    """cpt_aa_coverage and cpt_present_aa queued behind an unsynchronised cpt_render read the
    accumulator that render leaves: the bytes of the sequence synchronised after every call, which
    are the host hook's on the finished accumulator."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    want, _, first = ao._run(ORDER_CASE, shared, twin=True)
    got, (t_launch, t_call, render_ms), _ = ao._run(ORDER_CASE, shared, twin=False)
    ao.assert_overlap(ORDER_CASE.name, t_launch, t_call, render_ms)
    ao._assert_same_bits(got, want)
    counts = got["call.1.0"]
    assert ((got["call.1.1"] & am.EDGE) != 0).sum() > 1000 and (counts[..., am.SELF] < 16).any()
    np.testing.assert_array_equal(got["call.0"], antialias.present_aa_host(ao.W, ao.H, 4, first[0], counts, 1.0, "accum", "aces",
                                                                           WHITE, "srgb"))


# ----------------------------------------------------------------------------------- C++ API
def test_headless_aa_equals_the_python_sequence(gpu, sky, tmp_path):
    """cpt_headless --aa 4 --present aces (PathTracer::ResolveCoverage / PresentAntialiased) writes
    the frame the same calls give through the Python module; --aa without --present is a usage
    error, and with two devices' tiles the antialiased presentation is refused."""
    from cpppathtracer_amd import build
    W, H, SPP = 48, 32, 2
    exe = build.build_examples()
    common = ["--scene", "s4", "--width", str(W), "--height", str(H), "--spp", str(SPP), "--depth", "4", "--seed", str(SEED)]
    out = tmp_path / "frame.bgra"
    r = subprocess.run([exe, *common, "--present", "aces", "--exposure", "auto", "--aa", "4", "--bgra", str(out)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, dtype=np.uint8).reshape(H, W, 4)
    cam = _cam(W, H)
    _frame(gpu, sky, W, H, scenes.scene_s4())
    gpu.render(cam, SPP, 4, aux=True, sync=True, ordered=True)
    present.meter_exposure(gpu)
    antialias.coverage(gpu, cam, 4, 0.9, WALK)
    want = antialias.present_aa(gpu, "accum", "aces", 4.0, "srgb")
    np.testing.assert_array_equal(got, want)
    assert (want != present.present(gpu, "accum", "aces", 4.0, "srgb")).any()
    bad = subprocess.run([exe, *common, "--aa", "4", "--bgra", str(tmp_path / "no.bgra")], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--aa" in bad.stderr and not (tmp_path / "no.bgra").exists()
    bad = subprocess.run([exe, *common, "--present", "aces", "--aa", "3", "--bgra", str(tmp_path / "no.bgra")], capture_output=True,
                         text=True, timeout=60)
    assert bad.returncode == 2 and "--aa" in bad.stderr
    two = subprocess.run([exe, *common, "--devices", "2", "--present", "aces", "--aa", "4", "--bgra", str(tmp_path / "no.bgra")],
                         capture_output=True, text=True, timeout=300)
    # (the example reaches ResolveCoverage first; PresentAntialiased's own refusal: test_gpu_antialias_tiles.py)
    assert two.returncode == 1 and "ResolveCoverage: ResolveCoverage: not available with SetDevices(n > 1)" in two.stderr, two.stdout + two.stderr
    assert not (tmp_path / "no.bgra").exists()
