"""The a-trous filter on the host (cpt_filter_prepare_host, cpt_filter_level_host; no GPU) against
its numpy restatement (filter_model), bit for bit, and the properties the definition promises
(DESIGN.md §19).  The device runs the same header functions (cpt_filter.hpp);
tests/test_gpu_filter.py holds it to this model."""
import ctypes

import adaptive_model as am
import filter_model as fm
import numpy as np
import pytest

from cpppathtracer_amd import _lib, camera_get_copy, scenes

F = np.float32
INVALID = 1


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_prepare(accum, stat):
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    stat = np.ascontiguousarray(stat, dtype=np.float32)
    npix = accum.shape[0]
    plane = np.zeros((npix, 4), dtype=np.float32)
    valid = np.zeros(npix, dtype=np.uint8)
    assert _lib.load().cpt_filter_prepare_host(npix, _ptr(accum), _ptr(stat), _ptr(plane), _ptr(valid)) == 0
    return plane, valid.astype(bool)


def host_level(plane, normal, valid, W, H, step, sigma_l=1.0, sharpness=7):
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    v8 = np.ascontiguousarray(valid, dtype=np.uint8)
    out = np.zeros_like(plane)
    st = _lib.load().cpt_filter_level_host(W, H, step, _ptr(plane), _ptr(normal), _ptr(v8), ctypes.c_float(sigma_l),
                                           sharpness, _ptr(out))
    assert st == 0
    return out


def host_run(accum, stat, normal, W, H, levels=5, sigma_l=1.0, sharpness=7):
    plane, valid = host_prepare(accum, stat)
    for l in range(levels):
        plane = host_level(plane, normal, valid, W, H, 1 << l, sigma_l, sharpness)
    return plane[:, :3].copy(), plane[:, 3].copy()


@pytest.mark.parametrize("wh", fm.SHAPES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_host_equals_model_level_by_level(wh):
    """prepare, then levels at steps 1, 4 and 16 (taps of the later ones fall outside the whole
    frame), each fed the one before; at the defaults, at sigma_l 4 / sharpness 3 and at sigma_l 0 / sharpness 0."""
    W, H = wh
    accum, stat, normal = fm.synthetic_state(W, H, seed=100 + W)
    plane, valid = fm.prepare(accum, stat)
    h_plane, h_valid = host_prepare(accum, stat)
    np.testing.assert_array_equal(h_valid, valid)
    fm.assert_same_bits(h_plane, plane, "prepare")
    if W * H > 60:
        assert valid.sum() > 0.6 * W * H and (~valid).sum() >= 4
        n0 = accum[:, 3] == 0
        assert n0.any() and not plane[n0].any()                     # count 0: its output is 0
    for sigma_l, sharp in ((1.0, 7), (4.0, 3), (0.0, 0)):
        p = plane
        for step in (1, 4, 16):
            want = fm.level(p, normal, valid, W, H, step, sigma_l, sharp)
            got = host_level(p, normal, valid, W, H, step, sigma_l, sharp)
            fm.assert_same_bits(got, want, f"step {step} sigma_l {sigma_l}")
            fm.assert_same_bits(want[~valid], p[~valid], "an invalid pixel is left as it is")
            assert np.isfinite(want[valid]).all()
            if W * H > 60 and step == 1:
                assert (want[valid] != p[valid]).any()               # the level did filter
            p = want


def test_levels_zero_returns_c0():
    W, H = 20, 12
    accum, stat, normal = fm.synthetic_state(W, H, seed=5)
    plane, _ = host_prepare(accum, stat)
    for run in (fm.run, host_run):
        rgb, var = run(accum, stat, normal, W, H, levels=0)
        fm.assert_same_bits(rgb, plane[:, :3])
        fm.assert_same_bits(var, plane[:, 3])
    ok = accum[:, 3] > 0
    with np.errstate(all="ignore"):
        fm.assert_same_bits(plane[ok, :3], accum[ok, :3] / accum[ok, 3:4])


def test_an_invalid_pixel_is_no_tap():
    """Whatever an invalid pixel holds, every other pixel's output is the same, bit for bit."""
    W, H = 20, 12
    accum, stat, normal = fm.synthetic_state(W, H, seed=6)
    plane, valid = host_prepare(accum, stat)
    bad = np.flatnonzero(~valid)
    assert bad.size >= 4
    other = plane.copy()
    other[bad] = np.array([[3.5, -2e5, 0.25, 7.0]], dtype=np.float32)
    others = np.ones(W * H, dtype=bool)
    others[bad] = False
    for step in (1, 2):
        a = host_level(plane, normal, valid, W, H, step)
        b = host_level(other, normal, valid, W, H, step)
        fm.assert_same_bits(a[others], b[others])
        fm.assert_same_bits(b[bad], other[bad])


def test_no_leak_across_a_normal_edge():
    """Left half normal (1,0,0), right half (0,1,0): the right half's colours reach no left-half
    output.  Colours only: the 3x3 variance prefilter is deliberately not edge-stopped."""
    W, H = 32, 16
    rs = np.random.RandomState(11)
    npix = W * H
    x = np.arange(npix) % W
    normal = np.where((x < W // 2)[:, None], [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]]).astype(np.float32)
    plane = np.concatenate([rs.uniform(0.2, 0.8, (npix, 3)), rs.uniform(0.0, 1e-2, (npix, 1))], axis=1).astype(np.float32)
    other = plane.copy()
    other[x >= W // 2, :3] = rs.uniform(0.0, 50.0, (int((x >= W // 2).sum()), 3)).astype(np.float32)
    valid = np.ones(npix, dtype=bool)
    # level by level from the same variances: a level's output variance depends on its weights and
    # so on the colours, and the next level's prefilter would carry that (and only that) across
    for l in range(5):
        a = host_level(plane, normal, valid, W, H, 1 << l)
        b = host_level(other, normal, valid, W, H, 1 << l)
        fm.assert_same_bits(a[x < W // 2], b[x < W // 2], f"level {l}")
        assert (a[x >= W // 2, :3] != b[x >= W // 2, :3]).any()
    # the edge is what stops them: with one normal everywhere the same colours do reach the left half
    flat = np.tile(np.array([[1.0, 0.0, 0.0]], dtype=np.float32), (npix, 1))
    a1, b1 = host_level(plane, flat, valid, W, H, 1), host_level(other, flat, valid, W, H, 1)
    assert (a1[x < W // 2, :3] != b1[x < W // 2, :3]).any()


def test_argument_checks_of_the_host_hook():
    W, H = 5, 3
    accum, stat, normal = fm.synthetic_state(W, H, seed=1)
    plane, valid = host_prepare(accum, stat)
    v8 = valid.astype(np.uint8)
    out = np.zeros_like(plane)
    L = _lib.load()

    def status(step=1, sigma_l=1.0, sharp=7, w=W, h=H):
        return L.cpt_filter_level_host(w, h, step, _ptr(plane), _ptr(normal), _ptr(v8), ctypes.c_float(sigma_l), sharp,
                                       _ptr(out))

    assert status() == 0 and status(step=128) == 0 and status(sharp=10) == 0 and status(sigma_l=0.0) == 0
    for bad in (dict(step=0), dict(step=256), dict(sigma_l=-1.0), dict(sigma_l=float("nan")), dict(sigma_l=float("inf")),
                dict(sharp=-1), dict(sharp=11), dict(w=0), dict(h=-1)):
        assert status(**bad) == INVALID, bad


def test_the_defaults_reduce_the_error(oracle_mod, sky):
    """The oracle's S4 at 64 x 64, depth 8: 32 spp as 8 batches of 4 with adaptive_model's moments,
    five levels at the defaults, against the oracle's 1024-spp mean.  (DESIGN.md §19 records both
    RMSEs.)"""
    W = H = 64
    depth, batch, rounds, seed = 8, 4, 8, 1234
    objs = scenes.scene_s4()
    cam = camera_get_copy(scenes.camera_for(W, H))
    rows = np.arange(H, dtype=np.int32)
    rng = oracle_mod.init_rng(seed, W, rows, threads=8)
    snaps = am.oracle_rounds(oracle_mod, objs, cam, sky, rows, batch, rounds, depth, rng, aux=True)
    m = am.run(snaps, W, H, batch, batch * rounds, batch * rounds, F(0.05))
    assert (m["stop"] == rounds).all()
    stat = fm.moments(snaps, m["stop"], W, H, m["noise"])
    assert (stat[2] == rounds).all()
    ref_rng = oracle_mod.init_rng(seed + 1, W, rows, threads=8)
    ref = oracle_mod.render(objs, cam, sky, rows, 1024, depth, ref_rng, threads=8)[0]
    ref = (ref[:, :3] / ref[:, 3:4]).astype(np.float64)
    noisy = (m["accum"][:, :3] / m["accum"][:, 3:4]).astype(np.float64)
    rgb, var = host_run(m["accum"], stat, m["normal"], W, H, **{"levels": fm.DEFAULTS["levels"],
                                                                "sigma_l": fm.DEFAULTS["sigma_l"],
                                                                "sharpness": fm.DEFAULTS["sharpness"]})
    rmse_noisy = float(np.sqrt(np.mean((noisy - ref) ** 2)))
    rmse_filtered = float(np.sqrt(np.mean((rgb.astype(np.float64) - ref) ** 2)))
    print(f"RMSE vs the 1024-spp mean: unfiltered 32 spp {rmse_noisy:.6f}, filtered {rmse_filtered:.6f}")
    assert np.isfinite(rgb).all() and np.isfinite(var).all()
    assert rmse_filtered < rmse_noisy, (rmse_filtered, rmse_noisy)
