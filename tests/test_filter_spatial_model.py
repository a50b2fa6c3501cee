"""The filter for frames without moments on the host (cpt_filter_prepare_spatial_host,
cpt_filter_level_id_host; no GPU) against its numpy restatement (filter_spatial_model), bit for bit,
and the properties the definition promises.  The device runs the same header
functions (cpt_filter.hpp); tests/test_gpu_filter_spatial.py holds it to these hooks."""
import ctypes
import os
import re

import filter_spatial_model as sm
import numpy as np
import pytest

from cpppathtracer_amd import Renderer, _lib

F = np.float32
INVALID = 1
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cpt.h")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_prepare(accum, ids, normal, W, H, sharpness=3):
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    plane = np.zeros((W * H, 4), dtype=np.float32)
    valid = np.zeros(W * H, dtype=np.uint8)
    st = _lib.load().cpt_filter_prepare_spatial_host(W, H, _ptr(accum), _ptr(ids), _ptr(normal), sharpness, _ptr(plane),
                                                     _ptr(valid))
    assert st == 0
    return plane, valid.astype(bool)


def host_level(plane, normal, ids, valid, W, H, step, sigma_l=4.0, sharpness=3):
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    v8 = np.ascontiguousarray(valid, dtype=np.uint8)
    out = np.zeros_like(plane)
    st = _lib.load().cpt_filter_level_id_host(W, H, step, _ptr(plane), _ptr(normal), _ptr(ids), _ptr(v8),
                                              ctypes.c_float(sigma_l), sharpness, _ptr(out))
    assert st == 0
    return out


def host_level_plain(plane, normal, valid, W, H, step, sigma_l=4.0, sharpness=3):
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    v8 = np.ascontiguousarray(valid, dtype=np.uint8)
    out = np.zeros_like(plane)
    st = _lib.load().cpt_filter_level_host(W, H, step, _ptr(plane), _ptr(normal), _ptr(v8), ctypes.c_float(sigma_l),
                                           sharpness, _ptr(out))
    assert st == 0
    return out


def host_run(accum, ids, normal, W, H, levels=5, sigma_l=4.0, sharpness=3):
    plane, valid = host_prepare(accum, ids, normal, W, H, sharpness)
    for l in range(levels):
        plane = host_level(plane, normal, ids, valid, W, H, 1 << l, sigma_l, sharpness)
    return plane[:, :3].copy(), plane[:, 3].copy()


@pytest.mark.parametrize("kind", sm.ID_KINDS)
@pytest.mark.parametrize("wh", sm.SHAPES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_host_equals_model_level_by_level(wh, kind):
    """prepare, then levels at steps 1, 2, 4 and 16, each fed the one before, at sigma_l 4 /
    sharpness 3, at sigma_l 1 / sharpness 7 and at sigma_l 0 / sharpness 0."""
    W, H = wh
    accum, normal = sm.synthetic_state(W, H, seed=200 + W)
    ids = sm.id_plane(W, H, kind)
    for sigma_l, sharp in ((4.0, 3), (1.0, 7), (0.0, 0)):
        plane, valid = sm.prepare(accum, ids, normal, W, H, sharp)
        h_plane, h_valid = host_prepare(accum, ids, normal, W, H, sharp)
        np.testing.assert_array_equal(h_valid, valid)
        sm.assert_same_bits(h_plane, plane, "prepare")
        _, b = sm.base(accum)
        assert not plane[~b, 3].any()                                   # v0 = 0 where !b
        if W * H > 60:
            assert b.sum() > 0.6 * W * H and (~b).sum() >= 4
            n0 = accum[:, 3] == 0
            assert n0.any() and not plane[n0].any()
            if kind == "one":
                assert (plane[valid, 3] > 0).any()
        p = plane
        for step in (1, 2, 4, 16):
            want = sm.level(p, normal, ids, valid, W, H, step, sigma_l, sharp)
            got = host_level(p, normal, ids, valid, W, H, step, sigma_l, sharp)
            sm.assert_same_bits(got, want, f"step {step} sigma_l {sigma_l}")
            sm.assert_same_bits(want[~valid], p[~valid], "an invalid pixel is left as it is")
            p = want


def test_a_nan_normal_invalidates_through_v0():
    """A pixel with a NaN normal poisons the sums of its neighbours in the window: they hold a finite
    mean (b) and are invalid all the same, on both sides."""
    W, H = 20, 12
    accum, normal = sm.synthetic_state(W, H, seed=9, nan_normal=True)
    accum[:, :3] = np.where(np.isfinite(accum[:, :3]), accum[:, :3], F(1.0))
    accum[:, 3] = np.where(np.isfinite(accum[:, 3]) & (accum[:, 3] > 0), accum[:, 3], F(2.0))
    ids = sm.id_plane(W, H, "one")
    plane, valid = sm.prepare(accum, ids, normal, W, H, 3)
    h_plane, h_valid = host_prepare(accum, ids, normal, W, H, 3)
    np.testing.assert_array_equal(h_valid, valid)
    sm.assert_same_bits(h_plane, plane)
    _, b = sm.base(accum)
    assert b.all() and (~valid).sum() >= 8 and np.isnan(plane[~valid, 3]).all()
    for step in (1, 2):
        want = sm.level(plane, normal, ids, valid, W, H, step, 4.0, 3)
        sm.assert_same_bits(host_level(plane, normal, ids, valid, W, H, step), want)
        sm.assert_same_bits(want[~valid], plane[~valid])


def _const_state(W, H, colour, rs):
    """A constant image of random counts.  The properties below are exact where the arithmetic is:
    the colours used have a few mantissa bits and so has their luminance (0.0625, 0.5, 2.4375 ->
    0.546875 and the like, found by search), so colour x count, weight x colour and the window's sums
    are all exact.  For a colour of 24 bits mu is the luminance only to rounding and v0 a few 1e-15."""
    n = rs.randint(1, 33, W * H).astype(np.float32)
    accum = np.concatenate([np.asarray(colour, dtype=np.float32)[None, :] * n[:, None], n[:, None]], axis=1).astype(np.float32)
    normal = np.tile(np.array([[0.0, 1.0, 0.0]], dtype=np.float32), (W * H, 1))
    return accum, normal


def test_a_constant_image_stays():
    W, H = 20, 12
    accum, normal = _const_state(W, H, (0.0625, 0.5, 2.4375), np.random.RandomState(1))
    ids = sm.id_plane(W, H, "one")
    plane, valid = host_prepare(accum, ids, normal, W, H)
    assert valid.all() and not plane[:, 3].any()
    p = plane
    for l in range(5):
        q = host_level(p, normal, ids, valid, W, H, 1 << l)
        sm.assert_same_bits(q, plane, f"level {l}")
        p = q


def test_a_constant_image_of_a_general_colour_stays_within_rounding():
    """A colour of 24 mantissa bits: with unit normals every w is 1, a = n and A = sum(n) are exact;
    each a x l rounds once and B's 49 additions once each, so B and mu = B / A are off by at most
    (1 + 49 + 1) u = 51 u relatively, u = 2^-24.  Then |l - mu| <= 51 u l (1 + u), D <= A (52 u l)^2,
    s2 = (D / W)(m / (m - 1)) <= (A / W)(52 u l)^2 x 2 with A / W <= max n = 32, and v0 = s2 / n_p <=
    64 x 52^2 u^2 l^2 < 2e5 u^2 l^2.  The levels then leave the colour exactly: d = 0, so wl = den /
    den = 1 whatever v0 is, and every tap carries the same colour; sum(w c) / sum(w) returns c within
    the 25 products' and sums' roundings, (25 + 25 + 1) u relatively, per level."""
    W, H = 20, 12
    u = 2.0 ** -24
    rs = np.random.RandomState(8)
    colour = (0.3712, 0.8123, 0.2291)
    accum, normal = _const_state(W, H, colour, rs)
    accum[:, 3] = 8.0                                        # c = S / n exact: S = c x 8
    accum[:, :3] = np.asarray(colour, dtype=np.float32)[None, :] * F(8.0)
    accum[::3, 3] = 16.0
    accum[::3, :3] *= F(2.0)
    ids = sm.id_plane(W, H, "one")
    plane, valid = host_prepare(accum, ids, normal, W, H)
    c = np.asarray(colour, dtype=np.float32)
    l = float((F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2])
    assert valid.all() and (plane[:, :3] == c).all()
    assert (plane[:, 3] >= 0).all() and plane[:, 3].max() <= 2e5 * u * u * l * l, plane[:, 3].max()
    p = plane
    for k in range(5):
        q = host_level(p, normal, ids, valid, W, H, 1 << k)
        assert (np.abs(q[:, :3].astype(np.float64) - p[:, :3]) <= 51 * u * np.abs(p[:, :3])).all(), k
        p = q


def test_a_lone_pixel_of_a_general_colour_drifts_by_rounding_only():
    """A pixel alone in its object leaves a level as (h c) / h, two roundings: within 2 u (1 + u) of c
    relatively, u = 2^-24, that is one unit in the last place at most, per level; its variance stays 0."""
    W, H = 20, 12
    u = 2.0 ** -24
    accum, normal = sm.synthetic_state(W, H, seed=12)
    own = np.arange(W * H, dtype=np.int32)
    plane, valid = host_prepare(accum, own, normal, W, H)
    assert valid.sum() > 0.6 * W * H and not plane[:, 3].any()
    p = plane
    for k in range(5):
        q = host_level(p, normal, own, valid, W, H, 1 << k)
        a, b = q[valid].astype(np.float64), p[valid].astype(np.float64)
        assert (np.abs(a[:, :3] - b[:, :3]) <= 2 * u * (1 + u) * np.abs(b[:, :3])).all(), k
        assert not q[valid, 3].any()
        sm.assert_same_bits(q[~valid], p[~valid])
        p = q
    assert (p[valid, :3] != plane[valid, :3]).any()          # 24-bit means do drift: the exact case needs few bits


def _few_bits(accum):
    """The same state with 16-bit mantissas in the sums and a count of 8: the mean is then exact and
    so is the centre tap's weight x mean (the weight 9/64 has four bits), and (h c) / h returns c.  A
    mean of 24 bits comes back from its own single tap to within one unit in the last place only."""
    out = np.array(accum, dtype=np.float32, copy=True)
    ok = np.isfinite(out).all(axis=1) & (out[:, 3] > 0)
    out[ok, :3] = (out[ok, :3].view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)
    out[ok, 3] = F(8.0)
    return out


def test_a_pixel_alone_in_its_object_stays():
    W, H = 20, 12
    accum, normal = sm.synthetic_state(W, H, seed=12)
    accum = _few_bits(accum)
    ids = sm.id_plane(W, H, "one").copy()
    _, b = sm.base(accum)
    lone = np.flatnonzero(b)[[3, 40, 90]]
    ids[lone] = 100 + np.arange(lone.size)
    plane, valid = host_prepare(accum, ids, normal, W, H)
    assert valid[lone].all() and not plane[lone, 3].any()
    p = plane
    for l in range(5):
        q = host_level(p, normal, ids, valid, W, H, 1 << l)
        sm.assert_same_bits(q[lone], plane[lone], f"level {l}")
        p = q
    # ... and the checkerboard of one-pixel objects: no tap at odd offsets, so step 1's diagonal
    # taps remain; with every pixel its own id nothing moves at all
    own = np.arange(W * H, dtype=np.int32)
    plane, valid = host_prepare(accum, own, normal, W, H)
    assert not plane[:, 3].any()
    sm.assert_same_bits(host_level(plane, normal, own, valid, W, H, 1), plane)


def test_two_objects_of_equal_normals_do_not_mix():
    """Two regions of different constant colours, equal normals, different ids: out as in, level by
    level.  With one id the colours do cross, so the id is what stops them."""
    W, H = 32, 16
    rs = np.random.RandomState(3)
    a, normal = _const_state(W, H, (0.125, 0.5625, 2.5), rs)
    b_, _ = _const_state(W, H, (0.1875, 1.25, 0.375), rs)
    x = np.arange(W * H) % W
    accum = np.where((x < W // 2)[:, None], a, b_)
    ids = np.where(x < W // 2, 0, 1).astype(np.int32)
    plane, valid = host_prepare(accum, ids, normal, W, H)
    assert valid.all() and not plane[:, 3].any()
    p = plane
    for l in range(5):
        q = host_level(p, normal, ids, valid, W, H, 1 << l)
        sm.assert_same_bits(q, plane, f"level {l}")
        p = q
    one = np.zeros(W * H, dtype=np.int32)
    plane1, valid1 = host_prepare(accum, one, normal, W, H)
    assert (plane1[:, 3] > 0).any()
    assert (host_level(plane1, normal, one, valid1, W, H, 1)[:, :3] != plane1[:, :3]).any()


@pytest.mark.parametrize("wh", [(20, 12), (67, 9)], ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_one_id_equals_the_plain_level(wh):
    W, H = wh
    accum, normal = sm.synthetic_state(W, H, seed=31)
    ids = sm.id_plane(W, H, "one")
    plane, valid = host_prepare(accum, ids, normal, W, H)
    for step in (1, 2, 4, 16):
        sm.assert_same_bits(host_level(plane, normal, ids, valid, W, H, step, 1.0, 7),
                            host_level_plain(plane, normal, valid, W, H, step, 1.0, 7), f"step {step}")


@pytest.mark.parametrize("counts", ["uniform16", "alternating4_32"])
def test_the_estimator_recovers_the_per_pass_variance(counts):
    """A 64 x 64 one-object plane of mean 0.5 plus Gaussian noise of variance sigma^2 / n: the mean of
    v0 x n over the pixels at least 3 from the border is within 10% of sigma^2 (expected relative
    deviation of that mean: about 2%, from 58 x 58 / 49 independent windows of 48 degrees of freedom)."""
    W = H = 64
    rs = np.random.RandomState(2024)
    sigma2 = 0.04
    y, x = np.mgrid[0:H, 0:W]
    n = np.full((H, W), 16.0) if counts == "uniform16" else np.where((x + y) % 2 == 0, 4.0, 32.0)
    n = n.reshape(-1).astype(np.float32)
    mean = (0.5 + rs.standard_normal(W * H) * np.sqrt(sigma2 / n)).astype(np.float32)
    accum = np.concatenate([(mean * n)[:, None].repeat(3, axis=1), n[:, None]], axis=1).astype(np.float32)
    normal = np.tile(np.array([[0.0, 0.0, 1.0]], dtype=np.float32), (W * H, 1))
    ids = np.zeros(W * H, dtype=np.int32)
    plane, valid = host_prepare(accum, ids, normal, W, H)
    assert valid.all()
    inner = ((x >= 3) & (x < W - 3) & (y >= 3) & (y < H - 3)).reshape(-1)
    est = float(np.mean(plane[inner, 3].astype(np.float64) * n[inner]))
    print(f"{counts}: mean of v0 x n = {est:.6f} for sigma^2 = {sigma2}")
    assert abs(est - sigma2) < 0.1 * sigma2, est


def test_argument_checks_of_the_host_hooks():
    W, H = 5, 3
    accum, normal = sm.synthetic_state(W, H, seed=1)
    ids = sm.id_plane(W, H, "one")
    plane, valid = host_prepare(accum, ids, normal, W, H)
    v8 = valid.astype(np.uint8)
    out = np.zeros_like(plane)
    ok8 = np.zeros(W * H, dtype=np.uint8)
    L = _lib.load()

    def level(step=1, sigma_l=1.0, sharp=7, w=W, h=H, idp=ids):
        return L.cpt_filter_level_id_host(w, h, step, _ptr(plane), _ptr(normal), None if idp is None else _ptr(idp),
                                          _ptr(v8), ctypes.c_float(sigma_l), sharp, _ptr(out))

    assert level() == 0 and level(step=128) == 0 and level(sharp=10) == 0 and level(sigma_l=0.0) == 0
    for bad in (dict(step=0), dict(step=256), dict(sigma_l=-1.0), dict(sigma_l=float("nan")), dict(sigma_l=float("inf")),
                dict(sharp=-1), dict(sharp=11), dict(w=0), dict(h=-1), dict(idp=None)):
        assert level(**bad) == INVALID, bad

    def prep(w=W, h=H, sharp=3, idp=ids):
        return L.cpt_filter_prepare_spatial_host(w, h, _ptr(accum), None if idp is None else _ptr(idp), _ptr(normal), sharp,
                                                 _ptr(out), _ptr(ok8))

    assert prep() == 0 and prep(sharp=0) == 0 and prep(sharp=10) == 0
    for bad in (dict(w=0), dict(h=0), dict(sharp=-1), dict(sharp=11), dict(idp=None)):
        assert prep(**bad) == INVALID, bad


DOCUMENTED = {
    "cpt_filter_frame_spatial": ["cpt_ctx*", "int", "float", "int"],
    "cpt_write_gbuffer": ["cpt_ctx*", "const int32_t*", "const float*", "const float*", "const float*", "size_t"],
    "cpt_filter_prepare_spatial_host": ["int", "int", "const float*", "const int32_t*", "const float*", "int", "float*",
                                        "uint8_t*"],
    "cpt_filter_level_id_host": ["int", "int", "int", "const float*", "const float*", "const int32_t*", "const uint8_t*",
                                 "float", "int", "float*"],
}
CTYPE_OF = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", text, re.M)
    assert m, name + " is not declared"
    params = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        params.append(re.sub(r"\s*\w+$", "", p) if not p.endswith("*") else p)
    return params


def test_bindings_declared_exported_and_checked():
    L = _lib.load()
    for name, want in DOCUMENTED.items():
        assert _declared(name) == want, name
        assert hasattr(L, name), name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int, name
        assert args == [CTYPE_OF.get(p, ctypes.c_void_p) for p in want], name
    assert L.cpt_abi_version() == 1
    assert L.cpt_filter_frame_spatial(None, 5, ctypes.c_float(4.0), 3) == INVALID
    assert L.cpt_write_gbuffer(None, None, None, None, None, 0) == INVALID
    for name in ("filter_frame_spatial", "write_gbuffer"):
        assert callable(getattr(Renderer, name)), name
