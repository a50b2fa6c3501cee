"""The host hooks of bloom (cpt_bloom_host, cpt_present_bloom_host) held bit for bit
and byte for byte to the numpy restatement tests/bloom_model.py, which is written from the
definition's text; the definition's identities; and the contract coverage of cpt_bloom_capi.cpp's
messages (tests/golden/capi_contract_bloom.json), as tests/test_antialias_model.py holds
cpt_antialias_capi.cpp's.  No GPU.
"""
import itertools
import json
import os
import re

import bloom_model as bm
import numpy as np
import present_model as pm
import pytest
import test_capi_contract_coverage as cc

from cpppathtracer_amd import CptError, bloom, present

F = np.float32
WHITE = 2.5
FIXTURE = os.path.join(cc.REPO, "tests", "golden", "capi_contract_bloom.json")
SOURCE = os.path.join(cc.CSRC, "cpt_bloom_capi.cpp")
ids = lambda wh: f"{wh[0]}x{wh[1]}"   # noqa: E731


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def planes(W, H):
    """(name, source, src, exposure, threshold): hashed bit patterns (every class of float in every
    position), ranged values with the special inputs (no pass, NaN, +-Inf, -0, denormals), the
    filtered rgb of both, and an exposure that overflows c' e."""
    n = W * H
    hashed = pm.hashed_floats(4 * n, seed=W * 1000 + H).reshape(n, 4)
    ranged = pm.synthetic_accum(n, seed=W + 7 * H)
    rgb = np.ascontiguousarray(ranged[:, :3] / F(8))
    return [("hashed accum", "accum", hashed, 1.0, 0.5), ("ranged accum", "accum", ranged, 0.37, 1.0),
            ("hashed rgb", "filtered", np.ascontiguousarray(hashed[:, :3]), 2.0, 0.0), ("ranged rgb", "filtered", rgb, 1.0, 4.0),
            ("overflowing exposure", "accum", ranged, 3e38, 1.0)]


# ------------------------------------------------------------------------------ hooks against the model
@pytest.mark.parametrize("L", bm.LEVELS)
@pytest.mark.parametrize("wh", bm.SHAPES, ids=ids)
def test_every_level_equals_the_model(wh, L):
    W, H = wh
    assert bloom.level_shapes(W, H, L) == bm.level_shapes(W, H, L)
    for name, source, src, e, thr in planes(W, H):
        x, U = bm.pyramid(W, H, src, e, pm.ACCUM if source == "accum" else pm.FILTERED, thr, L)
        assert np.isfinite(x).all() and (x >= 0).all()
        for l in range(1, L + 1):
            got = bloom.bloom_host(W, H, src, e, source, thr, L, l)
            assert got.shape == U[l].shape
            np.testing.assert_array_equal(_bits(got), _bits(U[l]), err_msg=f"{name}: U_{l} of {L}")


@pytest.mark.parametrize("L", bm.LEVELS)
@pytest.mark.parametrize("wh", bm.SHAPES, ids=ids)
def test_the_bytes_equal_the_model(wh, L):
    W, H = wh
    T = present.srgb_thresholds_host()
    for name, source, src, e, thr in planes(W, H):
        s = pm.ACCUM if source == "accum" else pm.FILTERED
        for tone, transfer in itertools.product(pm.TONES, pm.TRANSFERS):
            got = bloom.present_bloom_host(W, H, src, e, source, thr, L, 0.3, tone, WHITE, transfer)
            want = bm.present_bloom(W, H, src, e, s, thr, L, 0.3, pm.TONES[tone], WHITE, pm.TRANSFERS[transfer], T)
            np.testing.assert_array_equal(got, want, err_msg=f"{name}: {tone} {transfer}, {L} levels")


def test_the_model_takes_its_taps_where_the_definition_says():
    """The restatement's vectorised indices against the definition's words, texel by texel, on a
    5 x 3 level of distinct integers (exact in float32)."""
    T = np.arange(15, dtype=F).reshape(3, 5, 1).repeat(3, axis=2)
    d = bm.down(T)
    assert d.shape == (2, 3, 3)
    for Y, X in itertools.product(range(2), range(3)):
        rows = [min(max(2 * Y - 1 + j, 0), 2) for j in range(4)]
        cols = [min(max(2 * X - 1 + i, 0), 4) for i in range(4)]
        r = [(T[y, cols[0], 0] + 3 * T[y, cols[1], 0]) + (3 * T[y, cols[2], 0] + T[y, cols[3], 0]) for y in rows]
        assert d[Y, X, 0] == F(((r[0] + 3 * r[1]) + (3 * r[2] + r[3])) / 64)
    u = bm.up(d, 5, 3)
    for y, x in itertools.product(range(3), range(5)):
        px, py = x >> 1, y >> 1
        qx, qy = min(max(px + (1 if x & 1 else -1), 0), 2), min(max(py + (1 if y & 1 else -1), 0), 1)
        h = lambda row: F(3) * d[row, px, 0] + d[row, qx, 0]   # noqa: E731
        assert u[y, x, 0] == (F(3) * h(py) + h(qy)) * F(0.0625)


# ------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("wh", bm.SHAPES, ids=ids)
def test_a_constant_plane_sums_the_levels_exactly(wh):
    """threshold 0 and a constant plane of a small dyadic v: every tap sum is v times a power of
    two whatever the clamping, so U_l = (L - l + 1) v and the glow L v, exactly."""
    W, H = wh
    v = F(0.375)
    rgb = np.full((W * H, 3), v, dtype=F)
    accum = np.concatenate([rgb * F(4), np.full((W * H, 1), 4, dtype=F)], axis=1)
    for L, (source, src) in itertools.product(bm.LEVELS, (("filtered", rgb), ("accum", accum))):
        for l in range(1, L + 1):
            got = bloom.bloom_host(W, H, src, 1.0, source, 0.0, L, l)
            assert (got == F(L - l + 1) * v).all(), f"U_{l} of {L}"
        # x' = v + 0.5 L v through the clamp curve and the linear transfer: one byte everywhere
        out = bloom.present_bloom_host(W, H, src, 1.0, source, 0.0, L, 0.5, "clamp", WHITE, "linear")
        byte = int(F(255.99) * min(v + F(0.5) * (F(L) * v), F(1)))
        assert (out[..., :3] == byte).all() and (out[..., 3] == 255).all()


@pytest.mark.parametrize("wh", bm.SHAPES, ids=ids)
def test_no_intensity_and_no_light_above_the_threshold_give_present(wh):
    W, H = wh
    for name, source, src, e, thr in planes(W, H):
        for tone, transfer in itertools.product(pm.TONES, pm.TRANSFERS):
            plain = present.present_host(src, e, source, tone, WHITE, transfer).reshape(H, W, 4)
            for L in (1, 8):
                np.testing.assert_array_equal(bloom.present_bloom_host(W, H, src, e, source, thr, L, 0.0, tone, WHITE, transfer), plain,
                                              err_msg=f"{name}: intensity 0")
                np.testing.assert_array_equal(bloom.present_bloom_host(W, H, src, e, source, 65504.0, L, 0.7, tone, WHITE, transfer), plain,
                                              err_msg=f"{name}: threshold 65504")


@pytest.mark.parametrize("L", bm.LEVELS)
def test_one_bright_pixel_glows_within_the_taps_reach(L):
    """One pixel of 4000 in a black 64 x 48 frame: the coarsest level is not zero, and no byte
    outside the reach the taps give (bloom_model.reach derives it) differs from the black frame's."""
    W, H, px, py = 64, 48, 37, 20
    rgb = np.zeros((H, W, 3), dtype=F)
    rgb[py, px] = 4000.0
    top = bloom.bloom_host(W, H, rgb, 1.0, "filtered", 1.0, L, L)
    assert (top > 0).any()
    out = bloom.present_bloom_host(W, H, rgb, 1.0, "filtered", 1.0, L, 1.0, "clamp", WHITE, "linear")
    lit = (out[..., :3] != 0).any(axis=2)
    f = bm.reach()
    (x0, x1), (y0, y1) = f(px, L), f(py, L)
    inside = np.zeros((H, W), dtype=bool)
    inside[max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] = True
    assert lit[py, px] and lit.sum() > 1 and not (lit & ~inside).any()
    if L <= 2:   # the reach is tight while it lies inside the frame: its corners are lit
        assert 0 <= x0 and x1 < W and 0 <= y0 and y1 < H
        glow = bloom.bloom_host(W, H, rgb, 1.0, "filtered", 1.0, L, 1)
        gx0, gx1, gy0, gy1 = (x0 + 1) // 2, x1 // 2 - 1, (y0 + 1) // 2, y1 // 2 - 1   # up reads 2 lo - 1 .. 2 hi + 2
        assert (glow[[gy0, gy0, gy1, gy1], [gx0, gx1, gx0, gx1]] > 0).all()


# --------------------------------------------------------------------------------------- contract
def test_host_hooks_refuse_bad_arguments():
    W, H = 4, 3
    accum = pm.synthetic_accum(W * H, 3)
    nan, inf = float("nan"), float("inf")
    for call in (lambda: bloom.bloom_host(W, H, accum, levels=0), lambda: bloom.bloom_host(W, H, accum, levels=9),
                 lambda: bloom.bloom_host(W, H, accum, levels=2, level=3), lambda: bloom.bloom_host(W, H, accum, levels=2, level=0),
                 lambda: bloom.bloom_host(W, H, accum, threshold=-1.0), lambda: bloom.bloom_host(W, H, accum, threshold=nan),
                 lambda: bloom.bloom_host(W, H, accum, threshold=inf), lambda: bloom.bloom_host(W, H, accum, source=2),
                 lambda: bloom.bloom_host(0, 0, accum[:0]),
                 lambda: bloom.present_bloom_host(W, H, accum, intensity=-0.5), lambda: bloom.present_bloom_host(W, H, accum, intensity=nan),
                 lambda: bloom.present_bloom_host(W, H, accum, intensity=inf), lambda: bloom.present_bloom_host(W, H, accum, tone=3),
                 lambda: bloom.present_bloom_host(W, H, accum, white=0.0), lambda: bloom.present_bloom_host(W, H, accum, transfer=2),
                 lambda: bloom.present_bloom_host(W, H, accum, levels=9)):
        with pytest.raises(CptError) as e:
            call()
        assert e.value.status == 1
    with pytest.raises(ValueError):
        bloom.bloom_host(W, H + 1, accum)


def _formats():
    with open(SOURCE) as fh:
        src = fh.read()
    return src, ["".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))) for m in cc.FAIL.finditer(src)]


def test_every_fail_site_of_the_new_file_is_found():
    src, formats = _formats()
    sites = sum(len(re.findall(r"\bfail\(", line.split("//")[0])) for line in src.splitlines())
    assert len(formats) == sites and sites >= 6


def test_every_message_of_the_new_file_is_recorded():
    """Each fail(...) format of cpt_bloom_capi.cpp, and the text cpt_last_bloom_ms hands to
    last_span_ms, is in the recorded contract with a status other than CPT_OK."""
    with open(FIXTURE) as fh:
        steps = json.load(fh)
    assert all(len(s) == 3 and isinstance(s[1], int) for s in steps)
    texts = sorted({s[2] for s in steps if s[1] != 0})
    src, formats = _formats()
    missing = [f for f in formats if not any(cc.pattern_of(f).fullmatch(t) for t in texts)]
    assert not missing, missing
    spans = re.findall(r'last_span_ms\(c,\s*&cpt_ctx::\w+,\s*&?\w+,\s*"((?:[^"\\]|\\.)*)"\)', src)
    assert len(spans) == 1 and spans[0] in texts
    # and the file stays outside the other coverage test's reach, whose counts are pinned
    assert not os.path.basename(SOURCE).startswith("cpt_capi")
