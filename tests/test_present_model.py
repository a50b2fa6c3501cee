"""Presenting on the host (cpt_present_host, cpt_meter_host, cpt_present_srgb_thresholds_host; no GPU)
against the numpy restatement (present_model), byte for byte and word for word, and the properties
the definition promises.  The device runs the same header functions
(cpt_present.hpp); tests/test_gpu_present.py holds it to these hooks."""
import itertools

import numpy as np
import present_model as pm
import pytest

from cpppathtracer_amd import _lib, present

F = np.float32
COMBOS = list(itertools.product(pm.TONES, pm.TRANSFERS))
WHITE = 2.5


@pytest.fixture(scope="module")
def T():
    return present.srgb_thresholds_host()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _accum_of(values, n=1.0):
    """An accumulator whose three channels hold `values`, `values` reversed and `values` rolled, over count n."""
    v = np.asarray(values, dtype=F)
    return np.stack([v, v[::-1], np.roll(v, 7), np.full(len(v), n, dtype=F)], axis=1)


def _same_as_model(src, e, source, T, what):
    s = pm.ACCUM if source == "accum" else pm.FILTERED
    for tone, transfer in COMBOS:
        got = present.present_host(src, e, source, tone, WHITE, transfer)
        want = pm.present(src, e, s, pm.TONES[tone], WHITE, pm.TRANSFERS[transfer], T)
        np.testing.assert_array_equal(got, want, err_msg=f"{what}: {tone}, {transfer}")
    for key, permille, adapt in ((0.18, 500, 1.0), (0.5, 900, 0.25)):
        got_e, got_h = present.meter_host(src, e, source, key, permille, adapt)
        want_e, want_h = pm.meter(src, e, s, key, permille, adapt)
        np.testing.assert_array_equal(got_h, want_h, err_msg=what)
        assert _bits(got_e) == _bits(want_e), (what, got_e, want_e)


# ------------------------------------------------------------------------------ the thresholds
def test_thresholds_equal_an_independent_recomputation(T):
    want = pm.srgb_thresholds()
    np.testing.assert_array_equal(_bits(T), _bits(want))
    assert T.dtype == F and T[0] == 0 and (np.diff(T.astype(np.float64)) > 0).all() and T[255] <= 1
    # the byte of a threshold is its index, of the float just below it the index before
    below = (_bits(T[1:]) - 1).view(F)
    assert (pm.transfer_byte(T, pm.SRGB, T) == np.arange(256)).all()
    assert (pm.transfer_byte(below, pm.SRGB, T) == np.arange(255)).all()
    # and it is the rounded 255 * oetf(y)
    y = np.linspace(0, 1, 4097, dtype=F)
    np.testing.assert_array_equal(pm.transfer_byte(y, pm.SRGB, T), np.floor(255.0 * pm.oetf(y) + 0.5).astype(np.uint8))


def test_header_table_is_what_the_tool_writes(tmp_path, monkeypatch):
    """The committed header is tools/make_present_tables.py's output, byte for byte."""
    import importlib.util
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_present_tables", os.path.join(repo, "tools", "make_present_tables.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    committed = open(tool.OUT).read()
    monkeypatch.setattr(tool, "OUT", str(tmp_path / "tables.hpp"))
    tool.main()
    assert open(tool.OUT).read() == committed


# ------------------------------------------------------------------- the hooks equal the model
def test_every_threshold_and_its_neighbours(T):
    """Each threshold with its two float32 neighbours on either side, as the colour itself (count 1,
    exposure 1: the clamp curve hands it to the transfer unchanged) and through the other curves."""
    b = _bits(T[1:]).astype(np.int64)
    v = np.concatenate([(b + d).astype(np.uint32).view(F) for d in (-2, -1, 0, 1, 2)])
    acc = _accum_of(v)
    _same_as_model(acc, 1.0, "accum", T, "thresholds")
    _same_as_model(acc[:, :3], 1.0, "filtered", T, "thresholds, filtered")
    got = present.present_host(acc, 1.0, "accum", "clamp", WHITE, "srgb")[:, 2]   # R is channel 0
    want = np.concatenate([np.arange(1, 256) - (d < 0) for d in (-2, -1, 0, 1, 2)])
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("tone", list(pm.TONES))
def test_hashed_values(T, tone):
    """2^20 hashed bit patterns (every class of float) as sums over hashed counts, and the same as
    filtered rgb; 2^20 more in the curve's working range at three exposures."""
    n = 1 << 20
    seed = 11 + pm.TONES[tone]
    raw = np.stack([pm.hashed_floats(n, seed), pm.hashed_floats(n, seed + 100), pm.hashed_floats(n, seed + 200),
                    np.abs(pm.hashed_floats(n, seed + 300))], axis=1)
    u = pm.hashed_floats(n, seed + 400).view(np.uint32)
    ranged = np.stack([np.exp2((u >> 8).astype(np.float64) / 2 ** 24 * 24 - 16).astype(F)] * 3 + [np.ones(n, dtype=F)], axis=1)
    ranged[:, 1] *= F(0.5)
    ranged[:, 2] *= F(3.0)
    for src, source, e, what in ((raw, "accum", 1.0, "raw"), (raw[:, :3], "filtered", 0.75, "raw filtered"),
                                 (ranged, "accum", 1.0, "ranged"), (ranged, "accum", 0.037, "ranged"), (ranged, "accum", 21.0, "ranged")):
        s = pm.ACCUM if source == "accum" else pm.FILTERED
        for transfer in pm.TRANSFERS:
            got = present.present_host(src, e, source, tone, WHITE, transfer)
            want = pm.present(src, e, s, pm.TONES[tone], WHITE, pm.TRANSFERS[transfer], T)
            np.testing.assert_array_equal(got, want, err_msg=f"{what}: {tone}, {transfer}, e {e}")
        got_e, got_h = present.meter_host(src, e, source, 0.18, 500, 0.5)
        want_e, want_h = pm.meter(src, e, s, 0.18, 500, 0.5)
        np.testing.assert_array_equal(got_h, want_h)
        assert _bits(got_e) == _bits(want_e)
    assert len(np.unique(present.present_host(ranged, 1.0, "accum", tone, WHITE, "srgb")[:, 2])) == 256


# --------------------------------------------------------------------------- the special inputs
def test_special_inputs(T):
    one = F(1)
    rows = {                      # rgb, n -> the clamp curve's linear bytes (B, G, R) at exposure 1
        "no pass": ([5, 5, 5, 0], (0, 0, 0)),
        "negative count": ([5, 5, 5, -1], (0, 0, 0)),
        "infinite count": ([5, 5, 5, np.inf], (0, 0, 0)),
        "NaN count": ([5, 5, 5, np.nan], (0, 0, 0)),
        "NaN": ([np.nan, 0.5, 1, 1], (255, 127, 0)),
        "+Inf": ([np.inf, 0.5, 0.25, 1], (63, 127, 255)),
        "-Inf": ([-np.inf, 0.5, 0.25, 1], (63, 127, 0)),
        "-0": ([-0.0, -1.0, 0.25, 1], (63, 0, 0)),
        "denormals": ([1e-45, 1e-40, 1e-38, 1], (0, 0, 0)),
    }
    acc = np.array([v[0] for v in rows.values()], dtype=F)
    got = present.present_host(acc, 1.0, "accum", "clamp", WHITE, "linear")
    for (name, (_, bgr)), px in zip(rows.items(), got):
        assert tuple(px) == bgr + (255,), name
    _same_as_model(acc, 1.0, "accum", T, "special")
    _same_as_model(acc[:, :3], 1.0, "filtered", T, "special, filtered")
    # the four unsourced pixels and the infinite luminance are not metered; a NaN, -Inf or -0 channel
    # counts as 0 and its pixel is metered by the others; the denormal pixel lands in bin 0
    _, hist = present.meter_host(acc, 1.0)
    assert hist[256] == 5 and hist[0] == 1 and hist[:256].sum() == 4
    # an exposure that overflows c' * e: the product is +Inf, exposed as 65504, white under every curve
    big = np.array([[1e10, 1e-10, 0, 1]], dtype=F)
    for tone, transfer in COMBOS:
        px = present.present_host(big, 3e38, "accum", tone, WHITE, transfer)[0]
        assert px[2] == 255 and px[0] == 0 and px[3] == 255, (tone, transfer, px)
    _same_as_model(big, 3e38, "accum", T, "overflowing exposure")
    # luminance at both ends of the histogram: below 2^-16 to bin 0, from 2^16 on to bin 255
    grey = lambda l: [l, l, l, 1]
    ends = np.array([grey(2.0 ** -20), grey(2.0 ** -16 * 0.99), grey(2.0 ** -16 * 1.01), grey(2.0 ** 16 * 0.99), grey(2.0 ** 16 * 1.01),
                     grey(1e30)], dtype=F)
    _, hist = present.meter_host(ends, 1.0)
    assert hist[0] == 3 and hist[255] == 3 and hist.sum() == 6   # 0.99 * 2^16 is in the last bin of the top octave
    np.testing.assert_array_equal(hist, pm.histogram(ends, pm.ACCUM))
    e, _ = present.meter_host(ends[:1], 1.0, key=1.0, permille=0)
    assert e == one / pm.bin_luminance(0) == F(2.0 ** 16)


def test_invalid_arguments_are_refused():
    acc = np.ones((2, 4), dtype=F)
    for bad in (dict(source=2), dict(tone=3), dict(tone=-1), dict(transfer=2), dict(white=0.0), dict(white=-1.0), dict(white=np.nan)):
        with pytest.raises(_lib.CptError) as e:
            present.present_host(acc, **bad)
        assert e.value.status == _lib.CPT_ERR_INVALID_ARG, bad
    for bad in (dict(source=-1), dict(key=0.0), dict(key=np.inf), dict(key=np.nan), dict(permille=-1), dict(permille=1001),
                dict(adapt=-0.1), dict(adapt=1.5), dict(adapt=np.nan)):
        with pytest.raises(_lib.CptError) as e:
            present.meter_host(acc, **bad)
        assert e.value.status == _lib.CPT_ERR_INVALID_ARG, bad
    with pytest.raises(ValueError):
        present.present_host(acc, tone="filmic")


# ------------------------------------------------------------------------- the scaling property
def test_scaling_the_frame_scales_the_exposure_and_keeps_the_bytes(T):
    """rgb x 2^k, k = -8..8: every luminance moves 8k bins, the metered exposure is exactly 2^-k times
    the unscaled one at adapt 1, and the presented bytes do not change.  The luminances span 2^-7 ..
    2^7, so every scaled one stays inside the 32 octaves."""
    rs = np.random.RandomState(5)
    npix = 4096
    n = rs.randint(1, 33, npix).astype(F)
    rgb = np.exp2(rs.uniform(-6.5, 6.5, (npix, 1))).astype(F) * rs.uniform(0.8, 1.2, (npix, 3)).astype(F)
    base = np.concatenate([rgb * n[:, None], n[:, None]], axis=1).astype(F)
    e0, h0 = present.meter_host(base, 1.0, key=0.18, permille=500, adapt=1.0)
    assert h0[256] == 0 and h0[:72].sum() == 0 and h0[184:256].sum() == 0
    want = {c: present.present_host(base, e0, "accum", *c[:1], WHITE, c[1]) for c in COMBOS}
    assert all(len(np.unique(w[:, :3])) > 100 for w in want.values())
    for k in range(-8, 9):
        scaled = base.copy()
        scaled[:, :3] *= F(2.0 ** k)
        e, h = present.meter_host(scaled, 1.0, key=0.18, permille=500, adapt=1.0)
        assert _bits(e) == _bits(e0 * F(2.0 ** -k)), k
        np.testing.assert_array_equal(h[:256], np.roll(h0[:256], 8 * k), err_msg=str(k))
        for c in COMBOS:
            np.testing.assert_array_equal(present.present_host(scaled, e, "accum", c[0], WHITE, c[1]), want[c], err_msg=f"{k} {c}")


# ------------------------------------------------------------------- degenerate and boundary cases
def test_meter_boundaries():
    # nothing metered: the exposure stays, whatever it is
    nothing = np.array([[1, 1, 1, 0], [0, 0, 0, 4], [np.inf, 1, 1, 1], [-1, np.nan, -0.0, 2]], dtype=F)
    for e0 in (1.0, 0.125, 7.5):
        e, hist = present.meter_host(nothing, e0, adapt=1.0)
        assert e == F(e0) and hist[256] == 4 and hist[:256].sum() == 0
    e, hist = present.meter_host(np.zeros((0, 4), dtype=F), 3.0)
    assert e == F(3.0) and not hist.any()
    # ten grey pixels, one per octave 2^-3 .. 2^6
    lum = np.array([2.0 ** k for k in range(-3, 7)], dtype=F)
    acc = np.stack([lum * 2, lum * 2, lum * 2, np.full(10, 2, dtype=F)], axis=1)
    binl = lambda l: pm.bin_luminance(int(_bits(pm.luma(np.full((1, 3), l, dtype=F)))[0] >> 20) - pm.HIST_BIAS)
    for permille, index in ((0, 0), (500, 5), (1000, 9), (999, 9), (100, 1), (99, 0)):
        for adapt in (0.0, 0.25, 1.0):
            e, hist = present.meter_host(acc, 2.0, key=0.18, permille=permille, adapt=adapt)
            target = F(0.18) / binl(lum[index])
            want = target if adapt == 1.0 else F(F(2.0) + (target - F(2.0)) * F(adapt))
            assert _bits(e) == _bits(want), (permille, adapt)
            assert _bits(e) == _bits(pm.meter(acc, 2.0, pm.ACCUM, 0.18, permille, adapt)[0])
            if adapt == 0.0:
                assert e == F(2.0)
            assert hist[:256].sum() == 10 and hist[256] == 0
