"""The adaptive render's criterion on the host (cpt_adaptive_decide_host, no GPU) against its numpy
restatement (adaptive_model.decide): the decision and the noise read-out, bit for bit.  The device
runs the same header function (cpt_adaptive.hpp); tests/test_gpu_adaptive.py holds it to this model."""
import ctypes

import adaptive_model as am
import numpy as np

from cpppathtracer_amd import _lib

F = np.float32


def _host(m1, m2, k, t):
    L = _lib.load()
    conv = np.zeros(len(m1), dtype=bool)
    rel = np.zeros(len(m1), dtype=np.float32)
    c, r = ctypes.c_int(0), ctypes.c_float(0)
    for i, (a, b, kk, tt) in enumerate(zip(m1, m2, k, t)):
        st = L.cpt_adaptive_decide_host(ctypes.c_float(a), ctypes.c_float(b), ctypes.c_float(kk), ctypes.c_float(tt),
                                        ctypes.byref(c), ctypes.byref(r))
        assert st == 0
        conv[i] = c.value != 0
        rel[i] = r.value
    return conv, rel


def _same(m1, m2, k, t):
    m1, m2, k, t = (np.asarray(v, dtype=np.float32) for v in (m1, m2, k, t))
    conv, rel = _host(m1, m2, k, t)
    want_c = np.zeros(len(m1), dtype=bool)
    want_r = np.zeros(len(m1), dtype=np.float32)
    for tt in np.unique(t.view(np.uint32)).view(np.float32):   # the model takes one t at a time
        sel = t.view(np.uint32) == np.array(tt).view(np.uint32)
        want_c[sel], want_r[sel] = am.decide(m1[sel], m2[sel], k[sel], tt)
    np.testing.assert_array_equal(conv, want_c)
    # a NaN read-out is a NaN on both sides (its payload is not part of the contract)
    np.testing.assert_array_equal(np.isnan(rel), np.isnan(want_r))
    ok = ~np.isnan(rel)
    np.testing.assert_array_equal(rel[ok].view(np.uint32), want_r[ok].view(np.uint32))
    return conv, rel


def test_hashed_moments():
    """Moments of k batch means around a mean mu with spread sigma, so that both outcomes occur."""
    rs = np.random.RandomState(20241)
    n = 4000
    k = rs.randint(1, 257, n).astype(np.float32)
    mu = np.exp(rs.uniform(np.log(1e-5), np.log(50.0), n))
    sigma = mu * np.exp(rs.uniform(np.log(1e-4), np.log(3.0), n))
    m1 = (k * mu).astype(np.float32)
    m2 = (k * (mu * mu + sigma * sigma * rs.uniform(0.0, 2.0, n))).astype(np.float32)
    t = rs.choice(np.array([0.0, 0.005, 0.02, 0.1, 1.0], dtype=np.float32), n)
    conv, rel = _same(m1, m2, k, t)
    assert 0.1 * n < conv.sum() < 0.9 * n
    assert np.isfinite(rel[k >= 2]).all() and np.isinf(rel[k < 2]).all()


def test_raw_bit_patterns():
    """Any float32 at all in m1 and m2, NaN payloads and subnormals among them."""
    rs = np.random.RandomState(7)
    n = 2000
    m1 = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    m2 = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    k = rs.randint(1, 40, n).astype(np.float32)
    conv, rel = _same(m1, m2, k, np.full(n, 0.05, dtype=np.float32))
    assert np.isnan(rel).any() and conv.any() and not conv.all()


def test_edge_cases():
    inf, nan = np.inf, np.nan
    cases = [
        # m1, m2, k, t, converged
        (2.0, 2.0, 2.0, 0.01, True),        # zero variance: two means of 1
        (3.0, 3.0, 3.0, 0.0, True),         # zero variance at t = 0: 0 <= 0
        (3.0, 3.0000002, 3.0, 0.0, False),  # any variance at t = 0
        (0.3, 0.03 - 1e-9, 3.0, 0.5, True),  # k m2 - m1^2 < 0 before the clamp
        (2e-4, 3e-8, 2.0, 0.05, None),      # mean below the floor: the floor's absolute error
        (2e-4, 2e-8, 2.0, 0.05, True),
        (1.0, 1.0, 1.0, 10.0, False),       # k = 1 never converges
        (1.0, 0.5, 2.0, 10.0, True),        # k = 2 may
        (nan, 1.0, 4.0, 1.0, False),
        (1.0, nan, 4.0, 1.0, False),
        (inf, inf, 4.0, 1.0, False),
        (1.0, inf, 4.0, 1.0, False),
        (-inf, inf, 4.0, 1.0, False),
        (0.0, 0.0, 5.0, 0.0, True),         # a black pixel
    ]
    m1, m2, k, t, want = (np.array(c, dtype=object) for c in zip(*cases))
    conv, rel = _same(m1.astype(np.float32), m2.astype(np.float32), k.astype(np.float32), t.astype(np.float32))
    for i, w in enumerate(want):
        if w is not None:
            assert bool(conv[i]) == w, cases[i]
    assert np.isinf(rel[6]) and rel[0] == 0.0 and rel[13] == 0.0
    assert np.isnan(rel[8]) and np.isnan(rel[9])
    # below the floor the read-out is relative to the floor, not to the mean
    assert rel[5] < F(0.05)
