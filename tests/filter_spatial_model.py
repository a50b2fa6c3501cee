"""The filter for frames without moments restated in float32 numpy, from its definition (DESIGN.md
§25) and not from the kernel: whole-image arrays shifted per tap, the taps in their stated order,
`np.where` for every skipped tap.  numpy's float32 `+ - * /` are the correctly rounded IEEE
operations, one rounding per operation as written, which is all the filter uses.

prepare() gives level 0 (mean, spatial variance of the mean, validity) from an accumulator and the
G-buffer's id and normal planes, level() one level with the stop at object boundaries, run() all of
them.  synthetic_state() and id_plane() are the seeded inputs of the bit-for-bit tests, on the host
(test_filter_spatial_model.py) and on the device (test_gpu_filter_spatial.py).
"""
import numpy as np
from filter_model import KX, _finite, _luma, _shift, assert_same_bits  # noqa: F401  (re-exported)

F = np.float32
RADIUS = 3
DEFAULTS = dict(levels=3, sigma_l=2.0, sharpness=3)
SHAPES = [(1, 1), (5, 3), (20, 12), (67, 9), (130, 5)]   # width, height
ID_KINDS = ("one", "vstripes", "hstripes", "checker", "miss")


def _wn(N, Nq, sharpness):
    m = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
    wn = np.where(m < F(0.0), F(0.0), m).astype(np.float32)     # max that keeps a NaN
    for _ in range(sharpness):
        wn = wn * wn
    return wn


def base(accum):
    """accum [npix, 4] -> (c0 [npix, 3], b [npix]): the mean (0 where the count is 0) and base validity."""
    accum = np.asarray(accum, dtype=np.float32)
    n = accum[:, 3]
    with np.errstate(all="ignore"):
        c = (accum[:, :3] / n[:, None]).astype(np.float32)
        b = (n > F(0.0)) & _finite(n) & _finite(c[:, 0]) & _finite(c[:, 1]) & _finite(c[:, 2])
    c[n == F(0.0)] = F(0.0)
    return c, b


def prepare(accum, ids, normal, width, height, sharpness):
    """accum [npix, 4], ids [npix], normal [npix, 3] -> (plane [npix, 4] = c0 rgb + v0, valid [npix])."""
    accum = np.asarray(accum, dtype=np.float32)
    c, b = base(accum)
    with np.errstate(all="ignore"):
        L = _luma(c).reshape(height, width)
    n = accum[:, 3].reshape(height, width)
    B = b.reshape(height, width)
    I = np.asarray(ids, dtype=np.int32).reshape(height, width)
    N = np.asarray(normal, dtype=np.float32).reshape(height, width, 3)
    zero = np.zeros((height, width), dtype=np.float32)
    taps = [(dx, dy) for dy in range(-RADIUS, RADIUS + 1) for dx in range(-RADIUS, RADIUS + 1)]

    def tap(dx, dy):
        inside = _shift(np.ones((height, width), dtype=bool), dx, dy, False)
        use = inside & _shift(B, dx, dy, False) & (_shift(I, dx, dy, 0) == I)
        w = np.ones((height, width), dtype=np.float32) if (dx, dy) == (0, 0) else _wn(N, _shift(N, dx, dy, F(0.0)), sharpness)
        return use, w, w * _shift(n, dx, dy, F(0.0)), _shift(L, dx, dy, F(0.0))

    with np.errstate(all="ignore"):
        A, Bs, W = zero.copy(), zero.copy(), zero.copy()
        m = np.zeros((height, width), dtype=np.int32)
        for dx, dy in taps:
            use, w, a, lq = tap(dx, dy)
            A = np.where(use, A + a, A).astype(np.float32)
            Bs = np.where(use, Bs + a * lq, Bs).astype(np.float32)
            W = np.where(use, W + w, W).astype(np.float32)
            m = np.where(use & (w > F(0.0)), m + 1, m)
        mu = Bs / A
        D = zero.copy()
        for dx, dy in taps:
            use, w, a, lq = tap(dx, dy)
            d = lq - mu
            D = np.where(use, D + a * (d * d), D).astype(np.float32)
        mf = m.astype(np.float32)
        s2 = np.where(m >= 2, (D / W) * (mf / (mf - F(1.0))), F(0.0)).astype(np.float32)
        v = (s2 / n).reshape(-1).astype(np.float32)
        v = np.where(b, v, F(0.0)).astype(np.float32)
        valid = b & _finite(v)
    return np.concatenate([c, v[:, None]], axis=1).astype(np.float32), valid


def level(plane, normal, ids, valid, width, height, step, sigma_l, sharpness):
    """One level at `step` with the id stop: plane [npix, 4] -> plane [npix, 4]."""
    P = np.asarray(plane, dtype=np.float32).reshape(height, width, 4)
    N = np.asarray(normal, dtype=np.float32).reshape(height, width, 3)
    I = np.asarray(ids, dtype=np.int32).reshape(height, width)
    ok = np.asarray(valid, dtype=bool).reshape(height, width)
    s = F(sigma_l)
    zero = np.zeros((height, width), dtype=np.float32)

    def usable(dx, dy):
        return _shift(ok, dx, dy, False) & (_shift(I, dx, dy, 0) == I)

    with np.errstate(all="ignore"):
        ly = _luma(P)
        gs, gw = zero.copy(), zero.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                g = F(0.25) if (dx, dy) == (0, 0) else F(0.125) if dx == 0 or dy == 0 else F(0.0625)
                use = usable(dx, dy)
                vq = _shift(P[..., 3], dx, dy, F(0.0))
                gs = np.where(use, gs + g * vq, gs).astype(np.float32)
                gw = np.where(use, gw + g, gw).astype(np.float32)
        den = (s * s) * (gs / gw) + F(1e-10)
        sw, sv = zero.copy(), zero.copy()
        sc = np.zeros((height, width, 3), dtype=np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                use = usable(step * dx, step * dy)
                Pq = _shift(P, step * dx, step * dy, F(0.0))
                h = KX[abs(dx)] * KX[abs(dy)]
                if (dx, dy) == (0, 0):
                    w = np.full((height, width), h, dtype=np.float32)
                else:
                    d = ly - _luma(Pq)
                    wl = den / (den + d * d)
                    w = h * (_wn(N, _shift(N, step * dx, step * dy, F(0.0)), sharpness) * wl)
                sw = np.where(use, sw + w, sw).astype(np.float32)
                sc = np.where(use[..., None], sc + w[..., None] * Pq[..., :3], sc).astype(np.float32)
                sv = np.where(use, sv + (w * w) * Pq[..., 3], sv).astype(np.float32)
        out = np.concatenate([sc / sw[..., None], (sv / (sw * sw))[..., None]], axis=2).astype(np.float32)
    return np.where(ok[..., None], out, P).reshape(height * width, 4)


def run(accum, ids, normal, width, height, levels=3, sigma_l=2.0, sharpness=3):
    """prepare + `levels` levels: (rgb [npix, 3], variance [npix])."""
    plane, valid = prepare(accum, ids, normal, width, height, sharpness)
    for l in range(levels):
        plane = level(plane, normal, ids, valid, width, height, 1 << l, sigma_l, sharpness)
    return plane[:, :3].copy(), plane[:, 3].copy()


def id_plane(width, height, kind):
    """The id planes of the tests: one object; vertical stripes with a boundary between x = 63 and
    64 (the block seam); horizontal stripes with one between y = 3 and 4; a checkerboard of
    one-pixel objects; one object with a region of -1 (a miss)."""
    y, x = np.mgrid[0:height, 0:width]
    if kind == "one":
        ids = np.full((height, width), 3)
    elif kind == "vstripes":
        ids = (x + 64) // 32           # boundaries at x = 32, 64, 96, ...
    elif kind == "hstripes":
        ids = y // 4                   # boundaries at y = 4, 8, ...
    elif kind == "checker":
        ids = (x + y) % 2
    elif kind == "miss":
        ids = np.full((height, width), 2)
        ids[height // 3:, width // 2:] = -1
    else:
        raise ValueError(kind)
    return ids.astype(np.int32).reshape(-1)


def synthetic_state(width, height, seed, nan_normal=False):
    """A seeded random frame: (accum [npix, 4], normal [npix, 3]).  Counts from 1..32; half the
    frame near 0.5 so that taps count, the rest over eight decades; normals near one of three unit
    directions or zero; about 5% of the pixels invalid in each of four ways: count 0, a NaN sum, an
    infinite sum, an infinite count.  nan_normal: one pixel's normal is NaN."""
    rs = np.random.RandomState(seed)
    npix = width * height
    n = rs.randint(1, 33, npix).astype(np.float32)
    c = (rs.uniform(-1.0, 1.0, (npix, 3)) * 10.0 ** rs.uniform(-2.0, 6.0, (npix, 1))).astype(np.float32)
    smooth = rs.rand(npix) < 0.5
    c[smooth] = (0.5 + 0.05 * rs.uniform(-1.0, 1.0, (int(smooth.sum()), 3))).astype(np.float32)
    accum = np.concatenate([c * n[:, None], n[:, None]], axis=1).astype(np.float32)
    dirs = np.array([[0.0, 1.0, 0.0], [0.6, 0.0, 0.8], [-0.48, 0.6, 0.64]])
    nrm = dirs[rs.randint(0, 3, npix)] + 0.02 * rs.uniform(-1.0, 1.0, (npix, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[rs.rand(npix) < 0.05] = 0.0
    kind = rs.rand(npix)
    accum[kind < 0.05] = 0.0                                    # no pass
    accum[(kind >= 0.05) & (kind < 0.10), 1] = np.nan
    accum[(kind >= 0.10) & (kind < 0.15), 2] = np.inf
    accum[(kind >= 0.15) & (kind < 0.20), 3] = np.inf
    nrm = nrm.astype(np.float32)
    if nan_normal:
        nrm[npix // 2] = np.nan
    return accum, nrm
