"""The variance-guided a-trous filter restated in float32 numpy, from its definition
and not from the kernel: whole-image arrays, a loop over the 25 taps in their order, `np.where`
for every skipped tap.  numpy's float32 `+ - * /` are the correctly rounded IEEE operations, one
rounding per operation as written, which is all the filter uses.

prepare() gives level 0 (mean, variance of the mean, validity) from an accumulator and moments,
level() one level, run() all of them; moments() rebuilds an adaptive render's moments from the
oracle's per-round snapshots with adaptive_model's own batch_luma.
"""
import adaptive_model as am
import numpy as np

F = np.float32
KX = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))
DEFAULTS = dict(levels=5, sigma_l=1.0, sharpness=7)


def _finite(x):
    return (x - x) == F(0.0)


def _luma(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def prepare(accum, stat):
    """accum [npix, 4], stat [4, npix] (m1, m2, k, rel) -> (plane [npix, 4] = c0 rgb + v0, valid [npix])."""
    accum = np.asarray(accum, dtype=np.float32)
    m1, m2, k = (np.asarray(stat[i], dtype=np.float32) for i in range(3))
    n = accum[:, 3]
    with np.errstate(all="ignore"):
        c = accum[:, :3] / n[:, None]
        q = k * m2 - m1 * m1
        q = np.where(q < F(0.0), F(0.0), q).astype(np.float32)     # max that keeps a NaN
        v = (q / (k * (k - F(1.0)))) / k
        valid = (n > F(0.0)) & (k >= F(2.0)) & _finite(c[:, 0]) & _finite(c[:, 1]) & _finite(c[:, 2]) & _finite(v)
    plane = np.concatenate([c, v[:, None]], axis=1).astype(np.float32)
    plane[n == F(0.0)] = F(0.0)
    return plane, valid


def _shift(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx] where that is inside the frame, `fill` elsewhere."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dx) < W and abs(dy) < H:
        b[yd, xd] = a[ys, xs]
    return b


def level(plane, normal, valid, width, height, step, sigma_l, sharpness):
    """One level at `step`: plane [npix, 4], normal [npix, 3], valid [npix] -> plane [npix, 4]."""
    P = np.asarray(plane, dtype=np.float32).reshape(height, width, 4)
    N = np.asarray(normal, dtype=np.float32).reshape(height, width, 3)
    ok = np.asarray(valid, dtype=bool).reshape(height, width)
    s = F(sigma_l)
    zero = np.zeros((height, width), dtype=np.float32)
    with np.errstate(all="ignore"):
        ly = _luma(P)
        gs, gw = zero.copy(), zero.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                g = F(0.25) if (dx, dy) == (0, 0) else F(0.125) if dx == 0 or dy == 0 else F(0.0625)
                use = _shift(ok, dx, dy, False)
                vq = _shift(P[..., 3], dx, dy, F(0.0))
                gs = np.where(use, gs + g * vq, gs).astype(np.float32)
                gw = np.where(use, gw + g, gw).astype(np.float32)
        den = (s * s) * (gs / gw) + F(1e-10)
        sw, sv = zero.copy(), zero.copy()
        sc = np.zeros((height, width, 3), dtype=np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                use = _shift(ok, step * dx, step * dy, False)
                Pq = _shift(P, step * dx, step * dy, F(0.0))
                h = KX[abs(dx)] * KX[abs(dy)]
                if (dx, dy) == (0, 0):
                    w = np.full((height, width), h, dtype=np.float32)
                else:
                    Nq = _shift(N, step * dx, step * dy, F(0.0))
                    d = ly - _luma(Pq)
                    wl = den / (den + d * d)
                    m = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                    wn = np.where(m < F(0.0), F(0.0), m).astype(np.float32)
                    for _ in range(sharpness):
                        wn = wn * wn
                    w = h * (wn * wl)
                sw = np.where(use, sw + w, sw).astype(np.float32)
                sc = np.where(use[..., None], sc + w[..., None] * Pq[..., :3], sc).astype(np.float32)
                sv = np.where(use, sv + (w * w) * Pq[..., 3], sv).astype(np.float32)
        out = np.concatenate([sc / sw[..., None], (sv / (sw * sw))[..., None]], axis=2).astype(np.float32)
    return np.where(ok[..., None], out, P).reshape(height * width, 4)


def run(accum, stat, normal, width, height, levels=5, sigma_l=1.0, sharpness=7):
    """prepare + `levels` levels: (rgb [npix, 3], variance [npix])."""
    plane, valid = prepare(accum, stat)
    for l in range(levels):
        plane = level(plane, normal, valid, width, height, 1 << l, sigma_l, sharpness)
    return plane[:, :3].copy(), plane[:, 3].copy()


SHAPES = [(1, 1), (5, 3), (20, 12), (67, 9), (130, 5)]   # width, height


def synthetic_state(width, height, seed):
    """A seeded random frame for the bit-for-bit tests: (accum [npix, 4], stat [4, npix], normal
    [npix, 3]).  Colours |c| <= 1e6 over eight decades, variances of the mean in [0, 1e3], normals
    near one of three unit directions or zero; about 5% of the pixels invalid in each of four ways:
    count 0, k = 1, a NaN colour, a +inf variance."""
    rs = np.random.RandomState(seed)
    npix = width * height
    n = rs.randint(4, 65, npix).astype(np.float32)
    c = (rs.uniform(-1.0, 1.0, (npix, 3)) * 10.0 ** rs.uniform(-2.0, 6.0, (npix, 1))).astype(np.float32)
    smooth = rs.rand(npix) < 0.5                      # half the frame: close colours, so taps count
    c[smooth] = (0.5 + 0.05 * rs.uniform(-1.0, 1.0, (int(smooth.sum()), 3))).astype(np.float32)
    accum = np.concatenate([c * n[:, None], n[:, None]], axis=1).astype(np.float32)
    k = rs.randint(2, 17, npix).astype(np.float64)
    v = np.where(smooth, rs.uniform(0.0, 1e-3, npix), rs.uniform(0.0, 1e3, npix))
    m1 = k * rs.uniform(0.0, 10.0, npix)
    m2 = m1 * m1 / k + v * k * (k - 1.0)              # (k m2 - m1^2) / (k (k - 1)) / k = v
    stat = np.stack([m1, m2, k, np.zeros(npix)]).astype(np.float32)
    dirs = np.array([[0.0, 1.0, 0.0], [0.6, 0.0, 0.8], [-0.48, 0.6, 0.64]])
    nrm = dirs[rs.randint(0, 3, npix)] + 0.02 * rs.uniform(-1.0, 1.0, (npix, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[rs.rand(npix) < 0.05] = 0.0
    kind = rs.rand(npix)
    accum[kind < 0.05] = 0.0                          # no pass
    stat[2, (kind >= 0.05) & (kind < 0.10)] = 1.0     # one batch mean
    accum[(kind >= 0.10) & (kind < 0.15), 1] = np.nan
    stat[1, (kind >= 0.15) & (kind < 0.20)] = np.inf
    return accum, stat, nrm.astype(np.float32)


def assert_same_bits(got, want, what=""):
    """Bit for bit, a NaN being a NaN on both sides (its payload is not part of the contract)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32), err_msg=what)


def moments(snaps, stop, width, n_rows, noise, acc0=None):
    """The moments [4, npix] an adaptive render leaves, from adaptive_model.oracle_rounds' snapshots
    and adaptive_model.run's stop rounds and noise map: every round a pixel's tile was active in adds
    the round's batch mean (adaptive_model.batch_luma) to m1, its square to m2 and 1 to k."""
    npix = width * n_rows
    px_stop = np.asarray(stop)[am.tile_of_pixel(width, n_rows)]
    P = np.zeros((npix, 4), dtype=np.float32) if acc0 is None else np.array(acc0, dtype=np.float32, copy=True)
    m1, m2, k = (np.zeros(npix, dtype=np.float32) for _ in range(3))
    for r in range(1, int(px_stop.max()) + 1):
        S = snaps[r - 1][0]
        act = px_stop >= r
        y = am.batch_luma(S, P)
        with np.errstate(all="ignore"):
            m1 = np.where(act, m1 + y, m1).astype(np.float32)
            m2 = np.where(act, m2 + y * y, m2).astype(np.float32)
            k = np.where(act, k + F(1.0), k).astype(np.float32)
        P = np.where(act[:, None], S, P)
    return np.stack([m1, m2, k, np.asarray(noise, dtype=np.float32)])
