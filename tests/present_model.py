"""cpt_present and cpt_meter_exposure restated in numpy float32: the definition of
cpppathtracer_amd/csrc/cpt_present.hpp, operation by operation, for tests/test_present_model.py (which
holds the host hooks to it) and tests/test_gpu_present.py (which holds the device to the hooks).

Every intermediate is a float32 array or scalar, so numpy rounds each operation as the C++ does; min
and max are the definition's comparisons (a NaN first operand gives the second).
"""
import numpy as np

F = np.float32
ACCUM, FILTERED = 0, 1
CLAMP, REINHARD, ACES = 0, 1, 2
LINEAR, SRGB = 0, 1
TONES = {"clamp": CLAMP, "reinhard": REINHARD, "aces": ACES}
TRANSFERS = {"linear": LINEAR, "srgb": SRGB}
HIST_BINS, HIST_BIAS = 256, 888
SHAPES = [(1, 1), (3, 5), (63, 2), (64, 4), (65, 3), (257, 9), (130, 70)]


def lesser(a, b):
    return np.where(a < b, a, b).astype(F)


def positive(a):
    return np.where(a > F(0), a, F(0)).astype(F)


def oetf(t):
    """The sRGB transfer in double, on float32 inputs."""
    t = np.asarray(t, dtype=np.float64)
    return np.where(t <= 0.0031308, 12.92 * t, 1.055 * np.power(t, 1.0 / 2.4) - 0.055)


def srgb_thresholds():
    """T[0] = 0 and T[k], k = 1..255: the smallest float32 t >= 0 with 255 oetf(t) >= k - 0.5.  By
    another route than tools/make_present_tables.py's bisection: the curve inverted in double, then
    the float32 neighbours of that estimate tried in order."""
    T = np.zeros(256, dtype=F)
    for k in range(1, 256):
        v = (k - 0.5) / 255.0
        est = v / 12.92 if v / 12.92 <= 0.0031308 else ((v + 0.055) / 1.055) ** 2.4
        bits = int(np.array(est, dtype=F).view(np.uint32))
        cand = np.arange(bits - 8, bits + 9, dtype=np.uint32).view(F)
        ok = 255.0 * oetf(cand) >= k - 0.5
        assert not ok[0] and ok[-1] and (np.diff(ok.astype(int)) >= 0).all(), k
        T[k] = cand[np.argmax(ok)]
    return T


def source_colour(source, src):
    """(c' [npix, 3], sourced [npix]) of a source plane: the accumulator [npix, 4] or the filtered rgb [npix, 3]."""
    src = np.asarray(src, dtype=F)
    if source == FILTERED:
        return positive(src.reshape(-1, 3)), np.ones(src.size // 3, dtype=bool)
    src = src.reshape(-1, 4)
    n = src[:, 3]
    ok = (n > F(0)) & np.isfinite(n)
    with np.errstate(all="ignore"):
        c = positive(src[:, :3] / n[:, None])
    c[~ok] = F(0)
    return c, ok


def tone(c, e, curve, white=4.0):
    e, w, one = F(e), F(white), F(1)
    with np.errstate(all="ignore"):
        x = lesser(c * e, F(65504.0))
        if curve == REINHARD:
            return lesser((x * (one + x / (w * w))) / (one + x), one)
        if curve == ACES:
            return lesser(positive((x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))), one)
        return lesser(x, one)


def transfer_byte(y, transfer, T):
    if transfer == LINEAR:
        return (F(255.99) * y).astype(np.int32).astype(np.uint8)
    return np.searchsorted(T[1:], y, side="right").astype(np.uint8)   # the number of k in 1..255 with T[k] <= y


def present(src, exposure, source, curve, white, transfer, T):
    """[npix, 4] uint8: B, G, R, 255."""
    c, _ = source_colour(source, src)
    b = transfer_byte(tone(c, exposure, curve, white), transfer, T)
    out = np.full((len(c), 4), 255, dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = b[:, 2], b[:, 1], b[:, 0]
    return out


def luma(c):
    return (F(0.2126) * c[:, 0] + F(0.7152) * c[:, 1]) + F(0.0722) * c[:, 2]


def histogram(src, source):
    """The 257 words: 256 luminance bins, then the pixels that are not metered."""
    c, ok = source_colour(source, src)
    with np.errstate(all="ignore"):
        l = luma(c)
    metered = ok & np.isfinite(l) & (l > F(0))
    bins = np.clip((np.ascontiguousarray(l).view(np.uint32) >> 20).astype(np.int64) - HIST_BIAS, 0, HIST_BINS - 1)
    hist = np.zeros(HIST_BINS + 1, dtype=np.uint32)
    hist[:HIST_BINS] = np.bincount(bins[metered], minlength=HIST_BINS)
    hist[HIST_BINS] = int((~metered).sum())
    return hist


def bin_luminance(b):
    return np.array((b + HIST_BIAS) << 20, dtype=np.uint32).view(F)[()]


def resolve(hist, exposure, key, permille, adapt):
    e = F(exposure)
    n = int(hist[:HIST_BINS].astype(np.uint64).sum())
    if n == 0:
        return e
    rank = min(n * permille // 1000, n - 1)
    b = int(np.argmax(np.cumsum(hist[:HIST_BINS].astype(np.uint64)) > rank))
    with np.errstate(all="ignore"):
        target = F(key) / bin_luminance(b)
        return target if F(adapt) == F(1) else F(e + (target - e) * F(adapt))


def meter(src, exposure, source, key=0.18, permille=500, adapt=1.0):
    hist = histogram(src, source)
    return resolve(hist, exposure, key, permille, adapt), hist


def hashed_floats(n, seed):
    """n float32 whose bit patterns are a hash of (seed, index): every class of float among them."""
    x = np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(F)


SPECIAL_RGB = [np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, 1e-45, 1e-40, 3e38, 65504.0, 1.0]


def synthetic_accum(npix, seed):
    """An accumulator [npix, 4]: rgb sums spread over 24 octaves times counts 1..64, and, where the
    frame has room for them, pixels with no pass, counts that are negative, infinite or NaN, and the
    special values above in each channel."""
    rs = np.random.RandomState(seed)
    n = rs.randint(1, 65, npix).astype(F)
    rgb = np.exp2(rs.uniform(-14, 10, (npix, 3))).astype(F) * n[:, None]
    acc = np.concatenate([rgb, n[:, None]], axis=1).astype(F)
    k = 0
    for bad_n in (0.0, -1.0, np.inf, np.nan):
        if k < npix - 1:
            acc[k, 3] = bad_n
            k += 1
    for v in SPECIAL_RGB:
        for ch in range(3):
            if k < npix - 1:
                acc[k, ch] = F(v)
                k += 1
    return acc
