"""cpt_bloom and cpt_present_bloom restated in numpy float32 from the definition's
text in include/cpt.h, operation by operation, for tests/test_bloom_model.py (which holds the host
hooks to it) and tests/test_gpu_bloom.py (which holds the device to the hooks).

Every intermediate is a float32 array, so numpy rounds each operation as the C++ does.  c', x, the
tone curves and the bytes are tests/present_model.py's.
"""
import numpy as np
import present_model as pm

F = np.float32
MAX_LEVELS = 8
SHAPES = [(1, 1), (2, 2), (3, 5), (63, 2), (64, 4), (65, 3), (257, 9), (9, 7), (130, 70)]
LEVELS = [1, 2, 5, 8]


def level_shapes(W, H, levels=MAX_LEVELS):
    shapes = [(W, H)]
    for _ in range(levels):
        w, h = shapes[-1]
        shapes.append(((w + 1) // 2, (h + 1) // 2))
    return shapes


def exposed(src, exposure, source, W, H):
    """x [H, W, 3]: min(c' e, 65504) per component."""
    c, _ = pm.source_colour(source, src)
    with np.errstate(all="ignore"):
        return pm.lesser(c * F(exposure), F(65504.0)).reshape(H, W, 3)


def bright(x, threshold):
    with np.errstate(all="ignore"):
        l = (F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2]
        k = np.where(l > F(0), pm.positive(l - F(threshold)) / l, F(0)).astype(F)
        return (x * k[..., None]).astype(F)


def _tap4(t0, t1, t2, t3):
    return (t0 + F(3) * t1) + (F(3) * t2 + t3)


def down(T):
    """The level below T [h, w, 3]."""
    h, w, _ = T.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    cols = [np.clip(2 * np.arange(wc) - 1 + i, 0, w - 1) for i in range(4)]
    rows = [np.clip(2 * np.arange(hc) - 1 + j, 0, h - 1) for j in range(4)]
    with np.errstate(all="ignore"):
        r = [_tap4(*[T[rows[j]][:, cols[i]] for i in range(4)]) for j in range(4)]
        return (_tap4(*r) * F(0.015625)).astype(F)


def up(T, w, h):
    """up(T) at every texel of the w x h level above T [hc, wc, 3]."""
    hc, wc, _ = T.shape
    x, y = np.arange(w), np.arange(h)
    px, py = x >> 1, y >> 1
    qx = np.clip(px + np.where(x & 1, 1, -1), 0, wc - 1)
    qy = np.clip(py + np.where(y & 1, 1, -1), 0, hc - 1)
    with np.errstate(all="ignore"):
        h0 = F(3) * T[py][:, px] + T[py][:, qx]
        h1 = F(3) * T[qy][:, px] + T[qy][:, qx]
        return ((F(3) * h0 + h1) * F(0.0625)).astype(F)


def pyramid(W, H, src, exposure, source, threshold, levels):
    """(x [H, W, 3], [None, U_1, .., U_levels])."""
    x = exposed(src, exposure, source, W, H)
    B = [bright(x, threshold)]
    for _ in range(levels):
        B.append(down(B[-1]))
    U = [None] * (levels + 1)
    U[levels] = B[levels]
    for l in range(levels - 1, 0, -1):
        with np.errstate(all="ignore"):
            U[l] = (B[l] + up(U[l + 1], B[l].shape[1], B[l].shape[0])).astype(F)
    return x, U


def present_bloom(W, H, src, exposure, source, threshold, levels, intensity, curve, white, transfer, T):
    """[H, W, 4] uint8: B, G, R, 255."""
    x, U = pyramid(W, H, src, exposure, source, threshold, levels)
    with np.errstate(all="ignore"):
        xp = (x + F(intensity) * up(U[1], W, H)).astype(F)
    b = pm.transfer_byte(pm.tone(xp.reshape(-1, 3), 1.0, curve, white), transfer, T)
    out = np.full((W * H, 4), 255, dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = b[:, 2], b[:, 1], b[:, 0]
    return out.reshape(H, W, 4)


def reach():
    """How far from a source pixel, in frame pixels per axis, each number of levels can move light,
    from the taps alone.  A texel X of level l + 1 reads level-l columns 2X-1..2X+2, so a level-l
    column c is read by the texels X with 2X-1 <= c <= 2X+2: an interval [lo, hi] of level l becomes
    [(lo - 2 + 1) // 2, (hi + 1) // 2] one level down (ceil((lo - 2) / 2), floor((hi + 1) / 2)).
    up at x reads x >> 1 and its neighbour on x's side, so a coarse interval [lo, hi] reaches the
    fine columns 2 lo - 1 .. 2 hi + 2.  Returns f(p, L): the frame interval (lo, hi) a pixel at
    column p can change with L levels, before clamping to the frame."""
    def f(p, L):
        lo = hi = p
        for _ in range(L):
            lo, hi = (lo - 1) // 2, (hi + 1) // 2
        for _ in range(L):
            lo, hi = 2 * lo - 1, 2 * hi + 2
        return lo, hi
    return f
