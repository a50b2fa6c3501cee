"""Antialiased presentation (cpt_aa_coverage, cpt_present_aa) restated in numpy
float32 from the definition's text (include/cpt.h), not from cpt_antialias.hpp: the sub-sample rays,
the edge test, the attribution of a sub-sample to a pixel of the 3x3 block and the coverage-weighted
resolve.  tests/test_antialias_model.py holds the host hooks to it; tests/test_gpu_antialias.py holds
the device to the hooks.  The tone curve and the byte transfer are tests/present_model.py's.

Every intermediate is a float32 array or scalar, so numpy rounds each operation as the C++ does.
"""
import numpy as np
import present_model as pm

F = np.float32
EDGE, UNMATCHED = 1, 2
SELF = 4
BLOCK = [(k % 3 - 1, k // 3 - 1) for k in range(9)]   # (dx, dy) of pixel k of the block, row-major
SHAPES = [(1, 1), (2, 2), (3, 5), (63, 2), (65, 3)]
# the flat-colour frame of tests/test_gpu_antialias.py: tracked_reproject_model.scene() (S4 + cylinder)
# at scenes.camera_for(W, H), every normal accepted.  test_antialias_model.py checks on the CPU that
# at most FLAT_UNMATCHED_SHARE of its edge pixels are unmatched, the condition of that test.
FLAT_W, FLAT_H, FLAT_COS = 64, 48, -1.0
FLAT_UNMATCHED_SHARE = 0.05


def _v(c, name):
    return np.asarray(c[name], dtype=F).reshape(3)


def offsets(S):
    """(ox, oy) of sub-sample s = j * S + i: (2i + 1 - S) / 2S, exact floats."""
    s = np.arange(S * S)
    i, j = s % S, s // S
    return (2 * i + 1 - S).astype(F) / F(2 * S), (2 * j + 1 - S).astype(F) / F(2 * S)


def rays(cam_copy, W, H, S, x, y):
    """RayGen at zero lens offset through ((x + ox) / W, (y + oy) / H) for pixel (x, y)'s S x S
    sub-samples: (origins, directions), each [S^2, 3]."""
    c = cam_copy
    ox, oy = offsets(S)
    zero = F(0.0)
    offset = (_v(c, "u") * zero + _v(c, "v") * zero).astype(F)
    dx = ((F(x) + ox) / F(W)).astype(F)[:, None]
    dy = ((F(y) + oy) / F(H)).astype(F)[:, None]
    origin = (_v(c, "origin") + offset).astype(F)
    with np.errstate(all="ignore"):
        v = ((((_v(c, "top_left_corner") + dx * _v(c, "horizontal")) + dy * _v(c, "vertical")) - _v(c, "origin")) - offset).astype(F)
        dot = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        inv = F(1.0) / np.sqrt(dot, dtype=F)
        d = (v * inv[:, None]).astype(F)
    return np.broadcast_to(origin, d.shape).copy(), d


def _dot(a, b):
    with np.errstate(all="ignore"):
        return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def is_edge(W, H, x, y, ids, normals, cos):
    p = y * W + x
    for dx, dy in BLOCK:
        qx, qy = x + dx, y + dy
        if (dx, dy) == (0, 0) or not (0 <= qx < W and 0 <= qy < H):
            continue
        q = qy * W + qx
        if ids[q] != ids[p]:
            return True
        if ids[p] >= 0 and _dot(normals[p], normals[q]) < F(cos):
            return True
    return False


def attribute(W, H, x, y, S, s, id_s, n_s, ids, normals, cos):
    """The k the sub-sample goes to, or -1 with no match: the nearest matching in-frame pixel of the
    block, ties to k = 4 first, then to the lowest k."""
    sx, sy = 2 * (s % S) + 1 - S, 2 * (s // S) + 1 - S
    cands = []
    for k, (dx, dy) in enumerate(BLOCK):
        qx, qy = x + dx, y + dy
        if not (0 <= qx < W and 0 <= qy < H):
            continue
        q = qy * W + qx
        if ids[q] != id_s:
            continue
        if id_s != -1 and not (_dot(n_s, normals[q]) >= F(cos)):
            continue
        dist = (sx - 2 * S * dx) ** 2 + (sy - 2 * S * dy) ** 2
        cands.append((dist, 0 if k == SELF else 1, k))
    return min(cands)[2] if cands else -1


def coverage(W, H, S, cos, ids, normals, sub_id, sub_normal):
    """(counts [H, W, 9] uint8, flags [H, W] uint8)."""
    ids = np.asarray(ids, dtype=np.int32).reshape(-1)
    normals = np.asarray(normals, dtype=F).reshape(-1, 3)
    sub_id = np.asarray(sub_id, dtype=np.int32).reshape(W * H, S * S)
    sub_normal = np.asarray(sub_normal, dtype=F).reshape(W * H, S * S, 3)
    counts = np.zeros((H, W, 9), dtype=np.uint8)
    flags = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            p = y * W + x
            if not is_edge(W, H, x, y, ids, normals, cos):
                counts[y, x, SELF] = S * S
                continue
            flags[y, x] = EDGE
            for s in range(S * S):
                k = attribute(W, H, x, y, S, s, sub_id[p, s], sub_normal[p, s], ids, normals, cos)
                if k < 0:
                    flags[y, x] |= UNMATCHED
                    k = SELF
                counts[y, x, k] += 1
    return counts, flags


def toned(src, exposure, source, curve, white):
    """y [npix, 3]: every pixel after source, exposure and tone curve (before the transfer)."""
    c, _ = pm.source_colour(source, src)
    return pm.tone(c, exposure, curve, white)


def present_aa(W, H, S, src, counts, exposure, source, curve, white, transfer, T):
    """[H, W, 4] uint8: acc = 0, then acc = acc + float(c[k]) * y_k for k ascending with c[k] > 0,
    out = acc * (1 / S^2), cpt_present's transfer."""
    y = toned(src, exposure, source, curve, white).reshape(H, W, 3)
    counts = np.asarray(counts, dtype=np.uint8).reshape(H, W, 9)
    acc = np.zeros((H, W, 3), dtype=F)
    with np.errstate(all="ignore"):
        for k, (dx, dy) in enumerate(BLOCK):
            # y_k: the block's pixel k of every pixel (zeros where it is outside the frame: no count there)
            yk = np.zeros_like(y)
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            yk[yd, xd] = y[ys, xs]
            w = counts[..., k].astype(F)[..., None]
            acc = np.where(w > 0, (acc + (w * yk).astype(F)).astype(F), acc)
        out = (acc * F(F(1.0) / F(S * S))).astype(F)
    b = pm.transfer_byte(out.reshape(-1, 3), transfer, T)
    bgra = np.full((H * W, 4), 255, dtype=np.uint8)
    bgra[:, 0], bgra[:, 1], bgra[:, 2] = b[:, 2], b[:, 1], b[:, 0]
    return bgra.reshape(H, W, 4)


# --------------------------------------------------------------------------------- synthetic planes
def random_normals(n, seed):
    rs = np.random.RandomState(seed)
    v = rs.standard_normal((n, 3)).astype(F)
    return (v / np.sqrt((v * v).sum(axis=1, dtype=F), dtype=F)[:, None]).astype(F)


def planes(kind, W, H, seed=0):
    """(ids [npix], normals [npix, 3]) of a named synthetic G-buffer."""
    yy, xx = np.mgrid[0:H, 0:W]
    up = np.tile(np.array([0, 1, 0], dtype=F), (W * H, 1))
    if kind == "flat":
        return np.zeros(W * H, dtype=np.int32), up
    if kind == "vertical":
        return (xx >= W // 2).astype(np.int32).reshape(-1), up
    if kind == "horizontal":
        return (yy >= H // 2).astype(np.int32).reshape(-1), up
    if kind == "diagonal":
        return (xx + yy >= (W + H) // 2).astype(np.int32).reshape(-1), up
    if kind == "crease":   # one id, the normal turning by 90 degrees at the middle column
        n = up.copy()
        n[(xx >= W // 2).reshape(-1)] = np.array([1, 0, 0], dtype=F)
        return np.zeros(W * H, dtype=np.int32), n
    if kind == "misses":   # hits next to misses, whose normals are -dir: anything
        ids = np.where((xx + 2 * yy) % 5 < 2, -1, 3).astype(np.int32).reshape(-1)
        return ids, random_normals(W * H, seed)
    if kind == "random":
        rs = np.random.RandomState(seed)
        return rs.randint(-1, 3, W * H).astype(np.int32), random_normals(W * H, seed + 1)
    raise ValueError(kind)


KINDS = ["flat", "vertical", "horizontal", "diagonal", "crease", "misses", "random"]


def sub_hits(W, H, S, ids, normals, seed, stray=False):
    """Sub-sample hits [npix, S^2], [npix, S^2, 3] drawn from the ids and normals of each pixel's
    block (so most match somewhere); stray: some carry an id no centre of the frame holds."""
    rs = np.random.RandomState(seed)
    n = W * H
    sub_id = np.zeros((n, S * S), dtype=np.int32)
    sub_n = np.zeros((n, S * S, 3), dtype=F)
    for p in range(n):
        x, y = p % W, p // W
        for s in range(S * S):
            dx, dy = BLOCK[rs.randint(9)]
            qx, qy = min(max(x + dx, 0), W - 1), min(max(y + dy, 0), H - 1)
            q = qy * W + qx
            sub_id[p, s] = ids[q]
            sub_n[p, s] = normals[q] if rs.rand() < 0.8 else random_normals(1, rs.randint(1 << 30))[0]
            if stray and rs.rand() < 0.1:
                sub_id[p, s] = 77
    return sub_id, sub_n
