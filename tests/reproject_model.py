"""Float32 numpy restatement of the reprojection of the accumulated frame to a moved camera
(cpt_reproject_accum), written from the definition and not from the C code: the
yardstick tests/test_reproject_model.py holds cpt_reproject_host to bit for bit, which
tests/test_gpu_reproject.py in turn holds the kernel to.

Every expression is float32 `+ - * /`, a comparison or a floor, in the association order the
definition gives: dot(a, b) = (ax bx + ay by) + az bz; sums over the four taps run in the order
(x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) from 0 over the valid taps only.
"""
import numpy as np

import gbuffer_model as gm

F = np.float32
SNAP = F(1.0 / 32.0)
MIN_WEIGHT = F(1.0 / 64.0)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _finite(x):
    return (x - x) == 0


def _vec(c, name):
    return np.asarray(c[name], dtype=np.float32).reshape(3)


def _snap(f):
    r = np.floor(f + F(0.5))
    return np.where(np.abs(f - r) <= SNAP, r, f).astype(np.float32)


def reproject(cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1, accum, max_history, plane_tol):
    """(out [npix, 4], info): the new accumulator, and per pixel info["kind"] (0: no history,
    1: blended, 2: a tap copied unchanged) and info["own"] (taps inside the frame that carry the
    pixel's own id)."""
    W, H = int(cam0["width"]), int(cam0["height"])
    n = W * H
    dir0 = np.asarray(dir0, dtype=np.float32).reshape(n, 3)
    dir1 = np.asarray(dir1, dtype=np.float32).reshape(n, 3)
    normal1 = np.asarray(normal1, dtype=np.float32).reshape(n, 3)
    accum = np.asarray(accum, dtype=np.float32).reshape(n, 4)
    id0, id1 = np.asarray(id0, dtype=np.int32).reshape(n), np.asarray(id1, dtype=np.int32).reshape(n)
    t0, t1 = np.asarray(t0, dtype=np.float32).reshape(n), np.asarray(t1, dtype=np.float32).reshape(n)
    mh, tol = F(max_history), F(plane_tol)
    with np.errstate(all="ignore"):
        o0, o1 = _vec(cam0, "origin"), _vec(cam1, "origin")
        T = _vec(cam0, "top_left_corner") - o0
        Hh, Vv, w = _vec(cam0, "horizontal"), _vec(cam0, "vertical"), _vec(cam0, "w")
        Tw, TH, HH, TV, VV = _dot(T, w), _dot(T, Hh), _dot(Hh, Hh), _dot(T, Vv), _dot(Vv, Vv)
        # 1. the point to look up
        hit = id1 >= 0
        P = (o1 + t1[:, None] * dir1).astype(np.float32)
        q = np.where(hit[:, None], P - o0, dir1).astype(np.float32)
        # 2. into the old camera
        qw = _dot(q, w)
        ok = (qw < 0) & _finite(qw)
        s = Tw / qw
        fx = ((s * _dot(q, Hh) - TH) / HH) * F(W)
        fy = ((s * _dot(q, Vv) - TV) / VV) * F(H)
        ok &= _finite(fx) & _finite(fy)
        # 3. snap, split
        fx, fy = _snap(fx), _snap(fy)
        ok &= (fx > -1) & (fx < W) & (fy > -1) & (fy < H)   # else no tap is inside the frame
        fx, fy = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        flx, fly = np.floor(fx), np.floor(fy)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        wx, wy = (fx - flx).astype(np.float32), (fy - fly).astype(np.float32)
        bound = tol * t1
        # 4. the taps
        Wt = np.zeros(n, dtype=np.float32)
        sm = np.zeros((n, 3), dtype=np.float32)
        sn = np.zeros(n, dtype=np.float32)
        copied = np.zeros(n, dtype=bool)
        copy = np.zeros((n, 4), dtype=np.float32)
        own = np.zeros(n, dtype=np.int32)
        for b in (0, 1):
            for a in (0, 1):
                x, y = x0 + a, y0 + b
                inside = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
                k = np.where(inside, y * W + x, 0)
                A = accum[k]
                cnt = A[:, 3]
                same = inside & (id0[k] == id1)
                own += same
                valid = same & (cnt >= 1) & _finite(A[:, 0]) & _finite(A[:, 1]) & _finite(A[:, 2])
                P0 = (o0 + t0[k][:, None] * dir0[k]).astype(np.float32)
                valid &= ~hit | (np.abs(_dot(P0 - P, normal1)) <= bound)
                wgt = ((wx if a else F(1) - wx) * (wy if b else F(1) - wy)).astype(np.float32)
                take = valid & ~copied & (wgt == 1) & (cnt <= mh)
                copy[take] = A[take]
                copied |= take
                add = valid & ~copied
                Wt = np.where(add, Wt + wgt, Wt)
                sm = np.where(add[:, None], sm + wgt[:, None] * (A[:, :3] / cnt[:, None]), sm).astype(np.float32)
                sn = np.where(add, sn + wgt * cnt, sn)
        # 5. the output
        cnt_new = sn / Wt
        cap = np.floor(np.where(cnt_new < mh, cnt_new, mh)).astype(np.float32)
        good = ok & (Wt >= MIN_WEIGHT) & (cap >= 1)
        out = np.zeros((n, 4), dtype=np.float32)
        out[:, :3] = np.where(good[:, None], (sm / Wt[:, None]) * cap[:, None], F(0))
        out[:, 3] = np.where(good, cap, F(0))
        out[copied] = copy[copied]
    kind = np.where(copied, 2, np.where(good, 1, 0)).astype(np.int32)
    return out, {"kind": kind, "own": own}


# --------------------------------------------------------------------------------- fixtures
FRAMES = [(64, 48), (67, 9), (16, 16), (1, 1)]
MAX_HISTORY = 32
PLANE_TOL = 1e-2


def _cam(W, H, origin, look_at, fov=30.0):
    from cpppathtracer_amd.types import make_camera
    c = make_camera(W, H, origin=origin, look_at=look_at)
    c["view_fov"] = F(fov)
    c["lens_radius"] = F(0.0)
    return c


def camera_pairs(W, H):
    """{name: (camera the history was rendered with, new camera)}, both before camera_get_copy.
    The scenes' camera stands at (130, 103, 130) and looks at the origin, down on the floor: no
    sky.  `look_at` raises both views to the horizon, the only pair in which the sky reprojects."""
    from cpppathtracer_amd.scenes import CAMERA_LOOK_AT as AT, CAMERA_ORIGIN as O
    base = _cam(W, H, O, AT)
    away = tuple(2 * o - a for o, a in zip(O, AT))
    return {
        "identical": (base, base.copy()),
        "sideways": (base, _cam(W, H, (O[0] + 10.0, O[1], O[2] - 10.0), (AT[0] + 10.0, AT[1], AT[2] - 10.0))),
        "dolly_in": (base, _cam(W, H, tuple(0.8 * o for o in O), AT)),
        "look_at": (_cam(W, H, O, (0.0, 70.0, 0.0)), _cam(W, H, O, (8.0, 75.0, 0.0))),
        "fov": (base, _cam(W, H, O, AT, fov=36.0)),
        "away": (base, _cam(W, H, O, away)),
    }


MOVED = ("sideways", "dolly_in", "look_at", "fov")


def history(id0, W, H, seed=7):
    """A synthetic accumulator for a frame whose G-buffer ids are id0: the mean's rgb codes the
    object id plus a term that varies with the position, so a tap taken from the wrong object or the
    wrong place changes the result; pass counts of 0, 1, a few, and more than MAX_HISTORY; a block of
    pixels without any pass (about a seventh of the frame: a region a partial render left out), and
    a few NaN / inf sums."""
    rng = np.random.default_rng(seed)
    n = W * H
    x, y = np.arange(n) % W, np.arange(n) // W
    mean = np.stack([(id0 + 2) * F(0.25) + F(0.01) * x, (id0 + 2) * F(0.125) + F(0.02) * y,
                     F(0.5) + F(0.001) * (x * 3 + y * 5)], axis=1).astype(np.float32)
    cnt = rng.choice(np.array([0, 1, 3, 8, 24, 32, 40, 200], dtype=np.float32), size=n,
                     p=[0.04, 0.1, 0.2, 0.2, 0.2, 0.06, 0.1, 0.1]).astype(np.float32)
    cnt[(x * 3 >= W) & (x * 3 < 2 * W) & (y * 7 >= 2 * H) & (y * 7 < 5 * H)] = 0
    acc = np.concatenate([mean * cnt[:, None], cnt[:, None]], axis=1).astype(np.float32)
    bad = rng.choice(n, size=max(1, n // 50), replace=False) if n > 1 else np.zeros(0, dtype=np.int64)
    for j, k in enumerate(bad):
        acc[k, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    return acc


def case(oracle_mod, objs, pair):
    """The inputs of one reprojection from the numpy G-buffer model: the two cameras after
    camera_get_copy, their rays, their G-buffers and the synthetic history."""
    c0, c1 = oracle_mod.camera_get_copy(pair[0]), oracle_mod.camera_get_copy(pair[1])
    W, H = int(c0["width"]), int(c0["height"])
    (_, d0), (_, d1) = gm.camera_rays(c0), gm.camera_rays(c1)
    id0, t0, _, _ = gm.gbuffer(oracle_mod, objs, c0)
    id1, t1, n1, _ = gm.gbuffer(oracle_mod, objs, c1)
    return {"cam0": c0, "cam1": c1, "dir0": d0, "dir1": d1, "id0": id0, "t0": t0, "id1": id1, "t1": t1, "normal1": n1,
            "accum": history(id0, W, H)}
