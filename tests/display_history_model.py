"""Float32 numpy restatement of the reprojection of the display state to a moved camera
(cpt_reproject_display), written from the definition and not from the C code: the
yardstick tests/test_display_history_model.py holds cpt_reproject_display_host to bit for bit, which
tests/test_gpu_display_history.py in turn holds the kernel to.

The geometry is reproject_model's (the projection, the snap, the frame bounds, the id test, the
tangent-plane test, the order of the taps and of every expression); what is blended differs: the Mix
mean as it is and the per-pixel sample count beside it, from taps inside the display's launch
region W' x H' = 16 floor(W / 16) x 16 floor(H / 16) only, into pixels of that region only.
"""
import numpy as np

import reproject_model as rm
from reproject_model import F, MIN_WEIGHT, _dot, _finite, _snap, _vec

FRAMES = [(64, 48), (67, 41), (16, 16)]
MAX_HISTORY = rm.MAX_HISTORY
PLANE_TOL = rm.PLANE_TOL
MOVED = rm.MOVED
camera_pairs = rm.camera_pairs


def launch_region(W, H):
    return 16 * (W // 16), 16 * (H // 16)


def reproject_display(cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1, mean, count, max_history, plane_tol):
    """(mean [npix, 3], count [npix], info): the new display state, and per pixel info["kind"]
    (0: no history, 1: blended, 2: a tap copied unchanged)."""
    W, H = int(cam0["width"]), int(cam0["height"])
    We, He = launch_region(W, H)
    n = W * H
    dir0 = np.asarray(dir0, dtype=np.float32).reshape(n, 3)
    dir1 = np.asarray(dir1, dtype=np.float32).reshape(n, 3)
    normal1 = np.asarray(normal1, dtype=np.float32).reshape(n, 3)
    mean = np.asarray(mean, dtype=np.float32).reshape(n, 3)
    count = np.asarray(count, dtype=np.float32).reshape(n)
    id0, id1 = np.asarray(id0, dtype=np.int32).reshape(n), np.asarray(id1, dtype=np.int32).reshape(n)
    t0, t1 = np.asarray(t0, dtype=np.float32).reshape(n), np.asarray(t1, dtype=np.float32).reshape(n)
    mh, tol = F(max_history), F(plane_tol)
    px, py = np.arange(n) % W, np.arange(n) // W
    with np.errstate(all="ignore"):
        o0, o1 = _vec(cam0, "origin"), _vec(cam1, "origin")
        T = _vec(cam0, "top_left_corner") - o0
        Hh, Vv, w = _vec(cam0, "horizontal"), _vec(cam0, "vertical"), _vec(cam0, "w")
        Tw, TH, HH, TV, VV = _dot(T, w), _dot(T, Hh), _dot(Hh, Hh), _dot(T, Vv), _dot(Vv, Vv)
        hit = id1 >= 0
        P = (o1 + t1[:, None] * dir1).astype(np.float32)
        q = np.where(hit[:, None], P - o0, dir1).astype(np.float32)
        qw = _dot(q, w)
        ok = (qw < 0) & _finite(qw)
        s = Tw / qw
        fx = ((s * _dot(q, Hh) - TH) / HH) * F(W)
        fy = ((s * _dot(q, Vv) - TV) / VV) * F(H)
        ok &= _finite(fx) & _finite(fy)
        fx, fy = _snap(fx), _snap(fy)
        ok &= (fx > -1) & (fx < W) & (fy > -1) & (fy < H)
        ok &= (px < We) & (py < He)   # a pixel outside the launch region holds nothing
        fx, fy = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        flx, fly = np.floor(fx), np.floor(fy)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        wx, wy = (fx - flx).astype(np.float32), (fy - fly).astype(np.float32)
        bound = tol * t1
        Wt = np.zeros(n, dtype=np.float32)
        sm = np.zeros((n, 3), dtype=np.float32)
        sn = np.zeros(n, dtype=np.float32)
        copied = np.zeros(n, dtype=bool)
        copy_m = np.zeros((n, 3), dtype=np.float32)
        copy_n = np.zeros(n, dtype=np.float32)
        for b in (0, 1):
            for a in (0, 1):
                x, y = x0 + a, y0 + b
                inside = ok & (x >= 0) & (x < We) & (y >= 0) & (y < He)   # the launch region, not the frame
                k = np.where(inside, y * W + x, 0)
                m, cnt = mean[k], count[k]
                valid = inside & (id0[k] == id1) & (cnt >= 1) & _finite(m[:, 0]) & _finite(m[:, 1]) & _finite(m[:, 2])
                P0 = (o0 + t0[k][:, None] * dir0[k]).astype(np.float32)
                valid &= ~hit | (np.abs(_dot(P0 - P, normal1)) <= bound)
                wgt = ((wx if a else F(1) - wx) * (wy if b else F(1) - wy)).astype(np.float32)
                take = valid & ~copied & (wgt == 1) & (cnt <= mh)
                copy_m[take], copy_n[take] = m[take], cnt[take]
                copied |= take
                add = valid & ~copied
                Wt = np.where(add, Wt + wgt, Wt)
                sm = np.where(add[:, None], sm + wgt[:, None] * m, sm).astype(np.float32)
                sn = np.where(add, sn + wgt * cnt, sn)
        cnt_new = sn / Wt
        cap = np.floor(np.where(cnt_new < mh, cnt_new, mh)).astype(np.float32)
        good = ok & (Wt >= MIN_WEIGHT) & (cap >= 1)
        out_m = np.where(good[:, None], sm / Wt[:, None], F(0)).astype(np.float32)
        out_n = np.where(good, cap, F(0)).astype(np.float32)
        out_m[copied], out_n[copied] = copy_m[copied], copy_n[copied]
    kind = np.where(copied, 2, np.where(good, 1, 0)).astype(np.int32)
    return out_m, out_n, {"kind": kind}


def display_state(id0, W, H, seed=11):
    """A synthetic display state for a frame whose G-buffer ids are id0: a mean in [0, 1] that codes
    the object id and the position, counts of 0, 1, a few and above MAX_HISTORY, a block without any
    sample, a few NaN / inf means.  Outside the launch region the planes hold what no display pass
    could have left there (a mean of 0.5 and 7 samples): history there must be ignored."""
    rng = np.random.default_rng(seed)
    We, He = launch_region(W, H)
    n = W * H
    x, y = np.arange(n) % W, np.arange(n) // W
    mean = np.stack([((id0 + 2) % 5) * F(0.125) + F(0.004) * x, ((id0 + 2) % 3) * F(0.25) + F(0.006) * y,
                     F(0.25) + F(0.001) * (x * 3 + y * 5)], axis=1).astype(np.float32)
    cnt = rng.choice(np.array([0, 1, 3, 8, 24, 32, 40, 200], dtype=np.float32), size=n,
                     p=[0.04, 0.1, 0.2, 0.2, 0.2, 0.06, 0.1, 0.1]).astype(np.float32)
    cnt[(x * 3 >= W) & (x * 3 < 2 * W) & (y * 7 >= 2 * H) & (y * 7 < 5 * H)] = 0
    mean[cnt == 0] = 0
    bad = rng.choice(n, size=max(1, n // 50), replace=False)
    for j, k in enumerate(bad):
        mean[k, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    outside = (x >= We) | (y >= He)
    mean[outside] = F(0.5)
    cnt[outside] = F(7)
    return mean, cnt


def case(oracle_mod, objs, pair):
    """The inputs of one reprojection: reproject_model.case's geometry with the synthetic display
    state in place of the accumulator."""
    c = rm.case(oracle_mod, objs, pair)
    del c["accum"]
    W, H = int(c["cam0"]["width"]), int(c["cam0"]["height"])
    c["mean"], c["count"] = display_state(c["id0"], W, H)
    return c
