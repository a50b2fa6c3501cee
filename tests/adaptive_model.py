"""The adaptive render's criterion and round loop restated in float32 numpy (DESIGN.md §Adaptive
sampling; cpt_adaptive.hpp, cpt_capi_adaptive.cpp).

A pixel's passes do not depend on any other pixel, so the oracle renders every pixel for every
round (`oracle_rounds`: oracle.render(..., spp=batch, accumulate=True) round after round) and the
model only decides which round each 8x8 tile stops at; the expected accumulator, RNG planes, noise
map and first-hit normals take each pixel from its tile's stop round.  numpy's float32 `+ - * /` and
sqrt are the correctly rounded IEEE operations, one rounding per operation as written.
"""
import math

import numpy as np

from cpppathtracer_amd.tiling import tile_grid

F = np.float32
REL_FLOOR = F(1e-3)


def _max_keep_nan(a, b):
    return np.where(a < b, b, a).astype(np.float32)


def decide(m1, m2, k, t):
    """(converged, rel) for float32 arrays m1, m2, k and a float32 t."""
    m1, m2, k = (np.asarray(v, dtype=np.float32) for v in (m1, m2, k))
    t = F(t)
    with np.errstate(all="ignore"):
        q = _max_keep_nan(k * m2 - m1 * m1, F(0.0))
        mm = _max_keep_nan(m1, k * REL_FLOOR)
        rhs = ((k - F(1.0)) * (t * t)) * (mm * mm)
        enough = k >= F(2.0)
        rel = np.sqrt((q / (k * (k - F(1.0)))) / k) / (mm / k)
        rel = np.where(enough, rel, F(np.inf)).astype(np.float32)
        return enough & (q <= rhs), rel


def batch_luma(S, P):
    """The luminance of the batch mean between accumulators P (before) and S (after), [npix, 4]."""
    with np.errstate(all="ignore"):
        dn = S[:, 3] - P[:, 3]
        br, bg, bb = ((S[:, c] - P[:, c]) / dn for c in range(3))
        return ((F(0.2126) * br + F(0.7152) * bg) + F(0.0722) * bb).astype(np.float32)


def tile_of_pixel(width, n_rows):
    i = np.arange(n_rows * width)
    return ((i // width) // 8) * tile_grid(width, n_rows)[1] + (i % width) // 8


def oracle_rounds(oracle, objs, cam, env, rows, batch, rounds, depth, rng, acc0=None, aux=False):
    """The state after each of `rounds` rounds of `batch` passes over all pixels, from the RNG
    planes `rng` (advanced in place) and the accumulator acc0 (zeros without one):
    [(accum, rng, normal or None)] copies."""
    rows = np.asarray(rows, dtype=np.int32)
    npix = rows.size * int(np.asarray(cam["width"]).reshape(-1)[0])
    acc = np.zeros((npix, 4), dtype=np.float32) if acc0 is None else np.array(acc0, dtype=np.float32, copy=True)
    out = []
    for _ in range(rounds):
        acc, _, normal, _ = oracle.render(objs, cam, env, rows, batch, depth, rng, accum=acc, want_aux=aux,
                                          accumulate=True, threads=8)
        out.append((acc.copy(), rng.copy(), None if normal is None else normal.copy()))
    return out


def run(snaps, width, n_rows, batch, min_spp, max_spp, t, acc0=None):
    """The round loop on the per-round snapshots `snaps` of oracle_rounds.  Returns a dict: `stop`
    (each tile's stop round, 1-based), `active` (tiles rendered per round), `accum`, `rng`,
    `normal` (None without aux), `noise`, `passes_done`."""
    npix = width * n_rows
    rounds = max_spp // batch
    assert len(snaps) == rounds and min_spp % batch == 0 and max_spp % batch == 0
    tile = tile_of_pixel(width, n_rows)
    n_tiles = math.prod(tile_grid(width, n_rows))
    P = np.zeros((npix, 4), dtype=np.float32) if acc0 is None else np.array(acc0, dtype=np.float32, copy=True)
    m1, m2, k = (np.zeros(npix, dtype=np.float32) for _ in range(3))
    rel = np.full(npix, np.inf, dtype=np.float32)
    active = np.ones(n_tiles, dtype=bool)
    stop = np.zeros(n_tiles, dtype=np.int64)
    counts = []
    for r in range(1, rounds + 1):
        if not active.any():
            break
        counts.append(int(active.sum()))
        S = snaps[r - 1][0]
        act = active[tile]
        y = batch_luma(S, P)
        with np.errstate(all="ignore"):
            m1 = np.where(act, m1 + y, m1).astype(np.float32)
            m2 = np.where(act, m2 + y * y, m2).astype(np.float32)
            k = np.where(act, k + F(1.0), k).astype(np.float32)
        conv, rel_now = decide(m1, m2, k, t)
        rel = np.where(act, rel_now, rel).astype(np.float32)
        P = np.where(act[:, None], S, P)
        open_tiles = np.zeros(n_tiles, dtype=bool)
        np.logical_or.at(open_tiles, tile, ~conv)
        leave = active & (~open_tiles if r * batch >= min_spp else False)
        if r == rounds:
            leave = active.copy()
        stop[leave] = r
        active = active & ~leave
    px_stop = stop[tile]
    assert (px_stop >= 1).all()   # every tile has left the list by the last round

    def at_stop(planes, axis):   # each pixel (along `axis`) from the snapshot of its stop round
        out = planes[0].copy()
        for r in range(2, len(snaps) + 1):
            sel = np.nonzero(px_stop == r)[0]
            if axis == 0:
                out[sel] = planes[r - 1][sel]
            else:
                out[:, sel] = planes[r - 1][:, sel]
        return out

    accum = at_stop([s[0] for s in snaps], 0)
    rng = at_stop([s[1] for s in snaps], 1)
    normal = None
    if snaps[0][2] is not None:
        normal = at_stop([s[2] for s in snaps], 0)
    return dict(stop=stop, active=np.array(counts, dtype=np.uint32), accum=accum, rng=rng, normal=normal, noise=rel,
                passes_done=int(px_stop.sum()) * batch)
