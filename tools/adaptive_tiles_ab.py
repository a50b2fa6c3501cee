#!/usr/bin/env python
"""The row-tiled adaptive render against one context's, and the cost of the moments in the gather
(DESIGN.md §18 "Row tiles").  One GPU: every context sits on device 0, so the tiled figures are a
rehearsal of the call sequence (more launches, more tails, no second device), not a scaling claim.

    python tools/adaptive_tiles_ab.py render [--config c4] [--max-spp 1024] [--batch 64] [--min-spp 128]
                                             [--rel 0.05] [--contexts 1 2 8] [--repeat 3]
    python tools/adaptive_tiles_ab.py gather [--width 1920] [--height 1080] [--world 2] [--repeat 5]

render: per context count, the host wall time of the whole call (1: Renderer.render_adaptive; N > 1:
multigpu.render_adaptive_tiled into a frame context, gathers and the final waits included), the
runs interleaved over the counts, and the passes done.  With CPT_LIB_PATH naming a build that
predates cpt_adaptive_begin only `--contexts 1` works: the A/B against the parent commit runs this
tool once per library, alternately.

gather: HIP-event time on the frame context's stream of gather_rows from a rank-0-of-`world` tile
that holds moments and from the same tile without them, interleaved; the difference is
k_stitch_moments (and, the first time, nothing else: the planes exist after the warm-up).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from cpppathtracer_amd import Renderer, camera_get_copy, multigpu, scenes, texture_io, tiling
from cpppathtracer_amd._lib import CPT_RENDER_AUX, CPT_SCHEDULE_COST, CPT_TRAVERSAL_ORDERED


def render(a):
    cfg = scenes.CONFIGS[a.config]
    W, H, depth = cfg["width"], cfg["height"], cfg["depth"]
    max_spp = a.max_spp or cfg["spp"]
    flags = CPT_TRAVERSAL_ORDERED | CPT_SCHEDULE_COST | CPT_RENDER_AUX
    cam = camera_get_copy(scenes.camera_for(W, H))
    objs, sky = scenes.SCENES[cfg["scene"]](), texture_io.load_cptex()
    sets = {}
    for n in a.contexts:
        tiles = [Renderer(0) for _ in range(n)]
        for rank, t in enumerate(tiles):
            t.set_scene(objs)
            t.set_env(sky)
            t.set_frame(W, H, None if n == 1 else tiling.partition_rows(H, n, rank))
        frame = None
        if n > 1:
            frame = Renderer(0)
            frame.set_frame(W, H)
        sets[n] = (tiles, frame)
    out = dict(mode="render", config=a.config, max_spp=max_spp, batch=a.batch, min_spp=a.min_spp, rel_error=a.rel,
               lib=os.environ.get("CPT_LIB_PATH", "tree"), runs={n: [] for n in a.contexts}, passes={})
    for rep in range(a.repeat + 1):   # the first round is the warm-up
        for n in a.contexts:
            tiles, frame = sets[n]
            for t in tiles:
                t.init_rng(scenes.DEFAULT_SEED)
            t0 = time.perf_counter()
            if n == 1:
                passes = tiles[0].render_adaptive(cam, a.min_spp, max_spp, a.batch, a.rel, depth, flags=flags)["passes_done"]
            else:
                per = multigpu.render_adaptive_tiled(frame, tiles, cam, a.min_spp, max_spp, a.batch, a.rel, depth, flags=flags)
                passes = sum(p for _, p in per)
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                out["runs"][n].append(round(ms, 2))
            out["passes"][n] = passes
    for n in a.contexts:
        r = out["runs"][n]
        print(f"{n} context(s): {min(r):.1f} .. {max(r):.1f} ms (median {statistics.median(r):.1f}), "
              f"{100 * out['passes'][n] / (W * H * max_spp):.1f}% of the passes")
    assert len(set(out["passes"].values())) == 1, out["passes"]
    print(json.dumps(out))


def gather(a):
    W, H = a.width, a.height
    rows = tiling.partition_rows(H, a.world, 0)
    npix = rows.size * W
    rs = np.random.RandomState(1)
    stream = torch.cuda.Stream()
    with Renderer(0) as frame, Renderer(0) as with_m, Renderer(0) as without_m:
        frame.set_stream(stream.cuda_stream)
        frame.set_frame(W, H)
        for t in (with_m, without_m):
            t.set_frame(W, H, rows)
            t.write_aux(rs.rand(npix, 3).astype(np.float32), rs.rand(npix).astype(np.float32))
        with_m.write_moments(rs.rand(4, npix).astype(np.float32))
        moved = 2 * 32 * npix   # the moments: 32 B per pixel read and 32 B written
        out = dict(mode="gather", width=W, height=H, rows=int(rows.size), lib=os.environ.get("CPT_LIB_PATH", "tree"))
        # warm: the gathers back to back (source and destination planes, 134 MB in all, stay in
        # the 256 MB Infinity Cache); cold: a 1 GB streaming read before each one evicts them
        for state in ("warm", "cold"):
            ms = {"with": [], "without": []}
            order = (("without", without_m), ("with", with_m), ("with", with_m), ("without", without_m))
            for rep in range(a.repeat + 1):   # the first round is the warm-up (dst's planes, the row maps)
                for name, src in order:        # ABBA: what the previous gather left in the caches cancels
                    if state == "cold":
                        frame.measure_read_bandwidth(nbytes=1 << 30, iters=1)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    frame.synchronize()
                    e0.record(stream)
                    frame.gather_rows(src)
                    e1.record(stream)
                    e1.synchronize()
                    if rep:
                        ms[name].append(e0.elapsed_time(e1))
            med = {k: statistics.median(v) for k, v in ms.items()}
            added = med["with"] - med["without"]
            gbps = moved / (added * 1e6) if added > 0 else float("nan")
            out[state] = dict(ms={k: [round(x, 4) for x in v] for k, v in ms.items()}, median_ms=med, added_ms=added,
                              moments_gbps_read_plus_write=gbps)
            print(f"{state}: gather of {rows.size} rows x {W}: {med['without']:.4f} ms without moments, {med['with']:.4f} ms "
                  f"with, added {added:.4f} ms = {gbps:.0f} GB/s over {moved / 1e6:.1f} MB read + written")
        out["stream_read_gbps"] = frame.measure_read_bandwidth(nbytes=1 << 30, iters=5)
    print(f"streaming read: {out['stream_read_gbps']:.0f} GB/s")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("render")
    r.add_argument("--config", default="c4", choices=list(scenes.CONFIGS))
    r.add_argument("--max-spp", type=int, default=None, help="default: the config's spp")
    r.add_argument("--batch", type=int, default=64)
    r.add_argument("--min-spp", type=int, default=128)
    r.add_argument("--rel", type=float, default=0.05)
    r.add_argument("--contexts", type=int, nargs="+", default=[1, 2, 8])
    r.add_argument("--repeat", type=int, default=3)
    g = sub.add_parser("gather")
    g.add_argument("--width", type=int, default=1920)
    g.add_argument("--height", type=int, default=1080)
    g.add_argument("--world", type=int, default=2)
    g.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    render(a) if a.mode == "render" else gather(a)


if __name__ == "__main__":
    main()
