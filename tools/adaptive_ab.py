#!/usr/bin/env python
"""Adaptive render against the plain one on a benchmark config (DESIGN.md §Adaptive sampling).

C4 by default (S1000, 1920 x 1080, depth 16), one GPU: a plain render of max_spp passes, then
render_adaptive at each --rel value with the same walk and schedule flags.  Per run: the host wall
time of the call (the adaptive render waits for every round, so this is what a caller sees; the
plain render's HIP-event time beside it), the share of the plain render's pixel passes that ran,
the rounds, the tiles each round rendered, and the RMSE of the mean image against the plain one.

    python tools/adaptive_ab.py [--config c4] [--max-spp 1024] [--batch 64] [--min-spp 128]
                                [--rel 0.01 0.02 0.05] [--repeat 2] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: torch's)

from cpppathtracer_amd import Renderer, camera_get_copy, scenes, texture_io
from cpppathtracer_amd._lib import CPT_SCHEDULE_COST, CPT_TRAVERSAL_ORDERED


def mean_image(acc):
    return acc[:, :3] / np.maximum(acc[:, 3:4], 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=list(scenes.CONFIGS))
    ap.add_argument("--max-spp", type=int, default=None, help="default: the config's spp")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--min-spp", type=int, default=128)
    ap.add_argument("--rel", type=float, nargs="+", default=[0.01, 0.02, 0.05])
    ap.add_argument("--repeat", type=int, default=2, help="timed runs of each render (the best is kept)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    cfg = scenes.CONFIGS[a.config]
    W, H, depth = cfg["width"], cfg["height"], cfg["depth"]
    max_spp = a.max_spp or cfg["spp"]
    flags = CPT_TRAVERSAL_ORDERED | CPT_SCHEDULE_COST
    cam = camera_get_copy(scenes.camera_for(W, H))
    out = dict(config=a.config, width=W, height=H, depth=depth, max_spp=max_spp, batch=a.batch, min_spp=a.min_spp, runs=[])
    with Renderer(0) as r:
        r.set_scene(scenes.SCENES[cfg["scene"]]())
        r.set_env(texture_io.load_cptex())
        r.set_frame(W, H)
        plain_ms, plain_event_ms = [], []
        for _ in range(a.repeat):
            r.init_rng(scenes.DEFAULT_SEED)
            t0 = time.perf_counter()
            r.render(cam, max_spp, depth, sync=True, flags=flags)
            plain_ms.append((time.perf_counter() - t0) * 1e3)
            plain_event_ms.append(r.last_render_ms())
        ref = mean_image(r.read_accum())
        out["plain"] = dict(ms=min(plain_ms), event_ms=min(plain_event_ms))
        print(f"plain {max_spp} spp: {min(plain_ms):.1f} ms (HIP events {min(plain_event_ms):.1f} ms)")
        for rel in a.rel:
            ms = []
            for _ in range(a.repeat):
                r.init_rng(scenes.DEFAULT_SEED)
                t0 = time.perf_counter()
                info = r.render_adaptive(cam, a.min_spp, max_spp, a.batch, rel, depth, flags=flags)
                ms.append((time.perf_counter() - t0) * 1e3)
            acc = r.read_accum()
            rmse = float(np.sqrt(np.mean((mean_image(acc).astype(np.float64) - ref) ** 2)))
            share = info["passes_done"] / (W * H * max_spp)
            noise = r.read_noise()
            run = dict(rel_error=rel, ms=min(ms), passes_share=share, rounds=info["rounds"],
                       active_tiles=[int(x) for x in info["active_tiles"]], rmse_vs_plain=rmse,
                       noise_median=float(np.median(noise)), noise_max=float(noise.max()))
            out["runs"].append(run)
            print(f"rel_error {rel}: {run['ms']:.1f} ms ({run['ms'] / out['plain']['ms']:.2f} x plain), "
                  f"{100 * share:.1f}% of the passes, {run['rounds']} rounds, RMSE vs plain {rmse:.5f}, "
                  f"noise median {run['noise_median']:.4f} max {run['noise_max']:.4f}")
            print("  tiles per round:", run["active_tiles"])
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
