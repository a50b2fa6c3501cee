#!/usr/bin/env python
"""The a-trous filter on an adaptive render of a benchmark config.

C4 by default (S1000, 1920 x 1080, depth 16), one GPU.  The reference image is one plain render of
--ref-spp passes of the same frame.  For each --rel value: render_adaptive (with first-hit normals),
then filter_frame; reported are the RMSE of the mean image against the reference, unfiltered and
filtered (the defaults and each --params set), the filter's device time in total and per level (the
median of --repeat calls after a warm-up; level l = the time of l + 1 levels less the time of l
levels, level -1 = the prepare launch alone), its share of the adaptive call's wall time, and per
level the algorithmic bytes (16 B read + 16 B written + 12 B normal per pixel) over the time, beside
the box's measured streaming-read bandwidth.

    python tools/filter_ab.py [--config c4] [--max-spp 1024] [--batch 64] [--min-spp 128]
                              [--rel 0.02 0.05] [--ref-spp 4096] [--levels 5] [--repeat 5]
                              [--params 5,4,7 3,1,3] [--json out.json]
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
from cpppathtracer_amd._lib import CPT_RENDER_AUX, CPT_SCHEDULE_COST, CPT_TRAVERSAL_ORDERED


def mean_image(acc):
    return (acc[:, :3] / np.maximum(acc[:, 3:4], 1.0)).astype(np.float64)


def rmse(a, ref):
    return float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))


def filter_ms(r, levels, sigma_l, sharp, repeat):
    r.filter_frame(levels, sigma_l, sharp)
    r.last_filter_ms()   # warm-up
    ms = []
    for _ in range(repeat):
        r.filter_frame(levels, sigma_l, sharp)
        ms.append(r.last_filter_ms())
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=list(scenes.CONFIGS))
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--min-spp", type=int, default=128)
    ap.add_argument("--rel", type=float, nargs="+", default=[0.02, 0.05])
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--sigma-l", type=float, default=1.0)
    ap.add_argument("--sharpness", type=int, default=7)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--params", nargs="*", default=[], help="further levels,sigma_l,sharpness sets (RMSE only)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    cfg = scenes.CONFIGS[a.config]
    W, H, depth = cfg["width"], cfg["height"], cfg["depth"]
    flags = CPT_TRAVERSAL_ORDERED | CPT_SCHEDULE_COST
    cam = camera_get_copy(scenes.camera_for(W, H))
    out = dict(config=a.config, width=W, height=H, depth=depth, max_spp=a.max_spp, batch=a.batch, min_spp=a.min_spp,
               ref_spp=a.ref_spp, levels=a.levels, sigma_l=a.sigma_l, sharpness=a.sharpness, runs=[])
    level_bytes = W * H * (16 + 16 + 12)
    with Renderer(0) as r:
        r.set_scene(scenes.SCENES[cfg["scene"]]())
        r.set_env(texture_io.load_cptex())
        r.set_frame(W, H)
        r.init_rng(scenes.DEFAULT_SEED + 1)   # a reference independent of the renders it judges
        t0 = time.perf_counter()
        r.render(cam, a.ref_spp, depth, sync=True, flags=flags)
        ref = mean_image(r.read_accum())
        print(f"reference: plain {a.ref_spp} spp, {(time.perf_counter() - t0) * 1e3:.0f} ms", flush=True)
        out["read_bandwidth_gbps"] = r.measure_read_bandwidth(1 << 30, 5)
        print(f"streaming-read bandwidth {out['read_bandwidth_gbps']:.0f} GB/s", flush=True)
        for rel in a.rel:
            r.init_rng(scenes.DEFAULT_SEED)
            t0 = time.perf_counter()
            info = r.render_adaptive(cam, a.min_spp, a.max_spp, a.batch, rel, depth, flags=flags | CPT_RENDER_AUX)
            adaptive_ms = (time.perf_counter() - t0) * 1e3
            unfiltered = rmse(mean_image(r.read_accum()), ref)
            noise = r.read_noise()
            totals = [filter_ms(r, l, a.sigma_l, a.sharpness, a.repeat) for l in range(a.levels + 1)]
            r.filter_frame(a.levels, a.sigma_l, a.sharpness)
            rgb, var = r.read_filtered()
            run = dict(rel_error=rel, adaptive_ms=adaptive_ms, passes_share=info["passes_done"] / (W * H * a.max_spp),
                       rmse_unfiltered=unfiltered, rmse_filtered=rmse(rgb, ref), noise_max=float(noise.max()),
                       filter_ms=totals[-1], prepare_ms=totals[0],
                       level_ms=[totals[l + 1] - totals[l] for l in range(a.levels)],
                       filter_share=totals[-1] / (adaptive_ms + totals[-1]),
                       variance_median=float(np.median(var)), other=[])
            run["level_gbps"] = [level_bytes / (ms * 1e-3) / 1e9 if ms > 0 else None for ms in run["level_ms"]]
            print(f"rel_error {rel}: adaptive {adaptive_ms:.1f} ms ({100 * run['passes_share']:.1f}% of the passes), RMSE vs "
                  f"reference unfiltered {unfiltered:.5f} filtered {run['rmse_filtered']:.5f}; filter {totals[-1]:.3f} ms "
                  f"({100 * run['filter_share']:.3f}% of adaptive + filter), prepare {totals[0]:.3f} ms")
            for l, (ms, gb) in enumerate(zip(run["level_ms"], run["level_gbps"])):
                print(f"  level {l} (step {1 << l}): {ms:.3f} ms, {gb:.0f} GB/s algorithmic" if gb else f"  level {l}: {ms:.3f} ms")
            for spec in a.params:
                lv, sg, sh = spec.split(",")
                r.filter_frame(int(lv), float(sg), int(sh))
                e = rmse(r.read_filtered()[0], ref)
                run["other"].append(dict(levels=int(lv), sigma_l=float(sg), sharpness=int(sh), rmse_filtered=e))
                print(f"  levels {lv} sigma_l {sg} sharpness {sh}: RMSE filtered {e:.5f}")
            sys.stdout.flush()
            out["runs"].append(run)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
