#!/usr/bin/env python3
"""Measurements behind cpt_reproject_accum.

    python tools/reproject_ab.py [--timing] [--quality] > profiles/r13/reproject_ab.log

--timing   S1000 at 1920x1080 (the C4 frame): medians of 5 after a warm-up of cpt_last_reproject_ms
           split into its three launches, beside two cpt_gbuffer calls, and the look-up kernel's
           algorithmic bytes over the measured HBM read rate (cpt_measure_read_bandwidth).
--quality  S4 and S1000 at 256x144, depth 8, a small orbit step: 32 spp at C0 reprojected to C1 plus k
           new passes against a restart of k passes, k in {1, 4, 16}; MSE to 4096 spp at C1, for the
           whole frame and for the pixels that see the diffuse floor; max_history in {8, 32, 128},
           plane_tol in {1e-3, 1e-2, 1e-1}.
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpppathtracer_amd import Renderer, camera_get_copy, scenes, texture_io   # noqa: E402
from cpppathtracer_amd._lib import CPT_TRAVERSAL_ORDERED as ORD                # noqa: E402


def moved(cam, step):
    c = cam.copy()
    for k in ("origin", "look_at"):
        c[k] = np.asarray(cam[k], np.float32) + np.array([step, 0.0, -step], np.float32)
    return c


def timing(r):
    W, H = 1920, 1080
    base = scenes.camera_for(W, H)
    c0, c1 = camera_get_copy(base), camera_get_copy(moved(base, 1.0))
    r.set_scene(scenes.scene_s1000())
    r.set_env(texture_io.load_cptex())
    r.set_frame(W, H)
    r.init_rng(scenes.DEFAULT_SEED)
    r.render(c0, 4, 8, sync=True, ordered=True)
    hist = r.read_accum()
    runs, gb = [], []
    for i in range(6):
        r.write_accum(hist)
        r.reproject_accum(c0, c1, flags=ORD)
        runs.append(r.last_reproject_ms(split=True))
        two = 0.0
        for c in (c0, c1):
            r.gbuffer(c, ORD)
            two += r.last_query_ms()
        gb.append(two)
    med = [statistics.median(x[k] for x in runs[1:]) for k in range(3)]
    gbps = r.measure_read_bandwidth()
    npix = W * H
    # per pixel: id1, t1 (8 B), normal1 (12 B), the old frame's accumulator, id and t once each
    # (16 + 8 B: neighbouring lanes share their taps), the output (16 B)
    algo = npix * (8 + 12 + 16 + 8 + 16)
    floor_ms = algo / (gbps * 1e9) * 1e3
    print(f"timing S1000 {W}x{H}: trace(from) {med[0]:.4f} ms, trace(to) {med[1]:.4f} ms, k_reproject_accum {med[2]:.4f} ms, "
          f"total {sum(med):.4f} ms; two cpt_gbuffer calls {statistics.median(gb[1:]):.4f} ms")
    print(f"  look-up kernel: {algo / 1e6:.1f} MB algorithmic over {gbps:.0f} GB/s = {floor_ms:.4f} ms; measured / floor = "
          f"{med[2] / floor_ms:.2f}")


def quality(r):
    W, H, DEPTH, STEP = 256, 144, 8, 1.0
    sky = texture_io.load_cptex()
    for name in ("s4", "s1000"):
        base = scenes.camera_for(W, H)
        c0, c1 = camera_get_copy(base), camera_get_copy(moved(base, STEP))
        r.set_scene(scenes.SCENES[name]())
        r.set_env(sky)
        r.set_frame(W, H)
        r.init_rng(scenes.DEFAULT_SEED + 1)
        r.render(c1, 4096, DEPTH, sync=True, ordered=True)
        truth = r.read_accum()
        truth = truth[:, :3].astype(np.float64) / truth[:, 3:4]
        r.init_rng(scenes.DEFAULT_SEED)
        r.render(c0, 32, DEPTH, sync=True, ordered=True)
        hist, states = r.read_accum(), r.read_rng()
        r.gbuffer(c1, ORD)
        floor = r.read_gbuffer()["id"] == 0

        def err(a):
            e = ((a[:, :3] / np.maximum(a[:, 3:4], 1)).astype(np.float64) - truth) ** 2
            return e.mean(), e[floor].mean()
        for k in (1, 4, 16):
            r.write_rng(states)
            r.clear_accum()
            r.render(c1, k, DEPTH, accumulate=True, sync=True, ordered=True)
            rst = err(r.read_accum())
            print(f"quality {name} {W}x{H} step {STEP} k={k}: restart MSE {rst[0]:.6g} (floor {rst[1]:.6g})")
            for mh in (8, 32, 128):
                for tol in (1e-3, 1e-2, 1e-1):
                    r.write_rng(states)
                    r.write_accum(hist)
                    r.reproject_accum(c0, c1, mh, tol, ORD)
                    reused = (r.read_accum()[:, 3] > 0).mean()
                    r.render(c1, k, DEPTH, accumulate=True, sync=True, ordered=True)
                    rep = err(r.read_accum())
                    print(f"  max_history {mh:3d} plane_tol {tol:g}: reused {reused:.3f}, MSE {rep[0]:.6g} (x{rep[0] / rst[0]:.3f}), "
                          f"floor {rep[1]:.6g} (x{rep[1] / rst[1]:.3f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process)
    with Renderer(0) as r:
        if a.timing or not a.quality:
            timing(r)
        if a.quality or not a.timing:
            quality(r)
