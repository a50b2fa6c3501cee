#!/usr/bin/env python3
"""The filter for frames without moments (cpt_filter_frame_spatial): the sweep behind
its defaults, and its device time.

    tools/filter_spatial_ab.py --rehearsal [--truth 1024]             CPU only
    tools/filter_spatial_ab.py --timing [--rounds 5]                  one GPU

--rehearsal runs tests/test_gpu_filter_spatial.py's end-to-end case without a GPU: the oracle's
renders, tests/gbuffer_model.py's G-buffers, cpt_reproject_host, tests/topup_model.py for the top-up,
then the two host hooks.  Case 1 is §24's: S4 + cylinder, 64 x 48, depth 8, 32 passes at C0,
reprojected to C1 (camera and look-at moved 8 units sideways), topped up to 32.  Case 2 is the same
sequence with S1000 at 96 x 64.  The truth is --truth passes at C1.  Per case the sweep levels {3, 5}
x sigma_l {1, 2, 4} x sharpness {3, 7}: the frame's MSE unfiltered and filtered; then, for case 1 at
the chosen point (lowest frame MSE on case 1 among those that improve case 2), the table frame /
floor / each object.  Every step is bit-exact on the device, so the device's figures (the test
prints them) should agree to every printed digit.

--timing: S1000 at 1920 x 1080, depth 8: an adaptive render (8..32 passes) for cpt_filter_frame, and
on the same frame cpt_gbuffer and cpt_filter_frame_spatial at its defaults and at levels 0.  Every
arm is a fresh process, the arms run by turns, each figure is the median over --rounds of a median
of 5 calls after a warm-up call; the read bandwidth is cpt_measure_read_bandwidth's in that run.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

DEPTH, PASSES, SEED, STEP = 8, 32, 1234, 8.0
SWEEP = [(l, s, k) for l in (3, 5) for s in (1.0, 2.0, 4.0) for k in (3, 7)]


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_filter(accum, ids, normal, W, H, levels, sigma_l, sharpness):
    """prepare + levels through the two host hooks: rgb [npix, 3]."""
    from cpppathtracer_amd import _lib
    L = _lib.load()
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    plane = np.zeros((W * H, 4), dtype=np.float32)
    valid = np.zeros(W * H, dtype=np.uint8)
    assert L.cpt_filter_prepare_spatial_host(W, H, _ptr(accum), _ptr(ids), _ptr(normal), sharpness, _ptr(plane), _ptr(valid)) == 0
    for l in range(levels):
        out = np.zeros_like(plane)
        assert L.cpt_filter_level_id_host(W, H, 1 << l, _ptr(plane), _ptr(normal), _ptr(ids), _ptr(valid),
                                          ctypes.c_float(sigma_l), sharpness, _ptr(out)) == 0
        plane = out
    return plane[:, :3].copy()


def case_state(objs, W, H, truth_spp):
    """(topped-up accumulator at C1, id and normal planes at C1, the truth's mean image)."""
    import gbuffer_model as gm
    import oracle
    import topup_model as tu
    from cpppathtracer_amd import texture_io
    from cpppathtracer_amd.renderer import reproject_host
    from topup_ab import _cameras
    rows = np.arange(H, dtype=np.int32)
    sky = texture_io.load_cptex()
    c0, c1 = _cameras(W, H, STEP)
    rng = oracle.init_rng(SEED + 1, W, rows, threads=8)
    t, _, _, _ = oracle.render(objs, c1, sky, rows, truth_spp, DEPTH, rng, threads=8)
    truth = t[:, :3].astype(np.float64) / t[:, 3:4]
    rng = oracle.init_rng(SEED, W, rows, threads=8)
    acc, _, _, _ = oracle.render(objs, c0, sky, rows, PASSES, DEPTH, rng, threads=8)
    (_, d0), (_, d1) = gm.camera_rays(c0), gm.camera_rays(c1)
    i0, t0, _, _ = gm.gbuffer(oracle, objs, c0)
    i1, t1, n1, _ = gm.gbuffer(oracle, objs, c1)
    hist = reproject_host(c0, c1, d0, d1, i0, t0, i1, t1, n1, acc)
    topped, _, _, _, _ = tu.expected(oracle, objs, c1, sky, rows, DEPTH, PASSES, rng, hist)
    return topped, i1, n1, truth


def mse(rgb, truth, mask=None):
    e = ((rgb.astype(np.float64) - truth) ** 2).mean(axis=1)
    return float(e.mean() if mask is None else e[mask].mean())


def rehearsal(truth_spp):
    import tracked_reproject_model as tm
    from cpppathtracer_amd import scenes
    cases = [("S4 + cylinder 64x48", tm.scene(), 64, 48), ("S1000 96x64", scenes.scene_s1000(), 96, 64)]
    results = []
    for name, objs, W, H in cases:
        topped, ids, nrm, truth = case_state(objs, W, H, truth_spp)
        with np.errstate(all="ignore"):
            noisy = np.where(topped[:, 3:4] > 0, topped[:, :3] / topped[:, 3:4], 0.0).astype(np.float32)
        base = mse(noisy, truth)
        print(f"{name}: unfiltered frame MSE {base:.6g}", flush=True)
        res = {}
        for levels, sigma_l, sharp in SWEEP:
            rgb = host_filter(topped, ids, nrm, W, H, levels, sigma_l, sharp)
            res[(levels, sigma_l, sharp)] = mse(rgb, truth)
            print(f"{name}: levels {levels} sigma_l {sigma_l:g} sharpness {sharp}: filtered frame MSE {res[(levels, sigma_l, sharp)]:.6g}"
                  f" ({res[(levels, sigma_l, sharp)] / base:.3f} of unfiltered)", flush=True)
        results.append((name, W, H, topped, ids, nrm, truth, noisy, base, res))
    first, second = results
    ok = [k for k in SWEEP if second[9][k] < second[8]]
    best = min(ok, key=lambda k: first[9][k]) if ok else None
    print(f"# points that improve case 2: {len(ok)} of {len(SWEEP)}; chosen (lowest case-1 MSE among them): {best}")
    if best is None:
        return
    name, W, H, topped, ids, nrm, truth, noisy, base, _ = first
    rgb = host_filter(topped, ids, nrm, W, H, *best)
    print(f"# {name} at levels {best[0]} sigma_l {best[1]:g} sharpness {best[2]}: MSE unfiltered, filtered")
    print(f"frame: {mse(noisy, truth):.6g} {mse(rgb, truth):.6g}")
    for obj in sorted(set(ids.tolist())):
        m = ids == obj
        label = "miss (sky)" if obj < 0 else f"object {obj}"
        print(f"{label} ({int(m.sum())} pixels): {mse(noisy, truth, m):.6g} {mse(rgb, truth, m):.6g}", flush=True)


def arm(name):
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    from cpppathtracer_amd import Renderer, camera_get_copy, scenes, texture_io
    from cpppathtracer_amd._lib import CPT_RENDER_AUX, CPT_TRAVERSAL_ORDERED
    W, H = 1920, 1080
    cam = camera_get_copy(scenes.camera_for(W, H))
    with Renderer(0) as r:
        r.set_scene(scenes.scene_s1000())
        r.set_env(texture_io.load_cptex())
        r.set_frame(W, H)
        r.init_rng(SEED)
        r.render_adaptive(cam, 8, 32, 4, 0.05, DEPTH, flags=CPT_RENDER_AUX | CPT_TRAVERSAL_ORDERED)
        r.gbuffer(cam, flags=CPT_TRAVERSAL_ORDERED)
        r.synchronize()
        call = {"moments5": lambda: r.filter_frame(), "moments0": lambda: r.filter_frame(levels=0),
                "spatial": lambda: r.filter_frame_spatial(), "spatial0": lambda: r.filter_frame_spatial(levels=0)}[name]
        ms = []
        for k in range(6):
            call()
            if k:   # the first call is the warm-up
                ms.append(r.last_filter_ms())
        bw = float(r.measure_read_bandwidth()) if name == "spatial0" else None
    print(json.dumps(dict(arm=name, ms=statistics.median(ms), read_gbs=bw)))


def timing(rounds):
    names = ["spatial", "spatial0", "moments5", "moments0"]
    out = {n: [] for n in names}
    for k in range(rounds):
        for n in names:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", n], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"{n}: rc {p.returncode}\n{p.stdout}{p.stderr}")
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            print(k + 1, json.dumps(rec), flush=True)
            out[n].append(rec)
    med = lambda n, key="ms": statistics.median(r[key] for r in out[n])
    npix = 1920 * 1080
    print(f"# cpt_filter_frame_spatial at its defaults: {med('spatial'):.4f} ms; levels 0 (k_filter_prepare_spatial alone): "
          f"{med('spatial0'):.4f} ms")
    print(f"# cpt_filter_frame, 5 levels: {med('moments5'):.4f} ms; levels 0 (k_filter_prepare alone): {med('moments0'):.4f} ms")
    rate = 49 * npix / (med("spatial0") * 1e-3) / 1e9
    bws = [r["read_gbs"] for r in out["spatial0"] if r["read_gbs"]]
    print(f"# k_filter_prepare_spatial: 49 algorithmic bytes per pixel = {rate:.1f} GB/s"
          + (f", {100 * rate / statistics.median(bws):.1f}% of the measured read bandwidth {statistics.median(bws):.0f} GB/s" if bws else ""))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rehearsal", action="store_true")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--arm", choices=["spatial", "spatial0", "moments5", "moments0"])
    ap.add_argument("--truth", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.arm:
        arm(a.arm)
    elif a.timing:
        timing(a.rounds)
    elif a.rehearsal:
        rehearsal(a.truth)
    else:
        ap.error("one of --rehearsal, --timing")
