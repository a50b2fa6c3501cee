#!/usr/bin/env python3
"""Top-up render (cpt_render_to_count) against the uniform accumulating render it
replaces after a reprojection.

    tools/topup_ab.py --rehearsal [--steps 4,8,12] [--truth 1024]     CPU only
    tools/topup_ab.py --timing [--rounds 3] [--calls 5]               one GPU

--rehearsal runs tests/test_gpu_topup.py's end-to-end comparison without a GPU: the oracle's
renders, tests/gbuffer_model.py's G-buffers, cpt_reproject_host, and tests/topup_model.py for the
top-up arm.  S4 + cylinder, 64 x 48, depth 8, 32 passes, a sideways camera step; per step the share
of the frame left at count 0 and reused at 32, both arms' budgets, and their MSE to the truth over
the count-0 pixels and over the frame.  Every step is bit-exact on the device, so the device's
figures (the test prints them) should agree to every printed digit.

--timing: S1000 at 1920 x 1080, depth 8, 32 passes, one orbit step (one degree), reprojected with
max_history 32; then from that state, restored before every call, (a) render_to_count(32): the plan's
launches and the top-up launch, and (b) render(ceil(B / npix), accumulate) with B the top-up's
passes.  Every arm is a fresh process, the arms run by turns, each figure is the median over the
rounds of a median of --calls calls after a warm-up call.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

DEPTH, PASSES, SEED = 8, 32, 1234


def _cameras(W, H, step):
    from cpppathtracer_amd import camera_get_copy
    from cpppathtracer_amd.scenes import CAMERA_LOOK_AT as AT, CAMERA_ORIGIN as O
    from cpppathtracer_amd.types import make_camera
    move = lambda p: tuple(a + b for a, b in zip(p, (step, 0.0, -step)))
    return (camera_get_copy(make_camera(W, H, origin=O, look_at=AT)),
            camera_get_copy(make_camera(W, H, origin=move(O), look_at=move(AT))))


def rehearsal(steps, truth_spp):
    import gbuffer_model as gm
    import oracle
    import topup_model as tu
    import tracked_reproject_model as tm
    from cpppathtracer_amd import texture_io
    from cpppathtracer_amd.renderer import reproject_host
    W, H = 64, 48
    rows = np.arange(H, dtype=np.int32)
    objs, sky = tm.scene(), texture_io.load_cptex()
    for step in steps:
        c0, c1 = _cameras(W, H, step)
        rng = oracle.init_rng(SEED + 1, W, rows, threads=8)
        t, _, _, _ = oracle.render(objs, c1, sky, rows, truth_spp, DEPTH, rng, threads=8)
        truth = t[:, :3].astype(np.float64) / t[:, 3:4]
        rng = oracle.init_rng(SEED, W, rows, threads=8)
        acc, _, _, _ = oracle.render(objs, c0, sky, rows, PASSES, DEPTH, rng, threads=8)
        (_, d0), (_, d1) = gm.camera_rays(c0), gm.camera_rays(c1)
        i0, t0, _, _ = gm.gbuffer(oracle, objs, c0)
        i1, t1, n1, _ = gm.gbuffer(oracle, objs, c1)
        hist = reproject_host(c0, c1, d0, d1, i0, t0, i1, t1, n1, acc)
        topped, _, _, _, plan = tu.expected(oracle, objs, c1, sky, rows, DEPTH, PASSES, rng, hist)
        spp = -(-plan["passes"] // (W * H))
        uniform, _, _, _ = oracle.render(objs, c1, sky, rows, spp, DEPTH, rng.copy(), accum=hist.copy(), accumulate=True, threads=8)
        err = lambda a: ((a[:, :3] / a[:, 3:4]).astype(np.float64) - truth) ** 2
        a, b = err(topped).mean(axis=1), err(uniform).mean(axis=1)
        empty, reused = hist[:, 3] == 0, hist[:, 3] == PASSES
        print(f"step {step:g}: top-up: {plan['passes']} passes; uniform: {spp} per pixel = {spp * W * H} passes; "
              f"{empty.mean():.4f} of the frame at count 0, {reused.mean():.4f} reused at {PASSES}")
        print(f"step {step:g}: count-0 pixels: top-up MSE {a[empty].mean():.6g}, uniform MSE {b[empty].mean():.6g}")
        print(f"step {step:g}: frame: top-up MSE {a.mean():.6g}, uniform MSE {b.mean():.6g}", flush=True)


def arm(name, calls):
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    from cpppathtracer_amd import Renderer, camera_get_copy, scenes, texture_io
    from cpppathtracer_amd._lib import CPT_TRAVERSAL_ORDERED
    from cpppathtracer_amd.types import make_camera
    W, H = 1920, 1080
    O, AT = scenes.CAMERA_ORIGIN, scenes.CAMERA_LOOK_AT
    c, s = np.float32(0.99984770), np.float32(0.01745241)
    dx, dz = np.float32(O[0] - AT[0]), np.float32(O[2] - AT[2])
    c0 = camera_get_copy(make_camera(W, H, origin=O, look_at=AT))
    c1 = camera_get_copy(make_camera(W, H, origin=(AT[0] + c * dx + s * dz, O[1], AT[2] + c * dz - s * dx), look_at=AT))
    with Renderer(0) as r:
        r.set_scene(scenes.scene_s1000())
        r.set_env(texture_io.load_cptex())
        r.set_frame(W, H)
        r.init_rng(SEED)
        r.render(c0, PASSES, DEPTH, sync=True, ordered=True, schedule="cost")
        r.reproject_accum(c0, c1, max_history=PASSES, flags=CPT_TRAVERSAL_ORDERED)
        acc, rng = r.read_accum(), r.read_rng()
        r.render_to_count(c1, PASSES, DEPTH, sync=True, flags=CPT_TRAVERSAL_ORDERED)
        info = r.topup_info()
        spp = -(-info["passes"] // (W * H))
        total, kernel = [], []
        for k in range(calls + 1):
            r.write_accum(acc)
            r.write_rng(rng)
            r.synchronize()
            if name == "topup":
                r.render_to_count(c1, PASSES, DEPTH, sync=True, flags=CPT_TRAVERSAL_ORDERED)
            else:
                r.render(c1, spp, DEPTH, accumulate=True, sync=True, ordered=True)
            if k:   # the first call is the warm-up
                total.append(r.last_render_ms())
                kernel.append(r.last_kernel_stats()[0])
    print(json.dumps(dict(arm=name, call_ms=statistics.median(total), launch_ms=statistics.median(kernel), uniform_spp=spp,
                          share_at_0=float((acc[:, 3] == 0).mean()), share_at_32=float((acc[:, 3] == PASSES).mean()), **info)))


def timing(rounds, calls):
    out = {"topup": [], "uniform": []}
    for k in range(rounds):
        for name in out:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", name, "--calls", str(calls)], capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"{name}: rc {p.returncode}\n{p.stdout}{p.stderr}")
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            print(k + 1, json.dumps(rec), flush=True)
            out[name].append(rec)
    med = lambda name, key: statistics.median(r[key] for r in out[name])
    t, u = out["topup"][0], out["uniform"][0]
    print(f"# frame: {t['share_at_0']:.4f} at count 0, {t['share_at_32']:.4f} at 32; top-up: {t['tiles']} tiles, {t['pixels']} pixels, "
          f"{t['passes']} passes; uniform: {u['uniform_spp']} per pixel = {u['uniform_spp'] * 1920 * 1080} passes")
    print(f"# render_to_count(32): call {med('topup', 'call_ms'):.4f} ms, of which the top-up launch {med('topup', 'launch_ms'):.4f} ms "
          f"and the plan {med('topup', 'call_ms') - med('topup', 'launch_ms'):.4f} ms")
    print(f"# render({u['uniform_spp']}, accumulate): call {med('uniform', 'call_ms'):.4f} ms")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rehearsal", action="store_true")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--arm", choices=["topup", "uniform"])
    ap.add_argument("--steps", default="4,8,12")
    ap.add_argument("--truth", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    if a.arm:
        arm(a.arm, a.calls)
    elif a.timing:
        timing(a.rounds, a.calls)
    elif a.rehearsal:
        rehearsal([float(v) for v in a.steps.split(",")], a.truth)
    else:
        ap.error("--rehearsal or --timing")
