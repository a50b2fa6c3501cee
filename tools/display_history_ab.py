#!/usr/bin/env python3
"""Measurements behind the display's per-pixel history.

    python tools/display_history_ab.py > profiles/r14/display_history_ab.log
    python tools/display_history_ab.py --rehearsal > profiles/r14/display_history_rehearsal.log   (no GPU)

S1000 at 1920x1080 (the C4 frame), one session:
  display  cpt_last_display_ms of denoise_mix_history against denoise_mix (the kernel's two
           instantiations; the second is the parent's code object), device frame only, interleaved,
           medians of 5 after a warm-up, with each one's spread.
  look-up  cpt_last_reproject_ms of reproject_display split into its three launches, medians of 5
           after a warm-up, and the look-up kernel's algorithmic bytes over the measured HBM read
           rate (cpt_measure_read_bandwidth).

--rehearsal is the end-to-end case of tests/test_gpu_display_history.py on the CPU alone, an
independent check of its ratio: S4, 64x48, depth 8, the reference's default lens; every pass is the
oracle's render and the oracle's Denoising + Mix (at each pixel's own count + 1: the stencil reads
the pass, not the mean, so mixing the frame once per distinct count and keeping each pixel's own
is exact), the move is cpt_reproject_display_host on tests/gbuffer_model.py's G-buffers.  32 passes
at C0, the state reprojected to C1 = C0 + (4, 0, -4), 4 passes, against a restart of 4 passes from the
same RNG states; truth: the mean of 1024 display passes at C1.
"""
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


def main(r):
    W, H = 1920, 1080
    base = scenes.camera_for(W, H)
    c0, c1 = camera_get_copy(base), camera_get_copy(moved(base, 1.0))
    r.set_scene(scenes.scene_s1000())
    r.set_env(texture_io.load_cptex())
    r.set_frame(W, H)
    r.init_rng(scenes.DEFAULT_SEED)
    r.render(c0, 1, 8, aux=True, sync=True, ordered=True)
    hist, glob = [], []
    for i in range(6):
        r.denoise_mix(i + 1, host=False)
        glob.append(r.last_display_ms())
        r.denoise_mix_history(host=False)
        hist.append(r.last_display_ms())
    g, h = statistics.median(glob[1:]), statistics.median(hist[1:])
    print(f"display S1000 {W}x{H}, device frame: denoise_mix {g:.4f} ms ({min(glob[1:]):.4f}-{max(glob[1:]):.4f}), "
          f"denoise_mix_history {h:.4f} ms ({min(hist[1:]):.4f}-{max(hist[1:]):.4f}), ratio {h / g:.3f} "
          f"(bytes per pixel 68 / 60 = {68 / 60:.3f})")
    runs = []
    for i in range(6):
        r.reproject_display(c0, c1, flags=ORD) if i % 2 == 0 else r.reproject_display(c1, c0, flags=ORD)
        runs.append(r.last_reproject_ms(split=True))
    med = [statistics.median(x[k] for x in runs[1:]) for k in range(3)]
    gbps = r.measure_read_bandwidth()
    # per pixel: id1, t1 (8 B), normal1 (12 B), the old frame's mean, count, id and t once each
    # (12 + 4 + 8 B: neighbouring lanes share their taps), the output (12 + 4 B)
    algo = W * H * (8 + 12 + 12 + 4 + 8 + 16)
    floor_ms = algo / (gbps * 1e9) * 1e3
    print(f"look-up S1000 {W}x{H}: trace(from) {med[0]:.4f} ms, trace(to) {med[1]:.4f} ms, k_reproject_display {med[2]:.4f} ms, "
          f"total {sum(med):.4f} ms")
    print(f"  look-up kernel: {algo / 1e6:.1f} MB algorithmic over {gbps:.0f} GB/s = {floor_ms:.4f} ms; measured / floor = "
          f"{med[2] / floor_ms:.2f}")


def rehearsal():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import gbuffer_model as gm
    import oracle
    from cpppathtracer_amd.renderer import reproject_display_host
    from cpppathtracer_amd.scenes import CAMERA_LOOK_AT as AT, CAMERA_ORIGIN as O
    from cpppathtracer_amd.types import make_camera
    W, H, DEPTH, STEP = 64, 48, 8, (4.0, 0.0, -4.0)
    step = lambda p: tuple(a + b for a, b in zip(p, STEP))
    c0 = oracle.camera_get_copy(make_camera(W, H, origin=O, look_at=AT))
    c1 = oracle.camera_get_copy(make_camera(W, H, origin=step(O), look_at=step(AT)))
    objs, sky, rows = scenes.scene_s4(), texture_io.load_cptex(), np.arange(H, dtype=np.int32)
    threads = min(16, os.cpu_count() or 1)
    st = {}

    def reset(seed=None, rng=None):
        st["rng"] = oracle.init_rng(seed, W, rows) if rng is None else rng.copy()
        st["mix"], st["cnt"] = np.zeros((W * H, 3), np.float32), np.zeros(W * H, np.float32)

    def passes(cam, n):
        out = np.zeros((H, W, 4), np.uint8)
        for _ in range(n):
            acc, _, normal, depth = oracle.render(objs, cam, sky, rows, 1, DEPTH, st["rng"], want_aux=True, threads=threads)
            new = st["mix"].copy()
            for k in np.unique(st["cnt"]):
                m = st["mix"].copy()
                oracle.denoise_mix(acc, normal, depth, m, out, W, H, int(k) + 1)
                new[st["cnt"] == k] = m[st["cnt"] == k]
            st["mix"], st["cnt"] = new, st["cnt"] + 1   # 64x48: the launch region is the frame

    reset(scenes.DEFAULT_SEED + 1)
    passes(c1, 1024)
    truth = st["mix"].astype(np.float64)
    reset(scenes.DEFAULT_SEED)
    passes(c0, 32)
    states = st["rng"].copy()
    (_, d0), (_, d1) = gm.camera_rays(c0), gm.camera_rays(c1)
    id0, t0, _, _ = gm.gbuffer(oracle, objs, c0)
    ids, t1, n1, _ = gm.gbuffer(oracle, objs, c1)
    st["mix"], st["cnt"] = reproject_display_host(c0, c1, d0, d1, id0, t0, ids, t1, n1, st["mix"], st["cnt"])
    reused = st["cnt"] > 0
    passes(c1, 4)
    reprojected = st["mix"]
    assert (st["cnt"][reused] == 36).all() and (st["cnt"][~reused] == 4).all()
    reset(rng=states)
    passes(c1, 4)
    a = ((reprojected.astype(np.float64) - truth) ** 2).mean(axis=1)
    b = ((st["mix"].astype(np.float64) - truth) ** 2).mean(axis=1)
    print(f"CPU rehearsal S4 {W}x{H}, depth {DEPTH}: the oracle's render and Denoising + Mix, cpt_reproject_display_host")
    for k in range(4):
        m = ids == k
        print(f"object {k}: {int(m.sum())} pixels, reprojected MSE {a[m].mean():.6g}, restart MSE {b[m].mean():.6g}")
    print(f"frame: reprojected MSE {a.mean():.6g}, restart MSE {b.mean():.6g}, ratio {a.mean() / b.mean():.4f}; "
          f"floor ratio {a[ids == 0].mean() / b[ids == 0].mean():.4f}; {reused.mean():.3f} of the frame reused")


if __name__ == "__main__":
    if "--rehearsal" in sys.argv[1:]:
        rehearsal()
        sys.exit(0)
    import torch  # noqa: F401  (one HIP runtime per process)
    with Renderer(0) as r:
        main(r)
