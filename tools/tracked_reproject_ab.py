#!/usr/bin/env python3
"""Measurements behind the tracked reprojection.

    python tools/tracked_reproject_ab.py --timing [--parent build/ab/libcpt_parent.so] [--rounds 3]
    python tools/tracked_reproject_ab.py --rehearsal

--timing     S1000 at 1920x1080 (the C4 frame), modelled on tools/reproject_ab.py --timing: medians of
             5 calls after a warm-up of cpt_last_reproject_launch_ms for cpt_reproject_accum_tracked
             without an edit, after an edit of 50 objects (with the motion table's upload), and for
             cpt_reproject_accum, each in a fresh child process (one library per process), the
             children run by turns for --rounds rounds.  With --parent the untracked call is the
             parent commit's build (CPT_LIB_PATH), interleaved with this build's in the same session.
             Then the tracked look-up kernel's algorithmic bytes over the HBM read rate
             cpt_measure_read_bandwidth gave in the same child.
--rehearsal  no GPU: tests/test_gpu_tracked_reproject.py's end-to-end sequence with the oracle's
             renders and the host entries on tests/gbuffer_model.py's G-buffers; prints the MSE per
             region for the three arms, in the device fixture's format.
"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H = 1920, 1080


def _moved(cam, step):
    c = cam.copy()
    for k in ("origin", "look_at"):
        c[k] = np.asarray(cam[k], np.float32) + np.array([step, 0.0, -step], np.float32)
    return c


def one(which):
    """A child: six calls of one kind, the medians of the last five on one line."""
    import torch  # noqa: F401  (one HIP runtime per process)
    from cpppathtracer_amd import Renderer, camera_get_copy, scenes, texture_io
    from cpppathtracer_amd._lib import CPT_TRAVERSAL_ORDERED as ORD
    base = scenes.camera_for(W, H)
    cams = [camera_get_copy(base), camera_get_copy(_moved(base, 1.0))]
    objs = scenes.scene_s1000()
    with Renderer(0) as r:
        r.set_scene(objs)
        r.set_env(texture_io.load_cptex())
        r.set_frame(W, H)
        r.init_rng(scenes.DEFAULT_SEED)
        r.render(cams[0], 4, 8, sync=True, ordered=True)
        hist = r.read_accum()
        idx = np.arange(1, 501, 10)
        shifted = np.array(objs[idx], copy=True)
        shifted["center"][:, 0] += np.float32(0.75)
        if which != "untracked":
            r.history_capture(cams[0], ORD)
        runs = []
        for i in range(6):
            r.write_accum(hist)
            if which == "untracked":
                r.reproject_accum(cams[0], cams[1], flags=ORD)
            else:
                if which == "edited":   # there and back: every call follows an edit of 50 objects
                    r.update_objects(idx, shifted if i % 2 == 0 else objs[idx])
                r.reproject_accum_tracked(cams[(i + 1) % 2], flags=ORD)   # from the camera the last call left
            runs.append(r.last_reproject_ms(split=True) + (r.last_reproject_ms(),))
        med = [statistics.median(x[k] for x in runs[1:]) for k in range(4)]
        gbps = r.measure_read_bandwidth()
    print("RESULT %s %.5f %.5f %.5f %.5f %.1f" % (which, *med, gbps))


def timing(parent, rounds):
    arms = [("tracked", None), ("edited", None), ("untracked", None)]
    if parent:
        arms.append(("untracked", os.path.abspath(parent)))
    got = {a: [] for a in arms}
    for rnd in range(rounds):
        for arm in arms:
            env = dict(os.environ)
            if arm[1]:
                env["CPT_LIB_PATH"] = arm[1]
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", arm[0]], env=env, capture_output=True,
                                 text=True, timeout=240)
            line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not line:
                sys.exit("child %s failed (%d): %s" % (arm, out.returncode, (out.stdout + out.stderr)[-600:]))
            v = [float(x) for x in line[0].split()[2:]]
            got[arm].append(v)
            print("round %d %-9s %-6s: trace(from) %.4f ms, trace(to) %.4f ms, look-up %.4f ms, call %.4f ms; read rate %.0f GB/s"
                  % (rnd + 1, arm[0], "parent" if arm[1] else "this", *v), flush=True)
    print("# medians over %d rounds (each a median of 5 calls after a warm-up), S1000 %dx%d" % (rounds, W, H))
    med = {}
    for arm in arms:
        med[arm] = [statistics.median(v[k] for v in got[arm]) for k in range(5)]
        print("%-9s %-6s: trace(from) %.4f ms, trace(to) %.4f ms, look-up %.4f ms, call %.4f ms"
              % (arm[0], "parent" if arm[1] else "this", *med[arm][:4]))
    npix = W * H
    gbps = med[arms[0]][4]
    # per pixel: id1, t1 (8 B), normal1 (12 B), the old frame's accumulator, id and t once each
    # (16 + 8 B), the output (16 B), the new history's id and t (8 B); the motion record is 40 B per
    # lane before sharing, next to nothing once a wave shares it
    for name, per in (("records shared", 68), ("40 B per lane", 108)):
        floor = npix * per / (gbps * 1e9) * 1e3
        print("tracked look-up, %s: %.1f MB over %.0f GB/s = %.4f ms; no edit / floor = %.2f, edited / floor = %.2f"
              % (name, npix * per / 1e6, gbps, floor, med[arms[0]][2] / floor, med[arms[1]][2] / floor))
    ref = med[arms[-1]]
    print("tracked call / %s cpt_reproject_accum call: no edit %.3f, edited %.3f; look-up / k_reproject_accum: %.3f, %.3f"
          % ("the parent's" if parent else "this build's", med[arms[0]][3] / ref[3], med[arms[1]][3] / ref[3],
             med[arms[0]][2] / ref[2], med[arms[1]][2] / ref[2]))


def rehearsal():
    """The end-to-end fixture of tests/test_gpu_tracked_reproject.py on the CPU, each device step
    replaced by its CPU counterpart: the oracle's renders (the scene built from the edited objects,
    the 32 old passes through an UpdateObject back, as the fixture does), gbuffer_model's G-buffers,
    the host entries.  Prints the fixture's three lines."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import gbuffer_model as gm
    import oracle
    import tracked_reproject_model as tm
    from cpppathtracer_amd import scenes, texture_io
    from cpppathtracer_amd.renderer import object_motion_host, reproject_host, reproject_tracked_host
    from cpppathtracer_amd.types import make_camera
    Wr, Hr, DEPTH, MOVE, T = 64, 48, 8, (4.0, 0.0, 6.0), 16
    oracle.build()
    oracle.set_walk(True)
    cam = oracle.camera_get_copy(make_camera(Wr, Hr, origin=scenes.CAMERA_ORIGIN, look_at=scenes.CAMERA_LOOK_AT))
    sky = texture_io.load_cptex()
    rows = np.arange(Hr, dtype=np.int32)
    old = tm.scene()
    c = np.asarray(old[tm.METAL]["center"], np.float32)
    new = tm._edit(old, tm.METAL, center=tuple(c + np.asarray(MOVE, np.float32)))
    rng = oracle.init_rng(scenes.DEFAULT_SEED + 1, Wr, rows, T)
    truth = oracle.render(new, cam, sky, rows, 1024, DEPTH, rng, threads=T)[0]
    truth = truth[:, :3].astype(np.float64) / truth[:, 3:4]
    rng = oracle.init_rng(scenes.DEFAULT_SEED, Wr, rows, T)
    a32 = oracle.render_edited(new, [(tm.METAL, old[tm.METAL])], cam, sky, rows, 32, DEPTH, rng, threads=T)[0]
    states = rng.copy()
    O, d = gm.camera_rays(cam)
    order = gm.reference_order(oracle, new)
    id0, t0, _, _ = gm.first_hit(oracle, old, O, d, order=order)
    id1, t1, n1, _ = gm.first_hit(oracle, new, O, d, order=order)
    more = lambda acc, r: oracle.render(new, cam, sky, rows, 4, DEPTH, r, accum=acc, accumulate=acc is not None, threads=T)[0]
    arms = {
        "tracked": more(reproject_tracked_host(cam, cam, d, d, id0, t0, id1, t1, n1, a32, object_motion_host(old, new)), states.copy()),
        "restart": more(None, states.copy()),
        # today's only alternative to clearing: both traces in the edited scene
        "stale": more(reproject_host(cam, cam, d, d, id1, t1, id1, t1, n1, a32), states.copy()),
    }
    errs = {k: (((v[:, :3] / v[:, 3:4]).astype(np.float64) - truth) ** 2).mean(axis=1) for k, v in arms.items()}
    union = (id0 == tm.METAL) | (id1 == tm.METAL)
    near = union.reshape(Hr, Wr).copy()
    for _ in range(2):
        g = near.copy()
        g[1:] |= near[:-1]
        g[:-1] |= near[1:]
        g[:, 1:] |= near[:, :-1]
        g[:, :-1] |= near[:, 1:]
        near = g
    far_floor = (id0 == tm.FLOOR) & (id1 == tm.FLOOR) & ~near.reshape(-1)
    for name, m in (("frame", np.ones(Wr * Hr, bool)), ("union of the sphere's footprints", union), ("floor away from them", far_floor)):
        print("%s: %d pixels, MSE tracked %.6g, restart %.6g, stale %.6g" %
              (name, m.sum(), *(errs[k][m].mean() for k in ("tracked", "restart", "stale"))))
    same = arms["tracked"][far_floor].tobytes() == arms["stale"][far_floor].tobytes()
    print("floor away from them: tracked and stale are %s" % ("the same bits" if same else "NOT the same bits"))
    ok = errs["tracked"].mean() < errs["restart"].mean() and errs["tracked"][union].mean() < errs["stale"][union].mean() and same
    print("the three assertions of test_tracked_history_beats_restart_and_stale: %s" % ("hold" if ok else "FAIL"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--rehearsal", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--one", default=None, choices=["tracked", "edited", "untracked"])
    a = ap.parse_args()
    if a.one:
        one(a.one)
    elif a.rehearsal:
        rehearsal()
    else:
        timing(a.parent, a.rounds)
