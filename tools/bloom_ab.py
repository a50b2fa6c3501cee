"""The measurements of DESIGN.md §28 on one GPU at 1920x1080, printed as one JSON line:

  bloom_ms        cpt_last_bloom_ms at 1 level (k_bloom_first alone), 6 and 8 levels
  first_gbps      the 33 MB k_bloom_first reads over its time, beside the same session's
                  cpt_measure_read_bandwidth
  present_*_ms    cpt_last_present_ms of cpt_present_bloom and of cpt_present
  filter_ms       cpt_last_filter_ms of cpt_filter_frame_spatial on the same frame
  host_ms         the one-core host hook cpt_bloom_host (6 levels), wall time, with --host

Medians over --repeat calls (20) after two warm-up calls; the spreads are the calls' min and max.
The library is the tree's, or CPT_LIB_PATH's (two builds run by turns in one session make an A/B).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

F = np.float32


def spans(call, read_ms, repeat):
    for _ in range(2):
        call()
    ms = []
    for _ in range(repeat):
        call()
        ms.append(read_ms())
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--bandwidth", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    import tracked_reproject_model as tm
    from cpppathtracer_amd import Renderer, bloom, present
    W, H = a.width, a.height
    rs = np.random.RandomState(28)
    n = rs.randint(1, 65, W * H).astype(F)
    accum = np.concatenate([np.exp2(rs.uniform(-8, 6, (W * H, 3))).astype(F) * n[:, None], n[:, None]], axis=1).astype(F)
    out = dict(width=W, height=H, repeat=a.repeat, lib=os.environ.get("CPT_LIB_PATH", "tree"))
    with Renderer(0) as r:
        r.set_scene(tm.scene())
        r.set_frame(W, H)
        r.write_accum(accum)
        present.meter_exposure(r)
        out["bloom_ms"] = {L: spans(lambda: bloom.build(r, "accum", 1.0, L), lambda: bloom.last_bloom_ms(r), a.repeat) for L in (1, 6, 8)}
        out["first_gbps"] = W * H * 16 / (out["bloom_ms"][1]["median"] * 1e-3) / 1e9
        bloom.build(r, "accum", 1.0, 6)
        out["present_bloom_ms"] = spans(lambda: bloom.present_bloom(r, "accum", "aces", 4.0, "srgb", 0.25, host=False),
                                        lambda: present.last_present_ms(r), a.repeat)
        out["present_ms"] = spans(lambda: present.present(r, "accum", "aces", 4.0, "srgb", host=False), lambda: present.last_present_ms(r),
                                  a.repeat)
        r.write_gbuffer(id=np.zeros(W * H, dtype=np.int32), normal=np.tile(np.array([0, 1, 0], dtype=F), (W * H, 1)))
        out["filter_ms"] = spans(lambda: r.filter_frame_spatial(), lambda: r.last_filter_ms(), a.repeat)
        if a.bandwidth:
            out["read_bandwidth_gbps"] = float(r.measure_read_bandwidth(1 << 30, 10))
    if a.host:
        t0 = time.perf_counter()
        bloom.bloom_host(W, H, accum, 1.0, "accum", 1.0, 6, 1)
        out["host_ms"] = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
