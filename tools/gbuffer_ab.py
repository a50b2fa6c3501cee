#!/usr/bin/env python
"""The G-buffer pass beside the nearest thing a render can do.

C4 by default (S1000, 1920 x 1080), one GPU, ordered walk.  Reported: the device time of cpt_gbuffer
(cpt_last_query_ms) and of cpt_render(spp = 1, max_depth = 1) with and without CPT_RENDER_AUX
(cpt_last_render_ms), each the median of --repeat calls after a warm-up, and the G-buffer's hit
share.  With --skip-gbuffer only the renders run, so a build that predates the G-buffer (CPT_LIB_PATH
pointing at it) gives the render's time on that build.

    python tools/gbuffer_ab.py [--config c4] [--walk ordered] [--repeat 5] [--skip-gbuffer]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: torch's)

from cpppathtracer_amd import Renderer, camera_get_copy, scenes, texture_io
from cpppathtracer_amd._lib import CPT_TRAVERSAL_ORDERED


def median_ms(call, read, repeat):
    call()
    read()   # warm-up
    ms = []
    for _ in range(repeat):
        call()
        ms.append(read())
    return float(np.median(ms)), [round(m, 4) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=list(scenes.CONFIGS))
    ap.add_argument("--walk", default="ordered", choices=["reference", "ordered"])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-gbuffer", action="store_true")
    a = ap.parse_args()
    cfg = scenes.CONFIGS[a.config]
    W, H = cfg["width"], cfg["height"]
    flags = CPT_TRAVERSAL_ORDERED if a.walk == "ordered" else 0
    cam = camera_get_copy(scenes.camera_for(W, H))
    out = dict(config=a.config, width=W, height=H, walk=a.walk, repeat=a.repeat, lib=os.environ.get("CPT_LIB_PATH", "default"))
    with Renderer(0) as r:
        r.set_scene(scenes.SCENES[cfg["scene"]]())
        r.set_env(texture_io.load_cptex())
        r.set_frame(W, H)
        r.init_rng(scenes.DEFAULT_SEED)
        for aux in (False, True):
            med, all_ms = median_ms(lambda: r.render(cam, 1, 1, aux=aux, flags=flags), r.last_render_ms, a.repeat)
            out["render_1spp_depth1" + ("_aux" if aux else "") + "_ms"] = med
            print(f"render spp=1 max_depth=1 aux={aux}: median {med:.4f} ms {all_ms}", flush=True)
        if not a.skip_gbuffer:
            med, all_ms = median_ms(lambda: r.gbuffer(cam, flags), r.last_query_ms, a.repeat)
            g = r.read_gbuffer()
            out["gbuffer_ms"] = med
            out["hit_share"] = float((g["id"] >= 0).mean())
            print(f"gbuffer: median {med:.4f} ms {all_ms}; {100 * out['hit_share']:.1f}% of the pixels hit an object", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
