"""The measurements of DESIGN.md §27 on one GPU, printed as one JSON line each:

  quality   S4 + cylinder at 64x48, 256 passes, ACES: the mean squared error of cpt_present_aa and of
            cpt_present on edge pixels against an 8W x 8H render of the same camera sampled at the
            sub-sample positions 8x + {-3, -1, 1, 3}, in tone-mapped linear values (bytes of the
            linear transfer / 255.99); the ratio must be below 1
  coverage  S1000 at 1920x1080, S = 4: cpt_last_aa_ms (and the call's G-buffer trace) against the S^2
            cpt_gbuffer calls with shifted cameras that give the same sub-sample data without this
            feature, timed by cpt_last_query_ms; the share of edge pixels
  present   cpt_present_aa against cpt_present at 1080p, cpt_last_present_ms over 20 calls of each
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

F = np.float32


def quality(r, sky):
    import tracked_reproject_model as tm
    from cpppathtracer_amd import antialias, camera_get_copy, present, scenes
    W, H, S, SPP = 64, 48, 4, 256
    r.set_scene(tm.scene())
    r.set_env(sky)

    def linear(frame):
        return frame[..., 2::-1].astype(np.float64) / 255.99   # R, G, B

    cam8 = camera_get_copy(scenes.camera_for(8 * W, 8 * H))
    r.set_frame(8 * W, 8 * H)
    r.init_rng(scenes.DEFAULT_SEED)
    r.render(cam8, SPP, 8, sync=True, ordered=True)
    big = linear(present.present(r, "accum", "aces", 4.0, "linear"))
    cam = camera_get_copy(scenes.camera_for(W, H))
    r.set_frame(W, H)
    r.init_rng(scenes.DEFAULT_SEED)
    r.render(cam, SPP, 8, sync=True, ordered=True)
    antialias.coverage(r, cam, S)
    _, flags = antialias.read_coverage(r)
    aa = linear(antialias.present_aa(r, "accum", "aces", 4.0, "linear"))
    plain = linear(present.present(r, "accum", "aces", 4.0, "linear"))
    # the reference of pixel (x, y): the 16 pixels (8x + o, 8y + p) of the large frame; x, y >= 1
    ref = np.zeros((H, W, 3))
    for p in (-3, -1, 1, 3):
        for o in (-3, -1, 1, 3):
            ref[1:, 1:] += big[8 + p::8, 8 + o::8][:H - 1, :W - 1]
    ref /= 16.0
    edge = (flags & 1).astype(bool)
    edge[0, :] = edge[:, 0] = False
    mse_aa = float(((aa - ref)[edge] ** 2).mean())
    mse_plain = float(((plain - ref)[edge] ** 2).mean())
    print(json.dumps(dict(what="quality", edge_pixels=int(edge.sum()), mse_aa=mse_aa, mse_plain=mse_plain, ratio=mse_aa / mse_plain)))
    assert mse_aa < mse_plain


def coverage(r):
    from cpppathtracer_amd import antialias, camera_get_copy, scenes
    from cpppathtracer_amd._lib import CPT_TRAVERSAL_ORDERED
    W, H, S = 1920, 1080, 4
    cam = camera_get_copy(scenes.camera_for(W, H))
    r.set_scene(scenes.scene_s1000())
    r.set_frame(W, H)
    aa_ms, trace_ms = [], []
    for _ in range(7):
        antialias.coverage(r, cam, S, 0.9, CPT_TRAVERSAL_ORDERED)
        aa_ms.append(antialias.last_aa_ms(r))
        trace_ms.append(r.last_query_ms())
    _, flags = antialias.read_coverage(r)
    share = float((flags & 1).astype(bool).mean())
    shifted_ms = []
    for _ in range(3):
        total = 0.0
        for s in range(S * S):
            ox, oy = (2 * (s % S) + 1 - S) / (2.0 * S), (2 * (s // S) + 1 - S) / (2.0 * S)
            c = np.array(cam, copy=True)
            c["top_left_corner"] = (np.asarray(cam["top_left_corner"], dtype=F) + F(ox / W) * np.asarray(cam["horizontal"], dtype=F)
                                    + F(oy / H) * np.asarray(cam["vertical"], dtype=F))
            r.gbuffer(c, CPT_TRAVERSAL_ORDERED)
            total += r.last_query_ms()
        shifted_ms.append(total)
    a, t, g = float(np.median(aa_ms[2:])), float(np.median(trace_ms[2:])), float(np.median(shifted_ms))
    print(json.dumps(dict(what="coverage", edge_share=share, aa_ms=a, gbuffer_trace_ms=t, sixteen_gbuffers_ms=g, ratio=a / g,
                          ratio_with_trace=(a + t) / g, aa_ms_all=aa_ms, shifted_ms_all=shifted_ms)))


def presents(r):
    import present_model as pm
    from cpppathtracer_amd import antialias, present
    W, H = 1920, 1080
    r.write_accum(pm.synthetic_accum(W * H, seed=5))   # the frame and the coverage are coverage()'s
    out = {}
    for tone, transfer in (("aces", "srgb"), ("clamp", "linear")):
        for name, call in (("present_aa", antialias.present_aa), ("present", present.present)):
            ms = []
            for _ in range(22):
                call(r, "accum", tone, 4.0, transfer, host=False)
                ms.append(present.last_present_ms(r))
            out[f"{name} {tone} {transfer}"] = float(np.median(ms[2:]))
    print(json.dumps(dict(what="present", median_ms=out)))


def main():
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    from cpppathtracer_amd import Renderer, texture_io
    sky = texture_io.load_cptex()
    with Renderer(0) as r:
        quality(r, sky)
        coverage(r)
        presents(r)


if __name__ == "__main__":
    main()
