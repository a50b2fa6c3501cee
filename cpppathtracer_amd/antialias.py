"""Antialiased presentation: functions on a ``Renderer`` over the C-ABI's
cpt_aa_coverage, cpt_read_aa_coverage, cpt_present_aa and cpt_last_aa_ms, and the host-only hooks
on the same arithmetic.

    from cpppathtracer_amd import antialias
    antialias.coverage(r, cam, samples=4)              # S x S first-hit rays in every edge pixel
    frame = antialias.present_aa(r, tone="aces")       # (height, width, 4) uint8: B, G, R, 255

The coverage belongs to the camera and the scene it was traced with: run it again after a camera
move or an object edit, as ``Renderer.gbuffer``, whose planes it rewrites.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import CPT_AA_EDGE, CPT_AA_UNMATCHED, CPT_TRAVERSAL_ORDERED, check  # noqa: F401  (the flag bits are re-exported)
from .present import SOURCES, TONES, TRANSFERS, _call, _enum, _p, _source_plane
from .types import CAMERA_DTYPE


def _cam(cam):
    return np.array(cam, dtype=CAMERA_DTYPE)


# ---- on a Renderer ------------------------------------------------------------------------------
def coverage(r, cam, samples=4, normal_cos=0.9, flags=CPT_TRAVERSAL_ORDERED):
    """cpt_aa_coverage: the frame's G-buffer at `cam` (as r.gbuffer(cam, flags)), then samples x
    samples first-hit rays inside every edge pixel, each attributed to the pixel of the 3x3 block
    whose centre saw the same surface.  Needs a full frame.  Asynchronous."""
    c = _cam(cam)
    _call(r, "cpt_aa_coverage", _p(c), int(flags), int(samples), ctypes.c_float(normal_cos))


def read_coverage(r):
    """cpt_read_aa_coverage: (counts (n_rows, width, 9) uint8, summing to samples^2 per pixel;
    flags (n_rows, width) uint8 of CPT_AA_EDGE | CPT_AA_UNMATCHED).  Waits for the stream."""
    counts = np.zeros((r.n_rows, r.width, 9), dtype=np.uint8)
    flags = np.zeros((r.n_rows, r.width), dtype=np.uint8)
    _call(r, "cpt_read_aa_coverage", _p(counts), _p(flags), r.npix)
    return counts, flags


def present_aa(r, source="accum", tone="aces", white=4.0, transfer="srgb", host=True):
    """cpt_present_aa: present.present through the last coverage: each pixel the coverage-weighted
    mix of its block's tone-mapped colours.  host=True waits and returns the plane, (n_rows, width,
    4) uint8; host=False only queues the kernel (present.read_present later)."""
    out = np.zeros((r.n_rows, r.width, 4), dtype=np.uint8) if host else None
    _call(r, "cpt_present_aa", _enum(SOURCES, source, "source"), _enum(TONES, tone, "tone"), ctypes.c_float(white),
          _enum(TRANSFERS, transfer, "transfer"), _p(out))
    if host:
        _call(r, "cpt_synchronize")   # the copy to `out` follows the kernel on the stream
    return out


def last_aa_ms(r) -> float:
    """Device time of the last coverage's edge and coverage kernels (HIP events); waits for it."""
    ms = ctypes.c_float(0.0)
    _call(r, "cpt_last_aa_ms", ctypes.byref(ms))
    return ms.value


# ---- host only, no GPU ---------------------------------------------------------------------------
def rays_host(cam, W, H, samples, x, y):
    """cpt_aa_rays_host: (origins, directions), each (samples^2, 3) float32, of pixel (x, y)'s
    sub-samples in the order s = j * samples + i."""
    L = _lib.load()
    c = _cam(cam)
    n = int(samples) * int(samples) if samples in (2, 4) else 16
    o, d = np.zeros((n, 3), dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
    check(L.cpt_aa_rays_host(_p(c), int(W), int(H), int(samples), int(x), int(y), _p(o), _p(d)))
    return o, d


def coverage_host(W, H, samples, normal_cos, id, normal, sub_id, sub_normal):
    """cpt_aa_coverage_host: (counts (H, W, 9), flags (H, W)) from the G-buffer's id [npix] and
    normal [npix, 3] and every pixel's sub-sample hits sub_id [npix, samples^2], sub_normal [npix,
    samples^2, 3] (read for edge pixels only)."""
    L = _lib.load()
    n, s2 = int(W) * int(H), int(samples) * int(samples)
    id = np.ascontiguousarray(id, dtype=np.int32).reshape(n)
    normal = np.ascontiguousarray(normal, dtype=np.float32).reshape(n, 3)
    sub_id = np.ascontiguousarray(sub_id, dtype=np.int32).reshape(n, s2)
    sub_normal = np.ascontiguousarray(sub_normal, dtype=np.float32).reshape(n, s2, 3)
    counts = np.zeros((H, W, 9), dtype=np.uint8)
    flags = np.zeros((H, W), dtype=np.uint8)
    check(L.cpt_aa_coverage_host(int(W), int(H), int(samples), ctypes.c_float(normal_cos), _p(id), _p(normal), _p(sub_id),
                                 _p(sub_normal), _p(counts), _p(flags)))
    return counts, flags


def present_aa_host(W, H, samples, src, counts, exposure=1.0, source="accum", tone="aces", white=4.0, transfer="srgb"):
    """cpt_present_aa_host: the bytes present_aa gives for a source plane (present.present_host's
    `src`) under `counts` (H, W, 9) at `exposure`: (H, W, 4) uint8."""
    L = _lib.load()
    s, src = _source_plane(source, src)
    counts = np.ascontiguousarray(counts, dtype=np.uint8).reshape(int(W) * int(H), 9)
    if len(src) != len(counts):
        raise ValueError(f"present_aa_host: {len(src)} source pixels for a {W}x{H} frame")
    out = np.zeros((H, W, 4), dtype=np.uint8)
    check(L.cpt_present_aa_host(int(W), int(H), int(samples), s, _p(src), _p(counts), ctypes.c_float(exposure),
                                _enum(TONES, tone, "tone"), ctypes.c_float(white), _enum(TRANSFERS, transfer, "transfer"), _p(out)))
    return out
