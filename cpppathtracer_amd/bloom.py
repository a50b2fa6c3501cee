"""Bloom for presented frames: functions on a ``Renderer`` over the C-ABI's
cpt_bloom, cpt_read_bloom, cpt_present_bloom and cpt_last_bloom_ms, and the host-only hooks on the
same arithmetic.

    from cpppathtracer_amd import bloom, present
    present.meter_exposure(r)                          # the pyramid is in exposed units: meter first
    bloom.build(r, threshold=1.0, levels=6)            # the bright pass's pyramid, on the device
    frame = bloom.present_bloom(r, tone="aces", intensity=0.25)   # (height, width, 4) uint8: B, G, R, 255

The pyramid belongs to the source plane and the exposure it was built at: build it again after a
render, a filter or a meter.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import CPT_BLOOM_MAX_LEVELS, check
from .present import SOURCES, TONES, TRANSFERS, _call, _enum, _p, _source_plane

MAX_LEVELS = CPT_BLOOM_MAX_LEVELS


def level_shapes(W, H, levels=MAX_LEVELS):
    """[(w_l, h_l) for l = 0..levels]: level 0 is the frame, each further level half of the one
    before it, rounded up."""
    shapes = [(int(W), int(H))]
    for _ in range(int(levels)):
        w, h = shapes[-1]
        shapes.append(((w + 1) // 2, (h + 1) // 2))
    return shapes


# ---- on a Renderer ------------------------------------------------------------------------------
def build(r, source="accum", threshold=1.0, levels=6):
    """cpt_bloom: the pyramid U_1..U_levels of the source's bright pass (the exposed light above
    `threshold`) at the current exposure.  Needs a full frame.  Asynchronous."""
    _call(r, "cpt_bloom", _enum(SOURCES, source, "source"), ctypes.c_float(threshold), int(levels))


def present_bloom(r, source="accum", tone="aces", white=4.0, transfer="srgb", intensity=0.25, host=True):
    """cpt_present_bloom: present.present with intensity x the last build's glow added in front of
    the tone curve.  host=True waits and returns the plane, (n_rows, width, 4) uint8; host=False
    only queues the kernel (present.read_present later)."""
    out = np.zeros((r.n_rows, r.width, 4), dtype=np.uint8) if host else None
    _call(r, "cpt_present_bloom", _enum(SOURCES, source, "source"), _enum(TONES, tone, "tone"), ctypes.c_float(white),
          _enum(TRANSFERS, transfer, "transfer"), ctypes.c_float(intensity), _p(out))
    if host:
        _call(r, "cpt_synchronize")   # the copy to `out` follows the kernel on the stream
    return out


def read_level(r, level):
    """cpt_read_bloom: U_level of the last build, (h_level, w_level, 3) float32.  Waits for the stream."""
    shapes = level_shapes(r.width, r.height)
    w, h = shapes[level] if 0 <= int(level) < len(shapes) else (1, 1)   # an unknown level reaches the library, which refuses it
    out = np.zeros((h, w, 3), dtype=np.float32)
    _call(r, "cpt_read_bloom", int(level), _p(out), w * h)
    return out


def last_bloom_ms(r) -> float:
    """Device time of the last build's launches (HIP events); waits for it."""
    ms = ctypes.c_float(0.0)
    _call(r, "cpt_last_bloom_ms", ctypes.byref(ms))
    return ms.value


# ---- host only, no GPU ---------------------------------------------------------------------------
def _frame_plane(who, W, H, source, src):
    s, src = _source_plane(source, src)
    if len(src) != int(W) * int(H):
        raise ValueError(f"{who}: {len(src)} source pixels for a {W}x{H} frame")
    return s, src


def bloom_host(W, H, src, exposure=1.0, source="accum", threshold=1.0, levels=6, level=1):
    """cpt_bloom_host: U_level of the pyramid build() makes of a source plane (present.present_host's
    `src`) at `exposure`: (h_level, w_level, 3) float32."""
    L = _lib.load()
    s, src = _frame_plane("bloom_host", W, H, source, src)
    shapes = level_shapes(W, H)
    w, h = shapes[level] if 0 <= int(level) < len(shapes) else (1, 1)
    out = np.zeros((h, w, 3), dtype=np.float32)
    check(L.cpt_bloom_host(int(W), int(H), s, _p(src), ctypes.c_float(exposure), ctypes.c_float(threshold), int(levels), int(level),
                           _p(out)))
    return out


def present_bloom_host(W, H, src, exposure=1.0, source="accum", threshold=1.0, levels=6, intensity=0.25, tone="aces", white=4.0,
                       transfer="srgb"):
    """cpt_present_bloom_host: the bytes build() then present_bloom() give for a source plane at
    `exposure`: (H, W, 4) uint8."""
    L = _lib.load()
    s, src = _frame_plane("present_bloom_host", W, H, source, src)
    out = np.zeros((H, W, 4), dtype=np.uint8)
    check(L.cpt_present_bloom_host(int(W), int(H), s, _p(src), ctypes.c_float(exposure), ctypes.c_float(threshold), int(levels),
                                   ctypes.c_float(intensity), _enum(TONES, tone, "tone"), ctypes.c_float(white),
                                   _enum(TRANSFERS, transfer, "transfer"), _p(out)))
    return out

