"""Presenting an HDR frame: functions on a ``Renderer`` over the C-ABI's
cpt_set_exposure, cpt_meter_exposure, cpt_read_exposure, cpt_present and their read-outs, and the
host-only hooks on the same arithmetic.

    from cpppathtracer_amd import present
    present.meter_exposure(r)                    # the median luminance to middle grey, on the device
    frame = present.present(r, tone="aces")      # (n_rows, width, 4) uint8: B, G, R, 255

The exposure lives in device memory: a meter and a present queue behind a render and behind each
other on the context's stream with no host wait between them.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import (CPT_PRESENT_ACCUM, CPT_PRESENT_FILTERED, CPT_TONE_ACES, CPT_TONE_CLAMP, CPT_TONE_REINHARD,
                   CPT_TRANSFER_LINEAR, CPT_TRANSFER_SRGB, check)

SOURCES = {"accum": CPT_PRESENT_ACCUM, "filtered": CPT_PRESENT_FILTERED}
TONES = {"clamp": CPT_TONE_CLAMP, "reinhard": CPT_TONE_REINHARD, "aces": CPT_TONE_ACES}
TRANSFERS = {"linear": CPT_TRANSFER_LINEAR, "srgb": CPT_TRANSFER_SRGB}
HIST_WORDS = 257


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _enum(table, v, what):
    """A name of `table` or the integer itself (an unknown integer reaches the library, which refuses it)."""
    if isinstance(v, str):
        if v not in table:
            raise ValueError(f"{what} must be one of {tuple(table)}")
        return table[v]
    return int(v)


def _call(r, name, *args):
    st = getattr(r._L, name)(r._ctx, *args)
    return r._check(st) if st else st


# ---- on a Renderer ------------------------------------------------------------------------------
def set_exposure(r, exposure):
    """cpt_set_exposure: the exposure (finite, > 0), written on the context's stream."""
    _call(r, "cpt_set_exposure", ctypes.c_float(exposure))


def meter_exposure(r, source="accum", key=0.18, permille=500, adapt=1.0):
    """cpt_meter_exposure: histogram of the source's positive luminances (eight bins per octave),
    its `permille` thousandth brought to `key`: exposure <- key / L at adapt 1, else moved the
    share `adapt` of the way.  Asynchronous."""
    _call(r, "cpt_meter_exposure", _enum(SOURCES, source, "source"), ctypes.c_float(key), int(permille), ctypes.c_float(adapt))


def read_exposure(r):
    """cpt_read_exposure: (exposure as numpy float32, the last meter's 257 histogram words uint32:
    256 bins, then the pixels that were not metered).  Waits for the stream."""
    e = ctypes.c_float(0.0)
    hist = np.zeros(HIST_WORDS, dtype=np.uint32)
    _call(r, "cpt_read_exposure", ctypes.byref(e), _p(hist))
    return np.float32(e.value), hist


def present(r, source="accum", tone="aces", white=4.0, transfer="srgb", host=True):
    """cpt_present: the source times the exposure, through the tone curve and the transfer, into
    the context's BGRA8 plane.  host=True waits and returns it, (n_rows, width, 4) uint8;
    host=False only queues the kernel (read_present, or the library's cpt_copy_present_device, later)."""
    out = np.zeros((r.n_rows, r.width, 4), dtype=np.uint8) if host else None
    _call(r, "cpt_present", _enum(SOURCES, source, "source"), _enum(TONES, tone, "tone"), ctypes.c_float(white),
          _enum(TRANSFERS, transfer, "transfer"), _p(out))
    if host:
        _call(r, "cpt_synchronize")   # the copy to `out` follows the kernel on the stream
    return out


def read_present(r):
    """cpt_read_present: the last present's plane, (n_rows, width, 4) uint8.  Waits."""
    out = np.zeros((r.n_rows, r.width, 4), dtype=np.uint8)
    _call(r, "cpt_read_present", _p(out), out.size)
    return out


def last_present_ms(r) -> float:
    """Device time of the last meter_exposure's or present's launches (HIP events); waits for it."""
    ms = ctypes.c_float(0.0)
    _call(r, "cpt_last_present_ms", ctypes.byref(ms))
    return ms.value


# ---- host only, no GPU ---------------------------------------------------------------------------
def _source_plane(source, src):
    s = _enum(SOURCES, source, "source")
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 3 if s == CPT_PRESENT_FILTERED else 4)
    return s, src


def present_host(src, exposure=1.0, source="accum", tone="aces", white=4.0, transfer="srgb"):
    """cpt_present_host: the bytes present() gives for a source plane (the accumulator [npix, 4], or
    the filtered rgb [npix, 3]) at `exposure`: [npix, 4] uint8."""
    L = _lib.load()
    s, src = _source_plane(source, src)
    out = np.zeros((len(src), 4), dtype=np.uint8)
    check(L.cpt_present_host(len(src), s, _p(src), ctypes.c_float(exposure), _enum(TONES, tone, "tone"), ctypes.c_float(white),
                             _enum(TRANSFERS, transfer, "transfer"), _p(out)))
    return out


def meter_host(src, exposure=1.0, source="accum", key=0.18, permille=500, adapt=1.0):
    """cpt_meter_host: (the exposure that follows `exposure`, the 257 histogram words) as
    meter_exposure leaves them for a source plane."""
    L = _lib.load()
    s, src = _source_plane(source, src)
    e = ctypes.c_float(exposure)
    hist = np.zeros(HIST_WORDS, dtype=np.uint32)
    check(L.cpt_meter_host(len(src), s, _p(src), ctypes.c_float(key), int(permille), ctypes.c_float(adapt), ctypes.byref(e),
                           _p(hist)))
    return np.float32(e.value), hist


def srgb_thresholds_host():
    """cpt_present_srgb_thresholds_host: the 256 thresholds of the sRGB transfer, float32 (T[0] = 0)."""
    L = _lib.load()
    t = np.zeros(256, dtype=np.float32)
    check(L.cpt_present_srgb_thresholds_host(_p(t)))
    return t
