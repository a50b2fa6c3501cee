"""What the Python binding passes across the C-ABI, pinned without a device.

A ``Renderer`` made by ``Renderer.__new__`` gets a sentinel ``_ctx`` and, as ``_L``, a stub whose
``cpt_*`` attributes return 0 and record each call: the entry's name, every scalar argument with
the ctypes type the prototype converts it to, and for every pointer argument whether it is null
and, for inputs, the bytes behind it (by name when they are one of this file's own inputs).
Every public method is driven once per branch and the recorded calls, the returned shapes and
dtypes, the ``ValueError`` texts and the public signatures are compared with literals.  The
module's host functions run against the same stub in place of the loaded library; their results
are held bit for bit against numpy models in test_reproject_model.py and its neighbours.
"""
import ctypes
import functools
import inspect
import types as pytypes

import numpy as np
import pytest

from cpppathtracer_amd import _lib, renderer
from cpppathtracer_amd.renderer import Renderer
from cpppathtracer_amd.types import CAMERA_DTYPE, MOTION_DTYPE, OBJECT_DTYPE, SPHERE, make_camera, make_material, make_object

W, H, NPIX = 4, 3, 12
CTX, SRC = 0xC0FFEE, 0xBEEF
I, U32, U64, SZ, FL = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_float
F32, I32, U8 = np.dtype(np.float32), np.dtype(np.int32), np.dtype(np.uint8)
UI32, UI64 = np.dtype(np.uint32), np.dtype(np.uint64)


def f(x):
    """A float argument as the entry receives it: rounded to float32."""
    return (FL, ctypes.c_float(x).value)


# ---- the inputs, each under the name the recorded calls show it by ------------------------------
IN = {}


def _in(name, a):
    IN[name] = a
    return a


def _ramp(name, shape, dtype, start):
    return _in(name, (np.arange(int(np.prod(shape))) + start).astype(dtype).reshape(shape))


CAM = _in("cam", make_camera(W, H, origin=(0.0, 0.0, -5.0)))
CAM2 = _in("cam2", make_camera(W, H, origin=(1.0, 0.0, -5.0)))
OBJS = _in("objs", np.array([make_object(SPHERE, make_material(kd=(0.5, 0.5, 0.5)), (0, 0, 0), 1.0),
                             make_object(SPHERE, make_material(kd=(0.1, 0.2, 0.3)), (2, 0, 0), 0.5)], dtype=OBJECT_DTYPE))
OBJS_B = _in("objs_b", np.array([OBJS[1], OBJS[0]], dtype=OBJECT_DTYPE))
_in("obj1", OBJS[1])
IDX = _in("idx", np.array([0, 1], dtype=np.int32))
ROWS = _in("rows", np.array([0, 2], dtype=np.int32))
RGBA = _in("rgba", np.arange(16, dtype=np.uint8).reshape(2, 2, 4))
TEX = pytypes.SimpleNamespace(rgba=RGBA, width=2, height=2, valid_cols=2)
ORG = _ramp("origins", (3, 3), np.float32, 100)
DIRS = _ramp("dirs", (3, 3), np.float32, 200)
TMIN = _ramp("tmin", (3,), np.float32, 300)
MOM = _ramp("moments", (4, NPIX), np.float32, 400)
RNG = _ramp("rng", (6, NPIX), np.uint32, 500)
ACC = _ramp("accum", (NPIX, 4), np.float32, 600)
NRM = _ramp("normal", (NPIX, 3), np.float32, 700)
DEP = _ramp("depth", (NPIX,), np.float32, 800)
GID = _ramp("id", (NPIX,), np.int32, 900)
ALB = _ramp("albedo", (NPIX, 3), np.float32, 1000)
DIR0 = _ramp("dir0", (NPIX, 3), np.float32, 1100)
DIR1 = _ramp("dir1", (NPIX, 3), np.float32, 1200)
ID0 = _ramp("id0", (NPIX,), np.int32, 1300)
T0 = _ramp("t0", (NPIX,), np.float32, 1400)
MEAN = _ramp("mean", (NPIX, 3), np.float32, 1500)
CNT = _ramp("count", (NPIX,), np.float32, 1600)
MA = _ramp("ma", (3,), np.float32, 1700)
MB = _ramp("mb", (3,), np.float32, 1800)
_in("zeros3", np.zeros(3, dtype=np.float32))
MOTION = np.zeros(2, dtype=MOTION_DTYPE)
MOTION["kind"] = (1, 4)
_in("motion", MOTION)
NAMES = {np.ascontiguousarray(a).tobytes(): name for name, a in IN.items()}
assert len(NAMES) == len(IN)

CAMB, OBJB = CAMERA_DTYPE.itemsize, OBJECT_DTYPE.itemsize
_HOST = {0: CAMB, 1: CAMB, 4: 144, 5: 144, 6: 48, 7: 48, 8: 48, 9: 48, 10: 144}
# byte length of every input pointer, by entry and argument index; "handle": an opaque address,
# recorded as a number; a pointer not listed is an output
PTRS = {
    "cpt_set_stream": {1: "handle"}, "cpt_set_scene": {1: 2 * OBJB}, "cpt_update_object": {2: OBJB},
    "cpt_update_objects": {2: 8, 3: 2 * OBJB}, "cpt_update_objects_rebuild": {2: 8, 3: 2 * OBJB},
    "cpt_set_env_texture": {1: 16}, "cpt_bind_texture": {2: 16}, "cpt_set_frame": {3: 8},
    "cpt_render": {1: CAMB}, "cpt_render_to_count": {1: CAMB}, "cpt_render_adaptive": {1: CAMB},
    "cpt_adaptive_begin": {1: CAMB}, "cpt_write_moments": {1: 192}, "cpt_gbuffer": {1: CAMB},
    "cpt_write_gbuffer": {1: 48, 2: 48, 3: 144, 4: 144}, "cpt_trace_rays": {2: 36, 3: 36, 4: 12}, "cpt_pick": {1: CAMB},
    "cpt_reproject_accum": {1: CAMB, 2: CAMB}, "cpt_reproject_display": {1: CAMB, 2: CAMB},
    "cpt_history_capture": {1: CAMB}, "cpt_reproject_accum_tracked": {1: CAMB},
    "cpt_reproject_display_tracked": {1: CAMB}, "cpt_tile_costs": {1: CAMB}, "cpt_write_rng": {1: 288},
    "cpt_write_accum": {1: 192}, "cpt_write_aux": {1: 144, 2: 48},
    "cpt_copy_accum_device": {1: "handle", 3: "handle"}, "cpt_copy_bgra_device": {1: "handle", 3: "handle"},
    "cpt_math_batch": {2: 12, 3: 12}, "cpt_camera_get_copy": {0: CAMB},
    "cpt_object_motion_host": {0: 2 * OBJB, 1: 2 * OBJB},
    "cpt_reproject_host": {**_HOST, 11: 192}, "cpt_reproject_display_host": {**_HOST, 11: 144, 12: 48},
    "cpt_reproject_tracked_host": {**_HOST, 11: 192, 12: 80},
    "cpt_reproject_display_tracked_host": {**_HOST, 11: 144, 12: 48, 13: 80},
}


def input_name(b):
    """The input these bytes are: by its bytes, or field by field for a struct with padding (a
    copy of one leaves the padding undefined); bytes that are no input show as hex."""
    if b in NAMES:
        return NAMES[b]
    for name, a in IN.items():
        if a.dtype.names and a.nbytes == len(b) and np.array_equal(np.frombuffer(b, dtype=a.dtype).reshape(a.shape), a):
            return name
    return b.hex()


class Stub:
    """Stands in for the loaded library.  `outs`: {entry: {argument index: bytes}} written through
    each non-null output pointer; `returns`: {entry: value} where an entry returns other than 0."""

    def __init__(self, outs=None, returns=None):
        self.calls, self.outs, self.returns = [], outs or {}, returns or {}

    def __getattr__(self, name):
        if not name.startswith("cpt_"):
            raise AttributeError(name)
        return functools.partial(self._entry, name)

    def _entry(self, name, *args):
        argtypes = _lib.PROTOTYPES[name][1]
        assert len(args) == len(argtypes), (name, len(args))
        rec = [name]
        for i, (a, t) in enumerate(zip(args, argtypes)):
            t.from_param(a)   # raises what the real entry's argument conversion would
            if t is not ctypes.c_void_p:
                rec.append((t, a.value if isinstance(a, ctypes._SimpleCData) else t(a).value))
                continue
            addr = None if a is None else ctypes.cast(a, ctypes.c_void_p).value
            kind = PTRS.get(name, {}).get(i)
            if addr is None:
                rec.append(None)
            elif addr in (CTX, SRC):
                rec.append("ctx" if addr == CTX else "src")
            elif kind == "handle":
                rec.append(addr)
            elif kind is not None:
                rec.append(input_name(ctypes.string_at(addr, kind)))
            else:
                rec.append("out")
                out = self.outs.get(name, {}).get(i)
                if out is not None:
                    ctypes.memmove(addr, bytes(out), len(bytes(out)))
        self.calls.append(tuple(rec))
        return self.returns.get(name, 0)


def make(outs=None, returns=None, ctx=CTX):
    r = Renderer.__new__(Renderer)
    r._L, r._ctx, r.device = Stub(outs, returns), ctypes.c_void_p(ctx), 0
    r.width, r.height, r.n_rows, r.rows = W, H, H, np.arange(H, dtype=np.int32)
    return r


def desc(v):
    """Shape and dtype of what a method returned (and the values of a small plain array)."""
    if isinstance(v, np.ndarray):
        small = v.dtype.names is None and v.size <= 8
        return (v.shape, v.dtype, v.tolist()) if small else (v.shape, v.dtype)
    if isinstance(v, dict):
        return {k: desc(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return type(v)(desc(x) for x in v)
    return None if v is None else (type(v).__name__, v)


def u64s(*v):
    return np.array(v, dtype=np.uint64).tobytes()


TIMELINE = np.zeros(4 * 4096 + 4, dtype=np.uint64)
TIMELINE[4 * 4096] = 9
BAND = {"cpt_display_band": {1: I(1), 2: I(3)}}
INFO = {"cpt_adaptive_info": {1: I(2), 2: np.array([5, 3], dtype=np.uint32).tobytes(), 4: U64(77)}}
INFO_CALLS = [("cpt_adaptive_info", "ctx", "out", None, (I, 0), "out"), ("cpt_adaptive_info", "ctx", "out", "out", (I, 2), "out")]
INFO_RET = {"rounds": ("int", 2), "active_tiles": ((2,), UI32, [5, 3]), "passes_done": ("int", 77)}
GBUF = {"id": ((NPIX,), I32), "t": ((NPIX,), F32), "normal": ((NPIX, 3), F32), "albedo": ((NPIX, 3), F32)}
FRAME = ((H, W, 4), U8)

# (id, the call, the entries it must reach, what it returns, scripted outputs)
CASES = [
    ("set_stream", lambda r: r.set_stream(0x1234), [("cpt_set_stream", "ctx", 0x1234)], None, None),
    ("set_stream_none", lambda r: r.set_stream(None), [("cpt_set_stream", "ctx", None)], None, None),
    ("set_scene", lambda r: r.set_scene(OBJS), [("cpt_set_scene", "ctx", "objs", (I, 2))], None, None),
    ("set_scene_empty", lambda r: r.set_scene(np.zeros(0, dtype=OBJECT_DTYPE)), [("cpt_set_scene", "ctx", None, (I, 0))],
     None, None),
    ("update_object", lambda r: r.update_object(1, OBJS[1]), [("cpt_update_object", "ctx", (I, 1), "obj1")], None, None),
    ("update_objects", lambda r: r.update_objects([0, 1], OBJS),
     [("cpt_update_objects", "ctx", (I, 2), "idx", "objs")], None, None),
    ("update_objects_rebuild", lambda r: r.update_objects([0, 1], OBJS, rebuild=True),
     [("cpt_update_objects_rebuild", "ctx", (I, 2), "idx", "objs")], None, None),
    ("material_count", lambda r: r.material_count(), [("cpt_get_material_count", "ctx", "out")], ("int", 7),
     {"cpt_get_material_count": {1: I(7)}}),
    ("last_update_ms", lambda r: r.last_update_ms(), [("cpt_last_update_ms", "ctx", "out")], ("float", 1.5),
     {"cpt_last_update_ms": {1: FL(1.5)}}),
    ("bvh_export", lambda r: r.bvh_export(),
     [("cpt_scene_bvh_export", "ctx", None, None, (I, 0), "out"), ("cpt_scene_bvh_export", "ctx", "out", "out", (I, 1), "out")],
     (((1, 6), F32, [[1, 2, 3, 4, 5, 6]]), ((1, 4), I32, [[7, 8, 9, 10]])),
     {"cpt_scene_bvh_export": {1: np.arange(1, 7, dtype=np.float32).tobytes(), 2: np.arange(7, 11, dtype=np.int32).tobytes(),
                               4: I(1)}}),
    ("set_env_none", lambda r: r.set_env(None), [("cpt_set_env_texture", "ctx", None, (I, 1), (I, 1), (I, 0))], None, None),
    ("set_env", lambda r: r.set_env(TEX), [("cpt_set_env_texture", "ctx", "rgba", (I, 2), (I, 2), (I, 2))], None, None),
    ("bind_texture", lambda r: r.bind_texture(5, TEX),
     [("cpt_bind_texture", "ctx", (U64, 5), "rgba", (I, 2), (I, 2), (I, 2), (I, 2), (I, 1))], None, None),
    ("bind_texture_modes", lambda r: r.bind_texture(5, TEX, address_mode=0, filter_mode=0),
     [("cpt_bind_texture", "ctx", (U64, 5), "rgba", (I, 2), (I, 2), (I, 2), (I, 0), (I, 0))], None, None),
    ("init_rng", lambda r: r.init_rng(1 << 40), [("cpt_init_rng", "ctx", (U64, 1 << 40))], None, None),
    ("render_to_count", lambda r: r.render_to_count(CAM, 16, 8),
     [("cpt_render_to_count", "ctx", "cam", (I, 16), (I, 8), (U32, 0))], None, None),
    ("render_to_count_flags", lambda r: r.render_to_count(CAM, 16, 8, aux=True, stats=True, sync=True, flags=0x200),
     [("cpt_render_to_count", "ctx", "cam", (I, 16), (I, 8), (U32, 0x20E))], None, None),
    ("topup_info", lambda r: r.topup_info(), [("cpt_topup_info", "ctx", "out", "out", "out")],
     {"tiles": ("int", 1), "pixels": ("int", 12), "passes": ("int", 1 << 33)},
     {"cpt_topup_info": {1: U32(1), 2: U64(12), 3: U64(1 << 33)}}),
    ("render_adaptive", lambda r: r.render_adaptive(CAM, 4, 64, 4, 0.05, 8, flags=0x200),
     [("cpt_render_adaptive", "ctx", "cam", (I, 4), (I, 64), (I, 4), f(0.05), (I, 8), (U32, 0x200))] + INFO_CALLS,
     INFO_RET, INFO),
    ("adaptive_info", lambda r: r.adaptive_info(), INFO_CALLS, INFO_RET, INFO),
    ("adaptive_info_none", lambda r: r.adaptive_info(),
     [("cpt_adaptive_info", "ctx", "out", None, (I, 0), "out"), ("cpt_adaptive_info", "ctx", "out", "out", (I, 1), "out")],
     {"rounds": ("int", 0), "active_tiles": ((0,), UI32, []), "passes_done": ("int", 0)}, None),
    ("adaptive_begin", lambda r: r.adaptive_begin(CAM, 4, 64, 4, 0.05, 8),
     [("cpt_adaptive_begin", "ctx", "cam", (I, 4), (I, 64), (I, 4), f(0.05), (I, 8), (U32, 0))], None, None),
    ("adaptive_step", lambda r: r.adaptive_step(), [("cpt_adaptive_step", "ctx", "out")], ("int", 3),
     {"cpt_adaptive_step": {1: I(3)}}),
    ("read_noise", lambda r: r.read_noise(), [("cpt_read_noise", "ctx", "out", (SZ, NPIX))], ((NPIX,), F32), None),
    ("read_moments", lambda r: r.read_moments(), [("cpt_read_moments", "ctx", "out", (SZ, 4 * NPIX))], ((4, NPIX), F32), None),
    ("write_moments", lambda r: r.write_moments(MOM.astype(np.float64)),
     [("cpt_write_moments", "ctx", "moments", (SZ, 4 * NPIX))], None, None),
    ("filter_frame", lambda r: r.filter_frame(), [("cpt_filter_frame", "ctx", (I, 5), f(1.0), (I, 7))], None, None),
    ("filter_frame_args", lambda r: r.filter_frame(2, 0.3, 4), [("cpt_filter_frame", "ctx", (I, 2), f(0.3), (I, 4))], None, None),
    ("filter_frame_spatial", lambda r: r.filter_frame_spatial(),
     [("cpt_filter_frame_spatial", "ctx", (I, 3), f(2.0), (I, 3))], None, None),
    ("read_filtered", lambda r: r.read_filtered(), [("cpt_read_filtered", "ctx", "out", "out", (SZ, NPIX))],
     (((NPIX, 3), F32), ((NPIX,), F32)), None),
    ("last_filter_ms", lambda r: r.last_filter_ms(), [("cpt_last_filter_ms", "ctx", "out")], ("float", 0.25),
     {"cpt_last_filter_ms": {1: FL(0.25)}}),
    ("gbuffer", lambda r: r.gbuffer(CAM), [("cpt_gbuffer", "ctx", "cam", (U32, 0))], None, None),
    ("gbuffer_flags", lambda r: r.gbuffer(CAM, flags=0x600), [("cpt_gbuffer", "ctx", "cam", (U32, 0x600))], None, None),
    ("read_gbuffer", lambda r: r.read_gbuffer(), [("cpt_read_gbuffer", "ctx", "out", "out", "out", "out", (SZ, NPIX))],
     GBUF, None),
    ("write_gbuffer", lambda r: r.write_gbuffer(GID, DEP, NRM.reshape(-1), ALB),
     [("cpt_write_gbuffer", "ctx", "id", "depth", "normal", "albedo", (SZ, NPIX))], None, None),
    ("write_gbuffer_none", lambda r: r.write_gbuffer(), [("cpt_write_gbuffer", "ctx", None, None, None, None, (SZ, NPIX))],
     None, None),
    ("write_gbuffer_some", lambda r: r.write_gbuffer(t=DEP, albedo=ALB),
     [("cpt_write_gbuffer", "ctx", None, "depth", None, "albedo", (SZ, NPIX))], None, None),
    ("trace_rays", lambda r: r.trace_rays(ORG, DIRS),
     [("cpt_trace_rays", "ctx", (SZ, 3), "origins", "dirs", None, (U32, 0), "out", "out", "out")],
     {"id": ((3,), I32, [0, 0, 0]), "t": ((3,), F32, [0, 0, 0]), "normal": ((3, 3), F32)}, None),
    ("trace_rays_tmin", lambda r: r.trace_rays(ORG.reshape(-1), DIRS, tmin=TMIN, flags=0x200),
     [("cpt_trace_rays", "ctx", (SZ, 3), "origins", "dirs", "tmin", (U32, 0x200), "out", "out", "out")],
     {"id": ((3,), I32, [0, 0, 0]), "t": ((3,), F32, [0, 0, 0]), "normal": ((3, 3), F32)}, None),
    ("pick", lambda r: r.pick(CAM, 2, 1, flags=0x200),
     [("cpt_pick", "ctx", "cam", (I, 2), (I, 1), (U32, 0x200), "out", "out")], (("int", 1), ("float32", np.float32(2.5))),
     {"cpt_pick": {5: ctypes.c_int32(1), 6: FL(2.5)}}),
    ("last_query_ms", lambda r: r.last_query_ms(), [("cpt_last_query_ms", "ctx", "out")], ("float", 0.5),
     {"cpt_last_query_ms": {1: FL(0.5)}}),
    ("reproject_accum", lambda r: r.reproject_accum(CAM, CAM2),
     [("cpt_reproject_accum", "ctx", "cam", "cam2", (I, 32), f(1e-2), (U32, 0))], None, None),
    ("reproject_accum_args", lambda r: r.reproject_accum(CAM2, CAM, max_history=8, plane_tol=0.5, flags=0x200),
     [("cpt_reproject_accum", "ctx", "cam2", "cam", (I, 8), f(0.5), (U32, 0x200))], None, None),
    ("reproject_display", lambda r: r.reproject_display(CAM, CAM2, 8, 0.5, 0x200),
     [("cpt_reproject_display", "ctx", "cam", "cam2", (I, 8), f(0.5), (U32, 0x200))], None, None),
    ("reproject_display_defaults", lambda r: r.reproject_display(CAM, CAM2),
     [("cpt_reproject_display", "ctx", "cam", "cam2", (I, 32), f(1e-2), (U32, 0))], None, None),
    ("history_capture", lambda r: r.history_capture(CAM, flags=0x200), [("cpt_history_capture", "ctx", "cam", (U32, 0x200))],
     None, None),
    ("history_info", lambda r: r.history_info(), [("cpt_history_info", "ctx", "out", "out")],
     (("bool", True), ((), CAMERA_DTYPE)), {"cpt_history_info": {1: I(1), 2: CAM.tobytes()}}),
    ("history_info_none", lambda r: r.history_info(), [("cpt_history_info", "ctx", "out", "out")], (("bool", False), None), None),
    ("reproject_accum_tracked", lambda r: r.reproject_accum_tracked(CAM2),
     [("cpt_reproject_accum_tracked", "ctx", "cam2", (I, 32), f(1e-2), (U32, 0))], None, None),
    ("reproject_accum_tracked_args", lambda r: r.reproject_accum_tracked(CAM2, 8, 0.5, 0x200),
     [("cpt_reproject_accum_tracked", "ctx", "cam2", (I, 8), f(0.5), (U32, 0x200))], None, None),
    ("reproject_display_tracked", lambda r: r.reproject_display_tracked(CAM2),
     [("cpt_reproject_display_tracked", "ctx", "cam2", (I, 32), f(1e-2), (U32, 0))], None, None),
    ("reproject_display_tracked_args", lambda r: r.reproject_display_tracked(CAM2, 8, 0.5, 0x200),
     [("cpt_reproject_display_tracked", "ctx", "cam2", (I, 8), f(0.5), (U32, 0x200))], None, None),
    ("last_reproject_ms", lambda r: r.last_reproject_ms(), [("cpt_last_reproject_ms", "ctx", "out")], ("float", 0.75),
     {"cpt_last_reproject_ms": {1: FL(0.75)}}),
    ("last_reproject_ms_split", lambda r: r.last_reproject_ms(split=True), [("cpt_last_reproject_launch_ms", "ctx", "out")],
     (("float", 0.0), ("float", 0.5), ("float", 0.25)),
     {"cpt_last_reproject_launch_ms": {1: np.array([0, 0.5, 0.25], dtype=np.float32).tobytes()}}),
    ("tile_costs", lambda r: r.tile_costs(CAM, 4, 8),
     [("cpt_tile_costs", "ctx", "cam", (I, 4), (I, 8), (U32, 0x200), "out", (SZ, 1))], ((1, 1), UI32, [[6]]),
     {"cpt_tile_costs": {5: U32(6)}}),
    ("tile_costs_reference", lambda r: r.tile_costs(CAM, 4, 8, ordered=False),
     [("cpt_tile_costs", "ctx", "cam", (I, 4), (I, 8), (U32, 0), "out", (SZ, 1))], ((1, 1), UI32, [[0]]), None),
    ("tile_costs_plain", lambda r: r.tile_costs(CAM, 4, 8, ordered="plain"),
     [("cpt_tile_costs", "ctx", "cam", (I, 4), (I, 8), (U32, 0x600), "out", (SZ, 1))], ((1, 1), UI32, [[0]]), None),
    ("synchronize", lambda r: r.synchronize(), [("cpt_synchronize", "ctx")], None, None),
    ("last_render_ms", lambda r: r.last_render_ms(), [("cpt_last_render_ms", "ctx", "out")], ("float", 2.5),
     {"cpt_last_render_ms": {1: FL(2.5)}}),
    ("last_kernel_stats", lambda r: r.last_kernel_stats(), [("cpt_last_kernel_stats", "ctx", "out", "out")],
     (("float", 1.25), ("int", 2)), {"cpt_last_kernel_stats": {1: FL(1.25), 2: I(2)}}),
    ("npix", lambda r: r.npix, [], ("int", NPIX), None),
    ("read_accum", lambda r: r.read_accum(), [("cpt_read_accum", "ctx", "out")], ((NPIX, 4), F32), None),
    ("clear_accum", lambda r: r.clear_accum(), [("cpt_clear_accum", "ctx")], None, None),
    ("read_rng", lambda r: r.read_rng(), [("cpt_read_rng", "ctx", "out")], ((6, NPIX), UI32), None),
    ("write_rng", lambda r: r.write_rng(RNG.astype(np.int64)), [("cpt_write_rng", "ctx", "rng")], None, None),
    ("read_aux", lambda r: r.read_aux(), [("cpt_read_aux", "ctx", "out", "out")], (((NPIX, 3), F32), ((NPIX,), F32)), None),
    ("write_accum", lambda r: r.write_accum(ACC.reshape(H, W, 4)), [("cpt_write_accum", "ctx", "accum")], None, None),
    ("write_aux", lambda r: r.write_aux(NRM.reshape(H, W, 3), DEP.reshape(H, W)), [("cpt_write_aux", "ctx", "normal", "depth")],
     None, None),
    ("copy_accum_device", lambda r: r.copy_accum_device(0x7000, 192, 0x55),
     [("cpt_copy_accum_device", "ctx", 0x7000, (SZ, 192), 0x55)], None, None),
    ("copy_accum_device_null_stream", lambda r: r.copy_accum_device(0x7000, 192, 0),
     [("cpt_copy_accum_device", "ctx", 0x7000, (SZ, 192), None)], None, None),
    ("gather_rows", lambda r: r.gather_rows(make(ctx=SRC)), [("cpt_gather_rows", "ctx", "src")], None, None),
    ("last_gather_mode", lambda r: r.last_gather_mode(make(ctx=SRC)), [("cpt_last_gather_mode", "ctx", "src", "out")],
     ("str", "peer"), {"cpt_last_gather_mode": {2: I(1)}}),
    ("set_debug_gather", lambda r: r.set_debug_gather("yes"), [("cpt_set_debug_gather", "ctx", (I, 1))], None, None),
    ("stats", lambda r: r.stats(), [("cpt_get_stats", "ctx", "out")],
     {"segments": ("int", 1), "nodes": ("int", 2), "prims": ("int", 3), "hits": ("int", 4), "misses": ("int", 1 << 40)},
     {"cpt_get_stats": {1: u64s(1, 2, 3, 4, 1 << 40)}}),
    ("raw_counters", lambda r: r.raw_counters(), [("cpt_get_raw_counters", "ctx", "out")],
     [("int", v) for v in (1, 2, 3, 4, 5, 6, 7, 8)], {"cpt_get_raw_counters": {1: u64s(1, 2, 3, 4, 5, 6, 7, 8)}}),
    ("debug_timeline", lambda r: r.debug_timeline(), [("cpt_debug_timeline", "ctx", "out", (I, 4 * 4096 + 4))],
     (((4096, 4), UI64), ("int", 9)), {"cpt_debug_timeline": {1: TIMELINE.tobytes()}}),
    ("diag_counters", lambda r: r.diag_counters(), [("cpt_get_diag_counters", "ctx", "out")], [("int", 0)] * 16, None),
    ("execdiag_counters", lambda r: r.execdiag_counters(), [("cpt_get_execdiag_counters", "ctx", "out")], ((4, 16), UI64), None),
    ("walk_info", lambda r: r.walk_info(), [("cpt_get_walk_info", "ctx", "out")],
     {"n_bvh": ("int", 3), "n_walk": ("int", 5), "n_wide": ("int", 2), "n_unb": ("int", 1)},
     {"cpt_get_walk_info": {1: np.array([3, 5, 2, 1], dtype=np.int32).tobytes()}}),
    ("read_nodes", lambda r: r.read_nodes(),
     [("cpt_debug_read_nodes", "ctx", None, (SZ, 0), "out"), ("cpt_debug_read_nodes", "ctx", "out", (SZ, 3), "out")],
     ((3,), U8, [7, 8, 9]), {"cpt_debug_read_nodes": {1: b"\x07\x08\x09", 3: SZ(3)}}),
    ("read_nodes_empty", lambda r: r.read_nodes(), [("cpt_debug_read_nodes", "ctx", None, (SZ, 0), "out")], ((0,), U8, []), None),
    ("debug_tile_order", lambda r: r.debug_tile_order(4),
     [("cpt_debug_read_tile_order", "ctx", (I, 4), "out", (SZ, 1), "out")], ((1,), UI32, [0]),
     {"cpt_debug_read_tile_order": {4: SZ(1)}}),
    ("measure_read_pattern", lambda r: r.measure_read_pattern(12),
     [("cpt_measure_read_pattern", "ctx", (I, 12), (SZ, 1 << 30), (I, 1), "out")], ("float", 4000.0),
     {"cpt_measure_read_pattern": {4: FL(4000.0)}}),
    ("measure_read_bandwidth", lambda r: r.measure_read_bandwidth(),
     [("cpt_measure_read_bandwidth", "ctx", (SZ, 4 << 30), (I, 10), "out")], ("float", 5000.0),
     {"cpt_measure_read_bandwidth": {3: FL(5000.0)}}),
    ("set_debug_consolidation", lambda r: r.set_debug_consolidation(3, 4, 5),
     [("cpt_set_debug_consolidation", "ctx", (U32, 3), (I, 4), (I, 5))], None, None),
    ("set_debug_grid", lambda r: r.set_debug_grid(2, 16), [("cpt_set_debug_grid", "ctx", (I, 2), (I, 16))], None, None),
    ("set_debug_grid_off", lambda r: r.set_debug_grid(), [("cpt_set_debug_grid", "ctx", (I, 0), (I, 0))], None, None),
    ("reset_stats", lambda r: r.reset_stats(), [("cpt_reset_stats", "ctx")], None, None),
    ("selftest_qdiv", lambda r: r.selftest_qdiv(2, 10, examples=2),
     [("cpt_selftest_qdiv", "ctx", (I, 2), (U64, 10), (U64, 1), "out", (I, 3))],
     (("int", 1), [(("float32", np.float32(1.5)), ("float32", np.float32(0.5)))]),
     {"cpt_selftest_qdiv": {4: u64s(1, (0x3FC00000 << 32) | 0x3F000000, 0)}}),
    ("denoise_mix", lambda r: r.denoise_mix(3), [("cpt_denoise_mix", "ctx", (U32, 3), "out")], FRAME, None),
    ("denoise_mix_device", lambda r: r.denoise_mix(3, host=False), [("cpt_denoise_mix", "ctx", (U32, 3), None)], None, None),
    ("denoise_mix_history", lambda r: r.denoise_mix_history(), [("cpt_denoise_mix_history", "ctx", "out")], FRAME, None),
    ("denoise_mix_history_device", lambda r: r.denoise_mix_history(host=False), [("cpt_denoise_mix_history", "ctx", None)],
     None, None),
    ("read_display_count", lambda r: r.read_display_count(),
     [("cpt_display_band", "ctx", "out", "out"), ("cpt_read_display_count", "ctx", "out", (SZ, 8))], ((8,), F32, [0.0] * 8), BAND),
    ("display_band", lambda r: r.display_band(), [("cpt_display_band", "ctx", "out", "out")], (("int", 1), ("int", 3)), BAND),
    ("read_mix", lambda r: r.read_mix(), [("cpt_display_band", "ctx", "out", "out"), ("cpt_read_mix", "ctx", "out", (SZ, 24))],
     ((8, 3), F32), BAND),
    ("last_display_ms", lambda r: r.last_display_ms(), [("cpt_last_display_ms", "ctx", "out")], ("float", 0.125),
     {"cpt_last_display_ms": {1: FL(0.125)}}),
    ("denoise_mix_band", lambda r: r.denoise_mix_band(3, 1, 3),
     [("cpt_denoise_mix_band", "ctx", (U32, 3), (I, 1), (I, 3), "out")], ((2, W, 4), U8), None),
    ("denoise_mix_band_device", lambda r: r.denoise_mix_band(3, 1, 3, host=False),
     [("cpt_denoise_mix_band", "ctx", (U32, 3), (I, 1), (I, 3), None)], None, None),
    ("copy_bgra_device", lambda r: r.copy_bgra_device(0x7000, 48, 0x55),
     [("cpt_copy_bgra_device", "ctx", 0x7000, (SZ, 48), 0x55)], None, None),
    ("copy_bgra_device_null_stream", lambda r: r.copy_bgra_device(0x7000, 48, None),
     [("cpt_copy_bgra_device", "ctx", 0x7000, (SZ, 48), None)], None, None),
    ("reset_display", lambda r: r.reset_display(), [("cpt_reset_display", "ctx")], None, None),
    ("math_batch", lambda r: r.math_batch(7, MA), [("cpt_math_batch", "ctx", (I, 7), "ma", "zeros3", "out", (SZ, 3))],
     ((3,), F32, [1.0, 2.0, 3.0]), {"cpt_math_batch": {4: np.array([1, 2, 3], dtype=np.float32).tobytes()}}),
    ("math_batch_two", lambda r: r.math_batch(7, MA, MB), [("cpt_math_batch", "ctx", (I, 7), "ma", "mb", "out", (SZ, 3))],
     ((3,), F32, [1.0, 2.0, 3.0]), {"cpt_math_batch": {4: np.array([1, 2, 3], dtype=np.float32).tobytes()}}),
]


@pytest.mark.parametrize("call,calls,ret,outs", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_method_reaches_its_entry(call, calls, ret, outs):
    r = make(outs)
    got = call(r)
    assert r._L.calls == calls
    assert desc(got) == ret


def test_every_public_method_is_driven():
    """A method added to Renderer without a case here fails this test."""
    driven = {c[0] for c in CASES} | {"render", "set_frame", "close", "GATHER_MODES"}
    public = [n for n in vars(Renderer) if not n.startswith("_")]
    assert [n for n in public if not any(d == n or d.startswith(n + "_") for d in driven)] == []


RENDER_FLAGS = [
    ({}, 0), ({"path": "megakernel"}, 0), ({"path": "wavefront"}, 0x100), ({"ordered": False}, 0), ({"ordered": True}, 0x200),
    ({"ordered": "plain"}, 0x600), ({"schedule": "tiles"}, 0), ({"schedule": "cost"}, 0x800), ({"schedule": "previous"}, 0x4000),
    ({"consolidate": None}, 0), ({"consolidate": True}, 0x1000), ({"consolidate": False}, 0x2000), ({"accumulate": True}, 0x1),
    ({"aux": True}, 0x2), ({"stats": True}, 0x4), ({"sync": True}, 0x8), ({"flags": 0x200}, 0x200),
    ({"flags": 0x200, "aux": True, "schedule": "previous", "consolidate": False, "path": "wavefront"}, 0x6302),
]


@pytest.mark.parametrize("kwargs,flags", RENDER_FLAGS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) or "defaults"
                                                             for kw, _ in RENDER_FLAGS])
def test_render_flags(kwargs, flags):
    r = make()
    assert r.render(CAM, 1, 8, **kwargs) is None
    assert r._L.calls == [("cpt_render", "ctx", "cam", (I, 1), (I, 8), (U32, flags))]


def test_set_frame():
    r = make()
    assert r.set_frame(8, 6) is None
    assert r._L.calls == [("cpt_set_frame", "ctx", (I, 8), (I, 6), None, (I, 0))]
    assert (r.width, r.height, r.n_rows, r.npix) == (8, 6, 6, 48)
    assert desc(r.rows) == ((6,), I32, [0, 1, 2, 3, 4, 5])
    r = make()
    r.set_frame(W, H, rows=[0, 2])
    assert r._L.calls == [("cpt_set_frame", "ctx", (I, W), (I, H), "rows", (I, 2))]
    assert (r.width, r.height, r.n_rows, r.npix) == (W, H, 2, 8)
    assert desc(r.rows) == ((2,), I32, [0, 2])


@pytest.mark.parametrize("who", ["denoise_mix", "denoise_mix_history"])
def test_display_into_a_given_frame(who):
    r = make()
    call = (lambda **kw: r.denoise_mix(3, **kw)) if who == "denoise_mix" else r.denoise_mix_history
    head = ("cpt_denoise_mix", "ctx", (U32, 3)) if who == "denoise_mix" else ("cpt_denoise_mix_history", "ctx")
    buf = np.zeros(H * W * 4, dtype=np.uint8)   # any shape of the frame's size
    assert call(out=buf) is buf
    assert r._L.calls == [head + ("out",)]
    ro = np.zeros((H, W, 4), dtype=np.uint8)
    ro.flags.writeable = False
    for bad, text in ((np.zeros((H, W, 4), dtype=np.float32), f"{who}: `out` must be a numpy uint8 array"),
                      ([0] * 48, f"{who}: `out` must be a numpy uint8 array"),
                      (np.zeros((H, W, 3), dtype=np.uint8), f"{who}: `out` holds 36 bytes, the frame needs 48"),
                      (np.zeros((H, W, 8), dtype=np.uint8)[:, :, ::2], f"{who}: `out` must be C-contiguous and writeable"),
                      (ro, f"{who}: `out` must be C-contiguous and writeable")):
        with pytest.raises(ValueError) as e:
            call(out=bad)
        assert str(e.value) == text
    assert len(r._L.calls) == 1   # a refused frame reaches no entry
    assert call(out=buf, host=False) is None
    assert r._L.calls[1] == head + (None,)


def test_value_errors():
    r = make()
    for call, text in (
            (lambda: r.render(CAM, 1, 8, path="mega"), "path must be one of ('megakernel', 'wavefront')"),
            (lambda: r.render(CAM, 1, 8, schedule="auto"), "schedule must be 'tiles', 'cost' or 'previous'"),
            (lambda: r.update_objects([0, 1, 2], OBJS), "update_objects: 2 objects for 3 indices"),
            (lambda: r.update_objects([[0, 1]], OBJS), "update_objects: 2 objects for 2 indices"),
            (lambda: r.write_moments(MOM[:3]), "write_moments: expected shape (4, 12), got (3, 12)"),
            (lambda: r.write_rng(RNG[:5]), "write_rng: expected shape (6, 12), got (5, 12)"),
            (lambda: r.write_gbuffer(id=GID[:5]), "write_gbuffer: id of 5 values, expected shape (12,)"),
            (lambda: r.write_gbuffer(normal=NRM[:, :2]), "write_gbuffer: normal of 24 values, expected shape (12, 3)"),
            (lambda: r.trace_rays(ORG, DIRS[:2]), "trace_rays: 3 origins for 2 directions"),
            (lambda: r.trace_rays(ORG, DIRS, tmin=TMIN[:2]), "trace_rays: 2 tmin values for 3 rays"),
            (lambda: renderer.object_motion_host(OBJS, OBJS[:1]), "object_motion_host: 2 old objects for 1 new ones")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    assert r._L.calls == []


def test_lifecycle(monkeypatch):
    stub = Stub({"cpt_create": {1: ctypes.c_void_p(CTX)}})
    monkeypatch.setattr(_lib, "load", lambda *a, **k: stub)
    with Renderer(1) as r:
        assert (r._L, r._ctx.value, r.device, r.width, r.height, r.n_rows, r.rows) == (stub, CTX, 1, 0, 0, 0, None)
        assert stub.calls == [("cpt_create", (I, 1), "out")]
    assert r._ctx is None and stub.calls[1:] == [("cpt_destroy", "ctx")]
    r.close()
    del r
    assert len(stub.calls) == 2   # destroyed once
    assert inspect.signature(Renderer.__init__).parameters["device"].default == 0


def test_errors_carry_the_status_and_the_library_text(monkeypatch):
    """A failed entry raises CptError with its status and cpt_last_error's text for the context
    (for cpt_create: for no context), or the status' own string when that text is empty."""
    stub = Stub(returns={"cpt_create": 2, "cpt_render": 5, "cpt_synchronize": 7, "cpt_last_error": b"the library's text",
                         "cpt_status_string": b"the status' string"})
    monkeypatch.setattr(_lib, "load", lambda *a, **k: stub)
    with pytest.raises(_lib.CptError) as e:
        Renderer(0)
    assert (e.value.status, str(e.value)) == (2, "[cpt status 2] the library's text")
    assert stub.calls == [("cpt_create", (I, 0), "out"), ("cpt_last_error", None)]
    r = make()
    r._L = stub
    del stub.calls[:]
    with pytest.raises(_lib.CptError) as e:
        r.render(CAM, 1, 8)
    assert (e.value.status, str(e.value)) == (5, "[cpt status 5] the library's text")
    assert [c[:2] for c in stub.calls] == [("cpt_render", "ctx"), ("cpt_last_error", "ctx")]
    stub.returns["cpt_last_error"] = b""
    with pytest.raises(_lib.CptError) as e:
        r.synchronize()
    assert (e.value.status, str(e.value)) == (7, "[cpt status 7] the status' string")
    assert stub.calls[-1] == ("cpt_status_string", (I, 7))


# ---- the module's host functions, against the same stub -----------------------------------------
_PLANES = ("cam", "cam2", (I, W), (I, H), "dir0", "dir1", "id0", "t0", "id", "depth", "normal")
_TAIL = ((I, 32), f(1e-2))
_GEOM = (CAM, CAM2, DIR0.astype(np.float64), DIR1.reshape(H, W, 3), ID0.astype(np.int64), T0, GID, DEP.reshape(H, W), NRM)
HOST_CASES = [
    ("device_count", lambda: renderer.device_count(), [("cpt_get_device_count", "out")], ("int", 2),
     {"cpt_get_device_count": {0: I(2)}}),
    ("camera_get_copy", lambda: renderer.camera_get_copy(CAM), [("cpt_camera_get_copy", "cam")], ((), CAMERA_DTYPE), None),
    ("topup_deficit_host", lambda: renderer.topup_deficit_host(3.0, 8), [("cpt_topup_deficit_host", f(3.0), (I, 8), "out")],
     ("int", 5), {"cpt_topup_deficit_host": {2: I(5)}}),
    ("object_motion_host", lambda: renderer.object_motion_host(OBJS, OBJS_B),
     [("cpt_object_motion_host", "objs", "objs_b", (I, 2), "out")], ((2,), MOTION_DTYPE), None),
    ("object_motion_host_empty", lambda: renderer.object_motion_host(OBJS[:0], OBJS[:0]),
     [("cpt_object_motion_host", None, None, (I, 0), None)], ((0,), MOTION_DTYPE), None),
    ("reproject_host", lambda: renderer.reproject_host(*_GEOM, ACC),
     [("cpt_reproject_host",) + _PLANES + ("accum",) + _TAIL + ("out",)], ((NPIX, 4), F32), None),
    ("reproject_host_args", lambda: renderer.reproject_host(*_GEOM, ACC, max_history=8, plane_tol=0.5),
     [("cpt_reproject_host",) + _PLANES + ("accum", (I, 8), f(0.5), "out")], ((NPIX, 4), F32), None),
    ("reproject_display_host", lambda: renderer.reproject_display_host(*_GEOM, MEAN, CNT),
     [("cpt_reproject_display_host",) + _PLANES + ("mean", "count") + _TAIL + ("out", "out")],
     (((NPIX, 3), F32), ((NPIX,), F32)), None),
    ("reproject_tracked_host", lambda: renderer.reproject_tracked_host(*_GEOM, ACC, MOTION),
     [("cpt_reproject_tracked_host",) + _PLANES + ("accum", "motion", (I, 2)) + _TAIL + ("out",)], ((NPIX, 4), F32), None),
    ("reproject_tracked_host_none", lambda: renderer.reproject_tracked_host(*_GEOM, ACC, None, 8, 0.5),
     [("cpt_reproject_tracked_host",) + _PLANES + ("accum", None, (I, 0), (I, 8), f(0.5), "out")], ((NPIX, 4), F32), None),
    ("reproject_tracked_host_empty", lambda: renderer.reproject_tracked_host(*_GEOM, ACC, MOTION[:0]),
     [("cpt_reproject_tracked_host",) + _PLANES + ("accum", None, (I, 0)) + _TAIL + ("out",)], ((NPIX, 4), F32), None),
    ("reproject_display_tracked_host", lambda: renderer.reproject_display_tracked_host(*_GEOM, MEAN, CNT, MOTION),
     [("cpt_reproject_display_tracked_host",) + _PLANES + ("mean", "count", "motion", (I, 2)) + _TAIL + ("out", "out")],
     (((NPIX, 3), F32), ((NPIX,), F32)), None),
    ("reproject_display_tracked_host_empty", lambda: renderer.reproject_display_tracked_host(*_GEOM, MEAN, CNT, [], 8, 0.5),
     [("cpt_reproject_display_tracked_host",) + _PLANES + ("mean", "count", None, (I, 0), (I, 8), f(0.5), "out", "out")],
     (((NPIX, 3), F32), ((NPIX,), F32)), None),
]


@pytest.mark.parametrize("call,calls,ret,outs", [c[1:] for c in HOST_CASES], ids=[c[0] for c in HOST_CASES])
def test_host_function_reaches_its_entry(monkeypatch, call, calls, ret, outs):
    stub = Stub(outs)
    monkeypatch.setattr(_lib, "load", lambda *a, **k: stub)
    got = call()
    assert stub.calls == calls
    assert desc(got) == ret


# ---- the public surface ---------------------------------------------------------------------------
_HOST_ARGS = "cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1, "
_REPROJECT = "max_history=32, plane_tol=0.01"
SIGNATURES = {
    "device_count": "() -> int",
    "camera_get_copy": "(cam)",
    "topup_deficit_host": "(count, target)",
    "reproject_host": f"({_HOST_ARGS}accum, {_REPROJECT})",
    "reproject_display_host": f"({_HOST_ARGS}mean, count, {_REPROJECT})",
    "object_motion_host": "(old_objs, new_objs)",
    "reproject_tracked_host": f"({_HOST_ARGS}accum, motion, {_REPROJECT})",
    "reproject_display_tracked_host": f"({_HOST_ARGS}mean, count, motion, {_REPROJECT})",
    "Renderer.__init__": "(self, device: int = 0)",
    "Renderer.close": "(self)",
    "Renderer.__enter__": "(self)",
    "Renderer.__exit__": "(self, *exc)",
    "Renderer._check": "(self, st)",
    "Renderer.set_stream": "(self, hip_stream_handle)",
    "Renderer.set_scene": "(self, objs)",
    "Renderer.update_object": "(self, index, obj)",
    "Renderer.update_objects": "(self, indices, objs, rebuild=False)",
    "Renderer.material_count": "(self) -> int",
    "Renderer.last_update_ms": "(self) -> float",
    "Renderer.bvh_export": "(self)",
    "Renderer.set_env": "(self, env)",
    "Renderer.bind_texture": "(self, handle, tex, address_mode=2, filter_mode=1)",
    "Renderer.set_frame": "(self, width, height, rows=None)",
    "Renderer.init_rng": "(self, seed)",
    "Renderer.render": "(self, cam, spp, max_depth, accumulate=False, aux=False, stats=False, sync=False, flags=0, "
                       "path='megakernel', ordered=False, schedule='tiles', consolidate=None)",
    "Renderer.render_to_count": "(self, cam, target, max_depth, aux=False, stats=False, sync=False, flags=0)",
    "Renderer.topup_info": "(self)",
    "Renderer.render_adaptive": "(self, cam, min_spp, max_spp, batch, rel_error, max_depth, flags=0)",
    "Renderer.adaptive_info": "(self)",
    "Renderer.adaptive_begin": "(self, cam, min_spp, max_spp, batch, rel_error, max_depth, flags=0)",
    "Renderer.adaptive_step": "(self) -> int",
    "Renderer.read_noise": "(self)",
    "Renderer.read_moments": "(self)",
    "Renderer.write_moments": "(self, planar4)",
    "Renderer.filter_frame": "(self, levels=5, sigma_l=1.0, normal_sharpness_log2=7)",
    "Renderer.filter_frame_spatial": "(self, levels=3, sigma_l=2.0, normal_sharpness_log2=3)",
    "Renderer.read_filtered": "(self)",
    "Renderer.last_filter_ms": "(self) -> float",
    "Renderer.gbuffer": "(self, cam, flags=0)",
    "Renderer.read_gbuffer": "(self)",
    "Renderer.write_gbuffer": "(self, id=None, t=None, normal=None, albedo=None)",
    "Renderer.trace_rays": "(self, origins, dirs, tmin=None, flags=0)",
    "Renderer.pick": "(self, cam, x, y, flags=0)",
    "Renderer.last_query_ms": "(self) -> float",
    "Renderer.reproject_accum": f"(self, cam_from, cam_to, {_REPROJECT}, flags=0)",
    "Renderer.reproject_display": f"(self, cam_from, cam_to, {_REPROJECT}, flags=0)",
    "Renderer.history_capture": "(self, cam, flags=0)",
    "Renderer.history_info": "(self)",
    "Renderer.reproject_accum_tracked": f"(self, cam_to, {_REPROJECT}, flags=0)",
    "Renderer.reproject_display_tracked": f"(self, cam_to, {_REPROJECT}, flags=0)",
    "Renderer.last_reproject_ms": "(self, split=False)",
    "Renderer.tile_costs": "(self, cam, passes, max_depth, ordered=True)",
    "Renderer.synchronize": "(self)",
    "Renderer.last_render_ms": "(self) -> float",
    "Renderer.last_kernel_stats": "(self)",
    "Renderer.read_accum": "(self)",
    "Renderer.clear_accum": "(self)",
    "Renderer.read_rng": "(self)",
    "Renderer.write_rng": "(self, planar6)",
    "Renderer.read_aux": "(self)",
    "Renderer.write_accum": "(self, rgba)",
    "Renderer.write_aux": "(self, normal3, depth)",
    "Renderer.copy_accum_device": "(self, device_ptr, nbytes, stream)",
    "Renderer.gather_rows": "(self, src)",
    "Renderer.last_gather_mode": "(self, src)",
    "Renderer.set_debug_gather": "(self, force_staged)",
    "Renderer.stats": "(self)",
    "Renderer.raw_counters": "(self)",
    "Renderer.debug_timeline": "(self)",
    "Renderer.diag_counters": "(self)",
    "Renderer.execdiag_counters": "(self)",
    "Renderer.walk_info": "(self)",
    "Renderer.read_nodes": "(self)",
    "Renderer.debug_tile_order": "(self, which)",
    "Renderer.measure_read_pattern": "(self, bytes_per_lane, nbytes=1073741824, iters=1)",
    "Renderer.measure_read_bandwidth": "(self, nbytes=4294967296, iters=10)",
    "Renderer.set_debug_consolidation": "(self, flags=0, keeper_spin_log2=0, publish_wait_log2=0)",
    "Renderer.set_debug_grid": "(self, max_workgroups=0, lanes_per_wave=0)",
    "Renderer.reset_stats": "(self)",
    "Renderer.selftest_qdiv": "(self, which, n, seed=1, examples=16)",
    "Renderer.denoise_mix": "(self, cur_sample_idx, out=None, host=True)",
    "Renderer.denoise_mix_history": "(self, out=None, host=True)",
    "Renderer.read_display_count": "(self)",
    "Renderer.display_band": "(self)",
    "Renderer.read_mix": "(self)",
    "Renderer.last_display_ms": "(self) -> float",
    "Renderer.denoise_mix_band": "(self, cur_sample_idx, y0, y1, host=True)",
    "Renderer.copy_bgra_device": "(self, device_ptr, nbytes, stream)",
    "Renderer.reset_display": "(self)",
    "Renderer.math_batch": "(self, op, a, b=None)",
}


def test_public_signatures():
    got = {n: str(inspect.signature(v)) for n, v in vars(renderer).items()
           if inspect.isfunction(v) and v.__module__ == renderer.__name__ and not n.startswith("_")}
    got.update({f"Renderer.{n}": str(inspect.signature(v)) for n, v in vars(Renderer).items()
                if inspect.isfunction(v) and (not n.startswith("_") or n in ("__init__", "__enter__", "__exit__", "_check"))})
    assert got == SIGNATURES
    assert isinstance(vars(Renderer)["npix"], property)
    assert Renderer.GATHER_MODES == {-1: None, 0: "same_device", 1: "peer", 2: "staged"}
    assert renderer.PATHS == ("megakernel", "wavefront")
