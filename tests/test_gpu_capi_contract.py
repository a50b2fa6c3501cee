"""The C ABI's statuses and cpt_last_error texts, pinned step by step (tests/golden/capi_contract.json).

The table drives libcpt.so through _lib.load(), not Renderer, so the binding's own validation never
runs first.  Five groups, each on fresh contexts: a new context; a frame only; scene, frame and RNG;
a frame of rows 4..11 of 16; an adaptive render pending.  Within a group every entry is issued with
its smallest valid arguments and once per invalid argument: a NULL context, a NULL pointer (only
where the entry checks it before it is read), a capacity one short, max_depth 33, a stray flag bit,
a camera of another size, a band outside [0, H').  16 x 16 frames, scene s3, 1 pass of depth 1.

A step records [group, entry, what, status, text].  text is cpt_last_error of the context the entry
reports on (NULL for the entries without one) after a status other than CPT_OK, and "" after
CPT_OK; an entry that returns a status without a message therefore records the message before it,
which pins that it wrote none.  No step ends in a HIP status: that text embeds a source line.
The one machine-dependent text, cpt_create's "device -1 of N", is recorded with N replaced.

`python tests/test_gpu_capi_contract.py --record` writes the fixture from the library in the tree
(or CPT_LIB_PATH's)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "capi_contract.json")

pytestmark = pytest.mark.gpu

W = H = 16
NPIX = W * H
TILES = 4
WAVEFRONT, ORDERED, COST, CONSOLIDATE, PREVIOUS = 0x100, 0x200, 0x800, 0x1000, 0x4000
ACCUMULATE, AUX, SYNC = 0x1, 0x2, 0x8
STRAY = 0x1   # CPT_RENDER_ACCUMULATE: no CPT_TRAVERSAL_* bit
HIP_STATUSES = (3, 4)   # CPT_ERR_HIP, CPT_ERR_OUT_OF_MEMORY


def _p(a):
    return a.ctypes.data


class Table:
    """The library, the shared host buffers and the recorded steps."""

    def __init__(self):
        import torch   # one HIP runtime per process: torch's

        from cpppathtracer_amd import _lib, scenes
        from cpppathtracer_amd.types import CAMERA_DTYPE, OBJECT_DTYPE
        self.L = L = _lib.load()
        self.steps = []
        self.group = ""
        n = ctypes.c_int(0)
        assert L.cpt_get_device_count(ctypes.byref(n)) == 0 and n.value >= 1
        self.n_devices = n.value
        self.objs = np.ascontiguousarray(scenes.scene_s3(), dtype=OBJECT_DTYPE)

        def camera(w, h):
            cam = np.array(scenes.camera_for(w, h), dtype=CAMERA_DTYPE, copy=True)
            assert L.cpt_camera_get_copy(_p(cam)) == 0
            return cam
        self.cam, self.cam8, self.cam1 = camera(W, H), camera(8, 8), camera(1, 1)
        # host buffers, each larger than anything a 16 x 16 frame reads or writes
        self.f = [np.zeros(8 * NPIX, dtype=np.float32) for _ in range(4)]
        self.u32 = np.zeros(8 * NPIX, dtype=np.uint32)
        self.i32 = np.zeros(8 * NPIX, dtype=np.int32)
        self.u8 = np.zeros(8 * NPIX, dtype=np.uint8)
        self.u64 = np.zeros(128, dtype=np.uint64)
        self.nodes = np.zeros(1 << 16, dtype=np.uint8)
        # one ray from the camera towards the scene: origin at float 0, direction at float 16
        self.rays = np.zeros(32, dtype=np.float32)
        self.rays[0:3] = scenes.CAMERA_ORIGIN
        self.rays[16:19] = -np.asarray(scenes.CAMERA_ORIGIN, dtype=np.float32) / np.float32(np.linalg.norm(scenes.CAMERA_ORIGIN))
        self.dev = torch.zeros(8 * NPIX, dtype=torch.uint8, device="cuda:0")
        self.i, self.j = ctypes.c_int(0), ctypes.c_int(0)
        self.sz = ctypes.c_size_t(0)
        self.fl = ctypes.c_float(1.0)
        self.q = ctypes.c_uint64(0)
        self.q2 = ctypes.c_uint64(0)
        self.w32 = ctypes.c_uint32(0)

    def __call__(self, entry, what, *args, on="first"):
        """Issue `entry(*args)` and record it; `on`: the context whose message the entry sets."""
        ctx = args[0] if on == "first" else on
        status = getattr(self.L, entry)(*args)
        assert status not in HIP_STATUSES, (entry, what, self.L.cpt_last_error(ctx))
        text = "" if status == 0 else (self.L.cpt_last_error(ctx) or b"").decode()
        text = text.replace(f"device -1 of {self.n_devices}", "device -1 of <device count>")
        self.steps.append([self.group, entry, what, status, text])
        return status

    def ok(self, entry, *args):
        """A set-up call: recorded like any other, and it must succeed."""
        assert self(entry, "valid", *args) == 0, (entry, self.steps[-1])

    def create(self):
        out = ctypes.c_void_p()
        assert self.L.cpt_create(0, ctypes.byref(out)) == 0
        return out.value

    def frame(self, c, rows=None, scene=True, rng=True):
        if scene:
            self.ok("cpt_set_scene", c, _p(self.objs), len(self.objs))
        if rows is None:
            self.ok("cpt_set_frame", c, W, H, None, 0)
        else:
            r = np.asarray(rows, dtype=np.int32)
            self.ok("cpt_set_frame", c, W, H, _p(r), len(r))
        if rng:
            self.ok("cpt_init_rng", c, 1234)


def _null_context(t):
    """Every entry that takes a context, with a NULL one (each checks it first)."""
    f, u32, i32, u8, u64, cam = _p(t.f[0]), _p(t.u32), _p(t.i32), _p(t.u8), _p(t.u64), _p(t.cam)
    i, sz, fl, q = ctypes.byref(t.i), ctypes.byref(t.sz), ctypes.byref(t.fl), ctypes.byref(t.q)
    for entry, args in [
        ("cpt_set_stream", (None,)), ("cpt_set_scene", (f, 1)), ("cpt_set_frame", (W, H, None, 0)), ("cpt_init_rng", (1,)),
        ("cpt_read_rng", (u32,)), ("cpt_write_rng", (u32,)), ("cpt_render", (cam, 1, 1, 0)),
        ("cpt_render_to_count", (cam, 1, 1, 0)), ("cpt_topup_info", (None, None, None)), ("cpt_synchronize", ()),
        ("cpt_read_accum", (f,)), ("cpt_clear_accum", ()), ("cpt_read_aux", (f, f)), ("cpt_write_accum", (f,)),
        ("cpt_write_aux", (f, f)), ("cpt_copy_accum_device", (f, 0, None)), ("cpt_set_debug_gather", (0,)),
        ("cpt_get_stats", (u64,)), ("cpt_reset_stats", ()), ("cpt_get_raw_counters", (u64,)), ("cpt_get_walk_info", (i32,)),
        ("cpt_debug_read_nodes", (None, 0, sz)), ("cpt_debug_read_tile_order", (0, u32, 64, sz)),
        ("cpt_measure_read_bandwidth", (16, 1, fl)), ("cpt_measure_read_pattern", (4, 64, 1, fl)),
        ("cpt_last_render_ms", (fl,)), ("cpt_get_diag_counters", (u64,)), ("cpt_get_execdiag_counters", (u64,)),
        ("cpt_last_kernel_stats", (fl, i)), ("cpt_denoise_mix", (1, None)), ("cpt_denoise_mix_band", (1, 0, 16, None)),
        ("cpt_copy_bgra_device", (f, 0, None)), ("cpt_last_display_ms", (fl,)), ("cpt_reset_display", ()),
        ("cpt_display_band", (i, i)), ("cpt_debug_timeline", (u64, 1)), ("cpt_tile_costs", (cam, 1, 1, 0, u32, 64)),
        ("cpt_read_mix", (f, 8 * NPIX)), ("cpt_math_batch", (7, f, f, f, 3)), ("cpt_selftest_qdiv", (2, 10, 1, u64, 3)),
        ("cpt_set_debug_consolidation", (0, 0, 0)), ("cpt_set_debug_grid", (0, 0)),
        ("cpt_render_adaptive", (cam, 1, 1, 1, 0.5, 1, 0)), ("cpt_adaptive_begin", (cam, 1, 1, 1, 0.5, 1, 0)),
        ("cpt_adaptive_step", (i,)), ("cpt_read_noise", (f, NPIX)), ("cpt_adaptive_info", (i, u32, 8, q)),
        ("cpt_read_moments", (f, 4 * NPIX)), ("cpt_write_moments", (f, 4 * NPIX)), ("cpt_filter_frame", (1, 1.0, 1)),
        ("cpt_read_filtered", (f, f, NPIX)), ("cpt_last_filter_ms", (fl,)), ("cpt_filter_frame_spatial", (1, 1.0, 1)),
        ("cpt_gbuffer", (cam, 0)), ("cpt_read_gbuffer", (i32, f, f, f, NPIX)), ("cpt_write_gbuffer", (i32, f, f, f, NPIX)),
        ("cpt_trace_rays", (0, None, None, None, 0, None, None, None)), ("cpt_pick", (cam, 0, 0, 0, i, fl)),
        ("cpt_last_query_ms", (fl,)), ("cpt_reproject_accum", (cam, cam, 1, 0.0, 0)), ("cpt_last_reproject_ms", (fl,)),
        ("cpt_last_reproject_launch_ms", (f,)), ("cpt_denoise_mix_history", (None,)), ("cpt_read_display_count", (f, NPIX)),
        ("cpt_reproject_display", (cam, cam, 1, 0.0, 0)), ("cpt_history_capture", (cam, 0)), ("cpt_history_info", (i, None)),
        ("cpt_reproject_accum_tracked", (cam, 1, 0.0, 0)), ("cpt_reproject_display_tracked", (cam, 1, 0.0, 0)),
        ("cpt_set_exposure", (1.0,)), ("cpt_meter_exposure", (0, 0.18, 500, 1.0)), ("cpt_read_exposure", (fl, u32)),
        ("cpt_present", (0, 0, 1.0, 0, None)), ("cpt_read_present", (u8, 4 * NPIX)), ("cpt_copy_present_device", (f, 0, None)),
        ("cpt_last_present_ms", (fl,)),
    ]:
        t(entry, "NULL context", None, *args)
    t("cpt_destroy", "NULL context", None)


def _host_hooks(t):
    """The entries without a context: a valid call and an invalid one each (they set no message)."""
    L = t.L
    f0, f1, f2, f3 = (_p(a) for a in t.f)
    i32, u8, cam1 = _p(t.i32), _p(t.u8), _p(t.cam1)
    i, fl, q = ctypes.byref(t.i), ctypes.byref(t.fl), ctypes.byref(t.q)
    none = {"on": None}
    assert L.cpt_abi_version() == 1
    for status in range(9):
        t.steps.append([t.group, "cpt_status_string", str(status), status, L.cpt_status_string(status).decode()])
    t("cpt_get_device_count", "valid", i, **none)
    t("cpt_get_device_count", "NULL count", None, **none)
    t("cpt_camera_get_copy", "NULL camera", None, **none)
    zero = t.cam.copy()
    zero["width"] = 0
    t("cpt_camera_get_copy", "width 0", _p(zero), **none)
    t("cpt_launch_grid_host", "valid", 1, 1, 64, 1, 64, 1, 0, i, q, **none)
    t("cpt_launch_grid_host", "NULL workgroups", 1, 1, 64, 1, 64, 1, 0, None, q, **none)
    t("cpt_launch_grid_host", "cus 0", 0, 1, 64, 1, 64, 1, 0, i, q, **none)
    t("cpt_adaptive_decide_host", "valid", 1.0, 1.0, 2.0, 0.1, i, fl, **none)
    t("cpt_adaptive_decide_host", "NULL converged", 1.0, 1.0, 2.0, 0.1, None, fl, **none)
    t("cpt_cap_disk_bound", "valid", 1.0, fl, **none)
    t("cpt_cap_disk_bound", "NULL out", 1.0, None, **none)
    t("cpt_topup_deficit_host", "valid", 0.0, 1, i, **none)
    t("cpt_topup_deficit_host", "NULL d", 0.0, 1, None, **none)
    t("cpt_topup_deficit_host", "target 0", 0.0, 0, i, **none)
    # the filter's hooks on a 2 x 2 frame (all buffers zero: every pixel invalid)
    t("cpt_filter_prepare_host", "valid", 4, f0, f1, f2, u8, **none)
    t("cpt_filter_prepare_host", "NULL accum", 4, None, f1, f2, u8, **none)
    t("cpt_filter_level_host", "valid", 2, 2, 1, f0, f1, u8, 1.0, 1, f2, **none)
    t("cpt_filter_level_host", "in == out", 2, 2, 1, f0, f1, u8, 1.0, 1, f0, **none)
    t("cpt_filter_level_host", "step 0", 2, 2, 0, f0, f1, u8, 1.0, 1, f2, **none)
    t("cpt_filter_prepare_spatial_host", "valid", 2, 2, f0, i32, f1, 1, f2, u8, **none)
    t("cpt_filter_prepare_spatial_host", "sharpness 11", 2, 2, f0, i32, f1, 11, f2, u8, **none)
    t("cpt_filter_level_id_host", "valid", 2, 2, 1, f0, f1, i32, u8, 1.0, 1, f2, **none)
    t("cpt_filter_level_id_host", "NULL id", 2, 2, 1, f0, f1, None, u8, 1.0, 1, f2, **none)
    # the reprojection's hooks: the argument checks alone (tests/test_reproject_model.py runs their loops)
    rp = (cam1, cam1, 1, 1, f0, f0, i32, f0, i32, f0, f0)
    t("cpt_reproject_host", "in == out", *rp, f1, 1, 0.0, f1, **none)
    t("cpt_reproject_host", "max_history 0", *rp, f1, 0, 0.0, f2, **none)
    t("cpt_reproject_display_host", "NULL count_out", *rp, f1, f2, 1, 0.0, f3, None, **none)
    t("cpt_object_motion_host", "valid", None, None, 0, None, **none)
    t("cpt_object_motion_host", "n -1", None, None, -1, None, **none)
    t("cpt_reproject_tracked_host", "a table of 0 records", *rp, f1, f3, 0, 1, 0.0, f2, **none)
    t("cpt_reproject_display_tracked_host", "camera of another size", _p(t.cam8), *rp[1:], f1, f2, None, 0, 1, 0.0, f3,
      f3 + 64, **none)
    t("cpt_present_host", "valid", 0, 0, None, 1.0, 0, 1.0, 0, None, **none)
    t("cpt_present_host", "source 2", 0, 2, None, 1.0, 0, 1.0, 0, None, **none)
    t("cpt_meter_host", "valid", 0, 0, None, 0.18, 500, 1.0, fl, None, **none)
    t("cpt_meter_host", "NULL exposure", 0, 0, None, 0.18, 500, 1.0, None, None, **none)
    t("cpt_present_srgb_thresholds_host", "valid", f0, **none)
    t("cpt_present_srgb_thresholds_host", "NULL t256", None, **none)
    t("cpt_host_register", "NULL buffer", None, 0, **none)
    t("cpt_host_unregister", "NULL buffer", None, **none)


def _renders_invalid(t, c):
    """The argument checks of the four render entries, which come before any look at the state."""
    cam = _p(t.cam)
    t("cpt_render", "NULL camera", c, None, 1, 1, 0)
    t("cpt_render", "spp -1", c, cam, -1, 1, 0)
    t("cpt_render", "max_depth 33", c, cam, 1, 33, 0)
    u32 = _p(t.u32)
    t("cpt_tile_costs", "passes 0", c, cam, 0, 1, 0, u32, 64)
    t("cpt_tile_costs", "max_depth 33", c, cam, 1, 33, 0, u32, 64)
    t("cpt_tile_costs", "NULL out", c, cam, 1, 1, 0, None, 64)
    for entry in ("cpt_adaptive_begin", "cpt_render_adaptive"):
        t(entry, "NULL camera", c, None, 1, 1, 1, 0.5, 1, 0)
        t(entry, "max_depth 33", c, cam, 1, 1, 1, 0.5, 33, 0)
        t(entry, "batch 0", c, cam, 1, 1, 0, 0.5, 1, 0)
        t(entry, "min_spp 1 < 2 batch, max_spp 2", c, cam, 1, 2, 1, 0.5, 1, 0)
        t(entry, "rel_error -1", c, cam, 1, 1, 1, -1.0, 1, 0)
        t(entry, "the wavefront path", c, cam, 1, 1, 1, 0.5, 1, WAVEFRONT)
        t(entry, "CPT_SCHEDULE_PREVIOUS", c, cam, 1, 1, 1, 0.5, 1, PREVIOUS)
    t("cpt_render_to_count", "NULL camera", c, None, 1, 1, 0)
    t("cpt_render_to_count", "target 0", c, cam, 0, 1, 0)
    t("cpt_render_to_count", "max_depth 33", c, cam, 1, 33, 0)
    t("cpt_render_to_count", "the wavefront path", c, cam, 1, 1, WAVEFRONT)
    t("cpt_render_to_count", "CPT_SCHEDULE_PREVIOUS", c, cam, 1, 1, PREVIOUS)
    t("cpt_render_to_count", "CPT_SCHEDULE_COST", c, cam, 1, 1, COST)
    t("cpt_render_to_count", "CPT_SCHEDULE_CONSOLIDATE", c, cam, 1, 1, CONSOLIDATE)


def _queries_invalid(t, c):
    """The argument checks of the queries, the reprojection, the filter and presenting."""
    cam, f, i32 = _p(t.cam), _p(t.f[0]), _p(t.i32)
    i, fl = ctypes.byref(t.i), ctypes.byref(t.fl)
    t("cpt_gbuffer", "NULL camera", c, None, 0)
    t("cpt_gbuffer", "a stray flag bit", c, cam, STRAY)
    t("cpt_trace_rays", "a stray flag bit", c, 1, f, f, None, STRAY, i32, f, f)
    t("cpt_trace_rays", "2^30 + 1 rays", c, (1 << 30) + 1, None, None, None, 0, None, None, None)
    t("cpt_trace_rays", "NULL origin3", c, 1, None, f, None, 0, i32, f, f)
    t("cpt_pick", "NULL object", c, cam, 0, 0, 0, None, fl)
    t("cpt_pick", "a stray flag bit", c, cam, 0, 0, STRAY, i, fl)
    for entry in ("cpt_reproject_accum", "cpt_reproject_display"):
        t(entry, "NULL from", c, None, cam, 1, 0.0, 0)
        t(entry, "a stray flag bit", c, cam, cam, 1, 0.0, STRAY)
        t(entry, "max_history 0", c, cam, cam, 0, 0.0, 0)
        t(entry, "plane_tol -1", c, cam, cam, 1, -1.0, 0)
    for entry in ("cpt_reproject_accum_tracked", "cpt_reproject_display_tracked"):
        t(entry, "NULL to", c, None, 1, 0.0, 0)
        t(entry, "a stray flag bit", c, cam, 1, 0.0, STRAY)
        t(entry, "max_history 0", c, cam, 0, 0.0, 0)
    t("cpt_history_capture", "NULL camera", c, None, 0)
    t("cpt_history_capture", "a stray flag bit", c, cam, STRAY)
    for entry in ("cpt_filter_frame", "cpt_filter_frame_spatial"):
        t(entry, "levels 9", c, 9, 1.0, 1)
        t(entry, "sigma_l -1", c, 1, -1.0, 1)
        t(entry, "normal_sharpness_log2 11", c, 1, 1.0, 11)
    t("cpt_set_exposure", "exposure 0", c, 0.0)
    t("cpt_meter_exposure", "source 2", c, 2, 0.18, 500, 1.0)
    t("cpt_meter_exposure", "permille 1001", c, 0, 0.18, 1001, 1.0)
    t("cpt_present", "tone 3", c, 0, 3, 1.0, 0, None)
    t("cpt_present", "white 0", c, 0, 0, 0.0, 0, None)


def _every_entry(t, c):
    """Every entry on a context with its smallest valid arguments, in one fixed order: what each
    makes of the context's state (a frame-only group runs it once more after filling the state)."""
    f0, f1, f2 = (_p(a) for a in t.f[:3])
    u32, i32, u8, u64, cam, dev = _p(t.u32), _p(t.i32), _p(t.u8), _p(t.u64), _p(t.cam), t.dev.data_ptr()
    i, j, sz, fl, q, q2, w32 = (ctypes.byref(x) for x in (t.i, t.j, t.sz, t.fl, t.q, t.q2, t.w32))
    t("cpt_synchronize", "valid", c)
    t("cpt_read_rng", "valid", c, u32)
    t("cpt_read_accum", "valid", c, f0)
    t("cpt_clear_accum", "valid", c)
    t("cpt_read_aux", "valid", c, f0, f1)
    t("cpt_copy_accum_device", "one float4 too many", c, dev, (t.npix + 1) * 16, None)
    t("cpt_get_stats", "valid", c, u64)
    t("cpt_get_raw_counters", "valid", c, u64)
    t("cpt_get_diag_counters", "valid", c, u64)
    t("cpt_get_execdiag_counters", "valid", c, u64)
    t("cpt_get_walk_info", "valid", c, i32)
    t("cpt_reset_stats", "valid", c)
    t("cpt_render", "valid", c, cam, 1, 1, SYNC)
    t("cpt_tile_costs", "valid", c, cam, 1, 1, 0, u32, 64)
    t("cpt_last_render_ms", "valid", c, fl)
    t("cpt_last_kernel_stats", "valid", c, fl, i)
    t("cpt_render_to_count", "valid", c, cam, 2, 1, SYNC)
    t("cpt_topup_info", "valid", c, w32, q, q2)
    t("cpt_render_adaptive", "valid", c, cam, 1, 1, 1, 0.5, 1, 0)
    t("cpt_adaptive_step", "valid", c, i)
    t("cpt_read_noise", "valid", c, f0, 8 * NPIX)
    t("cpt_adaptive_info", "valid", c, i, u32, 8, q)
    t("cpt_read_moments", "valid", c, f0, 8 * NPIX)
    t("cpt_gbuffer", "valid", c, cam, 0)
    t("cpt_read_gbuffer", "valid", c, i32, f0, f1, f2, 8 * NPIX)
    t("cpt_filter_frame", "valid", c, 1, 1.0, 1)
    t("cpt_filter_frame_spatial", "valid", c, 1, 1.0, 1)
    t("cpt_read_filtered", "valid", c, f0, f1, 8 * NPIX)
    t("cpt_last_filter_ms", "valid", c, fl)
    t("cpt_trace_rays", "valid", c, 1, _p(t.rays), _p(t.rays) + 64, None, 0, i32, f0, f1)
    t("cpt_pick", "valid", c, cam, 0, 0, 0, i, fl)
    t("cpt_last_query_ms", "valid", c, fl)
    t("cpt_reproject_accum_tracked", "valid", c, cam, 1, 0.0, 0)
    t("cpt_history_capture", "valid", c, cam, 0)
    t("cpt_history_info", "valid", c, i, None)
    t("cpt_reproject_accum", "valid", c, cam, cam, 1, 0.0, 0)
    t("cpt_last_reproject_ms", "valid", c, fl)
    t("cpt_last_reproject_launch_ms", "valid", c, f0)
    t("cpt_denoise_mix", "valid", c, 1, u8)
    t("cpt_denoise_mix_history", "valid", c, u8)
    t("cpt_display_band", "valid", c, i, j)
    t("cpt_read_mix", "valid", c, f0, 8 * NPIX)
    t("cpt_read_display_count", "valid", c, f0, 8 * NPIX)
    t("cpt_copy_bgra_device", "valid", c, dev, 4, None)
    t("cpt_last_display_ms", "valid", c, fl)
    t("cpt_reproject_display", "valid", c, cam, cam, 1, 0.0, 0)
    t("cpt_reproject_display_tracked", "valid", c, cam, 1, 0.0, 0)
    t("cpt_reset_display", "valid", c)
    t("cpt_set_exposure", "valid", c, 1.0)
    t("cpt_meter_exposure", "valid", c, 0, 0.18, 500, 1.0)
    t("cpt_meter_exposure", "the filtered source", c, 1, 0.18, 500, 1.0)
    t("cpt_read_exposure", "valid", c, fl, u32)
    t("cpt_read_present", "valid", c, u8, 8 * NPIX)
    t("cpt_copy_present_device", "valid", c, dev, 4, None)
    t("cpt_present", "valid", c, 0, 0, 1.0, 0, u8)
    t("cpt_present", "the filtered source", c, 1, 0, 1.0, 0, None)
    t("cpt_last_present_ms", "valid", c, fl)
    t("cpt_debug_timeline", "valid", c, u64, 1)
    t("cpt_debug_read_nodes", "the size alone", c, None, 0, sz)
    for which in (0, 1, 4, 2):
        t("cpt_debug_read_tile_order", f"which {which}", c, which, u32, 64, sz)


def _group_new_context(t):
    t.group = "new context"
    out = ctypes.c_void_p()
    t.npix = 0
    f0, u32, i32, u64 = _p(t.f[0]), _p(t.u32), _p(t.i32), _p(t.u64)
    i, sz, fl = ctypes.byref(t.i), ctypes.byref(t.sz), ctypes.byref(t.fl)
    # first, so that the message of the entries without a context is this one from here on
    t("cpt_create", "NULL out", 0, None, on=None)
    t("cpt_create", "device -1", -1, ctypes.byref(out), on=None)
    _host_hooks(t)
    _null_context(t)
    c, c2 = t.create(), t.create()
    t("cpt_set_stream", "valid", c, None)
    t("cpt_init_rng", "valid", c, 1)
    _every_entry(t, c)
    _renders_invalid(t, c)
    _queries_invalid(t, c)
    # NULL pointers and the arguments each entry checks before the state
    t("cpt_set_frame", "width 0", c, 0, H, None, 0)
    t("cpt_set_frame", "65536 pixels wide", c, 65536, H, None, 0)
    rows = np.array([0, 16], dtype=np.int32)
    t("cpt_set_frame", "n_rows -1", c, W, H, _p(rows), -1)
    t("cpt_set_frame", "row 16", c, W, H, _p(rows), 2)
    t("cpt_read_rng", "NULL planar6", c, None)
    t("cpt_write_rng", "valid", c, u32)
    t("cpt_write_rng", "NULL planar6", c, None)
    t("cpt_read_accum", "NULL rgba", c, None)
    t("cpt_write_accum", "valid", c, f0)
    t("cpt_write_accum", "NULL rgba", c, None)
    t("cpt_write_aux", "valid", c, f0, f0)
    t("cpt_write_aux", "NULL depth", c, f0, None)
    t("cpt_copy_accum_device", "NULL dst", c, None, 16, None)
    t("cpt_get_stats", "NULL out", c, None)
    t("cpt_get_raw_counters", "NULL out8", c, None)
    t("cpt_get_diag_counters", "NULL out16", c, None)
    t("cpt_get_execdiag_counters", "NULL out64", c, None)
    t("cpt_get_walk_info", "NULL out4", c, None)
    t("cpt_set_debug_consolidation", "valid", c, 0, 0, 0)
    t("cpt_set_debug_consolidation", "flags 4", c, 4, 0, 0)
    t("cpt_set_debug_consolidation", "keeper_spin_log2 31", c, 0, 31, 0)
    t("cpt_set_debug_consolidation", "publish_wait_log2 -1", c, 0, 0, -1)
    t("cpt_set_debug_grid", "valid", c, 0, 0)
    t("cpt_set_debug_grid", "max_workgroups -1", c, -1, 0)
    t("cpt_set_debug_grid", "lanes_per_wave 65", c, 0, 65)
    t("cpt_set_debug_gather", "valid", c, 0)
    t("cpt_last_render_ms", "NULL ms", c, None)
    t("cpt_last_kernel_stats", "NULL launches", c, fl, None)
    t("cpt_adaptive_step", "NULL active_tiles", c, None)
    t("cpt_read_noise", "NULL rel", c, None, NPIX)
    t("cpt_adaptive_info", "capacity -1", c, i, u32, -1, None)
    t("cpt_adaptive_info", "NULL list of capacity 1", c, i, None, 1, None)
    t("cpt_read_moments", "NULL planar4", c, None, 4 * NPIX)
    t("cpt_write_moments", "valid", c, f0, 4 * NPIX)
    t("cpt_write_moments", "NULL planar4", c, None, 4 * NPIX)
    t("cpt_write_gbuffer", "valid", c, i32, f0, f0, f0, NPIX)
    t("cpt_history_info", "NULL valid", c, None, None)
    t("cpt_last_reproject_launch_ms", "NULL ms3", c, None)
    t("cpt_denoise_mix_band", "valid", c, 1, 0, 16, None)
    t("cpt_copy_bgra_device", "NULL dst", c, None, 4, None)
    t("cpt_display_band", "NULL y1", c, i, None)
    t("cpt_read_mix", "NULL rgb", c, None, NPIX)
    t("cpt_read_display_count", "NULL count", c, None, NPIX)
    t("cpt_read_present", "NULL bgra", c, None, 4 * NPIX)
    t("cpt_copy_present_device", "NULL dst", c, None, 4, None)
    t("cpt_debug_timeline", "n 0", c, u64, 0)
    t("cpt_debug_read_nodes", "NULL n_bytes", c, None, 0, None)
    t("cpt_debug_read_tile_order", "which 3", c, 3, u32, 64, sz)
    t("cpt_debug_read_tile_order", "NULL n", c, 0, u32, 64, None)
    t("cpt_math_batch", "valid", c, 7, f0, f0, _p(t.f[1]), 3)
    t("cpt_math_batch", "n 0", c, 7, f0, f0, _p(t.f[1]), 0)
    t("cpt_math_batch", "NULL b", c, 7, f0, None, _p(t.f[1]), 3)
    t("cpt_measure_read_bandwidth", "valid", c, 16, 1, fl)
    t("cpt_measure_read_bandwidth", "15 bytes", c, 15, 1, fl)
    t("cpt_measure_read_pattern", "valid", c, 4, 64, 1, fl)
    t("cpt_measure_read_pattern", "8 bytes per lane", c, 8, 64, 1, fl)
    t("cpt_selftest_qdiv", "valid", c, 2, 10, 1, u64, 3)
    t("cpt_selftest_qdiv", "which 19", c, 19, 10, 1, u64, 3)
    t("cpt_selftest_qdiv", "NULL out", c, 2, 10, 1, None, 3)
    t("cpt_gather_rows", "one context twice", c, c)
    t("cpt_gather_rows", "no frames", c, c2)
    t("cpt_gather_rows", "NULL src", c, None)
    t("cpt_last_gather_mode", "valid", c, c2, i)
    t("cpt_last_gather_mode", "NULL src", c, None, i)
    t("cpt_destroy", "valid", c2)
    t("cpt_destroy", "valid", c)


def _group_frame_only(t):
    t.group = "frame only"
    t.npix = NPIX
    f0, f1, u32, i32, u8, dev = _p(t.f[0]), _p(t.f[1]), _p(t.u32), _p(t.i32), _p(t.u8), t.dev.data_ptr()
    i = ctypes.byref(t.i)
    c, c2 = t.create(), t.create()
    t.frame(c, scene=False, rng=False)
    _every_entry(t, c)
    # the state filled from the host, one piece at a time
    t("cpt_write_accum", "valid", c, f0)
    t("cpt_copy_accum_device", "valid", c, dev, NPIX * 16, None)
    t("cpt_write_moments", "one float short", c, f0, 4 * NPIX - 1)
    t("cpt_write_moments", "valid", c, f0, 4 * NPIX)
    t("cpt_read_moments", "one float short", c, f0, 4 * NPIX - 1)
    t("cpt_read_moments", "valid", c, f0, 4 * NPIX)
    t("cpt_filter_frame", "moments without normals", c, 1, 1.0, 1)
    t("cpt_denoise_mix", "no aux planes", c, 1, None)
    t("cpt_write_aux", "valid", c, f0, f1)
    t("cpt_read_aux", "valid", c, f0, f1)
    t("cpt_read_aux", "the normals alone", c, f0, None)
    t("cpt_filter_frame", "valid", c, 1, 1.0, 1)
    t("cpt_filter_frame", "levels 0", c, 0, 1.0, 1)
    t("cpt_read_filtered", "one pixel short", c, f0, f1, NPIX - 1)
    t("cpt_read_filtered", "valid", c, f0, f1, NPIX)
    t("cpt_read_filtered", "the variance alone", c, None, f1, NPIX)
    t("cpt_write_gbuffer", "one pixel short", c, i32, f0, f0, f0, NPIX - 1)
    t("cpt_write_gbuffer", "no plane given", c, None, None, None, None, NPIX)
    t("cpt_write_gbuffer", "valid", c, i32, f0, f0, f0, NPIX)
    t("cpt_read_gbuffer", "one pixel short", c, i32, f0, f0, f0, NPIX - 1)
    t("cpt_read_gbuffer", "valid", c, i32, f0, f0, f0, NPIX)
    t("cpt_read_gbuffer", "the ids alone", c, i32, None, None, None, NPIX)
    t("cpt_filter_frame_spatial", "valid", c, 1, 1.0, 1)
    t("cpt_denoise_mix", "cur_sample_idx 0", c, 0, None)
    t("cpt_denoise_mix_band", "band [-1, 16)", c, 1, -1, 16, None)
    t("cpt_denoise_mix_band", "band [0, 17)", c, 1, 0, 17, None)
    t("cpt_denoise_mix_band", "band [8, 8)", c, 1, 8, 8, None)
    _every_entry(t, c)
    t("cpt_read_mix", "one float short", c, f0, 3 * NPIX - 1)
    t("cpt_read_display_count", "one float short", c, f0, NPIX - 1)
    t("cpt_copy_bgra_device", "one byte too many", c, dev, 4 * NPIX + 1, None)
    t("cpt_read_present", "one byte short", c, u8, 4 * NPIX - 1)
    t("cpt_copy_present_device", "one byte too many", c, dev, 4 * NPIX + 1, None)
    t("cpt_copy_present_device", "valid", c, dev, 4 * NPIX, None)
    t("cpt_read_rng", "valid", c, u32)
    t("cpt_write_rng", "valid", c, u32)
    # gathers: a frame of another size, then the same frame
    t.ok("cpt_set_frame", c2, 8, 8, None, 0)
    t("cpt_gather_rows", "a source of another size", c, c2)
    t.ok("cpt_set_frame", c2, W, H, None, 0)
    t("cpt_gather_rows", "valid", c, c2)
    t("cpt_last_gather_mode", "valid", c, c2, i)
    t("cpt_synchronize", "valid", c)
    # every row, out of order
    rows = np.arange(H - 1, -1, -1, dtype=np.int32)
    t.ok("cpt_set_frame", c, W, H, _p(rows), H)
    t("cpt_denoise_mix", "rows out of order", c, 1, None)
    t("cpt_filter_frame", "rows out of order", c, 1, 1.0, 1)
    t.ok("cpt_write_aux", c, f0, f1)
    t("cpt_denoise_mix_band", "rows out of order", c, 1, 0, 16, None)
    t("cpt_destroy", "valid", c2)
    t("cpt_destroy", "valid", c)


def _group_scene_frame_rng(t):
    t.group = "scene, frame and RNG"
    t.npix = NPIX
    f0, f1, u32, i32, cam, cam8 = _p(t.f[0]), _p(t.f[1]), _p(t.u32), _p(t.i32), _p(t.cam), _p(t.cam8)
    i, sz, fl = ctypes.byref(t.i), ctypes.byref(t.sz), ctypes.byref(t.fl)
    c = t.create()
    t("cpt_set_scene", "NULL objects", c, None, 1)
    t("cpt_set_scene", "n -1", c, _p(t.objs), -1)
    t.ok("cpt_set_scene", c, _p(t.objs), len(t.objs))
    # a scene without a frame
    t("cpt_render", "no frame", c, cam, 1, 1, 0)
    t("cpt_gbuffer", "no frame", c, cam, 0)
    t("cpt_pick", "no frame", c, cam, 0, 0, 0, i, fl)
    t("cpt_reproject_accum", "no frame", c, cam, cam, 1, 0.0, 0)
    t("cpt_trace_rays", "valid", c, 1, _p(t.rays), _p(t.rays) + 64, None, 0, i32, f1, f1 + 64)
    t("cpt_trace_rays", "no rays", c, 0, None, None, None, 0, None, None, None)
    t("cpt_debug_read_nodes", "the size alone", c, None, 0, sz)
    n_bytes = t.sz.value
    assert 0 < n_bytes <= t.nodes.nbytes
    t("cpt_debug_read_nodes", "one byte short", c, _p(t.nodes), n_bytes - 1, sz)
    t("cpt_debug_read_nodes", "valid", c, _p(t.nodes), n_bytes, sz)
    t.ok("cpt_set_frame", c, W, H, None, 0)
    t("cpt_render", "no RNG", c, cam, 1, 1, 0)
    t.ok("cpt_init_rng", c, 1234)
    # the camera of another size, at every entry that takes one
    t("cpt_render", "a camera of another size", c, cam8, 1, 1, 0)
    t("cpt_tile_costs", "a camera of another size", c, cam8, 1, 1, 0, u32, 64)
    t("cpt_adaptive_begin", "a camera of another size", c, cam8, 1, 1, 1, 0.5, 1, 0)
    t("cpt_render_adaptive", "a camera of another size", c, cam8, 1, 1, 1, 0.5, 1, 0)
    t("cpt_render_to_count", "a camera of another size", c, cam8, 1, 1, 0)
    t("cpt_gbuffer", "a camera of another size", c, cam8, 0)
    t("cpt_pick", "a camera of another size", c, cam8, 0, 0, 0, i, fl)
    t("cpt_reproject_accum", "a `to` of another size", c, cam, cam8, 1, 0.0, 0)
    t("cpt_reproject_display", "a `from` of another size", c, cam8, cam, 1, 0.0, 0)
    t("cpt_reproject_accum_tracked", "a camera of another size", c, cam8, 1, 0.0, 0)
    t("cpt_history_capture", "a camera of another size", c, cam8, 0)
    t("cpt_pick", "pixel (16, 0)", c, cam, 16, 0, 0, i, fl)
    t("cpt_pick", "pixel (0, -1)", c, cam, 0, -1, 0, i, fl)
    t("cpt_pick", "valid, no distance", c, cam, 8, 8, ORDERED, i, None)
    t("cpt_tile_costs", "one tile short", c, cam, 1, 1, 0, u32, TILES - 1)
    # the renders, then everything that reads what they leave
    t("cpt_render", "valid, aux planes", c, cam, 1, 1, AUX | SYNC)
    t("cpt_render", "valid, cost order", c, cam, 1, 1, COST | SYNC)
    t("cpt_render", "valid, previous order", c, cam, 1, 1, PREVIOUS | ORDERED | SYNC)
    t("cpt_render", "valid, accumulating", c, cam, 1, 1, ACCUMULATE)
    t("cpt_render", "valid, the wavefront path", c, cam, 1, 1, WAVEFRONT | SYNC)
    t("cpt_render", "valid, no passes", c, cam, 0, 0, SYNC)
    t("cpt_reproject_display", "no display pass", c, cam, cam, 1, 0.0, 0)
    t("cpt_denoise_mix_band", "valid", c, 1, 0, 8, None)
    t("cpt_reproject_display", "a band on display", c, cam, cam, 1, 0.0, 0)
    t("cpt_reproject_display_tracked", "a band on display", c, cam, 1, 0.0, 0)
    _every_entry(t, c)
    t.ok("cpt_render_adaptive", c, cam, 1, 1, 1, 0.5, 1, 0)
    t("cpt_read_noise", "one pixel short", c, f0, NPIX - 1)
    t("cpt_adaptive_info", "valid, the counts alone", c, i, None, 0, None)
    t("cpt_debug_read_tile_order", "one tile short", c, 0, u32, TILES - 1, sz)
    # the tracked calls with a history, and an object edit behind it
    t.ok("cpt_history_capture", c, cam, 0)
    t("cpt_reproject_accum_tracked", "valid", c, cam, 1, 0.0, 0)
    t.ok("cpt_denoise_mix", c, 1, None)
    t("cpt_reproject_display_tracked", "valid", c, cam, 1, 0.0, 0)
    t("cpt_adaptive_begin", "valid", c, cam, 1, 1, 1, 0.5, 1, COST | AUX)
    t("cpt_adaptive_step", "valid", c, i)
    t("cpt_adaptive_step", "none pending", c, i)
    t("cpt_synchronize", "valid", c)
    t("cpt_destroy", "valid", c)


def _group_row_subset(t):
    t.group = "rows 4..11 of 16"
    t.npix = 8 * W
    f0, f1, u32, u8, cam = _p(t.f[0]), _p(t.f[1]), _p(t.u32), _p(t.u8), _p(t.cam)
    i = ctypes.byref(t.i)
    c, full = t.create(), t.create()
    t.frame(c, rows=range(4, 12))
    t.frame(full)
    t("cpt_render", "valid, aux planes", c, cam, 1, 1, AUX | SYNC)
    _every_entry(t, c)
    t("cpt_tile_costs", "one tile short", c, cam, 1, 1, 0, u32, 1)
    t("cpt_denoise_mix_band", "band [0, 16)", c, 1, 0, 16, None)
    t("cpt_denoise_mix_band", "band [4, 12)", c, 1, 4, 12, None)
    t("cpt_denoise_mix_band", "valid", c, 1, 7, 9, u8)
    t("cpt_display_band", "valid", c, i, ctypes.byref(t.j))
    t("cpt_read_mix", "one float short", c, f0, 2 * W * 3 - 1)
    t("cpt_read_mix", "valid", c, f0, 2 * W * 3)
    t("cpt_read_display_count", "one float short", c, f0, 2 * W - 1)
    t("cpt_read_display_count", "valid", c, f0, 2 * W)
    t("cpt_copy_bgra_device", "one byte too many", c, t.dev.data_ptr(), 2 * W * 4 + 1, None)
    t("cpt_reset_display", "valid", c)
    t("cpt_read_accum", "valid", c, f0)
    t("cpt_read_aux", "valid", c, f0, f1)
    t("cpt_gather_rows", "rows the destination lacks", c, full)
    t("cpt_gather_rows", "valid", full, c)
    t("cpt_last_gather_mode", "valid", full, c, i)
    t("cpt_synchronize", "valid", full)
    t("cpt_synchronize", "valid", c)
    t("cpt_destroy", "valid", full)
    t("cpt_destroy", "valid", c)


def _group_adaptive_pending(t):
    t.group = "adaptive render pending"
    t.npix = NPIX
    f0, u32, u8, cam = _p(t.f[0]), _p(t.u32), _p(t.u8), _p(t.cam)
    i, sz, fl = ctypes.byref(t.i), ctypes.byref(t.sz), ctypes.byref(t.fl)
    c, other = t.create(), t.create()
    t.frame(c)
    t.frame(other)
    t.ok("cpt_adaptive_begin", c, cam, 1, 1, 1, 0.5, 1, 0)
    t("cpt_debug_read_tile_order", "the pending round's list", c, 2, u32, 64, sz)
    t("cpt_debug_read_tile_order", "one tile short", c, 2, u32, TILES - 1, sz)
    # every entry that refuses while the rounds own the frame's buffers
    t("cpt_set_frame", "pending", c, W, H, None, 0)
    t("cpt_render", "pending", c, cam, 1, 1, 0)
    t("cpt_render_to_count", "pending", c, cam, 1, 1, 0)
    t("cpt_adaptive_begin", "pending", c, cam, 1, 1, 1, 0.5, 1, 0)
    t("cpt_render_adaptive", "pending", c, cam, 1, 1, 1, 0.5, 1, 0)
    t("cpt_gbuffer", "pending", c, cam, 0)
    t("cpt_reproject_accum", "pending", c, cam, cam, 1, 0.0, 0)
    t("cpt_reproject_display", "pending", c, cam, cam, 1, 0.0, 0)
    t("cpt_reproject_accum_tracked", "pending", c, cam, 1, 0.0, 0)
    t("cpt_reproject_display_tracked", "pending", c, cam, 1, 0.0, 0)
    t("cpt_history_capture", "pending", c, cam, 0)
    t("cpt_filter_frame", "pending", c, 1, 1.0, 1)
    t("cpt_filter_frame_spatial", "pending", c, 1, 1.0, 1)
    t("cpt_set_exposure", "pending", c, 1.0)
    t("cpt_meter_exposure", "pending", c, 0, 0.18, 500, 1.0)
    t("cpt_read_exposure", "pending", c, fl, u32)
    t("cpt_present", "pending", c, 0, 0, 1.0, 0, u8)
    t("cpt_gather_rows", "pending on the source", other, c)
    t("cpt_gather_rows", "pending on the destination", c, other)
    # what stays allowed: the entries that only wait and read
    t("cpt_read_noise", "pending", c, f0, NPIX)
    t("cpt_adaptive_info", "pending", c, i, u32, 8, None)
    t("cpt_adaptive_step", "valid", c, i)   # the one round was the last: the render ends
    assert t.i.value == 0
    t("cpt_adaptive_step", "none pending", c, i)
    t("cpt_adaptive_info", "valid", c, i, u32, 8, None)
    t("cpt_last_render_ms", "valid", c, fl)
    t("cpt_last_kernel_stats", "valid", c, fl, i)
    t("cpt_destroy", "valid", other)
    t("cpt_destroy", "valid", c)


def run_table():
    t = Table()
    for group in (_group_new_context, _group_frame_only, _group_scene_frame_rng, _group_row_subset, _group_adaptive_pending):
        group(t)
    return t.steps


def test_statuses_and_messages_match_the_recorded_contract():
    with open(FIXTURE) as fh:
        want = json.load(fh)
    got = run_table()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"step {k}: got {g}, recorded {w}"
    assert len(got) == len(want)


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_capi_contract.py --record")
    steps = run_table()
    with open(FIXTURE, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(s) for s in steps) + "\n]\n")
    for s in steps:
        print(s)
    print(f"{len(steps)} steps recorded to {os.path.relpath(FIXTURE, REPO)}")
