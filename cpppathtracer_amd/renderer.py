"""Host-side driver over the C-ABI: one ``Renderer`` = one ``cpt_ctx`` on one GPU.

This is the Python view of the reference's PathTracer pipeline (path_tracer.cu:44-115,
256-319) for tests, the benchmark and multi-GPU tiling; C++ users get the same through
include/cpppathtracer/path_tracer.h.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import (CPT_PATH_WAVEFRONT, CPT_RENDER_ACCUMULATE, CPT_RENDER_AUX, CPT_RENDER_STATS, CPT_RENDER_SYNC,
                   CPT_SCHEDULE_CONSOLIDATE, CPT_SCHEDULE_COST, CPT_SCHEDULE_NO_CONSOLIDATE, CPT_SCHEDULE_PREVIOUS,
                   CPT_TRAVERSAL_ORDERED,
                   CPT_TRAVERSAL_PLAIN_LEAVES, CptError, check)  # noqa: F401  (CptError: callers import it from here)

PATHS = ("megakernel", "wavefront")
from .tiling import tile_grid
from .types import CAMERA_DTYPE, MOTION_DTYPE, OBJECT_DTYPE


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _cam(cam):
    """A camera as it crosses the ABI: a copy as one CAMERA_DTYPE value (contiguous, being one)."""
    return np.array(cam, dtype=CAMERA_DTYPE)


def _render_flags(flags, aux, stats, sync):
    """`flags` with the CPT_RENDER_AUX / _STATS / _SYNC bits of render and render_to_count."""
    return flags | (CPT_RENDER_AUX if aux else 0) | (CPT_RENDER_STATS if stats else 0) | (CPT_RENDER_SYNC if sync else 0)


def _walk_flags(ordered):
    """The CPT_TRAVERSAL_* bits of `ordered`: False, True or "plain" (render's docstring)."""
    return (CPT_TRAVERSAL_ORDERED if ordered else 0) | (CPT_TRAVERSAL_PLAIN_LEAVES if ordered == "plain" else 0)


def device_count() -> int:
    L = _lib.load()
    n = ctypes.c_int(0)
    check(L.cpt_get_device_count(ctypes.byref(n)))
    return n.value


def camera_get_copy(cam):
    """MotionalCamera::GetCopy on a CAMERA_DTYPE value (returns the updated copy)."""
    L = _lib.load()
    c = np.array(cam, dtype=CAMERA_DTYPE, copy=True)
    check(L.cpt_camera_get_copy(_p(c)))
    return c


def topup_deficit_host(count, target):
    """cpt_topup_deficit_host (no GPU): the passes a pixel whose accumulator count is `count` (a
    float32) lacks to `target`, the rule render_to_count's kernels run."""
    L = _lib.load()
    d = ctypes.c_int(-1)
    check(L.cpt_topup_deficit_host(ctypes.c_float(np.float32(count)), int(target), ctypes.byref(d)))
    return d.value


def _reproject_host(entry, cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1, state, motion, max_history, plane_tol):
    """The four *_host reprojections: `state` is the (array, trailing shape) pairs looked up, `motion`
    the table a tracked entry takes.  Returns the new state, one [npix, ...] array per pair."""
    a, b = _cam(cam0), _cam(cam1)
    W, H = int(a["width"].reshape(-1)[0]), int(a["height"].reshape(-1)[0])
    n = W * H
    f32 = lambda v, *tail: np.ascontiguousarray(v, dtype=np.float32).reshape(n, *tail)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32).reshape(n)
    planes = [f32(dir0, 3), f32(dir1, 3), i32(id0), f32(t0), i32(id1), f32(t1), f32(normal1, 3)]
    planes += [f32(v, *tail) for v, tail in state]
    args = [_p(v) for v in planes]
    if entry.endswith("_tracked_host"):
        m, n_objs = _motion_arg(motion)
        args += [_p(m) if n_objs else None, n_objs]
    outs = tuple(np.zeros((n, *tail), dtype=np.float32) for _, tail in state)
    check(getattr(_lib.load(), entry)(_p(a), _p(b), W, H, *args, int(max_history), ctypes.c_float(plane_tol), *map(_p, outs)))
    return outs


def reproject_host(cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1, accum, max_history=32, plane_tol=1e-2):
    """cpt_reproject_host (no GPU): the function reproject_accum's kernel runs, on host arrays.  cam0 /
    cam1 after camera_get_copy; dir0 / dir1 [npix, 3] their centre-ray directions; (id0, t0) and
    (id1, t1, normal1) the G-buffers at cam0 and cam1; accum [npix, 4].  Returns the new [npix, 4]."""
    return _reproject_host("cpt_reproject_host", cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1, ((accum, (4,)),), None,
                           max_history, plane_tol)[0]


def reproject_display_host(cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1, mean, count, max_history=32, plane_tol=1e-2):
    """cpt_reproject_display_host (no GPU): the function reproject_display's kernel runs, on host
    arrays shaped as reproject_host's, with the display state (mean [npix, 3], count [npix]) in
    place of the accumulator.  Returns the new (mean [npix, 3], count [npix])."""
    return _reproject_host("cpt_reproject_display_host", cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1,
                           ((mean, (3,)), (count, ())), None, max_history, plane_tol)


def object_motion_host(old_objs, new_objs):
    """cpt_object_motion_host (no GPU): the motion table (MOTION_DTYPE [n]) of objects as a history
    was captured with (old_objs) and as they are now (new_objs), index by index."""
    L = _lib.load()
    a = np.ascontiguousarray(old_objs, dtype=OBJECT_DTYPE).reshape(-1)
    b = np.ascontiguousarray(new_objs, dtype=OBJECT_DTYPE).reshape(-1)
    if a.shape != b.shape:
        raise ValueError(f"object_motion_host: {a.size} old objects for {b.size} new ones")
    out = np.zeros(a.size, dtype=MOTION_DTYPE)
    check(L.cpt_object_motion_host(_p(a) if a.size else None, _p(b) if a.size else None, int(a.size), _p(out) if a.size else None))
    return out


def _motion_arg(motion):
    if motion is None:
        return None, 0
    m = np.ascontiguousarray(motion, dtype=MOTION_DTYPE).reshape(-1)
    return m, int(m.size)


def reproject_tracked_host(cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1, accum, motion, max_history=32, plane_tol=1e-2):
    """cpt_reproject_tracked_host (no GPU): reproject_host with the motion table (object_motion_host's;
    None: nothing moved) between the captured frame (cam0, id0, t0) and the new one."""
    return _reproject_host("cpt_reproject_tracked_host", cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1, ((accum, (4,)),),
                           motion, max_history, plane_tol)[0]


def reproject_display_tracked_host(cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1, mean, count, motion, max_history=32,
                                   plane_tol=1e-2):
    """cpt_reproject_display_tracked_host (no GPU): reproject_display_host with the motion table."""
    return _reproject_host("cpt_reproject_display_tracked_host", cam0, cam1, dir0, dir1, id0, t0, id1, t1, normal1,
                           ((mean, (3,)), (count, ())), motion, max_history, plane_tol)


class Renderer:
    def __init__(self, device: int = 0):
        self._L = _lib.load()
        h = ctypes.c_void_p()
        check(self._L.cpt_create(device, ctypes.byref(h)))
        self._ctx = h
        self.device = device
        self.width = self.height = self.n_rows = 0
        self.rows = None

    # -- lifecycle -------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._L.cpt_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st):
        return check(st, self._ctx)

    def _call(self, name, *args):
        """Entry `name` on this context, its status checked."""
        st = getattr(self._L, name)(self._ctx, *args)
        return self._check(st) if st else st

    def _get(self, name, ctype, *args):
        """The one value entry `name` writes through its last argument, as a Python float or int."""
        out = ctype()
        self._call(name, *args, ctypes.byref(out))
        return out.value

    def _read(self, name, shape, dtype, *tail):
        """Zeros of `shape`, filled by entry `name` (the array, then `tail`)."""
        out = np.zeros(shape, dtype=dtype)
        self._call(name, _p(out), *tail)
        return out

    # -- setup -----------------------------------------------------------------------
    def set_stream(self, hip_stream_handle):
        self._call("cpt_set_stream", ctypes.c_void_p(hip_stream_handle or 0))

    def set_scene(self, objs):
        objs = np.ascontiguousarray(objs, dtype=OBJECT_DTYPE)
        self._call("cpt_set_scene", _p(objs) if len(objs) else None, len(objs))

    def update_object(self, index, obj):
        o = np.array(obj, dtype=OBJECT_DTYPE, copy=True)
        self._call("cpt_update_object", index, _p(o))

    def update_objects(self, indices, objs, rebuild=False):
        """SceneBVH::UpdateObject for a batch: refit on the device (cpt_update_objects), or with
        the ordered walk's tree rebuilt on the host (rebuild=True, cpt_update_objects_rebuild)."""
        idx = np.ascontiguousarray(indices, dtype=np.int32)
        o = np.ascontiguousarray(objs, dtype=OBJECT_DTYPE)
        if o.shape != idx.shape:
            raise ValueError(f"update_objects: {o.shape[0] if o.ndim else 1} objects for {idx.size} indices")
        self._call("cpt_update_objects_rebuild" if rebuild else "cpt_update_objects", int(idx.size), _p(idx), _p(o))

    def material_count(self) -> int:
        """Material slots the scene holds (cpt_get_material_count)."""
        return self._get("cpt_get_material_count", ctypes.c_int)

    def last_update_ms(self) -> float:
        return self._get("cpt_last_update_ms", ctypes.c_float)

    def bvh_export(self):
        n = ctypes.c_int(0)
        self._call("cpt_scene_bvh_export", None, None, 0, ctypes.byref(n))
        m = n.value
        boxes = np.zeros((max(m, 1), 6), dtype=np.float32)
        links = np.zeros((max(m, 1), 4), dtype=np.int32)
        self._call("cpt_scene_bvh_export", _p(boxes), _p(links), m, ctypes.byref(n))
        return boxes[:m], links[:m]

    def set_env(self, env):
        """env: texture_io.EnvTexture (or None for a black environment)."""
        if env is None:
            self._call("cpt_set_env_texture", None, 1, 1, 0)
            return
        rgba = np.ascontiguousarray(env.rgba, dtype=np.uint8)
        self._call("cpt_set_env_texture", _p(rgba), env.width, env.height, env.valid_cols)

    def bind_texture(self, handle, tex, address_mode=2, filter_mode=1):
        """Bind texels (texture_io.EnvTexture) to a material texture handle (cpt_bind_texture);
        defaults = AddTexByFile's mirror + linear."""
        rgba = np.ascontiguousarray(tex.rgba, dtype=np.uint8)
        self._call("cpt_bind_texture", handle, _p(rgba), tex.width, tex.height, tex.valid_cols, address_mode, filter_mode)

    def set_frame(self, width, height, rows=None):
        if rows is None:
            self._call("cpt_set_frame", width, height, None, 0)
            self.rows = np.arange(height, dtype=np.int32)
        else:
            r = np.ascontiguousarray(rows, dtype=np.int32)
            self._call("cpt_set_frame", width, height, _p(r), r.size)
            self.rows = r
        self.width, self.height, self.n_rows = width, height, int(self.rows.size)

    def init_rng(self, seed):
        self._call("cpt_init_rng", ctypes.c_uint64(seed))

    # -- render ----------------------------------------------------------------------
    def render(self, cam, spp, max_depth, accumulate=False, aux=False, stats=False, sync=False, flags=0,
               path="megakernel", ordered=False, schedule="tiles", consolidate=None):
        """path: "megakernel" (per-lane regeneration, state in VGPRs) or "wavefront" (SoA state in
        HBM, extend/shade kernels with ballot compaction).  Both give identical results.
        ordered: near-first BVH walk per direction octant (CPT_TRAVERSAL_ORDERED); same closest
        hits as the reference order up to box/primitive rounding (DESIGN.md §Ordered walk).
        ordered="plain": the same walk testing each leaf where it meets it (per-ray node/prim
        counts, CPT_TRAVERSAL_PLAIN_LEAVES) instead of parking leaves for wave-wide rounds.
        schedule: "tiles" (8x8 tiles dequeued in row-major order) or "cost" (CPT_SCHEDULE_COST: a
        short pilot render measures each tile's work and the megakernel dequeues the tiles
        heaviest first; same results, DESIGN.md §Cost schedule) or "previous"
        (CPT_SCHEDULE_PREVIOUS: heaviest first by the previous such render's per-tile RNG draws,
        no pilot; for repeated renders of few passes, the DispatchRay loop).
        consolidate: None (the library's default: on for frames of more than 1 and at most 4
        pixels per lane and spp >= 512), True or
        False (CPT_SCHEDULE_[NO_]CONSOLIDATE): the megakernel's tail consolidation, same results."""
        if path not in PATHS:
            raise ValueError(f"path must be one of {PATHS}")
        if schedule not in ("tiles", "cost", "previous"):
            raise ValueError("schedule must be 'tiles', 'cost' or 'previous'")
        c = _cam(cam)
        f = _render_flags(flags, aux, stats, sync) | _walk_flags(ordered)
        f |= CPT_PATH_WAVEFRONT if path == "wavefront" else 0
        f |= CPT_RENDER_ACCUMULATE if accumulate else 0
        f |= CPT_SCHEDULE_COST if schedule == "cost" else 0
        f |= CPT_SCHEDULE_PREVIOUS if schedule == "previous" else 0
        if consolidate is not None:
            f |= CPT_SCHEDULE_CONSOLIDATE if consolidate else CPT_SCHEDULE_NO_CONSOLIDATE
        self._call("cpt_render", _p(c), spp, max_depth, f)

    def render_to_count(self, cam, target, max_depth, aux=False, stats=False, sync=False, flags=0):
        """cpt_render_to_count: every pixel runs the passes its accumulator count lacks to `target`
        (topup_deficit_host's rule), continuing its RNG stream and adding to its accumulator as an
        accumulating render of that many passes would; a pixel at or past the target is not
        written at all.  One plan (tiles keyed by their largest deficit, sorted) and one megakernel
        launch over the tiles with a deficit.  `flags`: CPT_TRAVERSAL_* bits (not the wavefront
        path, no CPT_SCHEDULE_PREVIOUS / _COST / _CONSOLIDATE).  Asynchronous unless sync."""
        c = _cam(cam)
        self._call("cpt_render_to_count", _p(c), int(target), int(max_depth), _render_flags(int(flags), aux, stats, sync))

    def topup_info(self):
        """cpt_topup_info of the last render_to_count: {"tiles", "pixels", "passes"}, the 8x8 tiles
        and the pixels with a deficit and the sum of the deficits.  Waits for the call."""
        tiles, pixels, passes = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._call("cpt_topup_info", ctypes.byref(tiles), ctypes.byref(pixels), ctypes.byref(passes))
        return {"tiles": int(tiles.value), "pixels": int(pixels.value), "passes": int(passes.value)}

    def render_adaptive(self, cam, min_spp, max_spp, batch, rel_error, max_depth, flags=0):
        """cpt_render_adaptive: rounds of `batch` passes over the 8x8 tiles whose pixels have not all
        reached a relative standard error of `rel_error` (none leaves before `min_spp`, all at
        `max_spp`); every pixel ends bit for bit as a render() of its own pass count.  `flags`: the
        CPT_* render flags (not the wavefront path, not CPT_SCHEDULE_PREVIOUS).  Synchronous.
        Returns {"rounds", "active_tiles" (uint32 per round), "passes_done" (pixel passes)}."""
        c = _cam(cam)
        self._call("cpt_render_adaptive", _p(c), int(min_spp), int(max_spp), int(batch), ctypes.c_float(rel_error),
                   int(max_depth), int(flags))
        return self.adaptive_info()

    def adaptive_info(self):
        """cpt_adaptive_info of the last adaptive render: {"rounds", "active_tiles" (uint32 per
        round), "passes_done" (pixel passes)}."""
        rounds, passes = ctypes.c_int(0), ctypes.c_uint64(0)
        self._call("cpt_adaptive_info", ctypes.byref(rounds), None, 0, ctypes.byref(passes))
        active = np.zeros(max(1, rounds.value), dtype=np.uint32)
        self._call("cpt_adaptive_info", ctypes.byref(rounds), _p(active), active.size, ctypes.byref(passes))
        return {"rounds": rounds.value, "active_tiles": active[:rounds.value].copy(), "passes_done": int(passes.value)}

    def adaptive_begin(self, cam, min_spp, max_spp, batch, rel_error, max_depth, flags=0):
        """cpt_adaptive_begin: render_adaptive's checks and its first round, queued without a host
        wait.  Until adaptive_step returns 0 the render is pending: render, render_adaptive,
        adaptive_begin, set_frame, filter_frame and gather_rows with this Renderer raise
        CPT_ERR_STATE."""
        c = _cam(cam)
        self._call("cpt_adaptive_begin", _p(c), int(min_spp), int(max_spp), int(batch), ctypes.c_float(rel_error),
                   int(max_depth), int(flags))

    def adaptive_step(self) -> int:
        """cpt_adaptive_step: waits for the queued round, then queues the next one and returns the
        tiles it renders, or ends the render and returns 0 (adaptive_info then has its record)."""
        return self._get("cpt_adaptive_step", ctypes.c_int)

    def read_noise(self):
        """The last render_adaptive's noise map (cpt_read_noise): each pixel's relative standard
        error as its last round left it, [npix] float32 (+inf with fewer than two batches)."""
        return self._read("cpt_read_noise", self.npix, np.float32, self.npix)

    def read_moments(self):
        """The adaptive render's per-pixel moments (cpt_read_moments): [4, npix] float32, the sum
        m1 of each pixel's k batch means' luminance, the sum m2 of their squares, k, and the noise
        map."""
        return self._read("cpt_read_moments", (4, self.npix), np.float32, 4 * self.npix)

    def write_moments(self, planar4):
        """Restore the moments ([4, npix] float32) from a host copy (cpt_write_moments): with
        write_accum, write_rng and write_aux, the checkpoint of an adaptive session."""
        a = np.ascontiguousarray(planar4, dtype=np.float32)
        if a.shape != (4, self.npix):
            raise ValueError(f"write_moments: expected shape (4, {self.npix}), got {a.shape}")
        self._call("cpt_write_moments", _p(a), a.size)

    def filter_frame(self, levels=5, sigma_l=1.0, normal_sharpness_log2=7):
        """cpt_filter_frame: the variance-guided a-trous filter of the frame an adaptive render left
        (needs a full frame, moments, and normals from CPT_RENDER_AUX or write_aux).  `levels`
        5x5 B3-spline iterations at step 1, 2, 4, ..., edge-stopped by the first-hit normals
        (sharper with a larger normal_sharpness_log2) and by luminance differences of more than
        about sigma_l standard errors.  Asynchronous; read_filtered waits."""
        self._call("cpt_filter_frame", int(levels), ctypes.c_float(sigma_l), int(normal_sharpness_log2))

    def filter_frame_spatial(self, levels=3, sigma_l=2.0, normal_sharpness_log2=3):
        """cpt_filter_frame_spatial: filter_frame for a frame without moments (a plain render, a
        reprojected or topped-up frame).  Level 0's variance is estimated from each pixel's 7x7
        window, count-weighted, within its object; the levels are guided by the G-buffer's normals
        and stop at its object boundaries.  Needs a full frame and a valid G-buffer OF THE CAMERA
        THE ACCUMULATOR BELONGS TO: a reprojection leaves it, after a plain render call gbuffer(cam)
        first.  Asynchronous; read_filtered and last_filter_ms serve both filters."""
        self._call("cpt_filter_frame_spatial", int(levels), ctypes.c_float(sigma_l), int(normal_sharpness_log2))

    def read_filtered(self):
        """The last filter_frame's or filter_frame_spatial's result (cpt_read_filtered): (rgb [npix, 3], variance of the
        filtered mean [npix]) float32."""
        rgb = np.zeros((self.npix, 3), dtype=np.float32)
        var = np.zeros(self.npix, dtype=np.float32)
        self._call("cpt_read_filtered", _p(rgb), _p(var), self.npix)
        return rgb, var

    def last_filter_ms(self) -> float:
        """Device time of the last filter_frame, all its launches (HIP events); waits for it."""
        return self._get("cpt_last_filter_ms", ctypes.c_float)

    # -- first-hit queries -----------------------------------------------------------
    def gbuffer(self, cam, flags=0):
        """cpt_gbuffer: the first hit of every pixel's centre ray (RayGen at zero lens offset), by
        the walk of `flags` (CPT_TRAVERSAL_* bits only).  Writes buffers of its own; the
        accumulator, the RNG states and the aux buffers are untouched.  Asynchronous;
        read_gbuffer waits."""
        c = _cam(cam)
        self._call("cpt_gbuffer", _p(c), int(flags))

    def read_gbuffer(self):
        """The last gbuffer's result (cpt_read_gbuffer): {"id" [npix] int32 (object index in
        set_scene's order, -1 = miss), "t" [npix] (1e30 on a miss), "normal" [npix, 3] (-dir on a
        miss), "albedo" [npix, 3] (0 on a miss)}."""
        out = {"id": np.zeros(self.npix, dtype=np.int32), "t": np.zeros(self.npix, dtype=np.float32),
               "normal": np.zeros((self.npix, 3), dtype=np.float32), "albedo": np.zeros((self.npix, 3), dtype=np.float32)}
        self._call("cpt_read_gbuffer", _p(out["id"]), _p(out["t"]), _p(out["normal"]), _p(out["albedo"]), self.npix)
        return out

    def write_gbuffer(self, id=None, t=None, normal=None, albedo=None):
        """Restore the G-buffer's planes from host copies (cpt_write_gbuffer; read_gbuffer's shapes)
        and make it valid.  A plane given as None is left as it is (zeros if never written)."""
        def plane(a, dtype, shape, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.size != int(np.prod(shape)):
                raise ValueError(f"write_gbuffer: {name} of {a.size} values, expected shape {shape}")
            return a.reshape(shape)
        i = plane(id, np.int32, (self.npix,), "id")
        d = plane(t, np.float32, (self.npix,), "t")
        n = plane(normal, np.float32, (self.npix, 3), "normal")
        k = plane(albedo, np.float32, (self.npix, 3), "albedo")
        self._call("cpt_write_gbuffer", _p(i), _p(d), _p(n), _p(k), self.npix)

    def trace_rays(self, origins, dirs, tmin=None, flags=0):
        """cpt_trace_rays: the first hit of each ray (origins, dirs [n, 3]; tmin [n] or None = 0);
        directions are used as given, not normalised.  Needs only a scene.  Returns {"id" [n]
        int32, "t" [n], "normal" [n, 3]} with gbuffer's miss conventions.  Synchronous."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError(f"trace_rays: {o.shape[0]} origins for {d.shape[0]} directions")
        n = o.shape[0]
        tm = None
        if tmin is not None:
            tm = np.ascontiguousarray(tmin, dtype=np.float32).reshape(-1)
            if tm.size != n:
                raise ValueError(f"trace_rays: {tm.size} tmin values for {n} rays")
        out = {"id": np.zeros(n, dtype=np.int32), "t": np.zeros(n, dtype=np.float32),
               "normal": np.zeros((n, 3), dtype=np.float32)}
        self._call("cpt_trace_rays", n, _p(o), _p(d), _p(tm), int(flags), _p(out["id"]), _p(out["t"]), _p(out["normal"]))
        return out

    def pick(self, cam, x, y, flags=0):
        """cpt_pick: (object index or -1, distance) under pixel (x, y) of the image: gbuffer's id
        and t of that pixel, by one ray.  Synchronous."""
        c = _cam(cam)
        obj, t = ctypes.c_int32(-1), ctypes.c_float(0)
        self._call("cpt_pick", _p(c), int(x), int(y), int(flags), ctypes.byref(obj), ctypes.byref(t))
        return int(obj.value), np.float32(t.value)

    def last_query_ms(self) -> float:
        """Device time of the last gbuffer, trace_rays or pick kernel (HIP events); waits for it."""
        return self._get("cpt_last_query_ms", ctypes.c_float)

    # -- reprojection ----------------------------------------------------------------
    def _reproject(self, entry, cams, max_history, plane_tol, flags):
        """The four reproject_* calls: `cams` is (cam_from, cam_to), or (cam_to,) for a tracked entry."""
        cams = [_cam(c) for c in cams]
        self._call(entry, *map(_p, cams), int(max_history), ctypes.c_float(plane_tol), int(flags))

    def reproject_accum(self, cam_from, cam_to, max_history=32, plane_tol=1e-2, flags=0):
        """cpt_reproject_accum: the accumulator, rendered with cam_from, looked up at cam_to (both
        after camera_get_copy): each new pixel's first hit is projected into the old frame and the
        four pixels around it blended, a tap only where it saw the same object on the new hit's
        tangent plane (within plane_tol x the hit distance); pass counts are capped at
        max_history, pixels without history end as zeros.  Needs a full frame and a static scene;
        leaves cam_to's G-buffer in read_gbuffer and drops the frame's adaptive result.
        flags: CPT_TRAVERSAL_* bits only.  Asynchronous."""
        self._reproject("cpt_reproject_accum", (cam_from, cam_to), max_history, plane_tol, flags)

    def reproject_display(self, cam_from, cam_to, max_history=32, plane_tol=1e-2, flags=0):
        """cpt_reproject_display: reproject_accum's look-up applied to the display state, the Mix
        running mean and the per-pixel sample counts of denoise_mix_history, which the next
        denoise_mix_history continues from.  Needs a display pass of the full frame; leaves the
        accumulator, the RNG and the BGRA8 frame alone and cam_to's G-buffer in read_gbuffer.
        Asynchronous."""
        self._reproject("cpt_reproject_display", (cam_from, cam_to), max_history, plane_tol, flags)

    def history_capture(self, cam, flags=0):
        """cpt_history_capture: makes the frame as rendered at `cam` (after camera_get_copy) the
        captured history of the tracked calls: cam's G-buffer in the current scene (read_gbuffer
        returns it), cam itself and a snapshot of the objects.  Asynchronous."""
        c = _cam(cam)
        self._call("cpt_history_capture", _p(c), int(flags))

    def history_info(self):
        """cpt_history_info: (whether a history is captured, its camera or None)."""
        valid = ctypes.c_int(0)
        cam = np.zeros((), dtype=CAMERA_DTYPE)
        self._call("cpt_history_info", ctypes.byref(valid), _p(cam))
        return bool(valid.value), (cam if valid.value else None)

    def reproject_accum_tracked(self, cam_to, max_history=32, plane_tol=1e-2, flags=0):
        """cpt_reproject_accum_tracked: reproject_accum from the captured history to cam_to through
        the object edits since the capture (each new hit is looked up where its object stood then;
        objects whose type or material changed restart).  One trace; cam_to, its G-buffer and the
        current objects become the captured history.  Asynchronous."""
        self._reproject("cpt_reproject_accum_tracked", (cam_to,), max_history, plane_tol, flags)

    def reproject_display_tracked(self, cam_to, max_history=32, plane_tol=1e-2, flags=0):
        """cpt_reproject_display_tracked: reproject_accum_tracked's look-up applied to the display
        state, as reproject_display is to reproject_accum.  Asynchronous."""
        self._reproject("cpt_reproject_display_tracked", (cam_to,), max_history, plane_tol, flags)

    def last_reproject_ms(self, split=False):
        """Device time of the last reproject_accum, reproject_display or tracked variant of either, all its
        launches (HIP events); waits for it.  split: (trace at cam_from, trace at cam_to, look-up kernel)
        instead of their total; after a tracked call, which does not trace at cam_from, the first is 0."""
        if split:
            ms3 = (ctypes.c_float * 3)()
            self._call("cpt_last_reproject_launch_ms", ms3)
            return tuple(float(v) for v in ms3)
        return self._get("cpt_last_reproject_ms", ctypes.c_float)

    def tile_costs(self, cam, passes, max_depth, ordered=True):
        """The cost schedule's pilot alone (cpt_tile_costs): the work of each 8x8 tile's heaviest
        pixel (the maximum over the tile's pixels, not their sum) over `passes` passes from the
        current RNG states (nothing written back), [tiles_y, tiles_x] uint32."""
        c = _cam(cam)
        out = np.zeros(tile_grid(self.width, self.n_rows), dtype=np.uint32)
        self._call("cpt_tile_costs", _p(c), int(passes), int(max_depth), _walk_flags(ordered), _p(out), out.size)
        return out

    def synchronize(self):
        self._call("cpt_synchronize")

    def last_render_ms(self) -> float:
        return self._get("cpt_last_render_ms", ctypes.c_float)

    def last_kernel_stats(self):
        """(average ms per launch, launches) of the last render's dominant kernel, without the
        cost schedule's pilot (HIP events on the launch stream; waits for the render)."""
        ms, n = ctypes.c_float(0), ctypes.c_int(0)
        self._call("cpt_last_kernel_stats", ctypes.byref(ms), ctypes.byref(n))
        return float(ms.value), int(n.value)

    # -- readback --------------------------------------------------------------------
    @property
    def npix(self):
        return self.n_rows * self.width

    def read_accum(self):
        return self._read("cpt_read_accum", (self.npix, 4), np.float32)

    def clear_accum(self):
        self._call("cpt_clear_accum")

    def read_rng(self):
        return self._read("cpt_read_rng", (6, self.npix), np.uint32)

    def write_rng(self, planar6):
        a = np.ascontiguousarray(planar6, dtype=np.uint32)
        if a.shape != (6, self.npix):
            raise ValueError(f"write_rng: expected shape (6, {self.npix}), got {a.shape}")
        self._call("cpt_write_rng", _p(a))

    def read_aux(self):
        n = np.zeros((self.npix, 3), dtype=np.float32)
        d = np.zeros(self.npix, dtype=np.float32)
        self._call("cpt_read_aux", _p(n), _p(d))
        return n, d

    def write_accum(self, rgba):
        """Restore the accumulator ([npix, 4] float32) from a host copy (checkpoint / resume)."""
        a = np.ascontiguousarray(rgba, dtype=np.float32).reshape(self.npix, 4)
        self._call("cpt_write_accum", _p(a))

    def write_aux(self, normal3, depth):
        """Restore the first-hit normal ([npix, 3]) and depth ([npix]) buffers from host copies."""
        n = np.ascontiguousarray(normal3, dtype=np.float32).reshape(self.npix, 3)
        d = np.ascontiguousarray(depth, dtype=np.float32).reshape(self.npix)
        self._call("cpt_write_aux", _p(n), _p(d))

    def copy_accum_device(self, device_ptr, nbytes, stream):
        """Device copy of the accumulator, ordered against the caller's HIP stream (a handle,
        e.g. torch.cuda.current_stream().cuda_stream; 0 = the null stream) with no host wait:
        it starts after the work queued there so far and that stream's next work sees it."""
        self._call("cpt_copy_accum_device", ctypes.c_void_p(device_ptr), nbytes, ctypes.c_void_p(stream or None))

    def gather_rows(self, src):
        """cpt_gather_rows: place the rows Renderer `src` rendered into this frame (row tiling)."""
        self._call("cpt_gather_rows", src._ctx)

    GATHER_MODES = {-1: None, 0: "same_device", 1: "peer", 2: "staged"}

    def last_gather_mode(self, src):
        """How the last gather_rows(src) reached src's buffers: "same_device", "peer" (xGMI
        reads with peer access), "staged" (a peer copy first), or None (no gather yet)."""
        m = ctypes.c_int(-1)
        self._call("cpt_last_gather_mode", src._ctx, ctypes.byref(m))
        return self.GATHER_MODES[m.value]

    def set_debug_gather(self, force_staged):
        """Test hook: route this context's gathers through the staged peer copy."""
        self._call("cpt_set_debug_gather", int(bool(force_staged)))

    def stats(self):
        s = (ctypes.c_uint64 * 5)()
        self._call("cpt_get_stats", s)
        return dict(zip(("segments", "nodes", "prims", "hits", "misses"), (int(x) for x in s)))

    def raw_counters(self):
        return [int(x) for x in self._read("cpt_get_raw_counters", 8, np.uint64)]

    def debug_timeline(self):
        """DIAGNOSTIC: the lane-occupancy timeline of a CPT_TIMELINE build (cpt_debug_timeline):
        ([4096, 4] uint64 bins, first tick the queue ran dry); clears it."""
        out = self._read("cpt_debug_timeline", 4 * 4096 + 4, np.uint64, 4 * 4096 + 4)
        return out[: 4 * 4096].reshape(4096, 4), int(out[4 * 4096])

    def diag_counters(self):
        """DIAGNOSTIC: the 16 stamp slots of a CPT_STAMPS build (cpt_stamps.hpp)."""
        return [int(x) for x in self._read("cpt_get_diag_counters", 16, np.uint64)]

    def execdiag_counters(self):
        """DIAGNOSTIC: the exec-mask census of a CPT_EXECDIAG build (cpt_stamps.hpp execdiag)."""
        return self._read("cpt_get_execdiag_counters", 64, np.uint64).reshape(4, 16)

    def walk_info(self):
        """[reference-order nodes, binary octant-order nodes, 4-wide nodes per octant, platforms]."""
        out = self._read("cpt_get_walk_info", 4, np.int32)
        return dict(zip(("n_bvh", "n_walk", "n_wide", "n_unb"), (int(x) for x in out)))

    def read_nodes(self):
        """DIAGNOSTIC: the device's node memory (cpt_debug_read_nodes) as uint8: the reference
        order, the eight octant orders, the 4-wide image and its leaf array (walk_info's counts)."""
        n = ctypes.c_size_t(0)
        self._call("cpt_debug_read_nodes", None, 0, ctypes.byref(n))
        out = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            self._call("cpt_debug_read_nodes", _p(out), out.size, ctypes.byref(n))
        return out

    def debug_tile_order(self, which):
        """DIAGNOSTIC: a device-built tile list (cpt_debug_read_tile_order) as uint32 tile ids:
        which = 0 the cost schedule's order, 1 the CPT_SCHEDULE_PREVIOUS order, 2 the list the
        pending adaptive round renders, 4 (CPT_TILE_ORDER_TOPUP) the tiles the last render_to_count
        rendered, largest deficit first.  Waits for the context's stream."""
        ty, tx = tile_grid(self.width, self.n_rows)
        out = np.zeros(max(1, ty * tx), dtype=np.uint32)
        n = ctypes.c_size_t(0)
        self._call("cpt_debug_read_tile_order", int(which), _p(out), ty * tx, ctypes.byref(n))
        return out[:n.value].copy()

    def measure_read_pattern(self, bytes_per_lane, nbytes=1 << 30, iters=1):
        """DIAGNOSTIC: GB/s of a streaming read in one of the display kernel's access shapes
        (cpt_measure_read_pattern: 4, 12 or 16 bytes per lane)."""
        return self._get("cpt_measure_read_pattern", ctypes.c_float, int(bytes_per_lane), int(nbytes), int(iters))

    def measure_read_bandwidth(self, nbytes=4 << 30, iters=10):
        """HBM streaming-read ceiling in GB/s (cpt_measure_read_bandwidth)."""
        return self._get("cpt_measure_read_bandwidth", ctypes.c_float, int(nbytes), int(iters))

    def set_debug_consolidation(self, flags=0, keeper_spin_log2=0, publish_wait_log2=0):
        """TEST HOOK (cpt_set_debug_consolidation): provoke the tail consolidation's error paths."""
        self._call("cpt_set_debug_consolidation", flags, keeper_spin_log2, publish_wait_log2)

    def set_debug_grid(self, max_workgroups=0, lanes_per_wave=0):
        """TEST HOOK (cpt_set_debug_grid): cap the megakernel's persistent grid at `max_workgroups`
        workgroups and let only the first `lanes_per_wave` lanes of a wave take pixels, so that
        small frames exercise the lane refill; 0, 0 (the default) is normal operation."""
        self._call("cpt_set_debug_grid", int(max_workgroups), int(lanes_per_wave))

    def reset_stats(self):
        self._call("cpt_reset_stats")

    def selftest_qdiv(self, which, n, seed=1, examples=16):
        """Returns (mismatch count, [(a, d) float32 pairs of some mismatches])."""
        out = np.zeros(examples + 1, dtype=np.uint64)
        self._call("cpt_selftest_qdiv", which, n, seed, _p(out), out.size)
        cnt = int(out[0])
        pairs = [(np.uint32(int(v) >> 32).view(np.float32), np.uint32(int(v) & 0xFFFFFFFF).view(np.float32))
                 for v in out[1:1 + min(cnt, examples)]]
        return cnt, pairs

    def _frame_out(self, out, who):
        """The host frame display call `who` writes: a new (height, width, 4) one, or `out` checked."""
        if out is None:
            return np.zeros((self.height, self.width, 4), dtype=np.uint8)
        # explicit checks, not asserts: the C-ABI writes a full H*W*4 frame into `out` (a kernel
        # store through a pinned alias or a hipMemcpyAsync), so a bad buffer must raise, also
        # under `python -O`
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8:
            raise ValueError(f"{who}: `out` must be a numpy uint8 array")
        if out.size != self.height * self.width * 4:
            raise ValueError(f"{who}: `out` holds {out.size} bytes, the frame needs {self.height * self.width * 4}")
        flags = out.flags
        if not flags.c_contiguous or not flags.writeable:
            raise ValueError(f"{who}: `out` must be C-contiguous and writeable")
        return out

    def denoise_mix(self, cur_sample_idx, out=None, host=True):
        """Denoising + Mix display pass; returns the BGRA8 frame (height, width, 4), into `out`
        when given (a preallocated, e.g. pinned, host array of that shape).  host=False keeps the
        frame on the device (no host write; returns None): the display kernel's device-only time."""
        out = self._frame_out(out, "denoise_mix") if host else None
        self._call("cpt_denoise_mix", cur_sample_idx, _p(out))
        return out

    def denoise_mix_history(self, out=None, host=True):
        """cpt_denoise_mix_history: denoise_mix with each pixel mixed at 1 / (its own sample count
        + 1), the count kept beside the running mean (read_display_count); `out` and `host` as
        denoise_mix's.  From a reset display, k calls equal denoise_mix(1), ..., denoise_mix(k)."""
        out = self._frame_out(out, "denoise_mix_history") if host else None
        self._call("cpt_denoise_mix_history", _p(out))
        return out

    def read_display_count(self):
        """The per-pixel sample counts of the display band (cpt_read_display_count):
        [(y1 - y0) * width] float32 holding integers, 0 outside the launch region."""
        y0, y1 = self.display_band()
        n = (y1 - y0) * self.width
        return self._read("cpt_read_display_count", n, np.float32, n)

    def display_band(self):
        """The output rows (y0, y1) the display buffers hold (cpt_display_band)."""
        y0, y1 = ctypes.c_int(0), ctypes.c_int(0)
        self._call("cpt_display_band", ctypes.byref(y0), ctypes.byref(y1))
        return y0.value, y1.value

    def read_mix(self):
        """The Mix running mean of the display band: [(y1 - y0) * width, 3] float32, sized from
        the library's own band (a failed band switch cannot leave it stale)."""
        y0, y1 = self.display_band()
        n = (y1 - y0) * self.width
        return self._read("cpt_read_mix", (n, 3), np.float32, 3 * n)

    def last_display_ms(self) -> float:
        """Device time of the last display kernel (Denoising + Mix), HIP events."""
        return self._get("cpt_last_display_ms", ctypes.c_float)

    def denoise_mix_band(self, cur_sample_idx, y0, y1, host=True):
        """Display path for output rows [y0, y1) (cpt_denoise_mix_band): the frame's rows must be
        one ascending run covering the band and its 3-row halo.  Returns the band's BGRA8 rows
        (y1 - y0, width, 4), or None with host=False (then copy_bgra_device moves them)."""
        out = np.zeros((y1 - y0, self.width, 4), dtype=np.uint8) if host else None
        self._call("cpt_denoise_mix_band", cur_sample_idx, int(y0), int(y1), _p(out))
        return out

    def copy_bgra_device(self, device_ptr, nbytes, stream):
        """Device copy of the display band's BGRA8 rows, ordered against `stream` as
        copy_accum_device."""
        self._call("cpt_copy_bgra_device", ctypes.c_void_p(device_ptr), nbytes, ctypes.c_void_p(stream or None))

    def reset_display(self):
        self._call("cpt_reset_display")

    def math_batch(self, op, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), dtype=np.float32)
        out = np.empty_like(a)
        self._call("cpt_math_batch", op, _p(a), _p(b), _p(out), a.size)
        return out
