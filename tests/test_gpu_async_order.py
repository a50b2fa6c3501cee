"""Every C-ABI call directly behind an unsynchronised render.

cpt_render without CPT_RENDER_SYNC returns while the render runs on the context's non-blocking
stream, so every other entry point has to order itself against that stream.  One mechanism, a
table of cases:

* the SUBJECT context issues render(sync=False) and then, at once, the call under test; it then
  synchronises and reads;
* its TWIN, a second Renderer(0) in the same process, runs the same steps with sync=True and a
  synchronize() (the context's and the device's) after every single call (`Synced`);
* everything the two can read back must agree bit for bit: the accumulator, the RNG planes and,
  where the case produces them, aux, moments, noise, filtered planes, G-buffer, mix and BGRA, tile
  costs and orders, node bytes, counters, and whatever the call itself returned;
* the twin's first render is held to the oracle (computed once for the module) in every case whose
  render in flight is the module's workload, which pins the twin itself.

Overlap, so that no case is vacuous: t_launch is taken immediately before render(sync=False),
t_call immediately before the call under test, both with time.perf_counter().  The render's first
timing event is recorded after t_launch, so the render cannot end before t_launch + render_ms, and
every case asserts

    render_ms >= 4 * (t_call - t_launch)

-- at least three quarters of the render was still ahead when the call began -- and fails, never
skips, otherwise.  render_ms is the subject's own cpt_last_render_ms, read after the final
synchronise.  Where the call under test is itself a render (a second cpt_render, cpt_render_adaptive)
it records the context's timing events again and the first render's time can no longer be read; for
those cases (`rerecords`) render_ms is the time of the identical launch -- same scene, frame,
passes, RNG states, device -- that the twin measured just before.

Workload: scenes.scene_s1000(n=150), 64 x 40, depth 8, megakernel:ordered, consolidate=False and
fewer than 512 passes (no hand-over spin loop can be involved).  Its synchronised render on one
MI355X, on the commit before this file (cpt_last_render_ms, four renders each):

    spp  32:  0.58 - 0.77 ms
    spp  64:  1.07 - 1.10 ms
    spp 128:  2.01 - 2.04 ms
    spp 256:  3.78 - 3.81 ms      (384: 5.6 ms; 511: 7.3 - 7.5 ms)

None of the four reaches the 50 ms first hoped for: the camera of scenes.camera_for sees the floor
and the sky, the 150 objects lie behind the look-at point.  SPP = 256, the largest of the four, is
used.  What the 50 ms were to buy is there all the same: render() returned after 0.016 ms and the
next ctypes call after another 0.006 ms in the same run, so the condition (3.8 ms against 4 x 0.016
ms) holds with a factor of about 60 to spare, and a call made 0.02 ms after the launch meets the
first percent of the render.  scenes.scene_s4_textured (the bind_texture case) takes 12.0 - 13.1 ms
at 256 passes.

A case for a new entry point is one line of CASES: a name, a function (r, e) that makes the call
and returns what it returned, and the names (READERS) of what to read afterwards.  Left out on
purpose: destroying a context behind a render in flight, and bad arguments with work in flight (a
regression there would be a device fault, which no test should be able to cause).
"""
import time
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Callable, Optional

import gbuffer_model as gm
import numpy as np
import pytest

from cpppathtracer_amd import Renderer, camera_get_copy, scenes, types
from cpppathtracer_amd._lib import (CPT_RENDER_AUX, CPT_SCHEDULE_NO_CONSOLIDATE, CPT_TRAVERSAL_ORDERED)
from cpppathtracer_amd.texture_io import EnvTexture

pytestmark = pytest.mark.gpu

W, H, DEPTH, SEED = 64, 40, 8, 7
SPP = 256
KW = dict(ordered=True, consolidate=False)
WALK = CPT_TRAVERSAL_ORDERED
ADAPTIVE = CPT_TRAVERSAL_ORDERED | CPT_SCHEDULE_NO_CONSOLIDATE | CPT_RENDER_AUX
NPIX = W * H
BAND_BYTES = 16 * (H // 16) * W * 4   # the display band of a full frame: rows 0 .. 16 * (H / 16)


def assert_overlap(name, t_launch, t_call, render_ms):
    """The overlap condition of the module docstring (also used by test_gpu_edit_fuzz.py)."""
    gap_ms = 1e3 * (t_call - t_launch)
    print(f"{name}: the call began {gap_ms:.3f} ms after the launch of a render of {render_ms:.2f} ms")
    assert render_ms >= 4 * gap_ms, (f"{name}: the call began {gap_ms:.3f} ms after the launch of a render of "
                                     f"{render_ms:.3f} ms: no overlap is shown")


class Synced:
    """The twin's view of a Renderer: render() with sync=True, and after every call the context's
    synchronize() and the device's."""

    def __init__(self, r):
        self._r = r

    def __getattr__(self, name):
        f = getattr(self._r, name)
        if not callable(f):
            return f

        def call(*a, **k):
            import torch
            if name == "render":
                k["sync"] = True
            out = f(*a, **k)
            self._r.synchronize()
            torch.cuda.synchronize()
            return out
        return call


# ------------------------------------------------------------------------------- the data
def _near(objs):
    """The scene moved to the look-at point, where the camera sees its objects."""
    out = objs.copy()
    out["center"][1:, 2] += np.float32(470.0)
    return out


@pytest.fixture(scope="module")
def shared(sky):
    import torch  # noqa: F401  (load torch's HIP runtime first: one runtime per process)
    rng = np.random.default_rng(0x6173796E)
    cam = camera_get_copy(scenes.camera_for(W, H))
    objs = scenes.scene_s1000(n=150)
    red = types.make_material(types.DIFFUSE, kd=(0.9, 0.2, 0.2))
    rays_o, rays_d = gm.camera_rays(cam)
    pick = np.linspace(0, NPIX - 1, 64).astype(np.int64)
    moments = rng.random((4, NPIX), dtype=np.float32)
    moments[2] = np.float32(3.0)
    return SimpleNamespace(
        cam=cam, objs=objs, sky=sky,
        sky_inverted=EnvTexture(255 - sky.rgba, sky.width, sky.height),
        sky_smaller=EnvTexture(np.ascontiguousarray(sky.rgba[::2, ::2]), sky.width // 2, sky.height // 2),
        sky_larger=EnvTexture(np.ascontiguousarray(np.tile(sky.rgba[::-1], (2, 1, 1))), sky.width, 2 * sky.height),
        objs_same_count=_near(scenes.scene_s1000(seed=77, n=150)),
        objs_larger=_near(scenes.scene_s1000(n=400)),
        one_object=types.make_object(types.SPHERE, red, center=(0.0, 20.0, 0.0), radius=20.0),
        some_indices=np.array([1, 2, 3, 4], dtype=np.int32),
        some_objects=_near(scenes.scene_s1000(seed=5, n=150))[[10, 11, 12, 13]],
        accum=rng.random((NPIX, 4), dtype=np.float32),
        rng_planes=rng.integers(1, 2 ** 32, size=(6, NPIX), dtype=np.uint32),
        normal=rng.standard_normal((NPIX, 3)).astype(np.float32), depth=rng.random(NPIX, dtype=np.float32),
        moments=moments,
        rays=(rays_o[pick], rays_d[pick]),
        texture=scenes.synthetic_texture(9))


@pytest.fixture(scope="module")
def oracle_first(oracle_mod, shared):
    """The oracle's (accumulator, RNG end states) of the module's workload, once."""
    rows = np.arange(H, dtype=np.int32)
    rng = oracle_mod.init_rng(SEED, W, rows, threads=8)
    acc, _, _, _ = oracle_mod.render(shared.objs, shared.cam, shared.sky, rows, SPP, DEPTH, rng, threads=8)
    return acc, rng


# ---------------------------------------------------------------------------- the read-outs
READERS = {
    "accum": lambda r: r.read_accum(),
    "rng": lambda r: r.read_rng(),
    "aux": lambda r: r.read_aux(),
    "moments": lambda r: r.read_moments(),
    "noise": lambda r: r.read_noise(),
    "adaptive_info": lambda r: r.adaptive_info(),
    "filtered": lambda r: r.read_filtered(),
    "gbuffer": lambda r: r.read_gbuffer(),
    "mix": lambda r: r.read_mix(),
    "stats": lambda r: r.stats(),
    "counters": lambda r: r.raw_counters(),
    "previous_order": lambda r: r.debug_tile_order(1),
    "nodes": lambda r: r.read_nodes(),
    "bvh": lambda r: r.bvh_export(),
    "walk_info": lambda r: r.walk_info(),
}
IMAGE = ("accum", "rng")


def _flat(prefix, v, out):
    if isinstance(v, dict):
        for k, x in v.items():
            _flat(f"{prefix}.{k}", x, out)
    elif isinstance(v, (tuple, list)):
        for i, x in enumerate(v):
            _flat(f"{prefix}.{i}", x, out)
    elif v is not None:
        out[prefix] = np.atleast_1d(np.ascontiguousarray(v))


def _assert_same_bits(got, want):
    assert list(got) == list(want)
    for k in got:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1))
            raise AssertionError(f"{k}: {np.unique(bad // a.itemsize).size} of {a.size} values differ from the "
                                 f"synchronised twin's")


# ------------------------------------------------------------------------------- the cases
@dataclass
class Case:
    name: str
    call: Callable                       # (r, e) -> what the call under test returned
    reads: tuple = IMAGE                 # READERS to compare after the final synchronise
    render: dict = field(default_factory=dict)   # further arguments of the render in flight
    before: Optional[Callable] = None    # (r, e): steps before the render in flight
    then: Optional[Callable] = None      # (r, e): steps after the read-out; `reads` are read again
    scene: str = "s1000"
    pinned: bool = True                  # the render in flight is the module's workload (oracle_first)
    rerecords: bool = False              # the call records the render's timing events again
    changes_image: bool = False          # `then` renders a different image (asserted on the twin)


def _again(r, e):
    """The next render, which must see what the call left."""
    r.render(e.cam, SPP, DEPTH, sync=True, **KW)


def _second(**kw):
    def call(r, e):
        r.render(e.cam, SPP, DEPTH, accumulate=True, **dict(KW, **kw))
    return call


def _stream(r, e):
    import torch
    e.ts = torch.cuda.Stream()


def _on_stream(r, e):
    _stream(r, e)
    r.set_stream(e.ts.cuda_stream)


def _device_buffer(nbytes):
    def before(r, e):
        import torch
        _stream(r, e)
        e.buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
    return before


def _copied(r, e):
    e.ts.synchronize()
    return e.buf.cpu().numpy()


def _copy_accum(r, e):
    r.copy_accum_device(e.buf.data_ptr(), NPIX * 16, e.ts.cuda_stream)
    return _copied(r, e)


def _display_copy(r, e):
    r.denoise_mix(1, host=False)
    r.copy_bgra_device(e.buf.data_ptr(), BAND_BYTES, e.ts.cuda_stream)
    return _copied(r, e)


def _display_once(r, e):
    r.render(e.cam, 1, DEPTH, aux=True, sync=True, **KW)
    r.denoise_mix(1)
    r.init_rng(SEED)


def _adaptive_filter(r, e):
    info = r.render_adaptive(e.cam, 4, 16, 2, 0.05, DEPTH, flags=ADAPTIVE)
    r.filter_frame()
    return info


def _switch_render_read(stream_of):
    def call(r, e):
        r.set_stream(stream_of(e))
        r.render(e.cam, SPP, DEPTH, accumulate=True, **KW)
        return r.read_accum(), r.read_rng()
    return call


def _set_stream_and_read(stream_of):
    def call(r, e):
        r.set_stream(stream_of(e))
        return r.read_accum(), r.read_rng()
    return call


AUX = dict(aux=True)
CASES = [
    # A. inputs of the render in flight: its image is the one from before the call, the next one from after
    Case("A-set_env-same-geometry", lambda r, e: r.set_env(e.sky_inverted), then=_again, changes_image=True),
    Case("A-set_env-smaller", lambda r, e: r.set_env(e.sky_smaller), then=_again, changes_image=True),
    Case("A-set_env-larger", lambda r, e: r.set_env(e.sky_larger), then=_again, changes_image=True),
    Case("A-bind_texture", lambda r, e: r.bind_texture(1, e.texture), then=_again, changes_image=True, scene="s4_textured",
         pinned=False),
    Case("A-set_scene-same-count", lambda r, e: r.set_scene(e.objs_same_count), IMAGE + ("nodes", "bvh", "walk_info"),
         then=_again, changes_image=True),
    Case("A-set_scene-larger", lambda r, e: r.set_scene(e.objs_larger), IMAGE + ("nodes", "bvh", "walk_info"), then=_again,
         changes_image=True),
    Case("A-update_object", lambda r, e: r.update_object(3, e.one_object), IMAGE + ("nodes", "bvh"), then=_again,
         changes_image=True),
    Case("A-update_objects-rebuild", lambda r, e: r.update_objects(e.some_indices, e.some_objects, rebuild=True),
         IMAGE + ("nodes", "bvh", "walk_info"), then=_again, changes_image=True),
    # B. outputs of the render in flight: the call wins, the state afterwards is what it wrote
    Case("B-write_accum", lambda r, e: r.write_accum(e.accum)),
    Case("B-write_rng", lambda r, e: r.write_rng(e.rng_planes), then=_again),
    Case("B-write_aux", lambda r, e: r.write_aux(e.normal, e.depth), IMAGE + ("aux",), render=AUX),
    Case("B-clear_accum", lambda r, e: r.clear_accum()),
    Case("B-init_rng", lambda r, e: r.init_rng(SEED + 1), then=_again),
    Case("B-set_frame-same-size", lambda r, e: r.set_frame(W, H)),
    Case("B-set_frame-other-size", lambda r, e: r.set_frame(48, 24)),
    Case("B-reset_display", lambda r, e: r.reset_display(), IMAGE + ("aux", "mix"), render=AUX, before=_display_once,
         then=lambda r, e: r.denoise_mix(1)),
    Case("B-write_moments", lambda r, e: r.write_moments(e.moments), IMAGE + ("moments", "noise", "adaptive_info"),
         before=lambda r, e: r.render_adaptive(e.cam, 4, 8, 2, 0.05, DEPTH, flags=ADAPTIVE), pinned=False),
    # C. more work queued behind it
    Case("C-render-wavefront", _second(path="wavefront"), rerecords=True),
    Case("C-render-cost-schedule", _second(schedule="cost"), rerecords=True),
    Case("C-render-previous-schedule", _second(schedule="previous"), IMAGE + ("previous_order",), rerecords=True),
    Case("C-tile_costs", lambda r, e: r.tile_costs(e.cam, 2, DEPTH, ordered="plain")),
    Case("C-gbuffer", lambda r, e: (r.gbuffer(e.cam, WALK), r.read_gbuffer())[1], IMAGE + ("gbuffer",)),
    Case("C-trace_rays", lambda r, e: r.trace_rays(*e.rays, flags=WALK)),
    Case("C-pick", lambda r, e: r.pick(e.cam, 32, 30, WALK)),
    Case("C-denoise_mix", lambda r, e: r.denoise_mix(1), IMAGE + ("aux", "mix"), render=AUX),
    Case("C-render_adaptive-filter_frame", _adaptive_filter, IMAGE + ("aux", "moments", "noise", "filtered"), render=AUX,
         rerecords=True),
    Case("C-copy_accum_device", _copy_accum, before=_device_buffer(NPIX * 16)),
    Case("C-copy_bgra_device", _display_copy, IMAGE + ("aux", "mix"), render=AUX, before=_device_buffer(BAND_BYTES)),
    # D. reads made directly behind the render return the finished render's values
    Case("D-read_accum", lambda r, e: r.read_accum()),
    Case("D-read_rng", lambda r, e: r.read_rng()),
    Case("D-read_aux", lambda r, e: r.read_aux(), IMAGE + ("aux",), render=AUX),
    Case("D-stats", lambda r, e: (r.stats(), r.raw_counters()), IMAGE + ("stats", "counters"), render=dict(stats=True),
         before=lambda r, e: r.reset_stats()),
    Case("D-debug_tile_order", lambda r, e: r.debug_tile_order(1), IMAGE + ("previous_order",),
         render=dict(schedule="previous")),
    Case("D-read_nodes", lambda r, e: r.read_nodes(), IMAGE + ("nodes",)),
    Case("D-bvh_export", lambda r, e: r.bvh_export(), IMAGE + ("bvh",)),
    # E. streams
    Case("E-own-to-user-stream", _switch_render_read(lambda e: e.ts.cuda_stream), before=_stream, rerecords=True),
    Case("E-user-to-own-stream", _switch_render_read(lambda e: None), before=_on_stream, rerecords=True),
    Case("E-own-to-user-stream-read", _set_stream_and_read(lambda e: e.ts.cuda_stream), before=_stream),
    Case("E-user-to-own-stream-read", _set_stream_and_read(lambda e: None), before=_on_stream),
    Case("E-same-own-stream", _set_stream_and_read(lambda e: None)),
    Case("E-same-user-stream", _set_stream_and_read(lambda e: e.ts.cuda_stream), before=_on_stream),
]


def _setup(r, e, scene):
    if scene == "s4_textured":
        for h in (1, 2, 3):
            r.bind_texture(h, scenes.synthetic_texture(h))
        r.set_scene(scenes.scene_s4_textured())
    else:
        r.set_scene(e.objs)
    r.set_env(e.sky)
    r.set_frame(W, H)
    r.init_rng(SEED)


def _run(case, shared, twin):
    """The case on a fresh context: ({what was read: bits}, (t_launch, t_call, render_ms), the
    twin's first image)."""
    e = SimpleNamespace(**vars(shared))
    got, first = {}, None
    raw = Renderer(0)
    try:
        r = Synced(raw) if twin else raw
        _setup(r, e, case.scene)
        if case.before:
            case.before(r, e)
        raw.synchronize()
        t_launch = time.perf_counter()
        r.render(e.cam, SPP, DEPTH, **KW, **case.render)
        t_call = time.perf_counter()
        if twin:
            first = raw.read_accum(), raw.read_rng(), raw.last_render_ms()
        _flat("call", case.call(r, e), got)
        raw.synchronize()
        render_ms = raw.last_render_ms()
        for k in case.reads:
            _flat(k, READERS[k](raw), got)
        if case.then:
            _flat("then.call", case.then(r, e), got)
            raw.synchronize()
            for k in case.reads:
                _flat(f"then.{k}", READERS[k](raw), got)
    finally:
        raw.close()   # before `e` goes: the context waits for a stream of the case's
    return got, (t_launch, t_call, render_ms), first


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_call_behind_a_render_in_flight(shared, oracle_first, case):
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    want, _, first = _run(case, shared, twin=True)   # first: the kernels are loaded when the subject launches
    if case.pinned:
        np.testing.assert_array_equal(first[1], oracle_first[1])
        np.testing.assert_array_equal(first[0].view(np.uint32), oracle_first[0].view(np.uint32))
    if case.changes_image:
        assert want["then.accum"].tobytes() != first[0].tobytes(), "the call does not change the image: a vacuous case"
    got, (t_launch, t_call, render_ms), _ = _run(case, shared, twin=False)
    assert_overlap(case.name, t_launch, t_call, first[2] if case.rerecords else render_ms)
    _assert_same_bits(got, want)


# ----------------------------------------------------------------------------- F. two contexts
def _tiles(shared, twin):
    wrap = Synced if twin else (lambda r: r)
    raws = [Renderer(0) for _ in range(3)]
    for r, rows, seed in zip(raws, (None, np.arange(0, 20), np.arange(20, 40)), (SEED + 1, SEED, SEED)):
        r = wrap(r)
        r.set_scene(shared.objs)
        r.set_env(shared.sky)
        r.set_frame(W, H, rows)
        r.init_rng(seed)
    return raws, [wrap(r) for r in raws]


def _gather(shared, busy, staged, twin):
    raws, (dst, a, b) = _tiles(shared, twin)
    try:
        cam = shared.cam
        dst.set_debug_gather(staged)
        a.render(cam, SPP, DEPTH, aux=True, sync=True, **KW)
        if busy == "src":
            # the source's render in flight; and its later work (a clear) stays behind the stitch
            dst.render(cam, 1, DEPTH, aux=True, sync=True, **KW)
            t_launch = time.perf_counter()
            b.render(cam, SPP, DEPTH, aux=True, **KW)
            t_call = time.perf_counter()
            dst.gather_rows(b)
            b.clear_accum()
            dst.gather_rows(a)
            timed = raws[2]
        else:
            # the destination's own render of the whole frame in flight: the stitch of rows 20-40 lands on it
            b.render(cam, SPP, DEPTH, aux=True, sync=True, **KW)
            t_launch = time.perf_counter()
            dst.render(cam, SPP, DEPTH, aux=True, **KW)
            t_call = time.perf_counter()
            dst.gather_rows(b)
            timed = raws[0]
        for r in raws:
            r.synchronize()
        got = {}
        _flat("dst", {k: READERS[k](raws[0]) for k in IMAGE + ("aux",)}, got)
        _flat("b", {k: READERS[k](raws[2]) for k in IMAGE + ("aux",)}, got)
        got["mode"] = np.frombuffer(raws[0].last_gather_mode(b).encode(), dtype=np.uint8)
        return got, (t_launch, t_call, timed.last_render_ms())
    finally:
        for r in raws:
            r.close()


@pytest.mark.parametrize("staged", [0, 1], ids=["same-device", "staged"])
@pytest.mark.parametrize("busy", ["src", "dst"])
def test_gather_behind_a_render_in_flight(shared, busy, staged):
    """dst.gather_rows(src) while src's render of its row tile is in flight, and while dst itself
    has a render in flight, through the same-device stitch and through the staged copy."""
    import torch  # noqa: F401
    want, _ = _gather(shared, busy, staged, twin=True)
    got, (t_launch, t_call, render_ms) = _gather(shared, busy, staged, twin=False)
    assert want["mode"].tobytes().decode() == ("staged" if staged else "same_device")
    assert_overlap(f"F-gather-{busy}-busy", t_launch, t_call, render_ms)
    _assert_same_bits(got, want)
    if busy == "src":
        assert not want["b.accum"].any()   # the clear queued behind the gather ran, after the stitch
