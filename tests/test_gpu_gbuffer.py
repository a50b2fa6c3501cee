"""cpt_gbuffer, cpt_trace_rays and cpt_pick against their numpy restatement (tests/gbuffer_model.py,
pinned to the oracle by tests/test_gbuffer_model.py): object id, distance, normal and albedo bit for
bit under the three walks, on the render's own first hits, through refits, and what the queries
must leave alone.
"""
import re
import subprocess

import gbuffer_model as gm
import numpy as np
import pytest

from cpppathtracer_amd import CptError, camera_get_copy, scenes
from cpppathtracer_amd._lib import CPT_RENDER_AUX, CPT_RENDER_STATS, CPT_TRAVERSAL_ORDERED, CPT_TRAVERSAL_PLAIN_LEAVES

pytestmark = pytest.mark.gpu

FIXTURES = gm.fixtures()
WALKS = {"reference": 0, "ordered": CPT_TRAVERSAL_ORDERED, "plain": CPT_TRAVERSAL_ORDERED | CPT_TRAVERSAL_PLAIN_LEAVES}
INVALID, STATE = 1, 5
LDS_TREE_NODES = 512   # cpt_internal.hpp: wide nodes staged in LDS
RAY_COUNTS = (1, 63, 64, 65, 4097)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_equal(got, want, what, albedo=True):
    """got: a read_gbuffer / trace_rays dict; want: the model's (id, t, normal, albedo)."""
    np.testing.assert_array_equal(got["id"], want[0], err_msg=what + " id")
    np.testing.assert_array_equal(_bits(got["t"]), _bits(want[1]), err_msg=what + " t")
    np.testing.assert_array_equal(_bits(got["normal"]), _bits(want[2]), err_msg=what + " normal")
    if albedo:
        np.testing.assert_array_equal(_bits(got["albedo"]), _bits(want[3]), err_msg=what + " albedo")


def _model(oracle_mod, name):
    """A fixture's camera copy and model G-buffer, computed once and shared (read only)."""
    if name not in _cache:
        objs, cam0, rows = FIXTURES[name]
        cam = camera_get_copy(cam0)
        _cache[name] = (cam, gm.gbuffer(oracle_mod, objs, cam, rows))
    return _cache[name]


def _setup(gpu, name):
    objs, cam0, rows = FIXTURES[name]
    gpu.set_scene(objs)
    gpu.set_env(None)
    gpu.set_frame(int(cam0["width"]), int(cam0["height"]), rows)
    return objs


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_gbuffer_equals_the_model(gpu, oracle_mod, name):
    """id, t, normal and albedo of every pixel, under the reference walk, the ordered walk (the
    4-wide walk on the LDS image where the scene has one) and the ordered walk with plain leaves."""
    _setup(gpu, name)
    cam, want = _model(oracle_mod, name)
    if name == "fuzz_hyb_48x32":
        assert gpu.walk_info()["n_wide"] > LDS_TREE_NODES   # the global-memory half of the hybrid node load
    if name == "s1000_96x64":
        assert 0 < gpu.walk_info()["n_wide"] <= LDS_TREE_NODES
    if name == "empty_16x8":
        assert (want[0] == -1).all() and (want[1] == gm.TMAX).all() and (want[3] == 0).all()
        np.testing.assert_array_equal(want[2], -gm.camera_rays(cam)[1])
    first = None
    for walk, flags in WALKS.items():
        gpu.gbuffer(cam, flags)
        got = gpu.read_gbuffer()
        _assert_equal(got, want, f"{name} {walk}")
        assert gpu.last_query_ms() > 0.0
        if first is None:
            first = got
        for k in first:
            np.testing.assert_array_equal(_bits(got[k]), _bits(first[k]), err_msg=f"{name} {walk} vs reference: {k}")


@pytest.mark.parametrize("name", ["s4_64x48", "s1000_96x64", "s4_rows"])
def test_gbuffer_normal_is_the_renders_first_hit(gpu, sky, name):
    """A 1-spp, depth-1 render with CPT_RENDER_AUX at lens_radius 0 leaves 0.f + the first hit's
    normal in the aux buffer: the G-buffer's normal, bit for bit."""
    objs, cam0, rows = FIXTURES[name]
    gpu.set_scene(objs)
    gpu.set_env(sky)
    W, H = int(cam0["width"]), int(cam0["height"])
    gpu.set_frame(W, H, rows)
    gpu.init_rng(scenes.DEFAULT_SEED)
    cam = camera_get_copy(cam0)
    for walk, flags in WALKS.items():
        gpu.render(cam, 1, 1, aux=True, sync=True, flags=flags)
        normal, _ = gpu.read_aux()
        gpu.gbuffer(cam, flags)
        g = gpu.read_gbuffer()
        np.testing.assert_array_equal(_bits(np.float32(0.0) + g["normal"]), _bits(normal), err_msg=f"{name} {walk}")


def _hashed(seed, n, k):
    """[n, k] floats in [0, 1) from a 64-bit mix of (seed, index): a hashed generator, no state."""
    base = np.uint64((seed * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        z = (np.arange(n * k, dtype=np.uint64) + base) * np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(31)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(29)
    return ((z >> np.uint64(40)).astype(np.float32) / np.float32(1 << 24)).reshape(n, k)


def explicit_rays(objs, seed, n=4097):
    """(origins, dirs, tmin) [n]: hand-placed rays first (inside a sphere: the second root; along a
    cylinder's axis from above and below: its caps, two zero components; parallel to the platform:
    a miss of it, one zero component; axis directions; non-unit directions; one ray from just above
    a surface with tmin 0 and again with the bounce tmin, which skips that surface), then hashed
    rays from outside and inside the scene toward points in it, a third of them non-unit, half of
    them with the bounce tmin.  All inputs finite."""
    F = np.float32
    sph = [o for o in objs if int(o["type"]) == gm.SPHERE]
    cyl = [o for o in objs if int(o["type"]) == gm.CYLINDER]
    O, D, T = [], [], []

    def add(o, d, tmin=0.0):
        O.append(np.asarray(o, dtype=np.float32))
        D.append(np.asarray(d, dtype=np.float32))
        T.append(F(tmin))

    s = sph[0]
    sc, sr = np.asarray(s["center"], dtype=np.float32), F(s["radius"])
    add(sc + sr * np.array([0.3, -0.2, 0.1], dtype=np.float32), (0.5, 0.7, -0.4))          # inside: second root
    add(sc + sr * np.array([0.0, 0.5, 0.0], dtype=np.float32), (0.0, 0.0, 1.0))            # inside, two zero components
    # just above the platform (y_pos 0): t = 1e-5 / 1 lies between the two tmin values
    add((3.0, 1e-5, -7.0), (0.25, -1.0, 0.125), 0.0)
    add((3.0, 1e-5, -7.0), (0.25, -1.0, 0.125), gm.BOUNCE_TMIN)
    # on a sphere's top (origin exactly on the surface), going in: root 1 is 0 or tiny, root 2 the far side
    add(sc + np.array([0.0, sr, 0.0], dtype=np.float32), (0.0, -1.0, 0.0), 0.0)
    add(sc + np.array([0.0, sr, 0.0], dtype=np.float32), (0.0, -1.0, 0.0), gm.BOUNCE_TMIN)
    add((-300.0, 5.0, 2.0), (1.0, 0.0, 0.5))                                                # parallel to the platform
    add((-300.0, 5.0, 2.0), (4.0, 0.0, 0.0))                                                # two zero components, non-unit
    add((0.0, 200.0, 0.0), (0.0, -0.01, 0.0))                                               # straight down, |d| = 0.01
    add((10.0, 40.0, -600.0), (0.0, -0.05, 1.0))                                            # d.x == 0
    add((-200.0, 30.0, 10.0), (3.0, -0.4, 0.0))                                             # d.z == 0
    for c in cyl[:3]:
        cc, h = np.asarray(c["center"], dtype=np.float32), F(c["height"])
        add(cc + np.array([0.0, h + 5.0, 0.0], dtype=np.float32), (0.0, -1.0, 0.0))        # the axis, from above: upper cap
        add(cc - np.array([0.0, h + 5.0, 0.0], dtype=np.float32), (0.0, 2.5, 0.0))         # from below the floor: lower cap
        add(cc + np.array([F(c["radius"]) * F(0.5), 0.0, 0.0], dtype=np.float32), (0.0, 1.0, 0.0))   # inside, up: upper cap from within
        add(cc + np.array([0.0, 0.0, 0.0], dtype=np.float32), (1.0, 0.0, 0.0))             # inside, level: the side's second root
    m = n - len(O)
    centre = np.asarray(objs["center"], dtype=np.float32).reshape(-1, 3)[1:]
    lo, hi = centre.min(axis=0) - F(20), centre.max(axis=0) + F(20)
    lo[1], hi[1] = F(0.5), F(45.0)
    u = _hashed(seed, m, 12)
    target = lo + u[:, 0:3] * (hi - lo)
    inside = lo + u[:, 3:6] * (hi - lo)
    shell = np.stack([(u[:, 3] - F(0.5)) * F(900.0), F(20.0) + u[:, 4] * F(150.0), (u[:, 5] - F(0.5)) * F(1500.0)], axis=1)
    origin = np.where((u[:, 6] < 0.5)[:, None], inside, shell).astype(np.float32)
    d = (target - origin).astype(np.float32)
    unit = d / np.sqrt((d * d).sum(axis=1, dtype=np.float32), dtype=np.float32)[:, None]
    scale = np.where(u[:, 7] < 1.0 / 3.0, F(0.01) + u[:, 8] * F(8.0), F(1.0)).astype(np.float32)
    d = np.where((u[:, 9] < 0.5)[:, None], unit * scale[:, None], d).astype(np.float32)   # the rest: unnormalised as they are
    tm = np.where(u[:, 10] < 0.5, gm.BOUNCE_TMIN, F(0.0)).astype(np.float32)
    Oa = np.concatenate([np.stack(O), origin]).astype(np.float32)
    Da = np.concatenate([np.stack(D), d]).astype(np.float32)
    Ta = np.concatenate([np.array(T, dtype=np.float32), tm])
    assert Oa.shape == (n, 3) and np.isfinite(Oa).all() and np.isfinite(Da).all() and (np.abs(Da).sum(axis=1) > 0).all()
    return Oa, Da, Ta


@pytest.mark.parametrize("scene", ["s4", "s1000"])
def test_trace_rays_equal_the_model(gpu, oracle_mod, scene):
    """1, 63, 64, 65 and 4097 explicit rays (an under-full last wave each time but one), under the
    three walks; tmin NULL is tmin 0."""
    objs = scenes.SCENES[scene]()
    gpu.set_scene(objs)
    O, D, T = explicit_rays(objs, 20261020 + len(objs))
    want = gm.first_hit(oracle_mod, objs, O, D, T)
    # the set holds what it must
    assert ((D == 0).sum(axis=1) == 1).any() and ((D == 0).sum(axis=1) == 2).any()
    assert (np.abs((D * D).sum(axis=1) - 1) > 0.1).any() and (T == 0).any() and (T == gm.BOUNCE_TMIN).any()
    assert (want[0] == -1).any() and (want[0] >= 0).any()
    assert want[0][2] == 0 and want[0][3] != 0   # the bounce tmin skips the platform the ray starts on
    assert (want[0] > 0).sum() > 100             # spheres / cylinders, not only the floor
    for n in RAY_COUNTS:
        for walk, flags in WALKS.items():
            got = gpu.trace_rays(O[:n], D[:n], T[:n], flags=flags)
            _assert_equal(got, tuple(w[:n] for w in want), f"{scene} n={n} {walk}", albedo=False)
    zero = gm.first_hit(oracle_mod, objs, O[:65], D[:65], None)
    _assert_equal(gpu.trace_rays(O[:65], D[:65], None, flags=CPT_TRAVERSAL_ORDERED), zero, f"{scene} tmin NULL", albedo=False)


def _edits(objs):
    """Three S4 objects moved (one enlarged): (indices, new objects)."""
    idx = [1, 3, 2]
    new = np.array([objs[i] for i in idx], dtype=objs.dtype)
    new[0]["center"] = np.array([-20.0, 22.0, 18.0], dtype=np.float32)
    new[1]["center"] = np.array([30.0, 9.0, -25.0], dtype=np.float32)
    new[1]["radius"] = np.float32(9.0)
    new[2]["center"] = np.array([5.0, 15.0, 40.0], dtype=np.float32)
    return idx, new


@pytest.mark.parametrize("rebuild", [False, True])
def test_ids_survive_refit_and_rebuild(gpu, oracle_mod, rebuild):
    """After update_objects moves three S4 objects the G-buffer and ray queries equal the model on
    the edited objects, with ids still in set_scene's order (the reference tree keeps its topology,
    so the model's reference order is that of the objects as built)."""
    objs = _setup(gpu, "s4_64x48")
    cam, before = _model(oracle_mod, "s4_64x48")
    idx, new = _edits(objs)
    gpu.update_objects(idx, new, rebuild=rebuild)
    edited = objs.copy()
    for i, o in zip(idx, new):
        edited[i] = o
    order = gm.reference_order(oracle_mod, objs)
    O, D = gm.camera_rays(cam)
    want = gm.first_hit(oracle_mod, edited, O, D, order=order)
    assert (want[0] != before[0]).any()
    for walk, flags in WALKS.items():
        gpu.gbuffer(cam, flags)
        _assert_equal(gpu.read_gbuffer(), want, f"edited {walk}")
    Oe, De, Te = explicit_rays(objs, 7, n=257)
    _assert_equal(gpu.trace_rays(Oe, De, Te, flags=CPT_TRAVERSAL_ORDERED), gm.first_hit(oracle_mod, edited, Oe, De, Te, order=order),
                  "edited rays", albedo=False)


def test_queries_leave_the_frame_state_alone(gpu, sky):
    """After an adaptive S4 render and filter_frame, gbuffer, trace_rays and pick change none of
    the accumulator, RNG states, aux buffers, moments and filtered planes, and the next render is
    the one a context without the calls makes."""
    W = H = 64
    objs = scenes.scene_s4()
    cam = camera_get_copy(scenes.camera_for(W, H))
    O, D, T = explicit_rays(objs, 3, n=300)

    def run(queries):
        gpu.set_scene(objs)
        gpu.set_env(sky)
        gpu.set_frame(W, H)
        gpu.init_rng(scenes.DEFAULT_SEED)
        gpu.render_adaptive(cam, 8, 32, 4, 0.1, 8, flags=CPT_RENDER_AUX | CPT_TRAVERSAL_ORDERED)
        gpu.filter_frame()
        gpu.reset_stats()

        def state():
            return [gpu.read_accum(), gpu.read_rng(), *gpu.read_aux(), gpu.read_moments(), *gpu.read_filtered()]
        s0 = state()
        if queries:
            for flags in WALKS.values():
                gpu.gbuffer(cam, flags)
                gpu.trace_rays(O, D, T, flags=flags)
                gpu.pick(cam, W // 2, H // 2, flags)
            gpu.read_gbuffer()
            for a, b in zip(s0, state()):
                np.testing.assert_array_equal(_bits(a), _bits(b))
        gpu.render(cam, 2, 8, accumulate=True, aux=True, sync=True, ordered=True)
        return state()

    for a, b in zip(run(False), run(True)):
        np.testing.assert_array_equal(_bits(a), _bits(b))


def test_pick_is_the_gbuffers_pixel(gpu, oracle_mod):
    """pick at the four corner pixels and the centre: the G-buffer's id and t there; on a row-list
    frame too, for rows the context does not render."""
    _setup(gpu, "s4_64x48")
    cam, want = _model(oracle_mod, "s4_64x48")
    W, H = 64, 48
    pixels = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)]
    for walk, flags in WALKS.items():
        gpu.gbuffer(cam, flags)
        g = gpu.read_gbuffer()
        for x, y in pixels:
            obj, t = gpu.pick(cam, x, y, flags)
            assert obj == g["id"][y * W + x] == want[0][y * W + x], (walk, x, y)
            assert np.float32(t).view(np.uint32) == g["t"][y * W + x].view(np.uint32), (walk, x, y)
    assert gpu.last_query_ms() > 0.0
    gpu.set_frame(W, H, [5, 2, 40])
    for x, y in pixels:
        obj, t = gpu.pick(cam, x, y, CPT_TRAVERSAL_ORDERED)
        assert obj == want[0][y * W + x] and np.float32(t).view(np.uint32) == want[1][y * W + x].view(np.uint32)


def _status(fn, *args, **kw):
    with pytest.raises(CptError) as e:
        fn(*args, **kw)
    return e.value.status


def test_argument_and_state_errors(gpu):
    import ctypes
    from cpppathtracer_amd import Renderer
    W, H = 64, 48
    cam = camera_get_copy(scenes.camera_for(W, H))
    with Renderer(0) as r:
        r.set_scene(scenes.scene_s4())
        assert _status(r.pick, cam, 0, 0) == STATE            # no frame
        assert _status(r.gbuffer, cam) == STATE
        r.trace_rays(np.zeros((1, 3)), np.ones((1, 3)))       # needs only a scene
        r.set_frame(W, H)
        assert _status(r.read_gbuffer) == STATE               # before any gbuffer
        for x, y in ((-1, 0), (W, 0), (0, -1), (0, H)):
            assert _status(r.pick, cam, x, y) == INVALID
        for bad in (CPT_RENDER_AUX, CPT_RENDER_STATS, 0x100, 0x80000000):
            assert _status(r.pick, cam, 1, 1, bad) == INVALID
            assert _status(r.gbuffer, cam, bad) == INVALID
            assert _status(r.trace_rays, np.zeros((1, 3)), np.ones((1, 3)), None, bad) == INVALID
        assert _status(r.gbuffer, camera_get_copy(scenes.camera_for(W, H + 1))) == INVALID
        assert _status(r.read_gbuffer) == STATE               # the failed calls queued nothing
        r.gbuffer(cam)
        ids = np.full(W * H, 77, dtype=np.int32)
        st = r._L.cpt_read_gbuffer(r._ctx, ctypes.c_void_p(ids.ctypes.data), None, None, None, W * H - 1)
        assert st == INVALID and (ids == 77).all()            # too small: nothing written
        assert r._L.cpt_read_gbuffer(r._ctx, ctypes.c_void_p(ids.ctypes.data), None, None, None, W * H) == 0
        assert (ids != 77).all()
        obj = ctypes.c_int32(55)
        assert r._L.cpt_pick(r._ctx, None, 0, 0, 0, ctypes.byref(obj), None) == INVALID and obj.value == 55
        assert r._L.cpt_trace_rays(r._ctx, 1, None, None, None, 0, None, None, None) == INVALID
        r.set_frame(W, H)
        assert _status(r.read_gbuffer) == STATE               # dropped by set_frame
    with Renderer(0) as r:
        r.set_frame(W, H)
        assert _status(r.gbuffer, cam) == STATE               # no scene
        assert _status(r.trace_rays, np.zeros((1, 3)), np.ones((1, 3))) == STATE


def test_gbuffer_refused_while_an_adaptive_render_is_pending(gpu, sky):
    W = H = 32
    cam = camera_get_copy(scenes.camera_for(W, H))
    gpu.set_scene(scenes.scene_s4())
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(1)
    gpu.adaptive_begin(cam, 4, 8, 2, 0.05, 4)
    try:
        assert _status(gpu.gbuffer, cam) == STATE
    finally:
        while gpu.adaptive_step():
            pass
    gpu.gbuffer(cam)
    assert gpu.read_gbuffer()["id"].shape == (W * H,)


def test_headless_pick_agrees(gpu):
    """The C++ API's Pick through the headless example: --pick on --scene s4 prints the Python
    pick's object and distance."""
    from cpppathtracer_amd import build as cbuild
    exe = cbuild.build_examples()
    W, H = 64, 36
    gpu.set_scene(scenes.scene_s4())
    gpu.set_frame(W, H)
    cam = camera_get_copy(scenes.camera_for(W, H))
    seen = set()
    for x, y in ((32, 18), (20, 20), (2, 2), (45, 19)):
        out = subprocess.run([exe, "--scene", "s4", "--width", str(W), "--height", str(H), "--pick", f"{x},{y}"],
                             capture_output=True, text=True, timeout=120, cwd=cbuild.REPO_DIR)
        assert out.returncode == 0, out.stderr
        m = re.search(r"pick \((\d+), (\d+)\): object (-?\d+), t (\S+)", out.stdout)
        assert m, out.stdout
        obj, t = gpu.pick(cam, x, y, CPT_TRAVERSAL_ORDERED)
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (x, y, obj), out.stdout
        assert np.float32(m.group(4)) == t, out.stdout
        seen.add(obj)
    assert len(seen) >= 2
