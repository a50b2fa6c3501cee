"""Deterministic scene / camera / material generators for the parity tests, beyond the three demo
scenes and the one camera pose (test_scene_fuzz.py checks the generators against the oracle on
the CPU; test_gpu_fuzz_parity.py renders them on the GPU).

Every generator is pure numpy on np.random.default_rng(fixed seed) and returns (objs, camera):
`objs` an OBJECT_DTYPE array, `camera` a CAMERA_DTYPE value still to go through
camera_get_copy.  Frames are at most 64 x 40 pixels; PARAMS gives each family's (spp, depth).
No expectation is stored: the oracle renders every case at test time.
"""
import numpy as np

from cpppathtracer_amd.types import (CYLINDER, DIFFUSE, GLASS, METAL, MIRROR, OBJECT_DTYPE, PLATFORM, SPHERE, TEST,
                                     make_camera, make_material, make_object)

F = np.float32

# (spp, depth) per family: <= 3 spp, depth <= 16
PARAMS = {
    "mixed": (2, 8),
    "mixed_large": (1, 8),
    "axis_aligned": (2, 8),
    "inside": (2, 16),
    "edge_materials": (3, 8),
    "edge_geometry": (2, 8),
    "degenerate_camera": (1, 4),
}

MIXED_SEEDS = list(range(101, 125))            # 24
AXIS_SEEDS = list(range(205, 215))             # 10: every view kind twice
INSIDE_SEEDS = list(range(300, 308))           # 8: every placement twice
MIXED_LARGE_SEEDS = [400]

AXIS_KINDS = ("+x", "-x", "+z", "-z", "level")
INSIDE_KINDS = ("glass_sphere", "diffuse_sphere", "cylinder", "below_platform")


def camera(W, H, origin, look_at, fov=30.0, lens_radius=0.0005, dist_to_focus=100.0, vup=(0.0, 1.0, 0.0)):
    c = make_camera(W, H, origin=origin, look_at=look_at)
    c["view_fov"] = F(fov)
    c["lens_radius"] = F(lens_radius)
    c["dist_to_focus"] = F(dist_to_focus)
    c["vup"] = np.asarray(vup, dtype=np.float32)
    return c


def _objs(items):
    out = np.zeros(len(items), dtype=OBJECT_DTYPE)
    for i, o in enumerate(items):
        out[i] = o
    return out


def _floor(mat, y=0.0):
    return make_object(PLATFORM, mat, center=(0.0, -10000.0, 0.0), radius=10000.0, y_pos=y)


# ------------------------------------------------------------------------------- mixed
def _mixed_materials(rng):
    n = int(rng.integers(6, 13))
    kinds = [DIFFUSE, METAL, MIRROR, GLASS, TEST] + [int(t) for t in rng.integers(0, 5, n - 5)]
    mats = []
    for t in kinds:
        refl = (0.0, 1.0, float(rng.random()))[int(rng.integers(0, 3))]
        emit = float(rng.uniform(0.5, 4.0)) if rng.random() < 1.0 / 3.0 else 0.0
        mats.append(make_material(t, kd=rng.random(3), refractive_index=rng.uniform(1.0, 3.2), emit_intensity=emit,
                                  smoothness=rng.uniform(0.0, 6.0), reflectivity=refl))
    return mats


def mixed(seed, n=None, cam=None):
    """8-60 overlapping and nested spheres / cylinders (some below the floor), 0-2 platforms at
    random heights, 6-12 materials over all five material types, a random camera on a shell
    around the scene.  `n` / `cam` override the primitive count and the camera."""
    rng = np.random.default_rng([0x6D69, seed])
    mats = _mixed_materials(rng)
    n = int(rng.integers(8, 61)) if n is None else n
    spread = 40.0 if n <= 60 else 90.0
    p_cyl = rng.uniform(0.2, 0.8)
    items = [_floor(mats[int(rng.integers(len(mats)))], y=rng.uniform(-5.0, 5.0)) for _ in range(int(rng.integers(0, 3)))]
    prev = None
    for k in range(n):
        mat = mats[(k if k < len(mats) else int(rng.integers(len(mats))))]
        if prev is not None and rng.random() < 0.2:
            c, r = prev[0] + rng.uniform(-0.3, 0.3, 3) * prev[1], prev[1] * rng.uniform(0.3, 0.8)   # nested
        else:
            c = np.array([rng.uniform(-spread, spread), rng.uniform(-8.0, 30.0), rng.uniform(-spread, spread)])
            r = rng.uniform(0.5, 12.0)
        if rng.random() < p_cyl:
            items.append(make_object(CYLINDER, mat, center=c, radius=r, height=rng.uniform(0.5, 25.0)))
        else:
            items.append(make_object(SPHERE, mat, center=c, radius=r))
        prev = (c, r)
    if cam is None:
        W, H = int(rng.integers(17, 64)), int(rng.integers(9, 40))
        W |= int(rng.integers(0, 2))   # odd half of the time; never a multiple of 64
        d = rng.standard_normal(3)
        d[1] = abs(d[1]) * 0.8 - 0.1 * np.linalg.norm(d)          # mostly above, sometimes below the floor
        origin = np.array([0.0, 10.0, 0.0]) + rng.uniform(90.0, 160.0) * d / np.linalg.norm(d)
        look_at = np.array([rng.uniform(-20, 20), rng.uniform(0, 20), rng.uniform(-20, 20)])
        cam = camera(W, H, origin, look_at, fov=rng.uniform(10.0, 90.0),
                     lens_radius=(0.0, 0.0005, 0.5)[int(rng.integers(0, 3))], dist_to_focus=rng.uniform(1.0, 300.0))
    return _objs(items), cam


def mixed_large(seed):
    """`mixed` with 260 primitives (a 4-wide walk tree) under an axis-aligned, zero-lens camera:
    the centre column and row rays carry exactly-zero direction components into the wide walk."""
    return mixed(seed, n=260, cam=camera(64, 40, (-200.0, 12.0, 4.0), (0.0, 12.0, 4.0), fov=50.0, lens_radius=0.0))


# ------------------------------------------------------------------------ axis_aligned
def axis_aligned(seed):
    """A zero-lens camera looking along +x, -x, +z or -z (origin and look-at differ in one
    coordinate: the centre column has a zero horizontal component and the centre row d.y == 0),
    or level along a diagonal (d.y == 0 on the centre row only); even W and H.  One sphere's box
    face lies at the camera's coordinate on each zeroed axis, one cylinder's cap plane passes
    through the camera's y, and a few more primitives sit on small dyadic coordinates."""
    rng = np.random.default_rng([0x6178, seed])
    kind = AXIS_KINDS[seed % len(AXIS_KINDS)]
    W, H = 2 * int(rng.integers(8, 33)), 2 * int(rng.integers(4, 21))
    D = float(rng.integers(60, 121))
    cy = float(rng.integers(2, 12)) + (0.5 if rng.random() < 0.5 else 0.0)   # the camera's height
    side = float(rng.integers(-6, 7))                                       # its coordinate on the zeroed horizontal axis
    mats = [make_material(DIFFUSE, kd=(0.9, 0.9, 0.9)),
            make_material(GLASS, kd=(1.0, 1.0, 1.0), refractive_index=1.5, smoothness=rng.uniform(1.0, 5.0)),
            make_material(METAL, kd=rng.random(3), smoothness=rng.uniform(0.5, 4.0)),
            make_material(MIRROR, kd=rng.random(3), smoothness=rng.uniform(0.5, 4.0), reflectivity=rng.random()),
            make_material(DIFFUSE, kd=rng.random(3), emit_intensity=1.5)]
    # (a, b, y): a along the view axis, b along the other horizontal axis
    prims = [("s", 10.0, side + 5.0, cy, 5.0, 0.0),            # box face b = side (the camera's)
             ("s", -6.0, side - 9.0, cy - 3.0, 3.0, 0.0),      # box top y = cy
             ("c", -20.0, side - 2.0, cy - 2.0, 4.0, 4.0),     # upper cap plane y = cy
             ("c", 22.0, side + 4.0, cy + 1.5, 4.0, 3.0)]      # lower cap plane y = cy; side face b = side
    for _ in range(int(rng.integers(3, 9))):
        prims.append(("s" if rng.random() < 0.5 else "c", float(rng.integers(-30, 31)), side + float(rng.integers(-14, 15)),
                      float(rng.integers(0, 24)) * 0.5, float(rng.integers(1, 7)), float(rng.integers(1, 9))))
    if kind == "level":
        s = D * 0.75   # 3-4-5 like diagonal: both horizontal components nonzero
        origin, look_at = (-s, cy, side - D), (0.0, cy, side)
        place = lambda a, b: (b, a)   # noqa: E731
    elif kind in ("+x", "-x"):
        sgn = 1.0 if kind == "+x" else -1.0
        origin, look_at = (-sgn * D, cy, side), (sgn * 10.0, cy, side)
        place = lambda a, b: (sgn * a, b)   # noqa: E731
    else:
        sgn = 1.0 if kind == "+z" else -1.0
        origin, look_at = (side, cy, -sgn * D), (side, cy, sgn * 10.0)
        place = lambda a, b: (b, sgn * a)   # noqa: E731
    items = [_floor(mats[0], y=-1.0)]
    for k, (t, a, b, y, r, h) in enumerate(prims):
        x, z = place(a, b)
        mat = mats[1 + k % 4]
        items.append(make_object(SPHERE, mat, center=(x, y, z), radius=r) if t == "s" else
                     make_object(CYLINDER, mat, center=(x, y, z), radius=r, height=h))
    return _objs(items), camera(W, H, origin, look_at, fov=float(rng.integers(20, 61)), lens_radius=0.0)


def _v(c, name):
    return np.asarray(c[name], dtype=np.float32).reshape(3)


def primary_directions(cam_copy):
    """MotionalCamera::RayGen restated in float32 numpy for a camera (after camera_get_copy) with
    lens_radius == 0, where the direction does not depend on the RNG: [H, W, 3], operation for
    operation (the offset's u * 0 + v * 0 terms included)."""
    c = cam_copy
    assert float(c["lens_radius"]) == 0.0
    W, H = int(c["width"]), int(c["height"])
    rd = F(c["lens_radius"]) * np.ones(3, dtype=np.float32)
    offset = _v(c, "u") * rd[0] + _v(c, "v") * rd[1]
    dx = (np.arange(W, dtype=np.float32) / F(W))[None, :, None]
    dy = (np.arange(H, dtype=np.float32) / F(H))[:, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (((_v(c, "top_left_corner") + dx * _v(c, "horizontal")) + dy * _v(c, "vertical")) - _v(c, "origin")) - offset
        dot = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        inv = F(1.0) / np.sqrt(dot, dtype=np.float32)
        return (v * inv[..., None]).astype(np.float32)


def zero_component_rays(cam_copy):
    """Number of primary rays with at least one direction component that is exactly +-0."""
    return int((primary_directions(cam_copy) == 0.0).any(axis=-1).sum())


# ------------------------------------------------------------------------------ inside
def inside(seed):
    """The camera inside a Glass sphere, inside a Diffuse sphere, inside a cylinder, or below the
    platform looking up."""
    rng = np.random.default_rng([0x696E, seed])
    kind = INSIDE_KINDS[seed % len(INSIDE_KINDS)]
    W, H = int(rng.integers(20, 49)), int(rng.integers(12, 33))
    white = make_material(DIFFUSE, kd=(0.9, 0.9, 0.9))
    lamp = make_material(DIFFUSE, kd=(1.0, 0.9, 0.8), emit_intensity=3.0)
    glass = make_material(GLASS, kd=(1.0, 1.0, 1.0), refractive_index=rng.uniform(1.2, 2.0), smoothness=rng.uniform(2.0, 5.0))
    metal = make_material(METAL, kd=(0.8, 0.6, 0.2), smoothness=rng.uniform(1.0, 4.0))
    c0 = np.array([rng.uniform(-10, 10), rng.uniform(12, 20), rng.uniform(-10, 10)])
    r0 = rng.uniform(8.0, 11.0)
    items = [_floor(white), make_object(SPHERE, lamp, center=c0 + (30.0, 0.0, 5.0), radius=6.0),
             make_object(CYLINDER, metal, center=c0 + (-25.0, -4.0, -8.0), radius=5.0, height=12.0),
             make_object(SPHERE, glass, center=c0 + (4.0, 25.0, 20.0), radius=7.0)]
    origin = c0 + rng.uniform(-0.4, 0.4, 3) * r0
    look_at = c0 + rng.uniform(-1.0, 1.0, 3) * 40.0
    if kind == "glass_sphere":
        items.append(make_object(SPHERE, glass, center=c0, radius=r0))
    elif kind == "diffuse_sphere":
        items.append(make_object(SPHERE, make_material(DIFFUSE, kd=(0.7, 0.8, 0.9), emit_intensity=0.2), center=c0, radius=r0))
        items.append(make_object(SPHERE, lamp, center=c0 + (0.0, 0.6 * r0, 0.0), radius=0.2 * r0))   # a lamp inside
    elif kind == "cylinder":
        items.append(make_object(CYLINDER, make_material(MIRROR, kd=(0.9, 0.9, 0.9), smoothness=3.0, reflectivity=0.5),
                                 center=c0, radius=r0, height=1.6 * r0))
        items.append(make_object(SPHERE, lamp, center=c0 + (0.0, 0.5 * r0, 0.0), radius=0.15 * r0))
    else:
        origin = np.array([rng.uniform(-5, 5), rng.uniform(-30.0, -5.0), rng.uniform(-5, 5)])
        look_at = np.array([rng.uniform(-10, 10), 20.0, rng.uniform(-10, 10)])
        items.append(make_object(SPHERE, lamp, center=(origin[0] + 6.0, origin[1] - 2.0, origin[2]), radius=3.0))
        items.append(make_object(CYLINDER, metal, center=(origin[0] - 8.0, origin[1] + 1.0, origin[2] + 3.0), radius=3.0,
                                 height=5.0))
    return _objs(items), camera(W, H, origin, look_at, fov=rng.uniform(40.0, 90.0), lens_radius=0.0005)


# ---------------------------------------------------------------------- edge_materials
def _s4_like(mat):
    """Floor + three spheres, all of one material under test, plus a Diffuse lamp."""
    white = make_material(DIFFUSE, kd=(0.95, 0.95, 0.95))
    lamp = make_material(DIFFUSE, kd=(1.0, 1.0, 1.0), emit_intensity=2.0)
    items = [_floor(white)]
    for cx in (-35.0, 0.0, 35.0):
        items.append(make_object(SPHERE, mat, center=(cx, 15.0, 0.0), radius=15.0))
    items.append(make_object(SPHERE, lamp, center=(0.0, 45.0, 0.0), radius=8.0))
    return _objs(items)


def edge_materials():
    """{name: (objs, camera)}: one S4-like scene per material edge case, 24 x 12 pixels each."""
    m = make_material
    kd = (0.8, 0.7, 0.6)
    cases = {
        "smooth0_metal": m(METAL, kd=kd, smoothness=0.0),                   # exponent exactly 1.0
        "smooth0_glass": m(GLASS, kd=kd, smoothness=0.0, refractive_index=1.5),
        "smooth_neg1_metal": m(METAL, kd=kd, smoothness=-1.0),              # exponent 1000: always the fallback
        "smooth_neg1_mirror": m(MIRROR, kd=kd, smoothness=-1.0, reflectivity=0.5),
        "smooth_half_metal": m(METAL, kd=kd, smoothness=0.5),
        "smooth_half_glass": m(GLASS, kd=kd, smoothness=0.5, refractive_index=1.3),
        "smooth13_metal": m(METAL, kd=kd, smoothness=13.0),                 # powf overflows: exponent 0, z = 1
        "smooth13_mirror": m(MIRROR, kd=kd, smoothness=13.0, reflectivity=0.5),
        "ior1_glass": m(GLASS, kd=kd, smoothness=3.0, refractive_index=1.0),
        "ior_half_glass": m(GLASS, kd=kd, smoothness=3.0, refractive_index=0.5),
        "ior0_glass": m(GLASS, kd=kd, smoothness=3.0, refractive_index=0.0),
        "refl0_mirror": m(MIRROR, kd=kd, smoothness=2.0, reflectivity=0.0),
        "refl1_mirror": m(MIRROR, kd=kd, smoothness=2.0, reflectivity=1.0),
        "type4_test": m(TEST, kd=kd, smoothness=2.0, refractive_index=1.5, reflectivity=0.5),
        "type7": m(7, kd=kd, smoothness=2.0, refractive_index=1.5, reflectivity=0.5),
    }
    cam = camera(24, 12, (130.0, 103.0, 130.0), (0.0, 10.0, 0.0), fov=35.0)
    return {k: (_s4_like(v), cam.copy()) for k, v in cases.items()}


# ----------------------------------------------------------------------- edge_geometry
def edge_geometry():
    """{name: (objs, camera)}: primitives outside the demo generators' ranges."""
    white = make_material(DIFFUSE, kd=(0.9, 0.9, 0.9))
    red = make_material(DIFFUSE, kd=(0.9, 0.3, 0.3), emit_intensity=0.5)
    glass = make_material(GLASS, kd=(1.0, 1.0, 1.0), refractive_index=1.5, smoothness=4.0)
    metal = make_material(METAL, kd=(0.8, 0.6, 0.2), smoothness=2.5)
    mirror = make_material(MIRROR, kd=(0.9, 0.9, 0.9), smoothness=3.0, reflectivity=0.6)
    s4 = [_floor(white), make_object(SPHERE, glass, center=(-35.0, 15.0, 0.0), radius=15.0),
          make_object(SPHERE, metal, center=(0.0, 15.0, 0.0), radius=15.0),
          make_object(CYLINDER, mirror, center=(35.0, 10.0, 0.0), radius=12.0, height=20.0)]
    cam = camera(32, 20, (130.0, 103.0, 130.0), (0.0, 10.0, 0.0), fov=35.0)
    cases = {}
    cases["unknown_type3"] = (s4 + [make_object(3, red, center=(0.0, 40.0, 30.0), radius=10.0, height=10.0),
                                    make_object(3, red, center=(20.0, 5.0, 40.0), radius=6.0, y_pos=3.0, height=4.0)], cam)
    cases["negative_radius"] = (s4 + [make_object(SPHERE, red, center=(0.0, 20.0, 40.0), radius=-12.0),
                                      make_object(SPHERE, glass, center=(40.0, 12.0, 40.0), radius=-10.0)], cam)
    cases["tiny_and_huge_sphere"] = ([_floor(white), make_object(SPHERE, red, center=(0.0, 10.0, 0.0), radius=2.0 ** -20),
                                      make_object(SPHERE, metal, center=(0.0, 15.0, 0.0), radius=6.0),
                                      make_object(SPHERE, glass, center=(-1.0e6, 2.0e5, -1.0e6), radius=1.0e6)], cam)
    cases["flat_cylinders"] = (s4 + [make_object(CYLINDER, red, center=(0.0, 32.0, 20.0), radius=10.0, height=0.0),
                                     make_object(CYLINDER, metal, center=(10.0, 2.0, 50.0), radius=400.0, height=0.5)], cam)
    far = np.array([1.0e5, 0.0, -1.0e5])
    cases["coords_1e5"] = ([_floor(white)] +
                           [make_object(SPHERE, mt, center=far + c, radius=15.0)
                            for mt, c in ((glass, (-35.0, 15.0, 0.0)), (metal, (0.0, 15.0, 0.0)), (mirror, (35.0, 15.0, 0.0)))] +
                           [make_object(CYLINDER, red, center=far + (0.0, 8.0, 40.0), radius=9.0, height=16.0)],
                           camera(32, 20, far + (130.0, 103.0, 130.0), far + (0.0, 10.0, 0.0), fov=35.0))
    cases["twin_platforms"] = (s4 + [_floor(red), _floor(mirror, y=30.0), _floor(metal, y=30.0)], cam)
    return {k: (_objs(o), c.copy()) for k, (o, c) in cases.items()}


# -------------------------------------------------------------------- degenerate_camera
def degenerate_camera():
    """{name: (objs, camera)}: origin == look_at, and vup parallel to the view direction.  The
    camera basis is NaN, so every primary ray is non-finite (the kernels' reference-order walk
    without the fast quotients), 16 x 8 pixels."""
    objs = edge_geometry()["twin_platforms"][0]
    return {
        "origin_is_look_at": (objs, camera(16, 8, (30.0, 20.0, 30.0), (30.0, 20.0, 30.0))),
        "vup_parallel": (objs, camera(16, 8, (0.0, 120.0, 0.0), (0.0, 0.0, 0.0))),
    }
