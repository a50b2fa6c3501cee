"""Sky and material-texture geometries beyond the one sky fixture (1280 x 1280 logical, 320 valid
columns), zero-lens views that sweep the whole sky, and a host restatement of the miss shader
plus the bilinear fetch that neither the kernels nor the oracle had a hand in
(test_sky_fuzz.py checks both against the oracle on the CPU; test_gpu_sky_parity.py renders them
on the GPU).

Everything is pure numpy on np.random.default_rng(fixed seed); no expectation is stored.
"""
import numpy as np
import scene_fuzz as sf

from cpppathtracer_amd.texture_io import EnvTexture

F = np.float32

# (logical_width, height, valid_cols)
GEOMETRIES = [
    (1, 1, 1),          # n == 1
    (1, 1, 0),          # cols == 0 with a non-null pointer
    (2, 2, 2),          # smallest texture with two distinct taps per axis
    (3, 5, 3),          # small, non-square, full
    (4, 4, 1),          # width/4 upload quirk, small
    (7, 3, 1),          # width/4 upload quirk, non-square
    (8, 8, 2),          # width/4 upload quirk
    (64, 32, 16),       # width/4 upload quirk, mid-size
    (37, 91, 37),       # odd sizes, full
    (37, 91, 9),        # odd sizes, cols below width/4 + 1
    (1280, 2, 320),     # very wide, two rows
    (5, 640, 5),        # very tall, full
    (16, 16, 16),       # square, full
    (12, 9, 5),         # cols between width/4 and width
]

# the lit-scene subset of test_gpu_sky_parity.py
LIT_GEOMETRIES = [(1, 1, 1), (1, 1, 0), (4, 4, 1), (37, 91, 9), (1280, 2, 320), (5, 640, 5), (12, 9, 5)]

# material textures: (logical_width, height, valid_cols)
TEXTURE_GEOMETRIES = [
    (1, 1, 1),          # n == 1
    (2, 2, 0),          # cols == 0
    (3, 1, 3),          # one row
    (1, 7, 1),          # one column
    (5, 4, 1),          # cols below the width
    (64, 2, 16),        # wide, width/4 upload quirk
]

W, H = 32, 24


def geometry_id(g):
    return "%dx%dc%d" % g


def texture(geometry, *seed):
    """Random RGBA8 texels (alpha too: the fetch must ignore it) for a (w, h, cols) geometry."""
    w, h, cols = geometry
    rng = np.random.default_rng([w, h, cols, *seed])
    return EnvTexture(rng.integers(0, 256, size=(h, cols, 4), dtype=np.uint8), w, h)


def sky(geometry):
    return texture(geometry)


def _view(look_at, vup=(0.0, 1.0, 0.0)):
    return sf.camera(W, H, (0.0, 0.0, 0.0), look_at, fov=100.0, lens_radius=0.0, vup=vup)


# The +-z views put d.x == d.y == 0 on the centre pixel (u = atan(0/0) is NaN: the fetch's guard
# returns black); the +-x and +-y views reach d.y / d.x = +-inf and +-0.
VIEWS = {
    "+x": _view((1.0, 0.0, 0.0)),
    "-x": _view((-1.0, 0.0, 0.0)),
    "+z": _view((0.0, 0.0, 1.0)),
    "-z": _view((0.0, 0.0, -1.0)),
    "diag": _view((1.0, 0.7, 0.4)),
    "+y": _view((0.0, 1.0, 0.001), vup=(0.0, 0.0, 1.0)),
    "-y": _view((0.0, -1.0, 0.001), vup=(0.0, 0.0, 1.0)),
}


def _reflect(i, n):
    """Mirror addressing in its general form: the index modulo 2n, the upper half reflected."""
    m = np.mod(i, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def sky_reference(dirs, tex):
    """Miss (path_tracer.cu:117-122) + tex2D on a uchar4 array with normalized coordinates, mirror
    addressing, linear filtering and a normalized-float read (textures.cu:14-71), restated in
    float32 numpy: dirs [..., 3] float32 -> (rgb [..., 3] float32, taps, finite).

    `taps` holds the unfolded tap indices i0, j0 (the second taps are i0 + 1, j0 + 1) and the
    folded ones x0, x1, y0, y1; `finite` is False where (u, v) is NaN or out of range and the
    fetch gives 0.  asinf / atanf are the oracle's sequences, pinned by test_oracle_math.py."""
    import oracle
    d = np.asarray(dirs, dtype=np.float32)
    w, h, cols = int(tex.width), int(tex.height), int(tex.valid_cols)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # normalize: the squared length summed left to right, one reciprocal, three products
        dot = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        inv = F(1.0) / np.sqrt(dot, dtype=np.float32)
        n = (d * inv[..., None]).astype(np.float32)
        asin = oracle.math_batch(3, n[..., 2]).reshape(dot.shape)
        atan = oracle.math_batch(4, (n[..., 1] / n[..., 0]).astype(np.float32)).reshape(dot.shape)
        v = (asin.astype(np.float64) / np.pi + 0.5).astype(np.float32)
        u = ((atan / F(2.0)).astype(np.float32).astype(np.float64) / np.pi).astype(np.float32)
        # unnormalised texel coordinates of the linear filter
        x = (u * F(w)).astype(np.float32) - F(0.5)
        y = (v * F(h)).astype(np.float32) - F(0.5)
        lim = F(1e7)
        finite = (x > -lim) & (x < lim) & (y > -lim) & (y < lim)
        x = np.where(finite, x, F(0.0))
        y = np.where(finite, y, F(0.0))
        fx, fy = np.floor(x), np.floor(y)
        # 9-bit fixed-point weights: 8 fractional bits, rounded to nearest
        a = np.floor((x - fx) * F(256.0) + F(0.5)) / F(256.0)
        b = np.floor((y - fy) * F(256.0) + F(0.5)) / F(256.0)
    i0, j0 = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, y0, y1 = _reflect(i0, w), _reflect(i0 + 1, w), _reflect(j0, h), _reflect(j0 + 1, h)
    # the whole logical texture as floats; columns the upload never wrote read as 0
    full = np.zeros((h, w, 3), dtype=np.float32)
    full[:, :cols] = tex.rgba[:, :, :3].astype(np.float32) / F(255.0)
    t00, t10, t01, t11 = full[y0, x0], full[y0, x1], full[y1, x0], full[y1, x1]
    one = F(1.0)
    w00, w10, w01, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    rgb = ((w00[..., None] * t00 + w10[..., None] * t10) + w01[..., None] * t01) + w11[..., None] * t11
    rgb = np.where(finite[..., None], rgb, F(0.0)).astype(np.float32)
    taps = dict(i0=i0, j0=j0, x0=x0, x1=x1, y0=y0, y1=y1, a=a, b=b)
    return rgb, taps, finite


_CACHE = {}


def reference(geometry, view, camera_get_copy):
    """sky_reference for one geometry and view at W x H, computed once and read-only:
    (rgb [H*W, 3], taps, finite)."""
    key = (geometry, view)
    if key not in _CACHE:
        dirs = sf.primary_directions(camera_get_copy(VIEWS[view]))
        rgb, taps, finite = sky_reference(dirs, sky(geometry))
        rgb = np.ascontiguousarray(rgb.reshape(-1, 3))
        for arr in (rgb, finite, *taps.values()):
            arr.setflags(write=False)
        _CACHE[key] = (rgb, taps, finite)
    return _CACHE[key]
