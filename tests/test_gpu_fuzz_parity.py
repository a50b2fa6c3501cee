"""GPU parity on the fuzzed scenes, cameras and materials of scene_fuzz.py: what
test_gpu_parity.py::test_render_bitexact asserts (RNG end states, traversal counters and the
accumulators' bits against the oracle), on cameras with exactly-zero direction components, inside
objects and under the floor, on overlapping and nested primitives, and on material and primitive
parameters outside the demo scenes' ranges.  Some edge cases legitimately give NaN radiance, so
the accumulators are compared as bits (NaN payloads included) and not required to be finite.
test_scene_fuzz.py checks on the CPU that the cases hit what they are meant to."""
import numpy as np
import pytest
import scene_fuzz as sf
from test_gpu_parity import PATHS, _check_stats, _run_both

pytestmark = pytest.mark.gpu

SHORT_PATHS = ["megakernel", "megakernel:ordered", "megakernel:plain", "wavefront:ordered", "megakernel:ordered+timed",
               "megakernel:ordered+timed+cons"]
EDGE_MATERIALS = sf.edge_materials()
EDGE_GEOMETRY = sf.edge_geometry()
DEGENERATE = sf.degenerate_camera()


def _parity(gpu, oracle_mod, sky, objs, cam, family, path):
    spp, depth = sf.PARAMS[family]
    W, H = int(cam["width"]), int(cam["height"])
    assert W <= 64 and H <= 40
    (ga, gr, gs, _), (oa, orng, os_, _) = _run_both(gpu, oracle_mod, sky, objs, W, H, spp, depth, path=path, cam=cam)
    np.testing.assert_array_equal(gr, orng)
    _check_stats(gs, os_, path)
    np.testing.assert_array_equal(ga.view(np.uint32), oa.view(np.uint32))
    return os_


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("seed", sf.MIXED_SEEDS)
def test_mixed(gpu, oracle_mod, sky, seed, path):
    objs, cam = sf.mixed(seed)
    _parity(gpu, oracle_mod, sky, objs, cam, "mixed", path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("seed", sf.AXIS_SEEDS)
def test_axis_aligned(gpu, oracle_mod, sky, seed, path):
    objs, cam = sf.axis_aligned(seed)
    _parity(gpu, oracle_mod, sky, objs, cam, "axis_aligned", path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("seed", sf.MIXED_LARGE_SEEDS)
def test_mixed_large_wide_walk_axis_aligned(gpu, oracle_mod, sky, seed, path):
    """More than 200 primitives under an axis-aligned, zero-lens camera: the 4-wide LDS walk is
    the code that meets the exactly-zero direction components."""
    objs, cam = sf.mixed_large(seed)
    gpu.set_scene(objs)
    assert gpu.walk_info()["n_wide"] > 0
    _parity(gpu, oracle_mod, sky, objs, cam, "mixed_large", path)


@pytest.mark.parametrize("path", SHORT_PATHS)
@pytest.mark.parametrize("seed", sf.INSIDE_SEEDS)
def test_inside(gpu, oracle_mod, sky, seed, path):
    objs, cam = sf.inside(seed)
    _parity(gpu, oracle_mod, sky, objs, cam, "inside", path)


@pytest.mark.parametrize("path", SHORT_PATHS)
@pytest.mark.parametrize("name", list(EDGE_MATERIALS))
def test_edge_materials(gpu, oracle_mod, sky, name, path):
    objs, cam = EDGE_MATERIALS[name]
    _parity(gpu, oracle_mod, sky, objs, cam, "edge_materials", path)


@pytest.mark.parametrize("path", SHORT_PATHS)
@pytest.mark.parametrize("name", list(EDGE_GEOMETRY))
def test_edge_geometry(gpu, oracle_mod, sky, name, path):
    objs, cam = EDGE_GEOMETRY[name]
    _parity(gpu, oracle_mod, sky, objs, cam, "edge_geometry", path)


# Kept last in the file: every primary ray is non-finite and takes the kernels' reference-order
# walk without the fast quotients (trace<.., FAST = false>).  That walk advances an integer node
# index (ni + 1 or the node's forward miss link) until it passes the node count, and the path loop
# counts segments up to the depth, so neither is bounded by a float comparison a NaN could defeat.
@pytest.mark.parametrize("path", ["megakernel", "megakernel:ordered", "wavefront"])
@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_camera(gpu, oracle_mod, sky, name, path):
    objs, cam = DEGENERATE[name]
    os_ = _parity(gpu, oracle_mod, sky, objs, cam, "degenerate_camera", path)
    assert os_["segments"] == 16 * 8 * sf.PARAMS["degenerate_camera"][0]
