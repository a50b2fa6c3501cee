"""The 4-wide walk's node visit (cpt_path.hpp trace_wide), held to the oracle and to recorded
counters on scenes chosen for what a change to the visit's bookkeeping can break: the four child
refs (leaf, empty, node; low and high halves of the stored words; beyond the byte range), the sort
keys (all four children hit, exact ties, negative entry distances), the pushes (deep stacks), the
HYB node fetch, and suspension with refill.  The floor alone and the floor with one primitive have
no 4-wide tree (n_wide == 0: the binary walk runs), so they guard that boundary and do not count
as coverage of the ref slots; those start at two primitives (root2 .. root5).

Frames are 32 x 32 at 4 spp, depth 8: at most 1024 pixels, so with the whole grid no lane takes a
second pixel and the lane-to-pixel mapping is static.  On such frames the wide walk's node,
primitive, fallback and global-node counts are reproducible run to run (each depends on the pixel's
wave-mates, which are fixed), so tests/golden/wide_visit_counters.json -- recorded from the walk as
it was before the visit's bookkeeping was rewritten -- pins the walk's decisions exactly: the same
hit masks, nearest children and pushes give the same visits and leaf tests.  The refill runs
(set_debug_grid) compare against the oracle only: there a lane's second pixel depends on timing.
"""
import json
import os

import numpy as np
import pytest
from test_gpu_parity import _check_stats, _run_both

from cpppathtracer_amd import scenes, types

pytestmark = pytest.mark.gpu

W = H = 32
SPP, DEPTH = 4, 8
LDS_TREE_NODES = 512   # cpt_internal.hpp: wide nodes staged in LDS
# S1000's generator at the smallest object count whose 4-wide tree outgrows the LDS image
# (walk_info()["n_wide"] > 512; test_hyb_scene_is_the_smallest checks both sides)
HYB_N = 1104
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_visit_counters.json")
COUNTERS = ("segments", "nodes", "prims", "hits", "misses", "fallbacks", "gnodes")

_S4 = scenes.scene_s4()
FLOOR = _S4[0]
MATS = [_S4[1]["material"], _S4[2]["material"], _S4[3]["material"],
        types.make_material(types.DIFFUSE, kd=(0.7, 0.4, 0.2))]


def _objs(items):
    out = np.zeros(len(items), dtype=types.OBJECT_DTYPE)
    for i, o in enumerate(items):
        out[i] = o
    return out


def _sphere(c, r, k):
    return types.make_object(types.SPHERE, MATS[k % len(MATS)], center=c, radius=r)


def _root_only(k):
    """The floor and k spheres in a row: k <= 4 is one wide node whose slots hold k leaf refs and
    4 - k empty ones; k = 5 adds the first node ref."""
    return _objs([FLOOR] + [_sphere((-44.0 + 22.0 * i, 10.0, 0.0), 10.0, i) for i in range(k)]), None


def _sheet():
    """320 small spheres in a sheet at eye height seen edge-on: leaf refs below -256 and node refs
    above 255 go through the 16-bit stack, from both halves of the stored words."""
    s = [_sphere((-60.0 + 6.0 * (i % 20), 10.0, -48.0 + 6.0 * (i // 20)), 2.0, i) for i in range(320)]
    return _objs([FLOOR] + s), types.make_camera(W, H, origin=(-200.0, 10.0, 3.0), look_at=(0.0, 10.0, 0.0))


def _line():
    """64 equal spheres on a line, the camera looking along it: every child of a node is hit and
    the stacks run deep."""
    s = [_sphere((9.0 * i, 10.0, 0.0), 4.0, 0 if i % 3 else 2) for i in range(64)]
    return _objs([FLOOR] + s), types.make_camera(W, H, origin=(-15.0, 11.0, 1.0), look_at=(300.0, 10.0, 0.0))


def _grid_objs():
    return _objs([FLOOR] + [_sphere((-15.0 + 10.0 * x, 5.0 + 10.0 * y, 10.0 * z), 3.0, x + y + z)
                            for x in range(4) for y in range(4) for z in range(4)])


def _grid_axis():
    """A 4 x 4 x 4 grid of equal spheres seen along z from its axis of symmetry: sibling boxes at
    equal entry distances in several slots."""
    return _grid_objs(), types.make_camera(W, H, origin=(0.0, 20.0, -110.0), look_at=(0.0, 20.0, 0.0))


def _grid_inside():
    """The camera in the middle of the grid: nested boxes around the origin, negative entry
    distances."""
    return _grid_objs(), types.make_camera(W, H, origin=(0.0, 20.0, 15.0), look_at=(40.0, 24.0, 100.0))


def _twins():
    """Every primitive of the grid twice, with another material, shuffled (as in
    test_gpu_parity.py::test_exact_ties_between_primitives): exact-twin boxes in sibling slots."""
    objs, cam = _grid_axis()
    twins = objs.copy()
    twins["material"] = np.roll(twins["material"].copy(), 7)
    both = np.concatenate([objs, twins]).astype(types.OBJECT_DTYPE)
    return np.ascontiguousarray(both[np.random.default_rng(5).permutation(both.size)]), cam


def _hyb():
    return scenes.scene_s1000(n=HYB_N), None


def _hyb3000():
    """A tree far past the LDS image, so that walks do read nodes from global memory (at HYB_N
    only the three smallest nodes lie there, and this frame's rays do not reach them)."""
    return scenes.scene_s1000(n=3000), None


SCENES = {"floor": lambda: (_objs([FLOOR]), None)}
SCENES.update({f"root{k}": (lambda k=k: _root_only(k)) for k in range(1, 6)})
SCENES.update(sheet=_sheet, line=_line, twins=_twins, grid_axis=_grid_axis, grid_inside=_grid_inside, hyb=_hyb,
              hyb3000=_hyb3000)

# the counting kernels, the kernel the bench times, its consolidating form, and k_wf_extend
PATHS = ["megakernel:ordered", "megakernel:ordered+timed", "megakernel:ordered+timed+cons", "wavefront:ordered"]
# the megakernel's counts are reproducible on these frames; k_wf_extend's are not (its waves are
# packed from a compacted ray list whose order depends on timing), so it is held to the oracle only
PINNED = "megakernel:ordered"


def render_and_check(gpu, oracle_mod, sky, name, path):
    """Image bits, RNG end states and hit / miss / segment counts against the oracle; returns the
    render's counters (None for a path without them)."""
    objs, cam = SCENES[name]()
    (ga, gr, gs, _), (oa, orng, os_, _) = _run_both(gpu, oracle_mod, sky, objs, W, H, SPP, DEPTH, path=path,
                                                    cam=cam if cam is not None else scenes.camera_for(W, H))
    np.testing.assert_array_equal(gr, orng)
    _check_stats(gs, os_, path)
    np.testing.assert_array_equal(ga.view(np.uint32), oa.view(np.uint32))
    if gs is None:
        return None
    return dict(gs, gnodes=int(gpu.raw_counters()[6]))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(SCENES))
def test_visit_scene(gpu, oracle_mod, sky, golden, name, path):
    got = render_and_check(gpu, oracle_mod, sky, name, path)
    if path == PINNED:
        assert [got[k] for k in COUNTERS] == golden[name]


def test_scenes_are_what_they_claim(gpu):
    """The trees behind the scene names: root-only up to four primitives, refs beyond the byte
    range, a tree past the LDS image."""
    for k, n_wide in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 2)):   # one primitive: no tree
        gpu.set_scene(_root_only(k)[0])
        assert gpu.walk_info()["n_wide"] == n_wide, k
    gpu.set_scene(_sheet()[0])
    info = gpu.walk_info()
    assert info["n_unb"] == 1 and info["n_walk"] == 2 * 320   # 320 leaves: refs down to -321
    assert 0 < info["n_wide"] <= LDS_TREE_NODES


def test_hyb_scene_is_the_smallest(gpu):
    gpu.set_scene(scenes.scene_s1000(n=HYB_N))
    assert gpu.walk_info()["n_wide"] > LDS_TREE_NODES
    gpu.set_scene(scenes.scene_s1000(n=HYB_N - 1))
    assert 0 < gpu.walk_info()["n_wide"] <= LDS_TREE_NODES


def test_hyb_reads_global_nodes(golden):
    g = COUNTERS.index("gnodes")
    assert golden["hyb3000"][g] > 0
    assert all(v[g] == 0 for k, v in golden.items() if k != "hyb3000")


# one workgroup of full waves (1024 lanes for 1024 pixels: suspension, no second pixel), and four
# lanes per wave (64 pixel slots: every lane refills, beside suspended walks)
@pytest.mark.parametrize("grid", [(1, 64), (1, 4)])
@pytest.mark.parametrize("path", ["megakernel:ordered", "megakernel:ordered+timed", "megakernel:ordered+timed+cons"])
@pytest.mark.parametrize("name", ["line", "hyb", "hyb3000"])
def test_visit_scene_capped_grid(gpu, oracle_mod, sky, name, path, grid):
    gpu.set_debug_grid(*grid)
    try:
        render_and_check(gpu, oracle_mod, sky, name, path)
    finally:
        gpu.set_debug_grid(0, 0)
