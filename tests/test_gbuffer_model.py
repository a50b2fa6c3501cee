"""Pins tests/gbuffer_model.py (the yardstick of test_gpu_gbuffer.py) to the oracle, on the CPU.

For every G-buffer fixture the oracle renders 1 spp at max_depth 1 with lens_radius 0 and an
environment that reads 0 everywhere: its first-hit normals must be the model's bit for bit (which
also pins t, the normal being formed from origin + t * dir), and on a copy of the scene whose
materials encode the object index its radiance must decode to the model's ids.  No pixel is left
out: a scene or camera where the brute-force model and the reference's BVH walk disagree (a
primitive's t outside its own box by rounding) does not belong in the fixtures.
"""
import numpy as np
import pytest

import gbuffer_model as gm
from cpppathtracer_amd import scenes

FIXTURES = gm.fixtures()


def _oracle_first_hit(oracle_mod, objs, cam, rows):
    W = int(cam["width"])
    rows = np.arange(int(cam["height"]), dtype=np.int32) if rows is None else np.asarray(rows, dtype=np.int32)
    rng = oracle_mod.init_rng(scenes.DEFAULT_SEED, W, rows)
    accum, _, normal, _ = oracle_mod.render(objs, cam, None, rows, 1, 1, rng, want_aux=True)   # env None: reads 0
    return accum, normal


@pytest.fixture(scope="module", params=sorted(FIXTURES))
def case(request, oracle_mod):
    objs, cam0, rows = FIXTURES[request.param]
    cam = oracle_mod.camera_get_copy(cam0)
    return objs, cam, rows, gm.gbuffer(oracle_mod, objs, cam, rows)


def test_normals_equal_the_oracles(case, oracle_mod):
    objs, cam, rows, (_, _, normal, _) = case
    _, onormal = _oracle_first_hit(oracle_mod, objs, cam, rows)
    want = (np.float32(0.0) + normal).astype(np.float32)   # the oracle accumulates 0.f + n
    np.testing.assert_array_equal(want.view(np.uint32), onormal.view(np.uint32))


def test_ids_equal_the_oracles(case, oracle_mod):
    objs, cam, rows, (ids, t, _, _) = case
    accum, _ = _oracle_first_hit(oracle_mod, gm.id_scene(objs), cam, rows)
    hit = accum[:, 2] == 1.0
    decoded = np.where(hit, accum[:, 0].astype(np.int32) + 256 * accum[:, 1].astype(np.int32), -1)
    assert set(np.unique(accum[:, 2])) <= {0.0, 1.0}
    np.testing.assert_array_equal(ids, decoded)
    np.testing.assert_array_equal(t[~hit], np.full(int((~hit).sum()), gm.TMAX))
    assert (t[hit] > 0).all() and (t[hit] < gm.TMAX).all()


def test_fixtures_see_several_objects(oracle_mod):
    """The full frames are not trivially one object or all sky."""
    for name in ("s4_64x48", "s4_67x9", "s1000_96x64", "fuzz_hyb_48x32"):
        objs, cam0, rows = FIXTURES[name]
        ids = gm.gbuffer(oracle_mod, objs, oracle_mod.camera_get_copy(cam0), rows)[0]
        assert len(np.unique(ids[ids >= 0])) >= 3, name
