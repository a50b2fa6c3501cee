"""GPU parity of the environment fetch and the material textures at the geometries of
sky_fuzz.py, beyond the one 1280 x 1280 x 320 sky fixture and the 16 x 8 synthetic textures.

Sky-only renders are compared, as bits, both with the oracle and with sky_fuzz.sky_reference, the
host restatement of Miss + tex2D that shares no code with either (a mistake the kernels and the
oracle had in common would pass GPU == oracle).  Lit scenes send bounce directions over the whole
sphere into the small skies; on the megakernel those fetches go through the deferred PendingSky
rounds.  test_sky_fuzz.py checks on the CPU that the views reach what they are meant to."""
import numpy as np
import pytest
import sky_fuzz as kf
from test_gpu_parity import PATHS, _check_stats, _run_both
from test_gpu_textures import MODES, _both

from cpppathtracer_amd import camera_get_copy, scenes, types

pytestmark = pytest.mark.gpu

SKY_PATHS = ["megakernel", "megakernel:ordered", "wavefront", "megakernel:ordered+timed", "megakernel:ordered+timed+cons"]
EMPTY = np.zeros(0, dtype=types.OBJECT_DTYPE)


@pytest.mark.parametrize("path", SKY_PATHS)
@pytest.mark.parametrize("g", kf.GEOMETRIES, ids=kf.geometry_id)
def test_sky_only(gpu, oracle_mod, g, path):
    """The empty scene under each sky, seven views: every pixel is one sky fetch."""
    tex = kf.sky(g)
    for view, cam in kf.VIEWS.items():
        (ga, gr, gs, _), (oa, orng, os_, _) = _run_both(gpu, oracle_mod, tex, EMPTY, kf.W, kf.H, 1, 4, path=path, cam=cam)
        np.testing.assert_array_equal(ga.view(np.uint32), oa.view(np.uint32), err_msg=view)
        rgb, _, _ = kf.reference(g, view, camera_get_copy)
        np.testing.assert_array_equal(np.ascontiguousarray(ga[:, :3]).view(np.uint32), rgb.view(np.uint32), err_msg=view)
        assert (ga[:, 3] == 1).all()
        np.testing.assert_array_equal(gr, orng, err_msg=view)
        if gs is not None:
            assert gs["hits"] == 0 and gs["misses"] == os_["misses"] == kf.W * kf.H, view
        _check_stats(gs, os_, path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("g", kf.LIT_GEOMETRIES, ids=kf.geometry_id)
def test_lit_scene_small_sky(gpu, oracle_mod, g, path):
    objs = scenes.scene_s1000(n=120)
    (ga, gr, gs, _), (oa, orng, os_, _) = _run_both(gpu, oracle_mod, kf.sky(g), objs, 48, 32, 2, 8, path=path)
    np.testing.assert_array_equal(gr, orng)
    _check_stats(gs, os_, path)
    assert os_["hits"] > 0 and os_["misses"] > 0
    np.testing.assert_array_equal(ga.view(np.uint32), oa.view(np.uint32))


@pytest.mark.parametrize("ordered", [False, True])
def test_sky_replaced_in_context(gpu, oracle_mod, sky, ordered):
    """One scene and one frame; the sky replaced by a smaller one, by none, by a larger one and by
    the first again: the device buffer shrinks and regrows, and no render may see the previous
    sky's width, height or column count."""
    W, H, spp, depth = 48, 32, 2, 8
    objs = scenes.scene_s1000(n=120)
    cam = camera_get_copy(scenes.camera_for(W, H))
    rows = np.arange(H, dtype=np.int32)
    gpu.set_scene(objs)
    gpu.set_frame(W, H)
    images = []
    for env in (sky, kf.sky((4, 4, 1)), None, kf.sky((37, 91, 37)), sky):
        gpu.set_env(env)
        gpu.init_rng(77)
        gpu.render(cam, spp, depth, sync=True, ordered=ordered)
        ga, gr = gpu.read_accum(), gpu.read_rng()
        rng = oracle_mod.init_rng(77, W, rows, threads=8)
        oa, _, _, _ = oracle_mod.render(objs, cam, env, rows, spp, depth, rng, threads=8)
        np.testing.assert_array_equal(gr, rng)
        np.testing.assert_array_equal(ga.view(np.uint32), oa.view(np.uint32))
        images.append(ga)
    np.testing.assert_array_equal(images[0], images[4])
    for k in (1, 2, 3):
        assert not np.array_equal(images[k], images[k - 1])


@pytest.mark.parametrize("addr,filt", MODES)
@pytest.mark.parametrize("g", kf.TEXTURE_GEOMETRIES, ids=kf.geometry_id)
def test_material_texture_geometries(gpu, oracle_mod, sky, g, addr, filt):
    """Material::GetKd samples at (0, 0): under linear filtering the taps sit at index -1 and 0, so
    every address mode's handling of -1 is reached at n == 1 and n == 2 (wrap's -1 % 1 included)."""
    objs = scenes.scene_s4_textured()
    texs = [kf.texture(g, k) for k in range(3)]
    img = _both(gpu, oracle_mod, sky, objs, [(h, t, addr, filt) for h, t in zip((1, 2, 3), texs)])
    if g == (1, 1, 1) and (addr, filt) == (types.ADDRESS_BORDER, types.FILTER_LINEAR):
        # not one constant colour under every mode: border blends three zero taps in (_both has
        # just shown both images to be the oracle's)
        clamp = _both(gpu, oracle_mod, sky, objs, [(h, t, types.ADDRESS_CLAMP, filt) for h, t in zip((1, 2, 3), texs)])
        assert not np.array_equal(img, clamp)
