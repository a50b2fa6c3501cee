"""What the frame's subsystems hold after the events that touch more than one of them
(cpt_context.hpp: TileSchedule, AdaptiveState, FilterState): a replaced RNG, a new frame, a plain
render after an adaptive one, an adaptive render between CPT_SCHEDULE_PREVIOUS renders.  Written
against the flat Frame before its state was grouped; tests/test_gpu_context_lifecycle.py holds the
buffers of a re-framed context and tests/test_gpu_tile_lists.py the orders themselves (and the
order dropped by cpt_init_rng).  Scene s3, 24 x 16 (six tiles) and 20 x 12 (partial tiles), at most
4 passes of depth 4; every comparison is of bits."""
import math

import adaptive_model as am
import numpy as np
import pytest
from test_gpu_tile_lists import STATE, WEYL, _draw_keys, _stable_descending, _status

from cpppathtracer_amd import CptError, Renderer, camera_get_copy, scenes
from cpppathtracer_amd._lib import CPT_RENDER_AUX
from cpppathtracer_amd.tiling import tile_grid

pytestmark = pytest.mark.gpu

DEPTH = 4
PREV_ORDER_EVERY = 8   # cpt_capi_render.cpp
ADAPT = dict(min_spp=4, max_spp=4, batch=2, rel_error=0.05, max_depth=DEPTH)   # two rounds of two passes


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32).copy()


def _frame(r, sky, W, H, seed=99):
    r.set_scene(scenes.scene_s3())
    r.set_env(sky)
    r.set_frame(W, H)
    r.init_rng(seed)
    return camera_get_copy(scenes.camera_for(W, H))


def _previous(r, cam, spp=1):
    r.render(cam, spp, DEPTH, ordered=True, schedule="previous", sync=True)


def _assert_previous_equals_raster(gpu, other, cam):
    """One CPT_SCHEDULE_PREVIOUS render on `gpu`, and the raster-order render of a second context
    from the same RNG states: the same image and the same states."""
    rng = gpu.read_rng()
    _previous(gpu, cam)
    other.write_rng(rng)
    other.render(cam, 1, DEPTH, ordered=True, sync=True)
    np.testing.assert_array_equal(_bits(gpu.read_accum()), _bits(other.read_accum()))
    np.testing.assert_array_equal(gpu.read_rng(), other.read_rng())


def _refreshed_order_counts_from(gpu, cam, W, H, renders, d_stale=None):
    """`renders` more CPT_SCHEDULE_PREVIOUS renders, the last of which rebuilds the order: it must
    be the sort of the draws since the first of them (not since the plane `d_stale` read earlier,
    where the caller has made sure that the two differ)."""
    d0 = gpu.read_rng()[5]
    for i in range(renders):
        before = gpu.debug_tile_order(1)
        _previous(gpu, cam)
        if i < renders - 1:
            np.testing.assert_array_equal(gpu.debug_tile_order(1), before, err_msg=f"render {i}: rebuilt early")
    d1 = gpu.read_rng()[5]
    want = _stable_descending(_draw_keys(d0, d1, W, H)[0])
    if d_stale is not None:
        stale = _stable_descending(_draw_keys(d_stale, d1, W, H)[0])
        assert (want != stale).any()   # the two counts tell the orders apart
    np.testing.assert_array_equal(gpu.debug_tile_order(1), want)


@pytest.mark.parametrize("W,H", [(24, 16), (20, 12)])
def test_write_rng_keeps_the_order_and_recounts_the_draws(gpu, sky, W, H):
    cam = _frame(gpu, sky, W, H)
    _previous(gpu, cam)
    d_stale = gpu.read_rng()[5]   # the plane the order's draws are counted from
    _previous(gpu, cam)
    order = gpu.debug_tile_order(1)
    assert sorted(order.tolist()) == list(range(math.prod(tile_grid(W, H))))
    # other states than the ones read: counted from d_stale, the lightest tile would have made
    # 4000 draws per pixel and come first
    rng = gpu.read_rng()
    rng[5][am.tile_of_pixel(W, H) == order[-1]] += np.uint32(WEYL * 4000)
    gpu.write_rng(rng)
    np.testing.assert_array_equal(gpu.debug_tile_order(1), order)
    with Renderer(0) as other:
        _frame(other, sky, W, H)
        _assert_previous_equals_raster(gpu, other, cam)
    np.testing.assert_array_equal(gpu.debug_tile_order(1), order)   # the third render since the order was built
    # renders 4 .. 9 keep it, render 9 rebuilds it from the draws since the write
    gpu.write_rng(rng)
    _refreshed_order_counts_from(gpu, cam, W, H, PREV_ORDER_EVERY - 2, d_stale)


def test_set_frame_drops_every_subsystems_result(gpu, sky):
    W, H = 24, 16
    cam = _frame(gpu, sky, W, H)
    gpu.render(cam, 2, DEPTH, ordered=True, schedule="cost", sync=True)
    _previous(gpu, cam)
    gpu.render_adaptive(cam, flags=CPT_RENDER_AUX, **ADAPT)
    gpu.filter_frame(levels=1)
    # all of it is there
    assert gpu.debug_tile_order(0).size == 6 and gpu.debug_tile_order(1).size == 6
    assert gpu.read_noise().size == W * H and gpu.adaptive_info()["rounds"] == 2
    assert gpu.read_moments().shape == (4, W * H) and gpu.read_filtered()[0].shape == (W * H, 3)
    gpu.set_frame(W, H)
    assert _status(gpu, 0) == STATE and _status(gpu, 1) == STATE
    for read in (gpu.read_noise, gpu.adaptive_info, gpu.read_moments, gpu.read_filtered):
        with pytest.raises(CptError) as e:
            read()
        assert e.value.status == STATE, read.__name__
    # and an RNG alone brings none of it back
    gpu.init_rng(3)
    assert _status(gpu, 0) == STATE and _status(gpu, 1) == STATE
    with pytest.raises(CptError) as e:
        gpu.read_noise()
    assert e.value.status == STATE


def test_plain_render_keeps_the_adaptive_result(gpu, sky):
    W, H = 20, 12
    cam = _frame(gpu, sky, W, H)
    info = gpu.render_adaptive(cam, **ADAPT)
    noise, moments = _bits(gpu.read_noise()), _bits(gpu.read_moments())
    assert info["rounds"] == 2 and info["active_tiles"][0] == 6 and info["passes_done"] >= 2 * W * H
    gpu.render(cam, 1, DEPTH, sync=True)
    _previous(gpu, cam)
    after = gpu.adaptive_info()
    assert after["rounds"] == info["rounds"] and after["passes_done"] == info["passes_done"]
    np.testing.assert_array_equal(after["active_tiles"], info["active_tiles"])
    np.testing.assert_array_equal(_bits(gpu.read_noise()), noise)
    np.testing.assert_array_equal(_bits(gpu.read_moments()), moments)


@pytest.mark.parametrize("W,H", [(24, 16), (20, 12)])
def test_previous_render_after_an_adaptive_one(gpu, sky, W, H):
    cam = _frame(gpu, sky, W, H)
    with Renderer(0) as other:
        _frame(other, sky, W, H)
        # no order valid: none after the adaptive render either, and the next such render builds
        # it from its own draws alone
        gpu.render_adaptive(cam, **ADAPT)
        assert _status(gpu, 1) == STATE
        d0 = gpu.read_rng()[5]
        _assert_previous_equals_raster(gpu, other, cam)
        keys, _ = _draw_keys(d0, gpu.read_rng()[5], W, H)
        order = gpu.debug_tile_order(1)
        np.testing.assert_array_equal(order, _stable_descending(keys))
        # an order valid: the adaptive render keeps it, the next such render uses and keeps it
        gpu.render_adaptive(cam, **ADAPT)
        np.testing.assert_array_equal(gpu.debug_tile_order(1), order)
        _assert_previous_equals_raster(gpu, other, cam)
        np.testing.assert_array_equal(gpu.debug_tile_order(1), order)
    # the render above was the second since the order was built; the ninth rebuilds it, from the
    # draws since the adaptive render (which six tiles' natural draws need not tell from a count
    # that includes it: test_write_rng_keeps_the_order_and_recounts_the_draws forces the difference)
    gpu.render_adaptive(cam, **ADAPT)
    _refreshed_order_counts_from(gpu, cam, W, H, PREV_ORDER_EVERY - 1)
