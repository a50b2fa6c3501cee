"""What a context owns across its lifecycle (cpt_context.hpp: DevBuf, Frame): re-framing one
context must leave nothing of the previous frame behind, gather maps must follow their source
context, contexts must come and go cleanly, and a refused display band must leave the good one
whole.  Every comparison is of bits.  Each test makes its own Renderers (the `gpu` fixture is
taken only so that torch's HIP runtime is loaded first); scene s3 at 2 spp and depth 4."""
import numpy as np
import pytest

from cpppathtracer_amd import CptError, Renderer, camera_get_copy, scenes

pytestmark = pytest.mark.gpu

SPP, DEPTH = 2, 4
# (W, H, rows): the last one a non-contiguous ascending subset of its frame's rows
FRAMES = [(40, 24, None), (72, 40, None), (24, 16, [1, 2, 5, 6, 7, 11, 12, 15])]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32).copy()


def _renderer(sky):
    r = Renderer(0)
    r.set_scene(scenes.scene_s3())
    r.set_env(sky)
    return r


def _walk_frame(r, W, H, rows, seed):
    """Frames the context and touches every lazily allocated buffer of the frame; returns the
    state after each step: [(step, {name: bits})]."""
    r.set_frame(W, H, None if rows is None else np.asarray(rows, dtype=np.int32))
    r.init_rng(seed)
    cam = camera_get_copy(scenes.camera_for(W, H))
    band = rows is None   # the display path needs one ascending run of rows
    seen = []

    def snap(step, aux=True, **extra):
        s = {"accum": _bits(r.read_accum()), "rng": r.read_rng().copy()}
        if aux:
            n, d = r.read_aux()
            s.update(normal=_bits(n), depth=_bits(d))
        s.update(extra)
        seen.append((step, s))

    r.render(cam, SPP, DEPTH, sync=True)
    snap("plain", aux=False)
    r.render(cam, SPP, DEPTH, aux=True, sync=True)
    snap("aux")
    r.render(cam, SPP, DEPTH, aux=True, path="wavefront", sync=True)
    snap("wavefront")
    r.render(cam, SPP, DEPTH, aux=True, ordered=True, schedule="cost", sync=True)
    snap("cost")
    for i in range(17):   # crosses PREV_ORDER_EVERY (8) twice
        r.render(cam, SPP, DEPTH, aux=True, ordered=True, schedule="previous", accumulate=True, sync=True)
        snap(f"previous[{i}]")
    r.render(cam, SPP, DEPTH, aux=True, ordered=True, consolidate=True, sync=True)
    snap("consolidate")
    snap("tile_costs", costs=r.tile_costs(cam, 2, DEPTH).copy())
    if band:
        for idx in (2, 3):
            bgra = r.denoise_mix(idx)
            snap(f"display[{idx}]", bgra=bgra.copy(), mix=_bits(r.read_mix()),
                 band=np.asarray(r.display_band()))
    return seen


def _assert_same(got, want, where):
    assert [s for s, _ in got] == [s for s, _ in want]
    for (step, g), (_, w) in zip(got, want):
        assert g.keys() == w.keys(), (where, step)
        for k in g:
            np.testing.assert_array_equal(g[k], w[k], err_msg=f"{where}, after {step}: {k}")


def test_reframing_equals_a_fresh_context(gpu, sky):
    with _renderer(sky) as r:
        walked = [_walk_frame(r, W, H, rows, 100 + i) for i, (W, H, rows) in enumerate(FRAMES)]
    for i, (W, H, rows) in enumerate(FRAMES):
        with _renderer(sky) as fresh:
            want = _walk_frame(fresh, W, H, rows, 100 + i)
        _assert_same(walked[i], want, f"frame {i} ({W}x{H})")


def _render_rows(r, W, H, y0, y1, seed):
    r.set_frame(W, H, np.arange(y0, y1, dtype=np.int32))
    r.init_rng(seed)
    r.render(camera_get_copy(scenes.camera_for(W, H)), SPP, DEPTH, aux=True, sync=True)
    n, d = r.read_aux()
    return _bits(r.read_accum()).reshape(y1 - y0, W, 4), _bits(n).reshape(y1 - y0, W, 3), _bits(d).reshape(y1 - y0, W)


def test_gather_maps_follow_their_source(gpu, sky):
    W = H = 32

    def dst_state():
        dst.synchronize()
        n, d = dst.read_aux()
        return _bits(dst.read_accum()).reshape(H, W, 4), _bits(n).reshape(H, W, 3), _bits(d).reshape(H, W)

    with _renderer(sky) as dst:
        dst.set_frame(W, H)
        src1 = _renderer(sky)
        top = _render_rows(src1, W, H, 0, 16, 7)
        dst.gather_rows(src1)
        dst.synchronize()
        src1.close()
        with _renderer(sky) as src2:   # may reuse src1's address
            bottom = _render_rows(src2, W, H, 16, 32, 8)
            dst.gather_rows(src2)
            for got, a, b in zip(dst_state(), top, bottom):
                np.testing.assert_array_equal(got[16:32], b)
                np.testing.assert_array_equal(got[0:16], a)
            middle = _render_rows(src2, W, H, 8, 24, 9)   # re-framed, new seed
            dst.gather_rows(src2)
            for got, a, b, m in zip(dst_state(), top, bottom, middle):
                np.testing.assert_array_equal(got[8:24], m)
                np.testing.assert_array_equal(got[0:8], a[0:8])
                np.testing.assert_array_equal(got[24:32], b[8:16])


def test_create_render_close_cycles(gpu, sky):
    W, H = 40, 32
    cam = camera_get_copy(scenes.camera_for(W, H))
    first = None
    for cycle in range(8):
        with _renderer(sky) as r:   # every call raises unless it returns CPT_OK
            r.set_frame(W, H)
            r.init_rng(5)
            r.render(cam, SPP, DEPTH, aux=True, path=("megakernel", "wavefront")[cycle % 2], sync=True)
            image = (_bits(r.read_accum()), r.denoise_mix(2).copy(), _bits(r.read_mix()))
        first = first or image
    for a, b in zip(image, first):
        np.testing.assert_array_equal(a, b)


def test_refused_band_keeps_the_good_one(gpu, sky):
    W, H = 64, 48
    with _renderer(sky) as r:
        r.set_frame(W, H, np.arange(13, 35, dtype=np.int32))   # band [16, 32) and its halo
        r.init_rng(11)
        r.render(camera_get_copy(scenes.camera_for(W, H)), SPP, DEPTH, aux=True, sync=True)
        r.denoise_mix_band(2, 16, 32)
        good = _bits(r.read_mix())
        assert good.shape == (16 * W, 3) and good.any()
        for y0, y1 in ((0, 16), (32, 48), (40, 64)):   # no halo rows rendered; past H'
            with pytest.raises(CptError):
                r.denoise_mix_band(3, y0, y1)
            assert r.display_band() == (16, 32)
            np.testing.assert_array_equal(_bits(r.read_mix()), good)
        # and the good band goes on from where it was
        r.denoise_mix_band(3, 16, 32)
        assert r.display_band() == (16, 32)
