"""The reprojection's definition on the CPU: cpt_reproject_host, the function the
kernel runs, against the numpy restatement tests/reproject_model.py bit for bit, and the
restatement's own properties without the C code.  G-buffers and rays come from
tests/gbuffer_model.py, which test_gbuffer_model.py pins to the oracle."""
import numpy as np
import pytest

import reproject_model as rm
from cpppathtracer_amd import scenes
from cpppathtracer_amd.renderer import reproject_host

PAIRS = sorted(rm.camera_pairs(1, 1))


@pytest.fixture(scope="module")
def cases(oracle_mod):
    """{(W, H, pair): (inputs, model output, model info)}, computed once."""
    objs = scenes.scene_s4()
    out = {}
    for W, H in rm.FRAMES:
        for name, pair in rm.camera_pairs(W, H).items():
            c = rm.case(oracle_mod, objs, pair)
            out[(W, H, name)] = (c, *rm.reproject(**c, max_history=rm.MAX_HISTORY, plane_tol=rm.PLANE_TOL))
    return out


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("wh", rm.FRAMES, ids=lambda wh: "%dx%d" % wh)
def test_host_equals_the_model(cases, wh, pair):
    c, want, _ = cases[(*wh, pair)]
    got = reproject_host(**c, max_history=rm.MAX_HISTORY, plane_tol=rm.PLANE_TOL)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("max_history,plane_tol", [(1, 0.0), (8, 1e-3), (128, 1e-1)])
def test_host_equals_the_model_at_other_settings(cases, max_history, plane_tol):
    for pair in rm.MOVED:
        c = cases[(64, 48, pair)][0]
        want, _ = rm.reproject(**c, max_history=max_history, plane_tol=plane_tol)
        got = reproject_host(**c, max_history=max_history, plane_tol=plane_tol)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_host_rejects_bad_arguments(cases):
    c = cases[(16, 16, "sideways")][0]
    from cpppathtracer_amd import CptError
    for kw in ({"max_history": 0}, {"plane_tol": -1.0}, {"plane_tol": float("nan")}, {"plane_tol": float("inf")}):
        with pytest.raises(CptError) as e:
            reproject_host(**c, **{"max_history": 32, "plane_tol": 1e-2, **kw})
        assert e.value.status == 1
    other = dict(c, cam1=cases[(1, 1, "sideways")][0]["cam1"])
    with pytest.raises(CptError) as e:
        reproject_host(**other)
    assert e.value.status == 1


# ------------------------------------------------------------------ the model alone
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("wh", rm.FRAMES, ids=lambda wh: "%dx%d" % wh)
def test_reused_pixels_have_a_tap_of_their_own_id(cases, wh, pair):
    _, out, info = cases[(*wh, pair)]
    assert (info["own"][out[:, 3] > 0] >= 1).all()


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("wh", rm.FRAMES, ids=lambda wh: "%dx%d" % wh)
def test_counts_are_integers_within_the_cap(cases, wh, pair):
    c, out, info = cases[(*wh, pair)]
    blended, copied = info["kind"] == 1, info["kind"] == 2
    n = out[blended, 3]
    assert (n == np.floor(n)).all() and (n >= 1).all() and (n <= rm.MAX_HISTORY).all()
    assert (out[info["kind"] == 0] == 0).all()
    assert np.isfinite(out).all()
    # a copied pixel is a pixel of the history, all four floats
    hist = {row.tobytes() for row in c["accum"]}
    assert all(row.tobytes() in hist for row in out[copied])
    assert (out[copied, 3] <= rm.MAX_HISTORY).all()


@pytest.mark.parametrize("wh", rm.FRAMES, ids=lambda wh: "%dx%d" % wh)
def test_identical_cameras_keep_the_history(cases, wh):
    c, out, info = cases[(*wh, "identical")]
    A = c["accum"]
    cnt = A[:, 3]
    usable = (cnt >= 1) & np.isfinite(A[:, :3]).all(axis=1)
    keep = usable & (cnt <= rm.MAX_HISTORY)
    np.testing.assert_array_equal(out[keep].view(np.uint32), A[keep].view(np.uint32))
    assert (info["kind"][keep] == 2).all()
    over = usable & (cnt > rm.MAX_HISTORY)
    cap = np.float32(rm.MAX_HISTORY)
    want = np.concatenate([(A[over, :3] / cnt[over, None]) * cap, np.full((int(over.sum()), 1), cap, np.float32)], axis=1)
    np.testing.assert_array_equal(out[over].view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert (out[~usable] == 0).all()
    if wh != (1, 1):
        assert keep.any() and over.any() and (~usable).any()


@pytest.mark.parametrize("wh", rm.FRAMES, ids=lambda wh: "%dx%d" % wh)
def test_a_camera_turned_away_has_no_history(cases, wh):
    _, out, _ = cases[(*wh, "away")]
    assert (out == 0).all()


@pytest.mark.parametrize("pair", rm.MOVED)
@pytest.mark.parametrize("wh", [(64, 48), (67, 9), (16, 16)], ids=lambda wh: "%dx%d" % wh)
def test_moved_cases_reuse_and_reject(cases, wh, pair):
    """The condition on the fixtures: at least 5% of the frame is reused and at least 5% rejected,
    so no comparison on them passes on an all-zero or an all-copied output.  (1x1 has one pixel.)"""
    _, out, info = cases[(*wh, pair)]
    reused = float((out[:, 3] > 0).mean())
    print("%dx%d %s: reused %.3f (blended %.3f, copied %.3f), rejected %.3f" %
          (*wh, pair, reused, (info["kind"] == 1).mean(), (info["kind"] == 2).mean(), 1 - reused))
    assert reused >= 0.05 and 1 - reused >= 0.05


def test_the_sky_reprojects_only_under_the_look_at_change(cases):
    for pair in rm.MOVED:
        c, out, _ = cases[(64, 48, pair)]
        sky = c["id1"] < 0
        if pair == "look_at":
            assert sky.mean() >= 0.05 and (out[sky, 3] > 0).mean() >= 0.25
        else:
            assert not sky.any()


def test_disocclusions_are_rejected(cases):
    """A pixel whose taps all carry another object's id has no history, whatever the taps hold."""
    c, out, info = cases[(64, 48, "sideways")]
    assert (info["own"] == 0).any()
    assert (out[info["own"] == 0] == 0).all()
