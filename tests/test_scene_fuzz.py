"""The fuzzed scenes of scene_fuzz.py against the oracle alone (no GPU): the conditions that keep
test_gpu_fuzz_parity.py from passing vacuously.  Every case really hits and misses, every material
and primitive type wins a hit somewhere, the axis-aligned cameras really shoot rays with exactly
zero direction components, the degenerate cameras really are NaN, and for every case the oracle's
reference walk and its restatement of the ordered walk (oracle.set_walk) give the same image and
RNG end states."""
import numpy as np
import pytest
import scene_fuzz as sf

SEED = 1234


def _render(oracle_mod, sky, objs, cam, spp, depth, walk=False):
    cam = oracle_mod.camera_get_copy(cam)
    W, H = int(cam["width"]), int(cam["height"])
    assert W <= 64 and H <= 40 and spp <= 3 and depth <= 16
    rows = np.arange(H, dtype=np.int32)
    rng = oracle_mod.init_rng(SEED, W, rows, threads=8)
    oracle_mod.set_walk(walk)
    try:
        acc, st, _, _ = oracle_mod.render(objs, cam, sky, rows, spp, depth, rng, threads=8)
    finally:
        oracle_mod.set_walk(False)
    return acc, rng, st


def _both_walks(oracle_mod, sky, objs, cam, spp, depth):
    acc, rng, st = _render(oracle_mod, sky, objs, cam, spp, depth)
    w_acc, w_rng, w_st = _render(oracle_mod, sky, objs, cam, spp, depth, walk=True)
    np.testing.assert_array_equal(w_acc.view(np.uint32), acc.view(np.uint32))
    np.testing.assert_array_equal(w_rng, rng)
    for k in ("segments", "hits", "misses"):
        assert w_st[k] == st[k], k
    return acc, st


def _wins(oracle_mod, sky, objs, cam, spp, depth, full, keep):
    """True when removing the objects outside `keep` changes the render: the paths are the same
    until a removed object would have been the closest hit, so one of them won a hit."""
    acc, rng, st = full
    a2, r2, s2 = _render(oracle_mod, sky, np.ascontiguousarray(objs[keep]), cam, spp, depth)
    return not (np.array_equal(a2.view(np.uint32), acc.view(np.uint32)) and np.array_equal(r2, rng) and
                s2["hits"] == st["hits"] and s2["misses"] == st["misses"])


@pytest.mark.parametrize("seed", sf.MIXED_SEEDS)
def test_mixed_hits_and_misses(oracle_mod, sky, seed):
    objs, cam = sf.mixed(seed)
    assert 8 <= (objs["type"] != sf.PLATFORM).sum() <= 60 and (objs["type"] == sf.PLATFORM).sum() <= 2
    assert 6 <= len({o["material"].tobytes() for o in objs})
    _, st = _both_walks(oracle_mod, sky, objs, cam, *sf.PARAMS["mixed"])
    print(seed, st)
    assert st["hits"] > 0 and st["misses"] > 0


def test_mixed_every_type_wins(oracle_mod, sky):
    """Over the mixed seeds, every material type 0-4 and every primitive type 0-2 is the winner of
    at least one hit: the render changes when the objects of that type are taken out."""
    assert len(sf.MIXED_SEEDS) >= 24
    spp, depth = sf.PARAMS["mixed"]
    mat_wins, prim_wins = {t: 0 for t in range(5)}, {t: 0 for t in range(3)}
    for seed in sf.MIXED_SEEDS:
        objs, cam = sf.mixed(seed)
        full = _render(oracle_mod, sky, objs, cam, spp, depth)
        for t in mat_wins:
            sel = objs["material"]["type"] == t
            mat_wins[t] += bool(sel.any() and _wins(oracle_mod, sky, objs, cam, spp, depth, full, ~sel))
        for t in prim_wins:
            sel = objs["type"] == t
            prim_wins[t] += bool(sel.any() and _wins(oracle_mod, sky, objs, cam, spp, depth, full, ~sel))
    print("seeds in which a material type wins a hit:", mat_wins, "a primitive type:", prim_wins)
    assert all(v > 0 for v in mat_wins.values()), mat_wins
    assert all(v > 0 for v in prim_wins.values()), prim_wins


@pytest.mark.parametrize("seed", sf.MIXED_LARGE_SEEDS)
def test_mixed_large(oracle_mod, sky, seed):
    objs, cam = sf.mixed_large(seed)
    assert (objs["type"] != sf.PLATFORM).sum() >= 200
    assert sf.zero_component_rays(oracle_mod.camera_get_copy(cam)) > 0
    _, st = _both_walks(oracle_mod, sky, objs, cam, *sf.PARAMS["mixed_large"])
    assert st["hits"] > 0 and st["misses"] > 0


@pytest.mark.parametrize("seed", sf.AXIS_SEEDS)
def test_axis_aligned_zero_components(oracle_mod, sky, seed):
    assert len(sf.AXIS_SEEDS) >= 6 and {sf.AXIS_KINDS[s % 5] for s in sf.AXIS_SEEDS} == set(sf.AXIS_KINDS)
    objs, cam = sf.axis_aligned(seed)
    c = oracle_mod.camera_get_copy(cam)
    W, H = int(c["width"]), int(c["height"])
    assert W % 2 == 0 and H % 2 == 0 and float(c["lens_radius"]) == 0.0
    d = sf.primary_directions(c)
    assert np.isfinite(d).all()
    zeros = sf.zero_component_rays(c)
    kind = sf.AXIS_KINDS[seed % 5]
    print(seed, kind, f"{W}x{H}", "rays with a zero component:", zeros, "per axis:", (d == 0.0).sum(axis=(0, 1)))
    # the centre row (d.y == 0); for the four axis views also the centre column
    assert (d[H // 2, :, 1] == 0.0).all()
    assert zeros >= (W if kind == "level" else W + H - 1)
    # a box face and a cap plane at the camera's own coordinate on a zeroed axis
    o = np.asarray(c["origin"], dtype=np.float32)
    sph, cyl = objs[objs["type"] == sf.SPHERE], objs[objs["type"] == sf.CYLINDER]
    faces = np.concatenate([sph["center"] - sph["radius"][:, None], sph["center"] + sph["radius"][:, None]])
    zeroed = [1] if kind == "level" else [1, 0 if kind in ("+z", "-z") else 2]
    for ax in zeroed:
        assert (faces[:, ax] == o[ax]).any(), ax
    caps = np.concatenate([cyl["center"][:, 1] + cyl["height"] / 2, cyl["center"][:, 1] - cyl["height"] / 2])
    assert (caps == o[1]).any()
    _, st = _both_walks(oracle_mod, sky, objs, cam, *sf.PARAMS["axis_aligned"])
    assert st["hits"] > 0


@pytest.mark.parametrize("seed", sf.INSIDE_SEEDS)
def test_inside_hits(oracle_mod, sky, seed):
    assert len(sf.INSIDE_SEEDS) >= 6 and {sf.INSIDE_KINDS[s % 4] for s in sf.INSIDE_SEEDS} == set(sf.INSIDE_KINDS)
    objs, cam = sf.inside(seed)
    spp, depth = sf.PARAMS["inside"]
    assert depth >= 2
    _, st = _both_walks(oracle_mod, sky, objs, cam, spp, depth)
    print(seed, sf.INSIDE_KINDS[seed % 4], st)
    assert st["hits"] > 0
    # every primary ray starts inside (or under) something: it is hit at depth 1 already
    _, _, st1 = _render(oracle_mod, sky, objs, cam, spp, 1)
    if sf.INSIDE_KINDS[seed % 4] != "below_platform":
        assert st1["misses"] == 0 and st1["hits"] == st1["segments"]


@pytest.mark.parametrize("family", ["edge_materials", "edge_geometry"])
def test_edge_families(oracle_mod, sky, family):
    cases = getattr(sf, family)()
    for name, (objs, cam) in cases.items():
        _, st = _both_walks(oracle_mod, sky, objs, cam, *sf.PARAMS[family])
        print(family, name, st)
        assert st["hits"] > 0, name


def test_degenerate_camera_is_nan(oracle_mod, sky):
    for name, (objs, cam) in sf.degenerate_camera().items():
        c = oracle_mod.camera_get_copy(cam)
        basis = np.concatenate([np.asarray(c[k], dtype=np.float32).reshape(-1)
                                for k in ("u", "v", "w", "top_left_corner", "horizontal", "vertical")])
        assert np.isnan(basis).any(), name
        assert (int(c["width"]), int(c["height"])) == (16, 8)
        acc, st = _both_walks(oracle_mod, sky, objs, cam, *sf.PARAMS["degenerate_camera"])
        print(name, st, "NaN accumulators:", int(np.isnan(acc[:, :3]).any(axis=1).sum()))
