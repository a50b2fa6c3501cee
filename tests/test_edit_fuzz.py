"""The edit sequences of edit_fuzz.py against the oracle, on the CPU: that every frame is visible,
that the oracle's own refit round-trips, that the sequences reach what they are meant to reach,
and an independent restatement of the reference's refit (edit_fuzz.refit_reference, written from
bvh.cu:122-157 and object.cu:134-170) that test_gpu_edit_fuzz.py holds the library's host tree to.
These are conditions on the generators and the oracle; no library code runs here."""
import edit_fuzz as ef
import numpy as np
import pytest

from cpppathtracer_amd import camera_get_copy

SEQ = ef.sequences()
NAMES = list(SEQ)
REFIT_ONLY = ef.refit_only()
MIXED = [n for n in NAMES if SEQ[n][0] in ("mixed_edits", "mixed_large_edits")]
SEED = 5
MIN_CHANGED = 16


def _render(oracle_mod, sky, name, edits, walk=False):
    family, objs, cam, _ = SEQ[name]
    spp, depth = ef.PARAMS[family]
    cam = camera_get_copy(cam)
    W, H = int(cam["width"]), int(cam["height"])
    assert W <= 64 and H <= 40 and spp <= 2 and depth <= 8
    rows = np.arange(H, dtype=np.int32)
    rng = oracle_mod.init_rng(SEED, W, rows, threads=8)
    oracle_mod.set_walk(walk)
    try:
        if edits is None:
            acc, st, _, _ = oracle_mod.render(objs, cam, sky, rows, spp, depth, rng, threads=8)
        else:
            acc, st = oracle_mod.render_edited(objs, edits, cam, sky, rows, spp, depth, rng, threads=8)
        if walk:
            st["fallbacks"] = oracle_mod.last_fallbacks()
    finally:
        oracle_mod.set_walk(False)
    return acc, rng, st


_CHANGED = {}


def _changed(oracle_mod, sky, name):
    """Pixels whose accumulator bits differ from the previous frame's, per frame."""
    if name in _CHANGED:
        return _CHANGED[name]
    frames = SEQ[name][3]
    prev = _render(oracle_mod, sky, name, None)[0]
    out = []
    for f in range(len(frames)):
        acc = _render(oracle_mod, sky, name, ef.flat(frames[:f + 1]))[0]
        out.append(int((acc.view(np.uint32) != prev.view(np.uint32)).any(axis=1).sum()))
        prev = acc
    _CHANGED[name] = (out, prev.shape[0])
    return _CHANGED[name]


@pytest.mark.parametrize("name", NAMES)
def test_edits_are_visible(oracle_mod, sky, name):
    """Every frame changes at least 16 pixels of the oracle's image against the frame before."""
    changed, npix = _changed(oracle_mod, sky, name)
    print(f"{name}: pixels changed per frame {changed} of {npix}")
    assert min(changed) >= MIN_CHANGED, (changed, npix)


def test_report_pixels_changed_per_family(oracle_mod, sky):
    """Prints the least and the mean number of changed pixels per frame of every family."""
    fam = {}
    for name in NAMES:
        changed, npix = _changed(oracle_mod, sky, name)
        fam.setdefault(SEQ[name][0], []).extend(c / npix for c in changed)
    for k, v in fam.items():
        print(f"{k}: {len(v)} frames, changed share min {min(v):.3f} mean {np.mean(v):.3f}")
        assert min(v) > 0


@pytest.mark.parametrize("name", REFIT_ONLY)
def test_oracle_round_trips(oracle_mod, sky, name):
    """render_edited(objs, all frames + inverse) == render(objs): image, RNG end states, counters,
    and the diagnostic ordered walk's counters (its own tree is refit the same way)."""
    _, objs, _, frames = SEQ[name]
    edits = ef.flat(frames) + ef.inverse(objs, frames)
    for walk in (False, True):
        a0, r0, s0 = _render(oracle_mod, sky, name, None, walk)
        a1, r1, s1 = _render(oracle_mod, sky, name, edits, walk)
        np.testing.assert_array_equal(a1.view(np.uint32), a0.view(np.uint32))
        np.testing.assert_array_equal(r1, r0)
        assert s1 == s0, walk


@pytest.mark.parametrize("name", REFIT_ONLY)
def test_net_is_the_sequence(oracle_mod, sky, name):
    """net(...) in one batch gives the oracle's image of the whole sequence, and the same scene."""
    _, objs, _, frames = SEQ[name]
    cur = objs.copy()
    ef._apply(cur, ef.net(objs, frames))
    assert (cur == ef.states(objs, frames)[-1]).all()
    a0, r0, s0 = _render(oracle_mod, sky, name, ef.flat(frames))
    a1, r1, s1 = _render(oracle_mod, sky, name, ef.net(objs, frames))
    np.testing.assert_array_equal(a1.view(np.uint32), a0.view(np.uint32))
    np.testing.assert_array_equal(r1, r0)
    assert s1 == s0


@pytest.mark.parametrize("name", NAMES)
def test_parameters_finite_and_no_zero_box_face(name):
    """No NaN or infinite object parameter, and no leaf box face that is exactly +-0, in any
    state of any sequence (the byte comparisons of two refit histories rely on the latter)."""
    _, objs, _, frames = SEQ[name]
    for st in [objs] + ef.states(objs, frames):
        for o in st:
            vals = np.concatenate([o["center"], [o["radius"], o["y_pos"], o["height"]], o["material"]["kd"],
                                   [o["material"][k] for k in ("refractive_index", "emit_intensity", "smoothness",
                                                               "reflectivity")]])
            assert np.isfinite(vals).all()
            assert (ef.leaf_box(o) != 0).all(), o


@pytest.mark.parametrize("name", NAMES)
def test_refit_reference_equals_the_build(oracle_mod, name):
    """With no edits the independent bottom-up refit reproduces the built tree's boxes bit for
    bit (the build takes MIN/MAX over a node's objects in order, the refit over its two children:
    the same values while no +-0 tie and no NaN is involved)."""
    objs = SEQ[name][1]
    boxes, links = oracle_mod.build_bvh(objs)
    np.testing.assert_array_equal(ef.refit_reference(boxes, links, objs).view(np.uint32), boxes.view(np.uint32))


@pytest.mark.parametrize("name", MIXED)
def test_mixed_edits_coverage(oracle_mod, name):
    """In every mixed_edits sequence: some frame shrinks the reference tree's root box on a face
    and some frame grows it; the deepest leaf is edited; every edit kind occurs."""
    _, objs, _, frames = SEQ[name]
    boxes, links = oracle_mod.build_bvh(objs)
    roots = [ef.refit_reference(boxes, links, st)[0] for st in [objs] + ef.states(objs, frames)]
    grew = [bool((b[:3] < a[:3]).any() or (b[3:] > a[3:]).any()) for a, b in zip(roots, roots[1:])]
    shrank = [bool((b[:3] > a[:3]).any() or (b[3:] < a[3:]).any()) for a, b in zip(roots, roots[1:])]
    assert any(grew) and any(shrank), (grew, shrank)
    depths = ef.leaf_depths(links)
    deepest = max(depths.values())
    touched = {i for i, _ in ef.flat(frames)}
    assert any(depths[i] == deepest for i in touched)
    kinds = {k for frame in ef.kinds_of(name) for k in frame}
    want = set(ef.KINDS) - (set() if (objs["type"] == 1).any() else {"platform_y"})
    assert want <= kinds, want - kinds
    assert len(frames) == 4 and all(len(k) == len(b) for k, b in zip(ef.kinds_of(name), frames))
    if SEQ[name][0] == "mixed_large_edits":
        assert min(len(b) for b in frames) >= 40
    for b in frames:   # the same index twice in one batch
        idx = [i for i, _ in b]
        assert len(idx) > len(set(idx))


@pytest.mark.parametrize("name", NAMES)
def test_material_slots(name):
    """The refit-only sequences stay below the compaction threshold, and the sequence and net(...)
    number the material slots alike (a leaf carries its slot, so the device bytes of the two
    histories can be compared); `compaction` crosses the threshold after its first frame and
    before its last."""
    family, objs, _, frames = SEQ[name]
    table, crossed = ef.material_table(objs, frames)
    if family in ef.REFIT_ONLY:
        assert not crossed
        assert len(table) - len(ef.material_table(objs, [])[0]) <= ef.MAX_NEW_MATERIALS
        assert ef.material_table(objs, [ef.net(objs, frames)]) == (table, False)
        # and one call per edit numbers them as one batch per frame does
        assert ef.material_table(objs, [[e] for e in ef.flat(frames)]) == (table, False)
    elif family == "compaction":
        assert crossed
        assert not ef.material_table(objs, frames[:1])[1] and ef.material_table(objs, frames[:-1])[1]


def test_flip_last_flips_last():
    for name in NAMES:
        family, objs, _, frames = SEQ[name]
        cur = objs.copy()
        for f, batch in enumerate(frames):
            for i, o in batch:
                flip = (int(cur[i]["type"]) == 1) != (int(o["type"]) == 1)
                assert flip == (family == "flip_last" and f == len(frames) - 1), (name, f, i)
                cur[i] = o
