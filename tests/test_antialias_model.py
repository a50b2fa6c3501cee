"""The host hooks of the antialiased presentation (cpt_aa_rays_host, cpt_aa_coverage_host,
cpt_present_aa_host) held bit for bit and byte for byte to the numpy restatement
tests/antialias_model.py, which is written from the definition's text; and the contract coverage of
cpt_antialias_capi.cpp's messages (tests/golden/capi_contract_antialias.json), as
tests/test_capi_contract_coverage.py holds the other implementation files'.  No GPU.
"""
import itertools
import json
import os
import re

import antialias_model as am
import numpy as np
import present_model as pm
import pytest
import test_capi_contract_coverage as cc

from cpppathtracer_amd import antialias, camera_get_copy, present, scenes

F = np.float32
WHITE = 2.5
FRAMES = am.SHAPES + [(9, 7)]
FIXTURE = os.path.join(cc.REPO, "tests", "golden", "capi_contract_antialias.json")
SOURCE = os.path.join(cc.CSRC, "cpt_antialias_capi.cpp")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ------------------------------------------------------------------------------------------- rays
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("wh", [(1, 1), (3, 5), (64, 48), (130, 70)], ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_rays_equal_the_restated_raygen(wh, S):
    """Every sub-sample ray of the corner, border and inner pixels, x = 0 and y = 0 (negative
    quotients) among them."""
    W, H = wh
    cam = camera_get_copy(scenes.camera_for(W, H))
    pixels = {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (W // 3, 0), (0, H // 3)}
    for x, y in sorted(pixels):
        o, d = antialias.rays_host(cam, W, H, S, x, y)
        mo, md = am.rays(cam, W, H, S, x, y)
        np.testing.assert_array_equal(_bits(o), _bits(mo), err_msg=f"origin of ({x}, {y})")
        np.testing.assert_array_equal(_bits(d), _bits(md), err_msg=f"direction of ({x}, {y})")
        assert np.isfinite(d).all() and len(np.unique(d, axis=0)) == S * S
    ox, oy = am.offsets(S)
    assert ox.min() == -(S - 1) / (2 * S) and oy.max() == (S - 1) / (2 * S) and (ox * 2 * S == np.round(ox * 2 * S)).all()


def test_rays_straddle_the_centre_ray():
    """The sub-samples surround the pixel's centre ray (gbuffer_model.camera_rays): mirrored
    sub-samples leave it in opposite directions.  Before the normalisation they are v +- e exactly;
    normalising is smooth, so the two deviations cancel up to its second-order term, which is below
    3 |e|^2 for unit v (the bound used), far below the deviation |e| itself."""
    import gbuffer_model as gm
    W, H = 64, 48
    cam = camera_get_copy(scenes.camera_for(W, H))
    _, centre = gm.camera_rays(cam)
    for x, y in ((10, 7), (63, 47), (1, 1)):
        _, d = antialias.rays_host(cam, W, H, 4, x, y)
        c = centre[y * W + x].astype(np.float64)
        d = d.astype(np.float64)
        for a, b in ((0, 15), (3, 12), (5, 10)):
            e = np.linalg.norm(d[a] - c)
            assert 1e-4 < e < 0.05
            assert np.linalg.norm((d[a] - c) + (d[b] - c)) < 3 * e * e + 1e-6


# --------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("kind", am.KINDS)
def test_coverage_equals_the_model_on_synthetic_planes(kind, S):
    """All one id, the three seams, a crease within one id, misses next to hits and random planes,
    at every border shape; sub-sample ids no centre holds raise the unmatched flag."""
    saw_edge = saw_unmatched = False
    for W, H in FRAMES:
        ids, normals = am.planes(kind, W, H, seed=W + H)
        for cos, stray in ((0.9, False), (0.9, True), (-1.0, False), (1.0, False)):
            sub_id, sub_n = am.sub_hits(W, H, S, ids, normals, seed=S + W, stray=stray)
            counts, flags = antialias.coverage_host(W, H, S, cos, ids, normals, sub_id, sub_n)
            want_counts, want_flags = am.coverage(W, H, S, cos, ids, normals, sub_id, sub_n)
            np.testing.assert_array_equal(counts, want_counts, err_msg=f"{kind} {W}x{H} cos {cos}")
            np.testing.assert_array_equal(flags, want_flags, err_msg=f"{kind} {W}x{H} cos {cos}")
            assert (counts.sum(axis=2) == S * S).all()
            non_edge = (flags & am.EDGE) == 0
            assert (counts[non_edge][:, am.SELF] == S * S).all() and not (flags[non_edge] & am.UNMATCHED).any()
            saw_edge |= bool((flags & am.EDGE).any())
            if stray:
                strayed = (sub_id.reshape(H, W, -1) == 77).any(axis=2) & ~non_edge
                assert ((flags[strayed] & am.UNMATCHED) != 0).all()
                saw_unmatched |= bool(strayed.any())
    assert saw_edge == (kind != "flat")
    if kind != "flat":
        assert saw_unmatched


def test_edges_of_the_seams_and_the_crease():
    W, H, S = 8, 6, 2
    for kind, cos, cols in (("vertical", 0.9, {3, 4}), ("crease", 0.9, {3, 4}), ("crease", -1.0, set()), ("flat", 1.0, set())):
        ids, normals = am.planes(kind, W, H)
        sub_id = np.repeat(ids[:, None], S * S, axis=1)
        sub_n = np.repeat(normals[:, None, :], S * S, axis=1)
        counts, flags = antialias.coverage_host(W, H, S, cos, ids, normals, sub_id, sub_n)
        assert {int(x) for x in np.nonzero((flags & am.EDGE).any(axis=0))[0]} == cols, kind
        # every sub-sample saw its own pixel's surface: all on k = 4, nothing unmatched
        assert (counts[..., am.SELF] == S * S).all() and not (flags & am.UNMATCHED).any()


@pytest.mark.parametrize("S", [2, 4])
def test_every_tie_of_the_nearest_match_rule(S):
    """A 3x3 frame whose centre pixel's sub-samples all carry id 1, for every subset of the nine
    pixels holding id 1: the centre pixel's counts equal the model's, whose choices are checked
    against the rule spelled out here (nearest in units of 1/2S, then k = 4, then the lowest k)."""
    W = H = 3
    normals = np.tile(np.array([0, 0, 1], dtype=F), (9, 1))
    sub_n = np.tile(np.array([0, 0, 1], dtype=F), (9, S * S, 1))
    sub_id = np.full((9, S * S), 1, dtype=np.int32)
    ties = 0
    for subset in range(512):
        ids = np.array([1 if subset >> k & 1 else 2 for k in range(9)], dtype=np.int32)
        counts, flags = antialias.coverage_host(W, H, S, 0.9, ids, normals, sub_id, sub_n)
        want = np.zeros(9, dtype=int)
        unmatched = False
        for s in range(S * S):
            sx, sy = 2 * (s % S) + 1 - S, 2 * (s // S) + 1 - S
            dist = {k: (sx - 2 * S * (k % 3 - 1)) ** 2 + (sy - 2 * S * (k // 3 - 1)) ** 2 for k in range(9) if subset >> k & 1}
            if not dist:
                unmatched = True
                want[4] += 1
                continue
            least = min(dist.values())
            nearest = [k for k in sorted(dist) if dist[k] == least]
            ties += len(nearest) > 1
            pick = 4 if 4 in nearest else nearest[0]
            assert am.attribute(W, H, 1, 1, S, s, 1, sub_n[4, s], ids, normals, 0.9) == pick
            want[pick] += 1
        if subset in (0, 511):   # one id everywhere: the centre is no edge pixel
            assert flags[1, 1] == 0 and counts[1, 1, 4] == S * S
            continue
        np.testing.assert_array_equal(counts[1, 1], want, err_msg=f"subset {subset:09b}")
        assert flags[1, 1] == (am.EDGE | (am.UNMATCHED if unmatched else 0))
    assert ties > 100
    # the first sub-sample between the pixel above (k = 1) and the pixel to the left (k = 3): the lower k
    ids = np.array([2, 1, 2, 1, 2, 2, 2, 2, 2], dtype=np.int32)
    counts, _ = antialias.coverage_host(W, H, S, 0.9, ids, normals, sub_id, sub_n)
    assert counts[1, 1, 1] + counts[1, 1, 3] == S * S and counts[1, 1, 1] > counts[1, 1, 3] > 0   # the diagonal's ties


# ---------------------------------------------------------------------------------------- resolve
def _valid_counts(W, H, S, seed):
    """Random coverages: S^2 spread over the in-frame pixels of each block; some all on k = 4."""
    rs = np.random.RandomState(seed)
    counts = np.zeros((H, W, 9), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            inside = [k for k, (dx, dy) in enumerate(am.BLOCK) if 0 <= x + dx < W and 0 <= y + dy < H]
            if rs.rand() < 0.4:
                counts[y, x, am.SELF] = S * S
                continue
            for k in rs.choice(inside, S * S):
                counts[y, x, k] += 1
    return counts


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("wh", FRAMES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_present_aa_equals_the_model(wh, S):
    W, H = wh
    T = present.srgb_thresholds_host()
    accum = pm.synthetic_accum(W * H, seed=40 + W)
    rgb = np.ascontiguousarray(pm.source_colour(pm.ACCUM, accum)[0])
    counts = _valid_counts(W, H, S, seed=W * H + S)
    self_only = counts[..., am.SELF] == S * S
    for (source, src), e in itertools.product((("accum", accum), ("filtered", rgb)), (1.0, 0.37)):
        for tone, transfer in itertools.product(pm.TONES, pm.TRANSFERS):
            got = antialias.present_aa_host(W, H, S, src, counts, e, source, tone, WHITE, transfer)
            want = am.present_aa(W, H, S, src, counts, e, pm.ACCUM if source == "accum" else pm.FILTERED, pm.TONES[tone], WHITE,
                                 pm.TRANSFERS[transfer], T)
            np.testing.assert_array_equal(got, want, err_msg=f"{source} {tone} {transfer} e {e}")
            plain = present.present_host(src, e, source, tone, WHITE, transfer).reshape(H, W, 4)
            np.testing.assert_array_equal(got[self_only], plain[self_only])   # non-edge pixels: cpt_present's bytes


def test_present_aa_mixes_after_the_tone_curve():
    """A bright pixel beside a dark one, half of each: the byte is the mean of the two tone-mapped
    values, not the tone-mapped mean radiance (which the bright side would saturate)."""
    W, H, S = 2, 1, 2
    accum = np.array([[100, 100, 100, 1], [0, 0, 0, 1]], dtype=F)
    counts = np.zeros((H, W, 9), dtype=np.uint8)
    counts[0, 0, 4] = counts[0, 0, 5] = 2
    counts[0, 1, 4] = 4
    out = antialias.present_aa_host(W, H, S, accum, counts, 1.0, "accum", "clamp", 4.0, "linear")
    assert out[0, 0].tolist() == [127, 127, 127, 255] and out[0, 1].tolist() == [0, 0, 0, 255]


def test_host_hooks_refuse_bad_arguments():
    from cpppathtracer_amd import CptError
    W, H, S = 4, 3, 2
    ids, normals = am.planes("vertical", W, H)
    sub_id, sub_n = am.sub_hits(W, H, S, ids, normals, 1)
    cam = camera_get_copy(scenes.camera_for(W, H))
    accum = pm.synthetic_accum(W * H, 3)
    counts = _valid_counts(W, H, S, 5)
    outside = counts.copy()
    outside[0, 0, 0] = 1
    for call in (lambda: antialias.rays_host(cam, W, H, 3, 0, 0), lambda: antialias.rays_host(cam, W, H, 2, W, 0),
                 lambda: antialias.rays_host(cam, W, H, 2, 0, -1), lambda: antialias.rays_host(cam, 0, H, 2, 0, 0),
                 lambda: antialias.coverage_host(W, H, 3, 0.9, ids, normals, np.zeros((W * H, 9)), np.zeros((W * H, 9, 3))),
                 lambda: antialias.coverage_host(W, H, S, 1.5, ids, normals, sub_id, sub_n),
                 lambda: antialias.coverage_host(W, H, S, float("nan"), ids, normals, sub_id, sub_n),
                 lambda: antialias.present_aa_host(W, H, S, accum, outside),
                 lambda: antialias.present_aa_host(W, H, S, accum, counts, tone=3),
                 lambda: antialias.present_aa_host(W, H, S, accum, counts, white=0.0),
                 lambda: antialias.present_aa_host(W, H, S, accum, counts, source=2)):
        with pytest.raises(CptError) as e:
            call()
        assert e.value.status == 1


# ------------------------------------------------------- the flat-colour frame's condition, on the CPU
@pytest.mark.parametrize("S", [2, 4])
def test_the_flat_colour_frame_has_few_unmatched_pixels(oracle_mod, S):
    """The condition of test_gpu_antialias.py's flat-colour tests, derived without a GPU: the G-buffer
    and the sub-sample hits of S4 + cylinder at 64x48 from tests/gbuffer_model.py (brute force, in
    reference order), the coverage from the host hook at normal_cos = -1.  At most 5% of the edge
    pixels may be unmatched."""
    import gbuffer_model as gm
    import tracked_reproject_model as tm
    W, H = am.FLAT_W, am.FLAT_H
    cam = camera_get_copy(scenes.camera_for(W, H))
    objs = tm.scene()
    gid, _, gn, _ = gm.gbuffer(oracle_mod, objs, cam)
    O = np.zeros((W * H, S * S, 3), dtype=F)
    D = np.zeros_like(O)
    for p in range(W * H):
        O[p], D[p] = antialias.rays_host(cam, W, H, S, p % W, p // W)
    sid, _, sn, _ = gm.first_hit(oracle_mod, objs, O.reshape(-1, 3), D.reshape(-1, 3))
    counts, flags = antialias.coverage_host(W, H, S, am.FLAT_COS, gid, gn, sid.reshape(W * H, -1), sn.reshape(W * H, -1, 3))
    edge = int(((flags & am.EDGE) != 0).sum())
    unmatched = int(((flags & am.UNMATCHED) != 0).sum())
    print(f"S = {S}: {edge} edge pixels, {unmatched} unmatched")
    assert edge > 200 and unmatched <= am.FLAT_UNMATCHED_SHARE * edge
    assert (counts.sum(axis=2) == S * S).all() and (counts[..., am.SELF] < S * S).any()   # and the frame is no vacuous case


# ------------------------------------------------------------------------------ contract coverage
def _formats():
    with open(SOURCE) as fh:
        src = fh.read()
    return src, ["".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))) for m in cc.FAIL.finditer(src)]


def test_every_fail_site_of_the_new_file_is_found():
    src, formats = _formats()
    sites = sum(len(re.findall(r"\bfail\(", line.split("//")[0])) for line in src.splitlines())
    assert len(formats) == sites and sites >= 8


def test_every_message_of_the_new_file_is_recorded():
    """Each fail(...) format of cpt_antialias_capi.cpp, and the text cpt_last_aa_ms hands to
    last_span_ms, is in the recorded contract with a status other than CPT_OK."""
    with open(FIXTURE) as fh:
        steps = json.load(fh)
    assert all(len(s) == 3 and isinstance(s[1], int) for s in steps)
    texts = sorted({s[2] for s in steps if s[1] != 0})
    src, formats = _formats()
    missing = [f for f in formats if not any(cc.pattern_of(f).fullmatch(t) for t in texts)]
    assert not missing, missing
    spans = re.findall(r'last_span_ms\(c,\s*&cpt_ctx::\w+,\s*&?\w+,\s*"((?:[^"\\]|\\.)*)"\)', src)
    assert len(spans) == 1 and spans[0] in texts
    # and the file stays outside the other coverage test's reach, whose counts are pinned
    assert not os.path.basename(SOURCE).startswith("cpt_capi")
