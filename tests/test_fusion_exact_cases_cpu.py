"""The exact fusion scenes (tests/fusion_exact_cases.py) without a device: their closed form agrees with the float64
restatement, evaluates to the same bits in float32 and in float64 (the premise of comparing a device result with it bit
for bit), and decides what each case is there to decide, each on an exact boundary.  Also the restatement's margin share
on the planted analytic scene that tests/test_fusion_entries_gpu.py compares with the device."""
import functools

import numpy as np
import pytest

import fusion_exact_cases as fx
from fusion_reference import fuse_reference

NAMES = sorted(fx.CASES)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def restatement(case):
    K, T = fx.cameras(case)
    return fuse_reference(case.depth[:, None], K, T, case.neighbours,
                          valid=None if case.valid is None else case.valid[:, None], ref_views=case.ref_views,
                          max_reproj_px=case.max_reproj_px, max_rel_depth=case.max_rel_depth,
                          min_consistent=case.min_consistent)


@functools.lru_cache(maxsize=None)
def expected(name):
    return fx.closed_form(fx.CASES[name], with_taps=True)


def _agrees_with_the_restatement(case, exp):
    ref = restatement(case)
    np.testing.assert_array_equal(ref["count"][:, 0], exp["count"])          # (everywhere: margin pixels included)
    np.testing.assert_array_equal(ref["keep"][:, 0], exp["keep"])
    np.testing.assert_array_equal(_bits(ref["fused"][:, 0]), _bits(exp["fused"]))
    np.testing.assert_array_equal(ref["view"], exp["view"])
    np.testing.assert_array_equal(ref["pixel"], exp["pixel"])
    finite = np.isfinite(exp["fused"][exp["keep"]])                          # (an infinite depth has no position)
    np.testing.assert_array_equal(_bits(ref["points"][finite]), _bits(exp["points"][finite]))
    return ref


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_agrees_with_the_restatement(name):
    _agrees_with_the_restatement(fx.CASES[name], expected(name))


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_is_the_same_in_float32_and_float64(name):
    case, e64 = fx.CASES[name], expected(name)
    e32 = fx.closed_form(case, np.float32)
    assert e32["fused"].dtype == np.float32 and e32["points"].dtype == np.float32
    np.testing.assert_array_equal(e32["count"], e64["count"])
    np.testing.assert_array_equal(e32["keep"], e64["keep"])
    np.testing.assert_array_equal(e32["pixel"], e64["pixel"])
    np.testing.assert_array_equal(_bits(e32["fused"]), _bits(e64["fused"]))
    np.testing.assert_array_equal(_bits(e32["points"]), _bits(e64["points"]))
    # every fused depth and coordinate is a multiple of 2^-10 below 2^10: fp32 holds it exactly, in any order of the
    # operations and with or without fused multiply-adds
    for a in (e64["fused"], e64["points"]):
        assert (a * 1024 == np.round(a * 1024)).all() and np.abs(a).max(initial=0) < 1024
    assert set(np.unique(case.depth)) <= set(fx.DEPTHS.tolist()) | {0.0}


def test_variants_coincident_shifted_baseline():
    # (b) pins the direction: read the other way round (s -> r for r -> s) the shifted scene gives other counts
    c = fx.CASES["shifted"]
    other = fx.closed_form(c._replace(centre=2 * c.centre[0] - c.centre))["count"]
    assert (other != expected("shifted")["count"]).sum() > 50
    # (c) true parallax: every disparity, the half pixel among them, confirms somewhere
    c, e = fx.CASES["baseline_x"], expected("baseline_x")
    for d in fx.DEPTHS:
        assert (e["count"][0][c.depth[0] == d] > 0).any(), d
    for name in ("coincident", "shifted", "baseline_x", "baseline_y", "baseline_x_shifted"):
        hist = np.bincount(expected(name)["count"].reshape(-1), minlength=3)
        assert (hist[:3] > 0).all(), (name, hist)


def test_last_row_and_column():
    e = expected("edge")
    H, W = e["count"].shape[1:]
    y, x = np.mgrid[:H, :W]
    # row 0 looks into view 1 at (x + 2, y + 1): on the last column / row rejected, one pixel inside accepted
    np.testing.assert_array_equal(e["count"][0], ((x + 2 <= W - 2) & (y + 1 <= H - 2)).astype(np.int64))
    assert e["count"][0, 0, W - 3] == 0 and e["count"][0, 0, W - 4] == 1
    assert e["count"][0, H - 2, 0] == 0 and e["count"][0, H - 3, 0] == 1
    # row 1 looks back at (x - 2, y - 1)
    np.testing.assert_array_equal(e["count"][1], ((x - 2 >= 0) & (y - 1 >= 0)).astype(np.int64))
    wrong = fx.closed_form(fx.CASES["edge"], edge_inclusive=True)["count"]
    assert wrong[0, 0, W - 3] == 1 and wrong[0, H - 2, 0] == 1


@pytest.mark.parametrize("name", ["hole", "masked"])
def test_a_hole_or_a_masked_tap_disqualifies_its_four_pixels(name):
    e = expected(name)
    H, W = e["count"].shape[1:]
    want = np.ones((H, W), np.int64)
    want[H - 1], want[:, W - 1] = 0, 0
    want[2:4, 3:5] = 0                          # neighbour pixel (4, 3): the tap sets of x in {3, 4}, y in {2, 3}
    np.testing.assert_array_equal(e["count"][0], want)
    assert e["count"][1, 3, 4] == 0 and e["keep"][1].sum() == (H - 1) * (W - 1) - 1


@pytest.mark.parametrize("which", ["depth", "reproj_x", "reproj_y"])
def test_thresholds_are_strict(which):
    at, above, zero = (expected(f"{which}_{k}_threshold".replace("zero_threshold", "threshold_zero"))
                       for k in ("at", "above", "zero"))
    flips = above["count"] - at["count"]
    assert (flips >= 0).all() and flips.sum() >= 10            # exactly at the threshold: out; one float above: in
    wrong = fx.closed_form(fx.CASES[f"{which}_at_threshold"], strict=False)["count"]
    np.testing.assert_array_equal(wrong, above["count"])
    assert zero["count"].max() == 0 and not zero["keep"].any() and zero["pixel"].size == 0
    assert fx.closed_form(fx.CASES[f"{which}_threshold_zero"], strict=False)["count"].max() == 1


def test_min_consistent():
    c, e = fx.CASES["min_consistent_0"], expected("min_consistent_0")
    assert e["keep"].all() and (e["count"] == 0).any()
    np.testing.assert_array_equal(_bits(e["fused"][e["count"] == 0]), _bits(c.depth[e["count"] == 0]))
    assert e["pixel"].size == c.depth.size
    e = expected("min_consistent_M_plus_1")
    assert e["count"].max() == fx.CASES["min_consistent_M_plus_1"].neighbours.shape[1] and not e["keep"].any()


def test_slots_rows_references_and_masks():
    c, e = fx.CASES["slots_32"], expected("slots_32")
    assert c.neighbours.shape == (3, 32) and e["count"].max() == 32 and (e["count"] == 32).sum() > 20
    np.testing.assert_array_equal(_bits(e["fused"][e["keep"]]), _bits(c.depth[e["keep"]]))
    e = expected("skipped_row")
    assert e["count"][1].max() == 0 and not e["keep"][1].any() and e["keep"][0].any() and e["keep"][2].any()
    e = expected("skipped_row_min_0")
    assert e["count"][1].max() == 0 and e["keep"][1].all()
    c, e = fx.CASES["repeated_reference"], expected("repeated_reference")
    np.testing.assert_array_equal(e["count"][0], e["count"][2])
    n = int(e["keep"][0].sum())
    assert n > 0 and (e["view"][:n] == 0).all() and (e["view"][-n:] == 0).all() and (e["view"][n:-n] == 1).all()
    np.testing.assert_array_equal(e["points"][:n], e["points"][-n:])
    c, e = fx.CASES["valid_bytes"], expected("valid_bytes")
    assert set(np.unique(c.valid)) == {0, 1, 2, 255}
    reduced = fx.closed_form(c._replace(valid=(c.valid != 0).astype(np.uint8)))
    for k in ("count", "fused", "pixel", "points"):
        np.testing.assert_array_equal(e[k], reduced[k])
    assert (e["count"] > 0).any() and not e["keep"][c.valid[c.ref_views] == 0].any()


def test_smallest_shapes():
    for name in ("shape_1x1", "shape_1x7", "shape_7x1"):
        assert expected(name)["count"].max() == 0              # no interior tap set
    for name in ("shape_2x2", "shape_3x5", "shape_25x41", "shape_3x5_baseline", "shape_25x41_baseline",
                 "two_references"):
        assert expected(name)["keep"].any() and not expected(name)["keep"].all(), name
    assert fx.CASES["shape_25x41"].depth[0].size == 1025       # one pixel in a second workgroup
    assert expected("shape_25x41")["count"][:, 24, 40].max() == 0


# ---- values that are not depths --------------------------------------------------------------------------------------
PLANTED = ["baseline_x", "shifted", "shape_25x41_baseline"]
TAPPED = {"baseline_x": 3, "shifted": 1, "shape_25x41_baseline": 2}     # of the three planted pixels, at least


@pytest.mark.parametrize("min_consistent", [0, 1])
@pytest.mark.parametrize("name", PLANTED)
def test_planted_values_in_the_exact_scenes(name, min_consistent):
    case = fx.CASES[name]._replace(min_consistent=min_consistent)
    base = fx.closed_form(case, with_taps=True)
    tapped = set()
    for what, view, pixel, planted in fx.plants(case):
        exp = fx.closed_form(planted)
        _agrees_with_the_restatement(planted, exp)
        reach = fx.touched(case, base, view, pixel)
        # nothing else moves, bit for bit
        np.testing.assert_array_equal(exp["count"][~reach], base["count"][~reach], err_msg=what)
        np.testing.assert_array_equal(_bits(exp["fused"][~reach]), _bits(base["fused"][~reach]), err_msg=what)
        value = planted.depth[view].reshape(-1)[pixel]
        own = np.zeros_like(reach)
        own[np.asarray(case.ref_views) == view, pixel // reach.shape[2], pixel % reach.shape[2]] = True
        as_tap = reach & ~own
        assert own.any(), what
        if as_tap.any():
            tapped.add((view, pixel))
        assert exp["count"][own].max() == 0, what                           # never confirmed, whatever it is
        if value > 0:                                                       # +inf and the denormal pass "> 0"
            assert (exp["keep"][own] == (min_consistent == 0)).all(), what
            np.testing.assert_array_equal(_bits(exp["fused"][own]), _bits(np.where(exp["keep"][own], value, 0)))
        else:
            assert not exp["keep"][own].any() and (exp["fused"][own] == 0).all(), what
        # as a tap it takes its slot from every pixel whose tap set holds it: the count can only fall
        assert (exp["count"][as_tap] <= base["count"][as_tap]).all(), what
        if what.split("@")[0] == "denormal":        # (a depth like any other, only never anybody's: nothing to add)
            continue
        for i in range(len(case.ref_views)):        # a slot whose tap set holds the value cannot count
            slots = case.neighbours[i]
            holds = sum((base["taps"][i, j] == pixel).any(0) for j in range(len(slots)) if slots[j] == view)
            assert (exp["count"][i].reshape(-1) <= (slots >= 0).sum() - holds).all(), what
    print(f"{name}: planted pixels that are also taps: {sorted(tapped)}")
    assert len(tapped) >= TAPPED[name]


@functools.lru_cache(maxsize=None)
def _analytic_reference(what):
    sc = fx.analytic_scene()
    depth = sc["depth"] if what is None else fx.analytic_plants()[what][0]
    return fuse_reference(depth, sc["K"], sc["T_cam_in_world"], sc["neighbours"], images=sc["images"])


def test_planted_values_in_the_analytic_scene_keep_the_margin_share():
    base = _analytic_reference(None)
    assert base["margin"].mean() <= 1e-3, base["margin"].sum()
    assert base["keep"].mean() > 0.5
    for what, (depth, spots) in fx.analytic_plants().items():
        ref = _analytic_reference(what)
        print(f"{what}: {int(ref['margin'].sum())} margin pixels of {ref['margin'].size}")
        assert ref["margin"].mean() <= 1e-3, (what, ref["margin"].sum())
        reach = fx.analytic_reach(spots)
        np.testing.assert_array_equal(ref["count"][~reach], base["count"][~reach], err_msg=what)
        np.testing.assert_array_equal(ref["fused"][~reach], base["fused"][~reach], err_msg=what)
        assert (ref["count"] != base["count"]).any() or what == "denormal", what
        for view, pixel in spots:
            assert ref["count"][view].reshape(-1)[pixel] == 0
            assert not ref["keep"][view].reshape(-1)[pixel]                 # (min_consistent is 2)
