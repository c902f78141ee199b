"""tests/cloud_reference.py against a float64 brute force, its tie rule, its metrics on a case worked out by hand, and
the claim behind the kernel's cell range: every accepted pair's target cell is visited."""
import numpy as np
import pytest

from cloud_reference import (cell_range, cloud_metrics_reference, cloud_nearest_reference, radius_outlier_reference,
                             radius_scalars, squared_distances, target_cells)

U = 2.0 ** -24          # unit roundoff of fp32
# Rounding bound of the fp32 d2 against the exact D = sum (q - p)^2 of the same fp32 coordinates: a difference carries
# one rounding (1 + e1), its square (1 + e1)^2 (1 + e2), and every square passes through at most two additions, each
# (1 + e): at most (1 + U)^5 on every non-negative term, so |d2 - D| <= ((1 + U)^5 - 1) D < 6 U D (no term here is
# small enough to underflow).  Two candidates keep their order when their exact squares differ by more than the sum
# of their bounds.
D2_BOUND = 6.0 * U


def _exact(query, target):
    q, p = np.asarray(query, np.float64), np.asarray(target, np.float64)
    return ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)


@pytest.mark.parametrize("h, spread", [(0.25, 1.0), (0.05, 0.5), (3.0, 20.0)])
def test_restatement_against_a_float64_brute_force(h, spread):
    rng = np.random.default_rng(21)
    target = rng.uniform(-spread, spread, (1500, 3)).astype(np.float32)
    query = rng.uniform(-1.6 * spread, 1.6 * spread, (1200, 3)).astype(np.float32)     # some of them far from every target
    ref = cloud_nearest_reference(query, target, h)
    r2 = np.float64(radius_scalars(h)[2])
    D = _exact(query, target)
    order = np.argsort(D, axis=1, kind="stable")
    rows = np.arange(len(query))
    d1, d2nd = D[rows, order[:, 0]], D[rows, order[:, 1]]
    clear_in = d1 * (1 + D2_BOUND) <= r2
    clear_out = d1 * (1 - D2_BOUND) > r2
    clear_order = (d2nd - d1) > D2_BOUND * (d1 + d2nd)
    sure = clear_in & clear_order
    assert sure.sum() > 100 and clear_out.sum() > 100
    np.testing.assert_array_equal(ref["index"][sure], order[sure, 0])
    assert (np.abs(ref["dist2"][sure].astype(np.float64) - d1[sure]) <= D2_BOUND * d1[sure]).all()
    assert (ref["index"][clear_out] == -1).all() and np.isinf(ref["dist2"][clear_out]).all()
    assert (ref["within"][clear_out] == 0).all()
    # within: every clearly inside pair counts, no clearly outside pair does
    lower = (D * (1 + D2_BOUND) <= r2).sum(1)
    upper = (D * (1 - D2_BOUND) <= r2).sum(1)
    assert (lower <= ref["within"]).all() and (ref["within"] <= upper).all()
    assert ref["dist2"].dtype == np.float32 and ref["index"].dtype == np.int64 and ref["within"].dtype == np.int32


def test_ties_go_to_the_lowest_row():
    target = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0.5, 0, 0], [0.5, 0, 0], [0, 0, -0.5]], np.float32)
    query = np.array([[0, 0, 0], [0.5, 0, 0], [5, 5, 5]], np.float32)
    ref = cloud_nearest_reference(query, target, 1.0)
    assert ref["index"].tolist() == [3, 3, -1]               # rows 3, 4 and 5 are all 0.5 away; 3 and 4 coincide
    assert ref["dist2"].tolist() == [0.25, 0.0, np.inf]
    assert ref["within"].tolist() == [6, 4, 0]               # d2 == r2 counts: rows 0, 1, 2 at distance exactly 1
    ref = cloud_nearest_reference(query, target[::-1], 1.0)
    assert ref["index"].tolist() == [0, 1, -1]
    # a non-finite target is nobody's neighbour, a non-finite query has none
    target[3] = (0.5, np.nan, 0)
    query[1] = (np.inf, 0, 0)
    ref = cloud_nearest_reference(query, target, 1.0)
    assert ref["index"].tolist() == [4, -1, -1] and ref["within"].tolist() == [5, 0, 0]
    assert radius_outlier_reference(target, 1.0, 1).tolist() == [True, False, False, False, True, True]


def test_a_finite_target_outside_the_grid_raises():
    target = np.zeros((4, 3), np.float32)
    target[2, 1] = 2.0 ** 20 * 0.5
    with pytest.raises(ValueError, match="max_dist too small for the target's extent"):
        cloud_nearest_reference(np.zeros((1, 3), np.float32), target, 0.5)
    target[2, 1] = np.nextafter(np.float32(2.0 ** 20 * 0.5), np.float32(0))
    target[3, 0] = -(2.0 ** 20) * 0.5
    assert cloud_nearest_reference(np.zeros((1, 3), np.float32), target, 0.5)["within"].tolist() == [2]
    target[1] = (3e38, 0, 0)                                 # finite, and t overflows: no cell either
    with pytest.raises(ValueError, match="max_dist too small"):
        cloud_nearest_reference(np.zeros((1, 3), np.float32), target, 0.5)
    target[1] = (np.inf, 0, 0)                               # not finite: nobody's neighbour, no error
    assert cloud_nearest_reference(np.zeros((1, 3), np.float32), target, 0.5)["within"].tolist() == [1]


def test_metrics_on_points_of_a_line():
    # truth at x = 0, 1, 2; pred at x = 0.125, 1, 2.5, 10 and one NaN row; threshold 0.25, cap 1.  Every number below is
    # exact in fp32.  pred -> truth: 0.125, 0, 0.5, (8 ->) cap 1: accuracy 1.625 / 4, two of four within 0.25.
    # truth -> pred: 0.125, 0, 0.5: completeness 0.625 / 3, two of three within 0.25.  F = 2 (1/2)(2/3) / (7/6) = 4/7.
    truth = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    pred = np.array([[0.125, 0, 0], [1, 0, 0], [np.nan, 0, 0], [2.5, 0, 0], [10, 0, 0]], np.float32)
    m = cloud_metrics_reference(pred, truth, 0.25, 1.0)
    assert m["n_pred"] == 4 and m["n_truth"] == 3
    assert m["accuracy"] == 1.625 / 4 and m["completeness"] == 0.625 / 3
    assert m["precision"] == 0.5 and m["recall"] == 2 / 3
    assert abs(m["fscore"] - 4 / 7) < 1e-15
    # the cap defaults to the threshold: 0.125, 0, 0.25, 0.25 and 0.125, 0, 0.25
    m = cloud_metrics_reference(pred, truth, 0.25)
    assert m["accuracy"] == 0.625 / 4 and m["completeness"] == 0.375 / 3 and m["precision"] == 0.5
    # nothing close: both fractions 0, F = 0
    m = cloud_metrics_reference(pred + np.float32(100), truth, 0.25)
    assert m["precision"] == m["recall"] == m["fscore"] == 0.0 and m["accuracy"] == 0.25


@pytest.mark.parametrize("scale", [10.0, 1.0e4, 5.0e5])
@pytest.mark.parametrize("h", [0.25, 0.1, 0.37, 2.0 ** -74])
def test_every_accepted_pairs_target_cell_is_in_the_querys_range(h, scale):
    """Pairs at a distance close to h (both sides of it), a third of them along one axis where the bound is tightest,
    around points at |t| ~ scale on every axis, both signs: where d2 <= r2, floor(t_target) lies in the range of cells
    the kernel visits for t_query, on every axis."""
    rng = np.random.default_rng(int(scale) + 5)
    hf, inv, r2 = radius_scalars(h)
    n = 400_000
    centre = (rng.choice([-1.0, 1.0], (n, 3)) * scale + rng.uniform(-3, 3, (n, 3))) * np.float64(hf)
    q = centre.astype(np.float32)
    step = rng.normal(size=(n, 3))
    step[: n // 3] = 0.0
    step[np.arange(n // 3), rng.integers(0, 3, n // 3)] = rng.choice([-1.0, 1.0], n // 3)
    step /= np.linalg.norm(step, axis=1, keepdims=True)
    if h > 1e-20:
        length = np.float64(hf) * (1.0 + rng.uniform(-1.0, 1.0, (n, 1)) * 2.0 ** rng.integers(-24, -1, (n, 1)))
    else:   # the squares are denormals, a few quanta of 2^-149 each: pairs up to ~1.12 h are accepted
        length = np.float64(hf) * rng.uniform(0.5, 2.0, (n, 1))
    p = (q.astype(np.float64) + step * length).astype(np.float32)
    dx, dy, dz = (q[:, a] - p[:, a] for a in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    accepted = d2 <= r2
    assert 0.2 * n < accepted.sum() < 0.9 * n                # the pairs straddle the radius
    _, tp, cp = target_cells(p, h)
    tq = (q - np.float32(0)) * inv
    lo, hi = cell_range(tq, r2)
    inside = (cp >= lo) & (cp <= hi)
    assert inside[accepted].all()
    cells = (hi - lo + 1)[accepted]
    if h > 1e-20:           # 3 cells per axis almost always, more where e = 2^-19 + |t| 2^-20 reaches over a face
        assert cells.min() == 3 and cells.max() <= (4 if scale < 100 else 5)
        if scale < 100:     # (and the claim is about THIS range: some rejected pair's cell lies outside it)
            assert (cells == 3).mean() > 0.999 and not inside[~accepted].all()
    else:
        assert cells.max() <= 7


def test_squared_distance_is_the_stated_expression():
    q = np.array([[0.1, 0.2, 0.3]], np.float32)
    p = np.array([[1.1, -0.7, 0.25]], np.float32)
    dx, dy, dz = (np.float32(q[0, a] - p[0, a]) for a in range(3))
    want = np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))
    assert squared_distances(q, p)[0, 0] == want
