"""The numpy restatement of cloud_knn and statistical_outlier_mask (tests/cloud_knn_reference.py) against independent
statements of the same thing, and the conditions under which the GPU tests (tests/test_cloud_knn_gpu.py) are not vacuous,
asserted here on the CPU."""
import numpy as np
import pytest

import cloud_knn_reference as ck
from cloud_reference import cloud_nearest_reference, radius_scalars, squared_distances
from multi_view_stereonet_amd.fusion import CLOUD_KNN_MAX, cloud_knn, statistical_outlier_mask  # noqa: F401  (the feature under test)


def test_the_limits_agree_with_the_package():
    assert ck.MAX_K == CLOUD_KNN_MAX == 64 and max(ck.ALL_K) == 64 and cloud_knn.__doc__ and statistical_outlier_mask.__doc__


@pytest.mark.parametrize("name", ck.CASE_IDS)
def test_k_1_is_cloud_nearest(name):
    c = ck.case(name)
    if True in c["exclude_self"]:                            # (cloud_nearest has no exclude_self)
        own = ck.cloud_knn_reference(c["query"], ck.case_target(name), 1, c["h"], True)
        assert (own["index"][:, 0] != np.arange(len(c["query"]))).all()
    got = ck.cloud_knn_reference(c["query"], ck.case_target(name), 1, c["h"])
    want = cloud_nearest_reference(c["query"], ck.case_target(name), c["h"])
    for key in ("dist2", "index", "within"):
        assert got[key].reshape(-1).tobytes() == want[key].tobytes(), key
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(got["mean"], np.where(want["within"] >= 1, np.sqrt(want["dist2"].astype(np.float64)), np.nan))


@pytest.mark.parametrize("name, k, exclude_self", ck.RUNS)
def test_the_first_k_of_a_full_lexsort(name, k, exclude_self):
    c, ref = ck.case(name), ck.case_reference(name, k, exclude_self)
    d2, ok = ck.candidates(c["query"], ck.case_target(name), c["h"], exclude_self)
    rows = np.broadcast_to(np.arange(d2.shape[1]), d2.shape)
    for i in range(0, len(d2), 7):                           # (every seventh query: a lexsort per row)
        cand = np.flatnonzero(ok[i])
        order = cand[np.lexsort((rows[i, cand], d2[i, cand]))][:k]          # the last key is the primary one
        assert ref["within"][i] == len(cand)
        assert ref["index"][i, :len(order)].tolist() == order.tolist() and (ref["index"][i, len(order):] == -1).all()
        assert ref["dist2"][i, :len(order)].tobytes() == d2[i, order].tobytes() and np.isposinf(ref["dist2"][i, len(order):]).all()
        # the key order: (d2 bits << 32) | row sorts as (d2, row)
        key = (d2[i, cand].view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64)
        assert cand[np.argsort(key)][:k].tolist() == order.tolist()
        assert np.isnan(ref["mean"][i]) == (len(cand) < k)


def test_lattice_in_closed_form():
    # the integer lattice {-3..3}^3 against its own origin: the neighbours by squared integer distance are 1 at 0, 6 at 1,
    # 12 at 2, 8 at 3, 6 at 4, 24 at 5, 24 at 6, 0 at 7, 12 at 8, 30 at 9 (the number of ways to write d2 as three squares)
    g = np.arange(-3, 4, dtype=np.float32)
    t = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * np.float32(0.125)
    q = np.zeros((1, 3), np.float32)
    ref = ck.cloud_knn_reference(q, t, 64, 0.125 * 3)
    shells = [(0, 1), (1, 6), (2, 12), (3, 8), (4, 6), (5, 24), (6, 24), (8, 12), (9, 30)]
    assert ref["within"][0] == sum(c for _, c in shells) == 123
    want = np.concatenate([np.full(c, d * 0.125 ** 2, np.float32) for d, c in shells])[:64]
    assert ref["dist2"][0].tobytes() == want.tobytes()
    idx = ref["index"][0]
    assert (np.diff(idx[1:7]) > 0).all() and (np.diff(idx[7:19]) > 0).all()       # inside a shell: ascending rows
    assert sorted(np.abs(t[idx[1:7]]).sum(axis=1).tolist()) == [0.125] * 6
    own = ck.cloud_knn_reference(t, t, 6, 0.125, exclude_self=True)               # the six face neighbours, less at the faces
    centre = len(t) // 2
    assert own["within"][centre] == 6 and own["mean"][centre] == 0.125 and centre not in own["index"][centre]
    assert own["within"].min() == 3 and np.isnan(own["mean"][own["within"] < 6]).all()


def test_mean_is_summed_in_slot_order():
    d2 = np.array([[1.0, 4.0, 9.0], [0.25, np.inf, np.inf]], np.float32)
    m = ck.mean_of_slots(d2, np.array([3, 1]), 3)
    assert m[0] == ((np.float64(0) + 1.0) + 2.0 + 3.0) / 3 and np.isnan(m[1])
    rng = np.random.default_rng(1)
    d2 = np.sort(rng.uniform(0, 1, (50, 64)).astype(np.float32), axis=1)
    m = ck.mean_of_slots(d2, np.full(50, 64), 64)
    exact = np.sqrt(d2.astype(np.longdouble)).sum(axis=1) / 64
    assert (np.abs(m - exact) <= 66 * 2.0 ** -53 * exact).all()


def test_statistics_and_their_bounds():
    assert ck.mean_stats_reference([np.nan, np.nan]) [0] == 0 and np.isnan(ck.mean_stats_reference([np.nan])[1])
    assert ck.mean_stats_reference([np.nan, 2.5]) == (1.0, 2.5, 0.0)
    c, mu, sd = ck.mean_stats_reference([1.0, np.nan, 3.0])
    assert (c, mu, sd) == (2.0, 2.0, np.sqrt(2.0))
    for n in ck.STATS_SIZES[2:]:
        m = ck.stats_input(n)
        v = m[~np.isnan(m)]
        assert 0 < np.isnan(m).sum() < n
        c, mu, sd = ck.mean_stats_reference(m)
        assert c == len(v) and abs(mu - np.mean(v)) <= 1e-15 and abs(sd - np.std(v, ddof=1)) <= 1e-15
        b_mu, b_sd = ck.mean_stats_bounds(m)
        # another order of the same sums (a running sum in longdouble, and the plain sequential fp64 order) stays inside
        seq_mu = np.cumsum(v)[-1] / len(v)
        seq_sd = np.sqrt(np.cumsum((v - seq_mu) ** 2)[-1] / (len(v) - 1))
        assert abs(seq_mu - mu) <= b_mu and abs(seq_sd - sd) <= b_sd
        assert b_mu <= 1e-9 * mu and b_sd <= 1e-9 * sd


def test_plane_with_planted_points():
    c, ref = ck.sor_case("plane"), ck.sor_reference("plane")
    kind = c["kind"]
    assert ref["keep"][kind == 0].all() and not ref["keep"][kind != 0].any()      # exactly the planted ones are rejected
    assert np.isfinite(ref["mean_dist"][kind == 1]).all()                         # (they do have their k neighbours)
    assert np.isnan(ref["mean_dist"][kind >= 2]).all() and (kind >= 2).sum() == 3
    # not a matter of the order of the rows
    perm = np.random.default_rng(5).permutation(len(kind))
    again = ck.statistical_outlier_reference(c["points"][perm], c["k"], c["std_ratio"], c["h"])
    assert (again["keep"] == ref["keep"][perm]).all()


def test_two_densities():
    from cloud_reference import radius_outlier_reference
    c, ref = ck.sor_case("two_density"), ck.sor_reference("two_density")
    assert ref["keep"].all()
    md = ref["mean_dist"]
    ratio = np.median(md[c["kind"] == 1]) / np.median(md[c["kind"] == 0])
    assert 2.9 < ratio < 3.1                                                      # spacings a factor 3 apart
    r = radius_outlier_reference(c["points"], *ck.RADIUS_COUNT)
    assert r[(c["kind"] == 0) & c["interior"]].all() and not r[c["kind"] == 1].any()


# ---- no GPU test passes emptily -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ck.CASE_IDS)
def test_every_gpu_case_holds_what_it_is_there_for(name):
    c = ck.case(name)
    for ex in c["exclude_self"]:
        d2, ok = ck.candidates(c["query"], ck.case_target(name), c["h"], ex)
        within = ok.sum(axis=1)
        ordered = np.sort(np.where(ok, d2, np.float32(np.inf)), axis=1)
        assert within.max() > 64                                                  # a candidate list longer than the longest list
        for k in c["ks"]:
            assert (within > k).any()
            tie = (within > k) & (ordered[:, k - 1] == ordered[:, k])               # the k-th and the next one are equally far
            assert tie.any(), (name, k)
            if name not in ck.SINGLE_IDS:
                assert (within < k).any() and (within == 0).any()
    assert set(ck.ALL_K) <= {k for n in ck.CASE_IDS for k in ck.case(n)["ks"]}
    assert {len(ck.case(n)["query"]) for n in ("n1", "n255", "n256", "n257")} == {1, 255, 256, 257}


def test_the_mixed_cases_hold_the_awkward_rows():
    for name in ("n255", "n256", "n257"):
        c = ck.case(name)
        q, t = c["query"], c["target"]
        assert (~np.isfinite(q)).any(axis=1).sum() >= 3 and (~np.isfinite(t)).any(axis=1).sum() >= 4
        assert (np.abs(np.nan_to_num(q, nan=0, posinf=0, neginf=0)).max(axis=1) > 2.0 ** 20 * c["h"]).sum() >= 3   # beyond the grid
        _, ok = ck.candidates(q, t, c["h"])
        within = ok.sum(axis=1)
        for k in ck.ALL_K:
            assert (within == k).any(), k                                         # exactly k candidates
        assert len(np.unique(t[np.isfinite(t).all(axis=1)], axis=0)) < np.isfinite(t).all(axis=1).sum()     # exact duplicates
        d2 = squared_distances(q, t)
        assert ((d2 == 0) & ok).any()                                             # a query on a target
    s = ck.case("self")
    assert s["target"] is None and s["exclude_self"] == (False, True)
    _, _, r2 = radius_scalars(ck.case("tiny")["h"])
    assert 0 < r2 < np.float32(2.0 ** -100)                                       # the two-cell reach
    up, down = ck.case("dense_up"), ck.case("dense_down")
    for c, sign in ((up, 1), (down, -1)):
        d = squared_distances(c["query"][:1], c["target"])[0]
        assert len(d) == 600 and (d <= radius_scalars(c["h"])[2]).all() and (np.diff(d) * sign >= 0).all() and d[0] != d[-1]


@pytest.mark.parametrize("name", ck.SOR_IDS)
def test_no_point_within_the_margin_of_its_threshold(name):
    c, ref = ck.sor_case(name), ck.sor_reference(name)
    margin = ck.outlier_margin(ref, c["k"], c["std_ratio"])
    has = ~np.isnan(ref["mean_dist"])
    gap = np.abs(ref["mean_dist"] - ref["threshold"])
    assert has.sum() >= 1600 and (gap[has] > margin[has]).all()                 # not one point excluded from the comparison
    assert margin[has].max() < 1e-12


@pytest.mark.parametrize("name", ck.WALK_IDS)
def test_the_walk_cases_are_cloud_nearests_hard_inputs(name):
    c = ck.case(name)
    q, t = c["query"], c["target"]
    assert c["ks"] == (1, 9) and len(q) <= 60 and len(t) <= 60
    h, inv, r2 = radius_scalars(c["h"])
    one, nine = ck.case_reference(name, 1), ck.case_reference(name, 9)
    want = cloud_nearest_reference(q, t, c["h"])
    for key in ("dist2", "index", "within"):
        assert one[key].reshape(-1).tobytes() == want[key].tobytes(), key
    assert nine["within"].tobytes() == want["within"].tobytes() and 0 < (want["within"] > 0).mean() < 1
    assert (want["within"] > 1).any() and (want["within"] < 9).any()
    cq, ct = np.floor(q * inv), np.floor(t * inv)
    if name == "reach2":
        assert 0 < r2 < np.float32(2.0 ** -100) and want["within"][0] >= 1 and want["dist2"][0] <= r2
        assert (want["within"] >= 9).any()                                        # a full list too
        accepted = squared_distances(q, t) <= r2
        assert (accepted & (np.abs(cq[:, None] - ct[None]).max(axis=2) == 2)).sum() >= 3     # pairs two cells apart
    else:
        assert ct.max() == 2 ** 20 - 1 and ct.min() == -2 ** 20                     # the grid's last cells, both ends
        beyond = (np.abs(q) > np.float32(2.0 ** 20 * c["h"])).any(axis=1)
        assert beyond.any() and (want["within"][beyond] > 0).any()                # a query beyond the edge with a neighbour
