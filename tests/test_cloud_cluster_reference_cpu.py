"""The numpy restatement of cloud_clusters (tests/cloud_cluster_reference.py) held to hand-worked cases, to scipy's
connected components, to cloud_nearest's restatement, and the named cases of tests/test_cloud_cluster_gpu.py held to what
their names promise: no GPU."""
import numpy as np
import pytest

import cloud_cluster_reference as cc
from cloud_reference import cloud_nearest_reference, radius_scalars, squared_distances


def _labels(points, eps, min_points):
    ref = cc.cloud_clusters_reference(np.asarray(points, np.float32), eps, min_points)
    return ref, ref["label"].tolist()


# ---- hand-worked cases: the labels are written out here -----------------------------------------------------------------
def test_two_triples_and_a_loner():
    p = [[0, 0, 0], [5, 5, 5], [0.1, 0, 0], [9, 0, 0], [5.1, 5, 5], [0, 0.1, 0], [5, 5.1, 5]]
    ref, label = _labels(p, 0.25, 3)
    assert label == [0, 1, 0, -1, 1, 0, 1]
    assert ref["core"].tolist() == [True, True, True, False, True, True, True]
    assert ref["within"].tolist() == [3, 3, 3, 1, 3, 3, 3] and ref["within"].dtype == np.int32
    assert ref["count"].tolist() == [3, 3] and ref["core_count"].tolist() == [3, 3] and ref["first"].tolist() == [0, 1]
    _, label = _labels(p, 0.25, 4)                           # nobody is core: no cluster at all
    assert label == [-1] * 7


def test_a_border_point_between_two_clusters_joins_the_nearer_one():
    # a point between two triples of duplicates is core itself (1 + 3 + 3 within) and joins them into one cluster
    left, right, mid = [0.0, 0, 0], [0.4375, 0, 0], [0.1875, 0, 0]
    p = [right, right, right, left, left, left, mid]         # the right triple holds the lower rows
    ref, label = _labels(p, 0.25, 4)
    assert ref["core"].tolist() == [True] * 7 and label == [0] * 7
    # so the ends get company that the point between does not see: each end is core (4 within), the point between is
    # not (itself and the two ends)
    p = [right, [0.6, 0, 0], [0.6, 0.01, 0], left, [-0.2, 0, 0], [-0.2, 0.01, 0], mid]
    ref, label = _labels(p, 0.25, 4)
    assert ref["within"].tolist() == [4, 3, 3, 4, 3, 3, 3]
    assert ref["core"].tolist() == [True, False, False, True, False, False, False]
    assert label == [0, 0, 0, 1, 1, 1, 1]                    # 0.1875 from the left end, 0.25 from the right: left, row 3
    assert ref["count"].tolist() == [3, 4] and ref["core_count"].tolist() == [1, 1] and ref["first"].tolist() == [0, 3]
    assert not ref["tied"].any()


def test_a_border_point_at_exactly_equal_distances_goes_to_the_lower_core_row():
    d2 = squared_distances(cc.TIE_POINTS[6:7], cc.TIE_POINTS[[0, 3]])[0]
    assert d2[0] == d2[1] == radius_scalars(cc.H)[2]         # exactly eps from both, bit for bit
    for flip in (False, True):
        ref, label = _labels(cc._tie(flip), cc.H, 4)
        assert label == cc.TIE_LABELS.tolist() == [0, 0, 0, 1, 1, 1, 0]
        assert ref["core"].tolist() == [True, False, False, True, False, False, False]
        assert ref["tied"].tolist() == [False] * 6 + [True]
        assert ref["count"].tolist() == [4, 3] and ref["first"].tolist() == [0, 3]
    # the same seven points: row 6 is with the right triple, then (rows flipped) with the left one
    assert cc._tie(False)[0, 0] == 0.25 and cc._tie(True)[0, 0] == -0.25


def test_a_chain_whose_middle_link_is_not_core_does_not_merge_its_ends():
    # rows 0-2 and 4-6 are triples at the two ends; row 3 in the middle sees one point of each end, 3/16 away (exact)
    p = [[0, 0, 0], [0, 0.05, 0], [0.1875, 0, 0], [0.375, 0, 0], [0.5625, 0, 0], [0.75, 0, 0], [0.75, 0.05, 0]]
    ref, label = _labels(p, 0.25, 3)
    assert ref["within"].tolist() == [3, 3, 4, 3, 4, 3, 3]
    assert label == [0] * 7                                  # at 3 the middle is core: one chain
    ref, label = _labels(p, 0.25, 4)
    assert ref["core"].tolist() == [False, False, True, False, True, False, False]
    assert label == [0, 0, 0, 0, 1, 1, 1]                    # the middle is a border point (tied: the lower row, 2)
    assert ref["first"].tolist() == [2, 4] and ref["count"].tolist() == [4, 3] and ref["tied"].tolist()[3]


def test_min_points_1_is_euclidean_cluster_extraction():
    p = [[0, 0, 0], [3, 0, 0], [0.2, 0, 0], [np.nan, 0, 0], [0.4, 0, 0], [3, 0.2, 0], [9, 9, 9], [0.2, np.inf, 0]]
    ref, label = _labels(p, 0.25, 1)
    assert label == [0, 1, 0, -1, 0, 1, 2, -1]               # a lone finite point is a cluster; a non-finite row is noise
    assert ref["core"].tolist() == [True, True, True, False, True, True, True, False]
    assert ref["within"].tolist() == [2, 2, 3, 0, 2, 2, 1, 0]
    assert ref["count"].tolist() == [3, 2, 1] and ref["first"].tolist() == [0, 1, 6]


def test_no_point_at_all():
    ref = cc.cloud_clusters_reference(np.zeros((0, 3), np.float32), 0.25, 3)
    assert all(ref[k].shape == (0,) for k in cc.OUTPUTS)


# ---- against scipy, and against cloud_nearest's restatement ---------------------------------------------------------------
@pytest.mark.parametrize("name, min_points", cc.RUNS)
def test_core_partition_against_scipy(name, min_points):
    sparse = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    points, eps, _ = cc.case(name)
    ref = cc.case_reference(name, min_points)
    i, j, _ = cc._case_pairs(name)
    core = ref["core"]
    e = core[i] & core[j]
    n = len(points)
    graph = sparse.coo_matrix((np.ones(int(e.sum()), np.int8), (i[e], j[e])), shape=(n, n))
    _, comp = csgraph.connected_components(graph, directed=False)
    assert cc.same_partition(np.where(core, comp, -1), np.where(core, ref["label"], -1))
    assert len(ref["first"]) == len(np.unique(comp[core]))
    # ids by lowest core row
    rows = np.arange(n)
    assert all(ref["first"][c] == rows[core & (ref["label"] == c)].min() for c in range(min(len(ref["first"]), 50)))
    assert (np.diff(ref["first"]) > 0).all()


@pytest.mark.parametrize("name", [n for n in cc.CASE_IDS if n != "scene"])
def test_within_is_cloud_nearests(name):
    points, eps, mps = cc.case(name)
    near = cloud_nearest_reference(points, points, eps)
    for mp in mps:
        ref = cc.case_reference(name, mp)
        assert ref["within"].dtype == np.int32 and ref["within"].tobytes() == near["within"].tobytes()
        finite = np.isfinite(points).all(axis=1)
        assert (ref["core"] == (finite & (near["within"] >= mp))).all()
        assert not ref["core"][~finite].any() and (ref["label"][~finite] == -1).all() and (ref["within"][~finite] == 0).all()


def test_the_relation_is_symmetric_bit_for_bit():
    for name in ("n257", "tiny", "far", "nonfinite", "mixed_2000"):
        points, _, _ = cc.case(name)
        d2 = squared_distances(points, points)
        assert d2.tobytes() == np.ascontiguousarray(d2.T).tobytes(), name
        i, j, _ = cc._case_pairs(name)
        pairs = set(zip(i.tolist(), j.tolist()))
        assert all((b, a) in pairs for a, b in pairs), name


# ---- the named cases are what their names say -----------------------------------------------------------------------------
def test_the_permutation_case_has_no_tied_border_distance():
    name, mp = cc.PERMUTATION_CASE
    ref = cc.case_reference(name, mp)
    border = (ref["label"] >= 0) & ~ref["core"]
    assert border.sum() > 1000 and not ref["tied"].any()
    assert len(ref["first"]) > 100 and (ref["label"] < 0).sum() > 1000
    # the restatement itself: the rows permuted, the same partition
    points, eps, _ = cc.case(name)
    perm = cc.permutation(len(points))
    moved = cc.cloud_clusters_reference(points[perm], eps, mp)
    assert moved["core"].tobytes() == ref["core"][perm].tobytes() and moved["within"].tobytes() == ref["within"][perm].tobytes()
    assert cc.same_partition(moved["label"], ref["label"][perm])
    assert sorted(moved["count"].tolist()) == sorted(ref["count"].tolist())
    assert sorted(moved["core_count"].tolist()) == sorted(ref["core_count"].tolist())


def test_no_case_is_vacuous():
    def ref(name, mp):
        r = cc.case_reference(name, mp)
        return r, len(r["first"])
    assert ref("n1", 1)[1] == 1 and ref("n1", 2)[1] == 0
    for name in ("n255", "n256", "n257"):
        points, _, _ = cc.case(name)
        assert len(points) == int(name[1:])
        r, c = ref(name, 4)
        assert c > 3 and (r["label"] < 0).any()
    r, c = ref("n257", 12)
    assert c >= 2 and ((r["label"] >= 0) & ~r["core"]).sum() > 5
    r, c = ref("all_noise", 2)
    assert c == 0 and (r["label"] == -1).all() and (r["within"] == 1).all()
    r, c = ref("one_cluster", 3)
    assert c == 1 and (r["label"] == 0).all() and r["core"].all() and r["count"].tolist() == [600]
    r, c = ref("duplicates", 1027)
    assert c == 1 and (r["within"] == 1027).all() and r["count"].tolist() == [1027]
    assert ref("duplicates", 1028)[1] == 0
    for name in ("chain_up", "chain_down", "chain_permuted"):
        r, c = ref(name, 2)
        assert c == 1 and r["core"].all() and r["first"].tolist() == [0] and set(r["within"].tolist()) == {2, 3}
        r, c = ref(name, 3)
        assert c == 1 and (~r["core"]).sum() == 2 and (r["label"] == 0).all() and r["core_count"].tolist() == [1027]
    x = cc.case("chain_up")[0][:, 0]
    assert (np.diff(x) > 0).all() and (np.diff(cc.case("chain_down")[0][:, 0]) < 0).all()
    r, c = ref("bridge_core", 6)
    assert c == 1 and r["core"].all()
    r, c = ref("bridge_border", 6)
    assert c == 2 and (~r["core"]).sum() == 1 and (r["label"] >= 0).all() and r["count"].tolist() == [81, 80]
    assert len(cc.case("bridge_core")[0]) == len(cc.case("bridge_border")[0]) + 1
    r, c = ref("nonfinite", 4)
    assert (~np.isfinite(cc.case("nonfinite")[0]).all(axis=1)).sum() == 5 and c > 3
    points, eps, _ = cc.case("far")
    r, c = ref("far", 3)
    t = points * radius_scalars(eps)[1]
    assert c == 3 and sorted(r["count"].tolist()) == [16, 16, 21] and (r["label"] < 0).sum() == 1
    assert np.floor(t).max() == 2 ** 20 - 1 and np.floor(t).min() == -2 ** 20 and (np.abs(t[:, 0]) >= 5e5).sum() == 22
    points, eps, _ = cc.case("tiny")
    h, _, r2 = radius_scalars(eps)
    assert h == np.float32(2.0 ** -74) and 0 < r2 < 2.0 ** -100
    r, c = ref("tiny", 4)
    assert c > 3 and (r["label"] < 0).any()
    for mp, want in ((1, 700), (3, 700), (4, 0)):
        r, c = ref("many_small", mp)
        assert c == want and (want == 0 or (r["count"] == 3).all())
    assert len(cc.case("many_small")[0]) == 2100
    points, _, _ = cc.case("scene")
    assert len(points) == cc.MAX_POINTS == 16384
    r, c = ref("scene", 4)
    assert c > 40 and r["count"].max() > 11000 and (r["label"] < 0).sum() > 2000 and ((r["label"] >= 0) & ~r["core"]).sum() > 100
    assert all(len(cc.case(name)[0]) <= cc.MAX_POINTS for name in cc.CASE_IDS)


# ---- cloud_cluster_mask's restatement ---------------------------------------------------------------------------------------
def test_the_mask_rules():
    ref = {"label": np.array([0, 1, 1, -1, 2, 2, 2, 3, 3, -1], np.int64), "count": np.array([1, 2, 3, 2], np.int64)}
    m = cc.cluster_mask_reference
    assert m(ref, min_size=2).tolist() == [False, True, True, False, True, True, True, True, True, False]
    assert m(ref, keep_largest=1).tolist() == [False] * 4 + [True] * 3 + [False] * 3
    assert m(ref, keep_largest=2).tolist() == [False, True, True, False, True, True, True, False, False, False]   # the tie: id 1
    assert m(ref, min_size=3, keep_largest=2).tolist() == [False] * 4 + [True] * 3 + [False] * 3
    assert m(ref, keep_largest=0).tolist() == [False] * 10 and m(ref, min_size=0).tolist() == (ref["label"] >= 0).tolist()
    assert m(ref, keep=[True, False, False, True]).tolist() == [True, False, False, False, False, False, False, True, True, False]
    assert m(ref, min_size=9).tolist() == [False] * 10 and m(ref, keep_largest=9).tolist() == (ref["label"] >= 0).tolist()


def test_the_walk_cases_are_cloud_nearests_hard_inputs():
    points, eps, mps = cc.case("reach2")
    h, inv, r2 = radius_scalars(eps)
    assert mps == (1,) and len(points) == 96 and 0 < r2 < np.float32(2.0 ** -100)
    ref = cc.case_reference("reach2", 1)
    i, j, _ = cc._case_pairs("reach2")
    c = np.floor(points * inv)
    assert (np.abs(c[i] - c[j]).max(axis=1) == 2).sum() >= 6                       # neighbours two cells apart
    assert ref["core"].all() and 1 < len(ref["first"]) < 96 and ref["count"].max() > 1
    points, eps, mps = cc.case("grid_edge")
    ref = cc.case_reference("grid_edge", 1)
    c = np.floor(points * radius_scalars(eps)[1])
    assert mps == (1,) and len(points) == 60 and c.max() == 2 ** 20 - 1 and c.min() == -2 ** 20
    assert ref["core"].all() and 6 <= len(ref["first"]) < 60 and ref["count"].max() > 1
    for name in ("reach2", "grid_edge"):                                          # min_points = 1: no border, no noise
        r = cc.case_reference(name, 1)
        assert (r["label"] >= 0).all() and r["within"].tobytes() == cloud_nearest_reference(*(cc.case(name)[0],) * 2, cc.case(name)[1])["within"].tobytes()
