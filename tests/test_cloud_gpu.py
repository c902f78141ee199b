"""cloud_nearest, radius_outlier_mask and cloud_metrics on the device (csrc/mvsn_cloud.hip) against the numpy
restatement (tests/cloud_reference.py): dist2, index and within exactly -- the restatement is the brute force over every
pair with the kernel's own fp32 operations, and the kernel claims to be that brute force for every input."""
import functools

import numpy as np
import pytest
import torch

from cloud_reference import (cloud_metrics_reference, cloud_nearest_reference, radius_outlier_reference,
                             radius_scalars)
from fusion_reference import nearest_neighbours
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard, bits_equal
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd.fusion import (cloud_nearest, depth_normals, fuse_depthmaps, point_normals,
                                             radius_outlier_mask)
from multi_view_stereonet_amd.metrics import cloud_metrics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INF = np.float32(np.inf)


def _nearest(query, target, h):
    return cloud_nearest(torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV), h)


def _arrays(got):
    assert got.dist2.dtype == torch.float32 and got.index.dtype == torch.int64 and got.within.dtype == torch.int32
    assert got.dist2.device.type == "cuda"
    return got.dist2.cpu().numpy(), got.index.cpu().numpy(), got.within.cpu().numpy()


def _equal(got, ref):
    dist2, index, within = got
    assert dist2.shape == ref["dist2"].shape
    np.testing.assert_array_equal(index, ref["index"])
    np.testing.assert_array_equal(within, ref["within"])
    np.testing.assert_array_equal(dist2.view(np.uint32), ref["dist2"].view(np.uint32))     # the bits


def _check(query, target, h):
    ref = cloud_nearest_reference(query, target, h)
    _equal(_arrays(_nearest(query, target, h)), ref)
    return ref


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _library_nearest(query, target, h, fill=POISON_NAN):
    """mvsn_cloud_index_build + mvsn_cloud_nearest on inputs that sit in poisoned buffers of their own (16-byte aligned
    only), with the workspace, the status word and the three outputs carved between guard bands and poisoned too: an
    element that is not written keeps the poison, a byte that is read before it is written changes a result between the
    two fills, a store outside a buffer breaks a band."""
    hf, inv, r2 = radius_scalars(h)
    n, m = len(query), len(target)
    guard = Guard(_alloc, fill)
    q = guard.poisoned(torch.from_numpy(np.ascontiguousarray(query)).to(DEV))
    t = guard.poisoned(torch.from_numpy(np.ascontiguousarray(target)).to(DEV))
    lib = _native.load()
    ws_bytes = lib.mvsn_cloud_workspace_bytes(m)
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    status = guard.empty((1,), torch.int64, DEV)
    dist2, index = guard.empty((n,), torch.float32, DEV), guard.empty((n,), torch.int64, DEV)
    within = guard.empty((n,), torch.int32, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_cloud_index_build(_native.ptr(t), m, float(hf), float(inv), _native.ptr(status),
                                                 _native.ptr(ws), ws_bytes, st), "mvsn_cloud_index_build")
        _native.check(lib.mvsn_cloud_nearest(_native.ptr(q), n, float(inv), float(r2), _native.ptr(ws), ws_bytes, m,
                                             _native.ptr(dist2), _native.ptr(index), _native.ptr(within), st),
                      "mvsn_cloud_nearest")
    torch.cuda.synchronize()
    guard.check()
    return (dist2.cpu().numpy(), index.cpu().numpy(), within.cpu().numpy()), int(status.item())


# ---- the hand case --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hand_case():
    nq, nt, h = 1027, 1031, 0.25
    hf = np.float32(h)
    rng = np.random.default_rng(41)
    t = rng.uniform(-3.0, 3.0, (nt, 3)).astype(np.float32)              # ~14^3 cells: less than one target per cell
    q = rng.uniform(-3.2, 3.2, (nq, 3)).astype(np.float32)
    t[100:110] = t[5]                                                   # exact duplicates: the tie goes to row 5
    q[5] = t[5]                                                         # and a query on top of them: d2 = 0
    q[6] = t[700]
    q[7] = t[105] + np.float32(0.01)
    # d2 == r2 exactly, and one ulp above (0.25^2 + (1.5 * 2^-14)^2 = 2^-4 + 1.125 ulp): far from everything else
    t[20], q[10] = (8.0, 8.0, 8.0), (8.25, 8.0, 8.0)
    t[21], q[11] = (0.0, 0.0, 8.0), (0.25, 1.5 * 2.0 ** -14, 8.0)
    # targets exactly on cell faces (t an integer on every axis), and the float just below a face on one axis
    for j, k in enumerate([(-3, 2, 0), (0, 0, 0), (5, -7, 1), (-1, -1, -1)]):
        t[200 + j] = np.asarray(k, np.float32) * hf
        q[200 + j] = t[200 + j] + np.array([0.1, -0.1, 0.05], np.float32)
        q[210 + j] = t[200 + j]
    below = np.nextafter(np.float32(0), np.float32(-np.inf))
    t[300], t[301], t[302] = (below, 1.1, 1.1), (1.1, -2.0 ** -22, 1.1), (1.5, 1.5, -2.0 ** -25)
    q[300], q[301], q[302] = (0.01, 1.1, 1.1), (1.1, 0.02, 1.1), (1.5, 1.5, 0.03)
    q[303], q[304] = (below, 1.1, 1.1), (-0.2, -0.2, np.nextafter(np.float32(-0.25), np.float32(-1)))
    # non-finite rows on both sides
    q[400], q[401], q[402] = (np.nan, 0, 0), (np.inf, 0, 0), (0.1, -np.inf, np.nan)
    t[400], t[401], t[402] = (np.nan, 0.1, 0.1), (0.1, -np.inf, 0.1), (np.nan, np.nan, np.nan)
    q[403] = (0.1, 0.1, 0.1)                                            # next to where those targets would be
    # queries far outside the grid: 4e6 cells out, just past the last cell, and one whose t overflows
    q[500], q[501], q[502] = (1.0e6, 0, 0), (2.0 ** 20 * h + 0.1, 0, -(2.0 ** 20) * h - 1.0), (-3.0e38, 3.0e38, 0)
    # rows 0 and N - 1 of the target are somebody's nearest
    t[0], t[nt - 1] = (5.0, 5.0, 5.0), (5.0, 5.0, -5.0)
    q[0], q[nq - 1] = (5.1, 5.0, 5.0), (5.0, 5.05, -5.0)
    return q, t, h


def test_hand_case_1027_queries_1031_targets():
    q, t, h = _hand_case()
    ref = _check(q, t, h)
    r2 = radius_scalars(h)[2]
    assert ref["index"][5] == 5 and ref["dist2"][5] == 0 and ref["within"][5] >= 11
    assert ref["index"][6] == 700 and ref["dist2"][6] == 0
    assert ref["index"][7] == 5 and ref["dist2"][7] > 0
    assert ref["index"][10] == 20 and ref["dist2"][10] == r2 and ref["within"][10] == 1
    assert ref["index"][11] == -1 and ref["within"][11] == 0
    dx, dy = np.float32(0.25), np.float32(1.5 * 2.0 ** -14)
    assert np.float32(dx * dx + dy * dy) == np.nextafter(r2, INF)       # what query 11 misses by
    assert (ref["index"][200:204] == np.arange(200, 204)).all() and (ref["index"][210:214] == np.arange(200, 204)).all()
    assert ref["index"][300:304].tolist() == [300, 301, 302, 300] and ref["dist2"][303] == 0
    assert (ref["index"][400:403] == -1).all() and (ref["within"][400:403] == 0).all() and np.isinf(ref["dist2"][400:403]).all()
    assert ref["within"][403] >= 1 and ref["index"][403] not in (400, 401, 402)
    assert (ref["index"][500:503] == -1).all() and (ref["within"][500:503] == 0).all()
    assert ref["index"][0] == 0 and ref["index"][-1] == len(t) - 1
    assert 0.2 < (ref["index"] >= 0).mean() < 0.95                       # both outcomes are common


# ---- densities, long record walks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("side, per_cell", [(4.275, 1), (1.376, 30)])
def test_uniform_targets_at_two_densities(side, per_cell):
    # 5000 targets in a cube of (side / h)^3 cells of h = 0.25: about `per_cell` targets per cell; 6000 queries in and
    # around it (24 workgroups of queries, the last one partly filled)
    rng = np.random.default_rng(42 + per_cell)
    t = rng.uniform(-side / 2, side / 2, (5000, 3)).astype(np.float32)
    q = rng.uniform(-side / 2 - 0.3, side / 2 + 0.3, (6000, 3)).astype(np.float32)
    assert 0.7 * per_cell < 5000 / (side / 0.25) ** 3 < 1.3 * per_cell
    ref = _check(q, t, 0.25)
    assert ref["within"].mean() > per_cell and (ref["within"] == 0).any()


def test_all_1027_targets_in_one_cell():
    # the long record walk: every query within reach walks all 1027 records of cell (1,1,1)
    rng = np.random.default_rng(43)
    t = rng.uniform(0.26, 0.49, (1027, 3)).astype(np.float32)
    t[500:520] = t[3]
    q = rng.uniform(-0.1, 0.85, (6000, 3)).astype(np.float32)
    ref = _check(q, t, 0.25)
    assert ref["within"].max() > 500 and (ref["within"] == 0).any()


def test_more_slot_block_counts_than_scan_threads():
    # 2^19 + 1 targets: a table of 2^21 slots, 2048 population sums of 1024 slots each for the scan's 1024 threads (a run
    # of 2 per thread); 2 targets per cell of h = 0.25 in a cube of 64^3 cells, 1027 queries in and around it
    nt, nq = 2 ** 19 + 1, 1027
    rng = np.random.default_rng(44)
    t = rng.uniform(-8.0, 8.0, (nt, 3)).astype(np.float32)
    q = rng.uniform(-8.2, 8.2, (nq, 3)).astype(np.float32)
    q[:8] = t[[0, 1, nt - 1, nt // 2, 1024, 1025, 2 ** 19, 2 ** 18]]    # on top of a target: d2 = 0, that row or a duplicate
    ref = _check(q, t, 0.25)
    assert (ref["dist2"][:8] == 0).all() and ref["index"][0] == 0 and ref["index"][2] == nt - 1
    assert ref["within"].mean() > 4 and (ref["within"] == 0).any()


# ---- far from the origin: the widened range, the clip to the grid ----------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cluster_at_half_a_million_cells_and_at_the_grids_edge(axis):
    h = 0.25
    rng = np.random.default_rng(44 + axis)
    t0 = rng.uniform(-1.0, 1.0, (800, 3)).astype(np.float32)
    q0 = rng.uniform(-1.2, 1.2, (1000, 3)).astype(np.float32)
    for sign in (1.0, -1.0):
        # |t| ~ 5e5 on this axis: a float there is h / 32 apart and e = 2^-19 + |t| 2^-20 ~ 0.48 cells
        shift = np.zeros(3, np.float32)
        shift[axis] = sign * 5.0e5 * h
        ref = _check(q0 + shift, t0 + shift, h)
        assert (ref["within"] > 0).mean() > 0.5
        # the last cells of the grid: targets up to the edge, queries on both sides of it
        edge = np.float32(2.0 ** 20 * h)
        shift[axis] = sign * (edge - 1.0)
        t, q = t0 + shift, q0 + shift
        top = np.nextafter(edge, np.float32(0))                         # the largest coordinate of cell 2^20 - 1
        t[:, axis] = np.clip(t[:, axis], -edge, top)                    # (-edge is in cell -2^20, the lowest)
        ref = _check(q, t, h)
        assert (np.abs(q[:, axis]) > edge).any() and (ref["within"][np.abs(q[:, axis]) > edge] > 0).any()


def test_tiny_max_dist_whose_square_is_a_denormal():
    # h = 2^-74: r2 = 2^-148 is two quanta of the denormal range, d2 is rounded to whole quanta and a pair 1.1 h apart
    # is accepted: the kernel reaches two cells there
    h = 2.0 ** -74
    rng = np.random.default_rng(45)
    t = (rng.uniform(-4, 4, (600, 3)) * h).astype(np.float32)
    q = (rng.uniform(-4.5, 4.5, (700, 3)) * h).astype(np.float32)
    t[0], q[0] = (0.95 * h, 0, 0), (2.05 * h, 0, 0)                     # cells 0 and 2, and within
    ref = _check(q, t, h)
    assert ref["within"][0] >= 1 and ref["dist2"][0] <= np.float32(2.0 ** -148)
    assert 0 < (ref["within"] > 0).mean() < 1


# ---- clustered keys --------------------------------------------------------------------------------------------------
def test_4096_targets_in_consecutive_cells_along_a_line():
    # clustered keys: 4096 consecutive cells along x (then along z: the key's low bits), one target each, shuffled
    rng = np.random.default_rng(46)
    k = rng.permutation(4096).astype(np.float32) - 2048.0
    for axis in (0, 2):
        t = np.full((4096, 3), 0.05, np.float32)
        t[:, axis] = (k + np.float32(0.5)) * np.float32(0.1)
        q = t[rng.permutation(4096)[:3000]] + rng.uniform(-0.05, 0.05, (3000, 3)).astype(np.float32)
        ref = _check(q, t, 0.1)
        assert (ref["index"] >= 0).all() and len(np.unique(ref["index"])) > 2000


# ---- range, empties, single points -----------------------------------------------------------------------------------
def test_target_out_of_range_raises():
    h = 0.5
    rng = np.random.default_rng(47)
    t = rng.uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
    q = rng.uniform(-1.0, 1.0, (50, 3)).astype(np.float32)
    for bad in (2.0 ** 20 * h, -(2.0 ** 20) * h - 1.0, 3.0e38):         # cell 2^20, below cell -2^20, t overflows
        far = t.copy()
        far[123, 1] = bad
        with pytest.raises(ValueError, match="max_dist too small for the target's extent"):
            _nearest(q, far, h)
        with pytest.raises(ValueError, match="max_dist too small"):
            cloud_nearest_reference(q, far, h)
    # the same coordinates in the QUERY are fine, and so is a non-finite target
    far = q.copy()
    far[7, 1], far[8, 0], far[9, 2] = 2.0 ** 20 * h, -(2.0 ** 20) * h - 1.0, 3.0e38
    t[5, 0] = np.inf
    _check(far, t, h)


def test_empties_and_single_points_on_the_device():
    pts = torch.rand(9, 3, device=DEV)
    got = cloud_nearest(torch.zeros(0, 3, device=DEV), pts, 0.1)
    assert got.dist2.shape == got.index.shape == got.within.shape == (0,) and got.dist2.device.type == "cuda"
    got = cloud_nearest(pts, torch.zeros(0, 3, device=DEV), 0.1)
    assert torch.isinf(got.dist2).all() and (got.index == -1).all() and (got.within == 0).all()
    assert got.dist2.device.type == "cuda" and got.within.dtype == torch.int32
    one = np.array([[0.3, -0.2, 0.1]], np.float32)
    near, far = one + np.float32(0.05), one + np.float32(1.0)
    for q, t in ((near, one), (far, one), (one, one)):
        _check(q, t, 0.1)
    assert _arrays(_nearest(near, one, 0.1))[1].tolist() == [0] and _arrays(_nearest(far, one, 0.1))[1].tolist() == [-1]


# ---- invariances ----------------------------------------------------------------------------------------------------
def test_permuting_the_target_and_calling_twice():
    rng = np.random.default_rng(48)
    t = rng.uniform(-1.0, 1.0, (5000, 3)).astype(np.float32)
    t[1000:1040] = t[17]                                                # ties, which a permutation re-orders
    q = rng.uniform(-1.1, 1.1, (4000, 3)).astype(np.float32)
    h = 0.12
    a, b = _nearest(q, t, h), _nearest(q, t, h)
    for x, y in zip(a, b):
        assert bits_equal(x, y)
    dist2, index, within = _arrays(a)
    perm = rng.permutation(5000)
    p_dist2, p_index, p_within = _arrays(_nearest(q, t[perm], h))
    np.testing.assert_array_equal(p_dist2.view(np.uint32), dist2.view(np.uint32))
    np.testing.assert_array_equal(p_within, within)
    # the row follows the permutation: among the targets at the least distance, the one with the lowest NEW row
    found = index >= 0
    assert (p_index >= 0).tolist() == found.tolist()
    same_point = (t[perm[p_index[found]]] == t[index[found]]).all(axis=1)
    assert same_point.all()
    untied = found & ~np.isin(index, np.r_[17, 1000:1040])
    np.testing.assert_array_equal(perm[p_index[untied]], index[untied])
    _equal((p_dist2, p_index, p_within), cloud_nearest_reference(q, t[perm], h))


def test_the_python_call_is_the_library_call():
    q, t, h = _hand_case()
    (dist2, index, within), status = _library_nearest(q, t, h)
    assert status == 0
    got = _arrays(_nearest(q, t, h))
    np.testing.assert_array_equal(got[0].view(np.uint32), dist2.view(np.uint32))
    np.testing.assert_array_equal(got[1], index)
    np.testing.assert_array_equal(got[2], within)


@pytest.mark.parametrize("fill", [POISON_NAN, POISON_FINITE], ids=["nan", "finite"])
def test_both_entries_stay_inside_their_buffers(fill):
    # the workspace, the status word and the outputs between guard bands, everything poisoned: every output element is
    # written (none keeps the poison) and nothing the kernels read is unwritten (the two fills agree with the restatement)
    q, t, h = _hand_case()
    got, status = _library_nearest(q, t, h, fill)
    assert status == 0
    _equal(got, cloud_nearest_reference(q, t, h))
    rng = np.random.default_rng(49)
    t = rng.uniform(-1.0, 1.0, (3001, 3)).astype(np.float32)            # no multiple of anything
    q = rng.uniform(-1.0, 1.0, (2049, 3)).astype(np.float32)
    got, status = _library_nearest(q, t, 0.2, fill)
    assert status == 0
    _equal(got, cloud_nearest_reference(q, t, 0.2))
    # a target out of range: the status bit, and still nothing outside the buffers
    t[2999, 2] = 1.0e6
    _, status = _library_nearest(q, t, 0.2, fill)
    assert status == 1


# ---- radius_outlier_mask, cloud_metrics ------------------------------------------------------------------------------
def test_radius_outlier_mask():
    rng = np.random.default_rng(50)
    pts = rng.uniform(-1.0, 1.0, (4000, 3)).astype(np.float32)          # ~ 2 neighbours within 0.1 on average
    pts[10], pts[11] = (5.0, 5.0, 5.0), (-5.0, 5.0, 5.0)                # isolated points
    pts[20] = pts[21] = (5.0, -5.0, 5.0)                                # an isolated duplicate pair: one neighbour each
    pts[30], pts[31] = (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0)
    dev = torch.from_numpy(pts).to(DEV)
    for k in (0, 1, 2, 5):
        got = radius_outlier_mask(dev, 0.1, k)
        assert got.dtype == torch.bool and got.shape == (4000,) and got.device.type == "cuda"
        want = radius_outlier_reference(pts, 0.1, k)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert 0 < want.sum() < 4000 or k == 0
        assert got[[10, 11]].tolist() == [k == 0] * 2 and got[[20, 21]].tolist() == [k <= 1] * 2
        assert got[[30, 31]].tolist() == [False, False]


def _metrics_agree(got, ref):
    assert got["n_pred"] == ref["n_pred"] and got["n_truth"] == ref["n_truth"]
    # the counts exactly: the fractions are quotients of the same integers
    assert got["precision"] == ref["close_pred"] / ref["n_pred"] and got["recall"] == ref["close_truth"] / ref["n_truth"]
    assert got["fscore"] == ref["fscore"]
    for key in ("accuracy", "completeness"):
        print(key, got[key], ref[key])
        assert abs(got[key] - ref[key]) <= 1e-12 * ref[key], key


def test_cloud_metrics_on_the_device_against_numpy():
    rng = np.random.default_rng(51)
    truth = np.concatenate([rng.uniform(-1, 1, (5000, 2)), np.zeros((5000, 1))], 1).astype(np.float32)
    pred = (truth[rng.permutation(5000)[:4000]] + rng.normal(0, 0.02, (4000, 3))).astype(np.float32)
    pred[7], truth[11], truth[12, 2] = np.nan, np.inf, -np.inf
    pred[pred[:, 0] > 0.7, 2] += 1.0                                    # a part of pred far off the sheet
    p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(truth).to(DEV)
    for threshold, max_dist in ((0.03, None), (0.03, 0.2), (0.01, 0.01)):
        ref = cloud_metrics_reference(pred, truth, threshold, max_dist)
        assert 0 < ref["precision"] < 1 and 0 < ref["recall"] < 1
        _metrics_agree(cloud_metrics(p, t, threshold, max_dist), ref)
    with pytest.raises(ValueError, match="no finite point"):
        cloud_metrics(torch.full((5, 3), float("nan"), device=DEV), t, 0.03)


# ---- the synthetic scene --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_cloud():
    sc = synthetic.fusion_scene(4, 48, 64, device=DEV)
    res = fuse_depthmaps(sc["depth"], sc["K"], sc["T_cam_in_world"], nearest_neighbours(4, 3))
    normals = point_normals(res, depth_normals(sc["depth"], sc["K"], T_cam_in_world=sc["T_cam_in_world"]))
    assert res.points.shape[0] > 4000
    return sc, res, normals


def test_scene_cloud_against_itself(scene_cloud):
    _, res, _ = scene_cloud
    m = cloud_metrics(res.points, res.points, 0.05)
    n = int(res.points.shape[0])
    assert m["precision"] == 1.0 and m["recall"] == 1.0 and m["fscore"] == 1.0
    assert m["accuracy"] == 0.0 and m["completeness"] == 0.0 and m["n_pred"] == n and m["n_truth"] == n
    nn = cloud_nearest(res.points, res.points, 0.05)
    assert (nn.dist2 == 0).all() and (nn.within >= 1).all()
    assert (nn.index <= torch.arange(n, device=DEV)).all()              # itself, or an earlier duplicate


def test_scene_cloud_pushed_along_its_normals(scene_cloud):
    """The points of view 1, pushed by delta along their normals (towards the camera), against the truth cloud of the
    other three views: mean analytic surface distance <= accuracy <= that + the truth cloud's sampling distance.

    Why the other views' points are the truth: were a pushed point's own origin among the truth points, its nearest
    distance would be delta to the last bit while its analytic distance is delta * cos(normal error) plus the origin's
    own distance from the surface (the fused depth is an average of interpolated depths: median 1e-5, up to 2e-2 world
    units on this scene), and the lower bound would hang on the sign of a 1e-6 effect.  Against an independent sampling
    of the same surfaces the nearest truth point is a lateral step away and both bounds have room: for every truth point
    y, dist(x, S) <= |x - y| + dist(y, S); and the nearest sample of a surface covered with spacing s is within s of the
    foot of x.  View 1 sits between views 0 and 2, so what it sees the others cover.

    The sampling distance is the scene's: the diagonal of one pixel's footprint at the largest depth, over the cosine of
    the steepest angle between a viewing ray and the plane's normal (the plane is the farther, more slanted surface)."""
    sc, res, normals = scene_cloud
    delta = 0.05
    mine = (res.view == 1) & (normals != 0).any(dim=1)
    truth = res.points[res.view != 1]
    pred = res.points[mine] + delta * normals[mine]
    assert int(mine.sum()) > 1000 and truth.shape[0] > 3000
    analytic = float(synthetic.fusion_scene_surface_distance(pred).mean())
    assert 0.9 * delta < analytic < 1.1 * delta
    fx = float(sc["K"][0, 0, 0])
    n = np.asarray(synthetic.SCENE_PLANE_NORMAL) / np.linalg.norm(synthetic.SCENE_PLANE_NORMAL)
    half_fov = np.arctan(np.hypot(32.0, 24.0) / fx) + 0.15              # image corner, plus half the arc of the cameras
    cos_slant = np.cos(np.arccos(abs(n[2])) + half_fov)
    sampling = float(sc["depth"].max()) / fx * np.sqrt(2.0) / cos_slant
    assert 0.1 < sampling < 1.0
    m = cloud_metrics(pred, truth, 2 * delta, max_dist=2.0)
    print("analytic", analytic, "accuracy", m["accuracy"], "sampling", sampling, m)
    assert analytic <= m["accuracy"] <= analytic + sampling
    assert m["n_pred"] == int(mine.sum()) and m["n_truth"] == int(truth.shape[0])
