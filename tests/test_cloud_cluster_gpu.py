"""cloud_clusters and cloud_cluster_mask on the device (csrc/mvsn_cloud_cluster.hip) against the numpy restatement
(tests/cloud_cluster_reference.py).  Every case goes through the C ABI with the cloud in a poisoned buffer and both
workspaces, the head, the index build's status word and every output between guard bands, under both poisons.  Every
output is an integer or exact by construction (the same fp32 distances, integer work on top): label, core, within, count,
core_count and first are compared byte for byte and no tolerance applies.

Figures of one MI355X run are in DESIGN.md section 24."""
import functools

import numpy as np
import pytest
import torch

import cloud_cluster_reference as cc
from cloud_reference import radius_scalars
from fusion_reference import nearest_neighbours
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd.fusion import (CloudClusters, cloud_cluster_mask, cloud_clusters, cloud_nearest,
                                             fuse_depthmaps, radius_outlier_mask)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISONS = (POISON_NAN, POISON_FINITE)


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _entry(points, eps, min_points, fill=POISON_NAN):
    """mvsn_cloud_index_build, mvsn_cloud_cluster_label, the read of the head, mvsn_cloud_cluster_emit, and
    mvsn_cloud_nearest on the same index: numpy arrays of the six outputs plus `nearest_within`."""
    hf, inv, r2 = radius_scalars(eps)
    n = len(points)
    guard = Guard(_alloc, fill)
    p = guard.poisoned(_to(points))
    lib = _native.load()
    index_bytes, ws_bytes = lib.mvsn_cloud_workspace_bytes(n), lib.mvsn_cloud_cluster_workspace_bytes(n)
    index_ws, ws = guard.empty((index_bytes,), torch.uint8, DEV), guard.empty((ws_bytes,), torch.uint8, DEV)
    status, head = guard.empty((1,), torch.int64, DEV), guard.empty((2,), torch.int64, DEV)
    within, core = guard.empty((n,), torch.int32, DEV), guard.empty((n,), torch.uint8, DEV)
    label = guard.empty((n,), torch.int64, DEV)
    nd, ni, nw = guard.empty((n,), torch.float32, DEV), guard.empty((n,), torch.int64, DEV), guard.empty((n,), torch.int32, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_cloud_index_build(_native.ptr(p), n, float(hf), float(inv), _native.ptr(status),
                                                 _native.ptr(index_ws), index_bytes, st), "mvsn_cloud_index_build")
        _native.check(lib.mvsn_cloud_cluster_label(_native.ptr(p), n, float(inv), float(r2), int(min_points),
                                                   _native.ptr(index_ws), index_bytes, _native.ptr(within), _native.ptr(core),
                                                   _native.ptr(head), _native.ptr(ws), ws_bytes, st),
                      "mvsn_cloud_cluster_label")
        c, uf_status = head.tolist()
        assert uf_status == 0 and 0 <= c <= n and int(status.item()) == 0            # the status words
        count, core_count, first = (guard.empty((c,), torch.int64, DEV) if c else None for _ in range(3))
        _native.check(lib.mvsn_cloud_cluster_emit(_native.ptr(p), n, float(inv), float(r2), _native.ptr(index_ws), index_bytes,
                                                  _native.ptr(core), _native.ptr(ws), ws_bytes, c, _native.ptr(label),
                                                  _native.ptr(count), _native.ptr(core_count), _native.ptr(first), st),
                      "mvsn_cloud_cluster_emit")
        _native.check(lib.mvsn_cloud_nearest(_native.ptr(p), n, float(inv), float(r2), _native.ptr(index_ws), index_bytes, n,
                                             _native.ptr(nd), _native.ptr(ni), _native.ptr(nw), st), "mvsn_cloud_nearest")
    torch.cuda.synchronize()
    guard.check()
    assert head.tolist() == [c, 0] and int(status.item()) == 0
    none = np.zeros(0, np.int64)
    core_bytes = core.cpu().numpy()
    assert set(np.unique(core_bytes).tolist()) <= {0, 1}
    return {"label": label.cpu().numpy(), "core": core_bytes.astype(bool), "within": within.cpu().numpy(),
            "count": count.cpu().numpy() if c else none, "core_count": core_count.cpu().numpy() if c else none,
            "first": first.cpu().numpy() if c else none, "nearest_within": nw.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def _device(name, min_points, fill=POISON_NAN):
    """Made once per (case, min_points, poison), never modified."""
    points, eps, _ = cc.case(name)
    return _entry(points, eps, min_points, fill)


def _same_bits(a, b, keys=cc.OUTPUTS):
    for key in keys:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


# ---- every case: one point (a cluster, and none at all: emit still writes -1), the workgroup edge (255, 256, 257), all
# ---- noise, one cluster, 1027 duplicates in one cell, chains of 1029 (deep trees; the root is the lowest row), a bridge
# ---- with a core and with a border middle, the planted tie, rows that are not finite, 5 * 10^5 cells and the grid's
# ---- edge, the two-cell reach, 700 roots to rank, the 16 384-point scene --------------------------------------------------
@pytest.mark.parametrize("name, min_points", cc.RUNS)
def test_cases_match_the_restatement_byte_for_byte(name, min_points):
    got, ref = _device(name, min_points), cc.case_reference(name, min_points)
    _same_bits(got, ref)
    assert got["within"].tobytes() == got["nearest_within"].tobytes()               # mvsn_cloud_nearest on the same index
    assert got["label"].max(initial=-1) == len(got["first"]) - 1 and got["count"].sum() == (got["label"] >= 0).sum()
    assert (got["core_count"] >= 1).all() and got["core_count"].sum() == got["core"].sum()
    assert (got["label"][got["first"]] == np.arange(len(got["first"]))).all()


@pytest.mark.parametrize("name, min_points", cc.RUNS)
def test_buffers_under_both_poisons(name, min_points):
    # (the guard bands of every buffer are checked inside _entry; an element nobody writes, or a read of foreign memory
    # that reaches a result, differs between the two fills)
    _same_bits(_device(name, min_points, POISON_NAN), _device(name, min_points, POISON_FINITE), cc.OUTPUTS + ("nearest_within",))


def test_the_hand_worked_tie_and_the_chains_root():
    for name in ("tie", "tie_flipped"):
        assert _device(name, 4)["label"].tolist() == cc.TIE_LABELS.tolist()
    for name in ("chain_up", "chain_down", "chain_permuted"):
        got = _device(name, 2)
        assert got["first"].tolist() == [0] and got["count"].tolist() == [1029] and (got["label"] == 0).all()
    assert len(_device("bridge_core", 6)["first"]) == 1 and len(_device("bridge_border", 6)["first"]) == 2
    none = _device("n1", 2)
    assert none["label"].tolist() == [-1] and none["first"].shape == (0,) and none["core"].tolist() == [False]


@pytest.mark.parametrize("name, min_points", [("scene", 4), ("chain_permuted", 3), ("duplicates", 1), ("many_small", 3)])
def test_calling_twice_gives_the_same_bytes(name, min_points):
    points, eps, _ = cc.case(name)
    _same_bits(_device(name, min_points), _entry(points, eps, min_points), cc.OUTPUTS + ("nearest_within",))


def test_permuting_the_rows_permutes_the_outputs_and_keeps_the_partition():
    name, mp = cc.PERMUTATION_CASE                                    # no tied border distance (asserted on the CPU)
    points, eps, _ = cc.case(name)
    perm = cc.permutation(len(points))
    base, moved = _device(name, mp), _entry(points[perm], eps, mp)
    assert moved["core"].tobytes() == base["core"][perm].tobytes()
    assert moved["within"].tobytes() == base["within"][perm].tobytes()
    assert cc.same_partition(moved["label"], base["label"][perm])
    assert len(moved["first"]) == len(base["first"]) and (moved["first"] != base["first"]).any()
    assert sorted(moved["count"].tolist()) == sorted(base["count"].tolist())
    assert sorted(moved["core_count"].tolist()) == sorted(base["core_count"].tolist())
    # and a case whose partition has no border rows at all, where nothing could be tied: the chains
    a, b = _device("chain_up", 2), _device("chain_permuted", 2)
    assert a["count"].tolist() == b["count"].tolist() == [1029]


# ---- the Python call ----------------------------------------------------------------------------------------------------
def _arrays(r):
    return {k: t.cpu().numpy() for k, t in zip(CloudClusters._fields, r)}


@pytest.mark.parametrize("name, min_points", [("n257", 12), ("scene", 10), ("many_small", 4), ("nonfinite", 4), ("n1", 1)])
def test_the_python_call_is_the_library_call(name, min_points):
    points, eps, _ = cc.case(name)
    r = cloud_clusters(_to(points), eps, min_points)
    assert isinstance(r, CloudClusters) and all(t.is_cuda for t in r)
    assert r.label.dtype == torch.int64 and r.core.dtype == torch.bool and r.within.dtype == torch.int32
    assert r.count.dtype == r.core_count.dtype == r.first.dtype == torch.int64
    _same_bits(_arrays(r), _device(name, min_points))
    near = cloud_nearest(_to(points), _to(points), eps)
    assert torch.equal(r.within, near.within)


def test_a_point_beyond_the_grid_raises():
    points, eps, _ = cc.case("n257")
    far = np.array(points)
    far[123, 1] = 2.0 ** 20 * eps
    with pytest.raises(ValueError, match="max_dist too small for the target's extent"):
        cloud_clusters(_to(far), eps, 4)
    empty = cloud_clusters(torch.zeros(0, 3, device=DEV), eps, 4)
    assert all(t.shape == (0,) and t.is_cuda for t in empty)


def _uploaded(name, min_points):
    ref = cc.case_reference(name, min_points)
    return ref, CloudClusters(*(_to(ref[k]) for k in cc.OUTPUTS))


@pytest.mark.parametrize("name, min_points", [("scene", 4), ("many_small", 3), ("n257", 12)])
def test_cloud_cluster_mask_on_uploaded_fixtures(name, min_points):
    ref, t = _uploaded(name, min_points)
    c = len(ref["first"])
    keep = np.random.default_rng(341).integers(0, 2, c).astype(bool)
    for rule in (dict(min_size=3), dict(min_size=40), dict(keep_largest=1), dict(keep_largest=3), dict(min_size=3, keep_largest=2),
                 dict(keep_largest=0), dict(min_size=10 ** 9), dict(keep=keep), dict(keep=np.zeros(c, bool))):
        want = cc.cluster_mask_reference(ref, **rule)
        if "keep" in rule:
            rule = dict(keep=_to(rule["keep"]))
        got = cloud_cluster_mask(t, **rule)
        assert got.is_cuda and got.dtype == torch.bool and got.cpu().numpy().tobytes() == want.tobytes(), rule


def test_cloud_cluster_mask_with_no_cluster_and_no_point():
    ref, t = _uploaded("all_noise", 2)
    for rule in (dict(min_size=0), dict(keep_largest=5), dict(keep=torch.zeros(0, dtype=torch.bool, device=DEV))):
        got = cloud_cluster_mask(t, **rule)
        assert got.is_cuda and got.shape == (343,) and not got.any()
    empty = cloud_clusters(torch.zeros(0, 3, device=DEV), 0.25, 1)
    assert cloud_cluster_mask(empty, keep_largest=1).shape == (0,) and cloud_cluster_mask(empty, keep_largest=1).is_cuda


# ---- end to end: a fused cloud with planted floaters --------------------------------------------------------------------
def test_fused_scene_the_floaters_go_and_nothing_else():
    """The analytic scene of test_cloud_gpu.py (a plane and a sphere in front of it, 4 views of 48 x 64) fused, and three
    specks of 40 mutually close points planted well off both surfaces.  Each speck passes radius_outlier_mask; the two
    largest clusters are the two surfaces, and keeping them drops the 120 planted points and nothing else.

    eps: the fused cloud's sampling distance is a pixel's footprint, depth / fx = 7 / (0.8 * 64) = 0.14 on the plane and
    more where it is seen at a slant; 0.5 is three to four of them, and the surfaces are 1.7 apart at their nearest."""
    sc = synthetic.fusion_scene(4, 48, 64, device=DEV)
    res = fuse_depthmaps(sc["depth"], sc["K"], sc["T_cam_in_world"], nearest_neighbours(4, 3))
    n = int(res.points.shape[0])
    assert n > 4000
    rng = np.random.default_rng(351)
    specks = np.concatenate([np.asarray(c) + rng.uniform(-0.03, 0.03, (40, 3))
                             for c in ([-1.5, -1.0, 3.0], [1.5, 1.0, 3.0], [0.0, 1.5, 2.5])]).astype(np.float32)
    assert float(synthetic.fusion_scene_surface_distance(torch.from_numpy(specks)).min()) > 1.0
    cloud = torch.cat([res.points, _to(specks)])
    assert radius_outlier_mask(cloud, 0.1, 8)[n:].all()              # the local filter passes every planted point
    clusters = cloud_clusters(cloud, 0.5, 4)
    print(f"fused {n} points + 120 planted: C = {clusters.first.shape[0]}, counts {clusters.count.tolist()[:8]}, "
          f"noise {int((clusters.label < 0).sum())}")
    mask = cloud_cluster_mask(clusters, keep_largest=2)
    assert mask[:n].all() and not mask[n:].any()
    assert clusters.first.shape[0] == 5 and sorted(clusters.count.tolist())[:3] == [40, 40, 40]
    assert torch.equal(cloud_cluster_mask(clusters, min_size=41), mask)
