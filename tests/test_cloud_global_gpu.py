"""cloud_fpfh, feature_nearest, cloud_ransac and cloud_register_global on the device (csrc/mvsn_cloud_fpfh.hip,
mvsn_cloud_match.hip, mvsn_cloud_ransac.hip) against the numpy restatement (tests/cloud_global_reference.py).  Every case
goes through the C ABI with every input, the workspace and every output between guard bands under both poisons.

Everything is compared bit for bit.  spfh, pairs, the matches and (hypothesis, inliers, status) are exact by construction
(single fp32 operations, integer counts and orders).  features, T64 and T are fp64 sequences of + - x / sqrt, rint and
conversions, one operation per step, that the device rounds as numpy does (DESIGN.md section 23 records that this held on
the MI355X), so no bound is derived here: were a device to round one of them differently these tests would say so.

The end-to-end test measures the errors of cloud_register started from the true motion with the restatement of section 20
(tests/cloud_register_reference.py) and prints them; nothing is hard-coded."""
import functools

import numpy as np
import pytest
import torch

import cloud_global_reference as cg
import cloud_register_reference as cr
from cloud_reference import radius_scalars
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd.fusion import (cloud_fpfh, cloud_normals, cloud_ransac, cloud_register, cloud_register_global,
                                             feature_nearest)
from multi_view_stereonet_amd.metrics import cloud_metrics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISONS = (POISON_NAN, POISON_FINITE)


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a copy: the cases are read-only)


def _same_bits(a, b, keys):
    for key in keys:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


# ---- FPFH ---------------------------------------------------------------------------------------------------------------
FPFH_KEYS = ("spfh", "pairs", "features")


def _fpfh_entry(points, normals, h, min_neighbours=3, fill=POISON_NAN):
    """mvsn_cloud_index_build of the cloud itself, then mvsn_cloud_fpfh; every buffer between guard bands and poisoned."""
    hf, inv, r2 = radius_scalars(h)
    n = len(points)
    guard = Guard(_alloc, fill)
    p, nm = guard.poisoned(_to(points)), guard.poisoned(_to(normals))
    lib = _native.load()
    ws_bytes = lib.mvsn_cloud_workspace_bytes(n)
    ws, status = guard.empty((ws_bytes,), torch.uint8, DEV), guard.empty((1,), torch.int64, DEV)
    spfh, pairs = guard.empty((n, 33), torch.int32, DEV), guard.empty((n,), torch.int32, DEV)
    features = guard.empty((n, 33), torch.float32, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_cloud_index_build(_native.ptr(p), n, float(hf), float(inv), _native.ptr(status),
                                                 _native.ptr(ws), ws_bytes, st), "mvsn_cloud_index_build")
        _native.check(lib.mvsn_cloud_fpfh(_native.ptr(p), _native.ptr(nm), n, float(hf), float(inv), float(r2), min_neighbours,
                                          _native.ptr(ws), ws_bytes, _native.ptr(spfh), _native.ptr(pairs),
                                          _native.ptr(features), st), "mvsn_cloud_fpfh")
    torch.cuda.synchronize()
    guard.check()
    assert int(status.item()) == 0
    return {"spfh": spfh.cpu().numpy(), "pairs": pairs.cpu().numpy(), "features": features.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def _fpfh_device(name, fill=POISON_NAN):
    c = cg.fpfh_case(name)
    return _fpfh_entry(c["points"], c["normals"], c["h"], fill=fill)


@pytest.mark.parametrize("name", cg.FPFH_IDS)
def test_fpfh_matches_the_restatement_bit_for_bit(name):
    got, ref = _fpfh_device(name), cg.fpfh_case_reference(name)
    print(f"{name}: {len(got['pairs'])} points, pairs up to {int(got['pairs'].max())}, {int(ref['defined'].sum())} defined rows")
    _same_bits(got, ref, ("spfh", "pairs"))
    assert (got["spfh"].reshape(-1, 3, 11).sum(axis=2) == got["pairs"][:, None]).all()
    _same_bits(got, ref, ("features",))
    if name == "crowded":
        assert got["pairs"].max() > 256
    if name in ("alone", "n1"):
        assert not got["pairs"].any() and not got["features"].any()


@pytest.mark.parametrize("name", cg.FPFH_IDS)
def test_fpfh_buffers_under_both_poisons(name):
    _same_bits(_fpfh_device(name, POISON_NAN), _fpfh_device(name, POISON_FINITE), FPFH_KEYS)


@pytest.mark.parametrize("name", ["s300", "s2049", "crowded", "hand"])
def test_fpfh_of_permuted_rows_is_the_permuted_output(name):
    c = cg.fpfh_case(name)
    perm = np.random.default_rng(261).permutation(len(c["points"]))
    moved = _fpfh_entry(c["points"][perm], c["normals"][perm], c["h"])
    _same_bits(moved, cg.fpfh_reference(c["points"][perm], c["normals"][perm], c["h"]), FPFH_KEYS)
    base = _fpfh_device(name)
    if name == "hand":
        # the hand case has pairs whose two angles tie exactly (lattice points on a common axis, both products 0): the tie
        # goes to the lower row, which a permutation changes.  The counts of pairs do not depend on it.
        _same_bits(moved, {k: base[k][perm] for k in FPFH_KEYS}, ("pairs",))
        return
    _same_bits(moved, {k: base[k][perm] for k in FPFH_KEYS}, FPFH_KEYS)


def test_fpfh_min_neighbours_and_twice():
    c = cg.fpfh_case("s300")
    base = _fpfh_device("s300")
    _same_bits(base, _fpfh_entry(c["points"], c["normals"], c["h"]), FPFH_KEYS)
    k = int(np.median(base["pairs"]))
    got = _fpfh_entry(c["points"], c["normals"], c["h"], min_neighbours=k)
    _same_bits(got, cg.fpfh_reference(c["points"], c["normals"], c["h"], k), FPFH_KEYS)
    zero = ~got["features"].any(axis=1)
    assert (zero == (base["pairs"] < k)).all() and zero.any() and not zero.all()


# ---- matching -----------------------------------------------------------------------------------------------------------
MATCH_KEYS = ("index", "dist2", "second_dist2", "mutual")


def _match_entry(query, target, fill=POISON_NAN):
    nq, nt = len(query), len(target)
    guard = Guard(_alloc, fill)
    q, t = guard.poisoned(_to(query)), guard.poisoned(_to(target))
    lib = _native.load()
    index, back = guard.empty((nq,), torch.int64, DEV), guard.empty((nt,), torch.int64, DEV)
    d2, second = guard.empty((nq,), torch.float32, DEV), guard.empty((nq,), torch.float32, DEV)
    bd2, bsecond = guard.empty((nt,), torch.float32, DEV), guard.empty((nt,), torch.float32, DEV)
    mutual = guard.empty((nq,), torch.uint8, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_cloud_feature_nearest(_native.ptr(q), nq, _native.ptr(t), nt, 33, _native.ptr(index),
                                                     _native.ptr(d2), _native.ptr(second), st), "mvsn_cloud_feature_nearest")
        _native.check(lib.mvsn_cloud_feature_nearest(_native.ptr(t), nt, _native.ptr(q), nq, 33, _native.ptr(back),
                                                     _native.ptr(bd2), _native.ptr(bsecond), st), "mvsn_cloud_feature_nearest")
        _native.check(lib.mvsn_cloud_feature_mutual(_native.ptr(index), nq, _native.ptr(back), nt, _native.ptr(mutual), st),
                      "mvsn_cloud_feature_mutual")
    torch.cuda.synchronize()
    guard.check()
    return {"index": index.cpu().numpy(), "dist2": d2.cpu().numpy(), "second_dist2": second.cpu().numpy(),
            "mutual": mutual.cpu().numpy().astype(bool), "back": back.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def _match_device(name, fill=POISON_NAN):
    c = cg.match_case(name)
    return _match_entry(c["query"], c["target"], fill)


@pytest.mark.parametrize("name", cg.MATCH_IDS)
def test_matches_equal_the_restatement_bit_for_bit(name):
    c = cg.match_case(name)
    got, ref = _match_device(name), cg.feature_nearest_reference(c["query"], c["target"], mutual=True)
    _same_bits(got, ref, MATCH_KEYS)
    _same_bits(got, _match_device(name, POISON_FINITE), MATCH_KEYS + ("back",))
    if name == "ties":
        assert (got["index"][:20] == 3).all() and (got["index"][20:40] == 258).all() and not got["dist2"][:40].any()
        assert not got["second_dist2"][:40].any()                           # the runner-up is another copy
    if name == "none":
        assert (got["index"] == -1).all() and np.isposinf(got["dist2"]).all() and not got["mutual"].any()
    if name == "absent":
        assert (got["index"][[5, 255, 256, 7, 8]] == -1).all() and not np.isin(got["index"], [0, 255, 256, 519, 300, 301]).any()


def test_the_python_matcher_is_the_library_call():
    c = cg.match_case("absent")
    for want in (False, True):
        r = feature_nearest(_to(c["query"]), _to(c["target"]), mutual=want)
        assert r.index.dtype == torch.int64 and r.dist2.dtype == r.second_dist2.dtype == torch.float32 and r.index.is_cuda
        got = {"index": r.index.cpu().numpy(), "dist2": r.dist2.cpu().numpy(), "second_dist2": r.second_dist2.cpu().numpy()}
        _same_bits(got, _match_device("absent"), MATCH_KEYS[:3])
        if want:
            assert r.mutual.dtype == torch.bool and (r.mutual.cpu().numpy() == _match_device("absent")["mutual"]).all()
        else:
            assert r.mutual is None


# ---- RANSAC -------------------------------------------------------------------------------------------------------------
RANSAC_KEYS = ("best", "T64", "T", "inlier")


def _ransac_entry(c, fill=POISON_NAN):
    ns, nt, nc = len(c["source"]), len(c["target"]), len(c["corr"])
    _, _, r2 = radius_scalars(c["max_dist"])
    guard = Guard(_alloc, fill)
    s, t, corr = guard.poisoned(_to(c["source"])), guard.poisoned(_to(c["target"])), guard.poisoned(_to(c["corr"]))
    lib = _native.load()
    ws_bytes = lib.mvsn_cloud_ransac_workspace_bytes()
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    T, T64 = guard.empty((4, 4), torch.float32, DEV), guard.empty((4, 4), torch.float64, DEV)
    best, inlier = guard.empty((3,), torch.int64, DEV), guard.empty((nc,), torch.uint8, DEV)
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_cloud_ransac(_native.ptr(s), ns, _native.ptr(t), nt, _native.ptr(corr), nc, float(r2),
                                            float(c["edge_similarity"]), int(c["hypotheses"]), int(c["seed"]), _native.ptr(ws),
                                            ws_bytes, _native.ptr(T), _native.ptr(T64), _native.ptr(best), _native.ptr(inlier),
                                            _native.stream()), "mvsn_cloud_ransac")
    torch.cuda.synchronize()
    guard.check()
    return {"best": best.cpu().numpy(), "T64": T64.cpu().numpy(), "T": T.cpu().numpy(), "inlier": inlier.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def _ransac_device(name, fill=POISON_NAN):
    return _ransac_entry(cg.ransac_case(name), fill)


@pytest.mark.parametrize("name", cg.RANSAC_IDS)
def test_ransac_equals_the_restatement_bit_for_bit(name):
    got, ref = _ransac_device(name), cg.ransac_case_reference(name)
    print(f"{name}: device best {got['best'].tolist()}, restatement {ref['best'].tolist()}")
    _same_bits(got, ref, ("best", "inlier"))
    _same_bits(got, ref, ("T64", "T"))
    _same_bits(got, _ransac_device(name, POISON_FINITE), RANSAC_KEYS)
    _same_bits(got, _ransac_entry(cg.ransac_case(name)), RANSAC_KEYS)          # twice: the same bytes
    status = {"rejected": 2, "two": 1, "unusable": 1}.get(name, None)
    if status is not None:
        assert got["best"].tolist() == [-1, 0, status] and (got["T64"] == np.eye(4)).all() and not got["inlier"].any()
    if name == "exact_edge_1":
        assert got["best"][2] == 0 and np.abs(got["T64"] - cg.ransac_case(name)["T_true"]).max() < 1e-12
    if name.startswith("scene"):
        assert got["best"][2] == 0 and int(got["inlier"].sum()) == got["best"][1]


# ---- end to end ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _truth_start():
    """cloud_register started from the true motion, in the restatement of section 20: (translation, rotation) error."""
    sc, f = cg.scene(), cg.scene_features()
    ref = cr.register_reference(sc["source"], sc["target"], cg.SCENE_MAX_DIST, T_init=sc["T_true"].astype(np.float32),
                                normals=f["target_normals"], centre=cr.default_centre(sc["target"]),
                                iterations=cg.SCENE_REFINE_ITERATIONS)
    return cr.pose_error(ref["T"], sc["T_true"])


@pytest.mark.parametrize("seed", cg.SCENE_SEEDS)
def test_register_global_on_the_scene(seed):
    sc = cg.scene()
    src, tgt = _to(sc["source"]), _to(sc["target"])
    args = dict(hypotheses=cg.SCENE_HYPOTHESES, seed=seed, edge_similarity=cg.SCENE_EDGE_SIMILARITY)
    res = cloud_register_global(src, tgt, cg.SCENE_MAX_DIST, feature_radius=cg.SCENE_FEATURE_RADIUS,
                                refine_iterations=cg.SCENE_REFINE_ITERATIONS, **args)
    coarse_rms = cg.rms_to_truth(res.coarse.T.cpu().numpy())
    print(f"seed {seed}: {len(res.correspondences)} correspondences, winner {int(res.coarse.hypothesis)} with "
          f"{int(res.coarse.inliers)} inliers, coarse RMS {coarse_rms:.4g} (max_dist {cg.SCENE_MAX_DIST})")
    assert int(res.coarse.status) == 0 and coarse_rms < cg.SCENE_MAX_DIST
    # the stages are the restatement's: the same correspondences, the same winner
    f, ref = cg.scene_features(), cg.scene_ransac(seed)
    assert np.array_equal(res.correspondences.cpu().numpy(), f["correspondences"])
    assert [int(res.coarse.hypothesis), int(res.coarse.inliers), int(res.coarse.status)] == ref["best"].tolist()
    assert res.coarse.T.cpu().numpy().tobytes() == ref["T"].tobytes()
    # coarse is cloud_ransac by hand, refined is cloud_register by hand
    by_hand = cloud_ransac(src, tgt, res.correspondences, cg.SCENE_MAX_DIST, **args)
    for a, b in zip(res.coarse, by_hand):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    tn = cloud_normals(tgt, float(np.float32(cg.SCENE_FEATURE_RADIUS)) / 2).normals
    icp = cloud_register(src, tgt, cg.SCENE_MAX_DIST, target_normals=tn, T_init=res.coarse.T,
                         iterations=cg.SCENE_REFINE_ITERATIONS)
    for a, b in zip(res.refined, icp):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert res.T.cpu().numpy().tobytes() == icp.T.cpu().numpy().tobytes()
    # no worse than twice the errors of ICP started from the true motion
    t_true, r_true = _truth_start()
    t_err, r_err = cr.pose_error(res.T.cpu().numpy(), sc["T_true"])
    t_coarse, r_coarse = cr.pose_error(res.coarse.T.cpu().numpy(), sc["T_true"])
    print(f"seed {seed}: coarse {t_coarse:.4g} / {np.degrees(r_coarse):.4g} deg, refined {t_err:.4g} / {np.degrees(r_err):.4g} deg, "
          f"from the true motion {t_true:.4g} / {np.degrees(r_true):.4g} deg")
    assert t_err <= 2 * t_true and r_err <= 2 * r_true
    # the F-score at one grid spacing is that under the true motion
    T, Tt = res.T.to(torch.float64), _to(sc["T_true"])
    moved = (src.to(torch.float64) @ T[:3, :3].T + T[:3, 3]).to(torch.float32)
    truth = (src.to(torch.float64) @ Tt[:3, :3].T + Tt[:3, 3]).to(torch.float32)
    f_got = cloud_metrics(moved, tgt, cg.SCENE_SPACING)["fscore"]
    f_true = cloud_metrics(truth, tgt, cg.SCENE_SPACING)["fscore"]
    print(f"seed {seed}: F-score {f_got:.4f}, under the true motion {f_true:.4f}")
    assert abs(f_got - f_true) <= 0.01


def test_the_python_calls_are_the_library_calls():
    c = cg.fpfh_case("s300")
    r = cloud_fpfh(_to(c["points"]), _to(c["normals"]), c["h"])
    assert r.features.dtype == torch.float32 and r.spfh.dtype == r.pairs.dtype == torch.int32 and r.features.is_cuda
    _same_bits({"spfh": r.spfh.cpu().numpy(), "pairs": r.pairs.cpu().numpy(), "features": r.features.cpu().numpy()},
               _fpfh_device("s300"), FPFH_KEYS)
    k = cg.ransac_case("messy")
    got = cloud_ransac(_to(k["source"]), _to(k["target"]), _to(k["corr"]), k["max_dist"], hypotheses=k["hypotheses"], seed=k["seed"])
    dev = _ransac_device("messy")
    assert got.inlier.dtype == torch.bool and got.T.cpu().numpy().tobytes() == dev["T"].tobytes()
    assert [int(got.hypothesis), int(got.inliers), int(got.status)] == dev["best"].tolist()
    assert (got.inlier.cpu().numpy() == dev["inlier"].astype(bool)).all()
