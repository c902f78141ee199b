"""cloud_fpfh, feature_nearest, cloud_ransac and cloud_register_global without a GPU: host-side validation (everything is
rejected before any launch), empty clouds, CPU tensors, and the library's entries in the header, the binding and the
binary."""
import ctypes
import os
import re

import pytest
import torch

from multi_view_stereonet_amd import _native, build, fusion
from multi_view_stereonet_amd.fusion import (CloudFeatures, CloudRansac, FeatureMatches, GlobalRegistration, cloud_fpfh,
                                             cloud_ransac, cloud_register_global, feature_nearest)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mvsn_cloud_fpfh": 13, "mvsn_cloud_feature_nearest": 9, "mvsn_cloud_feature_mutual": 6,
           "mvsn_cloud_ransac_workspace_bytes": 0, "mvsn_cloud_ransac": 17}
N, M, C = 5, 7, 4
BAD, TOOLARGE, WORKSPACE = -1, -2, -3


def fpfh(**kw):
    a = dict(points=torch.zeros(N, 3), normals=torch.zeros(N, 3), radius=0.5)
    a.update(kw)
    return cloud_fpfh(a.pop("points"), a.pop("normals"), a.pop("radius"), **a)


def match(**kw):
    a = dict(q=torch.zeros(N, 33), t=torch.zeros(M, 33))
    a.update(kw)
    return feature_nearest(a.pop("q"), a.pop("t"), **a)


def ransac(**kw):
    a = dict(source=torch.zeros(N, 3), target=torch.zeros(M, 3), corr=torch.zeros(C, 2, dtype=torch.int64), max_dist=0.5)
    a.update(kw)
    return cloud_ransac(a.pop("source"), a.pop("target"), a.pop("corr"), a.pop("max_dist"), **a)


def glob(**kw):
    a = dict(source=torch.zeros(N, 3), target=torch.zeros(M, 3), max_dist=0.5, feature_radius=0.25)
    a.update(kw)
    return cloud_register_global(a.pop("source"), a.pop("target"), a.pop("max_dist"), **a)


def _bad_radius(name):
    return [(dict([(name, v)]), name) for v in (0.0, -1.0, float("nan"), float("inf"), 1e-30, "far", None)]


BAD_FPFH = _bad_radius("radius") + [
    (dict(points=None), "points must be"), (dict(points=torch.zeros(N, 4)), "points must be"),
    (dict(points=torch.zeros(N, 3, dtype=torch.float64)), "points must be float32"),
    (dict(normals=None), "normals must be"), (dict(normals=torch.zeros(N + 1, 3)), "normals must be"),
    (dict(normals=torch.zeros(N, 3, dtype=torch.float64)), "normals must be"),
    (dict(normals=torch.zeros(N, 3).to("meta")), "normals is on"),
    (dict(min_neighbours=0), "min_neighbours"), (dict(min_neighbours=2.5), "min_neighbours"), (dict(min_neighbours=True), "min_neighbours"),
    (dict(min_neighbours=None), "min_neighbours"), (dict(min_neighbours="3"), "min_neighbours"),
]
BAD_MATCH = [
    (dict(q=None), "query_features must be"), (dict(q=torch.zeros(N, 32)), "query_features must be"),
    (dict(q=torch.zeros(N, 33, dtype=torch.float64)), "query_features must be float32"),
    (dict(t=torch.zeros(33)), "target_features must be"), (dict(t=torch.zeros(M, 34)), "target_features must be"),
    (dict(t=torch.zeros(M, 33, dtype=torch.float16)), "target_features must be float32"),
    (dict(t=torch.zeros(M, 33).to("meta")), "query_features is on"),
]
BAD_RANSAC_COMMON = _bad_radius("max_dist") + [
    (dict(source=None), "source must be"), (dict(target=torch.zeros(M, 2)), "target must be"),
    (dict(source=torch.zeros(N, 3, dtype=torch.float64)), "source must be float32"),
    (dict(target=torch.zeros(M, 3).to("meta")), "target is on"),
    (dict(hypotheses=0), "hypotheses"), (dict(hypotheses=2 ** 24 + 1), "hypotheses"), (dict(hypotheses=10.5), "hypotheses"),
    (dict(hypotheses=None), "hypotheses"), (dict(hypotheses=True), "hypotheses"),
    (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(seed=0.5), "seed"), (dict(seed=None), "seed"),
    (dict(edge_similarity=0.0), "edge_similarity"), (dict(edge_similarity=1.01), "edge_similarity"),
    (dict(edge_similarity=float("nan")), "edge_similarity"), (dict(edge_similarity="0.9"), "edge_similarity"),
    (dict(edge_similarity=None), "edge_similarity"), (dict(edge_similarity=-0.5), "edge_similarity"),
]
BAD_RANSAC = BAD_RANSAC_COMMON + [
    (dict(corr=None), "correspondences must be"), (dict(corr=torch.zeros(C, 3, dtype=torch.int64)), "correspondences must be"),
    (dict(corr=torch.zeros(C, 2, dtype=torch.int32)), "correspondences must be"), (dict(corr=torch.zeros(C, 2)), "correspondences must be"),
    (dict(corr=torch.zeros(C, 2, dtype=torch.int64).to("meta")), "correspondences is on"),
]
BAD_GLOBAL = BAD_RANSAC_COMMON + _bad_radius("feature_radius") + [
    (dict(normal_radius=v), "normal_radius") for v in (0.0, -1.0, float("nan"), float("inf"), "far")] + [
    (dict(source_normals=torch.zeros(N + 1, 3)), "source_normals must be"), (dict(target_normals=torch.zeros(M, 2)), "target_normals must be"),
    (dict(source_normals=torch.zeros(N, 3, dtype=torch.float64)), "source_normals must be"),
    (dict(target_normals=torch.zeros(M, 3).to("meta")), "target_normals is on"),
    (dict(refine_iterations=-1), "refine_iterations"), (dict(refine_iterations=1001), "refine_iterations"),
    (dict(refine_iterations=2.5), "refine_iterations"),
]


@pytest.mark.parametrize("kw, text", BAD_FPFH)
def test_cloud_fpfh_validates_before_any_launch(kw, text):
    with pytest.raises(ValueError, match=text):
        fpfh(**kw)
    if "points" not in kw and "normals" not in kw:
        with pytest.raises(ValueError, match=text):              # (validated before the empty cloud's answer)
            fpfh(points=torch.zeros(0, 3), normals=torch.zeros(0, 3), **kw)


@pytest.mark.parametrize("kw, text", BAD_MATCH)
def test_feature_nearest_validates_before_any_launch(kw, text):
    with pytest.raises(ValueError, match=text):
        match(**kw)


@pytest.mark.parametrize("kw, text", BAD_RANSAC)
def test_cloud_ransac_validates_before_any_launch(kw, text):
    with pytest.raises(ValueError, match=text):
        ransac(**kw)
    if not {"source", "target", "corr"} & set(kw):
        with pytest.raises(ValueError, match=text):
            ransac(corr=torch.zeros(0, 2, dtype=torch.int64), **kw)


@pytest.mark.parametrize("kw, text", BAD_GLOBAL)
def test_cloud_register_global_validates_before_any_launch(kw, text):
    with pytest.raises(ValueError, match=text):
        glob(**kw)
    if not {"source", "target", "source_normals", "target_normals"} & set(kw):
        with pytest.raises(ValueError, match=text):
            glob(source=torch.zeros(0, 3), **kw)


def test_feature_radius_is_required_and_the_options_are_keywords():
    with pytest.raises(ValueError, match="feature_radius"):
        cloud_register_global(torch.zeros(N, 3), torch.zeros(M, 3), 0.5)
    with pytest.raises(TypeError):
        cloud_register_global(torch.zeros(N, 3), torch.zeros(M, 3), 0.5, 0.25)
    with pytest.raises(TypeError):
        cloud_fpfh(torch.zeros(N, 3), torch.zeros(N, 3), 0.5, 3)
    with pytest.raises(TypeError):
        feature_nearest(torch.zeros(N, 33), torch.zeros(M, 33), True)
    with pytest.raises(TypeError):
        cloud_ransac(torch.zeros(N, 3), torch.zeros(M, 3), torch.zeros(C, 2, dtype=torch.int64), 0.5, 1000)
    big = torch.zeros(1, 3).expand(2 ** 31, 3)
    with pytest.raises(ValueError, match=r"2\^31 - 1 points"):
        fpfh(points=big)
    with pytest.raises(ValueError, match=r"2\^31 - 1 source"):
        ransac(source=big)


def test_empty_inputs_are_answered_without_a_launch():
    r = fpfh(points=torch.zeros(0, 3), normals=torch.zeros(0, 3))
    assert isinstance(r, CloudFeatures) and r.features.shape == r.spfh.shape == (0, 33) and r.pairs.shape == (0,)
    assert r.features.dtype == torch.float32 and r.spfh.dtype == r.pairs.dtype == torch.int32
    for q, t in ((0, M), (N, 0), (0, 0)):
        for want in (False, True):
            m = match(q=torch.zeros(q, 33), t=torch.zeros(t, 33), mutual=want)
            assert isinstance(m, FeatureMatches) and m.index.shape == (q,) and (m.index == -1).all() and m.index.dtype == torch.int64
            assert torch.isposinf(m.dist2).all() and torch.isposinf(m.second_dist2).all() and m.dist2.dtype == torch.float32
            assert (m.mutual is None) if not want else (m.mutual.dtype == torch.bool and m.mutual.shape == (q,) and not m.mutual.any())
    for kw in (dict(corr=torch.zeros(0, 2, dtype=torch.int64)), dict(source=torch.zeros(0, 3)), dict(target=torch.zeros(0, 3))):
        r = ransac(**kw)
        c = 0 if "corr" in kw else C
        assert isinstance(r, CloudRansac) and torch.equal(r.T, torch.eye(4)) and r.T.dtype == torch.float32
        assert int(r.hypothesis) == -1 and int(r.inliers) == 0 and int(r.status) == 1
        assert r.inlier.shape == (c,) and r.inlier.dtype == torch.bool and not r.inlier.any()
    for kw in (dict(source=torch.zeros(0, 3)), dict(target=torch.zeros(0, 3))):
        g = glob(**kw)
        assert isinstance(g, GlobalRegistration) and torch.equal(g.T, torch.eye(4)) and int(g.coarse.status) == 1
        assert g.correspondences.shape == (0, 2) and g.correspondences.dtype == torch.int64 and int(g.refined.status) == 1
        g = glob(refine=False, **kw)
        assert g.refined is None and torch.equal(g.T, torch.eye(4))


def test_cpu_tensors_raise_the_usual_runtime_error():
    with pytest.raises(RuntimeError, match="cloud_fpfh runs on HIP devices only"):
        fpfh()
    with pytest.raises(RuntimeError, match="feature_nearest runs on HIP devices only"):
        match()
    with pytest.raises(RuntimeError, match="feature_nearest runs on HIP devices only"):
        match(mutual=True)
    with pytest.raises(RuntimeError, match="cloud_ransac runs on HIP devices only"):
        ransac()
    with pytest.raises(RuntimeError, match="cloud_register_global runs on HIP devices only"):
        glob()


def test_the_functions_say_what_they_do():
    assert fusion.CloudFeatures._fields == ("features", "spfh", "pairs")
    assert fusion.FeatureMatches._fields == ("index", "dist2", "second_dist2", "mutual")
    assert fusion.CloudRansac._fields == ("T", "hypothesis", "inliers", "status", "inlier")
    assert fusion.GlobalRegistration._fields == ("T", "coarse", "correspondences", "refined")
    for name in ("cloud_fpfh", "feature_nearest", "cloud_ransac", "cloud_register_global"):
        assert name in fusion.__doc__, name
    assert "bitwise-reproducible" in cloud_fpfh.__doc__ and "Rusu" in cloud_fpfh.__doc__
    assert "lowest" in feature_nearest.__doc__ and "ratio test" in feature_nearest.__doc__
    assert "splitmix64" in cloud_ransac.__doc__ and "edge_similarity" in cloud_ransac.__doc__
    assert "one extra host read" in cloud_register_global.__doc__ and "voxel_merge" in cloud_register_global.__doc__


def test_entries_in_header_binding_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    for src in ("mvsn_cloud_fpfh.hip", "mvsn_cloud_match.hip", "mvsn_cloud_ransac.hip"):
        assert build.SOURCES.count(src) == 1 and os.path.exists(os.path.join(build.CSRC, src))
        with open(os.path.join(build.CSRC, src)) as f:
            assert "#pragma clang fp contract(off)" in f.read()
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    lib = ctypes.CDLL(_native.library_path())
    assert _native.load().mvsn_abi_version() == 7
    for entry, count in ENTRIES.items():
        assert re.search(r"\b%s\(" % entry, header) and entry in _native.SIGNATURES
        decl = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % entry, header, re.M).group(1)
        args = [] if decl.strip() == "void" else decl.split(",")
        assert len(args) == len(_native.SIGNATURES[entry][1]) == count, entry
        assert hasattr(lib, entry)


def test_mvsn_cloud_fpfh_checks_its_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    need = lib.mvsn_cloud_workspace_bytes(N)
    ok = dict(points=one, normals=one, n=N, cell=0.5, inv=2.0, r2=0.25, k=3, ws=one, ws_bytes=need - 1, spfh=one, pairs=one,
              features=one)

    def fn(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.mvsn_cloud_fpfh(a["points"], a["normals"], a["n"], a["cell"], a["inv"], a["r2"], a["k"], a["ws"],
                                   a["ws_bytes"], a["spfh"], a["pairs"], a["features"], None)
    assert fn() == WORKSPACE and b"mvsn_cloud_fpfh" in lib.mvsn_last_error() and b"workspace" in lib.mvsn_last_error()
    for name in ("points", "normals", "spfh", "pairs", "features"):
        assert fn(**{name: None}) == BAD, name
    assert fn(n=0) == BAD and fn(n=-4) == BAD and fn(k=0) == BAD and fn(k=-2) == BAD and b"min_neighbours = -2" in lib.mvsn_last_error()
    for name in ("cell", "inv", "r2"):
        assert fn(**{name: 0.0}) == BAD and fn(**{name: float("nan")}) == BAD and fn(**{name: float("inf")}) == BAD, name
    assert fn(n=2 ** 31) == TOOLARGE and fn(ws=None) == WORKSPACE and fn(ws_bytes=0) == WORKSPACE
    assert fn(ws=ctypes.c_void_p(24), ws_bytes=need) == BAD and b"aligned" in lib.mvsn_last_error()
    assert fn(points=None, n=2 ** 31, ws=None) == BAD and fn(n=2 ** 31, ws=None) == TOOLARGE


def test_mvsn_cloud_feature_nearest_checks_its_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)

    def fn(q=one, nq=N, t=one, nt=M, dim=33, index=one, d2=one, second=one):
        return lib.mvsn_cloud_feature_nearest(q, nq, t, nt, dim, index, d2, second, None)
    for dim in (0, 32, 34, 64, -33):                             # (checked before anything is launched: nothing else passes)
        assert fn(dim=dim) == BAD and b"mvsn_cloud_feature_nearest" in lib.mvsn_last_error()
        assert b"dim = %d" % dim in lib.mvsn_last_error() and b"only 33" in lib.mvsn_last_error()
    for name in ("q", "t", "index", "d2", "second"):
        assert fn(**{name: None}) == BAD and b"null pointer" in lib.mvsn_last_error(), name
    assert fn(nq=0) == BAD and fn(nt=0) == BAD and fn(nq=-1) == BAD
    assert fn(nq=2 ** 31) == TOOLARGE and fn(nt=2 ** 31) == TOOLARGE and fn(nq=2 ** 31, dim=5) == BAD

    def mutual(index=one, nq=N, back=one, nt=M, out=one):
        return lib.mvsn_cloud_feature_mutual(index, nq, back, nt, out, None)
    assert mutual(index=None) == BAD and mutual(back=None) == BAD and mutual(out=None) == BAD
    assert mutual(nq=0) == BAD and mutual(nt=-1) == BAD and mutual(nq=2 ** 31) == TOOLARGE and mutual(nt=2 ** 31) == TOOLARGE


def test_mvsn_cloud_ransac_checks_its_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)
    need = lib.mvsn_cloud_ransac_workspace_bytes()
    assert need >= 8
    ok = dict(s=one, ns=N, t=one, nt=M, corr=one, c=C, r2=0.25, es=0.9, hyp=100, seed=0, ws=one, ws_bytes=need - 1, T=one,
              T64=one, best=one, inlier=one)

    def fn(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.mvsn_cloud_ransac(a["s"], a["ns"], a["t"], a["nt"], a["corr"], a["c"], a["r2"], a["es"], a["hyp"], a["seed"],
                                     a["ws"], a["ws_bytes"], a["T"], a["T64"], a["best"], a["inlier"], None)
    # (nothing passes: the workspace is one byte short throughout, or misaligned)
    assert fn() == WORKSPACE and b"mvsn_cloud_ransac" in lib.mvsn_last_error() and b"workspace" in lib.mvsn_last_error()
    assert fn(seed=2 ** 64 - 1) == WORKSPACE and fn(es=1.0) == WORKSPACE and fn(hyp=1) == WORKSPACE and fn(hyp=2 ** 24) == WORKSPACE
    for name in ("s", "t", "corr", "T", "T64", "best", "inlier"):
        assert fn(**{name: None}) == BAD and b"null pointer" in lib.mvsn_last_error(), name
    assert fn(ns=0) == BAD and fn(nt=0) == BAD and fn(c=0) == BAD and fn(c=-1) == BAD
    assert fn(r2=0.0) == BAD and fn(r2=float("nan")) == BAD and fn(r2=float("inf")) == BAD and fn(r2=-1.0) == BAD
    for es in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert fn(es=es) == BAD and b"edge_similarity" in lib.mvsn_last_error(), es
    assert fn(hyp=0) == BAD and fn(hyp=-7) == BAD and b"hypotheses = -7" in lib.mvsn_last_error()
    assert fn(hyp=2 ** 24 + 1) == TOOLARGE and b"hypotheses" in lib.mvsn_last_error()
    assert fn(ns=2 ** 31) == TOOLARGE and fn(nt=2 ** 31) == TOOLARGE and fn(c=2 ** 31) == TOOLARGE
    assert fn(ws=None) == WORKSPACE and fn(ws_bytes=0) == WORKSPACE
    assert fn(ws=ctypes.c_void_p(24), ws_bytes=need) == BAD and b"aligned" in lib.mvsn_last_error()
    assert fn(s=None, hyp=2 ** 25, ws=None) == BAD and fn(hyp=2 ** 25, ws=None) == TOOLARGE
