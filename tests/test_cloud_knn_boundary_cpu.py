"""cloud_knn and statistical_outlier_mask without a GPU: host-side validation (everything is rejected before any launch),
empty clouds, CPU tensors, and the library's entries in the header, the binding and the binary."""
import ctypes
import os
import re

import pytest
import torch

from multi_view_stereonet_amd import _native, build, fusion
from multi_view_stereonet_amd.fusion import CloudKNN, CloudOutliers, cloud_knn, statistical_outlier_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mvsn_cloud_knn": 15, "mvsn_cloud_mean_stats_workspace_bytes": 1, "mvsn_cloud_mean_stats": 6}
N, M = 5, 7
MISSING = object()


def knn(**kw):
    a = dict(query=torch.zeros(N, 3), target=torch.zeros(M, 3), k=3, max_dist=0.5)
    a.update(kw)
    args = [a.pop("query"), a.pop("target"), a.pop("k")]
    h = a.pop("max_dist")
    return cloud_knn(*args, **a) if h is MISSING else cloud_knn(*args, h, **a)


def sor(**kw):
    a = dict(points=torch.zeros(N, 3), k=3, std_ratio=2.0, max_dist=0.5)
    a.update(kw)
    args = [a.pop("points"), a.pop("k"), a.pop("std_ratio")]
    h = a.pop("max_dist")
    assert not a
    return statistical_outlier_mask(*args) if h is MISSING else statistical_outlier_mask(*args, h)


BAD_K = [(dict(k=0), "k must be"), (dict(k=65), "k must be"), (dict(k=2.5), "k must be"), (dict(k=True), "k must be"),
         (dict(k=None), "k must be"), (dict(k=-1), "k must be"), (dict(k="8"), "k must be")]
BAD_RADIUS = [(dict(max_dist=0.0), "max_dist"), (dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
              (dict(max_dist=float("inf")), "max_dist"), (dict(max_dist=1e-30), "max_dist"), (dict(max_dist="far"), "max_dist"),
              (dict(max_dist=None), "max_dist"), (dict(max_dist=MISSING), "max_dist")]
BAD_KNN = BAD_K + BAD_RADIUS + [
    (dict(query=None), "query must be"), (dict(query=torch.zeros(N, 4)), "query must be"), (dict(query=torch.zeros(N)), "query must be"),
    (dict(query=torch.zeros(N, 3, dtype=torch.float64)), "query must be float32"),
    (dict(target=torch.zeros(3)), "target must be"), (dict(target=torch.zeros(M, 3, dtype=torch.float16)), "target must be float32"),
    (dict(target=torch.ones(M, 3).to("meta")), "query is on"), (dict(query=torch.ones(N, 3).to("meta")), "query is on"),
    (dict(exclude_self=True), "exclude_self"), (dict(exclude_self=True, target=torch.zeros(N + 1, 3)), "exclude_self"),
]
BAD_SOR = BAD_K + BAD_RADIUS + [
    (dict(points=None), "points must be"), (dict(points=torch.zeros(N, 2)), "points must be"),
    (dict(points=torch.zeros(N, 3, dtype=torch.float64)), "points must be float32"),
    (dict(std_ratio=-0.5), "std_ratio"), (dict(std_ratio=float("nan")), "std_ratio"), (dict(std_ratio=float("inf")), "std_ratio"),
    (dict(std_ratio="wide"), "std_ratio"), (dict(std_ratio=None), "std_ratio"), (dict(std_ratio="2"), "std_ratio"),
    (dict(std_ratio=[1.0, 2.0]), "std_ratio"),
]


@pytest.mark.parametrize("kw, match", BAD_KNN)
def test_cloud_knn_validates_before_any_launch(kw, match):
    with pytest.raises(ValueError, match=match):
        knn(**kw)
    if "query" not in kw and "target" not in kw and "exclude_self" not in kw:
        with pytest.raises(ValueError, match=match):              # (validated before the empty cloud's answer)
            knn(query=torch.zeros(0, 3), **kw)
        with pytest.raises(ValueError, match=match):
            knn(target=torch.zeros(0, 3), **kw)


@pytest.mark.parametrize("kw, match", BAD_SOR)
def test_statistical_outlier_mask_validates_before_any_launch(kw, match):
    with pytest.raises(ValueError, match=match):
        sor(**kw)
    if "points" not in kw:
        with pytest.raises(ValueError, match=match):
            sor(points=torch.zeros(0, 3), **kw)


def test_sizes_are_limited_and_exclude_self_is_a_keyword():
    big = torch.zeros(1, 3).expand(2 ** 31, 3)
    with pytest.raises(ValueError, match=r"2\^31 - 1 query"):
        knn(query=big)
    with pytest.raises(ValueError, match=r"2\^31 - 1 target"):
        knn(target=big)
    with pytest.raises(ValueError, match=r"2\^31 - 1 points"):
        sor(points=big)
    with pytest.raises(ValueError, match="exclude_self"):         # an empty query against a cloud is not the same cloud
        knn(query=torch.zeros(0, 3), exclude_self=True)
    with pytest.raises(TypeError):
        cloud_knn(torch.zeros(N, 3), torch.zeros(N, 3), 3, 0.5, True)


@pytest.mark.parametrize("n, m", [(0, M), (N, 0), (0, 0)])
@pytest.mark.parametrize("k", [1, 8, 64])
def test_empty_clouds_are_answered_without_a_launch(n, m, k):
    for ex in (False, True)[:2 if n == m else 1]:
        r = knn(query=torch.zeros(n, 3), target=torch.ones(m, 3), k=k, exclude_self=ex)
        assert isinstance(r, CloudKNN)
        assert r.dist2.shape == (n, k) and r.dist2.dtype == torch.float32 and torch.isposinf(r.dist2).all()
        assert r.index.shape == (n, k) and r.index.dtype == torch.int64 and (r.index == -1).all()
        assert r.within.shape == (n,) and r.within.dtype == torch.int32 and not r.within.any()
    o = sor(points=torch.zeros(0, 3), k=k)
    assert isinstance(o, CloudOutliers)
    assert o.keep.shape == (0,) and o.keep.dtype == torch.bool and o.mean_dist.shape == (0,) and o.mean_dist.dtype == torch.float64
    assert o.mean.shape == o.std.shape == () and o.mean.dtype == o.std.dtype == torch.float64
    assert torch.isnan(o.mean) and float(o.std) == 0.0            # the statistics of no point at all


def test_cpu_tensors_raise_the_usual_runtime_error():
    with pytest.raises(RuntimeError, match="cloud_knn runs on HIP devices only"):
        knn()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        knn(target=torch.zeros(N, 3), k=64, exclude_self=True)
    with pytest.raises(RuntimeError, match="statistical_outlier_mask runs on HIP devices only"):
        sor()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        sor(std_ratio=0, k=64)


def test_the_functions_sit_next_to_cloud_nearest_and_say_what_they_do():
    doc = cloud_knn.__doc__
    assert "bitwise-reproducible" in doc and "stable sort" in doc and "cloud_nearest" in doc and "bit for bit" in doc
    assert "quadratic" in doc and "exclude_self" in doc
    doc = statistical_outlier_mask.__doc__
    assert "StatisticalOutlierRemoval" in doc and "remove_statistical_outlier" in doc and "radius_outlier_mask" in doc and "NaN" in doc
    assert fusion.CloudKNN._fields == ("dist2", "index", "within")
    assert fusion.CloudOutliers._fields == ("keep", "mean_dist", "mean", "std")
    assert "cloud_knn" in fusion.__doc__ and "statistical_outlier_mask" in fusion.__doc__


def test_entries_in_header_binding_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_cloud_knn.hip") == 1 and build.HEADERS.count("mvsn_cloud.h") == 1
    for name in build.SOURCES + build.HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    lib = ctypes.CDLL(_native.library_path())
    for entry, count in ENTRIES.items():
        assert re.search(r"\b%s\(" % entry, header) and entry in _native.SIGNATURES
        decl = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % entry, header, re.M).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[entry][1]) == count, entry
        assert hasattr(lib, entry)


def test_mvsn_cloud_knn_checks_its_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    need = lib.mvsn_cloud_workspace_bytes(M)
    ok = dict(query=one, nq=N, k=8, exclude_self=0, cell=0.5, inv=2.0, r2=0.25, ws=one, ws_bytes=need - 1, m=M, dist2=one,
              index=one, within=one, mean=one)

    def fn(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.mvsn_cloud_knn(a["query"], a["nq"], a["k"], a["exclude_self"], a["cell"], a["inv"], a["r2"], a["ws"],
                                  a["ws_bytes"], a["m"], a["dist2"], a["index"], a["within"], a["mean"], None)
    # (nothing passes: the workspace is one byte short throughout, or misaligned)
    assert fn() == -3 and b"mvsn_cloud_knn" in lib.mvsn_last_error() and b"workspace" in lib.mvsn_last_error()
    assert fn(mean=None) == -3 and fn(exclude_self=1) == -3 and fn(k=1) == -3 and fn(k=64) == -3   # the mean is optional
    for name in ("query", "dist2", "index", "within"):
        assert fn(**{name: None}) == -1, name
    assert b"mvsn_cloud_knn" in lib.mvsn_last_error()
    assert fn(k=0) == -1 and fn(k=65) == -1 and fn(k=-3) == -1 and b"k = -3" in lib.mvsn_last_error()
    assert fn(nq=0) == -1 and fn(m=0) == -1 and fn(nq=-5) == -1
    for name in ("cell", "inv", "r2"):
        assert fn(**{name: 0.0}) == -1 and fn(**{name: float("nan")}) == -1 and fn(**{name: float("inf")}) == -1, name
    assert fn(nq=2 ** 31) == -2 and fn(m=2 ** 31) == -2 and b"mvsn_cloud_knn" in lib.mvsn_last_error()
    assert fn(ws=None) == -3 and fn(ws_bytes=0) == -3
    assert fn(ws=ctypes.c_void_p(24), ws_bytes=need) == -1        # not 16-byte aligned
    # the codes in their order: a null pointer before the size, the size before the workspace
    assert fn(query=None, nq=2 ** 31, ws=None) == -1 and fn(nq=2 ** 31, ws=None) == -2


def test_mvsn_cloud_mean_stats_checks_its_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)
    size = lib.mvsn_cloud_mean_stats_workspace_bytes
    assert size(0) == 0 and size(-1) == 0 and size(2 ** 31) == 0
    assert 0 < size(1) == size(1024) <= size(1025) < size(2 ** 20) == size(2 ** 31 - 1)    # at most 1024 records
    need = size(N)

    def fn(mean=one, n=N, ws=one, ws_bytes=need - 1, stats=one):
        return lib.mvsn_cloud_mean_stats(mean, n, ws, ws_bytes, stats, None)
    assert fn() == -3 and b"mvsn_cloud_mean_stats" in lib.mvsn_last_error() and b"workspace" in lib.mvsn_last_error()
    assert fn(mean=None) == -1 and fn(stats=None) == -1 and fn(n=0) == -1 and fn(n=-2) == -1
    assert fn(n=2 ** 31) == -2 and fn(ws=None) == -3 and fn(ws_bytes=0) == -3
    assert fn(ws=ctypes.c_void_p(24), ws_bytes=need) == -1
    assert fn(mean=None, n=2 ** 31, ws=None) == -1 and fn(n=2 ** 31, ws=None) == -2
