"""cloud_clusters and cloud_cluster_mask without a GPU: host-side validation (everything is rejected before any launch),
empty clouds, CPU tensors, the selection on CPU tensors against its restatement, and the library's entries in the header,
the binding and the binary."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cloud_cluster_reference as cc
from multi_view_stereonet_amd import _native, build, fusion
from multi_view_stereonet_amd.fusion import CloudClusters, cloud_cluster_mask, cloud_clusters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mvsn_cloud_cluster_workspace_bytes": 1, "mvsn_cloud_cluster_label": 13, "mvsn_cloud_cluster_emit": 15}
N = 5
MISSING = object()


def clusters(**kw):
    a = dict(points=torch.zeros(N, 3), eps=0.5, min_points=3)
    a.update(kw)
    args = [a[k] for k in ("points", "eps", "min_points") if a[k] is not MISSING]
    return cloud_clusters(*args)


BAD = [
    (dict(points=None), "points must be"), (dict(points=torch.zeros(N, 4)), "points must be"),
    (dict(points=torch.zeros(N)), "points must be"), (dict(points=torch.zeros(N, 3, 1)), "points must be"),
    (dict(points=torch.zeros(N, 3, dtype=torch.float64)), "points must be float32"),
    (dict(points=torch.zeros(N, 3, dtype=torch.int32)), "points must be float32"),
    (dict(eps=0.0), "eps"), (dict(eps=-1.0), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=float("inf")), "eps"),
    (dict(eps=1e-30), "eps"), (dict(eps=None), "eps"), (dict(eps="wide"), "eps"),
    (dict(min_points=0), "min_points must be"), (dict(min_points=-1), "min_points must be"),
    (dict(min_points=2.5), "min_points must be"), (dict(min_points=True), "min_points must be"),
    (dict(min_points="4"), "min_points must be"), (dict(min_points=None), "min_points must be"),
    (dict(min_points=2 ** 31), "min_points must be"),
]


@pytest.mark.parametrize("kw, match", BAD)
def test_cloud_clusters_validates_before_any_launch(kw, match):
    with pytest.raises(ValueError, match=match):
        clusters(**kw)
    if "points" not in kw:
        with pytest.raises(ValueError, match=match):              # (validated before the empty cloud's answer)
            clusters(points=torch.zeros(0, 3), **kw)


def test_sizes_are_limited_and_every_argument_is_required():
    with pytest.raises(ValueError, match=r"2\^31 - 1 points"):
        clusters(points=torch.zeros(1, 3).expand(2 ** 31, 3))
    with pytest.raises(TypeError):
        clusters(min_points=MISSING)
    with pytest.raises(TypeError):
        cloud_clusters(torch.zeros(N, 3))


@pytest.mark.parametrize("min_points", [1, 4, 2 ** 31 - 1])
def test_an_empty_cloud_is_answered_without_a_launch(min_points):
    r = clusters(points=torch.zeros(0, 3), min_points=min_points)
    assert isinstance(r, CloudClusters)
    want = dict(label=torch.int64, core=torch.bool, within=torch.int32, count=torch.int64, core_count=torch.int64,
                first=torch.int64)
    assert CloudClusters._fields == tuple(want) == cc.OUTPUTS
    for name, t in zip(CloudClusters._fields, r):
        assert t.shape == (0,) and t.dtype == want[name] and t.device.type == "cpu", name
    assert cloud_cluster_mask(r, min_size=1).shape == (0,)


def test_a_cpu_cloud_raises_the_usual_runtime_error():
    with pytest.raises(RuntimeError, match="cloud_clusters runs on HIP devices only"):
        clusters()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        clusters(points=torch.rand(1, 3), min_points=1)


def test_the_functions_sit_next_to_cloud_nearest_and_say_what_they_do():
    doc = cloud_clusters.__doc__
    for word in ("DBSCAN", "cluster_dbscan", "EuclideanClusterExtraction", "cloud_nearest", "border", "noise", "core",
                 "bitwise-reproducible", "symmetric bit for bit", "lowest row", "quadratic", "one host synchronisation"):
        assert word in doc, word
    doc = cloud_cluster_mask.__doc__
    assert "filter_mesh" in doc and "stable" in doc and "Noise is always False" in doc and "no host read" in doc
    assert "cloud_clusters" in fusion.__doc__ and "cloud_cluster_mask" in fusion.__doc__


# ---- cloud_cluster_mask --------------------------------------------------------------------------------------------------
def _tensors(ref):
    return CloudClusters(*(torch.from_numpy(np.array(ref[k])) for k in cc.OUTPUTS))


def _fixture():
    return _tensors(cc.case_reference("n257", 12))


def _bad_clusters():
    good = _fixture()
    n, c = good.label.shape[0], good.count.shape[0]
    yield None, "clusters must be"
    yield tuple(good)[:5], "clusters must be"
    yield list(good), "clusters must be"
    yield good._replace(label=good.label.to(torch.int32)), "clusters.label"
    yield good._replace(label=good.label[:-1]), "clusters.core"
    yield good._replace(label=good.label.reshape(-1, 1)), "clusters.label"
    yield good._replace(label=None), "clusters.label"
    yield good._replace(core=good.core.to(torch.uint8)), "clusters.core"
    yield good._replace(core=good.core[:-1]), "clusters.core"
    yield good._replace(within=good.within.to(torch.int64)), "clusters.within"
    yield good._replace(within=None), "clusters.within"
    yield good._replace(count=good.count.to(torch.int32)), "clusters.count"
    yield good._replace(count=good.count[:-1]), "clusters.core_count"
    yield good._replace(count=None), "clusters.count"
    yield good._replace(core_count=good.core_count[:-1]), "clusters.core_count"
    yield good._replace(first=good.first.to(torch.float32)), "clusters.first"
    yield good._replace(first=torch.zeros(c + 1, dtype=torch.int64)), "clusters.first"
    yield good._replace(label=good.label.to("meta")), "clusters.core is on"
    yield good._replace(first=good.first.to("meta")), "clusters.first is on"
    many = torch.zeros(n + 1, dtype=torch.int64)
    yield good._replace(count=many, core_count=many, first=many), f"holds {n + 1} clusters"


@pytest.mark.parametrize("bad, match", list(_bad_clusters()))
def test_a_malformed_clusters_is_a_value_error(bad, match):
    with pytest.raises(ValueError, match=match):
        cloud_cluster_mask(bad, min_size=1)


def test_the_rule_combinations():
    good = _fixture()
    c = good.count.shape[0]
    keep = torch.ones(c, dtype=torch.bool)
    with pytest.raises(ValueError, match="give one of min_size, keep_largest or keep"):
        cloud_cluster_mask(good)
    with pytest.raises(ValueError, match="keep replaces"):
        cloud_cluster_mask(good, keep=keep, min_size=1)
    with pytest.raises(ValueError, match="keep replaces"):
        cloud_cluster_mask(good, keep=keep, keep_largest=1)
    with pytest.raises(ValueError, match="keep replaces"):
        cloud_cluster_mask(good, keep=keep, min_size=1, keep_largest=1)
    with pytest.raises(TypeError):
        cloud_cluster_mask(good, 1)                                # the rules are keywords
    for bad in (-1, 2.5, True, "3", float("nan")):
        with pytest.raises(ValueError, match="min_size must be"):
            cloud_cluster_mask(good, min_size=bad)
        with pytest.raises(ValueError, match="keep_largest must be"):
            cloud_cluster_mask(good, keep_largest=bad)
    for bad in (keep[:-1], torch.ones(c + 1, dtype=torch.bool), keep.to(torch.uint8), keep.reshape(1, -1), [True] * c, 1,
                keep.to("meta")):
        with pytest.raises(ValueError, match="keep must be|keep is on"):
            cloud_cluster_mask(good, keep=bad)


@pytest.mark.parametrize("name, min_points", [("n257", 12), ("n257", 1), ("many_small", 3), ("scene", 10), ("n1", 2),
                                              ("bridge_border", 6)])
def test_the_mask_on_cpu_tensors_equals_its_restatement(name, min_points):
    ref = cc.case_reference(name, min_points)
    t = _tensors(ref)
    c = len(ref["first"])
    rng = np.random.default_rng(331)
    rules = [dict(min_size=0), dict(min_size=2), dict(min_size=4), dict(min_size=10 ** 9), dict(keep_largest=0),
             dict(keep_largest=1), dict(keep_largest=2), dict(keep_largest=c + 3), dict(min_size=3, keep_largest=2),
             dict(min_size=3, keep_largest=1000)]
    for rule in rules:
        got = cloud_cluster_mask(t, **rule)
        assert got.dtype == torch.bool and got.shape == (len(ref["label"]),)
        assert got.numpy().tobytes() == cc.cluster_mask_reference(ref, **rule).tobytes(), rule
        assert not got[t.label < 0].any()
    for keep in (np.zeros(c, bool), np.ones(c, bool), rng.integers(0, 2, c).astype(bool)):
        got = cloud_cluster_mask(t, keep=torch.from_numpy(keep))
        assert got.numpy().tobytes() == cc.cluster_mask_reference(ref, keep=keep).tobytes()
    assert cloud_cluster_mask(t, min_size=0).numpy().tolist() == (ref["label"] >= 0).tolist()


def test_keep_largest_ties_go_to_the_lower_id():
    ref = cc.case_reference("many_small", 3)                       # 700 clusters of 3
    got = cloud_cluster_mask(_tensors(ref), keep_largest=5).numpy()
    assert got.sum() == 15 and set(ref["label"][got].tolist()) == {0, 1, 2, 3, 4}


# ---- the library's entries ---------------------------------------------------------------------------------------------
def test_entries_in_header_binding_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_cloud_cluster.hip") == 1 and build.SOURCES.count("mvsn_mesh.hip") == 1
    assert build.HEADERS.count("mvsn_unionfind.h") == 1 and build.HEADERS.count("mvsn_cloud.h") == 1
    for name in build.SOURCES + build.HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    assert re.search(r"#define\s+MVSN_CLUSTER_STATUS_WORKSPACE\s+1\b", header) and fusion.CLUSTER_STATUS_WORKSPACE == 1
    lib = ctypes.CDLL(_native.library_path())
    for entry, count in ENTRIES.items():
        assert re.search(r"\b%s\(" % entry, header) and entry in _native.SIGNATURES
        decl = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % entry, header, re.M).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[entry][1]) == count, entry
        assert hasattr(lib, entry)


def test_the_union_find_lives_in_one_place():
    with open(os.path.join(build.CSRC, "mvsn_unionfind.h")) as f:
        shared = f.read()
    for name in ("mesh_load", "mesh_store", "mesh_find", "mesh_unite"):
        assert len(re.findall(r"__device__ __forceinline__ \w+ %s\(" % name, shared)) == 1, name
        for source in ("mvsn_mesh.hip", "mvsn_cloud_cluster.hip"):
            with open(os.path.join(build.CSRC, source)) as f:
                text = f.read()
            assert '#include "mvsn_unionfind.h"' in text and not re.search(r"__device__[^;{]*\b%s\(" % name, text), (source, name)


def test_the_entries_check_their_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    size = lib.mvsn_cloud_cluster_workspace_bytes
    assert size(0) == 0 and size(-1) == 0 and size(2 ** 31) == 0
    assert 0 < size(1) == size(64) < size(257) < size(2 ** 20) and size(1) % 256 == 0 and size(2 ** 31 - 1) > 8 * (2 ** 31 - 1)
    need, index_need = size(N), lib.mvsn_cloud_workspace_bytes(N)
    ok = dict(points=one, n=N, inv=2.0, r2=0.25, min_points=3, index=one, index_bytes=index_need, within=one, core=one,
              result=one, ws=one, ws_bytes=need - 1, c=0, label=one, count=one, core_count=one, first=one)

    def label(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.mvsn_cloud_cluster_label(a["points"], a["n"], a["inv"], a["r2"], a["min_points"], a["index"],
                                            a["index_bytes"], a["within"], a["core"], a["result"], a["ws"], a["ws_bytes"], None)

    def emit(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.mvsn_cloud_cluster_emit(a["points"], a["n"], a["inv"], a["r2"], a["index"], a["index_bytes"], a["core"],
                                           a["ws"], a["ws_bytes"], a["c"], a["label"], a["count"], a["core_count"], a["first"],
                                           None)
    # (nothing passes: the workspace is one byte short throughout, or misaligned)
    for fn, who in ((label, b"mvsn_cloud_cluster_label"), (emit, b"mvsn_cloud_cluster_emit")):
        assert fn() == -3 and who in lib.mvsn_last_error() and b"workspace" in lib.mvsn_last_error()
        assert fn(points=None) == -1 and fn(core=None) == -1 and who in lib.mvsn_last_error()
        assert fn(n=0) == -1 and fn(n=-5) == -1 and fn(n=2 ** 31) == -2
        for name in ("inv", "r2"):
            assert fn(**{name: 0.0}) == -1 and fn(**{name: float("nan")}) == -1 and fn(**{name: float("inf")}) == -1, name
        assert fn(index=None) == -3 and fn(index_bytes=index_need - 1) == -3 and fn(ws=None) == -3 and fn(ws_bytes=0) == -3
        assert fn(ws=ctypes.c_void_p(24), ws_bytes=need) == -1    # not 16-byte aligned
        assert fn(index=ctypes.c_void_p(24), ws_bytes=need) == -1
        # the codes in their order: a null pointer before the size, the size before the workspace
        assert fn(points=None, n=2 ** 31, ws=None) == -1 and fn(n=2 ** 31, ws=None) == -2
    assert label(within=None) == -1 and label(result=None) == -1
    assert label(min_points=0) == -1 and label(min_points=-2) == -1 and b"min_points = -2" in lib.mvsn_last_error()
    assert label(min_points=1) == -3 and label(min_points=2 ** 40) == -3
    assert emit(label=None) == -1
    # count, core_count and first may be null with no cluster, and only then
    assert emit(count=None, core_count=None, first=None) == -3
    for name in ("count", "core_count", "first"):
        assert emit(c=1, **{name: None}) == -1 and emit(c=1) == -3, name
    assert emit(c=-1) == -1 and emit(c=N + 1) == -1 and b"6 clusters of 5 points" in lib.mvsn_last_error() and emit(c=N) == -3
