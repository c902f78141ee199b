"""cloud_normals without a GPU: host-side validation (everything is rejected before any launch), empty clouds, CPU
tensors, and the library's entry in the header, the binding and the binary."""
import ctypes
import os
import re

import pytest
import torch

from multi_view_stereonet_amd import _native, build, fusion
from multi_view_stereonet_amd.fusion import CloudNormals, cloud_normals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mvsn_cloud_normals"
N, M = 5, 7


def call(**kw):
    a = dict(points=torch.zeros(N, 3), radius=0.5)
    a.update(kw)
    return cloud_normals(a.pop("points"), a.pop("radius"), **a)


BAD = [
    (dict(points=None), "points must be"), (dict(points=torch.zeros(N, 4)), "points must be"),
    (dict(points=torch.zeros(N, 3, dtype=torch.float64)), "points must be float32"),
    (dict(support=torch.zeros(3)), "support must be"), (dict(support=torch.zeros(M, 3, dtype=torch.float16)), "support must be float32"),
    (dict(support=torch.ones(M, 3).to("meta")), "support is on"),
    (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=float("nan")), "radius"),
    (dict(radius=float("inf")), "radius"), (dict(radius=1e-30), "radius"), (dict(radius="far"), "radius"),
    (dict(min_neighbours=2), "min_neighbours"), (dict(min_neighbours=0), "min_neighbours"), (dict(min_neighbours=3.5), "min_neighbours"),
    (dict(min_neighbours=None), "min_neighbours"), (dict(min_neighbours=True), "min_neighbours"),
    (dict(min_gap=-1e-9), "min_gap"), (dict(min_gap=1.0), "min_gap"), (dict(min_gap=float("nan")), "min_gap"),
    (dict(min_gap="small"), "min_gap"), (dict(min_gap=None), "min_gap"),
    (dict(viewpoint=(0.0, 1.0)), "viewpoint"), (dict(viewpoint="above"), "viewpoint"), (dict(viewpoint=torch.zeros(4)), "viewpoint"),
    (dict(viewpoint=torch.zeros(N + 1, 3)), "viewpoint"), (dict(viewpoint=torch.zeros(N, 3, dtype=torch.float64)), "viewpoint"),
    (dict(viewpoint=torch.zeros(N, 3).to("meta")), "viewpoint is on"), (dict(viewpoint=torch.zeros(3).to("meta")), "viewpoint"),
    (dict(viewpoint=torch.zeros(3, dtype=torch.bool)), "viewpoint"), (dict(viewpoint=torch.zeros(N, 3, 1)), "viewpoint"),
]


@pytest.mark.parametrize("kw, match", BAD)
def test_arguments_are_validated_before_any_launch(kw, match):
    with pytest.raises(ValueError, match=match):
        call(**kw)
    if "points" not in kw and "support" not in kw and not torch.is_tensor(kw.get("viewpoint")):
        with pytest.raises(ValueError, match=match):              # (validated before the empty cloud's answer)
            call(points=torch.zeros(0, 3), **kw)
        with pytest.raises(ValueError, match=match):
            call(support=torch.zeros(0, 3), **kw)


def test_devices_must_agree_sizes_are_limited_and_the_options_are_keywords():
    with pytest.raises(ValueError, match="support is on"):
        call(points=torch.zeros(N, 3).to("meta"), support=torch.zeros(M, 3))
    big = torch.zeros(1, 3).expand(2 ** 31, 3)
    with pytest.raises(ValueError, match=r"2\^31 - 1 points"):
        call(points=big)
    with pytest.raises(ValueError, match=r"2\^31 - 1 support"):
        call(support=big)
    with pytest.raises(TypeError):
        cloud_normals(torch.zeros(N, 3), 0.5, torch.zeros(M, 3))     # support is a keyword
    with pytest.raises(TypeError):
        cloud_normals(torch.zeros(N, 3))                             # radius is required


@pytest.mark.parametrize("n, m", [(0, M), (N, 0), (0, 0), (0, None)])
def test_empty_clouds_are_answered_without_a_launch(n, m):
    kw = {} if m is None else dict(support=torch.ones(m, 3))
    for view in (None, (0.0, 0.0, 1.0), torch.zeros(n, 3), torch.zeros(3, dtype=torch.float64)):
        r = call(points=torch.zeros(n, 3), viewpoint=view, **kw)
        assert isinstance(r, CloudNormals)
        assert r.normals.shape == (n, 3) and r.normals.dtype == torch.float32 and not r.normals.any()
        assert r.eigenvalues.shape == (n, 3) and r.eigenvalues.dtype == torch.float32 and not r.eigenvalues.any()
        assert r.count.shape == (n,) and r.count.dtype == torch.int32 and not r.count.any()


def test_cpu_tensors_raise_the_usual_runtime_error():
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call(support=torch.ones(M, 3), viewpoint=torch.zeros(N, 3), min_neighbours=10 ** 12, min_gap=0.0)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call(viewpoint=(1, 2, float("inf")), min_gap=0.5)             # (a viewpoint that is not finite decides nothing)


def test_the_function_sits_next_to_cloud_nearest_and_says_what_it_does():
    doc = cloud_normals.__doc__
    assert "bitwise-reproducible" in doc and "order of" in doc and "does not care about the sign" in doc
    assert "2^20" in doc and "quadratic" in doc and "cloud_nearest" in doc
    assert fusion.CloudNormals._fields == ("normals", "eigenvalues", "count")
    assert "cloud_normals" in fusion.__doc__


def test_entry_in_header_binding_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_cloud_normals.hip") == 1 and build.HEADERS.count("mvsn_cloud.h") == 1
    for name in build.SOURCES + build.HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    assert re.search(r"\b%s\(" % ENTRY, header) and ENTRY in _native.SIGNATURES
    decl = re.search(r"^int %s\(([^;]*)\);" % ENTRY, header, re.M).group(1)
    assert len(decl.split(",")) == len(_native.SIGNATURES[ENTRY][1]) == 16
    assert hasattr(ctypes.CDLL(_native.library_path()), ENTRY)


def test_the_c_entry_checks_its_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    need = lib.mvsn_cloud_workspace_bytes(M)
    ok = dict(query=one, nq=N, viewpoint=None, rows=0, cell=0.5, inv=2.0, r2=0.25, min_neighbours=3, min_gap=2.0 ** -20,
              ws=one, ws_bytes=need - 1, m=M, normals=one, eigenvalues=one, count=one)

    def fn(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.mvsn_cloud_normals(a["query"], a["nq"], a["viewpoint"], a["rows"], a["cell"], a["inv"], a["r2"],
                                      a["min_neighbours"], a["min_gap"], a["ws"], a["ws_bytes"], a["m"], a["normals"],
                                      a["eigenvalues"], a["count"], None)
    # (nothing passes: the workspace is one byte short throughout, or misaligned)
    assert fn() == -3 and b"mvsn_cloud_normals" in lib.mvsn_last_error() and b"workspace" in lib.mvsn_last_error()
    assert fn(eigenvalues=None) == -3                             # eigenvalues are optional
    for name in ("query", "normals", "count"):
        assert fn(**{name: None}) == -1, name
    assert b"mvsn_cloud_normals" in lib.mvsn_last_error()
    assert fn(nq=0) == -1 and fn(m=0) == -1 and fn(nq=-5) == -1
    assert fn(viewpoint=one, rows=0) == -1 and fn(rows=1) == -1 and fn(viewpoint=one, rows=2) == -1 and fn(viewpoint=one, rows=-1) == -1
    assert fn(viewpoint=one, rows=1) == -3 and fn(viewpoint=one, rows=N) == -3
    for name in ("cell", "inv", "r2"):
        assert fn(**{name: 0.0}) == -1 and fn(**{name: float("nan")}) == -1 and fn(**{name: float("inf")}) == -1, name
    assert fn(min_neighbours=2) == -1 and fn(min_gap=-0.5) == -1 and fn(min_gap=1.0) == -1 and fn(min_gap=float("nan")) == -1
    assert fn(min_gap=0.0) == -3
    assert fn(nq=2 ** 31) == -2 and fn(m=2 ** 31) == -2 and b"mvsn_cloud_normals" in lib.mvsn_last_error()
    assert fn(ws=None) == -3 and fn(ws_bytes=0) == -3
    assert fn(ws=ctypes.c_void_p(24), ws_bytes=need) == -1        # not 16-byte aligned
    # the codes in their order: a null pointer before the size, the size before the workspace
    assert fn(query=None, nq=2 ** 31, ws=None) == -1 and fn(nq=2 ** 31, ws=None) == -2
