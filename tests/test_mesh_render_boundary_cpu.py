"""mesh_render without a GPU: host-side validation (everything is rejected before any launch), empty meshes, CPU tensors,
and the library's entries in the header, the binding, the build list and the binary."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import mesh_render_reference as mr
from multi_view_stereonet_amd import _native, build, mesh
from multi_view_stereonet_amd.mesh import MeshRender, mesh_render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mvsn_mesh_render_workspace_bytes": 3, "mvsn_mesh_render_small_pixels": 0, "mvsn_mesh_render": 22}
M, F, V, H, W = 5, 4, 2, 3, 4
NAN, INF = float("nan"), float("inf")


@pytest.fixture
def no_library(monkeypatch):
    """The library unreachable: whatever passes under it was decided on the host, before any launch."""
    def unreachable():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load", unreachable)


def eyes(v=V, **kw):
    return torch.eye(4, **kw).expand(v, 4, 4).clone()


def faces(f=F, **kw):
    return torch.zeros(f, 3, dtype=torch.int64, **kw)


def render(**kw):
    a = dict(vertices=torch.zeros(M, 3), faces=faces(), K=eyes(), T=eyes(), size=(H, W))
    a.update(kw)
    pos = [a.pop(k) for k in ("vertices", "faces", "K", "T", "size")]
    return mesh_render(*pos, **a)


BAD_MESH = [
    (dict(vertices=None), "vertices must be"), (dict(vertices=torch.zeros(M, 4)), "vertices must be"),
    (dict(vertices=torch.zeros(M)), "vertices must be"), (dict(vertices=torch.zeros(M, 3, dtype=torch.float64)), "vertices must be"),
    (dict(faces=None), "faces must be"), (dict(faces=torch.zeros(F, 3, dtype=torch.int32)), "faces must be"),
    (dict(faces=torch.zeros(F, 4, dtype=torch.int64)), "faces must be"), (dict(faces=torch.zeros(F, dtype=torch.int64)), "faces must be"),
    (dict(faces=torch.zeros(1, 3, dtype=torch.int64).expand(2 ** 31, 3)), r"2\^31 - 1 vertices and faces"),
    (dict(vertices=torch.zeros(1, 3).expand(2 ** 31, 3)), r"2\^31 - 1 vertices and faces"),
    (dict(faces=faces(device="meta")), "faces are on meta"),
]
BAD_REST = [
    (dict(K=None), "K must be"), (dict(K=torch.eye(4)), "K must be"), (dict(K=eyes(V + 1)), "must be a"),
    (dict(K=torch.zeros(V, 3, 3)), "K must be"), (dict(K=eyes(dtype=torch.int32)), "K must be a floating-point"),
    (dict(T=None), "T_cam_in_world must be"), (dict(T=eyes(V + 1)), "T_cam_in_world must be"),
    (dict(T=eyes(dtype=torch.int64)), "T_cam_in_world must be a floating-point"),
    (dict(K=eyes(device="meta")), "K is on meta"), (dict(T=eyes(device="meta")), "T_cam_in_world is on meta"),
    (dict(K=torch.zeros(0, 4, 4), T=torch.zeros(0, 4, 4)), "1..65535 views"),
    (dict(K=torch.eye(4).expand(65536, 4, 4), T=torch.eye(4).expand(65536, 4, 4)), "1..65535 views"),
    (dict(size=None), "size must be"), (dict(size=5), "size must be"), (dict(size=(3,)), "size must be"),
    (dict(size=(3, 4, 5)), "size must be"), (dict(size=(0, 4)), "size must be"), (dict(size=(3, -1)), "size must be"),
    (dict(size=(2.5, 4)), "size must be"), (dict(size=(True, 4)), "size must be"), (dict(size=(2 ** 15 + 1, 1)), "size must be"),
    (dict(size=(1, 2 ** 15 + 1)), r"2\^15"),
    (dict(min_depth=-1.0), "min_depth must be"), (dict(min_depth=NAN), "min_depth must be"),
    (dict(min_depth=INF), "min_depth must be"), (dict(min_depth=None), "min_depth must be"),
    (dict(min_depth="near"), "min_depth must be"),
    (dict(max_depth=0.0), "max_depth must be"), (dict(max_depth=-2.0), "max_depth must be"),
    (dict(max_depth=NAN), "max_depth must be"), (dict(max_depth=None), "max_depth must be"),
]
BAD_GATHERS = [
    (dict(colors=torch.zeros(M, 3)), "colors must be"), (dict(colors=torch.zeros(M, 4, dtype=torch.uint8)), "colors must be"),
    (dict(colors=torch.zeros(M + 1, 3, dtype=torch.uint8)), "colors must be"), (dict(colors=[[0, 0, 0]] * M), "colors must be"),
    (dict(colors=torch.zeros(F, 3, dtype=torch.uint8)), "one row per vertex"),
    (dict(colors=torch.zeros(M, 3, dtype=torch.uint8, device="meta")), "colors are on meta"),
    (dict(normals=torch.zeros(M, 3, dtype=torch.float64)), "normals must be"),
    (dict(normals=torch.zeros(M - 1, 3)), "normals must be"), (dict(normals=torch.zeros(3, M)), "normals must be"),
    (dict(normals=torch.zeros(M, 3, device="meta")), "normals are on meta"),
]


@pytest.mark.parametrize("kw, match", BAD_MESH + BAD_REST + BAD_GATHERS)
def test_mesh_render_validates_before_any_launch(kw, match, no_library):
    with pytest.raises(ValueError, match=match):
        render(**kw)


@pytest.mark.parametrize("kw, match", BAD_REST)
def test_an_empty_mesh_is_validated_like_any_other(kw, match, no_library):
    with pytest.raises(ValueError, match=match):
        render(faces=faces(0), **kw)
    with pytest.raises(ValueError, match=match):
        render(vertices=torch.zeros(0, 3), **kw)


def test_the_options_are_keywords_and_the_defaults_are_the_interfaces():
    with pytest.raises(TypeError):
        mesh_render(torch.zeros(M, 3), faces(), eyes(), eyes(), (H, W), None)
    with pytest.raises(TypeError):
        mesh_render(torch.zeros(M, 3), faces(), eyes(), eyes())
    p = inspect.signature(mesh_render).parameters
    assert list(p)[:5] == ["vertices", "faces", "K", "T_cam_in_world", "size"]
    assert p["normals"].default is None and p["colors"].default is None
    assert p["min_depth"].default == 0.0 and p["max_depth"].default == INF
    assert MeshRender._fields == mr.OUTPUTS and mesh.RENDER_MAX_EXTENT == 2 ** 15


@pytest.mark.parametrize("gathers", [False, True])
@pytest.mark.parametrize("m, f", [(M, 0), (0, F), (0, 0)])
def test_an_empty_mesh_renders_all_misses_without_a_launch(m, f, gathers, no_library):
    kw = dict(normals=torch.zeros(m, 3), colors=torch.zeros(m, 3, dtype=torch.uint8)) if gathers else {}
    r = render(vertices=torch.zeros(m, 3), faces=faces(f), **kw)
    assert isinstance(r, MeshRender)
    assert r.depth.shape == (V, 1, H, W) and r.depth.dtype == torch.float32 and not r.depth.any()
    assert r.face.shape == (V, H, W) and r.face.dtype == torch.int64 and (r.face == -1).all()
    assert r.weights.shape == (V, 3, H, W) and r.weights.dtype == torch.float32 and not r.weights.any()
    assert r.clipped.shape == (V,) and r.clipped.dtype == torch.int64 and not r.clipped.any()
    if gathers:
        assert r.normals.shape == (V, 3, H, W) and r.normals.dtype == torch.float32 and not r.normals.any()
        assert r.colors.shape == (V, 3, H, W) and r.colors.dtype == torch.uint8 and not r.colors.any()
    else:
        assert r.normals is None and r.colors is None


def test_a_cpu_mesh_raises_the_usual_runtime_error(no_library):
    with pytest.raises(RuntimeError, match="mesh_render runs on HIP devices only"):
        render()
    with pytest.raises(RuntimeError, match="HIP devices only"):   # (double-precision cameras are accepted)
        render(K=eyes(dtype=torch.float64), T=eyes(dtype=torch.float16))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        render(normals=torch.zeros(M, 3), colors=torch.zeros(M, 3, dtype=torch.uint8), min_depth=0.5, max_depth=INF)


def test_the_function_says_what_it_does():
    for word in ("perspective-correct", "no near-plane clipping", "clipped[v]", "1/256", "exactly one owns", "lowest row",
                 "bitwise-reproducible", "integer minimum", "without a launch", "no host synchronisation",
                 "cloud_visibility", "depth_metric_rows", "both sides"):
        assert word in mesh_render.__doc__, word
    assert "mesh_render" in mesh.__doc__ and "section 27" in mesh.__doc__


# ---- the library's entries ---------------------------------------------------------------------------------------------
def test_entries_in_header_binding_build_list_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_mesh_render.hip") == 1 and build.HEADERS.count("mvsn_camera.h") == 1
    for name in build.SOURCES + build.HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert re.search(r"#define\s+MVSN_ABI_VERSION\s+7\b", header)
    lib = ctypes.CDLL(_native.library_path())
    for entry, count in ENTRIES.items():
        assert re.search(r"\b%s\(" % entry, header) and entry in _native.SIGNATURES
        decl = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % entry, header, re.M).group(1)
        args = [] if decl.strip() == "void" else decl.split(",")
        assert len(args) == len(_native.SIGNATURES[entry][1]) == count, entry
        assert hasattr(lib, entry)
    assert "DESIGN.md section 27" in header and "Integer atomics only" in header


def test_the_kernels_share_the_camera_and_keep_contraction_off():
    with open(os.path.join(build.CSRC, "mvsn_mesh_render.hip")) as f:
        text = f.read()
    assert '#include "mvsn_camera.h"' in text and not re.search(r"__device__[^;{]*\btsdf_camera\(", text)
    assert "#pragma clang fp contract(off)" in text
    assert "__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)" in text
    # one projection and one pixel function serve the raster and the resolve: the resolve forms the raster's bits
    assert len(re.findall(r"\bMrSnap mr_snap\(", text)) == 1 and len(re.findall(r"= mr_snap\(", text)) == 2
    assert len(re.findall(r"\bbool mr_pixel\(", text)) == 1


def test_the_entries_check_their_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    size = lib.mvsn_mesh_render_workspace_bytes
    assert lib.mvsn_mesh_render_small_pixels() == mr.SMALL_PIXELS
    assert size(0, 3, 4) == 0 and size(65536, 3, 4) == 0 and size(1, 0, 4) == 0 and size(1, 3, -1) == 0
    assert size(1, 2 ** 15 + 1, 1) == 0 and size(1, 1, 2 ** 15 + 1) == 0
    assert size(1, 1, 1) == 16 and size(V, H, W) == 8 * V * (H * W + 1)
    assert size(65535, 2 ** 15, 2 ** 15) == 8 * 65535 * (2 ** 30 + 1)
    need = size(V, H, W)
    ok = dict(vertices=one, m=M, faces=one, f=F, normals=one, colors=one, K=one, T=one, v=V, rows=H, cols=W, lo=0.0, hi=INF,
              ws=one, ws_bytes=need - 1, depth=one, face=one, weights=one, out_normals=one, out_colors=one, clipped=one)

    def rend(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.mvsn_mesh_render(a["vertices"], a["m"], a["faces"], a["f"], a["normals"], a["colors"], a["K"], a["T"],
                                    a["v"], a["rows"], a["cols"], a["lo"], a["hi"], a["ws"], a["ws_bytes"], a["depth"],
                                    a["face"], a["weights"], a["out_normals"], a["out_colors"], a["clipped"], None)
    # (nothing passes: the workspace is one byte short throughout)
    assert rend() == -3 and b"mvsn_mesh_render" in lib.mvsn_last_error() and b"workspace" in lib.mvsn_last_error()
    assert rend(ws=None) == -3 and rend(ws_bytes=0) == -3
    assert rend(ws=ctypes.c_void_p(24), ws_bytes=need) == -1      # not 16-byte aligned
    for name in ("vertices", "faces", "K", "T", "depth", "face", "weights", "clipped"):
        assert rend(**{name: None}) == -1 and b"null pointer" in lib.mvsn_last_error(), name
    assert rend(colors=None) == -1 and rend(out_colors=None) == -1 and rend(colors=None, out_colors=None) == -3
    assert rend(normals=None) == -1 and rend(out_normals=None) == -1 and rend(normals=None, out_normals=None) == -3
    assert b"workspace" in lib.mvsn_last_error()
    for name in ("m", "f"):
        assert rend(**{name: 0}) == -1 and rend(**{name: -3}) == -1 and rend(**{name: 2 ** 31}) == -1
        assert b"2^31 - 1" in lib.mvsn_last_error()
        assert rend(**{name: 2 ** 31 - 1}) == -3                  # (the limits themselves pass, up to the workspace)
    assert rend(v=0) == -1 and rend(v=65536) == -1 and rend(v=65535) == -3
    assert rend(rows=0) == -1 and rend(cols=0) == -1 and rend(rows=2 ** 15 + 1) == -1 and rend(cols=2 ** 15 + 1) == -1
    assert rend(rows=2 ** 15, cols=2 ** 15) == -3
    assert rend(lo=-1.0) == -1 and rend(lo=NAN) == -1 and rend(lo=INF) == -1 and rend(lo=1.0) == -3
    assert rend(hi=0.0) == -1 and rend(hi=NAN) == -1 and rend(hi=-1.0) == -1 and rend(hi=1.0) == -3
