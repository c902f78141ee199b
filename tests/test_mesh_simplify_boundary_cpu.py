"""mesh_simplify without a GPU: host-side validation (everything is rejected before any launch), CPU tensors, the answers
that need no launch, and the new entries in the header, the binding, the build and the binary."""
import ctypes
import os
import re

import pytest
import torch

from multi_view_stereonet_amd import _native, build, mesh
from multi_view_stereonet_amd.mesh import SimplifiedMesh, mesh_simplify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvsn_mesh_simplify_workspace_bytes", "mvsn_mesh_simplify_assign", "mvsn_mesh_simplify_mark",
           "mvsn_mesh_simplify_emit")
M = 4


def verts(**kw):
    return torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32, **kw)


def faces(**kw):
    return torch.tensor([[0, 1, 2], [0, 1, 3]], dtype=torch.int64, **kw)


@pytest.fixture
def no_launch(monkeypatch):
    """Any attempt to reach the library fails the test: what passes under it was answered on the host."""
    def refuse():
        raise AssertionError("the library was loaded: a launch was on its way")
    monkeypatch.setattr(_native, "load", refuse)


@pytest.mark.parametrize("args, kw, match", [
    (([[0, 0, 0]], faces(), 0.5), {}, "vertices"), ((torch.zeros(M, 2), faces(), 0.5), {}, "vertices"),
    ((torch.zeros(M, 3, dtype=torch.float64), faces(), 0.5), {}, "vertices"),
    ((verts(), torch.zeros((2, 3), dtype=torch.int32), 0.5), {}, "faces"),
    ((verts(), torch.zeros((2, 4), dtype=torch.int64), 0.5), {}, "faces"), ((verts(), [[0, 1, 2]], 0.5), {}, "faces"),
    ((verts(), faces(device="meta"), 0.5), {}, "faces are on"),
    ((verts(), torch.zeros((2 ** 31, 3), dtype=torch.int64, device="meta"), 0.5), {}, r"2\^31 - 1"),
    ((torch.zeros((2 ** 31, 3), device="meta"), faces(device="meta"), 0.5), {}, r"2\^31 - 1"),
    ((verts(), faces(), 0.0), {}, "voxel_size"), ((verts(), faces(), -1.0), {}, "voxel_size"),
    ((verts(), faces(), float("nan")), {}, "voxel_size"), ((verts(), faces(), float("inf")), {}, "voxel_size"),
    ((verts(), faces(), 1e-40), {}, "voxel_size"), ((verts(), faces(), 1e39), {}, "voxel_size"),
    ((verts(), faces(), "small"), {}, "voxel_size"),
    ((verts(), faces(), 0.5), dict(origin=(0.0, 0.0)), "origin"), ((verts(), faces(), 0.5), dict(origin=(0.0, 0.0, float("inf"))), "origin"),
    ((verts(), faces(), 0.5), dict(origin="here"), "origin"),
    ((verts(), faces(), 0.5), dict(placement="median"), "placement"), ((verts(), faces(), 0.5), dict(placement=1), "placement"),
    ((verts(), faces(), 0.5), dict(placement=None), "placement"), ((verts(), faces(), 0.5), dict(placement=["mean"]), "placement"),
    ((verts(), faces(), 0.5), dict(normals=torch.zeros(M + 1, 3)), "normals"),
    ((verts(), faces(), 0.5), dict(normals=torch.zeros(M, 3, dtype=torch.float64)), "normals"),
    ((verts(), faces(), 0.5), dict(normals=torch.zeros(M, 3, device="meta")), "normals are on"),
    ((verts(), faces(), 0.5), dict(colors=torch.zeros(M, 3)), "colors"),
    ((verts(), faces(), 0.5), dict(colors=torch.zeros(M, 4, dtype=torch.uint8)), "colors"),
    ((verts(), faces(), 0.5), dict(colors=torch.zeros(M, 3, dtype=torch.uint8, device="meta")), "colors are on"),
])
def test_arguments_are_validated_before_any_launch(no_launch, args, kw, match):
    with pytest.raises(ValueError, match=match):
        mesh_simplify(*args, **kw)


def test_cpu_tensors_raise_the_usual_runtime_error(no_launch):
    for kw in (dict(), dict(placement="mean"), dict(drop_unreferenced=False),
               dict(normals=torch.zeros(M, 3), colors=torch.zeros(M, 3, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="mesh_simplify runs on HIP devices only") as mine:
            mesh_simplify(verts(), faces(), 0.5, **kw)
        assert "(there is no CPU implementation)" in str(mine.value)
    with pytest.raises(RuntimeError, match="HIP devices only"):        # vertices without faces still have clusters
        mesh_simplify(verts(), torch.zeros((0, 3), dtype=torch.int64), 0.5, drop_unreferenced=False)


@pytest.mark.parametrize("placement", ["mean", "quadric"])
@pytest.mark.parametrize("v, f, drop", [
    (torch.zeros((0, 3)), faces(), True), (torch.zeros((0, 3)), faces(), False),
    (torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int64), False), (verts(), torch.zeros((0, 3), dtype=torch.int64), True)])
def test_empty_meshes_give_typed_empties_without_a_launch(no_launch, placement, v, f, drop):
    m = v.shape[0]
    for kw in (dict(), dict(normals=torch.zeros(m, 3)), dict(colors=torch.zeros(m, 3, dtype=torch.uint8)),
               dict(normals=torch.zeros(m, 3), colors=torch.zeros(m, 3, dtype=torch.uint8))):
        got = mesh_simplify(v, f, 0.5, placement=placement, drop_unreferenced=drop, **kw)
        assert isinstance(got, SimplifiedMesh) and got._fields == ("vertices", "faces", "normals", "colors", "count", "first",
                                                                   "inverse", "face_rows")
        assert got.vertices.shape == (0, 3) and got.vertices.dtype == torch.float32
        assert got.faces.shape == (0, 3) and got.faces.dtype == torch.int64
        assert got.count.shape == (0,) and got.count.dtype == torch.int32
        assert got.first.shape == got.face_rows.shape == (0,) and got.first.dtype == got.face_rows.dtype == torch.int64
        assert got.inverse.dtype == torch.int64 and got.inverse.tolist() == [-1] * m
        assert (got.normals is None) == ("normals" not in kw) and (got.colors is None) == ("colors" not in kw)
        if got.normals is not None:
            assert got.normals.shape == (0, 3) and got.normals.dtype == torch.float32
        if got.colors is not None:
            assert got.colors.shape == (0, 3) and got.colors.dtype == torch.uint8


def test_entries_in_header_binding_build_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_mesh_simplify.hip") == 1
    with open(os.path.join(build.CSRC, "mvsn_mesh_simplify.hip")) as f:
        included = set(re.findall(r'#include "(mvsn_\w+\.h)"', f.read()))
    assert included == {"mvsn_common.h", "mvsn_geom.h", "mvsn_mesh.h", "mvsn_voxel.h"} and included <= set(build.HEADERS)
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SIGNATURES
    assert re.search(r"#define\s+MVSN_MESH_SIMPLIFY_STATUS_TABLE\s+%d\b" % mesh.MESH_SIMPLIFY_STATUS_TABLE, header)
    assert mesh.SIMPLIFY_PLACEMENTS == {"mean": 0, "quadric": 1} and mesh.SIMPLIFY_LAMBDA == 2.0 ** -10
    lib = ctypes.CDLL(_native.library_path())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    size = _native.load().mvsn_mesh_simplify_workspace_bytes
    assert size(0, 5) == 0 and size(-1, 5) == 0 and size(2 ** 31, 5) == 0 and size(5, -1) == 0 and size(5, 2 ** 31) == 0
    assert size(1, 0) > 0 and size(1, 0) % 256 == 0 and size(5, 0) < size(5, 1)
    # on top of the voxel merge's workspace: 223 bytes per vertex, 12 per 256 of them; 4 per face and per slot of the face
    # table (1024 slots up to 512 faces, then the power of two >= 2 faces), 12 per 256 faces; 256-byte sections
    voxel = _native.load().mvsn_voxel_workspace_bytes
    for m, f, slots in ((1000, 0, 0), (1000, 300, 1024), (1000, 2000, 4096), (70000, 150000, 2 ** 19)):
        least = voxel(m) + 223 * m + 12 * ((m + 255) // 256) + 4 * f + 4 * slots + 12 * ((f + 255) // 256)
        assert least <= size(m, f) <= least + 20 * 256, (m, f)


def test_c_entries_check_their_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    big = 1 << 24

    def assign(vertices=one, m=8, v=1.0, inv=1.0, result=one, ws=one, ws_bytes=big):
        return lib.mvsn_mesh_simplify_assign(vertices, m, v, inv, 0.0, 0.0, 0.0, result, ws, ws_bytes, None)
    assert assign(vertices=None) == -1 and b"mvsn_mesh_simplify_assign" in lib.mvsn_last_error()
    assert assign(result=None) == -1 and assign(m=0) == -1 and assign(m=2 ** 31) == -2
    assert assign(ws=None) == -3 and assign(ws_bytes=8) == -3
    assert assign(v=0.0) == -1 and assign(inv=float("inf")) == -1 and assign(ws=ctypes.c_void_p(8)) == -1

    def mark(vertices=one, m=8, faces=one, f=4, placement=1, clusters=3, result=one, ws=one, ws_bytes=big):
        return lib.mvsn_mesh_simplify_mark(vertices, None, None, m, faces, f, 1.0, 1.0, 0.0, 0.0, 0.0, placement, 1, clusters,
                                           result, ws, ws_bytes, None)
    assert mark(vertices=None) == -1 and b"mvsn_mesh_simplify_mark" in lib.mvsn_last_error()
    assert mark(result=None) == -1 and mark(ws=None) == -1 and mark(faces=None) == -1 and mark(m=0) == -1 and mark(f=-1) == -1
    assert mark(clusters=0) == -1 and mark(clusters=9) == -1 and mark(placement=2) == -1 and mark(placement=-1) == -1
    assert mark(m=2 ** 31, clusters=3) == -2 and mark(f=2 ** 31) == -2
    assert mark(ws_bytes=8) == -3 and mark(ws=ctypes.c_void_p(8)) == -1

    def emit(faces=one, m=8, f=4, clusters=3, ws=one, ws_bytes=big, mo=2, fo=1, vertices=one, out_faces=one, count=one,
             first=one, inverse=one, face_rows=one):
        return lib.mvsn_mesh_simplify_emit(faces, m, f, clusters, ws, ws_bytes, mo, fo, vertices, out_faces, None, None, count,
                                           first, inverse, face_rows, None)
    assert emit(ws=None) == -1 and b"mvsn_mesh_simplify_emit" in lib.mvsn_last_error()
    assert emit(inverse=None) == -1 and emit(m=0) == -1 and emit(clusters=0) == -1 and emit(clusters=9) == -1
    assert emit(mo=-1) == -1 and emit(mo=4) == -1 and emit(fo=-1) == -1 and emit(fo=5) == -1
    assert emit(m=2 ** 31) == -2 and emit(f=2 ** 31) == -2 and emit(ws_bytes=8) == -3
    assert emit(vertices=None) == -1 and emit(count=None) == -1 and emit(first=None) == -1
    assert emit(faces=None) == -1 and emit(out_faces=None) == -1 and emit(face_rows=None) == -1
