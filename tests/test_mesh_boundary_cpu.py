"""The mesh components and the mesh filter without a GPU: host-side validation (everything is rejected before any
launch), CPU tensors, the empty mesh, and the library's mesh entries in the header, the binding and the binary."""
import ctypes
import os
import re

import pytest
import torch

from multi_view_stereonet_amd import _native, build
from multi_view_stereonet_amd.mesh import FilteredMesh, MeshComponents, filter_mesh, mesh_components
from multi_view_stereonet_amd.tsdf import TSDFMesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvsn_mesh_workspace_bytes", "mvsn_mesh_components_label", "mvsn_mesh_components_emit", "mvsn_mesh_select",
           "mvsn_mesh_compact")
M, F, C = 6, 2, 2


def faces(**kw):
    return torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int64, **kw)


def mesh(m=M, color=True, **kw):
    a = dict(vertices=torch.zeros(m, 3), normals=torch.zeros(m, 3), colors=torch.zeros(m, 3, dtype=torch.uint8) if color else None,
             faces=faces() if m == M else torch.zeros((0, 3), dtype=torch.int64), cell=torch.arange(m))
    a.update(kw)
    return TSDFMesh(**a)


def components(**kw):
    a = dict(vertex_label=torch.tensor([0, 0, 0, 1, 1, 1]), face_label=torch.tensor([0, 1]), vertex_count=torch.tensor([3, 3]),
             face_count=torch.tensor([1, 1]), first=torch.tensor([0, 3]))
    a.update(kw)
    return MeshComponents(**a)


@pytest.mark.parametrize("f, m, match", [
    ([[0, 1, 2]], 3, "faces"), (torch.zeros(3, dtype=torch.int64), 3, "faces"), (torch.zeros((2, 4), dtype=torch.int64), 3, "faces"),
    (torch.zeros((2, 3), dtype=torch.int32), 3, "faces"), (torch.zeros((2, 3)), 3, "faces"),
    (faces(), -1, "num_vertices"), (faces(), 2.5, "num_vertices"), (faces(), True, "num_vertices"), (faces(), "six", "num_vertices"),
    (faces(), None, "num_vertices"), (faces(), 2 ** 31, r"2\^31 - 1"),
    (torch.zeros((2 ** 31, 3), dtype=torch.int64, device="meta"), 3, r"2\^31 - 1"),
])
def test_mesh_components_arguments_are_validated(f, m, match):
    with pytest.raises(ValueError, match=match):
        mesh_components(f, m)


def test_cpu_tensors_raise_the_usual_runtime_error():
    with pytest.raises(RuntimeError, match="HIP devices only"):
        mesh_components(faces(), M)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        mesh_components(torch.zeros((0, 3), dtype=torch.int64), 4)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        filter_mesh(mesh(), min_faces=1)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        filter_mesh(mesh(color=False), keep=torch.ones(C, dtype=torch.bool), components=components())


def test_no_vertices_gives_empties_without_a_launch():
    comp = mesh_components(faces(), 0)                          # (every face names a row that is not there)
    assert isinstance(comp, MeshComponents)
    assert comp.vertex_label.shape == (0,) and comp.face_label.tolist() == [-1, -1]
    assert comp.vertex_count.shape == comp.face_count.shape == comp.first.shape == (0,)
    assert all(t.dtype == torch.int64 for t in comp)
    for color in (False, True):
        got = filter_mesh(mesh(0, color), min_faces=3)
        assert isinstance(got, FilteredMesh) and isinstance(got.mesh, TSDFMesh)
        assert got.mesh.vertices.shape == got.mesh.normals.shape == got.mesh.faces.shape == (0, 3)
        assert got.mesh.cell.shape == got.vertex_rows.shape == got.face_rows.shape == (0,)
        assert got.mesh.vertices.dtype == torch.float32 and got.mesh.faces.dtype == got.vertex_rows.dtype == torch.int64
        assert (got.mesh.colors is None) != color
        assert got.components.first.shape == (0,)


@pytest.mark.parametrize("kw, match", [
    (dict(), "give one of"), (dict(components=components()), "give one of"),
    (dict(keep=torch.ones(C, dtype=torch.bool), min_faces=1), "keep replaces"),
    (dict(keep=torch.ones(C, dtype=torch.bool), min_vertices=1), "keep replaces"),
    (dict(keep=torch.ones(C, dtype=torch.bool), keep_largest=1), "keep replaces"),
    (dict(min_faces=-1), "min_faces"), (dict(min_faces=1.5), "min_faces"), (dict(min_faces="many"), "min_faces"),
    (dict(min_faces=True), "min_faces"), (dict(min_vertices=-3), "min_vertices"), (dict(min_vertices=0.5), "min_vertices"),
    (dict(keep_largest=-1), "keep_largest"), (dict(keep_largest=1.25), "keep_largest"), (dict(keep_largest=[1]), "keep_largest"),
    (dict(keep=[True, False]), "keep must be"), (dict(keep=torch.ones(C, dtype=torch.uint8)), "keep must be"),
    (dict(keep=torch.ones((C, 1), dtype=torch.bool)), "keep must be"),
    (dict(keep=torch.ones(C, dtype=torch.bool, device="meta")), "keep is on"),
    (dict(keep=torch.ones(C + 1, dtype=torch.bool), components=components()), r"keep must be a \(2,\)"),
    (dict(min_faces=1, components=(1, 2, 3)), "components must be"),
    (dict(min_faces=1, components=components(vertex_label=torch.zeros(M + 1, dtype=torch.int64))), "components.vertex_label"),
    (dict(min_faces=1, components=components(face_label=torch.zeros(F, dtype=torch.int32))), "components.face_label"),
    (dict(min_faces=1, components=components(face_count=torch.zeros(C + 1, dtype=torch.int64))), "components.face_count"),
    (dict(min_faces=1, components=components(first=torch.zeros(C, dtype=torch.int64, device="meta"))), "components.first is on"),
    (dict(min_faces=1, components=components(vertex_count=torch.zeros(M + 1, dtype=torch.int64),
                                            face_count=torch.zeros(M + 1, dtype=torch.int64),
                                            first=torch.zeros(M + 1, dtype=torch.int64))), "7 components"),
])
def test_filter_mesh_arguments_are_validated(kw, match):
    with pytest.raises(ValueError, match=match):
        filter_mesh(mesh(), **kw)


@pytest.mark.parametrize("kw, match", [
    (dict(vertices=torch.zeros(M, 2)), "mesh.vertices"), (dict(vertices=torch.zeros(M, 3, dtype=torch.float64)), "mesh.vertices"),
    (dict(normals=torch.zeros(M + 1, 3)), "mesh.normals"), (dict(normals=torch.zeros(M, 3, device="meta")), "mesh.normals is on"),
    (dict(colors=torch.zeros(M, 3)), "mesh.colors"), (dict(cell=torch.zeros(M, dtype=torch.int32)), "mesh.cell"),
    (dict(faces=torch.zeros((F, 3), dtype=torch.int32)), "faces"), (dict(faces=torch.zeros((F, 3), dtype=torch.int64, device="meta")), "mesh.faces is on"),
])
def test_filter_mesh_checks_the_mesh(kw, match):
    with pytest.raises(ValueError, match=match):
        filter_mesh(mesh(**kw), min_faces=1)
    with pytest.raises(ValueError, match="mesh must be"):
        filter_mesh((torch.zeros(M, 3), faces()), min_faces=1)


def test_entries_in_header_binding_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_mesh.hip") == 1
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SIGNATURES
    lib = ctypes.CDLL(_native.library_path())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    lib.mvsn_abi_version.restype = ctypes.c_int
    assert lib.mvsn_abi_version() == 7
    size = lib.mvsn_mesh_workspace_bytes
    size.restype, size.argtypes = ctypes.c_size_t, [ctypes.c_long] * 2
    assert size(0, 4) == 0 and size(-1, 4) == 0 and size(4, -1) == 0
    assert size(2 ** 31, 4) == 0 and size(4, 2 ** 31) == 0
    assert size(1, 0) > 0 and size(1, 0) % 256 == 0
    # 8 bytes per vertex, 12 per 256 vertices and per 256 faces, every section on a 256-byte boundary
    top = size(2 ** 31 - 1, 2 ** 31 - 1)
    assert 8 * (2 ** 31 - 1) + 2 * 12 * 2 ** 23 <= top <= 8 * (2 ** 31 - 1) + 2 * 12 * 2 ** 23 + 6 * 256
    assert 8 * 1029 + 12 * 5 + 12 * 5 <= size(1029, 1027) <= 8 * 1029 + 120 + 6 * 256
    assert size(1029, 0) == size(1029, 256) < size(1029, 64 * 256 + 1)      # (one workgroup of faces at the least)


def test_c_entries_check_their_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    big = 1 << 20

    def label(faces=one, m=8, f=4, result=one, ws=one, ws_bytes=big):
        return lib.mvsn_mesh_components_label(faces, m, f, result, ws, ws_bytes, None)
    assert label(faces=None) == -1 and b"mvsn_mesh_components_label" in lib.mvsn_last_error()
    assert label(result=None) == -1 and label(m=0) == -1 and label(m=-1) == -1 and label(f=-1) == -1
    assert label(m=2 ** 31) == -2 and label(f=2 ** 31) == -2
    assert label(ws=None) == -3 and label(ws_bytes=8) == -3 and label(ws=ctypes.c_void_p(8)) == -1

    def emit(faces=one, m=8, f=4, ws=one, ws_bytes=big, c=2, vertex_label=one, face_label=one, first=one):
        return lib.mvsn_mesh_components_emit(faces, m, f, ws, ws_bytes, c, vertex_label, face_label, one, one, first, None)
    assert emit(faces=None) == -1 and b"mvsn_mesh_components_emit" in lib.mvsn_last_error()
    assert emit(vertex_label=None) == -1 and emit(face_label=None) == -1 and emit(first=None) == -1
    assert emit(m=0) == -1 and emit(f=-1) == -1 and emit(m=2 ** 31) == -2 and emit(f=2 ** 31) == -2
    assert emit(ws=None) == -3 and emit(ws_bytes=8) == -3
    assert emit(c=0) == -1 and emit(c=9) == -1 and emit(c=-1) == -1        # a count the workspace cannot hold

    def select(vertex_label=one, face_label=one, keep=one, m=8, f=4, c=2, result=one, ws=one, ws_bytes=big):
        return lib.mvsn_mesh_select(vertex_label, face_label, keep, m, f, c, result, ws, ws_bytes, None)
    assert select(vertex_label=None) == -1 and b"mvsn_mesh_select" in lib.mvsn_last_error()
    assert select(face_label=None) == -1 and select(keep=None) == -1 and select(result=None) == -1
    assert select(m=0) == -1 and select(f=-1) == -1 and select(m=2 ** 31) == -2 and select(f=2 ** 31) == -2
    assert select(ws=None) == -3 and select(ws_bytes=8) == -3 and select(c=0) == -1 and select(c=9) == -1

    def compact(vertices=one, colors=None, out_colors=None, keep=one, m=8, f=4, c=2, ws=one, ws_bytes=big, mo=1, fo=1,
                out_vertices=one, face_rows=one):
        return lib.mvsn_mesh_compact(vertices, one, colors, one, one, one, keep, m, f, c, ws, ws_bytes, mo, fo,
                                     out_vertices, one, out_colors, one, one, one, face_rows, None)
    assert compact(vertices=None) == -1 and b"mvsn_mesh_compact" in lib.mvsn_last_error()
    assert compact(keep=None) == -1 and compact(colors=one) == -1 and compact(out_colors=one) == -1
    assert compact(m=0) == -1 and compact(f=-1) == -1 and compact(m=2 ** 31) == -2 and compact(f=2 ** 31) == -2
    assert compact(ws=None) == -3 and compact(ws_bytes=8) == -3 and compact(c=0) == -1 and compact(c=9) == -1
    assert compact(mo=-1) == -1 and compact(mo=9) == -1 and compact(fo=-1) == -1 and compact(fo=5) == -1
    assert compact(out_vertices=None) == -1 and compact(face_rows=None) == -1
    assert compact(mo=0, fo=0, out_vertices=None, face_rows=None) == 0     # nothing kept: no launch
