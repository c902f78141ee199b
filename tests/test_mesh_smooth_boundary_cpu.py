"""mesh_edges, mesh_smooth and mesh_normals without a GPU: host-side validation (everything is rejected before any
launch), CPU tensors, the answers that need no launch, and the new entries in the header, the binding, the build and the
binary."""
import ctypes
import os
import re

import pytest
import torch

from multi_view_stereonet_amd import _native, build, mesh
from multi_view_stereonet_amd.mesh import MeshEdges, MeshNormals, SmoothedMesh, mesh_edges, mesh_normals, mesh_smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mvsn_mesh_edges_workspace_bytes": 2, "mvsn_mesh_edges_mark": 7, "mvsn_mesh_edges_emit": 13,
           "mvsn_mesh_smooth_workspace_bytes": 1, "mvsn_mesh_smooth": 13, "mvsn_mesh_normals_workspace_bytes": 1,
           "mvsn_mesh_normals": 10}
M = 4


def verts(**kw):
    return torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32, **kw)


def faces(**kw):
    return torch.tensor([[0, 1, 2], [0, 1, 3]], dtype=torch.int64, **kw)


def no_faces(**kw):
    return torch.zeros((0, 3), dtype=torch.int64, **kw)


def cpu_edges(m=M, f=2, e=5, **change):
    """A MeshEdges of the right shapes (the values are never looked at on the host)."""
    fields = dict(edges=torch.zeros((e, 2), dtype=torch.int64), first=torch.zeros(e, dtype=torch.int64),
                  face_count=torch.zeros(e, dtype=torch.int32), winding=torch.zeros(e, dtype=torch.int32),
                  face_edge=torch.zeros((f, 3), dtype=torch.int64), vertex_degree=torch.zeros(m, dtype=torch.int32),
                  vertex_boundary=torch.zeros(m, dtype=torch.bool))
    fields.update(change)
    return MeshEdges(**fields)


@pytest.fixture
def no_launch(monkeypatch):
    """Any attempt to reach the library fails the test: what passes under it was answered on the host."""
    def refuse():
        raise AssertionError("the library was loaded: a launch was on its way")
    monkeypatch.setattr(_native, "load", refuse)


@pytest.mark.parametrize("args, match", [
    (([[0, 1, 2]], M), "faces"), ((torch.zeros((2, 3), dtype=torch.int32), M), "faces"),
    ((torch.zeros((2, 4), dtype=torch.int64), M), "faces"), ((torch.zeros((6,), dtype=torch.int64), M), "faces"),
    ((faces(), -1), "num_vertices"), ((faces(), 2.5), "num_vertices"), ((faces(), True), "num_vertices"),
    ((faces(), 2 ** 31), r"2\^31 - 1"),
    ((torch.zeros(((2 ** 31 - 1) // 3 + 1, 3), dtype=torch.int64, device="meta"), M), r"\(2\^31 - 1\) / 3"),
])
def test_mesh_edges_arguments_are_validated_before_any_launch(no_launch, args, match):
    with pytest.raises(ValueError, match=match):
        mesh_edges(*args)


@pytest.mark.parametrize("args, kw, match", [
    (([[0, 0, 0]], faces()), {}, "vertices"), ((torch.zeros(M, 2), faces()), {}, "vertices"),
    ((torch.zeros(M, 3, dtype=torch.float64), faces()), {}, "vertices"),
    ((verts(), torch.zeros((2, 3), dtype=torch.int32)), {}, "faces"), ((verts(), [[0, 1, 2]]), {}, "faces"),
    ((verts(), faces(device="meta")), {}, "faces are on"),
    ((verts(), faces(), -1), {}, "iterations"), ((verts(), faces(), 10001), {}, "iterations"),
    ((verts(), faces(), 2.5), {}, "iterations"), ((verts(), faces(), True), {}, "iterations"),
    ((verts(), faces(), None), {}, "iterations"),
    ((verts(), faces()), dict(method="cotangent"), "method"), ((verts(), faces()), dict(method=1), "method"),
    ((verts(), faces()), dict(method=None), "method"), ((verts(), faces()), dict(method=["taubin"]), "method"),
    ((verts(), faces()), dict(lam=0.0), "lam"), ((verts(), faces()), dict(lam=-0.5), "lam"),
    ((verts(), faces()), dict(lam=1.0 + 2.0 ** -52), "lam"), ((verts(), faces()), dict(lam=float("nan")), "lam"),
    ((verts(), faces()), dict(lam=float("inf")), "lam"), ((verts(), faces()), dict(lam="half"), "lam"),
    ((verts(), faces()), dict(lam=True), "lam"),
    ((verts(), faces()), dict(mu=0.0), "mu"), ((verts(), faces()), dict(mu=0.5), "mu"),
    ((verts(), faces()), dict(mu=-2.0 - 2.0 ** -51), "mu"), ((verts(), faces()), dict(mu=float("nan")), "mu"),
    ((verts(), faces()), dict(mu=float("-inf")), "mu"), ((verts(), faces()), dict(mu=None), "mu"),
    ((verts(), faces()), dict(method="laplacian", mu=0.25), "mu"),
    ((verts(), faces()), dict(fix_boundary="yes"), "fix_boundary"), ((verts(), faces()), dict(fix_boundary=1), "fix_boundary"),
    ((verts(), faces()), dict(pinned=[False] * M), "pinned"), ((verts(), faces()), dict(pinned=torch.zeros(M + 1, dtype=torch.bool)), "pinned"),
    ((verts(), faces()), dict(pinned=torch.zeros(M, dtype=torch.uint8)), "pinned"),
    ((verts(), faces()), dict(pinned=torch.zeros((M, 1), dtype=torch.bool)), "pinned"),
    ((verts(), faces()), dict(pinned=torch.zeros(M, dtype=torch.bool, device="meta")), "pinned is on"),
    ((verts(), faces()), dict(edges=torch.zeros((5, 2), dtype=torch.int64)), "MeshEdges"),
    ((verts(), faces()), dict(edges=(1, 2, 3)), "MeshEdges"),
    ((verts(), faces()), dict(edges=cpu_edges(m=M + 1)), r"edges\.vertex_degree"),
    ((verts(), faces()), dict(edges=cpu_edges(f=3)), r"edges\.face_edge"),
    ((verts(), faces()), dict(edges=cpu_edges(first=torch.zeros(4, dtype=torch.int64))), r"edges\.first"),
    ((verts(), faces()), dict(edges=cpu_edges(edges=torch.zeros((5, 2), dtype=torch.int32))), r"edges\.edges"),
    ((verts(), faces()), dict(edges=cpu_edges(vertex_boundary=torch.zeros(M, dtype=torch.uint8))), r"edges\.vertex_boundary"),
    ((verts(), faces()), dict(edges=cpu_edges(winding=torch.zeros(5, dtype=torch.int32, device="meta"))), r"edges\.winding is on"),
])
def test_mesh_smooth_arguments_are_validated_before_any_launch(no_launch, args, kw, match):
    with pytest.raises(ValueError, match=match):
        mesh_smooth(*args, **kw)


@pytest.mark.parametrize("args, match", [
    (([[0, 0, 0]], faces()), "vertices"), ((torch.zeros(M, 2), faces()), "vertices"),
    ((torch.zeros(M, 3, dtype=torch.float16), faces()), "vertices"),
    ((verts(), torch.zeros((2, 3), dtype=torch.int32)), "faces"), ((verts(), torch.zeros((2, 2), dtype=torch.int64)), "faces"),
    ((verts(), faces(device="meta")), "faces are on"),
    ((torch.zeros((2 ** 31, 3), device="meta"), faces(device="meta")), r"2\^31 - 1"),
])
def test_mesh_normals_arguments_are_validated_before_any_launch(no_launch, args, match):
    with pytest.raises(ValueError, match=match):
        mesh_normals(*args)


def test_cpu_tensors_raise_the_usual_runtime_error(no_launch):
    calls = (("mesh_edges", lambda: mesh_edges(faces(), M)), ("mesh_normals", lambda: mesh_normals(verts(), faces())),
             ("mesh_normals", lambda: mesh_normals(verts(), no_faces())),     # vertices without faces still get zeros
             ("mesh_smooth", lambda: mesh_smooth(verts(), faces(), edges=cpu_edges())))
    for name, call in calls:
        with pytest.raises(RuntimeError, match="%s runs on HIP devices only" % name) as mine:
            call()
        assert "(there is no CPU implementation)" in str(mine.value)
    with pytest.raises(RuntimeError, match="mesh_edges runs on HIP devices only"):   # the edges come first
        mesh_smooth(verts(), faces(), 3, method="laplacian", fix_boundary=True, pinned=torch.zeros(M, dtype=torch.bool))


def _empty_edges(got, m, f):
    assert isinstance(got, MeshEdges) and got._fields == ("edges", "first", "face_count", "winding", "face_edge",
                                                          "vertex_degree", "vertex_boundary")
    assert got.edges.shape == (0, 2) and got.edges.dtype == torch.int64
    assert got.first.shape == (0,) and got.first.dtype == torch.int64
    assert got.face_count.shape == got.winding.shape == (0,) and got.face_count.dtype == got.winding.dtype == torch.int32
    assert got.face_edge.dtype == torch.int64 and got.face_edge.tolist() == [[-1, -1, -1]] * f
    assert got.vertex_degree.dtype == torch.int32 and got.vertex_degree.tolist() == [0] * m
    assert got.vertex_boundary.dtype == torch.bool and got.vertex_boundary.tolist() == [False] * m


def test_answers_that_need_no_launch(no_launch):
    _empty_edges(mesh_edges(no_faces(), M), M, 0)
    _empty_edges(mesh_edges(no_faces(), 0), 0, 0)
    _empty_edges(mesh_edges(faces(), 0), 0, 2)                        # every face is out of range
    v = verts()
    v[1, 2] = float("nan")
    for kw in (dict(), dict(method="laplacian", iterations=7), dict(fix_boundary=True, pinned=torch.ones(M, dtype=torch.bool))):
        got = mesh_smooth(v, no_faces(), **kw)                        # F = 0: no edge, nothing moves
        assert isinstance(got, SmoothedMesh) and got._fields == ("vertices", "edges")
        assert got.vertices.dtype == torch.float32 and got.vertices.data_ptr() != v.data_ptr()
        assert got.vertices.numpy().tobytes() == v.numpy().tobytes()
        _empty_edges(got.edges, M, 0)
    mine = cpu_edges()
    for method in ("laplacian", "taubin"):                            # iterations = 0 with the edges at hand
        got = mesh_smooth(v, faces(), 0, method=method, edges=mine)
        assert got.vertices.numpy().tobytes() == v.numpy().tobytes() and got.vertices.data_ptr() != v.data_ptr()
        assert all(a is b for a, b in zip(got.edges, mine))
    got = mesh_smooth(torch.zeros((0, 3)), no_faces())
    assert got.vertices.shape == (0, 3)
    _empty_edges(got.edges, 0, 0)
    for f in (no_faces(), faces()):                                   # M = 0
        got = mesh_normals(torch.zeros((0, 3)), f)
        assert isinstance(got, MeshNormals) and got._fields == ("face_normals", "face_area", "vertex_normals")
        assert got.face_normals.dtype == got.face_area.dtype == got.vertex_normals.dtype == torch.float32
        assert got.face_normals.tolist() == [[0.0] * 3] * f.shape[0] and got.face_area.tolist() == [0.0] * f.shape[0]
        assert got.vertex_normals.shape == (0, 3)


def test_entries_in_header_binding_build_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    for source, headers in (("mvsn_mesh_edges.hip", {"mvsn_common.h", "mvsn_geom.h", "mvsn_mesh.h", "mvsn_voxel.h"}),
                            ("mvsn_mesh_smooth.hip", {"mvsn_common.h", "mvsn_geom.h", "mvsn_mesh.h"})):
        assert build.SOURCES.count(source) == 1
        with open(os.path.join(build.CSRC, source)) as f:
            text = f.read()
        assert set(re.findall(r'#include "(mvsn_\w+\.h)"', text)) == headers and headers <= set(build.HEADERS)
        assert text.count("#pragma clang fp contract(off)") == 1 and text.index("#pragma clang fp contract(off)") < text.index("#include")
    lib = ctypes.CDLL(_native.library_path())
    for name, count in ENTRIES.items():
        decl = re.search(r"\b%s\(([^)]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]) == count, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+MVSN_MESH_EDGES_STATUS_TABLE\s+%d\b" % mesh.MESH_EDGES_STATUS_TABLE, header)
    assert mesh.SMOOTH_METHODS == {"laplacian": 0, "taubin": 1} and mesh.SMOOTH_MAX_ITERATIONS == 10000
    assert mesh.MAX_EDGE_FACES == (2 ** 31 - 1) // 3
    typed = _native.load()
    size = typed.mvsn_mesh_edges_workspace_bytes
    assert size(0, 5) == 0 and size(-1, 5) == 0 and size(2 ** 31, 5) == 0 and size(5, 0) == 0 and size(5, -1) == 0
    assert size(5, mesh.MAX_EDGE_FACES + 1) == 0 and size(5, mesh.MAX_EDGE_FACES) > 0
    # 24 bytes per slot of the edge table (1024 slots up to 170 faces, then the power of two >= 6 faces), 12 per face, 12
    # per 256 sides; 256-byte sections
    for f, slots in ((1, 1024), (170, 1024), (171, 2048), (512, 4096), (150000, 2 ** 20)):
        least = 24 * slots + 12 * f + 12 * ((3 * f + 255) // 256)
        assert least <= size(1000, f) <= least + 8 * 256 and size(1000, f) % 256 == 0, f
    for size, per_vertex in ((typed.mvsn_mesh_smooth_workspace_bytes, 56), (typed.mvsn_mesh_normals_workspace_bytes, 32)):
        assert size(0) == 0 and size(-1) == 0 and size(2 ** 31) == 0
        for m in (1, 257, 70000):
            assert per_vertex * m <= size(m) <= per_vertex * m + 6 * 256 and size(m) % 256 == 0, m


def test_c_entries_check_their_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    big = 1 << 24

    def mark(faces=one, m=8, f=4, result=one, ws=one, ws_bytes=big):
        return lib.mvsn_mesh_edges_mark(faces, m, f, result, ws, ws_bytes, None)
    assert mark(faces=None) == -1 and b"mvsn_mesh_edges_mark" in lib.mvsn_last_error()
    assert mark(result=None) == -1 and mark(ws=None) == -1 and mark(m=0) == -1 and mark(f=0) == -1 and mark(f=-1) == -1
    assert mark(m=2 ** 31) == -2 and mark(f=(2 ** 31 - 1) // 3 + 1) == -2
    assert mark(ws_bytes=8) == -3 and mark(ws=ctypes.c_void_p(8)) == -1

    def emit(m=8, f=4, ws=one, ws_bytes=big, e=5, edges=one, first=one, count=one, winding=one, face_edge=one, degree=one,
             boundary=one):
        return lib.mvsn_mesh_edges_emit(m, f, ws, ws_bytes, e, edges, first, count, winding, face_edge, degree, boundary, None)
    assert emit(ws=None) == -1 and b"mvsn_mesh_edges_emit" in lib.mvsn_last_error()
    assert emit(face_edge=None) == -1 and emit(degree=None) == -1 and emit(boundary=None) == -1
    assert emit(m=0) == -1 and emit(f=0) == -1 and emit(e=-1) == -1 and emit(e=13) == -1
    assert emit(m=2 ** 31) == -2 and emit(f=(2 ** 31 - 1) // 3 + 1) == -2 and emit(ws_bytes=8) == -3
    assert emit(edges=None) == -1 and emit(first=None) == -1 and emit(count=None) == -1 and emit(winding=None) == -1

    def smooth(vertices=one, m=8, edges=one, e=5, method=1, iterations=3, lam=0.5, mu=-0.53, ws=one, ws_bytes=big, out=one):
        return lib.mvsn_mesh_smooth(vertices, m, edges, e, None, method, iterations, lam, mu, ws, ws_bytes, out, None)
    assert smooth(vertices=None) == -1 and b"mvsn_mesh_smooth" in lib.mvsn_last_error()
    assert smooth(out=None) == -1 and smooth(ws=None) == -1 and smooth(edges=None) == -1 and smooth(m=0) == -1
    assert smooth(e=-1) == -1 and smooth(m=2 ** 31) == -2 and smooth(e=2 ** 31) == -2
    assert smooth(method=2) == -1 and smooth(method=-1) == -1 and smooth(iterations=-1) == -1 and smooth(iterations=10001) == -1
    assert smooth(lam=0.0) == -1 and smooth(lam=1.5) == -1 and smooth(lam=float("nan")) == -1
    assert smooth(mu=0.0) == -1 and smooth(mu=-2.5) == -1 and smooth(mu=float("nan")) == -1
    assert smooth(ws_bytes=8) == -3 and smooth(ws=ctypes.c_void_p(8)) == -1

    def normals(vertices=one, m=8, faces=one, f=4, ws=one, ws_bytes=big, fn=one, area=one, vn=one):
        return lib.mvsn_mesh_normals(vertices, m, faces, f, ws, ws_bytes, fn, area, vn, None)
    assert normals(vertices=None) == -1 and b"mvsn_mesh_normals" in lib.mvsn_last_error()
    assert normals(vn=None) == -1 and normals(ws=None) == -1 and normals(m=0) == -1 and normals(f=-1) == -1
    assert normals(faces=None) == -1 and normals(fn=None) == -1 and normals(area=None) == -1
    assert normals(m=2 ** 31) == -2 and normals(f=2 ** 31) == -2
    assert normals(ws_bytes=8) == -3 and normals(ws=ctypes.c_void_p(8)) == -1
