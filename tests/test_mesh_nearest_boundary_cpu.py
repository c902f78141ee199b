"""mesh_sample, mesh_nearest and mesh_metrics without a GPU: host-side validation (everything is rejected before any
launch), CPU tensors, the answers that need no launch, and the new entries in the header, the binding, the build and the
binary."""
import ctypes
import os
import re

import pytest
import torch

from multi_view_stereonet_amd import _native, build, mesh, metrics
from multi_view_stereonet_amd.mesh import MeshNearest, MeshSamples, mesh_nearest, mesh_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvsn_mesh_sample_workspace_bytes", "mvsn_mesh_sample_prefix", "mvsn_mesh_sample_draw",
           "mvsn_mesh_nearest_box_cells", "mvsn_mesh_nearest_workspace_bytes", "mvsn_mesh_nearest_count",
           "mvsn_mesh_nearest_build", "mvsn_mesh_nearest")
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
    (([[0, 0, 0]], faces(), 4), {}, "vertices"), ((torch.zeros(M, 2), faces(), 4), {}, "vertices"),
    ((torch.zeros(M, 3, dtype=torch.float64), faces(), 4), {}, "vertices"),
    ((verts(), torch.zeros((2, 3), dtype=torch.int32), 4), {}, "faces"), ((verts(), torch.zeros((2, 4), dtype=torch.int64), 4), {}, "faces"),
    ((verts(), faces(device="meta"), 4), {}, "faces are on"),
    ((verts(), torch.zeros((2 ** 31, 3), dtype=torch.int64, device="meta"), 4), {}, r"2\^31 - 1"),
    ((verts(), faces(), -1), {}, "n must be"), ((verts(), faces(), 2.5), {}, "n must be"), ((verts(), faces(), True), {}, "n must be"),
    ((verts(), faces(), None), {}, "n must be"), ((verts(), faces(), 2 ** 31), {}, r"2\^31 - 1"),
    ((verts(), faces(), 4), dict(seed=-1), "seed"), ((verts(), faces(), 4), dict(seed=2 ** 64), "seed"),
    ((verts(), faces(), 4), dict(seed=1.0), "seed"), ((verts(), faces(), 4), dict(seed=True), "seed"),
    ((verts(), faces(), 4), dict(normals=torch.zeros(M + 1, 3)), "normals"),
    ((verts(), faces(), 4), dict(normals=torch.zeros(M, 3, dtype=torch.float64)), "normals"),
    ((verts(), faces(), 4), dict(normals=torch.zeros(M, 3, device="meta")), "normals are on"),
    ((verts(), faces(), 4), dict(colors=torch.zeros(M, 3)), "colors"),
    ((verts(), faces(), 4), dict(colors=torch.zeros(M, 4, dtype=torch.uint8)), "colors"),
    ((verts(), faces(), 4), dict(colors=torch.zeros(M, 3, dtype=torch.uint8, device="meta")), "colors are on"),
    ((verts(), torch.zeros((0, 3), dtype=torch.int64), 4), {}, "the mesh has no area"),
    ((torch.zeros((0, 3)), faces(), 4), {}, "the mesh has no area"),
])
def test_mesh_sample_arguments_are_validated_before_any_launch(no_launch, args, kw, match):
    with pytest.raises(ValueError, match=match):
        mesh_sample(*args, **kw)


@pytest.mark.parametrize("args, match", [
    (([[0, 0, 0]], verts(), faces(), 1.0), "points"), ((torch.zeros(5, 2), verts(), faces(), 1.0), "points"),
    ((torch.zeros(5, 3, dtype=torch.float64), verts(), faces(), 1.0), "points must be float32"),
    ((torch.zeros(5, 3), torch.zeros(M, 3, dtype=torch.float16), faces(), 1.0), "vertices"),
    ((torch.zeros(5, 3), verts(), torch.zeros((2, 3)), 1.0), "faces"),
    ((torch.zeros(5, 3), verts(), faces(device="meta"), 1.0), "faces are on"),
    ((torch.zeros(5, 3, device="meta"), verts(), faces(), 1.0), "points are on"),
    ((torch.zeros(5, 3), verts(), faces(), 0.0), "max_dist"), ((torch.zeros(5, 3), verts(), faces(), -1.0), "max_dist"),
    ((torch.zeros(5, 3), verts(), faces(), float("nan")), "max_dist"), ((torch.zeros(5, 3), verts(), faces(), float("inf")), "max_dist"),
    ((torch.zeros(5, 3), verts(), faces(), 1e-30), "max_dist"), ((torch.zeros(5, 3), verts(), faces(), 1e30), "max_dist"),
    ((torch.zeros(5, 3), verts(), faces(), "near"), "max_dist"),
])
def test_mesh_nearest_arguments_are_validated_before_any_launch(no_launch, args, match):
    with pytest.raises(ValueError, match=match):
        mesh_nearest(*args)


@pytest.mark.parametrize("kw, match", [
    (dict(truth=torch.zeros(5, 2)), "truth"), (dict(threshold=0.0), "threshold"), (dict(threshold=0.2, max_dist=0.1), "must not be below"),
    (dict(samples=0), "samples"), (dict(samples=2.5), "samples"), (dict(samples=True), "samples"),
    (dict(truth=torch.zeros(5, 3, device="meta")), "one device"), (dict(vertices=torch.zeros(M, 2)), "vertices"),
    (dict(faces=torch.zeros((2, 3), dtype=torch.int32)), "faces"), (dict(seed=-1), "seed"),
])
def test_mesh_metrics_arguments_are_validated_before_any_launch(no_launch, kw, match):
    a = dict(vertices=verts(), faces=faces(), truth=torch.zeros(5, 3), threshold=0.1, samples=16)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        metrics.mesh_metrics(a.pop("vertices"), a.pop("faces"), a.pop("truth"), a.pop("threshold"), **a)


def test_cpu_tensors_raise_the_usual_runtime_error(no_launch):
    with pytest.raises(RuntimeError, match="HIP devices only"):
        mesh_sample(verts(), faces(), 4)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        mesh_sample(verts(), faces(), 4, normals=torch.zeros(M, 3), colors=torch.zeros(M, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        mesh_nearest(torch.zeros(5, 3), verts(), faces(), 1.0)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        metrics.mesh_metrics(verts(), faces(), torch.zeros(5, 3), 0.1, samples=16)
    # the text is mesh_components' own
    with pytest.raises(RuntimeError) as theirs:
        mesh.mesh_components(faces(), M)
    assert "(there is no CPU implementation)" in str(theirs.value)


def test_no_samples_come_without_a_launch(no_launch):
    for kw in (dict(), dict(normals=torch.zeros(M, 3)), dict(colors=torch.zeros(M, 3, dtype=torch.uint8))):
        got = mesh_sample(verts(), faces(), 0, **kw)
        assert isinstance(got, MeshSamples)
        assert got.points.shape == got.weights.shape == (0, 3) and got.face.shape == (0,)
        assert got.points.dtype == got.weights.dtype == torch.float32 and got.face.dtype == torch.int64
        assert (got.normals is None) == ("normals" not in kw) and (got.colors is None) == ("colors" not in kw)
    both = mesh_sample(verts(), faces(), 0, normals=torch.zeros(M, 3), colors=torch.zeros(M, 3, dtype=torch.uint8))
    assert both.normals.shape == both.colors.shape == (0, 3) and both.colors.dtype == torch.uint8
    # no samples of a mesh without faces is still no samples
    assert mesh_sample(verts(), torch.zeros((0, 3), dtype=torch.int64), 0).points.shape == (0, 3)


@pytest.mark.parametrize("n, v, f", [(0, verts(), faces()), (5, verts(), torch.zeros((0, 3), dtype=torch.int64)),
                                     (5, torch.zeros((0, 3)), faces()), (0, torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int64))])
def test_empty_inputs_give_the_all_miss_answer_without_a_launch(no_launch, n, v, f):
    got = mesh_nearest(torch.zeros(n, 3), v, f, 1.0)
    assert isinstance(got, MeshNearest)
    assert got.dist2.tolist() == [float("inf")] * n and got.face.tolist() == [-1] * n and got.within.tolist() == [0] * n
    assert got.point.shape == got.weights.shape == (n, 3) and not got.point.any() and not got.weights.any()
    assert (got.dist2.dtype, got.face.dtype, got.point.dtype, got.weights.dtype, got.within.dtype) == \
        (torch.float32, torch.int64, torch.float32, torch.float32, torch.int32)


def test_entries_in_header_binding_build_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_mesh_sample.hip") == 1 and build.SOURCES.count("mvsn_mesh_nearest.hip") == 1
    for name in ("mvsn_cloud.h", "mvsn_voxel.h", "mvsn_geom.h", "mvsn_common.h"):      # what the two files include
        assert build.HEADERS.count(name) == 1
    for s in ("mvsn_mesh_sample.hip", "mvsn_mesh_nearest.hip"):
        with open(os.path.join(build.CSRC, s)) as f:
            included = set(re.findall(r'#include "(mvsn_\w+\.h)"', f.read()))
        assert included and included <= set(build.HEADERS), s
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SIGNATURES
    assert re.search(r"#define\s+MVSN_MESH_NEAREST_BOX_CELLS\s+%d\b" % mesh.NEAREST_BOX_CELLS, header)
    assert re.search(r"#define\s+MVSN_MESH_NEAREST_STATUS_RANGE\s+%d\b" % mesh.MESH_NEAREST_STATUS_RANGE, header)
    assert re.search(r"#define\s+MVSN_MESH_SAMPLE_STATUS_NO_AREA\s+%d\b" % mesh.MESH_SAMPLE_STATUS_NO_AREA, header)
    lib = ctypes.CDLL(_native.library_path())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert _native.load().mvsn_mesh_nearest_box_cells() == mesh.NEAREST_BOX_CELLS == 512
    size = _native.load().mvsn_mesh_sample_workspace_bytes
    assert size(0) == 0 and size(-1) == 0 and size(2 ** 31) == 0 and size(1) > 0 and size(1) % 256 == 0
    # 8 bytes per face, 16 per 256 faces, a head, every section on a 256-byte boundary
    assert 8 * 1027 + 16 * 5 + 32 <= size(1027) <= 8 * 1027 + 16 * 5 + 32 + 5 * 256
    top = size(2 ** 31 - 1)
    assert 8 * (2 ** 31 - 1) + 16 * 2 ** 23 <= top <= 8 * (2 ** 31 - 1) + 16 * 2 ** 23 + 32 + 5 * 256
    size = _native.load().mvsn_mesh_nearest_workspace_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(2 ** 31, 0) == 0 and size(0, 2 ** 31) == 0
    assert size(0, 0) > 0 and size(0, 0) % 256 == 0 and size(0, 0) == size(512, 0) - 2048 < size(513, 0)
    # 20 bytes per slot (1024 slots up to 512 pairs, then the power of two >= 2 pairs), 4 per pair and per large face
    assert 20 * 2048 + 4 * 1000 + 4 * 7 <= size(1000, 7) <= 20 * 2048 + 4 * 1000 + 4 * 7 + 24 + 16 + 10 * 256
    assert size(2 ** 31 - 1, 2 ** 31 - 1) >= 20 * 2 ** 31 + 8 * (2 ** 31 - 1)


def test_c_entries_check_their_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    big = 1 << 24

    def prefix(vertices=one, m=8, faces=one, f=4, result=one, ws=one, ws_bytes=big):
        return lib.mvsn_mesh_sample_prefix(vertices, m, faces, f, result, ws, ws_bytes, None)
    assert prefix(vertices=None) == -1 and b"mvsn_mesh_sample_prefix" in lib.mvsn_last_error()
    assert prefix(faces=None) == -1 and prefix(result=None) == -1 and prefix(m=0) == -1 and prefix(f=0) == -1
    assert prefix(m=2 ** 31) == -2 and prefix(f=2 ** 31) == -2
    assert prefix(ws=None) == -3 and prefix(ws_bytes=8) == -3 and prefix(ws=ctypes.c_void_p(8)) == -1

    def draw(vertices=one, m=8, faces=one, f=4, ws=one, ws_bytes=big, n=5, normals=None, colors=None, points=one,
             face=one, weights=one, out_normals=None, out_colors=None):
        return lib.mvsn_mesh_sample_draw(vertices, m, faces, f, ws, ws_bytes, n, 0, normals, colors, points, face, weights,
                                         out_normals, out_colors, None)
    assert draw(vertices=None) == -1 and b"mvsn_mesh_sample_draw" in lib.mvsn_last_error()
    assert draw(faces=None) == -1 and draw(points=None) == -1 and draw(face=None) == -1 and draw(weights=None) == -1
    assert draw(n=0) == -1 and draw(n=-1) == -1 and draw(n=2 ** 31) == -2 and draw(m=2 ** 31) == -2 and draw(f=0) == -1
    assert draw(ws=None) == -3 and draw(ws_bytes=8) == -3
    assert draw(normals=one) == -1 and draw(out_normals=one) == -1 and draw(colors=one) == -1 and draw(out_colors=one) == -1

    def count(vertices=one, m=8, faces=one, f=4, inv=1.0, result=one):
        return lib.mvsn_mesh_nearest_count(vertices, m, faces, f, inv, result, None)
    assert count(vertices=None) == -1 and b"mvsn_mesh_nearest_count" in lib.mvsn_last_error()
    assert count(faces=None) == -1 and count(result=None) == -1 and count(m=0) == -1 and count(f=0) == -1
    assert count(m=2 ** 31) == -2 and count(f=2 ** 31) == -2
    assert count(inv=0.0) == -1 and count(inv=float("inf")) == -1 and count(inv=float("nan")) == -1

    def built(vertices=one, m=8, faces=one, f=4, inv=1.0, pairs=10, large=1, ws=one, ws_bytes=big):
        return lib.mvsn_mesh_nearest_build(vertices, m, faces, f, inv, pairs, large, ws, ws_bytes, None)
    assert built(vertices=None) == -1 and b"mvsn_mesh_nearest_build" in lib.mvsn_last_error()
    assert built(faces=None) == -1 and built(m=0) == -1 and built(f=2 ** 31) == -2 and built(inv=-1.0) == -1
    assert built(pairs=-1) == -1 and built(large=-1) == -1 and built(pairs=2 ** 31) == -2 and built(large=2 ** 31) == -2
    assert built(ws=None) == -3 and built(ws_bytes=8) == -3 and built(ws=ctypes.c_void_p(8)) == -1

    def nearest(query=one, nq=5, vertices=one, m=8, faces=one, f=4, inv=1.0, r2=1.0, pairs=10, large=1, ws=one,
                ws_bytes=big, dist2=one, within=one):
        return lib.mvsn_mesh_nearest(query, nq, vertices, m, faces, f, inv, r2, pairs, large, ws, ws_bytes, dist2, one, one,
                                     one, within, None)
    assert nearest(query=None) == -1 and b"mvsn_mesh_nearest" in lib.mvsn_last_error()
    assert nearest(dist2=None) == -1 and nearest(within=None) == -1 and nearest(vertices=None) == -1 and nearest(faces=None) == -1
    assert nearest(nq=0) == -1 and nearest(nq=2 ** 31) == -2 and nearest(m=0) == -1 and nearest(f=2 ** 31) == -2
    assert nearest(inv=0.0) == -1 and nearest(r2=0.0) == -1 and nearest(r2=float("inf")) == -1
    assert nearest(pairs=-1) == -1 and nearest(pairs=2 ** 31) == -2 and nearest(ws=None) == -3 and nearest(ws_bytes=8) == -3
