"""mesh_edges, mesh_smooth and mesh_normals on the device (csrc/mvsn_mesh_edges.hip, csrc/mvsn_mesh_smooth.hip) against
the numpy restatement (tests/mesh_smooth_reference.py).  Every case goes through the C ABI with the inputs in poisoned
buffers of their own and the workspace and every output between guard bands, under both poisons.  The sums are integers
and every fp64 step of the restatement is one numpy operation: every output is compared byte for byte and no tolerance
applies anywhere."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_smooth_reference as sr
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd.fusion import write_ply
from multi_view_stereonet_amd.mesh import (SMOOTH_METHODS, MeshEdges, MeshNormals, SimplifiedMesh, SmoothedMesh, mesh_edges,
                                           mesh_normals, mesh_render, mesh_simplify, mesh_smooth)
from multi_view_stereonet_amd.tsdf import TSDFVolume

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = list(sr.SMOOTH_CASES)
EDGE_TYPES = (torch.int64, torch.int64, torch.int32, torch.int32, torch.int64, torch.int32, torch.bool)


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _numpy(out):
    return {k: t.cpu().numpy() for k, t in out.items()}


def _edges(faces, m, fill=POISON_NAN):
    """mvsn_mesh_edges_mark and _emit: numpy arrays of the outputs."""
    f = len(faces)
    if f == 0 or m == 0:                                             # no launch: the library refuses the sizes
        return _numpy(mesh_edges(_to(faces), m)._asdict())
    guard = Guard(_alloc, fill)
    fc = guard.poisoned(_to(faces))
    lib = _native.load()
    ws_bytes = lib.mvsn_mesh_edges_workspace_bytes(m, f)
    assert ws_bytes > 0
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    head = guard.empty((2,), torch.int64, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_edges_mark(_native.ptr(fc), m, f, _native.ptr(head), _native.ptr(ws), ws_bytes, st),
                      "mvsn_mesh_edges_mark")
        e, status = head.tolist()
        assert status == 0 and 0 <= e <= 3 * f
        shapes = ((e, 2), (e,), (e,), (e,), (f, 3), (m,), (m,))
        out = {k: guard.empty(shape, dtype, DEV) for k, shape, dtype in zip(sr.EDGE_OUTPUTS, shapes, EDGE_TYPES)}
        p = {k: _native.ptr(t) if t.numel() else None for k, t in out.items()}
        _native.check(lib.mvsn_mesh_edges_emit(m, f, _native.ptr(ws), ws_bytes, e, p["edges"], p["first"], p["face_count"],
                                               p["winding"], p["face_edge"], p["vertex_degree"], p["vertex_boundary"], st),
                      "mvsn_mesh_edges_emit")
    torch.cuda.synchronize()
    guard.check()
    return _numpy(out)


def _smooth(V, edges, held, iterations, method="taubin", lam=sr.LAM, mu=sr.MU, fill=POISON_NAN):
    """mvsn_mesh_smooth: the output vertices as a numpy array."""
    m, e = len(V), len(edges)
    guard = Guard(_alloc, fill)
    v = guard.poisoned(_to(V))
    ed = guard.poisoned(_to(edges)) if e else None
    pin = guard.poisoned(_to(held)) if held is not None else None
    lib = _native.load()
    ws_bytes = lib.mvsn_mesh_smooth_workspace_bytes(m)
    assert ws_bytes > 0
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    out = guard.empty((m, 3), torch.float32, DEV)
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_mesh_smooth(_native.ptr(v), m, _native.ptr(ed), e, _native.ptr(pin), SMOOTH_METHODS[method],
                                           iterations, lam, mu, _native.ptr(ws), ws_bytes, _native.ptr(out), _native.stream()),
                      "mvsn_mesh_smooth")
    torch.cuda.synchronize()
    guard.check()
    return out.cpu().numpy()


def _normals(V, faces, fill=POISON_NAN):
    """mvsn_mesh_normals: numpy arrays of the outputs."""
    m, f = len(V), len(faces)
    guard = Guard(_alloc, fill)
    v = guard.poisoned(_to(V))
    fc = guard.poisoned(_to(faces)) if f else None
    lib = _native.load()
    ws_bytes = lib.mvsn_mesh_normals_workspace_bytes(m)
    assert ws_bytes > 0
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    out = {"face_normals": guard.empty((f, 3), torch.float32, DEV), "face_area": guard.empty((f,), torch.float32, DEV),
           "vertex_normals": guard.empty((m, 3), torch.float32, DEV)}
    p = {k: _native.ptr(t) if t.numel() else None for k, t in out.items()}
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_mesh_normals(_native.ptr(v), m, _native.ptr(fc), f, _native.ptr(ws), ws_bytes, p["face_normals"],
                                            p["face_area"], p["vertex_normals"], _native.stream()), "mvsn_mesh_normals")
    torch.cuda.synchronize()
    guard.check()
    return _numpy(out)


def _run(V, faces, configs, fill=POISON_NAN):
    """All three calls on one mesh: {edges, normals, smooth: {label: vertices}}, the smoothing over the device's edges."""
    m = len(V)
    edges = _edges(faces, m, fill)
    smooth = {}
    for label, kw in configs:
        kw = dict(kw)
        fix, pinned = kw.pop("fix_boundary", False), kw.pop("pinned", None)
        held = sr.held_mask(m, edges["vertex_boundary"], fix, pinned) if fix or pinned is not None else None
        smooth[label] = _smooth(V, edges["edges"], held, fill=fill, **kw)
    return {"edges": edges, "normals": _normals(V, faces, fill), "smooth": smooth}


@functools.lru_cache(maxsize=None)
def _device(name, fill=POISON_NAN):
    """Made once per (case, poison), never modified."""
    c = sr.smooth_case(name)
    return _run(c["vertices"], c["faces"], c["configs"], fill)


def _same_bits(a, b, keys=None):
    for key in keys if keys is not None else b:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


def _same_run(a, b):
    _same_bits(a["edges"], b["edges"], sr.EDGE_OUTPUTS)
    _same_bits(a["normals"], b["normals"], sr.NORMAL_OUTPUTS)
    assert list(a["smooth"]) == list(b["smooth"])
    _same_bits(a["smooth"], b["smooth"])


@pytest.mark.parametrize("name", CASES)
def test_cases_match_the_restatement_byte_for_byte(name):
    _same_run(_device(name), sr.smooth_case_reference(name))


@pytest.mark.parametrize("name", CASES)
def test_buffers_under_both_poisons(name):
    # (the guard bands of every buffer are checked inside the calls; an element nobody writes, or a read of foreign
    # memory or of the uninitialised workspace that reaches a result, differs between the two fills)
    _same_run(_device(name, POISON_NAN), _device(name, POISON_FINITE))


@pytest.mark.parametrize("name", ["three_on_edge", "nonfinite_in_fans", "fan_300", "grid_17", "icosphere"])
def test_calling_twice_gives_the_same_bytes(name):
    c = sr.smooth_case(name)
    _same_run(_run(c["vertices"], c["faces"], c["configs"]), _device(name))


@pytest.mark.parametrize("name", ["two_triangles", "three_on_edge", "nonfinite_in_fans", "fan_300", "grid_17", "icosphere"])
def test_the_order_of_the_faces_and_of_their_corners_does_not_show(name):
    c, plain = sr.smooth_case(name), _device(name)
    rng = np.random.default_rng(11)
    F = c["faces"][rng.permutation(c["faces"].shape[0])]
    F = np.stack([np.roll(face, k) for face, k in zip(F, rng.integers(0, 3, F.shape[0]))])
    got = _run(c["vertices"], F, c["configs"])
    _same_bits(got["smooth"], plain["smooth"])
    _same_bits(got["normals"], plain["normals"], ["vertex_normals"])
    _same_bits(got["edges"], plain["edges"], ["vertex_degree", "vertex_boundary"])
    _same_bits(got["edges"], sr.edges_reference(F, c["vertices"].shape[0]), sr.EDGE_OUTPUTS)
    pairs = lambda r: sorted(zip(map(tuple, r["edges"].tolist()), r["face_count"].tolist(), r["winding"].tolist()))   # noqa: E731
    assert pairs(got["edges"]) == pairs(plain["edges"])


def _fields(t):
    return {k: v.cpu().numpy() for k, v in t._asdict().items()}


def test_the_python_calls_are_the_library_calls():
    for name in ("out_of_range", "no_faces", "coincident", "nonfinite_in_fans", "grid_17", "icosphere"):
        c, ref = sr.smooth_case(name), sr.smooth_case_reference(name)
        v, f = _to(c["vertices"]), _to(c["faces"])
        edges = mesh_edges(f, v.shape[0])
        assert isinstance(edges, MeshEdges) and MeshEdges._fields == sr.EDGE_OUTPUTS and edges.edges.device == DEV
        _same_bits(_fields(edges), ref["edges"], sr.EDGE_OUTPUTS)
        normals = mesh_normals(v, f)
        assert isinstance(normals, MeshNormals) and MeshNormals._fields == sr.NORMAL_OUTPUTS
        _same_bits(_fields(normals), ref["normals"], sr.NORMAL_OUTPUTS)
        for label, kw in c["configs"]:
            kw = {k: _to(x) if isinstance(x, np.ndarray) else x for k, x in kw.items()}
            got = mesh_smooth(v, f, **kw)                             # edges= left out: mesh_smooth finds them
            assert isinstance(got, SmoothedMesh) and got.vertices.device == DEV and got.vertices.data_ptr() != v.data_ptr()
            assert got.vertices.cpu().numpy().tobytes() == ref["smooth"][label].tobytes(), (name, label)
            _same_bits(_fields(got.edges), ref["edges"], sr.EDGE_OUTPUTS)
            again = mesh_smooth(v, f, edges=edges, **kw)              # and with them: the same bytes, the same object
            assert torch.equal(again.vertices.view(torch.int32), got.vertices.view(torch.int32)) and again.edges is edges
    v, f = _to(sr.smooth_case("grid_17")["vertices"]), _to(sr.smooth_case("grid_17")["faces"])
    sliced = torch.stack([v, v], dim=1)[:, 0]                         # not contiguous
    assert torch.equal(mesh_smooth(sliced, f, 2).vertices, mesh_smooth(v, f, 2).vertices)
    assert torch.equal(mesh_normals(sliced, f).vertex_normals, mesh_normals(v, f).vertex_normals)


def _sphere_depth(K, T, centre, radius, size, noise, seed):
    """z-depth maps (V,1,H,W) of a sphere seen from cameras (K, T_cam_in_world), NaN off the sphere, with Gaussian noise."""
    H, W = size
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    maps = []
    for k, t in zip(K, T):
        d = np.stack([(u - k[0, 2]) / k[0, 0], (v - k[1, 2]) / k[1, 1], np.ones_like(u)], axis=-1)   # z = 1 along the ray
        c = np.linalg.inv(t) @ np.append(centre, 1.0)
        dd, dc = (d * d).sum(-1), d @ c[:3]
        disc = dc * dc - dd * (c[:3] @ c[:3] - radius * radius)
        z = np.where(disc > 0, (dc - np.sqrt(np.maximum(disc, 0))) / dd, np.nan)
        maps.append(z + noise * rng.standard_normal(z.shape))
    return np.stack(maps)[:, None].astype(np.float32)


def test_a_noisy_tsdf_sphere_end_to_end(tmp_path):
    dims, voxel, origin = (32, 32, 32), 0.1, (-1.6, -1.6, 2.0)
    centre, radius = np.array([-0.03, 0.02, 3.57]), 1.0
    K = np.array([[90.0, 0, 48, 0], [0, 90.0, 48, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    T = []
    for angle in np.arange(6) * np.pi / 3:                            # six cameras on a circle round the sphere, looking in
        R = np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = R, centre - R @ np.array([0.0, 0.0, 3.5])
        T.append(pose)
    K, T = np.stack([K] * 6), np.stack(T)
    depth = _sphere_depth(K, T, centre, radius, (96, 96), 0.03, seed=7)
    vol = TSDFVolume(dims, voxel, origin, 0.3, device=DEV)
    vol.integrate(torch.from_numpy(np.nan_to_num(depth, nan=0.0)).to(DEV), torch.from_numpy(K).float().to(DEV),
                  torch.from_numpy(T).float().to(DEV))
    mesh = vol.extract_mesh()
    m, f = mesh.vertices.shape[0], mesh.faces.shape[0]
    assert m > 1000 and f > 2000
    edges = mesh_edges(mesh.faces, m)
    assert (edges.winding[edges.face_count == 2] == 0).all()          # extract_mesh winds every face one way
    smooth = mesh_smooth(mesh.vertices, mesh.faces, 10, edges=edges)
    assert isinstance(smooth, SmoothedMesh) and smooth.edges is edges and smooth.vertices.shape == (m, 3)
    off = lambda v: (torch.linalg.norm(v.double().cpu() - torch.from_numpy(centre), dim=1) - radius).square().mean().sqrt()   # noqa: E731
    before, after = float(off(mesh.vertices)), float(off(smooth.vertices))
    print(f"sphere: M {m}, F {f}, E {edges.edges.shape[0]}, border edges {int((edges.face_count == 1).sum())}; rms distance "
          f"to the sphere {before / voxel:.4f} -> {after / voxel:.4f} voxels")
    assert after < before
    normals = mesh_normals(smooth.vertices, mesh.faces)
    assert isinstance(normals, MeshNormals) and normals.vertex_normals.shape == (m, 3)
    outwards = (normals.vertex_normals.double().cpu() * (smooth.vertices.double().cpu() - torch.from_numpy(centre))).sum(dim=1)
    used = (edges.vertex_degree > 0).cpu()                            # (a cell at the rim of what was seen can have no quad)
    assert used.sum() > 0.9 * m and (outwards[used] > 0).all()        # extract_mesh winds its faces outwards
    assert (normals.vertex_normals[~used.to(DEV)] == 0).all()
    small = mesh_simplify(smooth.vertices, mesh.faces, 2 * voxel, origin=origin, normals=normals.vertex_normals)
    assert isinstance(small, SimplifiedMesh) and 0 < small.faces.shape[0] < f and small.normals.dtype == torch.float32
    view = mesh_render(smooth.vertices, mesh.faces, torch.from_numpy(K[:1]).float().to(DEV),
                       torch.from_numpy(T[:1]).float().to(DEV), (96, 96), normals=normals.vertex_normals)
    assert view.depth.dtype == torch.float32 and int((view.face[0] >= 0).sum()) > 1000 and view.normals is not None
    path = os.path.join(tmp_path, "smooth.ply")
    write_ply(path, smooth.vertices, normals=normals.vertex_normals, faces=mesh.faces)
    assert os.path.getsize(path) > m * 24 + f * 13
