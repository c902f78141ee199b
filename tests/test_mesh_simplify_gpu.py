"""mesh_simplify on the device (csrc/mvsn_mesh_simplify.hip) against the numpy restatement
(tests/mesh_simplify_reference.py).  Every case goes through the C ABI with the inputs in poisoned buffers of their own
and the workspace and every output between guard bands, under both poisons.  The sums are integers, the face set is
integer work and every fp64 step of the restatement is one numpy operation: every output is compared byte for byte and
no tolerance applies anywhere."""
import functools

import numpy as np
import pytest
import torch

import mesh_simplify_reference as ms
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd.fusion import voxel_merge
from multi_view_stereonet_amd.mesh import (SIMPLIFY_PLACEMENTS, SimplifiedMesh, mesh_nearest, mesh_render, mesh_sample,
                                           mesh_simplify)
from multi_view_stereonet_amd.tsdf import TSDFVolume
from tsdf_reference import voxel_centres

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = list(ms.SIMPLIFY_CASES)


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _simplify(c, placement, fill=POISON_NAN, faces=None):
    """mvsn_mesh_simplify_assign, _mark and _emit: numpy arrays of the outputs, and clusters, status and fallbacks."""
    V, Fc = c["vertices"], c["faces"] if faces is None else faces
    m, f = len(V), len(Fc)
    guard = Guard(_alloc, fill)
    v, fc = guard.poisoned(_to(V)), guard.poisoned(_to(Fc)) if f else None
    nor = guard.poisoned(_to(c["normals"])) if c["normals"] is not None else None
    col = guard.poisoned(_to(c["colors"])) if c["colors"] is not None else None
    size = np.float32(c["voxel_size"])
    o = np.asarray(c["origin"], np.float64).astype(np.float32)
    scalars = (float(size), float(np.float32(1) / size), float(o[0]), float(o[1]), float(o[2]))
    lib = _native.load()
    ws_bytes = lib.mvsn_mesh_simplify_workspace_bytes(m, f)
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    head = guard.empty((4,), torch.int64, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_simplify_assign(_native.ptr(v), m, *scalars, _native.ptr(head), _native.ptr(ws), ws_bytes,
                                                    st), "mvsn_mesh_simplify_assign")
        clusters, status = head[:2].tolist()
        assert status == 0 and 0 < clusters <= m
        _native.check(lib.mvsn_mesh_simplify_mark(_native.ptr(v), _native.ptr(nor), _native.ptr(col), m, _native.ptr(fc), f,
                                                  *scalars, SIMPLIFY_PLACEMENTS[placement], int(c["drop"]), clusters,
                                                  _native.ptr(head), _native.ptr(ws), ws_bytes, st), "mvsn_mesh_simplify_mark")
        mo, fo, status, fallbacks = head.tolist()
        assert 0 <= mo <= clusters and 0 <= fo <= f
        out = {"vertices": guard.empty((mo, 3), torch.float32, DEV), "faces": guard.empty((fo, 3), torch.int64, DEV),
               "normals": guard.empty((mo, 3), torch.float32, DEV) if nor is not None else None,
               "colors": guard.empty((mo, 3), torch.uint8, DEV) if col is not None else None,
               "count": guard.empty((mo,), torch.int32, DEV), "first": guard.empty((mo,), torch.int64, DEV),
               "inverse": guard.empty((m,), torch.int64, DEV), "face_rows": guard.empty((fo,), torch.int64, DEV)}
        p = {k: _native.ptr(t) if t is not None and t.numel() else None for k, t in out.items()}
        _native.check(lib.mvsn_mesh_simplify_emit(_native.ptr(fc), m, f, clusters, _native.ptr(ws), ws_bytes, mo, fo,
                                                  p["vertices"], p["faces"], p["normals"], p["colors"], p["count"], p["first"],
                                                  p["inverse"], p["face_rows"], st), "mvsn_mesh_simplify_emit")
    torch.cuda.synchronize()
    guard.check()
    got = {k: t.cpu().numpy() if t is not None else None for k, t in out.items()}
    got.update(clusters=clusters, status=status, fallbacks=fallbacks)
    return got


@functools.lru_cache(maxsize=None)
def _device(name, placement, fill=POISON_NAN):
    """Made once per (case, placement, poison), never modified."""
    return _simplify(ms.simplify_case(name), placement, fill)


def _same_bits(a, b, keys=ms.OUTPUTS):
    for key in keys:
        if b[key] is None:
            assert a[key] is None, key
            continue
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("placement", ms.PLACEMENTS)
@pytest.mark.parametrize("name", CASES)
def test_cases_match_the_restatement_byte_for_byte(name, placement):
    got, ref = _device(name, placement), ms.simplify_case_reference(name, placement)
    assert (got["clusters"], got["status"], got["fallbacks"]) == (ref["clusters"], 0, ref["fallbacks"])
    _same_bits(got, ref)


@pytest.mark.parametrize("placement", ms.PLACEMENTS)
@pytest.mark.parametrize("name", CASES)
def test_buffers_under_both_poisons(name, placement):
    # (the guard bands of every buffer are checked inside _simplify; an element nobody writes, or a read of foreign
    # memory or of the uninitialised workspace that reaches a result, differs between the two fills)
    a, b = _device(name, placement, POISON_NAN), _device(name, placement, POISON_FINITE)
    assert (a["clusters"], a["status"], a["fallbacks"]) == (b["clusters"], b["status"], b["fallbacks"])
    _same_bits(a, b)


@pytest.mark.parametrize("name", ["plane_3", "many_equal", "soup_coarse_1", "nonfinite"])
def test_calling_twice_gives_the_same_bytes(name):
    _same_bits(_simplify(ms.simplify_case(name), "quadric"), _device(name, "quadric"))


@pytest.mark.parametrize("placement", ms.PLACEMENTS)
@pytest.mark.parametrize("name", ["plane_3", "crease", "duplicates", "many_equal", "soup_coarse_2"])
def test_the_order_of_the_faces_does_not_show(name, placement):
    c, plain = ms.simplify_case(name), _device(name, placement)
    perm = np.random.default_rng(21).permutation(len(c["faces"]))
    got = _simplify(c, placement, faces=c["faces"][perm])
    _same_bits(got, plain, ms.VERTEX_OUTPUTS)
    _same_bits(got, ms.simplify_reference(c["vertices"], c["faces"][perm], c["voxel_size"], c["origin"], placement, c["normals"],
                                          c["colors"], c["drop"]))
    triples = lambda r: {tuple(t) for t in ms.canonical(r["faces"]).tolist()}   # noqa: E731
    assert triples(got) == triples(plain)
    if name in ("plane_3", "crease"):                                # no two faces alike: the very same rows survive
        assert sorted(perm[got["face_rows"]].tolist()) == plain["face_rows"].tolist()


def test_many_equal_faces_in_one_wave_leave_the_lowest_row():
    got, c = _device("many_equal", "quadric"), ms.simplify_case("many_equal")
    tri = [3, 11, 19]
    rows = [r for r, face in enumerate(c["faces"].tolist()) if sorted(face) == tri]
    assert len(rows) == 204 and rows[0] == 7                         # 140 of one winding (two rotations), 64 of the other
    kept = [r for r in got["face_rows"].tolist() if r in rows]
    assert kept == [7, rows[140]]


@pytest.mark.parametrize("name", ["plane_3", "cube_origin", "nonfinite", "loose_vertices_keep", "soup_1"])
def test_mean_placement_without_dropping_is_voxel_merge_bit_for_bit(name):
    c = ms.simplify_case(name)
    v, f = _to(c["vertices"]), _to(c["faces"])
    col = _to(c["colors"]) if c["colors"] is not None else None
    got = mesh_simplify(v, f, c["voxel_size"], origin=c["origin"], placement="mean", colors=col, drop_unreferenced=False)
    vc = voxel_merge(v, c["voxel_size"], colors=col, origin=c["origin"])
    for mine, theirs in ((got.vertices, vc.points), (got.colors, vc.colors), (got.count, vc.count), (got.first, vc.first),
                         (got.inverse, vc.inverse)):
        assert (mine is None and theirs is None) or (mine.dtype == theirs.dtype and torch.equal(mine, theirs))
    assert got.vertices.cpu().numpy().tobytes() == vc.points.cpu().numpy().tobytes()


def test_the_python_call_is_the_library_call():
    for name, placement in (("cube_origin", "quadric"), ("soup_coarse_1", "mean"), ("plane_3_bare", "quadric"),
                            ("no_faces_keep", "quadric"), ("fallback", "quadric")):
        c = ms.simplify_case(name)
        tensor = lambda a: _to(a) if a is not None else None          # noqa: E731
        got = mesh_simplify(_to(c["vertices"]), _to(c["faces"]), c["voxel_size"], origin=c["origin"], placement=placement,
                            normals=tensor(c["normals"]), colors=tensor(c["colors"]), drop_unreferenced=c["drop"])
        assert isinstance(got, SimplifiedMesh) and SimplifiedMesh._fields == ms.OUTPUTS
        _same_bits({k: getattr(got, k).cpu().numpy() if getattr(got, k) is not None else None for k in ms.OUTPUTS},
                   ms.simplify_case_reference(name, placement))
    c = ms.simplify_case("plane_one_cell")                            # every face collapses: empties, on the device
    got = mesh_simplify(_to(c["vertices"]), _to(c["faces"]), c["voxel_size"], origin=c["origin"])
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.vertices.device == DEV
    assert got.inverse.tolist() == [-1] * 289
    nan = torch.full((5, 3), float("nan"), device=DEV)                # every vertex dropped
    got = mesh_simplify(nan, _to(np.array([[0, 1, 2]])), 0.5, drop_unreferenced=False)
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.inverse.tolist() == [-1] * 5
    with pytest.raises(ValueError, match="voxel_size too small for the mesh's extent"):
        mesh_simplify(_to(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)), _to(np.array([[0, 1, 2]])), 2.0 ** -21)


def _holes(hit):
    """misses that no path of misses joins to the border of the picture"""
    reach = np.zeros_like(hit)
    reach[0], reach[-1], reach[:, 0], reach[:, -1] = ~hit[0], ~hit[-1], ~hit[:, 0], ~hit[:, -1]
    for _ in range(hit.size):
        grown = reach.copy()
        grown[1:] |= reach[:-1]
        grown[:-1] |= reach[1:]
        grown[:, 1:] |= reach[:, :-1]
        grown[:, :-1] |= reach[:, 1:]
        grown &= ~hit
        if (grown == reach).all():
            break
        reach = grown
    return int((~hit & ~reach).sum())


def test_a_tsdf_sphere_end_to_end():
    dims, voxel, origin = (32, 32, 32), 0.1, (-1.6, -1.6, 2.0)
    cx, cy, cz = voxel_centres(dims, voxel, origin)
    pz, py, px = np.meshgrid(cz, cy, cx, indexing="ij")
    field = np.sqrt((px + 0.03) ** 2 + (py - 0.02) ** 2 + (pz - 3.57) ** 2) - 1.0
    vol = TSDFVolume(dims, voxel, origin, 0.3, device=DEV)
    vol.sdf_sum.copy_(torch.from_numpy(np.clip(field, -0.3, 0.3).astype(np.float32)))
    vol.weight.fill_(1.0)
    mesh = vol.extract_mesh()
    small = mesh_simplify(mesh.vertices, mesh.faces, 3 * voxel, origin=origin, normals=mesh.normals)
    assert 0 < small.faces.shape[0] < mesh.faces.shape[0] // 4 and 0 < small.vertices.shape[0] < mesh.vertices.shape[0] // 4
    K = torch.tensor([[[60.0, 0, 32, 0], [0, 60.0, 24, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], device=DEV)
    T = torch.eye(4, device=DEV)[None]
    full = (mesh_render(mesh.vertices, mesh.faces, K, T, (48, 64)).face[0] >= 0).cpu().numpy()
    less = (mesh_render(small.vertices, small.faces, K, T, (48, 64)).face[0] >= 0).cpu().numpy()
    assert full.sum() > 600 and _holes(full) == 0
    assert _holes(less) == 0 and less.sum() > 0.85 * full.sum()
    # every output vertex lies in its members' cell, so no vertex moved by the cell's diagonal
    diagonal = float(np.sqrt(3.0) * np.float32(3 * voxel))
    samples = mesh_sample(small.vertices, small.faces, 4000, seed=5)
    near = mesh_nearest(samples.points, mesh.vertices, mesh.faces, diagonal)
    worst = float(near.dist2.max().sqrt())
    print(f"sphere: {tuple(mesh.vertices.shape)} {tuple(mesh.faces.shape)} -> {tuple(small.vertices.shape)} "
          f"{tuple(small.faces.shape)}, farthest sample {worst / voxel:.3f} voxels, diagonal {diagonal / voxel:.3f}")
    assert (near.face >= 0).all() and worst < diagonal
