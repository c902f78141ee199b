"""The mesh components and the mesh filter on the device (csrc/mvsn_mesh.hip) against the numpy restatement
(tests/mesh_reference.py), exactly: every output is integers or copied bits.  Inputs sit in poisoned buffers, the
workspace and every output between guard bands, under both poisons."""
import functools

import numpy as np
import pytest
import torch

from guarded_alloc import POISON_FINITE, POISON_NAN, Guard, bits_equal
from mesh_reference import (SPHERES, SPHERES_F, SPHERES_FACE_COUNT, SPHERES_FIRST, SPHERES_M, SPHERES_VERTEX_COUNT, cases,
                            components_reference, filter_reference, keep_reference, spheres_mesh, spheres_state)
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd.mesh import MeshComponents, filter_mesh, mesh_components
from multi_view_stereonet_amd.tsdf import TSDFMesh, TSDFVolume
from tsdf_reference import mesh_topology

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COMPONENT_KEYS = ("vertex_label", "face_label", "vertex_count", "face_count", "first")
MESH_KEYS = ("vertices", "normals", "colors", "faces", "cell")
POISONS = pytest.mark.parametrize("fill", [POISON_NAN, POISON_FINITE], ids=["nan", "finite"])


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The restatement's components of a case: computed once, shared, never modified."""
    faces, m = cases()[name]
    ref = components_reference(faces, m)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _spheres_reference():
    ref = components_reference(spheres_mesh()["faces"], SPHERES_M)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _device_components(faces_np, m, fill=POISON_NAN):
    """mvsn_mesh_components_label + _emit on faces in a poisoned buffer of their own, the workspace, the head and every
    output between guard bands: a dict of numpy arrays like components_reference's."""
    f = int(faces_np.shape[0])
    guard = Guard(_alloc, fill)
    faces = guard.poisoned(torch.from_numpy(np.array(faces_np)).to(DEV))
    lib = _native.load()
    ws_bytes = lib.mvsn_mesh_workspace_bytes(m, f)
    assert ws_bytes > 0
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    head = guard.empty((2,), torch.int64, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_components_label(_native.ptr(faces) if f else None, m, f, _native.ptr(head),
                                                     _native.ptr(ws), ws_bytes, st), "mvsn_mesh_components_label")
        c, status = head.tolist()
        assert status == 0 and 1 <= c <= m, (c, status)
        out = {"vertex_label": guard.empty((m,), torch.int64, DEV), "face_label": guard.empty((f,), torch.int64, DEV),
               "vertex_count": guard.empty((c,), torch.int64, DEV), "face_count": guard.empty((c,), torch.int64, DEV),
               "first": guard.empty((c,), torch.int64, DEV)}
        _native.check(lib.mvsn_mesh_components_emit(
            _native.ptr(faces) if f else None, m, f, _native.ptr(ws), ws_bytes, c, _native.ptr(out["vertex_label"]),
            _native.ptr(out["face_label"]) if f else None, _native.ptr(out["vertex_count"]),
            _native.ptr(out["face_count"]), _native.ptr(out["first"]), st), "mvsn_mesh_components_emit")
    torch.cuda.synchronize()
    guard.check()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_components(got, ref, what=""):
    for key in COMPONENT_KEYS:
        assert got[key].shape == ref[key].shape and got[key].dtype == np.int64, (what, key, got[key].shape, ref[key].shape)
        np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")


@POISONS
@pytest.mark.parametrize("name", sorted(cases()))
def test_components_match_the_restatement(name, fill):
    faces, m = cases()[name]
    got = _device_components(faces, m, fill)
    ref = _reference(name)
    print(f"{name}: M {m}, F {faces.shape[0]}, C {ref['first'].shape[0]}, largest component "
          f"{int(ref['vertex_count'].max())} vertices")
    _assert_components(got, ref, name)


@pytest.mark.parametrize("name", ["grid_256_permuted", "face_validity", "many_small"])
def test_the_order_of_faces_and_of_their_indices_does_not_show(name):
    faces, m = cases()[name]
    rng = np.random.default_rng(21)
    order = rng.permutation(faces.shape[0])
    first = _device_components(faces, m)
    again = _device_components(faces, m)
    shuffled = _device_components(faces[order], m)
    rotated = _device_components(np.roll(faces, 1, axis=1), m)
    _assert_components(first, _reference(name), name)
    for key in COMPONENT_KEYS:                                   # two runs of one input: the same bits everywhere
        assert first[key].tobytes() == again[key].tobytes(), key
    for other in (shuffled, rotated):
        for key in ("vertex_label", "vertex_count", "face_count", "first"):
            assert other[key].tobytes() == first[key].tobytes(), key
    undone = np.empty_like(shuffled["face_label"])
    undone[order] = shuffled["face_label"]
    np.testing.assert_array_equal(undone, first["face_label"])
    # a face's label is that of its first index; a rotation names another one of the same component, or a bad index still
    np.testing.assert_array_equal(rotated["face_label"], first["face_label"])


def test_the_public_entry_gives_the_same_components():
    for name in ("no_faces", "face_validity", "strip_permuted", "many_small"):
        faces, m = cases()[name]
        comp = mesh_components(torch.from_numpy(np.array(faces)).to(DEV), m)
        assert isinstance(comp, MeshComponents) and all(t.dtype == torch.int64 and t.device == DEV for t in comp)
        _assert_components({k: getattr(comp, k).cpu().numpy() for k in COMPONENT_KEYS}, _reference(name), name)
    # a view of a wider tensor: the rows are made dense before the launch
    faces, m = cases()["many_small"]
    wide = torch.from_numpy(np.concatenate([faces, faces[:, :1]], 1)).to(DEV)
    comp = mesh_components(wide[:, :3], m)
    _assert_components({k: getattr(comp, k).cpu().numpy() for k in COMPONENT_KEYS}, _reference("many_small"), "view")
    empty = mesh_components(torch.zeros((2, 3), dtype=torch.int64, device=DEV), 0)
    assert empty.first.shape == (0,) and empty.face_label.tolist() == [-1, -1] and empty.face_label.device == DEV


# ---- filter_mesh on the fixture: two spheres and a speck -------------------------------------------------------------
def _device_filter(mesh, comp, keep, fill=POISON_NAN):
    """mvsn_mesh_select + mvsn_mesh_compact on inputs in poisoned buffers, the workspace, the head and every output between
    guard bands: a dict like filter_reference's."""
    m, f, c = mesh["vertices"].shape[0], mesh["faces"].shape[0], comp["first"].shape[0]
    guard = Guard(_alloc, fill)
    put = lambda a: guard.poisoned(torch.from_numpy(np.array(a)).to(DEV))   # noqa: E731
    vertices, normals, cell, faces = put(mesh["vertices"]), put(mesh["normals"]), put(mesh["cell"]), put(mesh["faces"])
    colors = put(mesh["colors"]) if mesh["colors"] is not None else None
    vertex_label, face_label = put(comp["vertex_label"]), put(comp["face_label"])
    keep_d = put(np.asarray(keep, bool).astype(np.uint8))
    lib = _native.load()
    ws_bytes = lib.mvsn_mesh_workspace_bytes(m, f)
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    head = guard.empty((2,), torch.int64, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_select(_native.ptr(vertex_label), _native.ptr(face_label), _native.ptr(keep_d), m, f, c,
                                           _native.ptr(head), _native.ptr(ws), ws_bytes, st), "mvsn_mesh_select")
        mo, both = head.tolist()
        fo = both - mo
        assert 0 <= mo <= m and 0 <= fo <= f, (mo, both)
        out = {"vertices": guard.empty((mo, 3), torch.float32, DEV), "normals": guard.empty((mo, 3), torch.float32, DEV),
               "colors": guard.empty((mo, 3), torch.uint8, DEV) if colors is not None else None,
               "cell": guard.empty((mo,), torch.int64, DEV), "faces": guard.empty((fo, 3), torch.int64, DEV),
               "vertex_rows": guard.empty((mo,), torch.int64, DEV), "face_rows": guard.empty((fo,), torch.int64, DEV)}
        _native.check(lib.mvsn_mesh_compact(
            _native.ptr(vertices), _native.ptr(normals), _native.ptr(colors), _native.ptr(cell), _native.ptr(faces),
            _native.ptr(face_label), _native.ptr(keep_d), m, f, c, _native.ptr(ws), ws_bytes, mo, fo,
            _native.ptr(out["vertices"]) if mo else None, _native.ptr(out["normals"]) if mo else None,
            _native.ptr(out["colors"]) if mo and colors is not None else None, _native.ptr(out["cell"]) if mo else None,
            _native.ptr(out["faces"]) if fo else None, _native.ptr(out["vertex_rows"]) if mo else None,
            _native.ptr(out["face_rows"]) if fo else None, st), "mvsn_mesh_compact")
    torch.cuda.synchronize()
    guard.check()
    return {k: v.cpu().numpy() if v is not None else None for k, v in out.items()}


def _assert_filtered(got, ref, what=""):
    for key in MESH_KEYS + ("vertex_rows", "face_rows"):
        if ref[key] is None:
            assert got[key] is None, (what, key)
            continue
        assert got[key].shape == ref[key].shape and got[key].dtype == ref[key].dtype, (what, key, got[key].shape, ref[key].shape)
        assert got[key].tobytes() == ref[key].tobytes(), (what, key)            # the bits, NaN payloads included


def _plain(mesh, color):
    return dict(mesh, colors=mesh["colors"] if color else None)


@POISONS
@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
def test_select_and_compact_match_the_restatement(color, fill):
    mesh, comp = _plain(spheres_mesh(), color), _spheres_reference()
    for keep in ([True, True, False], [True, False, False], [False, False, True], [False, True, True], [False] * 3, [True] * 3):
        got = _device_filter(mesh, comp, keep, fill)
        _assert_filtered(got, filter_reference(mesh, comp, keep), str(keep))
    # faces that take no part are dropped, and a vertex of a dropped component is never a row: the validity case with
    # made-up vertex data whose bits say where they came from (every word a NaN with a payload of its own)
    faces, m = cases()["face_validity"]
    words = (np.arange(6 * m, dtype=np.uint32) * np.uint32(2654435761) | np.uint32(0x7f800001)).view(np.float32)
    odd = {"vertices": words[:3 * m].reshape(m, 3), "normals": words[3 * m:].reshape(m, 3),
           "colors": (np.arange(3 * m) % 251).astype(np.uint8).reshape(m, 3) if color else None, "faces": np.array(faces),
           "cell": np.arange(m, dtype=np.int64) * 7 + 3}
    ref = _reference("face_validity")
    for keep in ([True, False, True, False], [False, True, False, True], [True] * 4):
        _assert_filtered(_device_filter(odd, ref, keep, fill), filter_reference(odd, ref, keep), f"validity {keep}")


def _upload(mesh):
    to = lambda a: torch.from_numpy(np.array(a)).to(DEV) if a is not None else None   # noqa: E731
    return TSDFMesh(to(mesh["vertices"]), to(mesh["normals"]), to(mesh["colors"]), to(mesh["faces"]), to(mesh["cell"]))


def _download(filtered):
    out = {k: getattr(filtered.mesh, k) for k in MESH_KEYS}
    out.update(vertex_rows=filtered.vertex_rows, face_rows=filtered.face_rows)
    return {k: v.cpu().numpy() if v is not None else None for k, v in out.items()}


@pytest.mark.parametrize("color", [True, False], ids=["colour", "plain"])
def test_filter_mesh_on_two_spheres_and_a_speck(color):
    host = _plain(spheres_mesh(), color)
    ref = _spheres_reference()
    mesh = _upload(host)
    comp = mesh_components(mesh.faces, SPHERES_M)
    _assert_components({k: getattr(comp, k).cpu().numpy() for k in COMPONENT_KEYS}, ref, "fixture")
    assert comp.vertex_count.tolist() == SPHERES_VERTEX_COUNT and comp.face_count.tolist() == SPHERES_FACE_COUNT
    assert comp.first.tolist() == SPHERES_FIRST

    spheres = filter_mesh(mesh, min_faces=61)                     # the two spheres
    _assert_filtered(_download(spheres), filter_reference(host, ref, [True, True, False]), "min_faces=61")
    _assert_components({k: getattr(spheres.components, k).cpu().numpy() for k in COMPONENT_KEYS}, ref, "computed")
    assert spheres.mesh.vertices.shape[0] == 730 + 318 and spheres.mesh.faces.shape[0] == 1456 + 632
    by_vertices = filter_mesh(mesh, min_vertices=33, components=comp)
    for a, b in zip(_download(by_vertices).values(), _download(spheres).values()):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    assert by_vertices.components is comp

    largest = filter_mesh(mesh, keep_largest=1, components=comp)
    assert largest.mesh.vertices.shape == (730, 3) and largest.mesh.faces.shape == (1456, 3)
    _assert_filtered(_download(largest), filter_reference(host, ref, keep_reference(ref, keep_largest=1)), "keep_largest=1")
    both = filter_mesh(mesh, min_faces=61, min_vertices=33, keep_largest=2, components=comp)
    _assert_filtered(_download(both), filter_reference(host, ref, [True, True, False]), "all three rules")

    speck = filter_mesh(mesh, keep=torch.tensor([False, False, True], device=DEV), components=comp)
    _assert_filtered(_download(speck), filter_reference(host, ref, [False, False, True]), "keep: the speck")
    assert speck.vertex_rows[0].item() == SPHERES_FIRST[2] and speck.mesh.vertices.shape[0] == 32
    second = filter_mesh(mesh, keep=torch.tensor([False, True, False], device=DEV))
    # each sphere, and the speck, alone: a closed surface of Euler characteristic 2
    for part in (largest, second, speck):
        closed, euler, boundary = mesh_topology(part.mesh.faces.cpu().numpy(), part.mesh.vertices.shape[0])
        assert closed and euler == 2 and boundary == 0, (closed, euler, boundary)

    for nothing in (filter_mesh(mesh, min_faces=2000, components=comp), filter_mesh(mesh, keep_largest=0, components=comp),
                    filter_mesh(mesh, keep=torch.zeros(3, dtype=torch.bool, device=DEV), components=comp)):
        _assert_filtered(_download(nothing), filter_reference(host, ref, [False] * 3), "nothing kept")
        assert nothing.mesh.vertices.shape == (0, 3) and nothing.mesh.faces.shape == (0, 3) and nothing.mesh.vertices.device == DEV
        assert (nothing.mesh.colors is None) != color
    everything = filter_mesh(mesh, min_faces=0, components=comp)
    for key in MESH_KEYS:                                        # keeping all gives the input's bits
        a, b = getattr(everything.mesh, key), getattr(mesh, key)
        assert (a is None and b is None) or bits_equal(a, b), key
    assert everything.vertex_rows.tolist() == list(range(SPHERES_M)) and everything.face_rows.tolist() == list(range(SPHERES_F))
    with pytest.raises(ValueError, match=r"keep must be a \(3,\)"):      # (the length is known once the mesh is labelled)
        filter_mesh(mesh, keep=torch.ones(4, dtype=torch.bool, device=DEV))


def test_volume_to_clean_mesh_end_to_end():
    s, w, c = spheres_state()
    vol = TSDFVolume(SPHERES["dims"], SPHERES["voxel_size"], SPHERES["origin"], 0.3, device=DEV, color=True)
    vol.sdf_sum.copy_(torch.from_numpy(s))
    vol.weight.copy_(torch.from_numpy(w))
    vol.color_sum.copy_(torch.from_numpy(c))
    mesh = vol.extract_mesh()
    clean = filter_mesh(mesh, min_faces=100)
    # the restatement applied to the device's own mesh
    host = {k: getattr(mesh, k).cpu().numpy() for k in MESH_KEYS}
    ref = components_reference(host["faces"], host["vertices"].shape[0])
    assert host["vertices"].shape[0] == SPHERES_M and host["faces"].shape[0] == SPHERES_F
    assert ref["vertex_count"].tolist() == SPHERES_VERTEX_COUNT and ref["face_count"].tolist() == SPHERES_FACE_COUNT
    _assert_components({k: getattr(clean.components, k).cpu().numpy() for k in COMPONENT_KEYS}, ref, "end to end")
    _assert_filtered(_download(clean), filter_reference(host, ref, keep_reference(ref, min_faces=100)), "end to end")
    assert clean.mesh.vertices.shape[0] == 730 + 318 and clean.mesh.colors is not None
    closed, euler, boundary = mesh_topology(clean.mesh.faces.cpu().numpy(), clean.mesh.vertices.shape[0])
    assert closed and euler == 4 and boundary == 0               # two spheres
