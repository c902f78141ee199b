"""The numpy restatement of the mesh components (tests/mesh_reference.py) against hand-worked meshes, against scipy's
connected components, under permutations of the faces and of their indices, and on the fixture "two spheres and a
speck".  The import of multi_view_stereonet_amd.mesh pins the restatement to the module it restates."""
import numpy as np
import pytest

from mesh_reference import (SPHERES_F, SPHERES_FACE_COUNT, SPHERES_FIRST, SPHERES_M, SPHERES_VERTEX_COUNT, cases,
                            components_reference, filter_reference, keep_reference, spheres_mesh)
from multi_view_stereonet_amd.mesh import FilteredMesh, MeshComponents
from tsdf_reference import mesh_topology


def test_result_types_name_the_fields_of_the_restatement():
    assert MeshComponents._fields == ("vertex_label", "face_label", "vertex_count", "face_count", "first")
    assert FilteredMesh._fields == ("mesh", "vertex_rows", "face_rows", "components")
    assert set(components_reference(np.zeros((0, 3), np.int64), 2)) == set(MeshComponents._fields)


def test_hand_worked_meshes():
    c = cases()
    got = components_reference(*c["no_faces"])
    assert got["vertex_label"].tolist() == [0, 1, 2, 3, 4] and got["face_label"].shape == (0,)
    assert got["vertex_count"].tolist() == [1] * 5 and got["face_count"].tolist() == [0] * 5
    assert got["first"].tolist() == [0, 1, 2, 3, 4]
    got = components_reference(*c["one_triangle"])
    assert got["vertex_label"].tolist() == [0, 0, 0] and got["face_label"].tolist() == [0]
    assert got["vertex_count"].tolist() == [3] and got["face_count"].tolist() == [1] and got["first"].tolist() == [0]
    got = components_reference(*c["two_fans_one_vertex"])
    assert got["first"].tolist() == [0] and got["vertex_count"].tolist() == [9] and got["face_count"].tolist() == [6]
    got = components_reference(*c["coincident_positions"])
    assert got["vertex_label"].tolist() == [0, 0, 0, 1, 1, 1] and got["face_label"].tolist() == [0, 1]
    assert got["first"].tolist() == [0, 3]
    got = components_reference(*c["face_validity"])
    assert got["vertex_label"].tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 3]
    assert got["face_label"].tolist() == [0, -1, 1, -1, -1, 1, 1, 1, 1, -1, -1, 0, -1]
    assert got["vertex_count"].tolist() == [3, 4, 1, 1] and got["face_count"].tolist() == [2, 5, 0, 0]
    assert got["first"].tolist() == [0, 3, 7, 8]
    for name in ("strip_ascending", "strip_descending", "strip_permuted", "star_on_last_row", "star_on_row_0"):
        faces, m = c[name]
        got = components_reference(faces, m)
        assert got["first"].tolist() == [0] and got["vertex_count"].tolist() == [m], name
        assert got["face_count"].tolist() == [faces.shape[0]], name
    got = components_reference(*c["many_small"])
    assert got["first"].shape == (1400,) and sorted(set(got["vertex_count"].tolist())) == [1, 3]
    assert int(got["face_count"].sum()) == 700 and (got["face_count"] == (got["vertex_count"] == 3)).all()
    faces, m = c["grid_256_permuted"]
    assert (m, faces.shape[0]) == (65686, 130100)
    got = components_reference(faces, m)
    assert sorted(got["vertex_count"].tolist()) == [3] * 50 + [65536]
    assert sorted(got["face_count"].tolist()) == [1] * 50 + [130050]


@pytest.mark.parametrize("name", sorted(cases()))
def test_against_scipy(name):
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    faces, m = cases()[name]
    ref = components_reference(faces, m)
    good = faces[((faces >= 0) & (faces < m)).all(1)]
    u = np.concatenate([good[:, 0], good[:, 1], good[:, 2]])
    v = np.concatenate([good[:, 1], good[:, 2], good[:, 0]])
    graph = sparse.coo_matrix((np.ones(u.shape[0], np.int8), (u, v)), shape=(m, m))
    n, label = connected_components(graph, directed=False)
    assert n == ref["first"].shape[0]
    # the same partition: scipy's label of a component's lowest row names the component
    assert (label[ref["first"]][ref["vertex_label"]] == label).all()
    assert np.unique(label[ref["first"]]).shape[0] == n
    assert (np.diff(ref["first"]) > 0).all()
    for i in range(min(n, 60)):
        assert ref["first"][i] == np.nonzero(ref["vertex_label"] == i)[0][0]


@pytest.mark.parametrize("name", ["face_validity", "many_small", "strip_permuted", "two_fans_one_vertex"])
def test_the_order_of_faces_and_of_their_indices_does_not_show(name):
    faces, m = cases()[name]
    ref = components_reference(faces, m)
    rng = np.random.default_rng(5)
    order = rng.permutation(faces.shape[0])
    shuffled = components_reference(faces[order], m)
    rolled = components_reference(np.roll(faces, 1, axis=1), m)
    flipped = components_reference(faces[:, ::-1], m)
    for other in (shuffled, rolled, flipped):
        for key in ("vertex_label", "vertex_count", "face_count", "first"):
            np.testing.assert_array_equal(other[key], ref[key], err_msg=key)
    np.testing.assert_array_equal(shuffled["face_label"], ref["face_label"][order])
    np.testing.assert_array_equal(rolled["face_label"], ref["face_label"])
    np.testing.assert_array_equal(flipped["face_label"], ref["face_label"])


def test_two_spheres_and_a_speck():
    mesh = spheres_mesh()
    assert mesh["vertices"].shape == (SPHERES_M, 3) and mesh["faces"].shape == (SPHERES_F, 3)
    comp = components_reference(mesh["faces"], SPHERES_M)
    assert comp["vertex_count"].tolist() == SPHERES_VERTEX_COUNT
    assert comp["face_count"].tolist() == SPHERES_FACE_COUNT
    assert comp["first"].tolist() == SPHERES_FIRST
    assert (comp["face_label"] >= 0).all()
    # the rules of filter_mesh on it
    assert keep_reference(comp, min_faces=61).tolist() == [True, True, False]
    assert keep_reference(comp, min_vertices=33).tolist() == [True, True, False]
    assert keep_reference(comp, keep_largest=1).tolist() == [True, False, False]
    assert keep_reference(comp, min_faces=61, keep_largest=5).tolist() == [True, True, False]
    assert keep_reference(comp, min_faces=2000).tolist() == [False, False, False]
    assert keep_reference(comp, keep_largest=0).tolist() == [False, False, False]
    # every component alone is a closed surface of Euler characteristic 2, and the gather renumbers its faces
    for i in range(3):
        part = filter_reference(mesh, comp, np.arange(3) == i)
        assert part["vertices"].shape[0] == SPHERES_VERTEX_COUNT[i] and part["faces"].shape[0] == SPHERES_FACE_COUNT[i]
        assert part["faces"].min() == 0 and part["faces"].max() == SPHERES_VERTEX_COUNT[i] - 1
        np.testing.assert_array_equal(part["vertex_rows"][part["faces"]], mesh["faces"][part["face_rows"]])
        np.testing.assert_array_equal(part["vertices"], mesh["vertices"][part["vertex_rows"]])
        closed, euler, boundary = mesh_topology(part["faces"], part["vertices"].shape[0])
        assert closed and euler == 2 and boundary == 0
    whole = filter_reference(mesh, comp, np.ones(3, bool))
    for key in ("vertices", "normals", "colors", "cell", "faces"):
        assert whole[key].tobytes() == mesh[key].tobytes(), key
    none = filter_reference(mesh, comp, np.zeros(3, bool))
    assert none["vertices"].shape == (0, 3) and none["faces"].shape == (0, 3) and none["vertex_rows"].shape == (0,)


def test_ties_of_keep_largest_go_to_the_lower_id():
    comp = components_reference(*cases()["many_small"])
    keep = keep_reference(comp, keep_largest=3)
    triangles = np.nonzero(comp["face_count"] == 1)[0]
    assert np.nonzero(keep)[0].tolist() == triangles[:3].tolist()
