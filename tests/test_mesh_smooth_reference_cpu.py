"""The numpy restatement of mesh_edges, mesh_smooth and mesh_normals (tests/mesh_smooth_reference.py) held to
independent statements: a Python dict over the sides, Euler's formula, a dense float64 Laplacian iteration within the
bound DESIGN.md section 29 derives, and what smoothing and normals are for."""
import numpy as np
import pytest

import mesh_smooth_reference as sr

CASES = list(sr.SMOOTH_CASES)


def _edges_by_dict(faces, m):
    """{(low, high): [first side, count, winding]} in insertion order, which is the order of first."""
    table = {}
    for r, face in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if not all(0 <= v < m for v in face):
            continue
        for s in range(3):
            a, b = face[s], face[(s + 1) % 3]
            if a == b:
                continue
            entry = table.setdefault((min(a, b), max(a, b)), [3 * r + s, 0, 0])
            entry[1] += 1
            entry[2] += 1 if a < b else -1
    return table


@pytest.mark.parametrize("name", CASES)
def test_edges_against_a_dict_over_the_sides(name):
    c, ref = sr.smooth_case(name), sr.smooth_case_reference(name)["edges"]
    m, f = c["vertices"].shape[0], c["faces"].shape[0]
    table = _edges_by_dict(c["faces"], m)
    assert [tuple(e) for e in ref["edges"].tolist()] == list(table)
    assert ref["first"].tolist() == [v[0] for v in table.values()] == sorted(ref["first"].tolist())
    assert ref["face_count"].tolist() == [v[1] for v in table.values()]
    assert ref["winding"].tolist() == [v[2] for v in table.values()]
    rows = {e: i for i, e in enumerate(table)}
    for r, face in enumerate(c["faces"].tolist()):
        for s in range(3):
            a, b = face[s], face[(s + 1) % 3]
            takes_part = all(0 <= v < m for v in face) and a != b
            assert ref["face_edge"][r, s] == (rows[(min(a, b), max(a, b))] if takes_part else -1), (r, s)
    degree, border = [0] * m, [False] * m
    for (a, b), (_, count, _) in table.items():
        degree[a] += 1
        degree[b] += 1
        if count == 1:
            border[a] = border[b] = True
    assert ref["vertex_degree"].tolist() == degree and ref["vertex_boundary"].tolist() == border
    assert ref["face_edge"].shape == (f, 3) and ref["edges"].shape == (len(table), 2)
    for key, dtype in zip(sr.EDGE_OUTPUTS, (np.int64, np.int64, np.int32, np.int32, np.int64, np.int32, bool)):
        assert ref[key].dtype == dtype, key


def test_the_small_cases_are_what_their_names_say():
    e = lambda name: sr.smooth_case_reference(name)["edges"]         # noqa: E731
    assert e("one_triangle")["face_count"].tolist() == [1, 1, 1] and e("one_triangle")["vertex_boundary"].all()
    assert sorted(e("two_triangles")["face_count"].tolist()) == [1, 1, 1, 1, 2]
    shared = e("two_triangles")["face_count"] == 2
    assert e("two_triangles")["edges"][shared].tolist() == [[1, 2]] and e("two_triangles")["winding"][shared].tolist() == [0]
    three = e("three_on_edge")
    assert three["edges"][0].tolist() == [0, 1] and three["face_count"][0] == 3 and three["winding"][0] == 1
    twice = e("same_face_twice")                                     # (0,1,2) and its rotation (1,2,0): one winding
    assert twice["face_count"][:3].tolist() == [2, 3, 2] and twice["winding"][:3].tolist() == [2, 1, -2]
    opposite = e("opposite_winding")
    assert opposite["face_count"][:3].tolist() == [2, 3, 2] and opposite["winding"][:3].tolist() == [0, -1, 0]
    repeated = e("repeated_vertex")
    assert repeated["face_edge"][0].tolist() == [0, -1, 0] and repeated["face_edge"][2].tolist() == [-1, -1, -1]
    outside = e("out_of_range")
    assert (outside["face_edge"][[0, 1, 3]] == -1).all() and outside["edges"].tolist() == [[0, 1], [1, 2], [0, 2]]
    assert e("no_faces")["edges"].shape == (0, 2) and e("no_faces")["vertex_degree"].tolist() == [0, 0, 0]
    assert e("isolated_vertices")["vertex_degree"].tolist()[4:] == [0, 0, 0, 0]
    assert e("fan_300")["vertex_degree"][0] == 300 and e("fan_256_m257")["vertex_degree"].shape == (257,)
    g = e("grid_17")
    assert g["edges"].shape[0] == 2 * 16 * 17 + 256 and int((g["face_count"] == 1).sum()) == 64
    assert int(g["vertex_boundary"].sum()) == 64 and (g["winding"][g["face_count"] == 2] == 0).all()


@pytest.mark.parametrize("name", ["tetrahedron", "icosphere"])
def test_eulers_formula_on_the_closed_cases(name):
    c, ref = sr.smooth_case(name), sr.smooth_case_reference(name)["edges"]
    assert c["vertices"].shape[0] - ref["edges"].shape[0] + c["faces"].shape[0] == 2
    assert (ref["face_count"] == 2).all() and (ref["winding"] == 0).all() and not ref["vertex_boundary"].any()
    if name == "icosphere":
        assert c["faces"].shape[0] == 720 and c["vertices"].shape[0] == 362


def _dense_smooth(V, edges, held, factors):
    """(x (M,3) float64 by a dense Laplacian iteration, bound): the bound of DESIGN.md section 29 on the distance of the
    restatement from it.  Per step the quantised mean is off by at most step / 2 (every edge term by at most step / 2,
    and a mean of such terms by no more), an error e becomes at most (|1 - f| + |f|) e (the row sums of |I + f L|), and
    the fp64 operations of either side add at most (degree + 8) ulps of the largest coordinate; the output is rounded to
    fp32 once: 2^-24 of the largest coordinate."""
    m = V.shape[0]
    finite = np.isfinite(V).all(axis=1)
    x = np.where(finite[:, None], V.astype(np.float64), 0.0)
    L = np.zeros((m, m))
    for a, b in np.asarray(edges).tolist():
        if finite[a] and finite[b]:
            L[a, b] = L[b, a] = 1.0
    degree = L.sum(axis=1)
    moves = finite & ~held & (degree > 0)
    L[~moves] = 0.0
    L[moves] /= degree[moves][:, None]
    L[moves, moves] = -1.0
    _, step, _ = sr.smooth_step_size(V)
    bound, biggest = 0.0, np.abs(x).max()
    for f in factors:
        x = x + float(f) * (L @ x)
        biggest = max(biggest, np.abs(x).max())
        bound = (abs(1 - f) + abs(f)) * bound + abs(f) * step / 2 + (degree.max() + 8) * 2.0 ** -52 * biggest * (1 + abs(f))
    return x, bound + 2.0 ** -24 * biggest * (1 + 2.0 ** -20), finite


@pytest.mark.parametrize("name", ["two_triangles", "three_on_edge", "nonfinite_in_fans", "fan_300", "grid_17",
                                  "grid_17_offset_1e3", "icosphere"])
def test_smoothing_against_a_dense_float64_iteration_within_the_derived_bound(name):
    c, ref = sr.smooth_case(name), sr.smooth_case_reference(name)
    V, m = c["vertices"], c["vertices"].shape[0]
    for label, kw in c["configs"]:
        kw = dict(kw)
        held = sr.held_mask(m, ref["edges"]["vertex_boundary"], kw.pop("fix_boundary", False), kw.pop("pinned", None))
        factors = sr.smooth_factors(kw.pop("iterations"), kw.pop("method"), **kw)
        dense, bound, finite = _dense_smooth(V, ref["edges"]["edges"], held, factors)
        worst = np.abs(ref["smooth"][label].astype(np.float64) - dense)[finite].max()
        print(f"{name} {label}: farthest coordinate {worst:.3e}, bound {bound:.3e}")
        assert worst <= bound, (label, worst, bound)
        assert bound < 1e-4 * np.ptp(V[finite], axis=0).max() + 2.0 ** -23 * np.abs(V[finite]).max()   # (a bound that binds)


def test_a_plane_stays_a_plane():
    V, F = sr.grid(9, noise=0.0)
    V[:, 2] = np.float32(0.375)                                      # an axis plane: every z difference is exactly 0
    flat = sr.mesh_smooth_reference(V, F, 7)
    assert flat[:, 2].tobytes() == V[:, 2].tobytes() and not np.array_equal(flat, V)
    V[:, 2] = (0.25 * V[:, 0].astype(np.float64) + 0.5 * V[:, 1].astype(np.float64)).astype(np.float32)   # exact in fp32
    edges = sr.edges_reference(F, V.shape[0])
    for method in ("laplacian", "taubin"):
        out = sr.mesh_smooth_reference(V, F, 7, method).astype(np.float64)
        _, bound, _ = _dense_smooth(V, edges["edges"], np.zeros(V.shape[0], bool), sr.smooth_factors(7, method))
        off = np.abs(out[:, 2] - (0.25 * out[:, 0] + 0.5 * out[:, 1]))
        assert off.max() <= (1 + 0.25 + 0.5) * bound                 # every coordinate within `bound` of a point of the plane


def test_held_vertices_keep_their_bits():
    c, ref = sr.smooth_case("grid_17"), sr.smooth_case_reference("grid_17")
    V, border = c["vertices"], ref["edges"]["vertex_boundary"]
    configs = dict(c["configs"])
    pinned = configs["pinned"]["pinned"]
    same = lambda out, rows: out[rows].tobytes() == V[rows].tobytes()   # noqa: E731
    moved = lambda out, rows: (out[rows] != V[rows]).any(axis=1)        # noqa: E731
    assert same(ref["smooth"]["fix_boundary"], border) and moved(ref["smooth"]["fix_boundary"], ~border).all()
    assert same(ref["smooth"]["pinned"], pinned) and moved(ref["smooth"]["pinned"], ~pinned).all()
    assert same(ref["smooth"]["both_held"], border | pinned) and moved(ref["smooth"]["both_held"], ~(border | pinned)).all()
    assert moved(ref["smooth"]["taubin_5"], border).all()
    c, ref = sr.smooth_case("nonfinite_in_fans"), sr.smooth_case_reference("nonfinite_in_fans")
    bad = ~np.isfinite(c["vertices"]).all(axis=1)
    assert bad.sum() == 2
    for out in ref["smooth"].values():
        assert out[bad].tobytes() == c["vertices"][bad].tobytes() and np.isfinite(out[~bad]).all()
    # the hub at infinity contributes to no ring vertex: the ring moves as the ring alone would
    ring = np.arange(9, 15)
    alone = sr.smooth_reference(c["vertices"], np.stack([ring, np.roll(ring, -1)], axis=1), 5)
    assert ref["smooth"]["taubin_5"][ring].tobytes() == alone[ring].tobytes()


@pytest.mark.parametrize("name", ["coincident", "no_faces", "isolated_vertices"])
def test_what_cannot_move_keeps_its_bits(name):
    c, ref = sr.smooth_case(name), sr.smooth_case_reference(name)
    rows = slice(None) if name != "isolated_vertices" else slice(4, None)
    for out in ref["smooth"].values():
        assert out[rows].tobytes() == c["vertices"][rows].tobytes()
    for name in CASES:
        ref, V = sr.smooth_case_reference(name)["smooth"], sr.smooth_case(name)["vertices"]
        assert all(out.tobytes() == V.tobytes() for label, out in ref.items() if label.endswith("_0"))
    nan = np.full((4, 3), np.nan, np.float32)
    assert sr.mesh_smooth_reference(nan, [[0, 1, 2], [2, 1, 3]], 3).tobytes() == nan.tobytes()


@pytest.mark.parametrize("name", ["two_triangles", "three_on_edge", "nonfinite_in_fans", "fan_300", "grid_17", "icosphere"])
def test_the_order_of_the_faces_and_of_their_corners_does_not_show(name):
    c, ref = sr.smooth_case(name), sr.smooth_case_reference(name)
    rng = np.random.default_rng(11)
    F = c["faces"][rng.permutation(c["faces"].shape[0])]
    F = np.stack([np.roll(face, k) for face, k in zip(F, rng.integers(0, 3, F.shape[0]))])
    for label, kw in c["configs"]:
        assert sr.mesh_smooth_reference(c["vertices"], F, **kw).tobytes() == ref["smooth"][label].tobytes(), label
    assert sr.normals_reference(c["vertices"], F)["vertex_normals"].tobytes() == ref["normals"]["vertex_normals"].tobytes()


def _volume(V, F):
    P = V.astype(np.float64)[F]
    return np.einsum("ij,ij->i", P[:, 0], np.cross(P[:, 1], P[:, 2])).sum() / 6.0


def test_taubin_smooths_the_noisy_sphere_and_keeps_its_volume_better_than_laplacian():
    c = sr.smooth_case("icosphere")
    V, F = c["vertices"], c["faces"]
    radius_rms = lambda P: np.linalg.norm(P.astype(np.float64), axis=1).std()   # noqa: E731
    taubin = sr.mesh_smooth_reference(V, F, 5, "taubin")
    laplacian = sr.mesh_smooth_reference(V, F, 10, "laplacian")       # the same number of steps
    print(f"rms {radius_rms(V):.5f} -> taubin {radius_rms(taubin):.5f}, laplacian {radius_rms(laplacian):.5f}; "
          f"volume {_volume(V, F):.5f} -> {_volume(taubin, F):.5f}, {_volume(laplacian, F):.5f}")
    assert radius_rms(taubin) < radius_rms(V)
    assert abs(_volume(taubin, F) - _volume(V, F)) < abs(_volume(laplacian, F) - _volume(V, F))
    assert _volume(V, F) > 0                                          # wound outwards


@pytest.mark.parametrize("name", CASES)
def test_vertex_normals_within_the_derived_angle_of_the_float64_normal(name):
    """Every face's term is off by at most 1/2 per component in units where the vertex's largest component is at least
    2^30, so the integer sum S of n faces lies within sqrt(3) n / 2 of the scaled exact sum: the angle between them is
    at most asin(sqrt(3) n / (2 |S| - sqrt(3) n)).  Rounding the unit vector to fp32 turns it by at most sqrt(3) 2^-24;
    the fp64 operations of either side by far less than the 1e-12 allowed for them."""
    c, ref = sr.smooth_case(name), sr.smooth_case_reference(name)["normals"]
    V, F = c["vertices"], c["faces"]
    m = V.shape[0]
    ok, idx, cross, length = sr.face_cross(V, F)
    exact, faces_at = np.zeros((m, 3)), np.zeros(m, np.int64)
    P = V.astype(np.float64)
    for r in np.nonzero(ok)[0]:
        a, b, d = F[r]
        exact[[a, b, d]] += np.cross(P[b] - P[a], P[d] - P[a])
        faces_at[[a, b, d]] += 1
    sums = np.linalg.norm(sr.normal_sums(V, F).astype(np.float64), axis=1)
    assert (np.linalg.norm(ref["vertex_normals"], axis=1)[faces_at == 0] == 0).all()
    checked = 0
    for i in np.nonzero(faces_at)[0]:
        slack = np.sqrt(3.0) * faces_at[i]
        if sums[i] == 0:
            assert (ref["vertex_normals"][i] == 0).all()
            continue
        assert 2 * sums[i] > 2 * slack                               # (no case cancels that far)
        n64 = exact[i] / np.linalg.norm(exact[i])
        got = ref["vertex_normals"][i].astype(np.float64)
        angle = np.arctan2(np.linalg.norm(np.cross(n64, got)), n64 @ got)
        assert angle <= np.arcsin(slack / (2 * sums[i] - slack)) + np.sqrt(3.0) * 2.0 ** -24 + 1e-12, (i, angle)
        assert abs(np.linalg.norm(got) - 1) < 2.0 ** -22
        checked += 1
    assert checked or name in ("no_faces", "coincident")
    # face normals and areas: the float64 cross product's direction and half its length, zeros where there is none
    unit = np.where(ok[:, None], cross / np.where(ok, length, 1.0)[:, None], 0.0)
    assert np.abs(ref["face_normals"] - unit).max(initial=0.0) <= 2.0 ** -24
    assert np.allclose(ref["face_area"], np.where(ok, length / 2, 0.0), rtol=2.0 ** -23, atol=0.0)
    if name == "icosphere":                                          # wound outwards: so are the normals
        assert (np.einsum("ij,ij->i", ref["vertex_normals"], V) > 0.5 * np.linalg.norm(V, axis=1)).all()
