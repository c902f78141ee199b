"""The numpy restatement of mesh_simplify (tests/mesh_simplify_reference.py) against independent geometry and against
brute force: the clusters against a dict of cells, the faces against a Python set walked in row order, the invariances
the contract promises, and what the quadric is for (a plane stays a plane, a crease is found)."""
import numpy as np
import pytest

import mesh_simplify_reference as ms
import voxel_reference as vr

CASES = list(ms.SIMPLIFY_CASES)


def _ref(c, placement, **over):
    a = dict(vertices=c["vertices"], faces=c["faces"], voxel_size=c["voxel_size"], origin=c["origin"], placement=placement,
             normals=c["normals"], colors=c["colors"], drop_unreferenced=c["drop"])
    a.update(over)
    return ms.simplify_reference(**a)


def _brute(c):
    """(cluster of every vertex by first-seen order of a dict of cells, surviving rows and their cluster triples by a
    set of canonical triples walked in row order)"""
    kept, cell, _ = vr.cells_and_fractions(c["vertices"], c["voxel_size"], c["origin"])
    seen, cid = {}, []
    for i in range(len(kept)):
        cid.append(seen.setdefault(tuple(cell[i]), len(seen)) if kept[i] else -1)
    m, have, rows, tris = len(cid), set(), [], []
    for r, face in enumerate(c["faces"].tolist()):
        if any(not 0 <= i < m for i in face):
            continue
        g = [cid[i] for i in face]
        if min(g) < 0 or len(set(g)) < 3:
            continue
        k = g.index(min(g))
        key = (g[k], g[(k + 1) % 3], g[(k + 2) % 3])
        if key not in have:
            have.add(key)
            rows.append(r)
            tris.append(g)
    return np.array(cid, np.int64), rows, tris


@pytest.mark.parametrize("name", CASES)
def test_clusters_and_faces_equal_the_brute_force(name):
    c = ms.simplify_case(name)
    cid, rows, tris = _brute(c)
    ref = _ref(c, "mean", drop_unreferenced=False)
    assert ref["inverse"].tolist() == cid.tolist()                   # dense ids in first-seen order = ordered by `first`
    assert ref["face_rows"].tolist() == rows and ref["faces"].tolist() == tris
    assert ref["first"].tolist() == [int(np.nonzero(cid == k)[0][0]) for k in range(ref["clusters"])]
    assert ref["count"].tolist() == np.bincount(cid[cid >= 0], minlength=ref["clusters"]).tolist()
    dropped = _ref(c, "mean", drop_unreferenced=True)
    used = sorted({k for t in tris for k in t})
    assert dropped["first"].tolist() == ref["first"][used].tolist()
    renumber = {k: i for i, k in enumerate(used)}
    assert dropped["faces"].tolist() == [[renumber[k] for k in t] for t in tris]
    assert dropped["inverse"].tolist() == [renumber.get(k, -1) for k in cid.tolist()]


@pytest.mark.parametrize("placement", ms.PLACEMENTS)
@pytest.mark.parametrize("name", CASES)
def test_output_is_a_clean_mesh_inside_its_cells_and_simplifies_to_itself(name, placement):
    c, ref = ms.simplify_case(name), ms.simplify_case_reference(name, placement)
    faces, mo = ref["faces"], len(ref["vertices"])
    assert ((faces >= 0) & (faces < mo)).all()
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    assert len({tuple(t) for t in ms.canonical(faces).tolist()}) == len(faces)
    assert (np.diff(ref["first"]) > 0).all() and (np.diff(ref["face_rows"]) > 0).all()
    if c["drop"]:
        assert sorted(set(faces.reshape(-1).tolist())) == list(range(mo))
    inside, got = ms.cells(ref["vertices"], c["voxel_size"], c["origin"])
    assert inside.all() and (got == ref["cluster_cells"]).all()       # voxel_cell(output vertex) is its cluster's cell
    again = ms.simplify_reference(ref["vertices"], faces, c["voxel_size"], c["origin"], placement,
                                  drop_unreferenced=c["drop"])
    assert len(again["vertices"]) == mo and len(again["faces"]) == len(faces)
    assert again["inverse"].tolist() == list(range(mo)) and again["faces"].tolist() == faces.tolist()
    # every vertex moved by less than the cell's diagonal: members and output share the cell (whose faces the grid's
    # fp32 arithmetic places to a few steps of the coordinates)
    member = c["vertices"][ref["first"]].astype(np.float64)
    steps = 8 * float(np.spacing(np.float32(np.abs(c["vertices"][np.isfinite(c["vertices"])]).max())))
    assert (np.linalg.norm(ref["vertices"].astype(np.float64) - member, axis=1) <= np.sqrt(3.0) * c["voxel_size"] + steps).all()


@pytest.mark.parametrize("placement", ms.PLACEMENTS)
@pytest.mark.parametrize("name", ["plane_3", "crease", "duplicates", "bad_faces", "nonfinite", "many_equal", "soup_coarse_1"])
def test_face_order_and_corner_rotation_do_not_show(name, placement):
    c, ref = ms.simplify_case(name), ms.simplify_case_reference(name, placement)
    perm = np.random.default_rng(3).permutation(len(c["faces"]))
    got = _ref(c, placement, faces=c["faces"][perm])
    for key in ms.VERTEX_OUTPUTS:
        assert (ref[key] is None and got[key] is None) or ref[key].tobytes() == got[key].tobytes(), key
    assert {tuple(t) for t in ms.canonical(got["faces"]).tolist()} == {tuple(t) for t in ms.canonical(ref["faces"]).tolist()}
    if name in ("plane_3", "crease"):                                # no two faces alike: the very same rows survive
        assert sorted(perm[got["face_rows"]].tolist()) == ref["face_rows"].tolist()
    turn = np.random.default_rng(4).integers(0, 3, len(c["faces"]))
    turned = np.stack([np.roll(f, -k) for f, k in zip(c["faces"], turn)]) if len(turn) else c["faces"]
    got = _ref(c, placement, faces=turned)
    for key in ms.VERTEX_OUTPUTS + ("face_rows",):
        assert (ref[key] is None and got[key] is None) or ref[key].tobytes() == got[key].tobytes(), key
    assert got["faces"].tolist() == [np.roll(f, -k).tolist() for f, k in zip(ref["faces"], turn[ref["face_rows"]])]


def test_the_named_cases_are_what_their_names_say():
    ref = {n: ms.simplify_case_reference(n, "quadric") for n in CASES}
    fine, c = ref["plane_fine"], ms.simplify_case("plane_fine")
    assert fine["faces"].tolist() == c["faces"].tolist() and fine["inverse"].tolist() == list(range(289))
    assert 0 < len(ref["plane_3"]["vertices"]) < 289 // 4
    assert len(ref["plane_one_cell"]["vertices"]) == 0 and len(ref["plane_one_cell"]["faces"]) == 0
    assert (ref["plane_one_cell"]["inverse"] == -1).all()
    assert len(ref["plane_one_cell_keep"]["vertices"]) == 1 and ref["plane_one_cell_keep"]["count"].tolist() == [289]
    for n in (1, 255, 256, 257):
        assert len(ref["faces_%d" % n]["faces"]) == n and ref["clusters_%d" % n]["clusters"] == n
    assert len(ref["loose_vertices"]["vertices"]) < ref["loose_vertices"]["clusters"] == len(ref["loose_vertices_keep"]["vertices"])
    assert (ref["nonfinite"]["inverse"][[5, 17, 40]] == -1).all() and 0 not in ref["nonfinite"]["face_rows"]
    for n in ("soup_coarse_1", "soup_coarse_2"):                      # most faces meet an equal one
        assert 2 * len(ref[n]["faces"]) < len(ms.simplify_case(n)["faces"])
    assert len(ref["soup_1"]["faces"]) < 400
    for placement in ms.PLACEMENTS:
        assert ms.simplify_case_reference("fallback", placement)["fallbacks"] > 0
    assert all(ref[n]["fallbacks"] == 0 for n in CASES if n != "fallback")
    # the opposite winding is another face, a rotation is not
    d = ms.simplify_reference(np.eye(3, dtype=np.float32), [[0, 1, 2], [1, 2, 0], [2, 1, 0], [0, 2, 1]], 0.5)
    assert d["face_rows"].tolist() == [0, 2] and d["faces"].tolist() == [[0, 1, 2], [2, 1, 0]]


def test_mean_placement_without_dropping_is_the_voxel_merge():
    for name in ("plane_3", "cube_origin", "nonfinite", "loose_vertices_keep", "soup_1"):
        c = ms.simplify_case(name)
        ref, vx = _ref(c, "mean", drop_unreferenced=False), vr.voxel_reference(c["vertices"], c["voxel_size"], c["colors"], c["origin"])
        assert ref["fallbacks"] == 0
        for mine, theirs in (("vertices", "points"), ("colors", "colors"), ("count", "count"), ("first", "first"), ("inverse", "inverse")):
            assert (ref[mine] is None and vx[theirs] is None) or ref[mine].tobytes() == vx[theirs].tobytes(), mine


@pytest.mark.parametrize("placement", ms.PLACEMENTS)
def test_a_plane_stays_a_plane(placement):
    """A lattice on a plane in general position, three spacings per cell.  Bounds, in world units, |coordinates| < 4 so
    half an fp32 step is h = 2^-23:
      input: every vertex lies within e_in = sqrt(3) h of the plane; output rounding adds the same again.
      mean: the merge floors every member's in-cell fraction to 2^-16 of a cell and centres it (<= 2^-17 per axis), and
        forms t = (p - o) * inv in three fp32 operations (<= 3 * 2^-24 |t| per axis, |t| <= T = 4 / v cells); a mean of
        points that far from the plane is that far from it: e_mean = sqrt(3) v (2^-17 + 3 * 2^-24 T).
      quadric: the facets' planes are the plane up to the input rounding: a facet's normal is off by at most
        tilt = 2 e_in / (spacing / sqrt(2)), its altitude, so inside the cell (diagonal sqrt(3) v) a facet's plane is within
        e_in + tilt sqrt(3) v of the plane, and along the normal the minimiser is a weighted mean of the facets' planes,
        pulled by lambda / (1 + lambda) towards the mean; every one of the 9 quantised terms is off by at most 2^-31 per
        incidence against a stiffness of 1 per incidence along the normal: e_quant = v * 9 * 2^-31 * (1 + sqrt(3))."""
    v32, f, normal, at = ms.tilted_plane()
    voxel, h = 0.3, 2.0 ** -23
    assert np.abs(v32).max() < 4
    e_in = np.sqrt(3.0) * h
    e_mean = np.sqrt(3.0) * voxel * (2.0 ** -17 + 3 * 2.0 ** -24 * (4 / voxel))
    tilt = 2 * e_in / (ms.PLANE_SPACING / np.sqrt(2.0))
    e_quadric = (e_in + tilt * np.sqrt(3.0) * voxel) + ms.LAMBDA * (e_in + e_mean) + voxel * 9 * 2.0 ** -31 * (1 + np.sqrt(3.0))
    bound = e_in + (e_mean + e_in if placement == "mean" else e_quadric)
    ref = ms.simplify_reference(v32, f, voxel, placement=placement)
    off = np.abs((ref["vertices"].astype(np.float64) - at) @ normal)
    print(f"plane, {placement}: {len(off)} vertices, farthest {off.max():.3e} from the plane, bound {bound:.3e}")
    assert len(off) > 20 and ref["fallbacks"] == 0 and off.max() <= bound


def test_the_quadric_finds_a_crease_the_mean_does_not():
    """Two planes meeting at 90 degrees along y, four spacings per cell.  In a cluster with k1 incidences of faces of one
    arm and k2 of the other (k = k1 + k2), with n1, n2 and the crease's direction as axes, the solve decouples:
    (k_i + lambda k)(x_i + d_i) = lambda k (u_i + d_i), where u is the mean and |u_i + d_i| <= sqrt(3) cells is its
    distance from arm i's plane.  So the vertex lies within lambda k sqrt(3) sqrt(1 / k1^2 + 1 / k2^2) cells of the crease
    (plus 1e-6 cells for the quantisation and the roundings), provided the crease crosses the clamped cell, which the
    test asks for.  The mean of the same clusters lies inside the angle, more than 0.05 cells from the crease."""
    v32, f, side = ms.crease()
    voxel = ms.CREASE_VOXEL
    quadric, mean = (ms.simplify_reference(v32, f, voxel, placement=p, drop_unreferenced=False) for p in ms.PLACEMENTS[::-1])
    assert quadric["inverse"].tolist() == mean["inverse"].tolist()
    cid, cell = quadric["inverse"], quadric["cluster_cells"]
    arm = np.array([np.sign(side[t].sum()) for t in f])               # every face lies on one arm
    assert (arm != 0).all()
    local = (ms.CREASE_AT[[0, 2]] / voxel) - (cell[:, [0, 2]] + 0.5)  # the crease in every cell's own x, z
    tested = 0
    for k in range(quadric["clusters"]):
        members = np.nonzero(cid == k)[0]
        if not ((side[members] < 0).any() and (side[members] > 0).any() and (np.abs(local[k]) < ms.CLAMP).all()):
            continue
        inc = np.isin(f, members)
        k1, k2 = int(inc[arm < 0].sum()), int(inc[arm > 0].sum())
        assert k1 > 0 and k2 > 0 and quadric["quadric"][k, 9] == k1 + k2
        bound = ms.LAMBDA * (k1 + k2) * np.sqrt(3.0) * np.sqrt(1 / k1 ** 2 + 1 / k2 ** 2) + 1e-6
        dist = [np.linalg.norm((r["vertices"][k].astype(np.float64) - ms.CREASE_AT)[[0, 2]]) / voxel for r in (quadric, mean)]
        print(f"crease cluster {k}: k1 {k1}, k2 {k2}, quadric {dist[0]:.3e} cells (bound {bound:.3e}), mean {dist[1]:.3e}")
        assert dist[0] <= bound and dist[1] > 0.05
        tested += 1
    assert tested >= 3
