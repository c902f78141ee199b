"""The numpy restatement of the mesh render (tests/mesh_render_reference.py) held to independent ground, without a GPU:
watertight coverage, depth and weights against fp64 geometry within bounds derived here from the vertex snap and the
stated roundings, the integer arithmetic at the corners of the guard band, the agreement with the cloud render's
restatement where a vertex lies on a pixel centre, the order of the faces, the clipped counts against a plain loop, and
that every named case of tests/test_mesh_render_gpu.py exercises what its name says."""
import numpy as np
import pytest

import cloud_render_reference as cr
import mesh_render_reference as mr

f32, f64 = np.float32, np.float64
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53          # the relative error of one rounding to nearest
SNAP = 2.0 ** -9                               # rintf(256 u) / 256 moves a coordinate by at most half of 1/256 pixel


# ---- watertight coverage -------------------------------------------------------------------------------------------------
def test_a_jittered_height_field_is_covered_without_gaps_inside_and_nowhere_twice():
    c, ref = mr.case("watertight"), mr.case_reference("watertight")
    assert len(c["faces"]) == 288 and (c["rows"], c["cols"]) == (33, 65)
    cover = ref["cover"][0]
    assert set(np.unique(cover).tolist()) == {0, 1}
    assert cover.sum() == (ref["face"] >= 0).sum() > 0.75 * cover.size
    # no gaps: the covered pixels of a row form one run (the sheet's outline is convex up to the jitter of its rim)
    for r in range(c["rows"]):
        at = np.nonzero(cover[r])[0]
        assert len(at) == 0 or len(at) == at[-1] - at[0] + 1, r


def test_a_grid_on_the_pixel_centres_gives_every_interior_pixel_to_exactly_one_face():
    c, ref = mr.case("on_centres"), mr.case_reference("on_centres")
    view = mr.case_views("on_centres")[0]
    assert (view.X % 512 == 0).all() and (view.Y % 512 == 0).all()        # every vertex on a centre (2 c, 2 r)
    cover = ref["cover"][0]
    assert (cover[1:-1, 1:-1] == 1).all() and cover.max() == 1            # edges and vertices included
    # a centre on a shared edge, and one on a shared vertex, were decided by the tie rule alone
    face, r, col = view.pairs()
    E, covered = view.edges(face, r, col)
    on_edge = ((E == 0).sum(axis=0) == 1) & covered
    on_vertex = ((E == 0).sum(axis=0) == 2) & covered
    assert on_edge.sum() > 100 and on_vertex.sum() > 50
    assert (ref["depth"][ref["face"] >= 0] == f32(2.0)).all()


# ---- depth and weights -----------------------------------------------------------------------------------------------------
def test_the_reciprocal_of_the_reciprocal_rounds_back():
    z = np.random.default_rng(0).uniform(0.01, 1000.0, 10 ** 5).astype(f32)
    z = np.concatenate([z, np.exp(np.random.default_rng(1).uniform(-20, 20, 10 ** 5)).astype(f32)])
    assert ((1.0 / (1.0 / z.astype(f64))).astype(f32) == z).all()


@pytest.mark.parametrize("z0", [0.3, 1.0, 2.5, 3.1415927, 77.77, 1e-3, 12345.678])
def test_a_fronto_parallel_plane_has_its_own_depth_bit_for_bit(z0):
    K, T = mr.straight_camera(52.0, 31.7, 16.2)
    z0 = float(f32(z0))
    v, faces = mr.soup(K, [[-20.3, 150.1, -20.7]], [[-11.9, -10.2, 90.3]], z0)
    assert (v[:, 2] == f32(z0)).all()
    ref = mr.render_reference(v, faces, K, T, 33, 65)
    assert (ref["face"] == 0).all() and ref["depth"].tobytes() == np.full((1, 33, 65), z0, f32).tobytes()


def slanted():
    """A slanted face over the whole 33 x 65 map of a straight camera, and what the bounds below need."""
    f, cx, cy = 52.0, 31.7, 16.2
    K, T = mr.straight_camera(f, cx, cy)
    v, faces = mr.soup(K, [[-20.3, 150.1, -20.7]], [[-11.9, -10.2, 90.3]], [[2.0, 5.5, 3.25]])
    f, cx, cy = float(K[0, 0, 0]), float(K[0, 0, 2]), float(K[0, 1, 2])
    return K, T, v, faces, f, cx, cy


def test_a_slanted_plane_has_the_depth_of_the_ray_through_the_pixel_centre():
    K, T, v, faces, f, cx, cy = slanted()
    ref = mr.render_reference(v, faces, K, T, 33, 65)
    assert (ref["face"] == 0).all()
    p = v.astype(f64)                                                     # the plane n . x = d through the fp32 vertices
    n = np.cross(p[1] - p[0], p[2] - p[0])
    d = n @ p[0]
    r, c = np.mgrid[0:33, 0:65].astype(f64)
    w_true = (n[0] * (c - cx) / f + n[1] * (r - cy) / f + n[2]) / d       # the inverse depth: affine in (c, r)
    z_true = 1.0 / w_true
    # Derivation.  The render interpolates 1/z linearly over the SNAPPED triangle, with the vertices' own z.  Snapping
    # moves a vertex's screen position by at most `move` per coordinate: SNAP, plus the three fp32 roundings behind u
    # (c_x z, the fmaf, the division), each of relative size EPS32 on a magnitude of at most |u| + 2 |c_x|.  A covered
    # centre is the same convex combination of the snapped positions as its pre-image is of the true ones, so the render
    # evaluates the true, affine inverse depth at a point at most `move` per coordinate from the centre:
    # |dw| <= (|dw/dc| + |dw/dr|) move.  z and the rendered z' both lie within the vertices' range (convexity), and
    # |z' - z| = z z' |dw| <= z_hi^2 |dw|.  On top: the three divisions E/A, the three 1/zc, three products, two sums,
    # 1/S (12 roundings of EPS64, amplified by at most z_hi / z_lo through the sum) and the rounding to fp32.
    u_max = np.abs(np.stack([(p[:, 0] / p[:, 2]) * f + cx, (p[:, 1] / p[:, 2]) * f + cy])).max()
    move = SNAP + 3 * EPS32 * (u_max + 2 * max(cx, cy))
    grad = (abs(n[0]) + abs(n[1])) / (f * abs(d))
    z_lo, z_hi = p[:, 2].min(), p[:, 2].max()
    bound = z_hi ** 2 * grad * move + z_hi * (EPS32 + 12 * EPS64 * z_hi / z_lo)
    err = np.abs(ref["depth"][0].astype(f64) - z_true)
    assert err.max() <= bound and bound < 1e-3 * z_lo, (err.max(), bound)
    assert err.max() > 0                                                  # (the bound is not vacuous: the snap shows)


def test_the_weights_sum_to_one_and_reproject_to_the_pixel_centre():
    K, T, v, faces, f, cx, cy = slanted()
    ref = mr.render_reference(v, faces, K, T, 33, 65)
    w = ref["weights"][0].astype(f64)                                      # (3,33,65)
    assert (w >= 0).all() and (w <= 1).all()
    # each weight is (lambda_k q_k) / S in fp64, rounded to fp32 once: at most EPS32 / 2 off for a value below 1; the
    # fp64 weights sum to (sum of the products) / S = 1 up to the sum's two roundings and the three divisions'
    assert np.abs(w.sum(axis=0) - 1.0).max() <= 3 * EPS32 / 2 + 5 * EPS64
    p = v.astype(f64)
    x = np.einsum("krc,kj->jrc", w, p)                                    # sum b_k vertex_k
    u, vv = f * x[0] / x[2] + cx, f * x[1] / x[2] + cy
    r, c = np.mgrid[0:33, 0:65].astype(f64)
    # In exact arithmetic the point projects to sum lambda_k (true position of vertex k), and sum lambda_k (snapped
    # position of vertex k) is the centre: the distance is at most `move` (above).  The fp32 rounding of the weights
    # moves the point by at most 3 EPS32 / 2 of the largest coordinate; u = f x / z + c_x turns that into pixels.
    u_max = np.abs(np.stack([(p[:, 0] / p[:, 2]) * f + cx, (p[:, 1] / p[:, 2]) * f + cy])).max()
    move = SNAP + 3 * EPS32 * (u_max + 2 * max(cx, cy))
    xy, z_lo, z_hi = np.abs(p[:, :2]).max(), p[:, 2].min(), p[:, 2].max()
    rounding = 1.5 * EPS32 * f * (xy / z_lo + xy * z_hi / z_lo ** 2) * 1.001
    assert max(np.abs(u - c).max(), np.abs(vv - r).max()) <= move + rounding < 2.5e-3


# ---- integers at the corners of the guard band ----------------------------------------------------------------------------
def test_edge_functions_and_area_at_the_guard_band_are_exact():
    g = 2 ** 24
    tris = [((-g, -g), (g, -g), (-g, g)), ((g, g), (-g, g), (g, -g)), ((-g, g), (-g, -g), (g, g - 1)),
            ((g, -g), (g - 3, g), (-g, -g + 5))]
    view = mr.View.__new__(mr.View)
    X = np.array([[p[0] for p in t] for t in tris], np.int64)
    Y = np.array([[p[1] for p in t] for t in tris], np.int64)
    A = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    assert (A > 0).all()
    view.Xo, view.Yo, view.A = X, Y, A
    corners = [(0, 0), (0, 2 ** 15 - 1), (2 ** 15 - 1, 0), (2 ** 15 - 1, 2 ** 15 - 1), (12345, 6789)]
    for t, tri in enumerate(tris):
        area = (tri[1][0] - tri[0][0]) * (tri[2][1] - tri[0][1]) - (tri[1][1] - tri[0][1]) * (tri[2][0] - tri[0][0])
        assert int(A[t]) == area and abs(area) < 2 ** 52 and int(float(area)) == area
        for r, c in corners:
            E, _ = view.edges(np.array([t]), np.array([r]), np.array([c]))
            total = 0
            for k in range(3):
                p, q = tri[(k + 1) % 3], tri[(k + 2) % 3]
                e = (q[0] - p[0]) * (256 * r - p[1]) - (q[1] - p[1]) * (256 * c - p[0])      # Python integers
                assert int(E[k, 0]) == e and abs(e) < 2 ** 52 and int(float(e)) == e
                assert f64(E[k, 0]) / f64(A[t]) == float(e) / float(area)
                total += e
            assert total == area                                          # the three weights sum to one before rounding


# ---- a vertex on a pixel centre ----------------------------------------------------------------------------------------
def test_a_vertex_on_a_pixel_centre_has_the_cloud_renders_bits():
    rows, cols = 9, 11
    K, T = mr.straight_camera(52.0, 5.0, 4.0)
    rim = 6
    ang = 2 * np.pi * np.arange(rim) / rim + 0.2
    px = np.concatenate([[5.0], 5.0 + 3.3 * np.cos(ang)])
    py = np.concatenate([[4.0], 4.0 + 3.1 * np.sin(ang)])
    z = np.concatenate([[2.7182817], 3.0 + 0.4 * np.cos(3 * ang)])
    v = mr.at_pixels(K, px, py, z)
    faces = np.array([[0, 1 + k, 1 + (k + 1) % rim] for k in range(rim)], np.int64)
    for flip in (False, True):
        ref = mr.render_reference(v, faces[:, [0, 2, 1]] if flip else faces, K, T, rows, cols)
        cloud = cr.render_reference(v[:1], K, T, rows, cols)
        assert cloud["index"][0, 4, 5] == 0 and ref["cover"][0, 4, 5] == 1
        assert ref["depth"][0, 4, 5].tobytes() == cloud["depth"][0, 4, 5].tobytes() == v[0, 2].tobytes()
        k = int(np.argmax(ref["weights"][0, :, 4, 5]))
        assert ref["weights"][0, :, 4, 5].tolist() == [1.0 if j == k else 0.0 for j in range(3)]
        assert faces[ref["face"][0, 4, 5]][[0, 2, 1] if flip else [0, 1, 2]][k] == 0


# ---- order ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_65_33_65_0", "whole_map", "wave_mixed", "contention_shuffled"])
def test_permuted_faces_give_the_same_depth_bytes(name):
    c, base = mr.case(name), mr.case_reference(name)
    perm = mr.permutation(len(c["faces"]))
    moved = mr.render_reference(c["vertices"], c["faces"][perm], c["K"], c["T"], c["rows"], c["cols"])
    assert moved["depth"].tobytes() == base["depth"].tobytes() and moved["cover"].tobytes() == base["cover"].tobytes()
    assert moved["clipped"].tobytes() == base["clipped"].tobytes()
    hit = base["face"] >= 0
    assert (perm[moved["face"][hit]] == base["face"][hit]).mean() > 0.99


def test_a_tie_goes_to_the_lowest_row_and_the_nearest_face_wins_otherwise():
    r, c = mr.CONTENTION_PIXEL
    for order in ("equal", "ascending", "descending", "shuffled"):
        case, ref = mr.case("contention_" + order), mr.case_reference("contention_" + order)
        assert len(case["faces"]) == mr.CONTENTION_N == 4099 and ref["cover"][0, r, c] == 4099
        z = case["vertices"][::3, 2]
        assert ref["face"][0, r, c] == np.argmin(z) and ref["depth"][0, r, c] == z.min()
        assert (len(np.unique(z)) == 1) == (order == "equal")
    assert mr.case_reference("contention_equal")["face"][0, r, c] == 0
    assert np.argmin(mr.case("contention_descending")["vertices"][::3, 2]) == 4098


# ---- clipping --------------------------------------------------------------------------------------------------------------
def test_the_clipped_counts_are_those_of_a_plain_loop():
    for name in ("clipping", "nonpart", "edge_63_5_7_-1"):
        c, ref = mr.case(name), mr.case_reference(name)
        lo = float(f32(c.get("min_depth", 0.0)))
        P = mr.cameras(c["K"], c["T"])
        M = len(c["vertices"])
        for v in range(len(P)):
            zc, u, w = (a.tolist() for a in mr.project(P[v], c["vertices"]))
            count = 0
            for face in c["faces"].tolist():
                if not all(0 <= i < M for i in face) or not all(np.isfinite(c["vertices"][i]).all() for i in face):
                    continue
                part = all(zc[i] > lo and abs(zc[i]) != float("inf") and abs(u[i]) <= 65536.0 and abs(w[i]) <= 65536.0
                           for i in face)
                count += (not part) and any(zc[i] > lo for i in face)
            assert ref["clipped"][v] == count, (name, v)
    assert mr.case_reference("clipping")["clipped"].tolist()[0] == 5


def test_the_clipping_case_is_what_its_rows_say():
    c, ref, view = mr.case("clipping"), mr.case_reference("clipping"), mr.case_views("clipping")[0]
    for name, (row, part, counted) in mr.CLIP_ROWS.items():
        assert bool(view.part[row]) == part and bool(view.clipped[row]) == counted, name
        assert (ref["face"][0] == row).any() == part, name
    at, past = mr.CLIP_ROWS["u_at_guard"][0], mr.CLIP_ROWS["u_past_guard"][0]
    P = mr.cameras(c["K"], c["T"])[0]
    _, u, _ = mr.project(P, c["vertices"])
    assert u[3 * at] == f32(65536.0) and u[3 * past] == np.nextafter(f32(65536.0), f32(np.inf))
    assert view.X[at, 0] == 2 ** 24
    at, past = mr.CLIP_ROWS["v_at_minus_guard"][0], mr.CLIP_ROWS["v_past_minus_guard"][0]
    _, _, w = mr.project(P, c["vertices"])
    assert w[3 * at] == f32(-65536.0) and w[3 * past] == np.nextafter(f32(-65536.0), f32(-np.inf))
    assert view.Y[at, 0] == -2 ** 24


# ---- what the named cases exercise ----------------------------------------------------------------------------------------
def test_the_smallest_cases():
    assert mr.case_reference("one_hit")["depth"].tolist() == [[[2.0]]] and mr.case_reference("one_hit")["face"].tolist() == [[[0]]]
    miss = mr.case_reference("one_miss")
    assert miss["depth"].tolist() == [[[0.0]]] and miss["face"].tolist() == [[[-1]]] and not miss["weights"].any()
    assert not miss["normals"].any() and not miss["colors"].any() and mr.case_views("one_miss")[0].part.all()


@pytest.mark.parametrize("name", mr.EDGE_CASES)
def test_the_edge_cases_have_their_sizes_and_both_paths(name):
    n, rows, cols, dv = (int(t) for t in name.split("_")[1:])
    c, views = mr.case(name), mr.case_views(name)
    assert len(c["faces"]) == n and len(views) == mr.CAMERA_BATCH + dv == len(c["K"]) and (c["rows"], c["cols"]) == (rows, cols)
    small = sum(int(((v.n > 0) & (v.n <= mr.SMALL_PIXELS)).sum()) for v in views)
    large = sum(int((v.n > mr.SMALL_PIXELS).sum()) for v in views)
    assert small > 100 and (large > 100 or cols == 7)
    ref = mr.case_reference(name)
    hit = (ref["face"] >= 0).mean()
    assert 0.2 < hit < 0.95 and ref["cover"].max() > 1                    # hits, misses and contention


def test_the_threshold_case_straddles_the_threshold():
    view = mr.case_views("threshold")[0]
    assert tuple(view.n.tolist()) == mr.case("threshold")["boxes"] == (mr.SMALL_PIXELS, mr.SMALL_PIXELS + 1) * 2
    ref = mr.case_reference("threshold")
    assert set(np.unique(ref["face"]).tolist()) == {-1, 0, 1, 2, 3}


def test_the_whole_map_and_wave_cases():
    ref, views = mr.case_reference("whole_map"), mr.case_views("whole_map")
    for v, view in enumerate(views):
        assert view.n[0] == 33 * 65 and (view.n[1:] <= mr.SMALL_PIXELS).all() and (ref["face"][v] >= 0).all()
        winners = set(np.unique(ref["face"][v]).tolist())
        face, r, c = view.pairs()
        covering = set(face[view.edges(face, r, c)[1]].tolist())
        assert 0 in winners and len(winners) > 50 and len(covering - winners) > 50      # in front of it, and behind it
    large = mr.case_views("wave_large")[0]
    assert len(large.n) == 64 and (large.n > mr.SMALL_PIXELS).all()
    mixed = mr.case_views("wave_mixed")[0]
    assert len(mixed.n) == 130 and (mixed.n[0::2] > mr.SMALL_PIXELS).all()
    assert ((mixed.n[1::2] > 0) & (mixed.n[1::2] <= mr.SMALL_PIXELS)).all()
    for name in ("wave_large", "wave_mixed"):
        assert len(np.unique(mr.case_reference(name)["face"])) > 30


def test_the_faces_that_take_no_part():
    c, ref, view = mr.case("nonpart"), mr.case_reference("nonpart"), mr.case_views("nonpart")[0]
    valid, _ = mr.valid_faces(c["vertices"], c["faces"])
    rows = mr.NONPART_ROWS
    for name in ("index_minus_one", "index_m", "index_plus_2_40", "index_minus_2_40", "nan_x", "nan_z", "inf_x",
                 "minus_inf_y", "inf_z"):
        assert not valid[rows[name][0]] and not view.part[rows[name][0]], name
    assert c["faces"].min() == -2 ** 40 and c["faces"].max() == 2 ** 40 and len(c["vertices"]) in c["faces"]
    for name in ("collinear", "repeated_vertex", "point"):
        assert view.part[rows[name][0]] and view.A[rows[name][0]] == 0, name
    for name, boxed in (("sub_pixel", False), ("sliver", True)):             # no centre in its box; centres, none covered
        assert view.part[rows[name][0]] and view.A[rows[name][0]] > 0 and (view.n[rows[name][0]] > 0) == boxed, name
    for name, (row, covers) in rows.items():
        assert (ref["face"] == row).any() == covers, name
    assert ref["clipped"].tolist() == [0] and (ref["face"] >= 0).all()
    assert view.swapped[rows["flipped_twin"][0]] != view.swapped[rows["plain"][0]]
    # the flipped mesh: the same bytes apart from the order of the weights
    flipped = mr.case_reference("nonpart_flipped")
    for key in ("depth", "face", "clipped", "cover"):
        assert flipped[key].tobytes() == ref[key].tobytes(), key
    assert flipped["weights"].tobytes() == ref["weights"][:, [0, 2, 1]].tobytes()
    assert (mr.case_views("nonpart_flipped")[0].swapped != view.swapped)[view.A > 0].all()


def test_the_depth_limits_case():
    ref, view = mr.case_reference("depth_limits"), mr.case_views("depth_limits")[0]
    seen = {name: bool((ref["face"][0] == row).any()) for row, name in enumerate(mr.LIMIT_ROWS)}
    assert seen == {"at_min": False, "above_min": True, "at_max": True, "past_max": False, "between": True}
    assert not view.part[0] and not view.clipped[0] and view.part[1:].all()
    d = ref["depth"][ref["face"] >= 0]
    assert d.min() == np.nextafter(f32(mr.LIMIT_MIN), f32(np.inf)) and d.max() == f32(mr.LIMIT_MAX)
    assert (ref["depth"][0][ref["face"][0] == 2] == f32(mr.LIMIT_MAX)).all()
    between = mr.LIMIT_ROWS.index("between")
    assert 0 < (ref["face"][0] == between).sum() < ref["cover"][0, :, 15:].sum()      # its far pixels are cut off


def test_the_borders_case():
    c, ref, view = mr.case("borders"), mr.case_reference("borders"), mr.case_views("borders")[0]
    rows, cols = c["rows"], c["cols"]
    inside = view.n > 0
    assert inside[:16].all() and not inside[16:].any() and view.part.all()
    r1, c1 = view.r0 + view.n // np.maximum(view.width, 1) - 1, view.c0 + view.width - 1
    for touches in (view.r0 == 0, view.c0 == 0, r1 == rows - 1, c1 == cols - 1):
        assert (touches & inside & (view.n <= mr.SMALL_PIXELS)).any() and (touches & inside & (view.n > mr.SMALL_PIXELS)).any()
    for corner in ((view.r0 == 0) & (view.c0 == 0), (view.r0 == 0) & (c1 == cols - 1), (r1 == rows - 1) & (view.c0 == 0),
                   (r1 == rows - 1) & (c1 == cols - 1)):
        assert (corner & inside).sum() >= 2
    assert len(set(np.unique(ref["face"]).tolist()) - {-1}) >= 12


def test_the_gathers_case():
    c, ref = mr.case("gathers"), mr.case_reference("gathers")
    face, nor, col = ref["face"][0], ref["normals"][0], ref["colors"][0]
    at = lambda name: face == mr.GATHER_ROWS[name]   # noqa: E731
    for name in mr.GATHER_ROWS:
        assert at(name).sum() >= 3, name
    assert not nor[:, at("zero_normals")].any() and (col[:, at("zero_normals")] == 255).all()
    assert not nor[:, 1, 5].any() and face[1, 5] == mr.GATHER_ROWS["opposite_normals"]     # the sum cancels there
    assert np.abs(nor[:, at("opposite_normals")]).sum() > 0 and not col[:, at("opposite_normals")].any()
    assert not nor[:, at("inf_normals")].any()                                             # inf - inf: no direction
    nan_face = nor[:, at("nan_normal")]
    assert np.isfinite(nan_face).all() and not nan_face[1].any()                           # the NaN never comes out
    plain = nor[:, at("plain")].astype(f64)
    assert np.abs(np.sqrt((plain ** 2).sum(axis=0)) - 1).max() < 4 * EPS32
    assert np.isfinite(ref["normals"]).all() and not ref["normals"][0][:, face < 0].any()
    # colours: the fp64 weighted sum rounded to nearest, against the rounded weights within one level
    w = ref["weights"][0].astype(f64)
    want = np.einsum("kp,pkj->jp", w.reshape(3, -1)[:, (face >= 0).reshape(-1)],
                     c["colors"].astype(f64)[c["faces"][face[face >= 0]]])
    assert np.abs(col.reshape(3, -1)[:, (face >= 0).reshape(-1)].astype(f64) - want).max() <= 0.5 + 255 * 3 * EPS32


def test_gathers_are_optional_in_the_restatement():
    ref, bare = mr.case_reference("gathers"), mr.case_reference("gathers", False)
    assert bare["normals"] is None and bare["colors"] is None
    for key in ("depth", "face", "weights", "clipped"):
        assert bare[key].tobytes() == ref[key].tobytes()
