"""The numpy restatement of mesh_sample and mesh_nearest (tests/mesh_nearest_reference.py) held to independent ground:
exactly representable cases, a differently written closest point (Ericson's region walk, in fp64), the draws against
Python integers, and the statistics of the sampler.  The GPU tests compare the kernels with the restatement byte for
byte; this file is what says the restatement computes the right thing."""
import numpy as np
import pytest

import mesh_nearest_reference as mr

U = 2.0 ** -24                       # the unit roundoff of fp32


# ---- the seven regions: exactly representable answers --------------------------------------------------------------------
@pytest.mark.parametrize("query, dist2, point", mr.SEVEN_REGIONS)
def test_the_seven_regions_of_the_unit_triangle_are_exact(query, dist2, point):
    got = mr.nearest_reference([query], *mr.UNIT, 10.0)
    assert got["dist2"].tolist() == [dist2] and got["point"].tolist() == [list(point)]
    assert got["face"].tolist() == [0] and got["within"].tolist() == [1]
    w = got["weights"][0].astype(np.float64)
    assert (w >= 0).all() and w.sum() == 1.0
    assert (w @ mr.UNIT[0].astype(np.float64)).tolist() == list(point)
    # just out of reach: the same query with max_dist below the distance
    miss = mr.nearest_reference([query], *mr.UNIT, np.sqrt(dist2) * 0.999)
    assert miss["dist2"].tolist() == [np.inf] and miss["face"].tolist() == [-1] and miss["within"].tolist() == [0]
    assert not miss["point"].any() and not miss["weights"].any()


def test_degenerate_faces_are_their_sides_and_their_point():
    v = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [3, 4, 0]], np.float32)
    collinear = mr.nearest_reference([[1.5, 1, 0], [-1, 0, 0], [5, 0, 1]], v, [[0, 1, 2]], 10.0)
    assert collinear["dist2"].tolist() == [1.0, 1.0, 10.0]
    assert collinear["point"].tolist() == [[1.5, 0, 0], [0, 0, 0], [2, 0, 0]]
    point = mr.nearest_reference([[0, 0, 0], [3, 4, 1]], v, [[3, 3, 3]], 10.0)
    assert point["dist2"].tolist() == [25.0, 1.0] and point["point"].tolist() == [[3, 4, 0], [3, 4, 0]]
    assert point["weights"].sum(axis=1).tolist() == [1.0, 1.0]


def test_ties_go_to_the_lowest_row_and_invalid_faces_take_no_part():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [np.nan, 0, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 1]], np.int64)
    q = [[0.5, 0, 0.25]]                                # over the shared side: the same distance to both
    assert mr.nearest_reference(q, v, faces, 1.0)["face"].tolist() == [0]
    assert mr.nearest_reference(q, v, faces[::-1], 1.0)["face"].tolist() == [0]
    assert mr.nearest_reference(q, v, faces, 1.0)["within"].tolist() == [2]
    mixed = np.array([[0, 1, -1], [0, 1, 5], [0, 1, 4], [0, 1, 2]], np.int64)
    got = mr.nearest_reference(q, v, mixed, 1.0)
    assert got["face"].tolist() == [3] and got["within"].tolist() == [1]
    assert mr.nearest_reference([[np.nan, 0, 0], [np.inf, 0, 0]], v, faces, 1.0)["face"].tolist() == [-1, -1]


# ---- an independent closest point: Ericson's region walk (Real-Time Collision Detection, 5.1.5), scalar fp64 -------------
def ericson(p, a, b, c):
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return a
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return b
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return a + (d1 / (d1 - d3)) * ab
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return c
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return a + (d2 / (d2 - d6)) * ac
    va = d3 * d6 - d5 * d4
    if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        return b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b)
    denom = 1.0 / (va + vb + vc)
    return a + ab * (vb * denom) + ac * (vc * denom)


def _triangles(kind, n, rng):
    if kind == "random":
        return rng.uniform(-4, 4, (n, 3, 3)).astype(np.float32)
    # slivers: the third corner within 2^-10 of the first side's length off that side (sin of the angle >= ~2^-11)
    a, b = rng.uniform(-4, 4, (n, 3)), rng.uniform(-4, 4, (n, 3))
    t = rng.uniform(-0.2, 1.2, (n, 1))
    off = rng.standard_normal((n, 3))
    off *= (np.linalg.norm(b - a, axis=1, keepdims=True) * 2.0 ** -10) / np.linalg.norm(off, axis=1, keepdims=True)
    return np.stack([a, b, a + t * (b - a) + off], axis=1).astype(np.float32)


@pytest.mark.parametrize("kind", ["random", "sliver"])
def test_against_an_independent_closest_point(kind):
    """The bound, derived.  Let d be the true distance and x* the true closest point (Ericson's walk in fp64 gives both
    to ~2^-50).  The restatement forms x in fp64: with corners of magnitude <= S and the sine of the face's smallest
    angle >= 2^-11, the barycentric weights carry a relative error of a few 2^-53 / sine, so |x - x*| <= E64 =
    2^-36 S (a generous constant 2^6).  x32 = fp32(x) is ONE rounding, |x32_k - x_k| <= U |x_k| per axis, and the clamp
    to the face's box is a projection onto intervals that hold x*_k, so it brings x32 no farther from x*:
    |x32 - x*| <= EX = U |x| + E64.  So the exact distance of q to x32 lies in [d - EX, d + EX].  d2 is then formed in
    fp32 by THREE kinds of rounded step, each within (1 +- U): the differences (squared: two factors), the products,
    and the two additions (two factors): five factors in all.  Hence
        max(d - EX, 0)^2 (1 - U)^5  <=  d2  <=  (d + EX)^2 (1 + U)^5 ."""
    rng = np.random.default_rng(0 if kind == "random" else 1)
    n = 400
    tri = _triangles(kind, n, rng)
    q = (tri[np.arange(n), rng.integers(0, 3, n)] + rng.uniform(-3, 3, (n, 3))).astype(np.float32)
    d2, x32, w = mr.closest(q, tri)
    assert d2.dtype == np.float32 and x32.dtype == np.float32 and w.dtype == np.float64
    worst = 0.0
    for i in range(n):
        p, (a, b, c) = q[i].astype(np.float64), tri[i].astype(np.float64)
        star = ericson(p, a, b, c)
        d = np.linalg.norm(p - star)
        scale = max(np.abs(tri[i]).max(), np.abs(q[i]).max())
        ex = U * np.linalg.norm(x32[i].astype(np.float64)) + 2.0 ** -36 * scale
        lo, hi = max(d - ex, 0.0) ** 2 * (1 - U) ** 5, (d + ex) ** 2 * (1 + U) ** 5
        assert lo <= float(d2[i]) <= hi, (i, lo, float(d2[i]), hi)
        assert np.linalg.norm(x32[i] - star) <= ex
        # the weights reproduce the point, are non-negative and sum to one (to fp64 rounding)
        assert (w[i] >= 0).all() and abs(w[i].sum() - 1.0) <= 2.0 ** -50
        assert np.linalg.norm(w[i] @ tri[i].astype(np.float64) - star) <= ex
        worst = max(worst, abs(float(d2[i]) - d * d) / max(hi - lo, 1e-300))
    assert worst <= 1.0


def test_the_brute_force_is_the_minimum_over_the_faces():
    v, f = mr.height_field(6)
    q = mr.queries_near(v, 50)
    got = mr.nearest_reference(q, v, f, 1.5)
    d2, _, _ = mr.closest(q[:, None, :], v[f][None])
    r2 = np.float32(1.5) * np.float32(1.5)
    assert got["within"].tolist() == (d2 <= r2).sum(axis=1).tolist() and (got["within"] > 0).any()
    hit = got["face"] >= 0
    assert (got["dist2"][hit] == d2.min(axis=1)[hit]).all() and (got["face"][hit] == d2.argmin(axis=1)[hit]).all()
    # chunking the queries changes nothing
    again = mr.nearest_reference(q, v, f, 1.5, chunk=7)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def test_the_cloud_of_point_faces_is_cloud_nearest():
    rng = np.random.default_rng(4)
    target = rng.uniform(-2, 2, (60, 3)).astype(np.float32)
    q = rng.uniform(-2, 2, (80, 3)).astype(np.float32)
    faces = np.repeat(np.arange(60)[:, None], 3, axis=1)
    got = mr.nearest_reference(q, target, faces, 0.7)
    assert got["dist2"].tobytes() == mr.cloud_reference(q, target, 0.7).tobytes() and np.isfinite(got["dist2"]).any()


def test_the_boxes_and_the_counts():
    v = np.array([[0, 0, 0], [1.5, 0, 0], [0, 1.5, 0], [0, 0, 1.5], [-0.5, -0.5, -0.5], [np.inf, 0, 0], [3e6, 0, 0]],
                 np.float32)
    faces = np.array([[0, 1, 2], [4, 4, 4], [0, 1, 5], [0, 1, 9], [0, 1, 3]], np.int64)
    state, lo, hi = mr.face_boxes(v, faces, 1.0)
    assert state.tolist() == [1, 1, 0, 0, 1]
    assert lo[0].tolist() == [0, 0, 0] and hi[0].tolist() == [1, 1, 0] and lo[1].tolist() == hi[1].tolist() == [-1, -1, -1]
    assert mr.count_reference(v, faces, 1.0) == (4 + 1 + 4, 0, 0)
    assert mr.count_reference(v, faces, 0.1) == (256 + 1 + 256, 0, 0)       # 16 x 16 x 1 cells each: small still
    assert mr.count_reference(v, faces, 0.05) == (1, 2, 0)                  # 31 x 31 x 1 = 961 cells each: large
    assert mr.count_reference(v, [[0, 1, 6]], 1.0) == (0, 0, 1)  # a finite vertex 3e6 cells out
    assert mr.count_reference(v, [[0, 1, 6]], 4.0) == (0, 1, 0)  # 750001 cells in a row: large, inside the grid


# ---- the draws against Python integers -----------------------------------------------------------------------------------
def _fin(z):
    m = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_the_draws_are_splitmix64_and_the_product_is_exact():
    m = (1 << 64) - 1
    for seed in (0, 1, 0xDEADBEEF, m):
        c = np.array([1, 2, 3, 4097, 3 * (2 ** 31 - 2) + 3], np.uint64)
        want = [_fin((seed + int(k) * 0x9E3779B97F4A7C15) & m) for k in c]
        assert mr.splitmix(seed, c).tolist() == want
    assert int(mr.splitmix(0, np.array([1], np.uint64))[0]) == 0xE220A8397B1DCDAF      # splitmix64(0)'s first output
    rng = np.random.default_rng(9)
    a = rng.integers(0, 2 ** 64, 200, dtype=np.uint64)
    b = np.concatenate([rng.integers(0, 2 ** 64, 196, dtype=np.uint64), np.array([0, 1, m, 2 ** 63], np.uint64)])
    assert mr.umul64hi(a, b).tolist() == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]
    assert int(mr.umul64hi(np.uint64(m), np.uint64(m))) == (m * m) >> 64


def test_the_weights_are_exact_integers_below_2_to_the_32():
    v, f = mr.six_triangles()
    q, area = mr.sample_weights(v, f)
    assert area.tolist() == [1.0, 2.0, 4.0, 8.0, 0.0, 3.0]
    assert q.tolist() == [1 << 28, 1 << 29, 1 << 30, 1 << 31, 0, 3 << 28]
    assert mr.sample_prefix(v, f).tolist() == np.cumsum([int(x) for x in q]).tolist()
    # a face at 2^-32 of the largest gets weight 0, one at 2^-31 weight 1; the scale follows the largest alone
    v2 = np.array([[0, 0, 0], [2.0 ** 16, 0, 0], [0, 2.0 ** 16, 0], [1, 0, 0], [0, 1, 0], [0, 2, 0]], np.float32)
    q2, _ = mr.sample_weights(v2, [[0, 3, 4], [0, 1, 2], [0, 3, 5]])
    assert q2.tolist() == [0, 1 << 31, 1]
    # faces that take no part have weight 0, and a mesh of them no total
    bad = np.array([[0, 1, -1], [0, 1, 6], [0, 0, 0]], np.int64)
    assert mr.sample_weights(v2, bad)[0].tolist() == [0, 0, 0]
    assert mr.sample_reference(v2, bad, 5)["total"] == 0 and mr.sample_reference(v2, bad, 5)["face"].tolist() == [-1] * 5


# ---- the sampler's statistics ----------------------------------------------------------------------------------------------
def test_sampler_statistics_on_the_six_triangles():
    v, f = mr.six_triangles()
    n = 4096
    s = mr.sample_reference(v, f, n, seed=0)
    counts = np.bincount(s["face"], minlength=6)
    assert counts.tolist() == [223, 460, 910, 1845, 0, 658]     # the stated draws give exactly these
    p = np.array([1, 2, 4, 8, 0, 3]) / 18.0
    assert (np.abs(counts - n * p) <= 4 * np.sqrt(n * p * (1 - p))).all()
    assert counts[4] == 0                                        # the zero-area face is never drawn
    # a barycentric weight of a uniform sample has mean 1/3 and variance 1/18
    assert (np.abs(s["weights"].astype(np.float64).mean(axis=0) - 1 / 3) <= 4 * np.sqrt(1 / (18 * n))).all()


def test_every_sample_is_the_stated_combination_of_its_faces_vertices():
    v, f = mr.height_field(7)
    rng = np.random.default_rng(2)
    normals = rng.standard_normal(v.shape).astype(np.float32)
    normals[5] = 0
    colors = rng.integers(0, 256, v.shape, dtype=np.uint8)
    s = mr.sample_reference(v, f, 500, seed=7, normals=normals, colors=colors)
    w = s["weights"].astype(np.float64)
    assert (s["weights"] >= 0).all() and (np.abs(w.sum(axis=1) - 1) <= 3 * U).all()
    assert ((s["face"] >= 0) & (s["face"] < len(f))).all() and len(np.unique(s["face"])) > 30
    corners = v[f[s["face"]]].astype(np.float64)
    combo = np.einsum("nk,nkc->nc", w, corners)
    # (the weights were rounded to fp32 after the point was formed from them: three roundings of U times the corners)
    assert (np.abs(combo - s["points"]) <= 4 * U * np.abs(corners).max(axis=1)).all()
    nsum = np.einsum("nk,nkc->nc", w, normals[f[s["face"]]].astype(np.float64))
    unit = nsum / np.linalg.norm(nsum, axis=1, keepdims=True)
    assert np.abs(unit - s["normals"]).max() <= 1e-5 and np.abs(np.linalg.norm(s["normals"], axis=1) - 1).max() <= 1e-6
    csum = np.einsum("nk,nkc->nc", w, colors[f[s["face"]]].astype(np.float64))
    assert np.abs(csum - s["colors"]).max() <= 0.5 + 1e-4
    # a zero normal sum gives (0,0,0)
    zero = mr.sample_reference(v, f, 50, seed=7, normals=np.zeros_like(v))
    assert not zero["normals"].any()


def test_the_prefix_property_and_the_seed():
    v, f = mr.height_field(5)
    long, short = mr.sample_reference(v, f, 300, seed=3), mr.sample_reference(v, f, 77, seed=3)
    for k in ("points", "face", "weights"):
        assert long[k][:77].tobytes() == short[k].tobytes()
    other = mr.sample_reference(v, f, 77, seed=4)
    assert other["face"].tolist() != short["face"].tolist()
    # permuting the faces moves the prefix: the same draws land in other faces (expected, documented)
    perm = mr.permutation(len(f))
    moved = mr.sample_reference(v, f[perm], 77, seed=3)
    assert (perm[moved["face"]] != short["face"]).any()


# ---- the cases of the GPU tests are what they claim to be ------------------------------------------------------------------
def test_the_gpu_cases_are_what_they_claim():
    count = lambda name: (lambda c: mr.count_reference(c["vertices"], c["faces"], c["max_dist"]))(mr.nearest_case(name))  # noqa: E731
    assert count("span_2x2x2") == (8, 0, 0) and count("box_512") == (mr.BOX_CELLS, 0, 0) and count("box_513") == (0, 1, 0)
    for f in mr.FACE_COUNTS[:-1]:
        assert count("faces_%d" % f) == (f, 0, 0)
    assert mr.FACE_COUNTS[-1] == 2 ** 19 + 1                       # (its count is checked where its reference is made)
    c = mr.nearest_case("long_face")
    state, lo, hi = mr.face_boxes(c["vertices"], c["faces"][-1:], c["max_dist"])
    assert state.tolist() == [1] and (hi - lo + 1).tolist() == [[41, 1, 1]]
    c = mr.nearest_case("span_2x2x2")                              # all eight cells lie inside the first query's range
    assert mr.nearest_case_reference("span_2x2x2")["within"].tolist() == [1, 1, 1, 1]
    assert mr.nearest_case_reference("at_reach")["within"].tolist() == [1, 0, 1]
    tiny = mr.nearest_case_reference("tiny_radius")
    assert (tiny["dist2"] == 0).all() and (tiny["face"] >= 0).all()
    for name in mr.SAMPLE_CASES[:10]:
        assert (mr.sample_case_reference(name)["total"] > 0)
    assert mr.sample_case_reference("no_area")["total"] == 0
    assert mr.sample_case_reference("tiny_face")["total"] == (1 << 31) + 1
