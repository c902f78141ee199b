"""The restatement of integrate_cloud (tests/tsdf_cloud_reference.py) held to statements that do not share its code:
the float64 distance to a plane, the closed form of the definition on a sphere, the topology and the distance of the
sphere's mesh, and the properties the definition promises (no byte depends on the order of the rows, rows that take no
part leave no trace, a voxel out of reach keeps its bits)."""
import numpy as np

import tsdf_cloud_reference as tc
from tsdf_reference import EPS, SPHERE, mesh_topology, surface_nets_reference, voxel_centres

SQRT3 = np.sqrt(3.0)


def _run(c, **kw):
    a = dict(c)
    a.update(kw)
    return tc.tsdf_cloud_reference(a["points"], a["normals"], a["radius"], a["dims"], a["voxel_size"], a["origin"], a["trunc"],
                                   weights=a["weights"], colors=a["colors"], state=a["state"])


def _centres64(c):
    cx, cy, cz = (a.astype(np.float64) for a in tc.centres_f32(c["dims"], c["voxel_size"], c["origin"]))
    gz, gy, gx = np.meshgrid(cz, cy, cx, indexing="ij")
    return np.stack([gx, gy, gz], axis=-1)


def test_the_centres_are_a_multiply_and_an_add_within_one_rounding_of_the_fused_ones():
    for name in ("sphere", "plane", "offset", "prior"):
        c = tc.case(name)
        for mine, fused in zip(tc.centres_f32(c["dims"], c["voxel_size"], c["origin"]),
                               voxel_centres(c["dims"], c["voxel_size"], c["origin"])):
            assert mine.dtype == np.float32
            # the product is rounded at no more than EPS of itself, the sum once more: one rounding apart from the fma
            slack = EPS * np.abs(np.arange(len(mine)) * np.float64(np.float32(c["voxel_size"]))) + 2 * EPS * np.abs(fused)
            assert (np.abs(mine.astype(np.float64) - fused) <= slack).all()


def test_plane_values_are_the_float64_signed_distance_whatever_the_weights():
    c = tc.case("plane")
    nrm = np.asarray(tc.PLANE["normal"], np.float64)
    nrm /= np.linalg.norm(nrm)
    dims, vs, o = tc.PLANE["dims"], tc.PLANE["voxel_size"], np.asarray(tc.PLANE["origin"], np.float64)
    on_plane = o + 0.5 * vs * (np.asarray(dims) - 1) + tc.PLANE["offset"] * nrm
    x = _centres64(c)
    want = np.clip((x - on_plane) @ nrm, -np.float64(np.float32(c["trunc"])), np.float64(np.float32(c["trunc"])))
    # per row: the normal and the point rounded to fp32 (EPS sqrt3 of the difference and of the point), the three
    # differences, three products and two sums of s (6 EPS of sqrt3 radius), the quotient t / trunc (EPS), the quantum
    # of T (half of trunc 2^-20; a whole one is allowed), and the one rounding of each sum of the state (EPS each); the
    # value is a weighted mean of rows that all state the same plane, so the weights cancel
    pmax = np.abs(c["points"]).max()
    bound = c["trunc"] * 2.0 ** -20 + EPS * (8 * SQRT3 * c["radius"] + SQRT3 * pmax + 6 * c["trunc"])
    worst = []
    for weights in (c["weights"], None):
        r = _run(c, weights=weights)
        seen = r["weight"] > 0
        assert seen.sum() > 300 and np.array_equal(seen, r["updated"])
        err = np.abs(r["sdf_sum"][seen].astype(np.float64) / r["weight"][seen].astype(np.float64) - want[seen])
        worst.append(err.max())
        assert err.max() <= bound, (err.max(), bound)
    print(f"plane: error max {worst[0]:.3e} with weights, {worst[1]:.3e} without; bound {bound:.3e}")


def test_sphere_values_are_the_closed_form_and_the_level_set_lies_just_outside():
    c, r = tc.case("sphere"), tc.case_reference("sphere")
    centre, rad, R = np.asarray(SPHERE["centre"], np.float64), SPHERE["radius"], np.float64(np.float32(tc.SPHERE_RADIUS))
    x = _centres64(c).reshape(-1, 3)
    p = c["points"].astype(np.float64)
    d2 = ((x[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    phi = np.where(d2 <= R * R, (1.0 - d2 / (R * R)) ** 2, 0.0)
    s = np.linalg.norm(x - centre, axis=1)
    with np.errstate(all="ignore"):
        mean_d2 = (phi * d2).sum(axis=1) / phi.sum(axis=1)
    closed = ((s * s - rad * rad) - mean_d2) / (2 * rad)
    value = (r["sdf_sum"].astype(np.float64) / np.where(r["weight"] > 0, r["weight"], 1).astype(np.float64)).reshape(-1)
    weight, count = r["weight"].reshape(-1).astype(np.float64), r["count"].reshape(-1)
    # no row of the voxel is clamped: every s_j = (s^2 - r^2 - d_j^2) / (2 r) lies inside the truncation
    tr = np.float64(np.float32(c["trunc"]))
    free = (weight >= 1.0) & ((s * s - rad * rad) / (2 * rad) < tr - 1e-6) & ((s * s - rad * rad - R * R) / (2 * rad) > -tr + 1e-6)
    assert free.sum() > 1000
    # A_j is phi_j 2^16 to within one quantum (half from rint, 2^-4 from phi's fp32 steps), and moving the weights of a
    # mean of numbers inside +-trunc by e_j moves it by at most sum |e_j| 2 trunc / sum A; T's quantum and the fp32
    # steps of s are the plane test's
    bound = count * 2.0 * tr / (np.maximum(weight, 1.0) * 2.0 ** 16) + tr * 2.0 ** -20 + EPS * (8 * SQRT3 * R + SQRT3 * 1.0 + 6 * tr)
    err = np.abs(value - closed)
    print(f"sphere: {int(free.sum())} unclamped voxels of weight >= 1, |value - closed form| max {err[free].max():.3e}, "
          f"error / bound max {(err[free] / bound[free]).max():.3g}")
    assert (err[free] <= bound[free]).all()
    # the zero level: inside the sphere every tangent plane says inside; from radius^2 / (2 r) outside it every one says
    # outside (clamped or not: the clamp keeps the sign)
    seen, tol = weight > 0, 1e-5
    assert (value[seen & (s <= rad - tol)] < 0).all() and (seen & (s <= rad - tol)).sum() > 200
    far = seen & (s >= rad + R * R / (2 * rad) + tol)
    assert (value[far] > 0).all() and far.sum() > 200


def test_sphere_mesh_is_closed_wound_outwards_and_within_the_derived_bound():
    r = tc.case_reference("sphere")
    m = surface_nets_reference(r["sdf_sum"], r["weight"], None, 1.0, SPHERE["voxel_size"], SPHERE["origin"])
    v, f = m["vertices"], m["faces"]
    closed, euler, boundary = mesh_topology(f, len(v))
    assert closed and boundary == 0 and euler == 2, (closed, euler, boundary)
    centre = np.asarray(SPHERE["centre"], np.float64)
    tri = v[f]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((fn * (tri.mean(1) - centre)).sum(1) > 0).all(), "a face is wound inwards"
    dist = np.linalg.norm(v - centre, axis=1) - SPHERE["radius"]
    bound = tc.sphere_mesh_bound()
    print(f"sphere mesh: {len(v)} vertices, {len(f)} faces, distance {dist.min():.4f} to {dist.max():.4f}, bound {bound:.4f}")
    assert abs(bound - 0.062) < 5e-4                          # (derived: radius^2 / (2 r) + sphere_bound)
    assert np.abs(dist).max() <= bound
    assert len(v) > 500 and len(f) > 1000


def test_permuting_the_rows_changes_no_byte():
    for name in ("colours", "bad_rows", "duplicates"):
        c = tc.case(name)
        perm = np.random.default_rng(311).permutation(len(c["points"]))
        moved = _run(c, points=c["points"][perm], normals=c["normals"][perm],
                     weights=None if c["weights"] is None else c["weights"][perm],
                     colors=None if c["colors"] is None else c["colors"][perm])
        assert tc.state_bytes(moved) == tc.state_bytes(tc.case_reference(name)), name


def test_rows_that_take_no_part_leave_the_bytes_of_the_cloud_without_them():
    c = tc.case("bad_rows")
    part = tc.rows_taking_part(c["points"], c["normals"], c["weights"])
    assert (~part).sum() == tc.BAD_ROWS and part.sum() == tc.SMALL_POINTS
    bp, bn, bw = tc.bad_rows()
    assert not tc.rows_taking_part(bp, bn, bw).any()
    only = _run(c, points=c["points"][part], normals=c["normals"][part], weights=c["weights"][part])
    assert tc.state_bytes(only) == tc.state_bytes(tc.case_reference("bad_rows"))
    assert c["weights"][part].max() == 256.0                 # (the largest weight that takes part does)
    nothing = _run(c, points=bp, normals=bn, weights=bw)
    assert not nothing["updated"].any() and not nothing["count"].any()


def test_a_voxel_out_of_reach_keeps_its_bits_nan_payloads_included():
    c = tc.case("outside")
    nx, ny, nz = c["dims"]
    for word in (0x7FC12345, 0xFFFFFFFF, 0x7B7B7B7B, 0x80000000):
        prior = np.full((nz, ny, nx), word, np.uint32).view(np.float32)
        r = _run(c, state=(prior, prior.copy(), None))
        out = ~r["updated"]
        assert out.sum() > 150 and r["updated"].sum() == 13
        for k in ("sdf_sum", "weight"):
            assert (r[k].view(np.uint32)[out] == word).all(), (k, hex(word))
    # the far point reaches nothing; the near one reaches the first planes of voxels only
    assert not tc.case_reference("outside")["updated"][3:].any() and tc.case_reference("outside")["updated"][0].any()


def test_reach_edges_duplicates_clamps_and_the_limit():
    r = tc.case_reference("brick_border")
    # at d2 == r2 a row is accepted with phi = 0: counted, and the voxel keeps its bits
    for at in ((4, 4, 8), (4, 4, 12), (4, 5, 7), (4, 8, 3)):
        assert r["count"][at] == 1 and r["sum_a"][at] == 0 and not r["updated"][at], at
    assert r["count"][4, 4, 7] == 0 and r["count"][4, 4, 13] == 0 and r["count"][4, 5, 8] == 0
    # a duplicated row counts as often as it appears
    once, more = tc.case_reference("one_8x8x8"), tc.case("one_8x8x8")
    twice = _run(more, points=np.repeat(more["points"], 2, 0), normals=np.repeat(more["normals"], 2, 0))
    assert np.array_equal(twice["sum_a"], 2 * once["sum_a"]) and np.array_equal(twice["sum_at"], 2 * once["sum_at"])
    # non-unit normals clamp at +-trunc; a NaN s (inf - inf) is -trunc
    c, r = tc.case("non_unit"), tc.case_reference("non_unit")
    seen = r["weight"] > 0
    assert (np.abs(r["sdf_sum"][seen] / r["weight"][seen]) <= np.float32(c["trunc"]) * (1 + 2 ** -22)).all()
    o = tc.case_reference("overflow")
    assert o["count"][0, 0, 0] == 2 and o["sum_at"][0, 0, 0] < 0 and np.isfinite(o["sdf_sum"]).all()
    lim = tc.case_reference("limit")
    assert lim["count"].reshape(-1).tolist() == [tc.MAX_ROWS, tc.MAX_ROWS + 1]
    assert lim["updated"].reshape(-1).tolist() == [True, False] and lim["weight"].reshape(-1)[1] == 0
    e = tc.case_reference("empty")
    assert tc.state_bytes(e) == tc.state_bytes(tc.case("empty")["state"])


def test_colours_invert_the_uint8_conversion_and_the_prior_state_is_added_to():
    c, r = tc.case("colours"), tc.case_reference("colours")
    seen = r["weight"] >= 1.0
    with np.errstate(all="ignore"):
        back = (r["color_sum"] / r["weight"] + 1.0) * 127.5      # what extract_mesh converts
    assert (back[:, seen] >= -1e-3).all() and (back[:, seen] <= 255 + 1e-3).all()
    one = tc.tsdf_cloud_reference(c["points"][:1], c["normals"][:1], c["radius"], c["dims"], c["voxel_size"], c["origin"],
                                  c["trunc"], colors=c["colors"][:1])
    hit = one["weight"] > 0.01
    with np.errstate(all="ignore"):
        back = (one["color_sum"] / one["weight"] + 1.0) * 127.5
    assert hit.any() and (np.abs(back[:, hit] - c["colors"][0][:, None]) <= 1e-2).all()
    p, ref = tc.case("prior"), tc.case_reference("prior")
    fresh = _run(p, state=None)
    upd = ref["updated"]
    assert upd.any() and (~upd).any() and (p["state"][1] > 0)[upd].any()
    total = p["state"][1].astype(np.float64) + fresh["weight"].astype(np.float64)
    assert (np.abs(ref["weight"][upd] - total[upd]) <= 2 * EPS * total[upd]).all()
    assert tc.state_bytes((ref["sdf_sum"][~upd], ref["weight"][~upd], None)) == \
        tc.state_bytes((p["state"][0][~upd], p["state"][1][~upd], None))
