"""The numpy restatement of cloud_render and cloud_visibility (tests/cloud_render_reference.py) held to things it was not
written from: the analytic depth of synthetic.fusion_scene, an independent fp64 occlusion computation, a plain Python loop
over the views, exact rational arithmetic for its fused multiply-add; and the named cases of
tests/test_cloud_render_gpu.py held to what their names say."""
import fractions
import functools

import numpy as np
import pytest

import cloud_render_reference as cr
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd.fusion import RENDER_MAX_RADIUS, VISIBILITY_MAX_CHANNELS, CloudRender, CloudVisibility

f32 = np.float32
ROWS, COLS, VIEWS = 48, 64, 3


def test_the_restatement_states_the_interfaces_limits_and_outputs():
    assert cr.MAX_RADIUS == RENDER_MAX_RADIUS and cr.MAX_CHANNELS == VISIBILITY_MAX_CHANNELS
    assert cr.RENDER_OUTPUTS == CloudRender._fields and cr.VISIBILITY_OUTPUTS == CloudVisibility._fields
    assert cr.CAMERA_BATCH == _native.load().mvsn_cloud_render_camera_batch()
    assert max(int(n.rsplit("_", 1)[1]) for n in cr.RADIUS_CASES) == RENDER_MAX_RADIUS
    assert max(int(n.rsplit("_", 1)[1]) for n in cr.VISIBILITY_CASES if n.startswith("channels_")) == VISIBILITY_MAX_CHANNELS


@functools.lru_cache(maxsize=None)
def _scene():
    """fusion_scene(3, 48, 64) and, per view, its depth back-projected in fp64 and rounded to fp32 (row-major pixels)."""
    s = {k: v.numpy() for k, v in synthetic.fusion_scene(VIEWS, ROWS, COLS).items()}
    K, T = s["K"].astype(np.float64), s["T_cam_in_world"].astype(np.float64)
    ys, xs = np.meshgrid(np.arange(ROWS, dtype=np.float64), np.arange(COLS, dtype=np.float64), indexing="ij")
    clouds = []
    for v in range(VIEWS):
        d = s["depth"][v, 0].astype(np.float64)
        cam = np.stack([(xs - K[v, 0, 2]) / K[v, 0, 0] * d, (ys - K[v, 1, 2]) / K[v, 1, 1] * d, d], -1).reshape(-1, 3)
        clouds.append((cam @ T[v, :3, :3].T + T[v, :3, 3]).astype(f32))
    assert (s["depth"] > 0).all()                                     # the plane fills every view
    return s, clouds


def test_fmaf_is_the_correctly_rounded_one():
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal(4000).astype(f32), rng.standard_normal(4000).astype(f32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -24)).astype(f32)     # heavy cancellation
    c[::3] = rng.standard_normal(len(c[::3])).astype(f32) * f32(1e-6)
    # products that end exactly half an ulp from an fp32 number, with a small c that breaks the tie either way
    a[:200] = f32(1 + 2.0 ** -12)
    b[:200] = f32(1 + 2.0 ** -12)
    c[:200] = (rng.choice([-1.0, 1.0], 200) * 2.0 ** rng.integers(-70, -40, 200)).astype(f32)
    got = cr.fmaf(a, b, c)
    for k in range(len(a)):
        exact = fractions.Fraction(float(a[k])) * fractions.Fraction(float(b[k])) + fractions.Fraction(float(c[k]))
        lo = f32(float(exact))                  # (float(Fraction) is correctly rounded to fp64; then find the neighbours)
        cands = sorted({float(np.nextafter(lo, f32(-np.inf))), float(lo), float(np.nextafter(lo, f32(np.inf)))})
        best = min(cands, key=lambda t: (abs(fractions.Fraction(t) - exact), int(f32(t).view(np.uint32)) & 1))
        assert float(got[k]) == best, (k, a[k], b[k], c[k])


def test_the_camera_is_section_15s():
    import tsdf_reference
    s, _ = _scene()
    K, T = cr.arc_cameras(5, 33, 65, seed=3)
    for Kc, Tc in ((s["K"], s["T_cam_in_world"]), (K, T)):
        P = cr.cameras(Kc, Tc).reshape(-1, 3, 4)
        want = tsdf_reference.cameras(Kc, Tc)                          # K inv(T) by LAPACK, fp64
        assert np.abs(P - want).max() <= 1e-6 * np.abs(want).max()
    Ks, Ts = cr.straight_camera(64.0, 3.0, 2.0)
    assert cr.cameras(Ks, Ts)[0].tolist() == [64, 0, 3, 0, 0, 64, 2, 0, 0, 0, 1, 0]


def test_each_view_renders_its_own_cloud_onto_itself():
    s, clouds = _scene()
    own = np.arange(ROWS * COLS).reshape(ROWS, COLS)
    for v in range(VIEWS):
        ref = cr.render_reference(clouds[v], s["K"][v:v + 1], s["T_cam_in_world"][v:v + 1], ROWS, COLS)
        assert (ref["index"][0] == own).all()
        rel = np.abs(ref["depth"][0].astype(np.float64) / s["depth"][v, 0] - 1)
        print("view", v, "worst relative depth error", rel.max())
        assert rel.max() <= 1e-6


def test_all_views_clouds_together_never_render_behind_the_surface():
    s, clouds = _scene()
    ref = cr.render_reference(np.concatenate(clouds), s["K"], s["T_cam_in_world"], ROWS, COLS)
    for v in range(VIEWS):
        d, want = ref["depth"][v].astype(np.float64), s["depth"][v, 0].astype(np.float64)
        assert (ref["index"][v] >= 0).all() and (d > 0).all()                      # every valid pixel is covered
        behind = int((d > 1.01 * want).sum())
        print("view", v, "behind", behind, "in front", int((d < 0.99 * want).sum()), "of", d.size)
        assert behind == 0                                             # a z-buffer can only come forward


def test_a_permuted_cloud_gives_the_same_depth_and_its_index_follows():
    s, clouds = _scene()
    cloud = np.concatenate(clouds)
    perm = cr.permutation(len(cloud))
    base = cr.render_reference(cloud, s["K"], s["T_cam_in_world"], ROWS, COLS, radius=1)
    moved = cr.render_reference(cloud[perm], s["K"], s["T_cam_in_world"], ROWS, COLS, radius=1)
    assert moved["depth"].tobytes() == base["depth"].tobytes()
    # where the z values that reach a pixel are distinct the winner is the same point
    keys = cr.render_keys(cloud, s["K"], s["T_cam_in_world"], ROWS, COLS, radius=1)
    assert (perm[moved["index"]] == base["index"]).mean() > 0.99
    tied = perm[moved["index"]] != base["index"]
    zbits = (keys >> np.uint64(32)).reshape(base["index"].shape)
    for v, r, c in zip(*np.nonzero(tied)):                             # a tie on z: both winners have the pixel's z
        P = cr.cameras(s["K"], s["T_cam_in_world"])[v]
        z2 = cr.project(P, cloud[[perm[moved["index"][v, r, c]]]])[0]
        assert z2.view(np.uint32)[0] == zbits[v, r, c]
    # and the contention case, all z distinct: the index follows the permutation everywhere
    c = cr.case("contention_distinct")
    perm = cr.permutation(cr.CONTENTION_N, 3)
    a = cr.case_reference("contention_distinct")
    b = cr.render_reference(c["points"][perm], c["K"], c["T"], c["rows"], c["cols"])
    assert b["depth"].tobytes() == a["depth"].tobytes() and (perm[b["index"][0, 2, 3]] == a["index"][0, 2, 3])


@pytest.mark.parametrize("name", cr.EXACT_CASES)
def test_every_rendered_row_is_visible_with_no_tolerance(name):
    c, ref = cr.visibility_case(name), cr.visibility_case_reference(name)
    index = c["index"]
    assert (index >= 0).any()
    for v in range(index.shape[0]):
        rows = index[v][index[v] >= 0]
        assert ref["visible"][rows, v].all(), v
    assert (ref["count"] == ref["visible"].sum(axis=1)).all()


def test_the_far_plane_is_visible_exactly_inside_the_hole():
    c, ref = cr.visibility_case("occlusion"), cr.visibility_case_reference("occlusion")
    c0, c1, r0, r1 = cr.OCCLUSION_HOLE
    # independent, fp64: the pixel a point falls into, from where it was placed (a quarter of a pixel off the centres)
    col, row = np.floor(c["pixel_x"] + 0.5), np.floor(c["pixel_y"] + 0.5)
    assert (np.abs(c["pixel_x"] + 0.5 - np.round(c["pixel_x"] + 0.5)) >= 0.2).all()      # no rounding decides a case
    inside = (col >= c0) & (col < c1) & (row >= r0) & (row < r1) & (col >= 0) & (col < 32) & (row >= 0) & (row < 24)
    assert ref["visible"][:, 0].astype(bool).tolist() == inside.tolist()
    assert 0 < inside.sum() == (c1 - c0) * (r1 - r0)
    # the near plane's own points are all visible
    near = cr.at_pixels(c["K"], c["pixel_x"], c["pixel_y"], 2.0)
    seen = cr.visibility_reference(near, c["depth"], c["K"], c["T"], 0.01)["visible"][:, 0].astype(bool)
    in_map = (col >= 0) & (col < 32) & (row >= 0) & (row < 24)
    assert seen.tolist() == in_map.tolist()


@pytest.mark.parametrize("name", ["channels_1", "channels_3", "channels_16", "bad_depth", "occlusion"])
def test_values_and_count_against_a_plain_loop(name):
    c, ref = cr.visibility_case(name), cr.visibility_case_reference(name)
    maps, visible = c["maps"], ref["visible"]
    V, C = maps.shape[:2]
    P = cr.cameras(c["K"], c["T"])
    taps = [cr.project(P[v], c["points"]) for v in range(V)]
    assert visible.any() and not visible.all()
    for i in range(len(c["points"])):
        total, n = [f32(0)] * C, 0
        for v in range(V):
            if visible[i, v]:
                col, row = int(taps[v][1][i]), int(taps[v][2][i])
                total = [f32(t + maps[v, ch, row, col]) for ch, t in enumerate(total)]
                n += 1
        assert ref["count"][i] == n
        want = [f32(t / f32(n)) if n else f32(0) for t in total]
        assert ref["values"][i].tobytes() == np.array(want, f32).tobytes(), i
    assert np.isfinite(ref["values"]).all()                            # no NaN of the maps or of the depth reaches a value


def test_the_tolerance_boundary_and_the_bad_depths():
    c, ref = cr.visibility_case("rel_tol"), cr.visibility_case_reference("rel_tol")
    assert ref["visible"][:, 0].tolist() == [1, 0, 1, 1]
    assert c["edge"] > f32(3.0) and float(c["edge"]) != 3.0 * (1 + 0.0123)             # an fp32 number of its own
    ref = cr.visibility_case_reference("bad_depth")
    assert ref["visible"].tolist() == [[0, 1, 1], [0, 1, 1], [0, 0, 1], [0, 0, 1], [1, 1, 1], [1, 0, 1], [1, 1, 1], [1, 1, 0]]


def test_colorize_is_fusions_conversion():
    values = np.array([[-1.0, 0.0, 1.0], [0.5, 2.0, -3.0], [np.nan, 1 / 255 - 1, 0.2]], f32)
    got = cr.colorize_reference(values, np.array([1, 2, 0]))
    assert got.tolist() == [[0, 128, 255], [191, 255, 0], [0, 0, 0]]
    assert cr.colorize_reference(values, np.array([1, 1, 1]))[2].tolist() == [0, 0, 153]


# ---- the named cases do what their names say -------------------------------------------------------------------------
def test_the_smallest_cases():
    hit, miss = cr.case_reference("one_hit"), cr.case_reference("one_miss")
    assert hit["depth"].tolist() == [[[2.0]]] and hit["index"].tolist() == [[[0]]]
    assert hit["colors"].reshape(-1).tolist() == [7, 8, 9] and hit["normals"].reshape(-1).tolist() == [0.0, f32(0.6), f32(-0.8)]
    assert miss["depth"].tolist() == [[[0.0]]] and miss["index"].tolist() == [[[-1]]]
    assert not miss["colors"].any() and not miss["normals"].any()


@pytest.mark.parametrize("name", cr.EDGE_CASES)
def test_the_edge_cases_hit_and_miss_in_every_view(name):
    c, ref = cr.case(name), cr.case_reference(name)
    assert c["K"].shape[0] in (31, 32, 33) and len(c["points"]) in (255, 256, 257)
    hit = ref["index"] >= 0
    assert hit.reshape(len(hit), -1).any(axis=1).all() and not hit.all()
    assert len(np.unique(ref["index"][hit])) < len(c["points"])          # some points lose or miss
    nog = cr.case_reference(name, False)
    assert nog["colors"] is None and nog["depth"].tobytes() == ref["depth"].tobytes()
    rows = ref["index"][0][hit[0]]
    assert (ref["colors"][0][:, hit[0]].T == c["colors"][rows]).all()


def test_the_contention_cases():
    for order in ("distinct", "ascending", "descending"):
        c, ref = cr.case("contention_" + order), cr.case_reference("contention_" + order)
        z = c["points"][:, 2]
        assert len(np.unique(z)) == cr.CONTENTION_N == 4099
        assert (ref["index"] >= 0).sum() == 1 and ref["index"][0, 2, 3] == np.argmin(z) and ref["depth"][0, 2, 3] == 2.0
    assert (np.diff(cr.case("contention_ascending")["points"][:, 2]) > 0).all()
    assert (np.diff(cr.case("contention_descending")["points"][:, 2]) < 0).all()
    ref = cr.case_reference("contention_equal")
    assert ref["index"][0, 2, 3] == 0 and ref["depth"][0, 2, 3] == 2.5 and (ref["index"] >= 0).sum() == 1


def test_the_rows_that_take_no_part():
    c, ref = cr.case("nonpart"), cr.case_reference("nonpart")
    rendered = set(ref["index"][ref["index"] >= 0].tolist())
    for name, (row, part) in cr.NONPART_ROWS.items():
        assert (row in rendered) == part, name
    where = {name: tuple(np.argwhere(ref["index"][0] == row)[0]) for name, (row, part) in cr.NONPART_ROWS.items() if part}
    assert where == {"plain": (1, 0), "at_max_depth": (1, 8), "half_up": (1, 11), "minus_half": (2, 0)}
    assert (ref["index"][0, 4] == np.arange(16) + len(cr.NONPART_ROWS)).all()           # the ordinary row is whole
    assert len(cr.NONPART_ROWS) == 16


def test_the_radius_cases():
    refs = {r: cr.case_reference("radius_%d" % r) for r in (0, 1, 2, 8)}
    pts = cr.case("radius_1")["points"]
    assert all(cr.case("radius_%d" % r)["points"].tobytes() == pts.tobytes() for r in refs)
    covered = [int((refs[r]["index"] >= 0).sum()) for r in (0, 1, 2, 8)]
    assert covered[0] < covered[1] < covered[2] < covered[3]
    # one pixel outside the map: in at R = 1, not at R = 0 (view 0)
    seen0, seen1 = set(refs[0]["index"][0].reshape(-1).tolist()), set(refs[1]["index"][0].reshape(-1).tolist())
    for row in cr.RADIUS_OUTSIDE_ROWS:
        assert row not in seen0 and row in seen1, row
    # the corners: clipped squares of (R + 1)^2 pixels at least
    assert refs[2]["index"][0, 0, 0] >= 0 and refs[2]["index"][0, 32, 64] >= 0
    # a nearer splat covers the farther point's centre pixel
    assert refs[0]["index"][0, 16, 10] == cr.RADIUS_FAR_ROW and refs[1]["index"][0, 16, 10] == cr.RADIUS_NEAR_ROW
    assert refs[1]["depth"][0, 16, 10] == 2.0 and refs[0]["depth"][0, 16, 10] == 4.0


def test_what_the_flat_splat_costs_on_the_slanted_plane():
    """a covered neighbour takes the point's own z, so at R = 1 the slanted plane comes forward."""
    s, clouds = _scene()
    cloud = np.concatenate(clouds)
    want = s["depth"][:, 0].astype(np.float64)
    depth = {}
    for radius in (0, 1, 2):
        d = cr.render_reference(cloud, s["K"], s["T_cam_in_world"], ROWS, COLS, radius=radius)["depth"].astype(np.float64)
        own = cr.render_reference(clouds[0], s["K"][:1], s["T_cam_in_world"][:1], ROWS, COLS, radius=radius)["depth"][0]
        print("radius", radius, "share of pixels more than 1 % in front: all clouds", float((d < 0.99 * want).mean()),
              "a view's own cloud", float((own < 0.99 * want[0]).mean()))
        assert not (d > 1.01 * want).any()
        depth[radius] = d
    # a larger square only adds candidates to a pixel: the depth can only come forward, and on this scene it does
    for small, large in ((0, 1), (1, 2)):
        assert (depth[large] <= depth[small]).all() and (depth[large] < depth[small]).any()
    assert (depth[1] < 0.99 * want).sum() > (depth[0] < 0.99 * want).sum()
