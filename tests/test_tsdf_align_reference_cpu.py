"""The restatement of the alignment (tests/tsdf_align_reference.py) against itself and against analysis, without a GPU:
its Jacobian is the derivative of its residual under the stated update, an exactly linear field at the true pose gives
b = 0, the conditions on the inputs of the device test hold, and its loop converges on the end-to-end scene."""
import math

import numpy as np
import pytest

import tsdf_align_reference as ar
from tsdf_raycast_reference import _corner, _trilinear, camera
from tsdf_reference import BORDERLINE_CAP


def test_camera_from_pose_is_the_raycast_camera_on_float32_poses():
    c = ar.align_case("sphere_rolled_23x31")
    A, g0 = camera(c["K"][0], c["T"][0], c["voxel_size"], c["origin"])
    A2, g02 = ar.camera_from_pose(c["K"][0], *ar.pose_of(c["T"][0]), c["voxel_size"], c["origin"])
    assert A.tobytes() == A2.tobytes() and g0.tobytes() == g02.tobytes()


@pytest.mark.parametrize("name", ["sphere_rolled_23x31", "hole_rolled_23x31", "valid_weights_rolled_23x31"])
def test_jacobian_is_the_derivative_of_the_residual(name):
    """r(delta) at a pixel: the point moves to g' = c0 + exp([omega]x) (g - c0) + v and the residual is the cell's own
    trilinear polynomial there over the voxel size.  Central differences with h = 1e-5 carry a truncation error of
    h^2 / 6 times a third derivative (the polynomial's are bounded by its coefficients times |q|^3: below 1e-6 here) and a
    rounding error of 1e-16 / h = 1e-11."""
    c = ar.align_case(name)
    ref = ar.reference(name)[0]
    grid = ar.case_grid(c)
    vs = float(np.float32(c["voxel_size"]))
    c0 = (grid.dims.astype(np.float64) - 1.0) / 2.0
    dv = [_corner(grid.d, k, ref["index"]) for k in range(8)]
    base = np.stack([ref["index"][a].astype(np.float64) for a in range(3)])

    def residual(delta):
        q = ref["g"] - c0[:, None, None]
        g = c0[:, None, None] + np.einsum("ab,bhw->ahw", ar.rotation(delta[3:]), q) + delta[:3, None, None]
        return _trilinear(dv, g - base) / vs
    sel = ref["takes_part"]
    assert sel.sum() >= 300
    h = 1e-5
    worst = 0.0
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        diff = (residual(e) - residual(-e)) / (2 * h)
        worst = max(worst, float(np.abs(diff - ref["J"][i])[sel].max()))
    assert worst <= 1e-6, worst


def test_the_pose_update_is_the_update_of_the_points():
    """A point of the camera at the updated pose is c0 + Rd (g - c0) + v in grid coordinates."""
    c = ar.align_case("sphere_rolled_23x31")
    grid = ar.case_grid(c)
    R, t = ar.pose_of(c["T"][0])
    delta = np.array([0.3, -0.2, 0.25, 0.01, -0.02, 0.015])
    R2, t2 = ar.apply_update(R, t, delta, grid.dims, c["voxel_size"], c["origin"])
    vs, o = float(np.float32(c["voxel_size"])), np.asarray(c["origin"], np.float32).astype(np.float64)
    c0 = (grid.dims.astype(np.float64) - 1.0) / 2.0
    rng = np.random.default_rng(3)
    for xc in rng.normal(size=(5, 3)):
        g = (R @ xc + t - o) / vs
        g2 = (R2 @ xc + t2 - o) / vs
        np.testing.assert_allclose(g2, c0 + ar.rotation(delta[3:]) @ (g - c0) + delta[:3], atol=1e-12)
    for omega in (delta[3:], 1e-5 * delta[3:], np.zeros(3)):          # (both branches of the series, and none)
        Rd = ar.rotation(omega)
        np.testing.assert_allclose(Rd @ Rd.T, np.eye(3), atol=1e-14)


def test_a_linear_field_at_the_true_pose_gives_no_gradient():
    """d = a.p - c exactly representable on the grid (dyadic numbers) and a depth map that puts every pixel exactly on
    its zero set: the trilinear interpolant of a linear field is the field, so r = 0 up to the rounding of the points
    and b vanishes against its own bound."""
    dims, vs = (12, 11, 10), 0.125
    k, j, i = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    a = np.array([0.25, -0.5, 1.0])
    s = ((a[0] * i + a[1] * j + a[2] * k) * vs - 0.5).astype(np.float32)
    w = np.ones_like(s)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (0.7, 0.65, -1.0)
    H, W = 17, 19
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 40.0
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    o, v = ar._rays(K, T, (H, W))
    depth = ((0.5 - a @ o) / (v * a[:, None, None]).sum(0)).astype(np.float32)       # a.(o + D v) = 0.5
    ref = ar.align_system_reference(ar.grid_of(s, w, 1.0), vs, (0.0, 0.0, 0.0), depth, K, T, band=0.2)
    assert ref["count"] == H * W and not ref["borderline"].any()
    # the depth is rounded to fp32 (EPS D |a.v| of residual) and so is the camera (m_f): r is within that of 0
    slack = ref["r_bound"] + 2.0 ** -24 * depth * np.abs((v * a[:, None, None]).sum(0)) / vs
    assert (np.abs(ref["r"]) <= slack).all()
    assert (np.abs(ref["b"]) <= (np.abs(ref["J"]) * slack).reshape(6, -1).sum(1)).all()
    assert np.abs(ref["b"]).max() <= 1e-3 and np.abs(np.diag(ref["H"])).min() > 1.0


@pytest.mark.parametrize("name", ar.CASE_IDS)
def test_conditions_on_the_inputs(name):
    c = ar.align_case(name)
    for v, ref in enumerate(ar.reference(name)):
        lattice = int(ref["lattice"].sum())
        assert lattice == sum(1 for y in range(0, c["size"][0], c["kw"]["stride"]) for x in range(0, c["size"][1], c["kw"]["stride"]))
        assert not ref["takes_part"][~ref["lattice"]].any()
        if not c["hits"]:
            assert ref["count"] == 0
            continue
        assert ref["borderline"].sum() <= BORDERLINE_CAP * lattice, (name, v)
        assert ref["count"] >= 0.1 * lattice, (name, v)
        assert c["small"] == (lattice < 100)
        if not c["small"]:
            assert ref["count"] >= 100, (name, v)
        assert np.isfinite(ref["H_bound"]).all() and np.isfinite(ref["b_bound"]).all()
        # the perturbation is about half a voxel and half a degree
        dt, da = ar.pose_error(c["T"][v], c["T_true"][v])
        assert 0.03 <= dt <= 0.07 and math.radians(0.3) <= da <= math.radians(0.7)


def test_the_pixels_that_must_not_take_part_do_not():
    c = ar.align_case("bad_depths_outside_23x31")
    ref = ar.reference("bad_depths_outside_23x31")[0]
    bad = ~(np.isfinite(c["depth"][0]) & (c["depth"][0] > 0))
    plain = ar.reference("sphere_outside_23x31")[0]
    assert (bad & plain["takes_part"]).sum() >= 4 and not ref["takes_part"][bad].any()
    c = ar.align_case("valid_weights_rolled_23x31")
    ref = ar.reference("valid_weights_rolled_23x31")[0]
    wt = c["kw"]["weights"][0]
    off = ~c["kw"]["valid"][0] | ~(np.isfinite(wt) & (wt > 0))
    assert off.sum() >= 50 and not ref["takes_part"][off].any()
    hole, plain = ar.reference("hole_rolled_23x31")[0], ar.reference("sphere_rolled_23x31")[0]
    assert plain["count"] - hole["count"] >= 50
    for other in ("nan_under_weight_0_rolled_23x31", "min_weight_rolled_23x31"):
        assert (ar.reference(other)[0]["takes_part"] == hole["takes_part"]).all()


def test_the_plane_state_has_three_zero_columns():
    s, w, vs, origin = ar.plane_state()
    depth, K, T = ar.plane_view()
    ref = ar.align_system_reference(ar.grid_of(s, w, 1.0), vs, origin, depth[0], K[0], T[0], band=0.1)
    assert ref["count"] >= 100
    for i in (0, 1, 5):
        assert not ref["H"][i].any() and not ref["H"][:, i].any()
    assert ar.solve_reference(ref["H"], ref["b"], ref["count"])[0] == 2
    assert ar.solve_reference(ref["H"], ref["b"], 5)[0] == 1


def test_the_loop_converges_on_the_corner_scene():
    K, T, depth = ar.corner_views()
    assert not (depth == 0).any()
    out = ar.corner_loop(ar.corner_state())
    start = ar.pose_error(ar.corner_start(), T[3])
    final = ar.pose_error(out["T"], T[3])
    hist = out["history"]
    print(f"corner scene: start {start[0]:.4f} / {math.degrees(start[1]):.3f} deg, after {ar.CORNER_ITERATIONS} iterations "
          f"{final[0]:.4f} / {math.degrees(final[1]):.3f} deg; sum w r^2 {hist[0, 2]:.2f} -> {hist[-1, 2]:.4f}; "
          f"count {int(hist[0, 0])} -> {int(hist[-1, 0])}; step bounds (voxels, rad) {[('%.1e' % a, '%.1e' % b) for a, b in out['step_bounds']]}")
    # about one voxel and one degree off, inside the band of 1.5 voxels
    assert 0.08 <= start[0] <= 0.12 and math.radians(0.7) <= start[1] <= math.radians(1.2)
    assert out["status"] == 0 and hist[0, 0] >= 0.5 * depth[3].size
    # converged: the last update is far below the first, the cost fell by an order of magnitude, and the pose is closer
    # to the truth in both parts (how close is the volume's accuracy, recorded in DESIGN.md section 17, not asked here)
    assert final[0] < 0.25 * start[0] and final[1] < 0.5 * start[1]
    assert hist[-1, 2] < 0.1 * hist[0, 2]
    last = np.linalg.norm(out["poses"][-1][1] - out["poses"][-2][1])
    assert last < 1e-3 * np.linalg.norm(out["poses"][1][1] - out["poses"][0][1])
    assert np.isfinite(out["step_bounds"]).all()
    # sum w r^2 does not increase between consecutive rows by more than its own bound
    for i in range(len(hist) - 1):
        slack = out["systems"][i]["sum_w_r2_bound"] + out["systems"][i + 1]["sum_w_r2_bound"]
        assert hist[i + 1, 2] <= hist[i, 2] + slack, i
