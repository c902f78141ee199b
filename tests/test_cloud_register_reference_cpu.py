"""The restatement of the cloud registration (tests/cloud_register_reference.py) against itself, without a GPU: its
Jacobian is the derivative of its own residual under the stated update, the update of the pose is the update of the
points, the conditions on the cases that keep the GPU tests from passing vacuously, and what the loop reaches on the
corner scene (the figures are in DESIGN.md section 20)."""
import math

import numpy as np
import pytest

import cloud_register_reference as rr
import tsdf_align_reference as ar
from cloud_reference import radius_scalars


def _moved(points, delta, centre):
    """Rd (p - c) + c + v in fp64: the stated update applied to points."""
    c = np.asarray(centre, np.float64)
    return (points - c) @ ar.rotation(delta[3:]).T + c + np.asarray(delta[:3], np.float64)


@pytest.mark.parametrize("mode", rr.MODES)
def test_jacobian_is_the_central_difference_of_the_residual(mode):
    c = rr.system_case("n257")
    ref = rr.register_system_reference(c["source"], c["target"], c["h"], T=c["T"], **rr.case_args(c, mode, False))
    sel = ref["takes_part"]
    assert sel.sum() >= 200
    p = ref["p"][sel].astype(np.float64)
    tgt = c["target"][ref["index"][sel]].astype(np.float64)
    nrm = c["normals"][ref["index"][sel]].astype(np.float64)

    def residuals(delta):
        d = _moved(p, delta, c["centre"]) - tgt              # the match held fixed
        return [(d * nrm).sum(axis=1)] if mode == "plane" else [d[:, 0], d[:, 1], d[:, 2]]
    at_zero = residuals(np.zeros(6))
    step = 1e-6
    q = np.abs(p - c["centre"].astype(np.float64)).max()
    for k, (r, J) in enumerate(ref["rows"]):
        # the fp32 residual is the fp64 one up to the roundings of p' - target and the dot product
        assert np.abs(r[sel] - at_zero[k]).max() <= 8 * 2.0 ** -24 * (np.abs(p).max() + 1.0)
        for i in range(6):
            e = np.zeros(6)
            e[i] = step
            numeric = (residuals(e)[k] - residuals(-e)[k]) / (2 * step)
            # the fp32 products of J (2^-24 relative, a few of them), the truncation (step^2) and the cancellation
            # (2^-53 / step) of the difference quotient, all times the lever
            assert np.abs(J[i, sel] - numeric).max() <= (1.0 + q) * (8 * 2.0 ** -24 + 10 * step ** 2 + 2.0 ** -50 / step), (k, i)


def test_the_update_of_the_pose_is_the_update_of_the_points():
    rng = np.random.default_rng(3)
    R, t = rr.pose_of(rr.general_pose())
    centre = np.array([0.3, -1.2, 0.7], np.float32)
    pts = rng.uniform(-2, 2, (50, 3))
    for delta in (np.array([0.02, -0.01, 0.03, 0.01, 0.02, -0.015]), np.array([0.0, 0.0, 0.0, 1e-6, 0.0, 2e-6]),
                  np.array([0.5, 0.1, -0.2, 0.4, -0.3, 0.2])):
        Rn, tn = rr.apply_update(R, t, delta, centre)
        assert np.abs((pts @ Rn.T + tn) - _moved(pts @ R.T + t, delta, centre)).max() <= 1e-13


def test_the_transform_is_fp32_in_the_stated_order():
    R32, t32 = rr.pose32(*rr.pose_of(rr.general_pose()))
    s = np.random.default_rng(1).uniform(-3, 3, (64, 3)).astype(np.float32)
    p = rr.transform32(R32, t32, s)
    assert p.dtype == np.float32
    for n in range(64):
        for a in range(3):
            want = np.float32(np.float32(np.float32(R32[a, 0] * s[n, 0]) + np.float32(R32[a, 1] * s[n, 1])) +
                              np.float32(R32[a, 2] * s[n, 2])) + t32[a]
            assert p[n, a] == want
    # the default centre: the fp64 mean of the finite rows, rounded once
    t = np.array([[1, 2, 3], [np.nan, 0, 0], [3, 2, 1], [0, np.inf, 0]], np.float32)
    assert rr.default_centre(t).dtype == np.float32 and rr.default_centre(t).tolist() == [2.0, 2.0, 2.0]
    assert rr.default_centre(np.full((2, 3), np.nan, np.float32)).tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("mode", rr.MODES)
def test_hand_case_holds_what_it_is_there_for(mode):
    c = rr.system_case("hand")
    assert c["source"].shape == (1027, 3) and c["target"].shape == (1031, 3) and c["h"] == 0.25
    ref = rr.system_reference("hand", mode, True)
    takes, index, res = ref["takes_part"], ref["index"], ref["residual"]
    r2 = radius_scalars(c["h"])[2]
    assert takes.sum() >= len(takes) // 4 and (~takes).sum() >= 16
    assert (index[takes] >= 0).all() and (index[~takes] == -1).all() and np.isnan(res[~takes]).all()
    assert not np.isnan(res[takes]).any()
    plain = rr.system_reference("hand", "point", False)             # the matches alone
    assert plain["index"][5] == 5 and plain["residual"][5] == 0          # on a target, the tie to the lowest duplicate
    assert plain["index"][6] == 700 and plain["residual"][6] == 0
    assert plain["index"][10] == 20 and plain["residual"][10] == r2      # d2 == r2 is within
    assert (plain["index"] == -1).sum() >= 100                            # sources with nothing in reach
    src, p, w = c["source"], ref["p"], c["weights"]
    assert np.isfinite(src[503]).all() and not np.isfinite(p[503]).all() and not takes[503]
    assert (~np.isfinite(src).all(axis=1)).sum() >= 3 and (~np.isfinite(c["target"]).all(axis=1)).sum() >= 3
    bad_w = ~(np.isfinite(w) & (w > 0))
    assert bad_w.sum() == 5 and (plain["index"][bad_w] >= 0).all() and not takes[bad_w].any()
    assert any(np.isnan(w[bad_w])) and any(w[bad_w] == 0) and any(w[bad_w] < 0) and np.isinf(w[bad_w]).sum() == 2
    bad_n = ~np.isfinite(c["normals"]).all(axis=1)
    lost = np.isin(plain["index"], np.flatnonzero(bad_n)) & ~bad_w
    assert bad_n.sum() == 3 and lost.sum() >= 3
    assert not takes[lost].any() if mode == "plane" else takes[lost].all()


@pytest.mark.parametrize("name", rr.SMALL_CASE_IDS)
@pytest.mark.parametrize("mode", rr.MODES)
def test_system_cases_have_points_that_take_part_and_positive_bounds(name, mode):
    c = rr.system_case(name)
    ref = rr.system_reference(name, mode, True)
    assert ref["count"] >= max(1, len(c["source"]) // 4)
    assert np.array_equal(ref["H"], ref["H"].T) and (np.diag(ref["H"]) > 0).all()
    assert (ref["H_bound"][np.abs(ref["H"]) > 0] > 0).all() and ref["sum_w_bound"] > 0 and ref["sum_w_r2_bound"] >= 0
    # the bound is an fp64 rounding bound: far below the sums it belongs to
    assert (ref["H_bound"] <= 1e-9 * np.sqrt(np.outer(np.diag(ref["H"]), np.diag(ref["H"])))).all()


def test_sizes_cover_the_kernels_paths():
    n = [len(rr.system_case(k)["source"]) for k in rr.SMALL_CASE_IDS]
    assert {1, 255, 256, 257, rr.BLOCK_POINTS + 1} <= set(n)
    assert rr.wrapping_points() == 1024 * 1024 + 1
    assert len(rr.system_case("m1")["target"]) == 1
    one = rr.system_case("one_cell_1027")
    cells = np.floor(one["target"] / np.float32(one["h"]))
    assert len(one["target"]) == 1027 and (cells == cells[0]).all()


@pytest.mark.parametrize("name", rr.STOP_IDS)
def test_stop_cases_stop_the_restatement(name):
    c = rr.stop_case(name)
    ref = rr.register_reference(c["source"], c["target"], c["h"], T_init=c["T"], normals=c["normals"], centre=c["centre"],
                                iterations=3, min_points=c["min_points"])
    assert ref["status"] == c["status"]
    assert np.array_equal(ref["T"], c["T"])                              # the input's pose bits
    assert (ref["history"] == ref["history"][0]).all()                   # the rows repeat
    H, count = ref["systems"][0]["H"], ref["systems"][0]["count"]
    if name == "out_of_reach":
        assert count == 0 and not H.any()
    elif name == "plane_z0":
        assert count >= 100 and (np.diag(H)[[0, 1, 5]] == 0).all() and (np.diag(H)[[2, 3, 4]] > 0).all()
    else:
        assert count == 2 and (np.diag(H) > 0).all()                     # not the diagonal: the pivot stops it
        assert ar.solve_reference(H, ref["systems"][0]["b"], count, 1, 1e-9)[0] == 2


def _errors(loop, T_true):
    return [rr.pose_error(rr.pose_matrix(R, t), T_true) for R, t in loop["poses"]]


def test_corner_scene_is_what_the_issue_describes():
    s = rr.corner_scene()
    assert s["target"].shape == (9216, 3) and s["normals"].shape == (9216, 3) and s["source"].shape == (3072, 3)
    assert np.abs(np.linalg.norm(s["normals"].astype(np.float64), axis=1) - 1).max() < 1e-6
    start = rr.pose_error(s["T_init"], s["T_true"])
    assert abs(start[0] - 0.0985) < 5e-4 and abs(math.degrees(start[1]) - 0.897) < 5e-3
    # at the true pose the source lies on the surfaces the target samples
    at = rr.register_system_reference(s["source"], s["target"], s["h"], T=s["T_true"], normals=s["normals"], centre=s["centre"])
    # (all but the sources next to an edge, whose nearest target may lie on the other surface)
    assert at["count"] == 3072 and np.median(np.abs(at["residual"])) < 1e-5 and np.abs(at["residual"]).max() < s["h"]


def test_corner_loop_plane_mode_converges():
    s = rr.corner_scene()
    loop = rr.corner_loop("plane")
    assert loop["status"] == 0 and (loop["history"][:, 0] == 3072).all()   # every source takes part at every iteration
    err = _errors(loop, s["T_true"])
    print("plane: " + " -> ".join(f"{a:.5f} / {math.degrees(b):.3f} deg" for a, b in err))
    print("plane sum w r^2: " + " ".join(f"{x:.4g}" for x in loop["history"][:, 2]))
    assert err[-1][0] <= err[0][0] / 10 and err[-1][1] <= err[0][1] / 10


def test_corner_loop_point_mode_descends():
    s = rr.corner_scene()
    loop = rr.corner_loop("point")
    assert loop["status"] == 0 and (loop["history"][:, 0] == 3072).all()
    err = _errors(loop, s["T_true"])
    print("point: " + " -> ".join(f"{a:.5f} / {math.degrees(b):.3f} deg" for a, b in err))
    print("point sum w r^2: " + " ".join(f"{x:.4g}" for x in loop["history"][:, 2]))
    cost, move = loop["history"][:, 2], np.array([e[0] for e in err])
    assert (np.diff(cost) <= 0).all() and (np.diff(move) <= 0).all()      # (nothing is asked of the rotation)
