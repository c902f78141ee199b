"""The alignment of depth maps to the TSDF volume on the device (csrc/mvsn_tsdf_align.hip) against the numpy restatement
(tests/tsdf_align_reference.py): which pixels take part, the residual map and the sums of one evaluation within the
derived bounds, one step within the bound that |H^-1| carries, the two ways a view stops, the exact properties
(repeatable, a view alone = the view among others, the state-level function = the method, iterations = 0, the history
rows) and the corner scene end to end.  Inputs sit in poisoned buffers, every output and the workspace between guard bands.

Figures of one MI355X run are in DESIGN.md section 17."""
import functools
import math

import numpy as np
import pytest
import torch

import tsdf_align_reference as ar
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard, bits_equal
from multi_view_stereonet_amd import _native, tsdf
from multi_view_stereonet_amd.tsdf import TSDFVolume
from tsdf_reference import EPS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _entry(c, fill, iterations=None, min_pixels=6, min_pivot=1e-9):
    """mvsn_tsdf_align_system (iterations None) or mvsn_tsdf_align on the inputs of a case dict, every input in a poisoned
    buffer of its own (16-byte aligned only), the outputs and the workspace carved between guard bands: numpy arrays."""
    s_np, w_np = c["state"]
    nz, ny, nx = s_np.shape
    V, (H, W) = c["K"].shape[0], c["size"]
    kw = c["kw"]
    guard = Guard(_alloc, fill)
    put = lambda a: None if a is None else guard.poisoned(_to(a))   # noqa: E731
    s, w, depth, K, T = put(s_np), put(w_np), put(c["depth"]), put(c["K"]), put(c["T"])
    valid = put(None if kw["valid"] is None else kw["valid"].astype(np.uint8))
    weights = put(kw["weights"])
    lib = _native.load()
    ws_bytes = lib.mvsn_tsdf_align_workspace_bytes(nx, ny, nz, V, H, W, kw["stride"])
    assert ws_bytes >= 4 * nx * ny * nz + 96 * V + 240 * V * ar.records_per_view((H, W), kw["stride"])
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    o = np.asarray(c["origin"], np.float32)
    f = lambda x: float(np.float32(x))   # noqa: E731
    head = (_native.ptr(s), _native.ptr(w), nx, ny, nz, f(c["voxel_size"]), float(o[0]), float(o[1]), float(o[2]),
            _native.ptr(depth), _native.ptr(valid), _native.ptr(weights), _native.ptr(K), _native.ptr(T), V, H, W,
            kw["stride"], f(c["min_weight"]), f(kw["band"]))
    with torch.cuda.device(DEV):
        if iterations is None:
            Hm, b = guard.empty((V, 6, 6), torch.float64, DEV), guard.empty((V, 6), torch.float64, DEV)
            sums, res = guard.empty((V, 3), torch.float64, DEV), guard.empty((V, 1, H, W), torch.float32, DEV)
            _native.check(lib.mvsn_tsdf_align_system(*head, _native.ptr(ws), ws_bytes, _native.ptr(Hm), _native.ptr(b),
                                                     _native.ptr(sums), _native.ptr(res), _native.stream()),
                          "mvsn_tsdf_align_system")
            out = {"H": Hm, "b": b, "sums": sums, "residual": res}
        else:
            To, hist = guard.empty((V, 4, 4), torch.float32, DEV), guard.empty((V, iterations + 1, 3), torch.float64, DEV)
            status, info = guard.empty((V,), torch.int32, DEV), guard.empty((V, 6, 6), torch.float64, DEV)
            _native.check(lib.mvsn_tsdf_align(*head, iterations, min_pixels, min_pivot, _native.ptr(ws), ws_bytes,
                                              _native.ptr(To), _native.ptr(hist), _native.ptr(status), _native.ptr(info),
                                              _native.stream()), "mvsn_tsdf_align")
            out = {"T": To, "history": hist, "status": status, "information": info}
    torch.cuda.synchronize()
    guard.check()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _device_system(name, fill=POISON_NAN):
    """Made once per (case, poison), never modified."""
    return _entry(ar.align_case(name), fill)


@pytest.mark.parametrize("name", ar.CASE_IDS)
def test_system_matches_the_restatement(name):
    c = ar.align_case(name)
    got = _device_system(name)
    vs = float(np.float32(c["voxel_size"]))
    for v, own in enumerate(ar.reference(name)):
        res = got["residual"][v, 0].astype(np.float64)
        took = ~np.isnan(res)
        assert not took[~own["lattice"]].any(), "a pixel off the lattice has a residual"
        clear = ~own["borderline"]
        np.testing.assert_array_equal(took[clear], own["takes_part"][clear], err_msg="takes part differs off the borderline pixels")
        # the restatement with the device's own decision on the borderline pixels only
        ref = ar.case_reference(c, v, decided=took) if own["borderline"].any() else own
        assert not ref["unresolved"].any()
        sel = ref["takes_part"]
        assert int(got["sums"][v, 0]) == ref["count"] == int(took.sum())
        ratios = {}
        # (m_f / voxel_size as it stands covers the division's own rounding: m_f keeps 3 EPS D of room and |f| <= D)
        ratios["residual"] = float((np.abs(res - ref["r"])[sel] / (ref["m_f"][sel] / vs)).max()) if sel.any() else 0.0

        def ratio(err, bound):
            err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
            assert (err[bound == 0] == 0).all()
            return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        ratios["H"] = ratio(np.abs(got["H"][v] - ref["H"]), ref["H_bound"])
        ratios["b"] = ratio(np.abs(got["b"][v] - ref["b"]), ref["b_bound"])
        ratios["sum_w"] = ratio(abs(got["sums"][v, 1] - ref["sum_w"]), ref["sum_w_bound"])
        ratios["sum_w_r2"] = ratio(abs(got["sums"][v, 2] - ref["sum_w_r2"]), ref["sum_w_r2_bound"])
        print(f"{name}[{v}]: {ref['count']} of {int(ref['lattice'].sum())} lattice pixels take part, "
              f"{int(own['borderline'].sum())} borderline; error / bound max: " + ", ".join(f"{k} {x:.3g}" for k, x in ratios.items()))
        assert np.array_equal(got["H"][v], got["H"][v].T)
        assert all(x <= 1 for x in ratios.values()), ratios


@pytest.mark.parametrize("name", ["shape_1x1", "shape_1x1029", "views3_37x61", "stride3_rolled_17x9", "stride2_views3_37x61",
                                  "valid_weights_rolled_23x31", "bad_depths_outside_23x31", "nan_under_weight_0_rolled_23x31",
                                  "away_23x31"])
def test_buffers_under_both_poisons(name):
    # (the guard bands of every buffer are checked inside _entry; an element nobody writes, or a read of foreign memory
    # that reaches a result, differs between the two fills)
    a, b = _device_system(name, POISON_NAN), _device_system(name, POISON_FINITE)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    c = ar.align_case(name)
    la, lb = _entry(c, POISON_NAN, iterations=2), _entry(c, POISON_FINITE, iterations=2)
    for key in la:
        assert la[key].tobytes() == lb[key].tobytes(), key
    # the first history row and, where no view moved, the normal matrix are the single evaluation's
    assert la["history"][:, 0].tobytes() == np.ascontiguousarray(a["sums"]).tobytes()
    if not c["hits"]:
        assert la["status"].tolist() == [1] * len(la["status"]) and not la["history"].any()
        assert la["T"].tobytes() == c["T"].tobytes()


def _corner_case(state):
    K, T, depth = ar.corner_views()
    return {"state": state, "min_weight": 1.0, "voxel_size": ar.CORNER["voxel_size"], "origin": ar.CORNER["origin"],
            "depth": depth[3:4], "K": K[3:4], "T": ar.corner_start()[None], "size": ar.CORNER["size"],
            "kw": dict(band=ar.CORNER_BAND, stride=1, valid=None, weights=None)}


def _pose_within(T_dev, T_ref, x, t, c):
    """The device pose against the restatement's within what an update off by x (2-norm) allows."""
    dims = c["state"][0].shape[::-1]
    bt, br = ar.pose_bound(x, t, dims, c["voxel_size"], c["origin"])
    et = float(np.linalg.norm(T_dev[:3, 3].astype(np.float64) - T_ref[:3, 3]))
    er = float(np.linalg.norm(T_dev[:3, :3].astype(np.float64) - T_ref[:3, :3], 2))
    return et, bt, er, br


@pytest.mark.parametrize("which", ["corner", "sphere_rolled_23x31"])
def test_one_step_is_the_restatements(which):
    c = _corner_case(ar.corner_state()) if which == "corner" else ar.align_case(which)
    got = _entry(c, POISON_NAN, iterations=1)
    grid = ar.grid_of(c["state"][0], c["state"][1], c["min_weight"])
    out = ar.align_reference(grid, c["voxel_size"], c["origin"], c["depth"][0], c["K"][0], c["T"][0], band=c["kw"]["band"],
                             iterations=1)
    assert got["status"][0] == out["status"] == 0
    assert not out["systems"][0]["borderline"].any()
    x = out["step_bounds"][0]
    R, t = out["poses"][1]
    T_ref = np.eye(4)
    T_ref[:3, :3], T_ref[:3, 3] = R, t
    et, bt, er, br = _pose_within(got["T"][0], T_ref, x, t, c)
    print(f"one step, {which}: update bounds {x[0]:.3e} voxels, {x[1]:.3e} rad; translation off by {et:.3e} (bound {bt:.3e}), "
          f"rotation by {er:.3e} (bound {br:.3e}); the step moved the pose by {np.abs(t - ar.pose_of(c['T'][0])[1]).max():.3e}")
    assert np.isfinite(x).all() and et <= bt and er <= br
    assert got["T"][0, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert got["history"][0, 0, 0] == out["history"][0, 0]


def test_a_plane_stops_with_status_2_and_a_view_that_sees_nothing_with_status_1():
    s, w, vs, origin = ar.plane_state()
    depth, K, T = ar.plane_view()
    c = {"state": (s, w), "min_weight": 1.0, "voxel_size": vs, "origin": origin, "depth": depth, "K": K, "T": T,
         "size": depth.shape[1:], "kw": dict(band=0.1, stride=1, valid=None, weights=None)}
    one = _entry(c, POISON_NAN)
    assert one["sums"][0, 0] >= 100 and one["sums"][0, 2] > 0
    for i in (0, 1, 5):                                       # n_x = n_y = (q x n)_z = 0 exactly
        assert not one["H"][0, i].any() and not one["H"][0, :, i].any()
    assert one["H"][0, 2, 2] > 0 and one["H"][0, 3, 3] > 0 and one["H"][0, 4, 4] > 0
    got = _entry(c, POISON_NAN, iterations=3)
    assert got["status"].tolist() == [2]
    assert got["T"].tobytes() == T.tobytes()
    assert (got["history"][0] == got["history"][0, 0]).all() and got["history"][0, 0].tobytes() == one["sums"][0].tobytes()
    assert got["information"].tobytes() == one["H"].tobytes()
    # too few pixels comes first: the same view with min_pixels above its count
    few = _entry(c, POISON_NAN, iterations=3, min_pixels=int(one["sums"][0, 0]) + 1)
    assert few["status"].tolist() == [1] and few["T"].tobytes() == T.tobytes()
    away = ar.align_case("away_23x31")
    got = _entry(away, POISON_NAN, iterations=3)
    assert got["status"].tolist() == [1] and got["T"].tobytes() == away["T"].tobytes()
    assert not got["history"].any() and not got["information"].any()


def _sphere_volume(c):
    s, w = c["state"]
    nz, ny, nx = s.shape
    vol = TSDFVolume((nx, ny, nz), c["voxel_size"], c["origin"], 2 * c["kw"]["band"], device=DEV)
    vol.sdf_sum.copy_(torch.from_numpy(s))
    vol.weight.copy_(torch.from_numpy(w))
    return vol


def test_reproducible_view_by_view_and_on_the_state():
    c = ar.align_case("views3_37x61")
    vol = _sphere_volume(c)
    depth, K, T = _to(c["depth"])[:, None].contiguous(), _to(c["K"]), _to(c["T"])
    N = 3
    whole = vol.align(depth, K, T, iterations=N)              # band None: trunc / 2
    assert isinstance(whole, tsdf.TSDFAlignment) and whole.history.shape == (3, N + 1, 3)
    again = vol.align(depth, K, T, iterations=N)
    state = tsdf.align(vol.sdf_sum, vol.weight, vol.voxel_size, vol.origin, depth, K.double(), T.double(),
                       band=c["kw"]["band"], iterations=N)
    entry = _entry(c, POISON_NAN, iterations=N)
    for a, b, s, key in zip(whole, again, state, ("T", "history", "status", "information")):
        assert bits_equal(a, b) and bits_equal(a, s), key
        assert a.cpu().numpy().tobytes() == entry[key].tobytes(), key
    for v in range(3):
        one = vol.align(depth[v:v + 1], K[v:v + 1], T[v:v + 1], iterations=N)
        for a, b in zip(whole, one):
            assert bits_equal(a[v:v + 1], b)
    # one evaluation: the function, twice, a view alone, and the C entry
    sysm = tsdf.align_system(vol.sdf_sum, vol.weight, vol.voxel_size, vol.origin, depth, K, T, band=c["kw"]["band"],
                             with_residual=True)
    twice = tsdf.align_system(vol.sdf_sum, vol.weight, vol.voxel_size, vol.origin, depth, K, T, band=c["kw"]["band"],
                              with_residual=True)
    ent = _device_system("views3_37x61")
    assert sysm[2].dtype == torch.int64 and sysm[5].shape == (3, 1, 37, 61)
    for a, b in zip(sysm, twice):
        assert bits_equal(a, b)
    assert sysm[0].cpu().numpy().tobytes() == ent["H"].tobytes() and sysm[1].cpu().numpy().tobytes() == ent["b"].tobytes()
    assert sysm[5].cpu().numpy().tobytes() == ent["residual"].tobytes()
    assert sysm[2].tolist() == ent["sums"][:, 0].tolist() and sysm[3].tolist() == ent["sums"][:, 1].tolist()
    assert sysm[4].tolist() == ent["sums"][:, 2].tolist()
    for v in range(3):
        one = tsdf.align_system(vol.sdf_sum, vol.weight, vol.voxel_size, vol.origin, depth[v:v + 1], K[v:v + 1], T[v:v + 1],
                                band=c["kw"]["band"], with_residual=True)
        for a, b in zip(sysm, one):
            assert bits_equal(a[v:v + 1], b)
    assert tsdf.align_system(vol.sdf_sum, vol.weight, vol.voxel_size, vol.origin, depth, K, T, band=c["kw"]["band"])[5] is None
    # iterations = 0: the float32 values of the input poses, one history row, the evaluation's sums
    zero = vol.align(depth, K.double(), T.double(), iterations=0)
    assert bits_equal(zero.T_cam_in_world, T) and zero.status.tolist() == [0, 0, 0] and zero.history.shape == (3, 1, 3)
    assert bits_equal(zero.information, sysm[0])
    assert zero.history[:, 0, 0].tolist() == sysm[2].tolist() and bits_equal(zero.history[:, 0, 1].contiguous(), sysm[3])
    assert bits_equal(zero.history[:, 0, 2].contiguous(), sysm[4])
    # history[:, i] is the evaluation at the pose after i updates: the last row of a run of i iterations, bit for bit
    # (both at the fp64 pose), and align_system at that run's fp32 pose within its bound widened by the pose's rounding
    grid = ar.case_grid(c)
    vs = float(np.float32(c["voxel_size"]))
    for i in range(N + 1):
        part = vol.align(depth, K, T, iterations=i)
        assert bits_equal(part.history[:, i].contiguous(), whole.history[:, i].contiguous()), i
        assert bits_equal(part.history[:, :i].contiguous(), whole.history[:, :i].contiguous()), i
        at = tsdf.align_system(vol.sdf_sum, vol.weight, vol.voxel_size, vol.origin, depth, K, part.T_cam_in_world,
                               band=c["kw"]["band"])
        if i == 0:
            assert bits_equal(at[4], whole.history[:, 0, 2].contiguous())
            continue
        Ti = part.T_cam_in_world.cpu().numpy()
        for v in range(3):
            ref = ar.align_system_reference(grid, c["voxel_size"], c["origin"], c["depth"][v], c["K"][v], Ti[v], band=c["kw"]["band"])
            # each of the pose's twelve numbers moves by at most EPS of itself: the point by EPS (|g0| + |D dir|_1) and room
            dg = 4.0 * EPS * (np.abs(ref["g"]).sum(0) + 2.0 * np.abs(np.asarray(c["origin"]) / vs).sum())
            dr = ref["r_bound"] + np.abs(ref["J"][:3]).sum(0) * dg
            slack = float((ref["w"] * (2.0 * np.abs(ref["r"]) * dr + dr * dr)).sum()) + ref["sum_w_r2_bound"]
            flips = int(ref["borderline"].sum()) + abs(int(at[2][v]) - int(whole.history[v, i, 0]))
            diff = abs(float(at[4][v]) - float(whole.history[v, i, 2]))
            print(f"history[{v},{i}]: sum w r^2 {float(whole.history[v, i, 2]):.6f}, align_system at the fp32 pose off by "
                  f"{diff:.2e} (bound {slack:.2e}), {flips} decisions may differ")
            if flips == 0:
                assert diff <= slack


def test_corner_scene_end_to_end():
    K, T, depth = ar.corner_views()
    vol = TSDFVolume(ar.CORNER["dims"], ar.CORNER["voxel_size"], ar.CORNER["origin"], ar.CORNER["trunc"], device=DEV)
    vol.integrate(_to(depth[:3])[:, None].contiguous(), _to(K[:3]), _to(T[:3]))
    start = ar.corner_start()
    n = ar.CORNER_ITERATIONS
    got = vol.align(_to(depth[3:4])[:, None].contiguous(), _to(K[3:4]), _to(start[None]), iterations=n)
    state = (vol.sdf_sum.cpu().numpy(), vol.weight.cpu().numpy())
    ref = ar.corner_loop(state, n)                            # the restatement's loop on the device's own state
    assert got.status.tolist() == [0] and ref["status"] == 0
    T_dev = got.T_cam_in_world[0].cpu().numpy()
    e0, e_dev, e_ref = ar.pose_error(start, T[3]), ar.pose_error(T_dev, T[3]), ar.pose_error(ref["T"], T[3])
    c = _corner_case(state)
    bt = br = 0.0
    for x, (R, t) in zip(ref["step_bounds"], ref["poses"][1:]):
        a, b = ar.pose_bound(x, t, ar.CORNER["dims"], ar.CORNER["voxel_size"], ar.CORNER["origin"])
        bt, br = bt + a, br + 2.0 * math.asin(min(1.0, b / 2.0))   # (|R1 - R2|_2 = 2 sin(angle / 2))
    hist = got.history[0].cpu().numpy()
    print(f"corner scene: start {e0[0]:.4f} / {math.degrees(e0[1]):.3f} deg; device {e_dev[0]:.6f} / {math.degrees(e_dev[1]):.4f} deg; "
          f"restatement {e_ref[0]:.6f} / {math.degrees(e_ref[1]):.4f} deg; summed bounds {bt:.3e} / {math.degrees(br):.3e} deg; "
          f"device - restatement pose max {np.abs(T_dev.astype(np.float64) - ref['T']).max():.3e}; "
          f"sum w r^2 {hist[0, 2]:.3f} -> {hist[-1, 2]:.5f}, count {int(hist[0, 0])} -> {int(hist[-1, 0])}")
    assert np.isfinite(ref["step_bounds"]).all()
    assert e_dev[0] <= e_ref[0] + bt and e_dev[1] <= e_ref[1] + br
    assert e_dev[0] < 0.25 * e0[0] and e_dev[1] < 0.5 * e0[1]
    for i in range(n):
        slack = ref["systems"][i]["sum_w_r2_bound"] + ref["systems"][i + 1]["sum_w_r2_bound"]
        assert hist[i + 1, 2] <= hist[i, 2] + slack, i
