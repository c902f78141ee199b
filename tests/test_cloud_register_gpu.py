"""The registration of one cloud to another on the device (csrc/mvsn_cloud_register.hip) against the numpy restatement
(tests/cloud_register_reference.py): the matches and the residual bits of one evaluation and its sums within the bound of
their order, one step within the bound that |H^-1| carries, the identities of the loop bit for bit, the ways a run stops,
the corner scene end to end, every buffer between guard bands under both poisons, and the order of either cloud.

Figures of one MI355X run are in DESIGN.md section 20."""
import functools
import math

import numpy as np
import pytest
import torch

import cloud_register_reference as rr
from cloud_reference import radius_scalars
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native, fusion
from multi_view_stereonet_amd.fusion import cloud_register, cloud_register_system

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(_bits(a[k]), _bits(b[k])), k


def _entry(source, target, h, T, *, normals=None, weights=None, centre, fill=POISON_NAN, iterations=None, min_points=6,
           min_pivot=1e-9):
    """mvsn_cloud_index_build, then mvsn_cloud_register_system (iterations None) or mvsn_cloud_register, every input in a
    poisoned buffer of its own (16-byte aligned only), both workspaces, the status word and every output carved between
    guard bands and poisoned too: numpy arrays."""
    hf, inv, r2 = radius_scalars(h)
    n, m = len(source), len(target)
    guard = Guard(_alloc, fill)
    put = lambda a: None if a is None else guard.poisoned(_to(a))   # noqa: E731
    s, t, nm, wt = put(source), put(target), put(normals), put(weights)
    T32, cen = put(np.asarray(T, np.float32)), put(np.asarray(centre, np.float32))
    lib = _native.load()
    idx_bytes, ws_bytes = lib.mvsn_cloud_workspace_bytes(m), lib.mvsn_cloud_register_workspace_bytes(n)
    assert ws_bytes >= 96 + 240 * min(-(-n // rr.BLOCK_POINTS), rr.MAX_BLOCKS)
    idx_ws, ws = guard.empty((idx_bytes,), torch.uint8, DEV), guard.empty((ws_bytes,), torch.uint8, DEV)
    status = guard.empty((1,), torch.int64, DEV)
    head = (_native.ptr(s), n, _native.ptr(wt), _native.ptr(t), _native.ptr(nm), m, float(inv), float(r2),
            _native.ptr(idx_ws), idx_bytes, _native.ptr(T32), _native.ptr(cen))
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_cloud_index_build(_native.ptr(t), m, float(hf), float(inv), _native.ptr(status),
                                                 _native.ptr(idx_ws), idx_bytes, st), "mvsn_cloud_index_build")
        if iterations is None:
            Hm, b, sums = (guard.empty(shape, torch.float64, DEV) for shape in ((6, 6), (6,), (3,)))
            index, res = guard.empty((n,), torch.int64, DEV), guard.empty((n,), torch.float32, DEV)
            _native.check(lib.mvsn_cloud_register_system(*head, _native.ptr(ws), ws_bytes, _native.ptr(Hm), _native.ptr(b),
                                                         _native.ptr(sums), _native.ptr(index), _native.ptr(res), st),
                          "mvsn_cloud_register_system")
            out = {"H": Hm, "b": b, "sums": sums, "index": index, "residual": res}
        else:
            To, hist = guard.empty((4, 4), torch.float32, DEV), guard.empty((iterations + 1, 3), torch.float64, DEV)
            run, info = guard.empty((1,), torch.int32, DEV), guard.empty((6, 6), torch.float64, DEV)
            _native.check(lib.mvsn_cloud_register(*head, iterations, min_points, min_pivot, _native.ptr(ws), ws_bytes,
                                                  _native.ptr(To), _native.ptr(hist), _native.ptr(run), _native.ptr(info), st),
                          "mvsn_cloud_register")
            out = {"T": To, "history": hist, "status": run, "information": info}
    torch.cuda.synchronize()
    guard.check()
    assert int(status.item()) == 0
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _device_system(name, mode, weighted, fill=POISON_NAN):
    """Made once per (case, mode, weights, poison), never modified."""
    c = rr.system_case(name)
    return _entry(c["source"], c["target"], c["h"], c["T"], fill=fill, **rr.case_args(c, mode, weighted))


def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _sums_within(got, ref):
    ratios = {"H": _ratio(np.abs(got["H"] - ref["H"]), ref["H_bound"]), "b": _ratio(np.abs(got["b"] - ref["b"]), ref["b_bound"]),
              "sum_w": _ratio(abs(got["sums"][1] - ref["sum_w"]), ref["sum_w_bound"]),
              "sum_w_r2": _ratio(abs(got["sums"][2] - ref["sum_w_r2"]), ref["sum_w_r2_bound"])}
    assert np.array_equal(got["H"], got["H"].T)
    return ratios


SYSTEM_RUNS = [(n, m, w) for n in rr.SMALL_CASE_IDS for m in rr.MODES for w in (True, False)] + \
    [("wrapping", m, True) for m in rr.MODES]


# ---- one evaluation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, mode, weighted", SYSTEM_RUNS)
def test_system_matches_the_restatement(name, mode, weighted):
    got, ref = _device_system(name, mode, weighted), rr.system_reference(name, mode, weighted)
    np.testing.assert_array_equal(got["index"], ref["index"])
    np.testing.assert_array_equal(got["residual"].view(np.uint32), ref["residual"].view(np.uint32))     # the bits
    assert got["sums"][0] == ref["count"] == int((got["index"] >= 0).sum())
    ratios = _sums_within(got, ref)
    print(f"{name} {mode} weights={weighted}: {ref['count']} of {len(ref['index'])} take part; error / bound max: " +
          ", ".join(f"{k} {x:.3g}" for k, x in ratios.items()))
    assert all(x <= 1 for x in ratios.values()), ratios


# ---- buffers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rr.MODES)
@pytest.mark.parametrize("name", ["n1", "hand", "one_cell_1027", "wrapping"])
def test_buffers_under_both_poisons(name, mode):
    # (the guard bands of every buffer are checked inside _entry; an element nobody writes, or a read of foreign memory
    # that reaches a result, differs between the two fills)
    _same_bits(_device_system(name, mode, True, POISON_NAN), _device_system(name, mode, True, POISON_FINITE))
    c = rr.system_case(name)
    args = dict(iterations=2, **rr.case_args(c, mode, True))
    a = _entry(c["source"], c["target"], c["h"], c["T"], fill=POISON_NAN, **args)
    b = _entry(c["source"], c["target"], c["h"], c["T"], fill=POISON_FINITE, **args)
    _same_bits(a, b)
    assert np.isfinite(a["T"]).all() and np.isfinite(a["history"]).all() and np.isfinite(a["information"]).all()


# ---- the corner scene: the device's own poses ------------------------------------------------------------------------------
def _corner_args(mode):
    s = rr.corner_scene()
    return s, dict(target_normals=_to(s["normals"]) if mode == "plane" else None, centre=s["centre"])


@functools.lru_cache(maxsize=None)
def _corner_run(mode, iterations):
    """cloud_register on the corner scene: numpy arrays, made once, never modified."""
    s, kw = _corner_args(mode)
    r = cloud_register(_to(s["source"]), _to(s["target"]), s["h"], T_init=torch.from_numpy(s["T_init"]), iterations=iterations,
                       **kw)
    assert r.T.dtype == torch.float32 and r.history.dtype == torch.float64 and r.status.dtype == torch.int32
    assert r.T.shape == (4, 4) and r.history.shape == (iterations + 1, 3) and r.status.shape == () and r.information.shape == (6, 6)
    return {"T": r.T.cpu().numpy(), "history": r.history.cpu().numpy(), "status": r.status.cpu().numpy(),
            "information": r.information.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def _corner_step(mode, i):
    """The restatement's evaluation, solve and update at the device's own fp32 pose after i iterations: (how far the
    device's pose after i + 1 lies from it, the bound on that) for the translation and for the rotation."""
    s = rr.corner_scene()
    T_i, T_next = _corner_run(mode, i)["T"], _corner_run(mode, i + 1)["T"].astype(np.float64)
    status, (R, t), x, _ = rr.step_reference(s["source"], s["target"], s["h"], T_i, centre=s["centre"],
                                             normals=s["normals"] if mode == "plane" else None)
    assert status == 0 and math.isfinite(x[0]) and math.isfinite(x[1])
    bt, br = rr.pose_bound(x, rr.pose_of(T_i)[1], s["centre"])
    return (float(np.linalg.norm(T_next[:3, 3] - t)), bt), (float(np.linalg.norm(T_next[:3, :3] - R, 2)), br)


@pytest.mark.parametrize("mode", rr.MODES)
@pytest.mark.parametrize("i", range(4))
def test_one_step_from_the_devices_own_pose(mode, i):
    (et, bt), (er, br) = _corner_step(mode, i)
    print(f"{mode} step {i}: translation {et:.3g} of {bt:.3g}, rotation {er:.3g} of {br:.3g}")
    assert et <= bt and er <= br


@pytest.mark.parametrize("mode", rr.MODES)
def test_corner_scene_end_to_end(mode):
    s = rr.corner_scene()
    runs = [_corner_run(mode, i) for i in range(rr.CORNER_ITERATIONS + 1)]
    last = runs[-1]
    assert last["status"] == 0 and (last["history"][:, 0] == len(s["source"])).all()
    err = [rr.pose_error(r["T"], s["T_true"]) for r in runs]
    print(f"{mode}: " + " -> ".join(f"{a:.5f} / {math.degrees(b):.3f} deg" for a, b in err))
    print(f"{mode} sum w r^2: " + " ".join(f"{x:.4g}" for x in last["history"][:, 2]))
    if mode == "plane":
        assert err[-1][0] <= err[0][0] / 10 and err[-1][1] <= err[0][1] / 10
    else:
        assert (np.diff(last["history"][:, 2]) <= 0).all() and (np.diff([e[0] for e in err]) <= 0).all()
    # the restatement's loop run from the device's own poses: every step within its bound, so the final pose within
    # their sum
    steps = [_corner_step(mode, i) for i in range(rr.CORNER_ITERATIONS)]
    assert all(et <= bt and er <= br for (et, bt), (er, br) in steps)
    assert steps[-1][0][0] <= sum(x[0][1] for x in steps) and steps[-1][1][0] <= sum(x[1][1] for x in steps)


# ---- the identities of the loop, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rr.MODES)
def test_loop_identities(mode):
    s, kw = _corner_args(mode)
    k = 5
    run = _corner_run(mode, k)
    src, tgt = _to(s["source"]), _to(s["target"])
    again = cloud_register(src, tgt, s["h"], T_init=torch.from_numpy(s["T_init"]), iterations=k, **kw)
    _same_bits(run, {"T": again.T.cpu().numpy(), "history": again.history.cpu().numpy(), "status": again.status.cpu().numpy(),
                     "information": again.information.cpu().numpy()})                      # two calls agree
    entry = _entry(s["source"], s["target"], s["h"], s["T_init"], normals=s["normals"] if mode == "plane" else None,
                   centre=s["centre"], iterations=k)
    entry["status"] = entry["status"].reshape(())
    _same_bits(run, entry)                                                                  # the function is the entry
    for i in range(k + 1):                                                                  # row i of k = the last row of i
        assert np.array_equal(_bits(run["history"][i]), _bits(_corner_run(mode, i)["history"][-1])), i
    Hm, b, count, sw, swr2, index, res = cloud_register_system(src, tgt, s["h"], torch.from_numpy(run["T"]), **kw)
    assert index is None and res is None and count.dtype == torch.int64
    at = np.array([float(count), float(sw), float(swr2)])
    assert np.array_equal(_bits(at), _bits(run["history"][-1]))                             # the system at the returned T
    assert np.array_equal(_bits(Hm.cpu().numpy()), _bits(run["information"]))
    assert np.array_equal(_bits(_corner_run(mode, 0)["T"]), _bits(s["T_init"]))            # iterations = 0: T_init's bits
    # T_init of another dtype and on the device, its bottom row kept
    T64 = torch.from_numpy(s["T_init"]).double().to(DEV)
    T64[3] = torch.tensor([0.5, -2.0, 3.0, 7.0], dtype=torch.float64)
    other = cloud_register(src, tgt, s["h"], T_init=T64, iterations=k, **kw)
    assert np.array_equal(_bits(other.T[:3].cpu().numpy()), _bits(run["T"][:3])) and other.T[3].tolist() == [0.5, -2.0, 3.0, 7.0]


def test_python_system_is_the_entry_and_the_default_centre_is_the_targets_mean():
    c = rr.system_case("hand")
    src, tgt, nm, wt = _to(c["source"]), _to(c["target"]), _to(c["normals"]), _to(c["weights"])
    for mode in rr.MODES:
        kw = dict(target_normals=nm if mode == "plane" else None, weights=wt)
        Hm, b, count, sw, swr2, index, res = cloud_register_system(src, tgt, c["h"], torch.from_numpy(c["T"]), centre=c["centre"],
                                                                   with_matches=True, **kw)
        got = {"H": Hm.cpu().numpy(), "b": b.cpu().numpy(), "sums": np.array([float(count), float(sw), float(swr2)]),
               "index": index.cpu().numpy(), "residual": res.cpu().numpy()}
        _same_bits(got, _device_system("hand", mode, True))
        # the default: the fp64 mean of the finite rows, formed on the device (its order of addition is torch's: the
        # rounded centre may differ from numpy's by an ulp, and the call with it given must be the call without)
        centre = fusion._register_centre(None, tgt, DEV)
        assert centre.dtype == torch.float32 and centre.shape == (3,) and centre.is_cuda
        assert np.abs(centre.cpu().numpy().astype(np.float64) - c["centre"]).max() <= 2.0 ** -23 * np.abs(c["centre"]).max()
        given = cloud_register_system(src, tgt, c["h"], torch.from_numpy(c["T"]), centre=centre, **kw)
        default = cloud_register_system(src, tgt, c["h"], torch.from_numpy(c["T"]), **kw)
        for a, d in zip(given[:5], default[:5]):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(d.cpu().numpy()))


# ---- stops ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rr.STOP_IDS)
def test_stops_keep_the_pose_and_repeat_the_rows(name):
    c = rr.stop_case(name)
    got = _entry(c["source"], c["target"], c["h"], c["T"], normals=c["normals"], centre=c["centre"], iterations=3,
                 min_points=c["min_points"])
    assert got["status"][0] == c["status"]
    assert np.array_equal(_bits(got["T"]), _bits(c["T"]))
    assert (got["history"] == got["history"][0]).all()
    ref = rr.register_system_reference(c["source"], c["target"], c["h"], T=c["T"], normals=c["normals"], centre=c["centre"])
    assert got["history"][0, 0] == ref["count"]
    assert _ratio(np.abs(got["information"] - ref["H"]), ref["H_bound"]) <= 1
    if name == "plane_z0":
        assert (np.diag(got["information"])[[0, 1, 5]] == 0).all()
    # with enough points asked for, the same run stops with status 1
    many = _entry(c["source"], c["target"], c["h"], c["T"], normals=c["normals"], centre=c["centre"], iterations=2,
                  min_points=len(c["source"]) + 1)
    assert many["status"][0] == 1 and np.array_equal(_bits(many["T"]), _bits(c["T"]))


# ---- order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rr.MODES)
def test_permuting_either_cloud(mode):
    c = rr.system_case("hand")
    base, ref = _device_system("hand", mode, True), rr.system_reference("hand", mode, True)
    rng = np.random.default_rng(17)
    kw = rr.case_args(c, mode, True)
    # the target's rows permuted: the matched points (not their rows: a tie goes to another duplicate), the residual bits
    # and the count stay, the sums stay within the bound
    perm = rng.permutation(len(c["target"]))
    got = _entry(c["source"], c["target"][perm], c["h"], c["T"], weights=kw["weights"], centre=kw["centre"],
                 normals=None if kw["normals"] is None else kw["normals"][perm])
    took = base["index"] >= 0
    assert np.array_equal(got["index"] >= 0, took)
    assert np.array_equal(_bits(c["target"][perm][got["index"][took]]), _bits(c["target"][base["index"][took]]))
    assert np.array_equal(_bits(got["residual"]), _bits(base["residual"]))   # (the duplicates carry one normal)
    assert got["sums"][0] == base["sums"][0] and all(x <= 1 for x in _sums_within(got, ref).values())
    # the source's rows permuted: index and residual permuted, the sums within the bound
    perm = rng.permutation(len(c["source"]))
    got = _entry(c["source"][perm], c["target"], c["h"], c["T"], normals=kw["normals"], centre=kw["centre"],
                 weights=kw["weights"][perm])
    assert np.array_equal(got["index"], base["index"][perm]) and np.array_equal(_bits(got["residual"]), _bits(base["residual"][perm]))
    assert got["sums"][0] == base["sums"][0] and all(x <= 1 for x in _sums_within(got, ref).values())
