"""cloud_normals on the device (csrc/mvsn_cloud_normals.hip) against the numpy restatement
(tests/cloud_normals_reference.py): the count and the zero pattern exactly, the normal within one fp32 rounding per
component plus what two eigen-solvers may differ by, the eigenvalues likewise; every buffer between guard bands under both
poisons; the order of the support; and the corner scene, where the estimated normals take cloud_register's plane mode as
far as the analytic ones do.

The solver term is 8 K 2^-52 lambda2 / (lambda1 - lambda0) with K measured between the restatement's Jacobi iteration and
numpy.linalg.eigh (tests/test_cloud_normals_reference_cpu.py); the factor 8 is for the device's fp64 divide and square
root possibly differing from numpy's in the last place at each of the few dozen steps.  Where two solvers cannot agree on
the sign (the two largest components of the normal tie, or the viewpoint lies in the tangent plane, to within 1e-9) the
lines are compared and the device's own sign is checked against its own output.

Figures of one MI355X run are in DESIGN.md section 21."""
import functools
import math

import numpy as np
import pytest
import torch

import cloud_normals_reference as cn
import cloud_register_reference as rr
from cloud_reference import radius_scalars
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd.fusion import cloud_nearest, cloud_normals, cloud_register

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROUNDING = math.sqrt(3.0) * 2.0 ** -24                  # every component rounded once to fp32
SIGN_MARGIN = 1e-9


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _entry(points, support, h, *, viewpoint=None, fill=POISON_NAN, eigenvalues=True, min_neighbours=3, min_gap=cn.MIN_GAP):
    """mvsn_cloud_index_build, then mvsn_cloud_normals, every input in a poisoned buffer of its own (16-byte aligned
    only), the workspace, the status word and every output carved between guard bands and poisoned too: numpy arrays."""
    hf, inv, r2 = radius_scalars(h)
    support = points if support is None else support
    n, m = len(points), len(support)
    guard = Guard(_alloc, fill)
    q, t = guard.poisoned(_to(points)), guard.poisoned(_to(support))
    view = None if viewpoint is None else guard.poisoned(_to(np.asarray(viewpoint, np.float32).reshape(-1, 3)))
    lib = _native.load()
    ws_bytes = lib.mvsn_cloud_workspace_bytes(m)
    ws, status = guard.empty((ws_bytes,), torch.uint8, DEV), guard.empty((1,), torch.int64, DEV)
    normals, count = guard.empty((n, 3), torch.float32, DEV), guard.empty((n,), torch.int32, DEV)
    lam = guard.empty((n, 3), torch.float32, DEV) if eigenvalues else None
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_cloud_index_build(_native.ptr(t), m, float(hf), float(inv), _native.ptr(status),
                                                 _native.ptr(ws), ws_bytes, st), "mvsn_cloud_index_build")
        _native.check(lib.mvsn_cloud_normals(_native.ptr(q), n, _native.ptr(view), 0 if view is None else int(view.shape[0]),
                                             float(hf), float(inv), float(r2), min_neighbours, min_gap, _native.ptr(ws),
                                             ws_bytes, m, _native.ptr(normals), _native.ptr(lam), _native.ptr(count), st),
                      "mvsn_cloud_normals")
    torch.cuda.synchronize()
    guard.check()
    assert int(status.item()) == 0
    out = {"normals": normals.cpu().numpy(), "count": count.cpu().numpy()}
    if eigenvalues:
        out["eigenvalues"] = lam.cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def _device_run(name, view, fill):
    c = cn.case(name)
    return _entry(c["points"], c["support"], c["h"], viewpoint=cn.case_viewpoint(name, view), fill=fill)


def _device(name, view=None, fill=POISON_NAN):
    """Made once per (case, viewpoint, poison), never modified."""
    return _device_run(name, view, fill)


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def _sign_decided(ref, points, viewpoint):
    """Where the sign rule has a margin of SIGN_MARGIN on eigh's normal: another solver's normal gets the same sign."""
    n = np.abs(ref["eigh_normals"])
    top = np.sort(n, axis=1)
    decided = top[:, 2] - top[:, 1] > SIGN_MARGIN
    if viewpoint is not None:
        v = np.broadcast_to(np.asarray(viewpoint, np.float32).reshape(-1, 3), points.shape)
        with np.errstate(all="ignore"):
            e = v.astype(np.float64) - points.astype(np.float64)
            dot = (ref["eigh_normals"] * e).sum(axis=1)
            clear = np.abs(dot) > SIGN_MARGIN * np.linalg.norm(e, axis=1)
        finite = np.isfinite(v).all(axis=1)
        on_point = finite & (e == 0).all(axis=1)
        decided = np.where(finite & ~on_point, clear, decided)
    return decided


def _agrees(got, ref, points, viewpoint=None, what=""):
    np.testing.assert_array_equal(got["count"], ref["count"])
    zero = ~ref["defined"]
    np.testing.assert_array_equal((got["normals"] == 0).all(axis=1), zero)
    d = ref["defined"]
    solver = cn.solver_term(ref, 8 * cn.K_JACOBI)
    ratio_n = ratio_l = 0.0
    if d.any():
        decided = _sign_decided(ref, points, viewpoint)
        ang = np.where(decided, cn.angle(got["normals"], ref["eigh_normals"]), cn.axis_angle(got["normals"], ref["eigh_normals"]))
        ratio_n = float((ang[d] / (ROUNDING + solver[d])).max())
    if "eigenvalues" in got:
        solved = (ref["count"] >= 1) & (ref["count"] <= cn.MAX_NEIGHBOURS)
        assert (got["eigenvalues"][~solved] == 0).all()
        with np.errstate(all="ignore"):
            want = ref["eigh_lam"].astype(np.float32)                  # rounded once, as the device rounds
        lam2 = ref["eigh_lam"][:, 2]
        err = np.abs(got["eigenvalues"].astype(np.float64) - want.astype(np.float64)).max(axis=1)
        # (where the direction is not defined the solvers still agree on the eigenvalues to rounding: the term at gap 1)
        term = np.where(d, solver, 8 * cn.K_JACOBI * cn.EPS)
        bound = (2.0 ** -23 + term) * lam2
        assert (err[solved & (lam2 <= 0)] == 0).all()                   # (coincident neighbours: the covariance is 0 exactly)
        pos = solved & (lam2 > 0)
        if pos.any():
            ratio_l = float((err[pos] / bound[pos]).max())
        assert (np.diff(got["eigenvalues"], axis=1) >= 0).all()
    print(f"{what}: {int(d.sum())} of {len(d)} with a normal; error / bound max: normals {ratio_n:.3g}, eigenvalues {ratio_l:.3g}; "
          f"bits equal to the restatement's Jacobi normals: {got['normals'].tobytes() == ref['normals'].tobytes()}")
    assert ratio_n <= 1 and ratio_l <= 1
    return ratio_n, ratio_l


# ---- every case, every form of the viewpoint ----------------------------------------------------------------------------
@pytest.mark.parametrize("view", [None, "one", "rows"])
@pytest.mark.parametrize("name", [n for n in cn.CASE_IDS if n != "limit"] + ["hand_self"])
def test_cases_match_the_restatement(name, view):
    c = cn.case(name)
    _agrees(_device(name, view), cn.case_reference(name, view), c["points"], cn.case_viewpoint(name, view), f"{name} {view}")


def test_the_limit_of_two_to_the_twenty_neighbours():
    c, ref = cn.case("limit"), cn.case_reference("limit", None)
    got = _device("limit")
    assert got["count"].tolist() == [2 ** 20, 2 ** 20 + 1]
    assert (got["normals"][1] == 0).all() and (got["eigenvalues"][1] == 0).all() and (got["normals"][0] != 0).any()
    _agrees(got, ref, c["points"], None, "limit")


def test_canonical_sign_on_the_devices_own_output():
    for name in ("hand", "hand_self", "n257", "far"):
        n = _device(name)["normals"]
        n = n[(n != 0).any(axis=1)]
        a = np.abs(n)
        lead = np.take_along_axis(n, a.argmax(axis=1)[:, None], axis=1)[:, 0]
        strict = np.sort(a, axis=1)[:, 2] > np.sort(a, axis=1)[:, 1]
        assert (lead[strict] > 0).all() and strict.mean() > 0.9
        assert (np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1) <= 2.0 ** -23).all()


def test_viewpoint_on_the_devices_own_output():
    for name in ("hand", "n257"):
        q, v = cn.case(name)["points"], cn.case_viewpoint(name, "rows")
        got, base = _device(name, "rows")["normals"], _device(name)["normals"]
        assert (np.abs(got) == np.abs(base)).all() and (got != base).any()
        with np.errstate(invalid="ignore"):
            dot = (got.astype(np.float64) * (v.astype(np.float64) - q.astype(np.float64))).sum(axis=1)
        finite = np.isfinite(v).all(axis=1) & (got != 0).any(axis=1)
        assert (dot[finite] >= -1e-6).all()                             # (the fp32 rounding of n against |v - p| of a few units)
        keeps = ~np.isfinite(v).all(axis=1) | (v == q).all(axis=1)
        assert keeps.sum() >= 10 and got[keeps].tobytes() == base[keeps].tobytes()


# ---- buffers, options ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cn.CASE_IDS + ("hand_self",))
def test_buffers_under_both_poisons(name):
    # (the guard bands of every buffer are checked inside _entry; an element nobody writes, or a read of foreign memory
    # that reaches a result, differs between the two fills)
    for view in (None, "rows")[:1 if name == "limit" else 2]:        # (the limit walks a million records: once per poison)
        _same_bits(_device(name, view, POISON_NAN), _device(name, view, POISON_FINITE))


def test_eigenvalues_left_out_and_the_thresholds():
    c = cn.case("hand")
    full = _device("hand")
    for fill in (POISON_NAN, POISON_FINITE):
        got = _entry(c["points"], c["support"], c["h"], eigenvalues=False, fill=fill)
        assert set(got) == {"normals", "count"}
        assert got["normals"].tobytes() == full["normals"].tobytes() and got["count"].tobytes() == full["count"].tobytes()
    # min_neighbours and min_gap decide the zero pattern and nothing else
    ref = cn.cloud_normals_reference(c["points"], c["h"], support=c["support"], min_neighbours=6, min_gap=0.05)
    assert 0 < ref["defined"].sum() < cn.case_reference("hand", None)["defined"].sum()
    near = (ref["gap"] > 0.05 * (1 - 1e-9)) & (ref["gap"] < 0.05 * (1 + 1e-9))
    assert not near.any()                                               # nobody within rounding of the threshold
    got = _entry(c["points"], c["support"], c["h"], min_neighbours=6, min_gap=0.05)
    np.testing.assert_array_equal((got["normals"] == 0).all(axis=1), ~ref["defined"])
    keep = ref["defined"]
    assert got["normals"][keep].tobytes() == full["normals"][keep].tobytes()
    assert got["eigenvalues"].tobytes() == full["eigenvalues"].tobytes()


def test_permuting_the_support_and_calling_twice():
    c = cn.case("hand")
    perm = np.random.default_rng(173).permutation(len(c["support"]))
    view = cn.case_viewpoint("hand", "rows")
    base = _device("hand", "rows")
    _same_bits(base, _entry(c["points"], c["support"], c["h"], viewpoint=view))
    _same_bits(base, _entry(c["points"], c["support"][perm], c["h"], viewpoint=view))
    # the cloud against itself: permuting it permutes the rows of the outputs
    s = cn.case("hand_self")["points"]
    own, moved = _device("hand_self"), _entry(s[perm], None, c["h"])
    for k in own:
        assert own[k][perm].tobytes() == moved[k].tobytes(), k


def test_the_python_call_is_the_library_call():
    c = cn.case("hand")
    q, t = _to(c["points"]), _to(c["support"])
    rows = cn.case_viewpoint("hand", "rows")
    for view, kind in ((None, None), ((0.3, -0.2, 5.0), "one"), (torch.tensor([0.3, -0.2, 5.0], dtype=torch.float64), "one"),
                       (_to(np.array([0.3, -0.2, 5.0], np.float32)), "one"), (_to(rows), "rows")):
        r = cloud_normals(q, c["h"], support=t, viewpoint=view)
        assert r.normals.dtype == r.eigenvalues.dtype == torch.float32 and r.count.dtype == torch.int32
        assert r.normals.shape == r.eigenvalues.shape == (len(q), 3) and r.count.shape == (len(q),) and r.normals.is_cuda
        _same_bits({"normals": r.normals.cpu().numpy(), "eigenvalues": r.eigenvalues.cpu().numpy(), "count": r.count.cpu().numpy()},
                   _device("hand", kind))
        assert torch.equal(r.count, cloud_nearest(q, t, c["h"]).within)
    own = cloud_normals(t, c["h"])                                      # the support defaults to the points
    _same_bits({"normals": own.normals.cpu().numpy(), "eigenvalues": own.eigenvalues.cpu().numpy(), "count": own.count.cpu().numpy()},
               _device("hand_self"))
    far = c["support"].copy()
    far[123, 1] = 2.0 ** 20 * c["h"]
    with pytest.raises(ValueError, match="max_dist too small for the target's extent"):
        cloud_normals(q, c["h"], support=_to(far))
    empty = cloud_normals(q, c["h"], support=torch.zeros(0, 3, device=DEV))
    assert empty.normals.is_cuda and not empty.normals.any() and not empty.eigenvalues.any() and not empty.count.any()


# ---- the corner scene -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene_normals():
    s = cn.corner_cloud()
    r = cloud_normals(_to(s["points"]), cn.SCENE_RADIUS, viewpoint=_to(s["viewpoint"]))
    return r


def test_corner_scene_normals_against_the_analytic_ones():
    s, r = cn.corner_cloud(), _scene_normals()
    got = r.normals.cpu().numpy()
    inner = s["interior"]
    assert inner.sum() > 3000 and (got[inner] != 0).any(axis=1).all()
    ang = cn.angle(got[inner], s["normals"][inner])
    every = cn.angle(got, s["normals"])
    print(f"corner scene: {int(inner.sum())} interior points, angle to the analytic normal max {ang.max():.4g} mean {ang.mean():.4g}; "
          f"all {len(got)} points: mean {every.mean():.4g} p99 {np.quantile(every, 0.99):.4g}, "
          f"{float((got != 0).any(axis=1).mean()):.3f} with a normal")
    assert ang.max() <= cn.SCENE_MAX_ANGLE
    # every normal faces its own camera
    e = s["viewpoint"].astype(np.float64) - s["points"].astype(np.float64)
    assert ((got.astype(np.float64) * e).sum(axis=1) >= 0).all()


def test_corner_scene_registration_with_the_estimated_normals():
    # section 20's end-to-end assertion, with the estimated normals in place of the analytic ones
    s = cn.corner_cloud()["scene"]
    tn = _scene_normals().normals
    src, tgt = _to(s["source"]), _to(s["target"])
    T0 = torch.from_numpy(s["T_init"])
    err = []
    for i in (0, rr.CORNER_ITERATIONS):
        r = cloud_register(src, tgt, s["h"], target_normals=tn, T_init=T0, iterations=i, centre=s["centre"])
        assert int(r.status) == 0
        err.append(rr.pose_error(r.T.cpu().numpy(), s["T_true"]))
    print("plane mode with estimated normals: " + " -> ".join(f"{a:.5f} / {math.degrees(b):.3f} deg" for a, b in err))
    assert err[-1][0] <= err[0][0] / 10 and err[-1][1] <= err[0][1] / 10
