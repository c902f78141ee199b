"""numpy restatement of the registration of one cloud to another (multi_view_stereonet_amd/fusion.py: cloud_register,
cloud_register_system; csrc/mvsn_cloud_register.hip).

The per-point arithmetic is restated in fp32 operation by operation (numpy rounds every elementwise operation once, as
the device does with contraction off), with the match taken from the brute force of tests/cloud_reference.py: which
points take part, the matched rows and the residual are the device's exactly, so there is no borderline class.  The
sums are formed in fp64 from the same products the kernel forms (each one fp64 operation on converted fp32 values, so
every term is the kernel's bit for bit) and added in extended precision; the kernel adds them in another order, which
moves a sum of `count` terms by at most (count + 4) 2^-53 sum |terms| (the bound the issue sets, for any order; in point
mode a point brings up to two non-zero terms to an entry of H, and the observed error stays far below the bound
either way).  The solve, the rotation, the update, `pose_error` and `step_bound` are tests/tsdf_align_reference.py's,
imported and not modified: the update about a centre c is `apply_update` with dims (1,1,1), voxel size 1 and origin c.
The file also holds the cases the test files run."""
import functools

import numpy as np

import tsdf_align_reference as ar
from cloud_reference import cloud_nearest_reference, radius_scalars

DBL = ar.DBL
BLOCK_POINTS = 1024              # source rows of a workgroup per block
MAX_BLOCKS = 1024                # workgroups at most
UNIT = ((1, 1, 1), 1.0)          # dims, voxel size that make apply_update's centre its origin and its step delta


def pose_of(T):
    return ar.pose_of(T)


def pose32(R, t):
    """The twelve numbers of an fp64 pose rounded once to fp32."""
    return np.asarray(R, np.float64).astype(np.float32), np.asarray(t, np.float64).astype(np.float32)


def pose_matrix(R, t, bottom=None):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = pose32(R, t)
    if bottom is not None:
        T[3] = np.asarray(bottom, np.float32)
    return T


def default_centre(target):
    """The fp64 mean of the finite rows of the target, rounded once to fp32."""
    t = np.asarray(target, np.float32)
    ok = np.isfinite(t).all(axis=1)
    return (t[ok].astype(np.float64).sum(axis=0) / max(int(ok.sum()), 1)).astype(np.float32)


def transform32(R32, t32, source):
    """p'_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a, every step one fp32 operation."""
    s = np.asarray(source, np.float32)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    with np.errstate(all="ignore"):
        p = np.stack([((R32[a, 0] * x + R32[a, 1] * y) + R32[a, 2] * z) + t32[a] for a in range(3)], axis=1)
    assert p.dtype == np.float32
    return p


def _sum(terms):
    """The sum of fp64 terms, added in extended precision and rounded once, and the sum of their magnitudes."""
    terms = np.asarray(terms, np.float64).reshape(-1)
    return float(terms.astype(np.longdouble).sum()), float(np.abs(terms).astype(np.longdouble).sum())


def register_system_reference(source, target, max_dist, *, T=None, pose=None, normals=None, weights=None, centre):
    """One evaluation at the fp32 values of T (4,4), or at the fp64 pose (R, t) rounded to fp32.  Returns a dict:
    takes_part (N,) bool, index (N,) int64 (-1 where the point takes no part), residual (N,) fp32 (r in plane mode, d2 in
    point mode, NaN where the point takes no part), p (N,3) fp32 the moved points, rows: a list of (r (N,), J (6,N)) in
    fp32 (one row in plane mode, three in point mode; only the columns of takes_part mean anything); H (6,6), b (6,),
    count, sum_w, sum_w_r2 in fp64 and H_bound, b_bound, sum_w_bound, sum_w_r2_bound for the kernel's order of
    addition."""
    src = np.ascontiguousarray(source, np.float32).reshape(-1, 3)
    tgt = np.ascontiguousarray(target, np.float32).reshape(-1, 3)
    N, M = len(src), len(tgt)
    R, t = pose_of(T) if pose is None else pose
    R32, t32 = pose32(R, t)
    c = np.asarray(centre, np.float32)
    assert c.shape == (3,)
    w = np.ones(N, np.float32) if weights is None else np.asarray(weights, np.float32)
    plane = normals is not None
    p = transform32(R32, t32, src)
    with np.errstate(all="ignore"):
        cand = np.isfinite(src).all(axis=1) & np.isfinite(p).all(axis=1) & np.isfinite(w) & (w > 0)
    index = np.full(N, -1, np.int64)
    d2 = np.full(N, np.inf, np.float32)
    if cand.any() and M:
        nn = cloud_nearest_reference(p[cand], tgt, max_dist)
        index[cand], d2[cand] = nn["index"], nn["dist2"]
    takes = cand & (index >= 0)
    j = np.where(takes, index, 0)
    if plane:
        nrm = np.asarray(normals, np.float32).reshape(M, 3)[j]
        takes &= np.isfinite(nrm).all(axis=1)
        j = np.where(takes, index, 0)
    with np.errstate(all="ignore"):
        d = (p - tgt[j]).astype(np.float32)                  # the differences the query forms
        q = p - c[None, :]
        zero, one = np.zeros(N, np.float32), np.ones(N, np.float32)
        if plane:
            r = (d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1]) + d[:, 2] * nrm[:, 2]
            J = np.stack([nrm[:, 0], nrm[:, 1], nrm[:, 2],
                          q[:, 1] * nrm[:, 2] - q[:, 2] * nrm[:, 1],
                          q[:, 2] * nrm[:, 0] - q[:, 0] * nrm[:, 2],
                          q[:, 0] * nrm[:, 1] - q[:, 1] * nrm[:, 0]])
            rows = [(r, J)]
            residual = r
        else:
            rows = [(d[:, 0], np.stack([one, zero, zero, zero, q[:, 2], -q[:, 1]])),
                    (d[:, 1], np.stack([zero, one, zero, -q[:, 2], zero, q[:, 0]])),
                    (d[:, 2], np.stack([zero, zero, one, q[:, 1], -q[:, 0], zero]))]
            residual = d2
    assert all(r_.dtype == np.float32 and J_.dtype == np.float32 for r_, J_ in rows)
    index = np.where(takes, index, -1)
    residual = np.where(takes, residual, np.float32(np.nan)).astype(np.float32)
    count = int(takes.sum())
    round64 = (count + 4.0) * DBL
    wd = w[takes].astype(np.float64)
    H, Hb, b, bb = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros(6), np.zeros(6)
    sel = [(r_[takes].astype(np.float64), J_[:, takes].astype(np.float64)) for r_, J_ in rows]
    some = [[bool(J_[i].any()) for i in range(6)] for _, J_ in sel]   # (a column of zeros brings zeros: left out)
    none = np.zeros(0)
    for i in range(6):
        # (w J_i), then times J_j or r: the kernel's two products
        wJ = [wd * J_[i] if some[a][i] else None for a, (_, J_) in enumerate(sel)]
        for k in range(i, 6):
            s, a = _sum(np.concatenate([none] + [wJ[a] * J_[k] for a, (_, J_) in enumerate(sel) if some[a][i] and some[a][k]]))
            H[i, k] = H[k, i] = s
            Hb[i, k] = Hb[k, i] = round64 * a
        s, a = _sum(np.concatenate([none] + [wJ[a] * r_ for a, (r_, _) in enumerate(sel) if some[a][i]]))
        b[i], bb[i] = s, round64 * a
    sw, swa = _sum(wd)
    if plane:
        rd = sel[0][0]
        swr2, swr2a = _sum((wd * rd) * rd)
    else:
        swr2, swr2a = _sum(wd * d2[takes].astype(np.float64))
    return {"takes_part": takes, "index": index, "residual": residual, "p": p, "rows": rows, "H": H, "b": b,
            "count": count, "sum_w": sw, "sum_w_r2": swr2, "H_bound": Hb, "b_bound": bb, "sum_w_bound": round64 * swa,
            "sum_w_r2_bound": round64 * swr2a}


def apply_update(R, t, delta, centre):
    """R <- Rd R, t <- Rd (t - c) + c + v about the fp32 centre c (section 17's update, imported)."""
    return ar.apply_update(R, t, delta, UNIT[0], UNIT[1], np.asarray(centre, np.float32))


def pose_bound(x, t, centre):
    """How far (translation distance, rotation as the 2-norm of the difference of the matrices) the fp32 pose after an
    update may lie from the restatement's when the update's parts move by x = (x_v, x_w) and the update starts from the
    fp32 rounding of the fp64 pose instead of the pose itself: `pose_bound` of section 17 (the move, and the rounding of
    the output) with its rounding allowance twice, once more for the rounded input (t_new moves as t does, R_new = Rd R as
    R does)."""
    bt, br = ar.pose_bound(x, t, UNIT[0], UNIT[1], np.asarray(centre, np.float32))
    lever = float(np.linalg.norm(np.asarray(t, np.float64) - np.asarray(centre, np.float32).astype(np.float64)))
    move = x[0] + lever * x[1]
    return bt + (bt - move), br + (br - x[1])


def step_reference(source, target, max_dist, T, *, normals=None, weights=None, centre, min_points=6, min_pivot=1e-9):
    """One evaluation, solve and update at the fp32 pose T (4,4): (status, (R, t) the fp64 pose after the update or T's
    where the solve stops, (x_v, x_w) = `step_bound` or zeros, the evaluation's dict)."""
    R, t = pose_of(T)
    sysm = register_system_reference(source, target, max_dist, pose=(R, t), normals=normals, weights=weights, centre=centre)
    status, delta = ar.solve_reference(sysm["H"], sysm["b"], sysm["count"], min_points, min_pivot)
    if status:
        return status, (R, t), (0.0, 0.0), sysm
    return 0, apply_update(R, t, delta, centre), ar.step_bound(sysm["H"], sysm["b"], sysm["H_bound"], sysm["b_bound"]), sysm


def register_reference(source, target, max_dist, *, T_init=None, normals=None, weights=None, centre, iterations=20,
                       min_points=6, min_pivot=1e-9):
    """The loop, carrying the fp64 pose along.  Returns a dict: poses (iterations+1 pairs (R, t) in fp64 before update i,
    the last the final one), T (4,4) fp32, history (iterations+1,3), status, information, systems and step_bounds
    (iterations: `step_bound` at pose i, zeros where the run is stopped)."""
    T0 = np.eye(4, dtype=np.float32) if T_init is None else np.asarray(T_init, np.float32)
    R, t = pose_of(T0)
    out_poses, history, systems, bounds = [], [], [], []
    status = 0
    for it in range(iterations + 1):
        sysm = register_system_reference(source, target, max_dist, pose=(R, t), normals=normals, weights=weights,
                                         centre=centre)
        out_poses.append((R.copy(), t.copy()))
        systems.append(sysm)
        history.append((float(sysm["count"]), sysm["sum_w"], sysm["sum_w_r2"]))
        if it == iterations:
            break
        delta = None
        if status == 0:
            status, delta = ar.solve_reference(sysm["H"], sysm["b"], sysm["count"], min_points, min_pivot)
        if status == 0:
            bounds.append(ar.step_bound(sysm["H"], sysm["b"], sysm["H_bound"], sysm["b_bound"]))
            R, t = apply_update(R, t, delta, centre)
        else:
            bounds.append((0.0, 0.0))
    return {"poses": out_poses, "T": pose_matrix(R, t, T0[3]), "history": np.array(history),
            "status": status, "information": systems[-1]["H"], "systems": systems, "step_bounds": bounds}


def pose_error(T, T_true):
    return ar.pose_error(T, T_true)


def wrapping_points():
    """One source row more than the workgroups own in their first round: workgroup 0 goes on to a second block."""
    return BLOCK_POINTS * MAX_BLOCKS + 1


# ---- the cases of one evaluation -----------------------------------------------------------------------------------------
GENERAL = ((0.3, -0.2, 0.25), (0.4, -0.3, 0.2))           # (omega, t): a pose in general position


def general_pose():
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = ar.rotation(GENERAL[0]), GENERAL[1]
    return T.astype(np.float32)


def _pulled_back(T, points):
    """fp32 source rows that T brings near `points` (a non-finite point gives a non-finite row)."""
    R, t = pose_of(T)
    with np.errstate(all="ignore"):
        return ((np.asarray(points, np.float64) - t) @ R).astype(np.float32)


def _unit_normals(rng, m):
    n = rng.normal(size=(m, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def _weights(rng, n, rows):
    """Weights in [0.5, 2) with 0, a negative one, NaN and +-inf at `rows`."""
    w = (0.5 + 1.5 * rng.random(n)).astype(np.float32)
    for row, bad in zip(rows, (0.0, -1.0, np.nan, np.inf, -np.inf)):
        w[row] = bad
    return w


def _hand():
    """The hand case of tests/test_cloud_gpu.py (1027 queries, 1031 targets, h = 0.25) with its queries as the places the
    sources are moved to.  The transform's roundings move a source off the query it was pulled back from, so the exact
    coincidences are restored on the target's side: target 5 and its ten duplicates sit on the moved source 5, target
    700 on the moved source 6, and target 20 exactly 0.25 along x from the moved source 10 (d2 == r2: the difference of
    two multiples of 2^-20 below 16 is exact)."""
    from test_cloud_gpu import _hand_case
    q, t, h = _hand_case()
    q, t = q.copy(), t.copy()
    rng = np.random.default_rng(43)
    q[800:1026] = t[800:1026] + rng.uniform(-0.05, 0.05, (226, 3)).astype(np.float32)   # more sources with a match
    T = general_pose()
    src = _pulled_back(T, q)
    src[503] = (3.0e38, -3.0e38, 3.0e38)                                # finite, and its moved point is not
    R32, t32 = pose32(*pose_of(T))
    p = transform32(R32, t32, src)
    t[5] = p[5]
    t[100:110] = t[5]
    t[700] = p[6]
    t[20] = p[10] - np.array([0.25, 0.0, 0.0], np.float32)
    normals = _unit_normals(rng, len(t))
    ref = cloud_nearest_reference(p[np.isfinite(p).all(axis=1)], t, h)["index"]
    hit = np.unique(ref[ref >= 0])
    normals[hit[3]] = (np.nan, 0.0, 1.0)                                # matched targets without a usable normal
    normals[hit[17]] = (0.0, np.inf, 0.0)
    normals[700] = (0.0, 0.0, -np.inf)
    normals[100:110] = normals[5]                                       # the duplicates are one oriented point
    matched = np.flatnonzero(np.isfinite(p).all(axis=1))[ref >= 0]
    weights = _weights(rng, len(src), matched[20:25])                   # bad weights on sources that do have a match
    return dict(source=src, target=t, h=h, T=T, normals=normals, weights=weights, centre=default_centre(t))


def _cube(n, m, seed, h=0.25, side=1.5, spread=0.1, target=None):
    """m targets uniform in a cube and n sources that the general pose brings to within `spread` of targets."""
    def make():
        rng = np.random.default_rng(seed)
        t = rng.uniform(-side, side, (m, 3)).astype(np.float32) if target is None else target(rng)
        T = general_pose()
        at = t[rng.integers(0, len(t), n)] + rng.uniform(-spread, spread, (n, 3))
        return dict(source=_pulled_back(T, at), target=t, h=h, T=T, normals=_unit_normals(rng, len(t)),
                    weights=_weights(rng, n, ()), centre=default_centre(t))
    return make


def _one_cell(rng):
    return rng.uniform(0.01, 0.24, (1027, 3)).astype(np.float32)


def _eight(rng):
    return (np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64) * 0.3 + 0.1).astype(np.float32)


_TABLE = {"hand": _hand}
for _n in (1, 255, 256, 257, BLOCK_POINTS + 1):
    _TABLE[f"n{_n}"] = _cube(_n, 300, 100 + _n)
_TABLE["m1"] = _cube(300, 1, 7, spread=0.2)
_TABLE["one_cell_1027"] = _cube(300, 1027, 8, spread=0.05, target=_one_cell)
_TABLE["wrapping"] = _cube(wrapping_points(), 8, 9, h=0.5, spread=0.4, target=_eight)
CASE_IDS = tuple(_TABLE)
SMALL_CASE_IDS = tuple(k for k in CASE_IDS if k != "wrapping")
MODES = ("plane", "point")


@functools.lru_cache(maxsize=None)
def system_case(name):
    """One case: made once, never modified."""
    return _TABLE[name]()


def case_args(c, mode, weighted):
    return dict(normals=c["normals"] if mode == "plane" else None, weights=c["weights"] if weighted else None,
                centre=c["centre"])


@functools.lru_cache(maxsize=None)
def system_reference(name, mode, weighted):
    """The restatement of one case: computed once, shared, never modified."""
    c = system_case(name)
    return register_system_reference(c["source"], c["target"], c["h"], T=c["T"], **case_args(c, mode, weighted))


# ---- the stops -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stop_case(name):
    rng = np.random.default_rng(5)
    T = general_pose()
    if name == "out_of_reach":             # status 1: every moved source is 2 or more from every target, max_dist 0.25
        t = rng.uniform(-1.0, 1.0, (200, 3)).astype(np.float32)
        at = rng.uniform(-1.0, 1.0, (150, 3)) + np.array([5.0, 0.0, 0.0])
        return dict(source=_pulled_back(T, at), target=t, h=0.25, T=T, normals=_unit_normals(rng, 200), mode="plane",
                    centre=default_centre(t), min_points=6, status=1)
    if name == "plane_z0":                 # status 2: J = (0, 0, 1, q_y, -q_x, 0), three zero diagonal entries of H
        t = np.concatenate([rng.uniform(-1.0, 1.0, (400, 2)), np.zeros((400, 1))], axis=1).astype(np.float32)
        normals = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (400, 1))
        at = t[rng.integers(0, 400, 150)] + rng.uniform(-0.05, 0.05, (150, 3))
        return dict(source=_pulled_back(T, at), target=t, h=0.25, T=T, normals=normals, mode="plane",
                    centre=default_centre(t), min_points=6, status=2)
    if name == "two_points":               # status 2 by the pivot: the turn about the line through both is free
        t = np.array([[0.5, 0.25, -0.5], [-0.75, 0.5, 0.25]], np.float32)
        at = t + np.array([[0.03, -0.02, 0.04], [-0.02, 0.05, 0.01]])
        return dict(source=_pulled_back(T, at), target=t, h=0.25, T=T, normals=None, mode="point",
                    centre=default_centre(t), min_points=1, status=2)
    raise KeyError(name)


STOP_IDS = ("out_of_reach", "plane_z0", "two_points")


# ---- the corner scene -----------------------------------------------------------------------------------------------------
CORNER_MAX_DIST = 0.15
CORNER_ITERATIONS = 8


def _corner_points(K, T, size):
    """The analytic surface points (H*W,3) and outward unit normals (H*W,3) of the corner scene as the camera sees them,
    in fp64: the nearest of the three planes and the sphere along every ray, as `corner_depth` takes it."""
    o, v = ar._rays(K, T, size)
    best = ar._sphere_depth(o, v, ar.CORNER["centre"], ar.CORNER["radius"])
    which = np.where(np.isfinite(best), 3, -1)
    for k, (n, c) in enumerate(ar.CORNER["planes"]):
        n = np.asarray(n, np.float64)
        nv = (v * n[:, None, None]).sum(0)
        with np.errstate(all="ignore"):
            D = (c - float(n @ o)) / nv
        D = np.where((nv < 0) & (D > 0), D, np.inf)
        which = np.where(D < best, k, which)
        best = np.minimum(best, D)
    assert np.isfinite(best).all()
    pts = (o[:, None, None] + best[None] * v).reshape(3, -1).T
    normals = np.empty_like(pts)
    flat = which.reshape(-1)
    for k, (n, _) in enumerate(ar.CORNER["planes"]):
        n = np.asarray(n, np.float64)
        normals[flat == k] = n / np.linalg.norm(n)
    ball = flat == 3
    normals[ball] = (pts[ball] - np.asarray(ar.CORNER["centre"], np.float64)) / ar.CORNER["radius"]
    return pts, normals


@functools.lru_cache(maxsize=None)
def corner_scene():
    """target (9216,3), normals (9216,3): views 0-2 of the corner scene back-projected from their analytic depth maps,
    with the scene's analytic normals; source (3072,3): view 3's points in its camera frame; T_init = corner_start(),
    T_true = view 3's pose; all fp32."""
    K, T, depth = ar.corner_views()
    size = ar.CORNER["size"]
    pts, nrm = zip(*[_corner_points(K[v], T[v], size) for v in range(3)])
    target, normals = np.concatenate(pts).astype(np.float32), np.concatenate(nrm).astype(np.float32)
    world, _ = _corner_points(K[3], T[3], size)
    R, t = pose_of(T[3])
    source = ((world - t) @ R).astype(np.float32)
    return dict(source=source, target=target, normals=normals, T_init=ar.corner_start(), T_true=T[3],
                h=CORNER_MAX_DIST, centre=default_centre(target))


@functools.lru_cache(maxsize=None)
def corner_loop(mode, iterations=CORNER_ITERATIONS):
    """The restatement's loop on the corner scene: computed once, shared, never modified."""
    s = corner_scene()
    return register_reference(s["source"], s["target"], s["h"], T_init=s["T_init"],
                              normals=s["normals"] if mode == "plane" else None, centre=s["centre"], iterations=iterations)
