"""fp64 numpy restatement of the alignment of depth maps to the TSDF volume (multi_view_stereonet_amd/tsdf.py: align,
align_system; csrc/mvsn_tsdf_align.hip): one evaluation of the Gauss-Newton system with bounds for
the kernel's fp32 evaluation that follow from its roundings alone, the pixels whose decision can flip under those bounds,
the loop with the bound that one step carries from the bounds on H and b, and the cases the test files run.

The sample is section 16's with the depth D in place of t_k, so the camera, the grid, the margins m_g and m_f and the
gradient bound are tests/tsdf_raycast_reference.py's, imported and not modified."""
import functools
import math

import numpy as np

from tsdf_raycast_reference import (DIR_EPS, GRAD_EPS, LERP_EPS, SPHERE_SIZES, _bilinear, _corner, _Grid, _intrinsics,
                                    _trilinear, camera, look_at, shape_camera, sphere_camera, sphere_variants, three_views)
from tsdf_reference import EPS, SPHERE, tsdf_integrate_reference

DBL = 2.0 ** -53            # the relative error of one correctly rounded fp64 operation
TILE = 32                   # lattice pixels of a workgroup along each axis


def camera_from_pose(K, R, t, voxel_size, origin):
    """`camera` of the ray-cast's restatement from an fp64 pose (R (3,3), t (3,)): the same operations in the same
    order, each of the twelve numbers rounded once to fp32; as fp64.  On float32 values it is `camera` (asserted in
    tests/test_tsdf_align_reference_cpu.py)."""
    K = np.asarray(K, np.float32).astype(np.float64)
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    a, b, c, d, e, f, g, h, i = K[:3, :3].reshape(-1)
    A_, B_, C_ = e * i - f * h, -(d * i - f * g), d * h - e * g
    r = 1.0 / (a * A_ + b * B_ + c * C_)
    Ki = np.array([[A_ * r, -(b * i - c * h) * r, (b * f - c * e) * r],
                   [B_ * r, (a * i - c * g) * r, -(a * f - c * d) * r],
                   [C_ * r, -(a * h - b * g) * r, (a * e - b * d) * r]])
    vs = np.float64(np.float32(voxel_size))
    o = np.asarray(origin, np.float32).astype(np.float64)
    A = np.empty((3, 3))
    for m in range(3):
        for n in range(3):
            A[m, n] = ((R[m, 0] * Ki[0, n] + R[m, 1] * Ki[1, n]) + R[m, 2] * Ki[2, n]) / vs
    g0 = (t - o) / vs
    return A.astype(np.float32).astype(np.float64), g0.astype(np.float32).astype(np.float64)


def pose_of(T):
    """(R, t) in fp64 of the float32 values of a (4,4) pose."""
    T = np.asarray(T, np.float32).astype(np.float64)
    return T[:3, :3].copy(), T[:3, 3].copy()


@functools.lru_cache(maxsize=None)
def _grid_cached(key):
    return _Grid(*_GRID_ARGS[key])


_GRID_ARGS = {}


def grid_of(sdf_sum, weight, min_weight):
    """The `_Grid` of a state (cached by the identity of its arrays: the states here are made once, never modified)."""
    key = (id(sdf_sum), id(weight), float(min_weight))
    _GRID_ARGS[key] = (sdf_sum, weight, None, min_weight)
    return _grid_cached(key)


def _cross(q, n):
    return np.stack([q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0]])


def _cross_bound(q, dq, n, dn):
    """|fl(q x n) - exact of the true q, n|: each product moves by |q| dn + |n| dq + dq dn, and the fma and the product
    inside it round once each (2 EPS of the magnitudes)."""
    def pair(i, j):
        return np.abs(q[i]) * dn[j] + np.abs(n[j]) * dq[i] + dq[i] * dn[j] + 2.0 * EPS * np.abs(q[i] * n[j])
    return np.stack([pair(1, 2) + pair(2, 1), pair(2, 0) + pair(0, 2), pair(0, 1) + pair(1, 0)])


def align_system_reference(grid, voxel_size, origin, depth, K, T, *, band, valid=None, weights=None, stride=1,
                           pose=None, decided=None):
    """One view: depth (H,W) fp32, K, T (4,4); `pose` = (R, t) fp64 replaces T (the loop's current pose).  Returns a
    dict: takes_part (H,W); r (H,W), J (6,H,W), w (H,W) in fp64 (0 where the pixel does not take part); the margins m_g
    (3,H,W), m_f (H,W), the bounds r_bound (H,W) and J_bound (6,H,W) on the kernel's fp32 r and J; borderline (H,W);
    lattice (H,W); g (3,H,W) and index, the points and their cells; H (6,6), b (6), count, sum_w, sum_w_r2 and H_bound,
    b_bound, sum_w_bound, sum_w_r2_bound: how far the kernel's fp64 sums may lie from them when it decides the borderline pixels as `decided` (H,W) says (the kernel's own
    decisions, used on the borderline pixels only; without it the restatement's).  unresolved: borderline pixels that
    `decided` takes but for which the restatement has no value (its cell is not defined): no bound covers them."""
    depth = np.asarray(depth, np.float32)
    Hh, Ww = depth.shape
    vs = np.float64(np.float32(voxel_size))
    A, g0 = camera(K, T, voxel_size, origin) if pose is None else camera_from_pose(K, pose[0], pose[1], voxel_size, origin)
    ys, xs = np.meshgrid(np.arange(Hh, dtype=np.float64), np.arange(Ww, dtype=np.float64), indexing="ij")
    lattice = (xs % stride == 0) & (ys % stride == 0)
    w32 = np.ones((Hh, Ww), np.float32) if weights is None else np.asarray(weights, np.float32)
    with np.errstate(all="ignore"):
        cand = lattice & np.isfinite(depth) & (depth > 0) & np.isfinite(w32) & (w32 > 0)
        if valid is not None:
            cand &= np.asarray(valid).astype(bool)
        D = np.where(cand, depth, np.float32(1)).astype(np.float64)
        w = np.where(cand, w32, np.float32(0)).astype(np.float64)
        dirs = np.stack([A[a, 0] * xs + A[a, 1] * ys + A[a, 2] for a in range(3)])
        ddir = np.stack([DIR_EPS * (np.abs(A[a, 0] * xs) + np.abs(A[a, 1] * ys) + np.abs(A[a, 2])) for a in range(3)])
        g0b = g0[:, None, None]
        # section 16's position and margin with D in place of t_k
        g = D * dirs + g0b
        mg = D * ddir + 2.0 * EPS * (np.abs(D * dirs) + np.abs(g0b))
        inr, here, index, fr, change, face = grid.locate(g, mg)
        dv = [_corner(grid.d, c, index) for c in range(8)]
        f = np.where(here, _trilinear(dv, fr), np.nan)
        mf = sum(grid.Ld[a] * mg[a] for a in range(3)) + LERP_EPS * grid.Ld[3]
        band64 = np.float64(np.float32(band))
        grad = np.stack([
            _bilinear([dv[1] - dv[0], dv[3] - dv[2], dv[5] - dv[4], dv[7] - dv[6]], fr[1], fr[2]),
            _bilinear([dv[2] - dv[0], dv[3] - dv[1], dv[6] - dv[4], dv[7] - dv[5]], fr[0], fr[2]),
            _bilinear([dv[4] - dv[0], dv[5] - dv[1], dv[6] - dv[2], dv[7] - dv[3]], fr[0], fr[1])])
        # component a moves with the two other fractions by at most a mixed second difference (2 L_a each); across a
        # cell face it jumps by at most 2 L_a (the values on both sides lie in [-L_a, L_a]): a point within its margin of
        # a face may sit in the neighbouring cell in fp32
        dgrad = np.stack([2.0 * grid.Ld[a] * sum(mg[b] for b in range(3) if b != a) + GRAD_EPS * grid.Ld[3]
                          + np.where(face, 2.0 * grid.Ld[a], 0.0) for a in range(3)])
        n = grad / vs
        dn = dgrad / vs + EPS * np.abs(n)
        ok = cand & here & (np.abs(f) <= band64) & np.isfinite(n).all(0)
        border = cand & (change | (here & (np.abs(np.abs(f) - band64) <= mf)))
        takes = ok.copy()
        unresolved = np.zeros_like(takes)
        if decided is not None:
            decided = np.asarray(decided, bool)
            takes = np.where(border, decided, ok)
            unresolved = takes & ~(here & np.isfinite(f) & np.isfinite(n).all(0))
            takes &= ~unresolved
        r = np.where(takes, f / vs, 0.0)
        dr = np.where(takes, mf / vs + EPS * np.abs(f / vs), 0.0)
        c0 = (grid.dims.astype(np.float64) - 1.0) / 2.0
        q = g - c0[:, None, None]
        dq = mg + EPS * np.abs(q)
        J = np.concatenate([n, _cross(q, n)])
        dJ = np.concatenate([dn, _cross_bound(q, dq, n, dn)])
        J = np.where(takes[None], J, 0.0)
        dJ = np.where(takes[None], dJ, 0.0)
        w = np.where(takes, w, 0.0)
        count = int(takes.sum())
        # the sums and their bounds: every term's bound, and the fp64 roundings of the products (3) and of a sum of
        # `count` terms in any order (count), of the magnitudes
        round64 = (count + 4.0) * DBL
        aJ = np.abs(J)
        Hm = np.einsum("ip,jp,p->ij", J.reshape(6, -1), J.reshape(6, -1), w.reshape(-1))
        Hb = np.einsum("ip,jp,p->ij", aJ.reshape(6, -1), dJ.reshape(6, -1), w.reshape(-1))
        Hb = Hb + Hb.T + np.einsum("ip,jp,p->ij", dJ.reshape(6, -1), dJ.reshape(6, -1), w.reshape(-1)) \
            + round64 * np.einsum("ip,jp,p->ij", aJ.reshape(6, -1), aJ.reshape(6, -1), w.reshape(-1))
        bv = (J * (w * r)).reshape(6, -1).sum(1)
        bb = ((aJ * dr + dJ * np.abs(r) + dJ * dr) * w).reshape(6, -1).sum(1) + round64 * (aJ * np.abs(w * r)).reshape(6, -1).sum(1)
        sw, swr2 = float(w.sum()), float((w * r * r).sum())
        swb = round64 * sw
        swr2b = float((w * (2.0 * np.abs(r) * dr + dr * dr)).sum()) + round64 * swr2
    return {"takes_part": takes, "r": r, "J": J, "w": w, "g": g, "index": index, "m_g": mg, "m_f": mf, "r_bound": dr, "J_bound": dJ,
            "borderline": border, "lattice": lattice, "unresolved": unresolved, "H": Hm, "b": bv, "count": count,
            "sum_w": sw, "sum_w_r2": swr2, "H_bound": Hb, "b_bound": bb, "sum_w_bound": swb, "sum_w_r2_bound": swr2b}


# ---- the solve, the update and the loop ---------------------------------------------------------------------------------
def solve_reference(H, b, count, min_pixels=6, min_pivot=1e-9):
    """(status, delta): the stated solve in fp64.  1: count < min_pixels; 2: a diagonal entry of H that is not a positive
    finite number, or a pivot (the square of a diagonal entry of the Cholesky factor of S H S) below min_pivot."""
    if count < min_pixels:
        return 1, None
    dg = np.diag(H)
    if not (np.isfinite(dg).all() and (dg > 0).all()):
        return 2, None
    s = 1.0 / np.sqrt(dg)
    M = H * s[:, None] * s[None, :]
    L = np.zeros((6, 6))
    for j in range(6):
        p = M[j, j] - (L[j, :j] ** 2).sum()
        if not p >= min_pivot:
            return 2, None
        L[j, j] = math.sqrt(p)
        for i in range(j + 1, 6):
            L[i, j] = (M[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y = np.linalg.solve(L.T, np.linalg.solve(L, -(b * s)))
    delta = y * s
    if not np.isfinite(delta).all():
        return 2, None
    return 0, delta


def rotation(omega):
    """exp([omega]x) by Rodrigues, the small-angle series below |omega|^2 = 1e-8."""
    omega = np.asarray(omega, np.float64)
    t2 = float(omega @ omega)
    if t2 < 1e-8:
        a, b = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0), 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0)
    else:
        t = math.sqrt(t2)
        a, b = math.sin(t) / t, (1.0 - math.cos(t)) / t2
    Wx = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    return np.eye(3) + a * Wx + b * (Wx @ Wx)


def centre_world(dims, voxel_size, origin):
    vs = np.float64(np.float32(voxel_size))
    return np.asarray(origin, np.float32).astype(np.float64) + vs * (np.asarray(dims, np.float64) - 1.0) / 2.0


def apply_update(R, t, delta, dims, voxel_size, origin):
    """R <- Rd R, t <- Rd (t - cw) + cw + voxel_size v."""
    vs = np.float64(np.float32(voxel_size))
    cw = centre_world(dims, voxel_size, origin)
    Rd = rotation(delta[3:])
    return Rd @ R, Rd @ (t - cw) + cw + vs * delta[:3]


def step_bound(H, b, H_bound, b_bound):
    """(x_v, x_w): how far the translation and the rotation part of the update solved from sums within (H_bound,
    b_bound) of (H, b) may lie from those of delta = -H^-1 b, in the 2-norm.  In the variables the solve works in,
    M = S H S (unit diagonal) and y = S^-1 delta: from M~ y~ = -S b~ follows M (y~ - y) = -S (b~ - b) - S (H~ - H) S y~,
    so with k = |M^-1|_2, e = |S b_bound|_2 and E = |S H_bound S|_F: X <= k (e + E (|y| + X)), that is
    X <= k (e + E |y|) / (1 - k E) where k E < 1 (inf elsewhere).  The fp64 factorisation of M adds 64 DBL k |M|_2 |y|
    (six steps, each a few DBL of the magnitudes, amplified by the condition number: room for the constants of a
    backward-stable solve).  delta_i = s_i y_i, so a part of delta moves by at most X times the 2-norm of its s_i.
    (S itself is formed from the perturbed diagonal; H~ = S~^-1 M~ S~^-1 exactly, so the argument holds with S fixed to
    the restatement's: scaling is a change of variables, not an approximation.)"""
    dg = np.diag(H)
    if not (np.isfinite(H).all() and (dg > 0).all()):
        return math.inf, math.inf
    s = 1.0 / np.sqrt(dg)
    M = H * s[:, None] * s[None, :]
    try:
        Mi = np.linalg.inv(M)
    except np.linalg.LinAlgError:
        return math.inf, math.inf
    y = -Mi @ (s * b)
    k = np.linalg.norm(Mi, 2)
    e = np.linalg.norm(s * b_bound)
    E = np.linalg.norm(H_bound * s[:, None] * s[None, :])
    yn = np.linalg.norm(y)
    if not (np.isfinite(k) and k * E < 1.0):
        return math.inf, math.inf
    X = k * (e + E * yn) / (1.0 - k * E) + 64.0 * DBL * k * np.linalg.norm(M, 2) * yn
    return float(X * np.linalg.norm(s[:3])), float(X * np.linalg.norm(s[3:]))


def pose_bound(x, t, dims, voxel_size, origin):
    """(translation distance, rotation: 2-norm of the difference of the matrices) by which the updated pose may move when
    the update's parts move by x = (x_v, x_w): the rotation by at most x_w (|exp([a]x) - exp([b]x)|_2 <= |a - b|), the
    translation by x_w |t - cw| through it and by voxel_size x_v directly; and the fp32 rounding of the output (EPS of
    the magnitudes, 2 with the room for the fp64 roundings of the update itself; sqrt 3 of an entry's for a column)."""
    vs = float(np.float32(voxel_size))
    lever = float(np.linalg.norm(np.asarray(t, np.float64) - centre_world(dims, voxel_size, origin)))
    move = vs * x[0] + lever * x[1]
    return move + 2.0 * math.sqrt(3.0) * EPS * (float(np.abs(t).max()) + move), x[1] + 2.0 * math.sqrt(3.0) * EPS


def align_reference(grid, voxel_size, origin, depth, K, T, *, band, valid=None, weights=None, stride=1, iterations=10,
                    min_pixels=6, min_pivot=1e-9):
    """The loop on one view.  Returns a dict: poses (iterations+1 pairs (R, t) in fp64: before update i, the last the
    final one), T (4,4) the final pose rounded to fp32, history (iterations+1, 3), status, information (6,6), systems
    (the dict of align_system_reference at every pose) and step_bounds (iterations: `step_bound` at pose i, zeros at a
    pose where the view is stopped)."""
    dims = grid.dims
    R, t = pose_of(T)
    poses, history, systems, bounds = [], [], [], []
    status = 0
    for it in range(iterations + 1):
        sysm = align_system_reference(grid, voxel_size, origin, depth, K, T, band=band, valid=valid, weights=weights,
                                      stride=stride, pose=(R, t))
        poses.append((R.copy(), t.copy()))
        systems.append(sysm)
        history.append((float(sysm["count"]), sysm["sum_w"], sysm["sum_w_r2"]))
        if it == iterations:
            break
        delta = None
        if status == 0:
            status, delta = solve_reference(sysm["H"], sysm["b"], sysm["count"], min_pixels, min_pivot)
        if status == 0:
            bounds.append(step_bound(sysm["H"], sysm["b"], sysm["H_bound"], sysm["b_bound"]))
            R, t = apply_update(R, t, delta, dims, voxel_size, origin)
        else:
            bounds.append((0.0, 0.0))
    Tout = np.asarray(T, np.float32).copy()
    Tout[:3, :3], Tout[:3, 3] = R.astype(np.float32), t.astype(np.float32)
    return {"poses": poses, "T": Tout, "history": np.array(history), "status": status, "information": systems[-1]["H"],
            "systems": systems, "step_bounds": bounds}


def pose_error(T, T_true):
    """(translation distance, rotation angle in radians) between two poses."""
    T, T_true = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    dR = T[:3, :3] @ T_true[:3, :3].T
    return float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), float(math.acos(min(1.0, max(-1.0, (np.trace(dR) - 1.0) / 2.0))))


def perturbed(T, omega, shift):
    """The pose T turned by exp([omega]x) about the camera centre and moved by `shift`; fp32."""
    T = np.asarray(T, np.float64).copy()
    T[:3, :3] = rotation(omega) @ T[:3, :3]
    T[:3, 3] += np.asarray(shift, np.float64)
    return T.astype(np.float32)


def records_per_view(size, stride):
    H, W = size
    return (-(-(-(-H // stride)) // TILE)) * (-(-(-(-W // stride)) // TILE))


# ---- analytic depth maps ------------------------------------------------------------------------------------------------
def _rays(K, T, size):
    """Camera centre o (3,) and the rays v (3,H,W) with camera z component 1: the point at depth D is o + D v."""
    H, W = size
    K, T = np.asarray(K, np.float32).astype(np.float64), np.asarray(T, np.float32).astype(np.float64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cam = np.linalg.solve(K[:3, :3], np.stack([xs.ravel(), ys.ravel(), np.ones(H * W)]))
    return T[:3, 3], (T[:3, :3] @ cam).reshape(3, H, W)


def _sphere_depth(o, v, centre, radius):
    """The depth at which the rays meet the sphere from outside (the near root), inf where they miss it."""
    oc = o - np.asarray(centre, np.float64)
    a, b, c = (v * v).sum(0), (v * oc[:, None, None]).sum(0), float(oc @ oc) - radius * radius
    disc = b * b - a * c
    with np.errstate(all="ignore"):
        root = np.sqrt(np.where(disc > 0, disc, np.nan))
        D = (-b - root) / a
    return np.where(np.isfinite(D) & (D > 0), D, np.inf)


def sphere_depth(K, T, size):
    """The analytic z-depth of section 15's sphere as the camera (K, T) sees it, 0 where the ray misses it; fp32."""
    o, v = _rays(K, T, size)
    D = _sphere_depth(o, v, SPHERE["centre"], SPHERE["radius"])
    return np.where(np.isfinite(D), D, 0.0).astype(np.float32)


# ---- the cases of align_system: the analytic sphere, the pose off by about half a voxel and half a degree -------------
SPHERE_BAND = 0.15                                   # 1.5 voxels: the perturbation moves the surface by about 0.6
TWISTS = (((0.004, -0.006, 0.005), (0.03, -0.025, 0.03)), ((-0.005, 0.004, 0.006), (-0.02, 0.035, 0.025)),
          ((0.006, 0.005, -0.004), (0.03, 0.03, -0.02)))     # (omega, shift): 0.5 degrees, 0.05 = half a voxel


def _sphere_views(cameras, size):
    """depth (V,H,W) from the true poses, K (V,4,4), the perturbed T (V,4,4) and the true T."""
    Ks, Ts = [np.asarray(c[0], np.float32) for c in cameras], [np.asarray(c[1], np.float32) for c in cameras]
    depth = np.stack([sphere_depth(K, T, size) for K, T in zip(Ks, Ts)])
    off = np.stack([perturbed(T, *TWISTS[v % len(TWISTS)]) for v, T in enumerate(Ts)])
    return depth, np.stack(Ks), off, np.stack(Ts)


def _case(name, variant, cameras, size, hits=True, depth=None, **kw):
    def make():
        (s, w, _), mw = sphere_variants()[variant]
        d, K, T, T_true = _sphere_views(cameras(size), size)
        opts = dict(band=SPHERE_BAND, stride=1, valid=None, weights=None)
        for key, val in kw.items():
            opts[key] = val(d) if callable(val) else val
        if depth is not None:
            d = depth(d)
        return {"id": name, "state": (s, w), "min_weight": mw, "voxel_size": SPHERE["voxel_size"], "origin": SPHERE["origin"],
                "depth": d, "K": K, "T": T, "T_true": T_true, "size": size, "kw": opts, "hits": hits,
                "small": len(range(0, size[0], opts["stride"])) * len(range(0, size[1], opts["stride"])) < 100}
    return make


def _one(name):
    return lambda size: [sphere_camera(name, size)]


def _valid_mask(d):
    rng = np.random.default_rng(7)
    return rng.random(d.shape) < 0.85


def _pixel_weights(d):
    """Weights in [0.5, 2) with a 0, a negative one, a NaN and an inf among them (pixels that must not take part)."""
    rng = np.random.default_rng(11)
    w = (0.5 + 1.5 * rng.random(d.shape)).astype(np.float32)
    flat = w.reshape(d.shape[0], -1)
    n = flat.shape[1]
    for k, bad in enumerate((0.0, -1.0, np.nan, np.inf, -np.inf)):
        flat[:, (n // 2 + 3 * k) % n] = bad
    return w


def _bad_depths(d):
    """Depth entries of 0, a negative one, NaN and +-inf around the middle of every map."""
    d = d.copy()
    flat = d.reshape(d.shape[0], -1)
    n = flat.shape[1]
    for k, bad in enumerate((0.0, -0.7, np.nan, np.inf, -np.inf)):
        flat[:, (n // 2 + 5 * k + 1) % n] = bad
    return d


def _far_depth(d):
    return np.ones_like(d)


# name -> maker.  `small`: the stride lattice has fewer than 100 pixels, so "100 pixels take part" cannot be asked of it
# (1 x 1 is the extreme); the share of the lattice pixels is asked of every hitting case.
_TABLE = {}
for _size in SPHERE_SIZES:
    for _cam in ("outside", "rolled"):
        _n = f"sphere_{_cam}_{_size[0]}x{_size[1]}"
        _TABLE[_n] = _case(_n, "sphere", _one(_cam), _size)
    for _stride in (2, 3):
        _n = f"stride{_stride}_rolled_{_size[0]}x{_size[1]}"
        _TABLE[_n] = _case(_n, "sphere", _one("rolled"), _size, stride=_stride)
_TABLE["stride2_views3_37x61"] = _case("stride2_views3_37x61", "sphere", lambda size: list(zip(*three_views(size))), (37, 61),
                                       stride=2)
_TABLE["stride3_outside_37x61"] = _case("stride3_outside_37x61", "sphere", _one("outside"), (37, 61), stride=3)
_TABLE["valid_weights_rolled_23x31"] = _case("valid_weights_rolled_23x31", "sphere", _one("rolled"), (23, 31),
                                             valid=_valid_mask, weights=_pixel_weights)
_TABLE["bad_depths_outside_23x31"] = _case("bad_depths_outside_23x31", "sphere", _one("outside"), (23, 31), depth=_bad_depths)
for _variant in ("hole", "nan_under_weight_0", "min_weight"):
    _n = f"{_variant}_rolled_23x31"
    _TABLE[_n] = _case(_n, _variant, _one("rolled"), (23, 31))
_TABLE["away_23x31"] = _case("away_23x31", "sphere", _one("away"), (23, 31), hits=False, depth=_far_depth)
_TABLE["shape_1x1"] = _case("shape_1x1", "sphere", lambda size: [shape_camera(size)], (1, 1))
_TABLE["shape_1x1029"] = _case("shape_1x1029", "sphere", lambda size: [shape_camera(size)], (1, 1029))
_TABLE["views3_37x61"] = _case("views3_37x61", "sphere", lambda size: list(zip(*three_views(size))), (37, 61))

CASE_IDS = tuple(_TABLE)


@functools.lru_cache(maxsize=None)
def align_case(name):
    """One case: made once, never modified."""
    return _TABLE[name]()


def case_grid(c):
    return grid_of(c["state"][0], c["state"][1], c["min_weight"])


def case_reference(c, v, decided=None):
    kw = c["kw"]
    return align_system_reference(case_grid(c), c["voxel_size"], c["origin"], c["depth"][v], c["K"][v], c["T"][v],
                                  band=kw["band"], stride=kw["stride"],
                                  valid=None if kw["valid"] is None else kw["valid"][v],
                                  weights=None if kw["weights"] is None else kw["weights"][v], decided=decided)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of one case with its own decisions, a dict per view: computed once, shared, never modified."""
    c = align_case(name)
    return [case_reference(c, v) for v in range(c["K"].shape[0])]


# ---- a state on which three columns of J are exactly zero: the plane d = z - z0 -----------------------------------------
def plane_state(dims=(12, 11, 10), z0=4.5):
    """sdf_sum = voxel_size (k - z0), unit weights: the gradient is (0, 0, voxel_size) in every cell, exactly (the
    differences along x and y are exact zeros), so n_x = n_y = 0 and (q x n)_z = 0: H has three zero columns."""
    nx, ny, nz = dims
    vs = np.float32(0.125)
    s = np.broadcast_to(((np.arange(nz, dtype=np.float32) - np.float32(z0)) * vs)[:, None, None], (nz, ny, nx))
    return np.ascontiguousarray(s, np.float32), np.ones((nz, ny, nx), np.float32), float(vs), (0.0, 0.0, 0.0)


def plane_view(size=(17, 19)):
    """A camera in front of the plane, looking along +z, with the constant depth that puts every pixel on it."""
    H, W = size
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (0.7, 0.65, -1.0)
    K = _intrinsics(40.0, 40.0, (W - 1) / 2.0, (H - 1) / 2.0)
    depth = np.full((1, H, W), 1.0 + 4.5 * 0.125 + 0.03, np.float32)
    return depth, K[None], T[None]


# ---- the end-to-end scene: three planes and a sphere, seen from inside ---------------------------------------------------
# A room corner: three planes whose normals are tilted off the axes and off each other, and a sphere off their axes.  The
# planes fix the three rotations and, through their three independent normals, the three translations; one plane and one
# sphere (synthetic.fusion_scene) would leave the rotation about the plane's normal through the sphere's centre free.
CORNER = dict(dims=(32, 32, 32), voxel_size=0.1, origin=(0.0, 0.0, 0.0), trunc=0.3, size=(48, 64),
              planes=(((-1.0, 0.12, 0.05), -2.55), ((0.08, -1.0, 0.1), -2.35), ((0.06, -0.09, -1.0), -2.6)),
              centre=(1.75, 1.55, 2.05), radius=0.45)


def corner_depth(K, T, size):
    """The analytic z-depth of the corner scene from a camera inside it (the nearest of the planes n.p = c met from
    their free side n.p > c and the sphere); fp32."""
    o, v = _rays(K, T, size)
    best = _sphere_depth(o, v, CORNER["centre"], CORNER["radius"])
    for n, c in CORNER["planes"]:
        n = np.asarray(n, np.float64)
        nv = (v * n[:, None, None]).sum(0)
        with np.errstate(all="ignore"):
            D = (c - float(n @ o)) / nv
        best = np.minimum(best, np.where((nv < 0) & (D > 0), D, np.inf))
    return np.where(np.isfinite(best), best, 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def corner_views():
    """K (4,4,4), T (4,4,4) fp32 and depth (4,H,W): three integrating poses and a fourth, all inside the room looking
    into the corner."""
    size = CORNER["size"]
    eyes = ((0.85, 0.95, 0.55), (1.15, 0.7, 0.75), (0.7, 1.2, 0.8), (1.0, 0.9, 0.65))
    targets = ((2.0, 1.8, 2.2), (1.9, 1.9, 2.1), (2.1, 1.7, 2.15), (1.95, 1.85, 2.15))
    rolls = (0.0, 0.15, -0.1, 0.05)
    K = np.stack([_intrinsics(46.0, 44.0, (size[1] - 1) / 2.0 + 0.8, (size[0] - 1) / 2.0 - 0.6)] * 4)
    T = np.stack([look_at(e, g, roll=r) for e, g, r in zip(eyes, targets, rolls)])
    depth = np.stack([corner_depth(K[v], T[v], size) for v in range(4)])
    return K, T, depth


CORNER_TWIST = ((0.010, -0.009, 0.008), (0.06, -0.05, 0.06))      # 0.9 degrees and 0.098: one voxel


def corner_start():
    """The fourth view's starting pose: about one voxel and one degree off (inside the band trunc / 2 = 1.5 voxels)."""
    return perturbed(corner_views()[1][3], *CORNER_TWIST)


@functools.lru_cache(maxsize=None)
def corner_state():
    """The restatement's integration of the three views, rounded to the fp32 state (sdf_sum, weight)."""
    K, T, depth = corner_views()
    ref = tsdf_integrate_reference(depth[:3], K[:3], T[:3], CORNER["dims"], CORNER["voxel_size"], CORNER["origin"],
                                   CORNER["trunc"])
    return ref["sdf_sum"].astype(np.float32), ref["weight"].astype(np.float32)


CORNER_ITERATIONS = 8
CORNER_BAND = float(np.float32(CORNER["trunc"]) / np.float32(2))       # the method's default


def corner_loop(state, iterations=CORNER_ITERATIONS):
    """The restatement's loop of the fourth view on `state` (sdf_sum, weight) from corner_start()."""
    K, T, depth = corner_views()
    grid = grid_of(state[0], state[1], 1.0)
    return align_reference(grid, CORNER["voxel_size"], CORNER["origin"], depth[3], K[3], corner_start(),
                           band=CORNER_BAND, iterations=iterations)
