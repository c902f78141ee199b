"""numpy restatement of the normals of a bare cloud (multi_view_stereonet_amd/fusion.py:
cloud_normals; csrc/mvsn_cloud_normals.hip).

The neighbourhood is `cloud_reference`'s acceptance (the brute force over every pair with the kernel's fp32 operations);
the differences are quantised as the kernel quantises them (one fp32 multiply by 1/h, one exact scaling by 2^20, rint:
ties to even) and summed in int64, so the ten sums are the device's exactly, whatever the order of the support.  The
covariance and the cyclic Jacobi iteration follow in fp64, operation by operation, vectorised over the points; next to
them `numpy.linalg.eigh` of the same covariance gives the eigenpairs an independent solver finds, which is what the
device is held to."""
import functools

import numpy as np

from cloud_reference import CHUNK_ELEMENTS, radius_scalars, squared_distances, target_cells

SWEEPS = 6
MAX_NEIGHBOURS = 1 << 20
QUANTUM = np.float32(2.0 ** 20)
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))               # (p, q, the third index)
EPS = 2.0 ** -52


def moments(points, support, radius):
    """(count (N,) int64, S (N,3) int64, SS (N,3,3) int64): the exact sums of u_a and u_a u_b over the accepted neighbours,
    u_a = rint((d_a * inv) * 2^20) of the fp32 differences d = point - neighbour."""
    q = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    p = np.ascontiguousarray(support, dtype=np.float32).reshape(-1, 3)
    _, inv, r2 = radius_scalars(radius)
    n, m = q.shape[0], p.shape[0]
    count, S, SS = np.zeros(n, np.int64), np.zeros((n, 3), np.int64), np.zeros((n, 3, 3), np.int64)
    if n == 0 or m == 0:
        return count, S, SS
    usable, _, _ = target_cells(p, radius)
    chunk = max(1, CHUNK_ELEMENTS // (4 * m))
    for a in range(0, n, chunk):
        qa = q[a:a + chunk]
        d2 = squared_distances(qa, p)
        with np.errstate(all="ignore"):
            ok = (d2 <= r2) & usable[None, :]
            d = qa[:, None, :] - p[None, :, :]                          # the differences the walk formed
            s = d * inv
            u = np.rint(s * QUANTUM)
        assert d.dtype == s.dtype == u.dtype == np.float32
        u = np.where(ok[:, :, None], u, np.float32(0)).astype(np.int64)
        assert (np.abs(u) < 2 ** 21).all()
        count[a:a + chunk] = ok.sum(axis=1)
        S[a:a + chunk] = u.sum(axis=1)
        for i in range(3):
            for j in range(i, 3):
                SS[a:a + chunk, i, j] = SS[a:a + chunk, j, i] = (u[:, :, i] * u[:, :, j]).sum(axis=1)
    return count, S, SS


def covariance(count, S, SS):
    """(N,3,3) fp64 in units of (2^-20 cells)^2: m_a = S_a / n, C_ab = S_ab / n - m_a m_b, one operation per step; zeros
    where n = 0."""
    n = np.maximum(count, 1).astype(np.float64)
    m = S.astype(np.float64) / n[:, None]
    C = SS.astype(np.float64) / n[:, None, None] - m[:, :, None] * m[:, None, :]
    return np.where((count > 0)[:, None, None], C, 0.0)


def jacobi(C, sweeps=SWEEPS):
    """(lambda (N,3) ascending, V (N,3,3) with the eigenvectors in the columns): cyclic Jacobi on the symmetric 3x3s in
    fp64, `sweeps` sweeps over the pairs (0,1), (0,2), (1,2), the kernel's steps one by one."""
    A = np.array(C, dtype=np.float64)
    N = A.shape[0]
    V = np.broadcast_to(np.eye(3), (N, 3, 3)).copy()
    for _ in range(sweeps):
        for p, q, r in PAIRS:
            apq = A[:, p, q].copy()
            live = apq != 0.0
            with np.errstate(all="ignore"):
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                mag = np.abs(theta) + np.sqrt(theta * theta + 1.0)
                t = np.where(theta < 0.0, -1.0, 1.0) / mag
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                tau = t * apq
            t, c, s, tau = (np.where(live, x, y) for x, y in ((t, 0.0), (c, 1.0), (s, 0.0), (tau, 0.0)))
            A[:, p, p] = A[:, p, p] - tau
            A[:, q, q] = A[:, q, q] + tau
            A[:, p, q] = A[:, q, p] = np.where(live, 0.0, apq)
            rp, rq = A[:, r, p].copy(), A[:, r, q].copy()
            A[:, r, p] = A[:, p, r] = np.where(live, c * rp - s * rq, rp)
            A[:, r, q] = A[:, q, r] = np.where(live, s * rp + c * rq, rq)
            vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
            V[:, :, p] = np.where(live[:, None], c[:, None] * vp - s[:, None] * vq, vp)
            V[:, :, q] = np.where(live[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1)
    for a, b in ((0, 1), (1, 2), (0, 1)):                               # the kernel's network; equal values keep their places
        swap = lam[:, b] < lam[:, a]
        la, lb = lam[:, a].copy(), lam[:, b].copy()
        lam[:, a], lam[:, b] = np.where(swap, lb, la), np.where(swap, la, lb)
        va, vb = V[:, :, a].copy(), V[:, :, b].copy()
        V[:, :, a], V[:, :, b] = np.where(swap[:, None], vb, va), np.where(swap[:, None], va, vb)
    return lam, V


def canonical_sign(n):
    """-1 where the component of largest magnitude (ties: the lowest axis) is negative, +1 elsewhere."""
    lead = np.take_along_axis(n, np.abs(n).argmax(axis=1)[:, None], axis=1)[:, 0]      # argmax: the first of equal maxima
    return np.where(lead < 0.0, -1.0, 1.0)


def oriented(n, points, viewpoint):
    """`n` (N,3) fp64 with the sign rule applied: canonical, and with a finite viewpoint row flipped where
    (n_x e_x + n_y e_y) + n_z e_z < 0, e = viewpoint - point in fp64, and left canonical where that is 0."""
    sign = canonical_sign(n)
    if viewpoint is not None:
        v = np.asarray(viewpoint, np.float32).reshape(-1, 3)
        v = np.broadcast_to(v, (len(n), 3))
        with np.errstate(all="ignore"):
            e = v.astype(np.float64) - np.asarray(points, np.float32).astype(np.float64)
            dot = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
        decides = np.isfinite(v).all(axis=1) & (dot != 0.0)
        sign = np.where(decides, np.where(dot < 0.0, -1.0, 1.0), sign)
    return n * sign[:, None]


def cloud_normals_reference(points, radius, *, support=None, viewpoint=None, min_neighbours=3, min_gap=2.0 ** -20):
    """dict of
      normals (N,3) f32, eigenvalues (N,3) f32, count (N,) i32     what the device returns, from the Jacobi iteration
      lam (N,3) f64, gap (N,) f64                                  Jacobi's eigenvalues in units of (2^-20 cells)^2 and the
                                                                   relative gap (lam1 - lam0) / lam2 (0 where lam2 <= 0)
      eigh_normals (N,3) f64, eigh_lam (N,3) f64                   numpy.linalg.eigh of the same covariance, the normal
                                                                   with the same sign rule and zero pattern; world units
      jacobi_normals (N,3) f64                                     before the rounding to fp32
      scale                                                        (h 2^-20)^2 in fp64: units -> squared world units
    """
    q = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    p = q if support is None else np.ascontiguousarray(support, dtype=np.float32).reshape(-1, 3)
    h, _, _ = radius_scalars(radius)
    count, S, SS = moments(q, p, radius)
    solved = (count >= 1) & (count <= MAX_NEIGHBOURS)
    C = covariance(np.where(solved, count, 0), S, SS)
    lam, V = jacobi(C)
    unit = np.float64(h) * 2.0 ** -20
    scale = unit * unit
    with np.errstate(all="ignore"):
        defined = solved & (count >= int(min_neighbours)) & ~(lam[:, 1] - lam[:, 0] <= np.float64(min_gap) * lam[:, 2])
        gap = np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / np.where(lam[:, 2] > 0, lam[:, 2], 1.0), 0.0)
    jn = np.where(defined[:, None], oriented(V[:, :, 0], q, viewpoint), 0.0)
    w, E = np.linalg.eigh(C)                                            # ascending
    en = np.where(defined[:, None], oriented(E[:, :, 0], q, viewpoint), 0.0)
    with np.errstate(all="ignore"):
        ev = np.where(solved[:, None], lam * scale, 0.0).astype(np.float32)
    return {"normals": jn.astype(np.float32), "eigenvalues": ev, "count": count.astype(np.int32), "lam": lam, "gap": gap,
            "eigh_normals": en, "eigh_lam": np.where(solved[:, None], w * scale, 0.0), "jacobi_normals": jn,
            "defined": defined, "scale": scale, "covariance": C}


def angle(a, b):
    """(N,) the angle between the rows of a and b in radians, from the cross product (exact near 0); 0 where both rows
    are zero."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(axis=1))


def axis_angle(a, b):
    """The angle between the LINES through a and b: the sign of either is ignored."""
    x = angle(a, b)
    return np.minimum(x, np.pi - x)


def solver_term(ref, K):
    """(N,) K 2^-52 lam2 / (lam1 - lam0): what the device's eigenvector may differ from eigh's by, in radians (and, times
    lam2, its eigenvalues); inf where the gap is 0."""
    with np.errstate(all="ignore"):
        return np.where(ref["gap"] > 0, K * EPS / np.where(ref["gap"] > 0, ref["gap"], 1.0), np.inf)


# ---- the cases of the GPU tests (tests/test_cloud_normals_gpu.py runs them, test_cloud_normals_reference_cpu.py holds them
# to the conditions that keep the GPU tests from passing vacuously) ---------------------------------------------------------
K_JACOBI = 4                    # the angle between Jacobi's and eigh's normal: 2.44 units at worst, rounded up (test_cloud_normals_reference_cpu.py)
MIN_GAP = 2.0 ** -20


def _surface(rng, n, scale=1.0, noise=0.01):
    """n points near the saddle z = 0.3 x y over [-1,1]^2, times scale."""
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    z = 0.3 * xy[:, 0] * xy[:, 1] + rng.normal(0.0, noise, n)
    return (np.column_stack([xy, z]) * scale).astype(np.float32)


def _hand():
    """The hand case of test_cloud_gpu.py (duplicates, d2 == r2 and one ulp above, cell faces, non-finite rows, queries
    beyond the grid), restated here because a test module is not imported from another: a surface dense enough to carry
    normals, with the special rows written over it."""
    nq, nt, h = 1027, 1031, 0.25
    hf = np.float32(h)
    rng = np.random.default_rng(41)
    t = _surface(rng, nt, 3.0, 0.02)
    q = _surface(rng, nq, 3.2, 0.02)
    t[100:110] = t[5]
    q[5], q[6], q[7] = t[5], t[700], t[105] + np.float32(0.01)
    t[20], q[10] = (8.0, 8.0, 8.0), (8.25, 8.0, 8.0)
    t[21], q[11] = (0.0, 0.0, 8.0), (0.25, 1.5 * 2.0 ** -14, 8.0)
    for j, k in enumerate([(-3, 2, 0), (0, 0, 0), (5, -7, 1), (-1, -1, -1)]):
        t[200 + j] = np.asarray(k, np.float32) * hf
        q[200 + j] = t[200 + j] + np.array([0.1, -0.1, 0.05], np.float32)
        q[210 + j] = t[200 + j]
    below = np.nextafter(np.float32(0), np.float32(-np.inf))
    t[300], t[301], t[302] = (below, 1.1, 1.1), (1.1, -2.0 ** -22, 1.1), (1.5, 1.5, -2.0 ** -25)
    q[300], q[301], q[302] = (0.01, 1.1, 1.1), (1.1, 0.02, 1.1), (1.5, 1.5, 0.03)
    q[303], q[304] = (below, 1.1, 1.1), (-0.2, -0.2, np.nextafter(np.float32(-0.25), np.float32(-1)))
    q[400], q[401], q[402] = (np.nan, 0, 0), (np.inf, 0, 0), (0.1, -np.inf, np.nan)
    t[400], t[401], t[402] = (np.nan, 0.1, 0.1), (0.1, -np.inf, 0.1), (np.nan, np.nan, np.nan)
    q[403] = (0.1, 0.1, 0.1)
    q[500], q[501], q[502] = (1.0e6, 0, 0), (2.0 ** 20 * h + 0.1, 0, -(2.0 ** 20) * h - 1.0), (-3.0e38, 3.0e38, 0)
    t[0], t[nt - 1] = (5.0, 5.0, 5.0), (5.0, 5.0, -5.0)
    q[0], q[nq - 1] = (5.1, 5.0, 5.0), (5.0, 5.05, -5.0)
    # the kinds of zero normal that need neighbours of their own, far from everything else
    # collinear: five support points on a line through the query
    line = np.array([-9.0, 9.0, 0.0]) + np.outer(np.linspace(-0.2, 0.2, 5), [1.0, 0.5, 0.25])
    t[600:605], q[600] = line.astype(np.float32), line[2].astype(np.float32)
    # coincident: four copies of one point, the query next to them
    t[610:614], q[610] = (9.0, -9.0, 0.0), (9.0625, -9.0, 0.0)
    # an isotropic blob: the eight corners of a cube around the query (exact in fp32)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * 0.125
    t[620:628], q[620] = (np.array([-9.0, -9.0, 4.0]) + corners).astype(np.float32), (-9.0, -9.0, 4.0)
    # too few: two support points
    t[630:632], q[630] = [(9.0, 9.0, 4.0), (9.0, 9.125, 4.0)], (9.0, 9.0625, 4.0)
    return dict(points=q, support=t, h=h, zero_rows=dict(few=630, not_finite=400, collinear=600, coincident=610, blob=620))


def _sized(n, m, seed, h=0.3):
    rng = np.random.default_rng(seed)
    return dict(points=_surface(rng, n), support=_surface(rng, m), h=h)


def _one_cell():
    rng = np.random.default_rng(143)
    t = rng.uniform(0.26, 0.49, (1027, 3))
    t[:, 2] = 0.3 + 0.2 * (t[:, 0] - 0.26) + rng.normal(0, 0.002, 1027)                 # a slanted sheet inside cell (1,1,1)
    t = t.astype(np.float32)
    t[500:520] = t[3]
    q = rng.uniform(0.1, 0.65, (300, 3)).astype(np.float32)
    return dict(points=q, support=t, h=0.25)


def _far():
    h = 0.25
    rng = np.random.default_rng(144)
    shift = np.array([5.0e5 * h, -5.0e5 * h, 0.0])
    t = (_surface(rng, 800).astype(np.float64) + shift).astype(np.float32)
    q = (_surface(rng, 300).astype(np.float64) + shift).astype(np.float32)
    return dict(points=q, support=t, h=h)


def _tiny():
    h = 2.0 ** -74
    rng = np.random.default_rng(145)
    t = (_surface(rng, 1500).astype(np.float64) * 4 * h).astype(np.float32)
    q = (_surface(rng, 300).astype(np.float64) * 4 * h).astype(np.float32)
    return dict(points=q, support=t, h=h)


def _limit():
    """2^20 + 1 support points in cell (1,1,1) of h = 0.5: a slanted sheet of 1024 x 1024 points within 0.12 of
    (0.75, 0.75, 0.75) along x and y, and one more point at x = 0.99.  Query 0 at x = 0.45 is 0.54 from that point and
    at most 0.44 from the sheet: exactly 2^20 neighbours, the last size that gets a normal.  Query 1 at x = 0.6 reaches
    all 2^20 + 1."""
    g = (np.arange(1024, dtype=np.float64) - 511.5) / 1024.0 * 0.24                    # |g| < 0.12
    x, y = np.meshgrid(g, g, indexing="ij")
    z = 0.1 * x + 0.05 * y
    sheet = np.stack([x + 0.75, y + 0.75, z + 0.75], axis=-1).reshape(-1, 3)
    t = np.concatenate([sheet, [[0.99, 0.75, 0.75]]]).astype(np.float32)
    q = np.array([[0.45, 0.75, 0.75], [0.6, 0.75, 0.75]], np.float32)
    return dict(points=q, support=t, h=0.5)


_CASES = {"hand": _hand, "n1": lambda: _sized(1, 400, 151), "n255": lambda: _sized(255, 400, 152),
          "n256": lambda: _sized(256, 400, 153), "n257": lambda: _sized(257, 400, 154),
          "m1": lambda: dict(points=_surface(np.random.default_rng(155), 40, 0.3), support=np.array([[0.1, 0.1, 0.0]], np.float32), h=0.3),
          "m2": lambda: dict(points=_surface(np.random.default_rng(156), 40, 0.3),
                             support=np.array([[0.1, 0.1, 0.0], [0.2, 0.1, 0.0]], np.float32), h=0.3),
          "one_cell_1027": _one_cell, "far": _far, "tiny": _tiny, "limit": _limit}
CASE_IDS = tuple(_CASES)
SPARSE_IDS = ("m1", "m2")       # a support of one or two points defines no normal anywhere: exempt from the quarter rule


@functools.lru_cache(maxsize=None)
def case(name):
    """Made once, never modified.  Every case uses itself as support where `support` is None ("hand_self")."""
    if name == "hand_self":
        c = _hand()
        return dict(points=c["support"], support=None, h=c["h"])
    return _CASES[name]()


@functools.lru_cache(maxsize=None)
def case_reference(name, viewpoint=None):
    """The restatement of a case (viewpoint: None, "one" = (0.3, -0.2, 5.0), "rows" = per point, some rows special)."""
    c = case(name)
    return cloud_normals_reference(c["points"], c["h"], support=c["support"], viewpoint=case_viewpoint(name, viewpoint),
                                   min_gap=MIN_GAP)


def case_viewpoint(name, kind):
    if kind is None:
        return None
    if kind == "one":
        return np.array([0.3, -0.2, 5.0], np.float32)
    q = case(name)["points"]
    v = (np.nan_to_num(q.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) +
         np.random.default_rng(160).normal(0, 1.0, q.shape)).astype(np.float32)
    v[::7] = q[::7]                                                     # on the point: n . (v - p) == 0
    v[3::11, 1] = np.nan                                                # not finite: the canonical sign
    v[5::13, 0] = np.inf
    return v


# ---- the corner scene (DESIGN.md section 17's, as section 20's test back-projects it) ---------------------------------
SCENE_RADIUS = 0.12             # about three pixel footprints at the scene's depths
SCENE_MARGIN = 4                # pixels a point keeps from the nearest edge between two surfaces, in its own view
SCENE_MAX_ANGLE = 0.04          # radians: twice the 0.0197 the restatement shows over every interior point


@functools.lru_cache(maxsize=None)
def corner_cloud():
    """Section 20's target cloud (views 0-2 of the corner scene back-projected from their analytic depth maps) with its
    analytic normals, the camera centre of every point's view, and `interior`: the points whose window of
    2 SCENE_MARGIN + 1 pixels in their own view shows one surface only."""
    import cloud_register_reference as rr
    import tsdf_align_reference as ar
    s = rr.corner_scene()
    _, T, _ = ar.corner_views()
    H, W = ar.CORNER["size"]
    n = s["normals"].astype(np.float64)
    label = np.full(len(n), 3)
    for k, (pn, _) in enumerate(ar.CORNER["planes"]):
        pn = np.asarray(pn, np.float64)
        label[(n == (pn / np.linalg.norm(pn)).astype(np.float32)[None, :]).all(axis=1)] = k
    label = label.reshape(3, H, W)
    interior = np.zeros((3, H, W), bool)
    m = SCENE_MARGIN
    for y in range(m, H - m):                           # (an edge just outside a view's image is in another view's)
        for x in range(m, W - m):
            win = label[:, y - m:y + m + 1, x - m:x + m + 1].reshape(3, -1)
            interior[:, y, x] = (win == win[:, :1]).all(axis=1)
    centres = np.repeat(T[:3, :3, 3].astype(np.float32), H * W, axis=0)
    return dict(points=s["target"], normals=s["normals"], viewpoint=np.ascontiguousarray(centres),
                interior=interior.reshape(-1), scene=s)
