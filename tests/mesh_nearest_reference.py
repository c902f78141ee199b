"""numpy restatement of mesh_sample and mesh_nearest (multi_view_stereonet_amd/mesh.py; csrc/mvsn_mesh_sample.hip,
csrc/mvsn_mesh_nearest.hip): the operations of the kernels one for one, without the index.

The sampler's prefix is a plain cumulative sum of the integer weights and its draws are uint64 arithmetic (the 128-bit
product is a split multiply); mesh_nearest is the brute force over every (query, face) pair.  fp64 steps are numpy
float64 operations, one per step, and fp32 steps numpy float32 operations, so every output can be compared byte for byte.
"""
import numpy as np

BOX_CELLS = 512                      # mesh.NEAREST_BOX_CELLS
CELL_LIMIT = 1 << 20
GOLDEN_GAMMA = np.uint64(0x9E3779B97F4A7C15)
MASK32 = np.uint64(0xFFFFFFFF)


# ---- the draws -------------------------------------------------------------------------------------------------------
def splitmix(seed, c):
    """fin(seed + c * 0x9E3779B97F4A7C15) for a uint64 array c: splitmix64's finaliser as ransac_draw forms it."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.asarray(c, dtype=np.uint64) * GOLDEN_GAMMA
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def umul64hi(a, b):
    """The high 64 bits of the 128-bit product of uint64 arrays, by a split multiply."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    s = np.uint64(32)
    a0, a1, b0, b1 = a & MASK32, a >> s, b & MASK32, b >> s
    with np.errstate(over="ignore"):
        mid = a1 * b0 + ((a0 * b0) >> s)              # < 2^64: (2^32-1)^2 + 2^32 - 1
        mid2 = a0 * b1 + (mid & MASK32)               # likewise
        return a1 * b1 + (mid >> s) + (mid2 >> s)


# ---- the faces that take part ------------------------------------------------------------------------------------------
def valid_faces(vertices, faces):
    """(F,) bool: every index inside [0, M) and every vertex finite; and the (F,3,3) fp32 corners (0 where not valid)."""
    vertices, faces = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    m = len(vertices)
    inside = ((faces >= 0) & (faces < m)).all(axis=1)
    safe = np.where(inside[:, None], faces, 0)
    corners = vertices[safe] if m else np.zeros((len(faces), 3, 3), np.float32)
    ok = inside & np.isfinite(corners).all(axis=(1, 2))
    return ok, np.where(ok[:, None, None], corners, np.float32(0))


# ---- mesh_sample -------------------------------------------------------------------------------------------------------
def sample_weights(vertices, faces):
    """(q, area): the integer weight of every face, uint64, and its fp64 area."""
    ok, p = valid_faces(vertices, faces)
    p = p.astype(np.float64)
    ab, ac = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    nn = (nx * nx + ny * ny) + nz * nz
    area = np.where(ok, 0.5 * np.sqrt(nn), 0.0)
    a_max = area.max() if len(area) else 0.0
    if a_max == 0.0:
        return np.zeros(len(area), np.uint64), area
    e = int(np.frexp(a_max)[1]) - 1                   # ilogb
    scale = np.ldexp(1.0, 31 - e) if 31 - e <= 1023 else 0.0
    with np.errstate(under="ignore"):
        return np.floor(area * scale).astype(np.uint64), area


def sample_prefix(vertices, faces):
    """P[f] = q_0 + ... + q_f, uint64."""
    return np.cumsum(sample_weights(vertices, faces)[0], dtype=np.uint64)


def sample_reference(vertices, faces, n, seed=0, normals=None, colors=None):
    """The five outputs of mesh_sample (normals / colors None where not asked for), and `total` = P[F-1]."""
    vertices, faces = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    P = sample_prefix(vertices, faces)
    total = int(P[-1]) if len(P) else 0
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        c = np.uint64(3) * i
    z1, z2, z3 = (splitmix(seed, c + np.uint64(j)) for j in (1, 2, 3))
    out = {"total": total, "points": np.zeros((n, 3), np.float32), "face": np.full(n, -1, np.int64),
           "weights": np.zeros((n, 3), np.float32),
           "normals": np.zeros((n, 3), np.float32) if normals is not None else None,
           "colors": np.zeros((n, 3), np.uint8) if colors is not None else None}
    if total == 0 or n == 0:
        return out
    pick = umul64hi(z1, np.uint64(total))
    f = np.searchsorted(P, pick, side="right")        # the first row with P[row] > pick
    _, p = valid_faces(vertices, faces[f])
    p = p.astype(np.float64)
    u = (z2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    v = (z3 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    flip = u + v > 1.0
    u, v = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - v, v)
    w = np.stack([(1.0 - u) - v, u, v], axis=1)
    ab, ac = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    x = (p[:, 0] + u[:, None] * ab) + v[:, None] * ac
    out["points"], out["face"], out["weights"] = x.astype(np.float32), f.astype(np.int64), w.astype(np.float32)
    if normals is not None:
        nv = np.asarray(normals, np.float32)[faces[f]].astype(np.float64)
        with np.errstate(all="ignore"):
            s = (w[:, 0:1] * nv[:, 0] + w[:, 1:2] * nv[:, 1]) + w[:, 2:3] * nv[:, 2]
            length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
            defined = (length > 0.0) & np.isfinite(length)
            out["normals"] = np.where(defined[:, None], (s / length[:, None]).astype(np.float32), np.float32(0))
    if colors is not None:
        cv = np.asarray(colors, np.uint8)[faces[f]].astype(np.float64)
        s = (w[:, 0:1] * cv[:, 0] + w[:, 1:2] * cv[:, 1]) + w[:, 2:3] * cv[:, 2]
        y = np.floor(s + 0.5)
        out["colors"] = np.where(y > 0.0, np.where(y < 255.0, y, 255.0), 0.0).astype(np.uint8)
    return out


# ---- the distance of a point to a face (normative: DESIGN.md section 26) -----------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def closest(q, p):
    """q (...,3) fp32 against faces p (...,3,3) fp32 (broadcast against each other): (d2 fp32, x32 fp32, w fp64)."""
    q32, p32 = np.asarray(q, np.float32), np.asarray(p, np.float32)
    shape = np.broadcast_shapes(q32.shape[:-1], p32.shape[:-2])
    q32, p32 = np.broadcast_to(q32, shape + (3,)), np.broadcast_to(p32, shape + (3, 3))
    qd, P = q32.astype(np.float64), p32.astype(np.float64)
    a = P[..., 0, :]
    ab, ac, aq = P[..., 1, :] - a, P[..., 2, :] - a, qd - a
    n = _cross(ab, ac)
    nn = _dot(n, n)
    with np.errstate(all="ignore"):
        wb, wc = _dot(_cross(aq, ac), n) / nn, _dot(_cross(ab, aq), n) / nn
        wa = (1.0 - wb) - wc
        inside = (nn > 0.0) & (wb >= 0.0) & (wc >= 0.0) & (wa >= 0.0)
        x = (a + wb[..., None] * ab) + wc[..., None] * ac
    w = np.stack([wa, wb, wc], axis=-1)
    best = None
    for s in range(3):                                # the sides (a,b), (b,c), (c,a): ties to the earlier
        s1, s2 = (s + 1) % 3, (s + 2) % 3
        p0 = P[..., s, :]
        e, d = P[..., s1, :] - p0, qd - p0
        ee = _dot(e, e)
        with np.errstate(all="ignore"):
            r = _dot(d, e) / ee
        t = np.where(ee > 0.0, np.where(r > 0.0, np.where(r < 1.0, r, 1.0), 0.0), 0.0)
        xs = p0 + t[..., None] * e
        d = qd - xs
        dd = _dot(d, d)
        ws = np.zeros(shape + (3,))
        ws[..., s], ws[..., s1], ws[..., s2] = 1.0 - t, t, 0.0
        if best is None:
            best, xe, we = dd, xs, ws
        else:
            take = dd < best
            best, xe, we = np.where(take, dd, best), np.where(take[..., None], xs, xe), np.where(take[..., None], ws, we)
    x = np.where(inside[..., None], x, xe)
    w = np.where(inside[..., None], w, we)
    b0, b1, b2 = p32[..., 0, :], p32[..., 1, :], p32[..., 2, :]
    mn, mx = np.where(b1 < b0, b1, b0), np.where(b1 > b0, b1, b0)
    mn, mx = np.where(b2 < mn, b2, mn), np.where(b2 > mx, b2, mx)
    xf = x.astype(np.float32)
    x32 = np.where(xf < mn, mn, np.where(xf > mx, mx, xf))
    with np.errstate(all="ignore"):
        df = q32 - x32
        d2 = (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]
    return d2, x32, w


def radius_scalars(max_dist):
    """(h, 1/h, h*h), each formed once in fp32."""
    h = np.float32(max_dist)
    return h, np.float32(1) / h, h * h


def face_boxes(vertices, faces, max_dist):
    """(state, lo, hi): 0 takes no part / 1 boxed / 2 a finite vertex without a cell; the box of cells per face."""
    _, inv, _ = radius_scalars(max_dist)
    ok, p = valid_faces(vertices, faces)
    with np.errstate(all="ignore"):
        tl, th = p.min(axis=1) * inv, p.max(axis=1) * inv
        fl, fh = np.floor(tl), np.floor(th)
        inside = (np.isfinite(tl) & np.isfinite(th) & (fl >= -CELL_LIMIT) & (fh < CELL_LIMIT))
        lo, hi = np.where(inside, fl, 0).astype(np.int64), np.where(inside, fh, 0).astype(np.int64)
    state = np.where(ok, np.where(inside.all(axis=1), 1, 2), 0)
    return state, lo, hi


def count_reference(vertices, faces, max_dist):
    """(pairs, large, status) as mvsn_mesh_nearest_count reports them."""
    state, lo, hi = face_boxes(vertices, faces, max_dist)
    cells = np.prod((hi - lo + 1).astype(object), axis=1) if len(lo) else np.zeros(0, object)
    boxed = state == 1
    small = np.array([bool(b) and c <= BOX_CELLS for b, c in zip(boxed, cells)], bool)
    return int(sum(int(c) for c in cells[small])), int((boxed & ~small).sum()), int((state == 2).any())


def nearest_reference(points, vertices, faces, max_dist, chunk=1 << 21):
    """The five outputs of mesh_nearest by brute force over every (query, face) pair."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    vertices, faces = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    _, _, r2 = radius_scalars(max_dist)
    N = len(points)
    out = {"dist2": np.full(N, np.inf, np.float32), "face": np.full(N, -1, np.int64), "point": np.zeros((N, 3), np.float32),
           "weights": np.zeros((N, 3), np.float32), "within": np.zeros(N, np.int32)}
    ok, p = valid_faces(vertices, faces)
    rows = np.nonzero(ok)[0]
    if N == 0 or len(rows) == 0:
        return out
    p = p[rows]
    finite = np.isfinite(points).all(axis=1)
    step = max(1, chunk // len(rows))
    for a in range(0, N, step):
        q = points[a:a + step]
        d2, x32, w = closest(q[:, None, :], p[None])
        hit = (d2 <= r2) & finite[a:a + step, None]
        key = np.where(hit, (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows[None].astype(np.uint64),
                       np.uint64(2 ** 64 - 1))
        j = key.argmin(axis=1)
        i = np.arange(len(q))
        any_ = hit[i, j]
        out["within"][a:a + step] = hit.sum(axis=1)
        out["dist2"][a:a + step] = np.where(any_, d2[i, j], np.float32(np.inf))
        out["face"][a:a + step] = np.where(any_, rows[j], -1)
        out["point"][a:a + step] = np.where(any_[:, None], x32[i, j], np.float32(0))
        out["weights"][a:a + step] = np.where(any_[:, None], w[i, j].astype(np.float32), np.float32(0))
    return out


def cloud_reference(points, target, max_dist):
    """cloud_nearest's dist2 by brute force: the same fp32 operations."""
    points, target = np.asarray(points, np.float32), np.asarray(target, np.float32)
    _, _, r2 = radius_scalars(max_dist)
    with np.errstate(all="ignore"):
        d = points[:, None, :] - target[None]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.where(d2 <= r2, d2, np.float32(np.inf)).min(axis=1).astype(np.float32)


# ---- the meshes the tests share ----------------------------------------------------------------------------------------
UNIT = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int64))
# one query in each of the triangle's seven regions: (query, dist2, point), all exactly representable
SEVEN_REGIONS = [
    ((0.25, 0.25, 0.5), 0.25, (0.25, 0.25, 0.0)),     # over the inside
    ((-1.0, -1.0, 0.0), 2.0, (0.0, 0.0, 0.0)),        # vertex a
    ((2.0, -0.5, 0.0), 1.25, (1.0, 0.0, 0.0)),        # vertex b
    ((-0.5, 2.0, 0.0), 1.25, (0.0, 1.0, 0.0)),        # vertex c
    ((0.5, -1.0, 0.0), 1.0, (0.5, 0.0, 0.0)),         # side (a,b)
    ((1.0, 1.0, 0.0), 0.5, (0.5, 0.5, 0.0)),          # side (b,c)
    ((-1.0, 0.5, 0.0), 1.0, (0.0, 0.5, 0.0)),         # side (c,a)
]


def six_triangles():
    """Six right triangles of areas 1, 2, 4, 8, 0 (collinear) and 3, far enough apart to tell their samples apart."""
    legs = [(1, 2), (2, 2), (2, 4), (4, 4), None, (2, 3)]
    vertices, faces = [], []
    for k, leg in enumerate(legs):
        o = np.array([10.0 * k, 0, 0])
        if leg is None:
            tri = [o, o + [1, 0, 0], o + [2, 0, 0]]
        else:
            tri = [o, o + [leg[0], 0, 0], o + [0, leg[1], 0]]
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
        vertices += tri
    return np.array(vertices, np.float32), np.array(faces, np.int64)


def equal_faces(f):
    """f copies of one triangle in a strip: every prefix boundary decides a face."""
    k = np.arange(f, dtype=np.float32)
    vertices = np.stack([np.stack([k, 0 * k, 0 * k], 1), np.stack([k + 1, 0 * k, 0 * k], 1),
                         np.stack([k, 0 * k + 1, 0 * k], 1)], 1).reshape(-1, 3)
    return vertices.astype(np.float32), np.arange(3 * f, dtype=np.int64).reshape(f, 3)


def height_field(side=13, seed=5, jitter=0.3):
    """A jittered side x side-vertex height field with unit spacing: 2 (side-1)^2 faces."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:side, 0:side].astype(np.float64)
    v = np.stack([x, y, np.zeros_like(x)], -1).reshape(-1, 3) + jitter * rng.uniform(-1, 1, (side * side, 3))
    idx = np.arange(side * side).reshape(side, side)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])
    return v.astype(np.float32), faces.astype(np.int64)


def small_faces(f, seed=11, extent=24.0, size=0.4):
    """f small random triangles scattered in a cube of side `extent`."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0, extent, (f, 1, 3))
    vertices = (centre + rng.uniform(-size, size, (f, 3, 3))).reshape(-1, 3)
    return vertices.astype(np.float32), np.arange(3 * f, dtype=np.int64).reshape(f, 3)


def queries_near(vertices, n, seed=3, spread=1.0):
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, np.float32)
    v = v[np.isfinite(v).all(axis=1)]
    pick = v[rng.integers(0, len(v), n)]
    return (pick + spread * rng.uniform(-1, 1, (n, 3))).astype(np.float32)


def permutation(n, seed=17):
    return np.random.default_rng(seed).permutation(n)


# ---- the cases of the GPU tests (made here so that the CPU tests can hold them to what they claim) ---------------------
def cellwise_faces(f, side=None):
    """f tiny triangles, each strictly inside a cell of its own of the unit grid: exactly f (cell, face) pairs."""
    side = side or int(np.ceil(f ** (1 / 3)))
    k = np.arange(f)
    centre = np.stack([k % side, (k // side) % side, k // (side * side)], 1).astype(np.float64) + 0.5
    tri = centre[:, None, :] + np.array([[0, 0, 0], [0.25, 0, 0.125], [0, 0.25, -0.125]])[None]
    return tri.reshape(-1, 3).astype(np.float32), np.arange(3 * f, dtype=np.int64).reshape(f, 3)


def _field_case(max_dist, n=1000, permuted=False, shift=None):
    v, f = height_field()
    q = queries_near(v, n, spread=1.5)
    if permuted:
        f = f[permutation(len(f))]
    if shift is not None:
        v, q = v + np.float32(shift), q + np.float32(shift)
    return dict(points=q, vertices=v, faces=f, max_dist=max_dist)


def nearest_case(name):
    """dict(points, vertices, faces, max_dist) of the named case; made afresh on every call."""
    f32, i64 = np.float32, np.int64
    if name == "seven_regions":
        return dict(points=np.array([q for q, _, _ in SEVEN_REGIONS], f32), vertices=UNIT[0], faces=UNIT[1], max_dist=2.0)
    if name == "at_reach":                            # d2 == r2 is within; one ulp beyond is not
        q = np.array([[0.25, 0.25, 0.5], [0.25, 0.25, np.nextafter(f32(0.5), f32(1))], [0.25, 0.25, -0.5]], f32)
        return dict(points=q, vertices=UNIT[0], faces=UNIT[1], max_dist=0.5)
    if name in ("shared_side", "shared_side_swapped"):
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0]], f32)
        f = np.array([[0, 1, 2], [0, 3, 1]], i64)
        q = np.array([[0.5, 0, 0.25], [0.25, 0, -0.5], [0.5, 0.25, 0.25], [0.5, -0.25, 0.25]], f32)
        return dict(points=q, vertices=v, faces=f[::-1].copy() if name.endswith("swapped") else f, max_dist=1.0)
    if name == "point_faces":
        rng = np.random.default_rng(21)
        v = rng.uniform(-3, 3, (300, 3)).astype(f32)
        v[7] = [np.nan, 0, 0]
        q = rng.uniform(-3, 3, (500, 3)).astype(f32)
        return dict(points=q, vertices=v, faces=np.repeat(np.arange(300)[:, None], 3, axis=1).astype(i64), max_dist=0.6)
    if name == "collinear":
        v = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [0.5, 0.5, 0.5], [1.5, 1.5, 1.5], [2.5, 2.5, 2.5]], f32)
        q = np.array([[1.5, 1, 0], [-1, 0, 0], [3, 0, 0.5], [1, 1, 1], [2, 2, 2.5], [0, 0, 0]], f32)
        return dict(points=q, vertices=v, faces=np.array([[0, 1, 2], [3, 5, 4], [2, 2, 0]], i64), max_dist=1.5)
    if name == "invalid_mixed":
        c = _field_case(1.0, 300)
        v, f = c["vertices"].copy(), c["faces"].copy()
        v[40] = [np.nan, 1, 1]
        v[90, 2] = np.inf
        f[3, 1], f[17, 0], f[100, 2], f[200, 0] = -1, len(v), 2 ** 40, -2 ** 40
        return dict(c, vertices=v, faces=f)
    if name == "span_2x2x2":                          # one face in eight cells, all inside the query's range
        v = np.array([[0.5, 0.5, 0.5], [1.5, 1.5, 0.6], [0.6, 1.4, 1.5]], f32)
        q = np.array([[1.0, 1.0, 1.0], [0.9, 1.1, 0.8], [1.7, 1.7, 0.2], [0.2, 0.2, 0.2]], f32)
        return dict(points=q, vertices=v, faces=np.array([[0, 1, 2]], i64), max_dist=1.0)
    if name in ("box_512", "box_513"):                # 8 x 8 x 8 cells: the last small face; 9 x 57 x 1: the first large
        v = np.array([[0.5, 0.5, 0.5], [7.5, 7.5, 0.5], [0.5, 7.5, 7.5]] if name == "box_512" else
                     [[0.5, 0.5, 0.5], [8.5, 56.5, 0.5], [0.5, 56.5, 0.75]], f32)
        rng = np.random.default_rng(31)
        w = rng.dirichlet([1, 1, 1], 200)
        q = (w @ v.astype(np.float64) + rng.uniform(-1.2, 1.2, (200, 3))).astype(f32)
        return dict(points=q, vertices=v, faces=np.array([[0, 1, 2]], i64), max_dist=1.0)
    if name == "long_face":                           # one face 40 cells long among small ones
        v, f = small_faces(120, extent=12.0)
        v = np.concatenate([v, np.array([[0.2, 0.3, 0.4], [40.2, 0.6, 0.5], [20.0, 0.9, 0.45]], f32)])
        f = np.concatenate([f, np.array([[360, 361, 362]], i64)])
        rng = np.random.default_rng(32)
        along = np.stack([rng.uniform(-1, 42, 200), rng.uniform(-0.5, 1.5, 200), rng.uniform(-0.5, 1.5, 200)], 1)
        return dict(points=np.concatenate([along.astype(f32), queries_near(v[:360], 200)]), vertices=v, faces=f, max_dist=1.0)
    if name == "shifted":
        return _field_case(1.0, 300, shift=(1000, -1000, 1000))
    if name == "far_and_non_finite":
        c = _field_case(1.0, 40)
        v = np.concatenate([c["vertices"], np.array([[-30, -30, 0], [60, -30, 0.5], [0, 60, 0]], f32)])     # and a large face
        f = np.concatenate([c["faces"], np.array([[len(v) - 3, len(v) - 2, len(v) - 1]], i64)])
        far = np.array([[1e30, 0, 0], [3e38, 3e38, -3e38], [-1e25, 5, 5], [5e6, 5, 5], [np.nan, 1, 1], [1, np.inf, 1],
                        [1, 1, -np.inf], [np.nan, np.nan, np.nan], [2.0 ** 21, 3, 3]], f32)
        return dict(c, points=np.concatenate([far, c["points"]]), vertices=v, faces=f)
    if name == "tiny_radius":                         # queries on the vertices, cells of 1e-20
        v = (np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [5, 5, 5], [-4, 2, 7], [9, 9, 9]], np.float64) * 1e-20).astype(f32)
        f = np.array([[0, 1, 2], [3, 3, 3], [2, 4, 0], [5, 5, 5]], i64)
        return dict(points=v.copy(), vertices=v, faces=f, max_dist=1e-20)
    if name.startswith("field_"):                     # field_<max_dist>[_permuted]
        parts = name.split("_")
        return _field_case(float(parts[1]), permuted=len(parts) > 2)
    if name.startswith("queries_"):
        return _field_case(1.0, int(name.split("_")[1]))
    if name.startswith("faces_"):                     # faces_<F>: F pairs exactly
        f = int(name.split("_")[1])
        v, fc = cellwise_faces(f)
        n = 8 if f > 100000 else 200
        return dict(points=queries_near(v, n, spread=0.6), vertices=v, faces=fc, max_dist=1.0)
    raise KeyError(name)


# workgroups of 256 faces; the table's 1024-slot workgroups change in number at 512 and 1024 pairs; geom_scan_kernel's
# runs grow from one to two of those workgroups above 2^19 pairs
FACE_COUNTS = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2 ** 19 + 1)
NEAREST_CASES = ["seven_regions", "at_reach", "shared_side", "shared_side_swapped", "point_faces", "collinear",
                 "invalid_mixed", "span_2x2x2", "box_512", "box_513", "long_face", "shifted", "far_and_non_finite",
                 "tiny_radius", "field_0.5", "field_1", "field_3", "field_0.5_permuted", "field_1_permuted",
                 "field_3_permuted"] + ["queries_%d" % n for n in (1, 63, 64, 65, 257, 300)] + ["faces_%d" % f for f in FACE_COUNTS]
NEAREST_OUTPUTS = ("dist2", "face", "point", "weights", "within")
_nearest_cache = {}


def nearest_case_reference(name):
    """Made once per case, never modified."""
    if name not in _nearest_cache:
        c = nearest_case(name)
        ref = nearest_reference(c["points"], c["vertices"], c["faces"], c["max_dist"], chunk=1 << 20)
        ref["counts"] = count_reference(c["vertices"], c["faces"], c["max_dist"])
        _nearest_cache[name] = ref
    return _nearest_cache[name]


ZERO_NORMAL_FACE, NAN_NORMAL_FACE = 2, 52               # two faces that field_1000 draws often


def sample_case(name):
    """dict(vertices, faces, n, seed, normals, colors) of the named case."""
    f32 = np.float32
    if name.startswith("field_"):                     # field_<n>: normals and colours too
        v, f = height_field()
        rng = np.random.default_rng(41)
        normals = rng.standard_normal(v.shape).astype(f32)
        normals[f[ZERO_NORMAL_FACE]] = 0                   # a face whose three normals are zero: a zero sum
        normals[f[NAN_NORMAL_FACE, 0]] = [np.nan, 0, 0]    # and one with a NaN among them
        return dict(vertices=v, faces=f, n=int(name.split("_")[1]), seed=12345, normals=normals,
                    colors=rng.integers(0, 256, v.shape, dtype=np.uint8))
    if name == "six_triangles":
        v, f = six_triangles()
        return dict(vertices=v, faces=f, n=4096, seed=0, normals=None, colors=None)
    if name.startswith("equal_"):                     # equal_<F>
        v, f = equal_faces(int(name.split("_")[1]))
        return dict(vertices=v, faces=f, n=1000, seed=2, normals=None, colors=None)
    if name == "tiny_face":                           # rows 0 and 2 at 2^-32 of the largest: weight 0
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2.0 ** 16, 0, 0], [0, 2.0 ** 16, 0], [0, 2, 0]], f32)
        return dict(vertices=v, faces=np.array([[0, 1, 2], [0, 3, 4], [0, 2, 1], [0, 1, 5]], np.int64), n=1000, seed=5,
                    normals=None, colors=None)
    if name == "no_area":
        v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [np.nan, 0, 0], [0, 1, 0]], f32)
        return dict(vertices=v, faces=np.array([[0, 1, 2], [0, 0, 0], [0, 4, 3], [0, 1, 9], [-1, 1, 4]], np.int64), n=70,
                    seed=1, normals=np.ones_like(v), colors=np.full(v.shape, 200, np.uint8))
    if name == "invalid_mixed":
        v, f = height_field(9)
        v, f = v.copy(), f.copy()
        v[20] = [np.nan, 0, 0]
        v[33, 1] = -np.inf
        f[0, 0], f[1, 2], f[50, 1], f[-1, 0], f[64, 2] = -1, len(v), 2 ** 40, -2 ** 40, 2 ** 31
        return dict(vertices=v, faces=f, n=1000, seed=9, normals=None, colors=np.arange(v.size, dtype=np.uint8).reshape(v.shape))
    raise KeyError(name)


# workgroups of 256 faces (1025 faces: 5, 2049: 9); the 64-bit scan's runs grow from one to two sums above 2^18 faces
SAMPLE_CASES = ["field_1", "field_64", "field_65", "field_1000", "six_triangles", "equal_255", "equal_256", "equal_257",
                "equal_1025", "equal_2049", "equal_%d" % (2 ** 18 + 1), "tiny_face", "no_area", "invalid_mixed"]
SAMPLE_OUTPUTS = ("points", "face", "weights", "normals", "colors")
_sample_cache = {}


def sample_case_reference(name):
    if name not in _sample_cache:
        c = sample_case(name)
        _sample_cache[name] = sample_reference(c["vertices"], c["faces"], c["n"], c["seed"], c["normals"], c["colors"])
    return _sample_cache[name]
