"""numpy restatement of the mesh edges, the smoothing and the normals (DESIGN.md section 29;
multi_view_stereonet_amd/mesh.py: mesh_edges, mesh_smooth, mesh_normals), and the table of named cases.

Every sum is an integer sum (np.add.at on int64); every fp64 step is one numpy operation in the order
csrc/mvsn_mesh_edges.hip and csrc/mvsn_mesh_smooth.hip state it, so every output is compared byte for byte and no
tolerance applies."""
import functools

import numpy as np

EDGE_OUTPUTS = ("edges", "first", "face_count", "winding", "face_edge", "vertex_degree", "vertex_boundary")
NORMAL_OUTPUTS = ("face_normals", "face_area", "vertex_normals")
METHODS = {"laplacian": 0, "taubin": 1}
CLAMP = 2.0 ** 31
LAM, MU = 0.5, -0.53                 # mesh_smooth's defaults


# ---- edges ---------------------------------------------------------------------------------------------------------

def edges_reference(faces, m):
    """The outputs of mesh_edges as numpy arrays."""
    Fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = Fc.shape[0]
    ok = ((Fc >= 0) & (Fc < m)).all(axis=1)
    a, b = Fc.reshape(-1), Fc[:, [1, 2, 0]].reshape(-1)              # side 3 r + s runs a -> b
    sides = np.nonzero(np.repeat(ok, 3) & (a != b))[0]               # ascending side indices
    lo, hi = np.minimum(a[sides], b[sides]), np.maximum(a[sides], b[sides])
    key, where, inverse, count = np.unique((lo << 32) | hi, return_index=True, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(where, kind="stable")                         # the edges by their first side
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    row = rank[inverse]                                              # the edge row of every taking side
    e = key.size
    out = {"edges": np.stack([key[order] >> 32, key[order] & 0xffffffff], axis=1).astype(np.int64).reshape(e, 2),
           "first": sides[where[order]].astype(np.int64), "face_count": count[order].astype(np.int32)}
    winding = np.zeros(e, np.int64)
    np.add.at(winding, row, np.where(a[sides] < b[sides], 1, -1))
    out["winding"] = winding.astype(np.int32)
    face_edge = np.full(3 * f, -1, np.int64)
    face_edge[sides] = row
    out["face_edge"] = face_edge.reshape(f, 3)
    degree = np.zeros(m, np.int64)
    np.add.at(degree, out["edges"].reshape(-1), 1)
    out["vertex_degree"] = degree.astype(np.int32)
    boundary = np.zeros(m, bool)
    boundary[out["edges"][out["face_count"] == 1].reshape(-1)] = True
    out["vertex_boundary"] = boundary
    return out


# ---- smoothing -----------------------------------------------------------------------------------------------------

def smooth_step_size(V):
    """(k, step, scale) with span = m 2^k, m in [0.5, 1), step = 2^(k-30), scale = 2^(30-k); None where nothing moves."""
    V = np.asarray(V, dtype=np.float32).reshape(-1, 3)
    finite = np.isfinite(V).all(axis=1)
    if not finite.any():
        return None
    span = (V[finite].max(axis=0).astype(np.float64) - V[finite].min(axis=0).astype(np.float64)).max()
    if not span > 0.0:
        return None
    _, k = np.frexp(span)
    return int(k), np.ldexp(1.0, int(k) - 30), np.ldexp(1.0, 30 - int(k))


def smooth_factors(iterations, method, lam=LAM, mu=MU):
    return [np.float64(lam)] * iterations if method == "laplacian" else [np.float64(lam), np.float64(mu)] * iterations


def smooth_reference(V, edges, iterations, method="taubin", lam=LAM, mu=MU, held=None):
    """(M,3) float32: mvsn_mesh_smooth on vertices V, the (E,2) edges and the (M,) bool mask of held vertices."""
    V = np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3)
    m = V.shape[0]
    E = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    finite = np.isfinite(V).all(axis=1)
    fixed = ~finite | (np.asarray(held, bool) if held is not None else np.zeros(m, bool))
    size = smooth_step_size(V)
    if size is None:
        return V.copy()
    _, step, scale = size
    a, b = E[:, 0], E[:, 1]
    use = (a >= 0) & (a < m) & (b >= 0) & (b < m) & (a != b)
    use[use] &= finite[a[use]] & finite[b[use]]
    a, b = a[use], b[use]
    degree = np.zeros(m, np.int64)
    np.add.at(degree, a, 1)
    np.add.at(degree, b, 1)
    moves = ~fixed & (degree > 0)
    x = V.astype(np.float64)
    with np.errstate(all="ignore"):
        for factor in smooth_factors(iterations, method, lam, mu):
            d = x[b] - x[a]
            q = np.rint(d * scale)
            q = np.where(q < -CLAMP, -CLAMP, q)
            q = np.where(q > CLAMP, CLAMP, q)
            q = np.where(q == q, q, 0.0).astype(np.int64)
            total = np.zeros((m, 3), np.int64)
            np.add.at(total, a, q)
            np.add.at(total, b, -q)
            mean = (total[moves].astype(np.float64) * step) / degree[moves].astype(np.float64)[:, None]
            x[moves] = x[moves] + factor * mean
        out = x.astype(np.float32)
    out[fixed] = V[fixed]
    return out


# ---- normals -------------------------------------------------------------------------------------------------------

def canonical(g):
    """(n,3) triples with the lowest row rotated to the front (the first of equal lowest rows)."""
    g = np.asarray(g, dtype=np.int64).reshape(-1, 3)
    k = np.argmin(g, axis=1)
    rows = np.arange(g.shape[0])
    return np.stack([g[rows, k], g[rows, (k + 1) % 3], g[rows, (k + 2) % 3]], axis=1)


def face_cross(V, faces):
    """(valid (F,) bool, rows (F,3), c (F,3) float64, |c| (F,)) by the kernel's operations."""
    V = np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3)
    Fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    m = V.shape[0]
    ok = ((Fc >= 0) & (Fc < m)).all(axis=1)
    idx = canonical(np.where(ok[:, None], Fc, 0))
    if m == 0:
        return ok, idx, np.zeros((Fc.shape[0], 3)), np.zeros(Fc.shape[0])
    P32 = V[idx]
    ok &= np.isfinite(P32).all(axis=(1, 2))
    P = P32.astype(np.float64)
    with np.errstate(all="ignore"):
        ab, ac = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        cx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        cy = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        cz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
        length = np.sqrt((cx * cx + cy * cy) + cz * cz)
    ok &= (length > 0.0) & (length <= 1.7e308)
    return ok, idx, np.stack([cx, cy, cz], axis=1), length


def normal_sums(V, faces):
    """(M,3) int64: per vertex the integer sum of its valid faces' quantised cross products."""
    m = np.asarray(V).reshape(-1, 3).shape[0]
    ok, idx, c, _ = face_cross(V, faces)
    idx, c = idx[ok], c[ok]
    big = np.abs(c).max(axis=1) if c.shape[0] else np.zeros(0)
    vmax = np.zeros(m, np.int64)                                     # the bits of positive doubles order as integers
    for j in range(3):
        np.maximum.at(vmax, idx[:, j], big.view(np.int64))
    total = np.zeros((m, 3), np.int64)
    for j in range(3):
        e = ((vmax[idx[:, j]] >> 52) & 0x7ff) - 1022
        scale = np.ldexp(1.0, (31 - e).astype(np.int32))
        np.add.at(total, idx[:, j], np.rint(c * scale[:, None]).astype(np.int64))
    return total


def normals_reference(V, faces):
    """The outputs of mesh_normals as numpy arrays."""
    ok, _, c, length = face_cross(V, faces)
    safe = np.where(ok, length, 1.0)
    with np.errstate(all="ignore"):
        face_normals = np.where(ok[:, None], c / safe[:, None], 0.0).astype(np.float32)
        face_area = np.where(ok, length / 2.0, 0.0).astype(np.float32)
        s = normal_sums(V, faces).astype(np.float64)
        norm = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        vertex_normals = np.where((norm > 0.0)[:, None], s / np.where(norm > 0.0, norm, 1.0)[:, None], 0.0).astype(np.float32)
    return {"face_normals": face_normals, "face_area": face_area, "vertex_normals": vertex_normals}


# ---- the cases -----------------------------------------------------------------------------------------------------

def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1, 3)


def fan(n, hub=(0.0, 0.0, 0.3), radius=1.0, seed=0):
    """Vertex 0 is the hub, 1..n the ring; n faces (0, 1 + i, 1 + (i + 1) % n); the ring slightly noisy."""
    t = 2 * np.pi * np.arange(n) / n
    rng = np.random.default_rng(seed)
    ring = np.stack([radius * np.cos(t), radius * np.sin(t), 0.05 * rng.standard_normal(n)], axis=1)
    i = np.arange(n)
    return _f32(np.concatenate([[hub], ring])), _i64(np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1))


def grid(n, noise=0.02, seed=1, offset=0.0):
    """n x n vertices on the unit square with noisy height, 2 (n - 1)^2 faces of one winding (+z)."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(n) / (n - 1), np.arange(n) / (n - 1), indexing="ij")
    V = np.stack([x, y, noise * rng.standard_normal((n, n))], axis=-1).reshape(-1, 3) + offset
    r, c = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    p = (r * n + c).reshape(-1)
    F = np.concatenate([np.stack([p, p + 1, p + n + 1], axis=1), np.stack([p, p + n + 1, p + n], axis=1)])
    return _f32(V), _i64(F)


def icosphere(frequency=6, noise=0.03, seed=2):
    """A closed geodesic sphere of 20 frequency^2 faces wound outwards; (noisy float32 vertices, faces, unit directions)."""
    g = (1 + 5 ** 0.5) / 2
    P = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], np.float64)
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    rows, points, faces = {}, [], []
    nu = frequency

    def row(p):
        key = tuple(np.round(p, 9))
        if key not in rows:
            rows[key] = len(points)
            points.append(p)
        return rows[key]
    for a, b, c in T:
        at = lambda i, j: row((i * P[a] + j * P[b] + (nu - i - j) * P[c]) / nu)   # noqa: E731
        for i in range(nu):
            for j in range(nu - i):
                faces.append((at(i, j), at(i + 1, j), at(i, j + 1)))
                if i + j < nu - 1:
                    faces.append((at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)))
    D = np.array(points)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    F = np.array(faces, np.int64)
    out = np.einsum("ij,ij->i", np.cross(D[F[:, 1]] - D[F[:, 0]], D[F[:, 2]] - D[F[:, 0]]), D[F].sum(axis=1)) < 0
    F[out] = F[out][:, [0, 2, 1]]
    radius = 1.0 + noise * np.random.default_rng(seed).standard_normal(D.shape[0])
    return _f32(D * radius[:, None]), _i64(F), D


TETRA = ([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
QUAD = [[0, 0, 0], [1, 0, 0.1], [0, 1, -0.1], [1, 1, 0.2], [0.5, 0.5, 1.0]]
# (method, iterations); "all" adds the held-vertex and parameter variants of the grid
BRIEF = (("taubin", 5), ("laplacian", 1))
FULL = (("laplacian", 0), ("laplacian", 1), ("laplacian", 5), ("taubin", 0), ("taubin", 1), ("taubin", 5))


def _nonfinite():
    va, fa = fan(7, seed=3)
    vb, fb = fan(6, seed=4)
    vb[:, 0] += np.float32(3.0)
    va[3, 1] = np.nan                                               # a ring vertex of the first fan
    vb[0, 2] = np.inf                                                # the hub of the second
    return np.concatenate([va, vb]), np.concatenate([fa, fb + va.shape[0]])


def _grid_case(**kw):
    V, F = grid(17, **kw)
    return dict(vertices=V, faces=F, smooth=FULL, variants=True)


@functools.lru_cache(maxsize=None)
def _cases():
    sphere_v, sphere_f, _ = icosphere()
    isolated = np.concatenate([_f32(QUAD), _f32([[5, 5, 5], [6, 6, 6], [np.nan, 0, 0]])])
    return {
        "one_triangle": dict(vertices=_f32(QUAD[:3]), faces=_i64([[0, 1, 2]])),
        "two_triangles": dict(vertices=_f32(QUAD[:4]), faces=_i64([[0, 1, 2], [2, 1, 3]])),
        "tetrahedron": dict(vertices=_f32(TETRA[0]), faces=_i64(TETRA[1])),
        "three_on_edge": dict(vertices=_f32(QUAD), faces=_i64([[0, 1, 2], [1, 0, 3], [0, 1, 4]])),
        "same_face_twice": dict(vertices=_f32(QUAD[:4]), faces=_i64([[0, 1, 2], [2, 1, 3], [1, 2, 0]])),
        "opposite_winding": dict(vertices=_f32(QUAD[:4]), faces=_i64([[0, 1, 2], [0, 2, 1], [2, 1, 3]])),
        "repeated_vertex": dict(vertices=_f32(QUAD[:4]), faces=_i64([[0, 1, 1], [0, 1, 2], [3, 3, 3], [2, 1, 3]])),
        "out_of_range": dict(vertices=_f32(QUAD[:4]), faces=_i64([[0, 1, -1], [1, 2, 4], [0, 1, 2], [2 ** 40, 1, 3]])),
        "no_faces": dict(vertices=_f32(QUAD[:3]), faces=_i64([])),
        "isolated_vertices": dict(vertices=isolated, faces=_i64([[0, 1, 2], [2, 1, 3]])),
        "nonfinite_in_fans": dict(zip(("vertices", "faces"), _nonfinite())),
        "coincident": dict(vertices=_f32([[0.25, -3.0, 7.0]] * 4), faces=_i64([[0, 1, 2], [2, 1, 3]])),
        "fan_300": dict(zip(("vertices", "faces"), fan(300, seed=5))),
        "fan_256_m257": dict(zip(("vertices", "faces"), fan(256, seed=6))),
        "grid_17": _grid_case(),
        "grid_17_offset_1e3": dict(zip(("vertices", "faces"), grid(17, offset=1e3))),
        "icosphere": dict(vertices=sphere_v, faces=sphere_f),
    }


SMOOTH_CASES = tuple(_cases())


def smooth_case(name):
    """{vertices, faces, configs}: configs is a tuple of (label, kwargs of smooth_case_reference's smoothing)."""
    c = dict(_cases()[name])
    m = c["vertices"].shape[0]
    configs = [("%s_%d" % (method, n), dict(method=method, iterations=n)) for method, n in c.pop("smooth", BRIEF)]
    if c.pop("variants", False):
        pinned = np.zeros(m, bool)
        pinned[[0, 40, 144, 145, 288]] = True
        configs += [("fix_boundary", dict(method="taubin", iterations=5, fix_boundary=True)),
                    ("pinned", dict(method="taubin", iterations=5, pinned=pinned)),
                    ("both_held", dict(method="laplacian", iterations=5, fix_boundary=True, pinned=pinned)),
                    ("strong", dict(method="taubin", iterations=5, lam=1.0, mu=-2.0)),
                    ("mild", dict(method="laplacian", iterations=5, lam=0.125))]
    c["configs"] = tuple(configs)
    return c


def held_mask(m, boundary, fix_boundary=False, pinned=None):
    held = np.zeros(m, bool) if pinned is None else np.asarray(pinned, bool).copy()
    return held | boundary if fix_boundary else held


def mesh_smooth_reference(V, faces, iterations, method="taubin", lam=LAM, mu=MU, fix_boundary=False, pinned=None):
    """mesh_smooth's vertices: the edges, the held mask and the smoothing."""
    V = _f32(V)
    edges = edges_reference(faces, V.shape[0])
    return smooth_reference(V, edges["edges"], iterations, method, lam, mu,
                            held_mask(V.shape[0], edges["vertex_boundary"], fix_boundary, pinned))


@functools.lru_cache(maxsize=None)
def smooth_case_reference(name):
    """{edges: {...}, normals: {...}, smooth: {label: vertices}}; made once per case, never modified."""
    c = smooth_case(name)
    V, F = c["vertices"], c["faces"]
    return {"edges": edges_reference(F, V.shape[0]), "normals": normals_reference(V, F),
            "smooth": {label: mesh_smooth_reference(V, F, **kw) for label, kw in c["configs"]}}
