"""numpy restatement of the mesh simplification (multi_view_stereonet_amd/mesh.py: mesh_simplify),
and the definition of the feature.

The cells are the voxel merge's (voxel_reference.py: the same fp32 operations as the kernels), so the partition into
clusters is the device's exactly.  Every sum is an integer sum; every fp64 step of the quadric is one numpy operation in
the order csrc/mvsn_mesh_simplify.hip states it, so positions are compared byte for byte and no tolerance applies."""
import functools

import numpy as np

import normals_reference as nr
import voxel_reference as vr

LAMBDA = 2.0 ** -10                  # the pull towards the mean, per incidence
QUANT = 2.0 ** 30                    # steps per unit of the quantised quadric terms
CLAMP = 0.5 - 2.0 ** -10             # |x| <= CLAMP on every axis
OUTPUTS = ("vertices", "faces", "normals", "colors", "count", "first", "inverse", "face_rows")
VERTEX_OUTPUTS = ("vertices", "normals", "colors", "count", "first", "inverse")


def cells(points, voxel_size, origin):
    """(in a cell (N,) bool, c (N,3) int64) of float32 points by voxel_cell's arithmetic; never raises."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    inv = np.float32(1) / np.float32(voxel_size)
    o = np.asarray(origin, dtype=np.float64).astype(np.float32)
    with np.errstate(all="ignore"):
        t = (p - o) * inv
        c = np.floor(t)
    ok = np.isfinite(p).all(axis=1) & np.isfinite(t).all(axis=1)
    ok &= ((c >= -vr.CELL_LIMIT) & (c < vr.CELL_LIMIT)).all(axis=1)
    return ok, np.where(ok[:, None], c, 0).astype(np.int64)


def canonical(g):
    """(n,3) triples of distinct rows with the lowest rotated to the front."""
    g = np.asarray(g, dtype=np.int64).reshape(-1, 3)
    k = np.argmin(g, axis=1)
    rows = np.arange(g.shape[0])
    return np.stack([g[rows, k], g[rows, (k + 1) % 3], g[rows, (k + 2) % 3]], axis=1)


def quadric_sums(V, Fc, cid, c, n_clusters, voxel_size, origin):
    """(C,10) int64: per cluster the quantised sums xx xy xz yy yz zz, dx dy dz and the incidence count."""
    M = V.shape[0]
    Q = np.zeros((n_clusters, 10), np.int64)
    if Fc.shape[0] == 0:
        return Q
    ok = ((Fc >= 0) & (Fc < M)).all(axis=1)
    idx = canonical(np.where(ok[:, None], Fc, 0))           # the lowest row first: the normal's bits are the face's
    P32 = V[idx]                                            # (F, corner, axis)
    ok &= np.isfinite(P32).all(axis=(1, 2))
    g = cid[idx]
    ok &= (g >= 0).all(axis=1)
    P = P32.astype(np.float64)
    v64 = np.float64(np.float32(voxel_size))
    o64 = np.asarray(origin, dtype=np.float64).astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        ab, ac = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        cx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        cy = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        cz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
        length = np.sqrt((cx * cx + cy * cy) + cz * cz)
        ok &= (length > 0.0) & (length <= 1.7e308)
        length = np.where(ok, length, 1.0)
        n = [np.where(ok, x, 0.0) / length for x in (cx, cy, cz)]
        qa = np.stack([np.rint((n[i] * n[j]) * QUANT) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
        for j in range(3):
            cj = c[idx[:, j]].astype(np.float64)
            u = [(np.where(ok, P[:, j, a], 0.0) - o64[a]) / v64 - (cj[:, a] + 0.5) for a in range(3)]
            d = -((n[0] * u[0] + n[1] * u[1]) + n[2] * u[2])
            qb = np.stack([np.rint((d * n[a]) * QUANT) for a in range(3)], axis=1)
            rows = g[ok, j]
            np.add.at(Q[:, 0:6], rows, qa[ok].astype(np.int64))
            np.add.at(Q[:, 6:9], rows, qb[ok].astype(np.int64))
            np.add.at(Q[:, 9], rows, 1)
    return Q


def quadric_positions(Q, sq, count, cluster_cells, voxel_size, origin):
    """(C,3) float32: the clamped minimiser of every cluster, mapped back and rounded once."""
    v64 = np.float64(np.float32(voxel_size))
    o64 = np.asarray(origin, dtype=np.float64).astype(np.float32).astype(np.float64)
    nd = count.astype(np.float64)
    ub = [(sq[:, a].astype(np.float64) / nd + 0.5) / 65536.0 - 0.5 for a in range(3)]
    k = Q[:, 9]
    scale = 1.0 / QUANT
    with np.errstate(all="ignore"):
        lk = LAMBDA * k.astype(np.float64)
        w = [Q[:, e].astype(np.float64) * scale for e in range(9)]
        m00, m01, m02, m11, m12, m22 = w[0] + lk, w[1], w[2], w[3] + lk, w[4], w[5] + lk
        r0, r1, r2 = lk * ub[0] - w[6], lk * ub[1] - w[7], lk * ub[2] - w[8]
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        solved = (k > 0) & (det > 0.0) & (det <= 1.7e308)
        x = [((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
             ((c02 * r0 + c12 * r1) + c22 * r2) / det]
        pos = np.empty((Q.shape[0], 3), np.float32)
        for a in range(3):
            xa = np.where(solved, x[a], ub[a])
            xa = np.where(xa == xa, xa, ub[a])
            xa = np.where(xa < -CLAMP, -CLAMP, xa)
            xa = np.where(xa > CLAMP, CLAMP, xa)
            pos[:, a] = (o64[a] + ((cluster_cells[:, a].astype(np.float64) + 0.5) + xa) * v64).astype(np.float32)
    return pos


def simplify_reference(vertices, faces, voxel_size, origin=(0.0, 0.0, 0.0), placement="quadric", normals=None,
                       colors=None, drop_unreferenced=True):
    """dict of OUTPUTS, and: clusters (C), fallbacks, quadric (C,10) int64 or None, cluster_cells (M',3) int64."""
    assert placement in ("mean", "quadric")
    V = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    Fc = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    M = V.shape[0]
    vx = vr.voxel_reference(V, voxel_size, colors, origin)
    cid, first, count, ccells = vx["inverse"], vx["first"], vx["count"], vx["cells"]
    C = first.shape[0]
    pos, Q = vx["points"].copy(), None
    if placement == "quadric" and C:
        kept, c, q = vr.cells_and_fractions(V, voxel_size, origin)
        sq = np.zeros((C, 3), np.int64)
        np.add.at(sq, cid[kept], q[kept])
        Q = quadric_sums(V, Fc, cid, c, C, voxel_size, origin)
        pos = quadric_positions(Q, sq, count, ccells, voxel_size, origin)
    inside, got = cells(pos, voxel_size, origin)
    bad = ~inside | (got != ccells).any(axis=1)
    pos[bad] = V[first[bad]]
    cnormals = nr.voxel_normals_reference(normals, cid, C)[0] if normals is not None else None

    # the faces: remap, classify, the lowest row of every class of canonical triples
    ok = ((Fc >= 0) & (Fc < M)).all(axis=1)
    g = np.where(ok[:, None], cid[np.where(ok[:, None], Fc, 0)], -1) if M else np.full(Fc.shape, -1, np.int64)
    ok &= (g >= 0).all(axis=1) & (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    rows = np.nonzero(ok)[0]
    if rows.size:
        _, lowest = np.unique(canonical(g[rows]), axis=0, return_index=True)   # the first occurrence of each
        rows = np.sort(rows[lowest])
    used = np.ones(C, bool)
    if drop_unreferenced:
        used[:] = False
        used[g[rows].reshape(-1)] = True
    crow = np.where(used, np.cumsum(used) - 1, -1).astype(np.int64)
    inverse = np.where(cid >= 0, crow[np.maximum(cid, 0)], -1).astype(np.int64) if C else np.full(M, -1, np.int64)
    return {"vertices": pos[used], "faces": crow[g[rows]].reshape(-1, 3).astype(np.int64),
            "normals": cnormals[used] if cnormals is not None else None,
            "colors": vx["colors"][used] if colors is not None else None, "count": count[used].astype(np.int32),
            "first": first[used].astype(np.int64), "inverse": inverse, "face_rows": rows.astype(np.int64),
            "clusters": C, "fallbacks": int(bad.sum()), "quadric": Q, "cluster_cells": ccells[used]}


# ---- meshes ------------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def grid_faces(nu, nv):
    """two triangles per quad of an nu x nv lattice of rows i * nv + j"""
    i, j = np.meshgrid(np.arange(nu - 1), np.arange(nv - 1), indexing="ij")
    a = (i * nv + j).reshape(-1)
    return np.concatenate([np.stack([a, a + nv, a + 1], 1), np.stack([a + 1, a + nv, a + nv + 1], 1)]).astype(np.int64)


PLANE_R = rotation((1.0, 2.0, 0.5), 0.6)
PLANE_AT = np.array([0.37, -0.21, 1.13])
PLANE_SPACING = 0.1


def tilted_plane(n=17, spacing=PLANE_SPACING):
    """(vertices, faces, unit normal, a point of the plane) of an n x n lattice in general position"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    local = np.stack([i.reshape(-1) * spacing, j.reshape(-1) * spacing, np.zeros(n * n)], 1)
    return (local @ PLANE_R.T + PLANE_AT).astype(np.float32), grid_faces(n, n), PLANE_R[:, 2].copy(), PLANE_AT.copy()


CREASE_R = rotation((0.0, 1.0, 0.0), 0.35)          # about the crease's own direction: the crease stays along y
CREASE_AT = np.array([0.1237, 0.013, 0.0313])       # a point of the crease: low in the middle of a column of cells
CREASE_VOXEL = 0.25


def crease():
    """(vertices, faces, side (M,) of -1 / 0 / +1) of two planes meeting at 90 degrees along y, 33 x 9 vertices a 16th apart:
    the arm t < 0 lies along local -x, the arm t > 0 along local +z, side 0 is the crease itself"""
    t, y = np.meshgrid(np.arange(-16, 17), np.arange(9), indexing="ij")
    t, y = t.reshape(-1) / 16.0, y.reshape(-1) / 16.0
    local = np.stack([np.minimum(t, 0.0), y, np.maximum(t, 0.0)], 1)
    return (local @ CREASE_R.T + CREASE_AT).astype(np.float32), grid_faces(33, 9), np.sign(t).astype(np.int64)


def cube(n=6, size=1.0):
    """a closed cube of n x n quads per side, welded: (vertices, faces) with outward winding"""
    verts, index, faces = [], {}, []

    def row(p):
        key = tuple(int(round(x)) for x in p)
        if key not in index:
            index[key] = len(verts)
            verts.append([k * size / n for k in key])
        return index[key]
    for axis in range(3):
        for side in (0, n):
            u, w = (axis + 1) % 3, (axis + 2) % 3
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        quad.append(row(p))
                    if side == 0:
                        quad = quad[::-1]
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return np.array(verts, np.float32), np.array(faces, np.int64)


def soup(seed, m=200, f=400, box=4.0):
    rng = np.random.default_rng(seed)
    return (rng.random((m, 3)) * box).astype(np.float32), rng.integers(0, m, (f, 3)).astype(np.int64)


def attributes(m, seed):
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((m, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    if m > 3:
        n[1] = 0.0
        n[2] = (np.nan, 0.0, 1.0)
    return n, rng.integers(0, 256, (m, 3)).astype(np.uint8)


def _case(vertices, faces, voxel_size, origin=(0.0, 0.0, 0.0), drop=True, attrs=False):
    m = len(vertices)
    normals, colors = attributes(m, m) if attrs else (None, None)
    return {"vertices": np.ascontiguousarray(vertices, np.float32).reshape(-1, 3),
            "faces": np.ascontiguousarray(faces, np.int64).reshape(-1, 3), "voxel_size": voxel_size, "origin": origin,
            "drop": drop, "normals": normals, "colors": colors}


def _plane(voxel_size, origin=(0.0, 0.0, 0.0), drop=True, attrs=False):
    v, f, _, _ = tilted_plane()
    return _case(v, f, voxel_size, origin, drop, attrs)


def _duplicates():
    v, f = soup(5, 40, 30)
    f = np.concatenate([f, f[:10], np.roll(f[5:15], 1, axis=1), np.roll(f[8:12], 2, axis=1), f[:12, ::-1],
                        np.roll(f[20:25, ::-1], 1, axis=1)])
    return _case(v, f, 0.5, attrs=True)


def _bad_faces():
    v, f = soup(6, 50, 60)
    m = len(v)
    f[3] = (7, 7, 9)
    f[10] = (4, 5, 4)
    f[11] = (6, 6, 6)
    f[20] = (-1, 2, 3)
    f[21] = (2, m, 3)
    f[22] = (1, 2, m + 5)
    f[30] = (2 ** 40, 2, 3)                 # rows whose low 32 bits are a valid row, or a negative int32: the compare
    f[31] = (1, -2 ** 40, 3)                # has to be on the int64
    f[32] = (1, 2, 2 ** 31)
    f[59] = (0, 1, -7)
    return _case(v, f, 0.7)


def _nonfinite():
    v, f = soup(7, 60, 90)
    v[5, 1] = np.nan
    v[17, 2] = np.inf
    v[40, 0] = -np.inf
    f[0] = (5, 6, 7)
    f[30] = (1, 17, 2)
    return _case(v, f, 0.6, attrs=True)


def _on_boundaries():
    k = np.arange(-4, 5)
    x, y, z = np.meshgrid(k, k[:5], k[3:6], indexing="ij")
    v = (np.stack([x, y, z], -1).reshape(-1, 3) * 0.25).astype(np.float32)       # exact multiples, negative ones included
    rng = np.random.default_rng(8)
    return _case(v, rng.integers(0, len(v), (300, 3)), 0.25)


def _loose_vertices(drop):
    v, f = soup(9, 80, 60)
    return _case(v, f % 40, 0.5, drop=drop, attrs=True)          # rows 40.. are used by no face


def _faces_n(n):
    v, _ = soup(10, 3 * n, 1, box=40.0)
    return _case(v, np.arange(3 * n).reshape(n, 3), 0.01)       # n separate triangles: every one survives


def _clusters_n(n):
    k = np.arange(n)
    base = np.stack([k % 16, (k // 16) % 16, k // 256], 1) + 0.5
    rng = np.random.default_rng(11)
    v = np.concatenate([base + 0.2 * (rng.random((n, 3)) - 0.5), base + 0.2 * (rng.random((n, 3)) - 0.5)])
    f = np.stack([k, (k + 1) % n + n, (k + 2) % n], 1) if n >= 3 else np.zeros((1, 3), np.int64)
    return _case(v, f, 1.0, drop=False)                         # exactly n clusters of two vertices each


def _many_equal():
    """Rows 7..146 are one triangle (70 copies, then 70 of its rotation: one class), so the wave of rows 64..127 holds 64
    equal faces that all want one slot; rows 160..223 are its opposite winding, another class."""
    v, f = soup(12, 30, 20)
    tri = np.array([[3, 11, 19]])
    f = np.concatenate([f[:7], np.repeat(tri, 70, 0), np.repeat(np.roll(tri, 1, 1), 70, 0), f[7:], np.repeat(tri[:, ::-1], 64, 0)])
    return _case(v, f, 0.4)


FALLBACK_VOXEL, FALLBACK_ORIGIN = 0.1, (0.3, -0.7, 0.11)


def _fallback():
    """Vertices one fp32 step below cell boundaries thousands of cells out, on a grid whose size and origin are no
    fp32 numbers' friends: for some the position o + (c + fraction) v, exact in fp64, rounds to a float that the grid's
    fp32 arithmetic puts into the neighbouring cell."""
    rng = np.random.default_rng(14)
    k = rng.integers(-30000, 30000, (300, 3))
    p = (np.asarray(FALLBACK_ORIGIN) + k * FALLBACK_VOXEL).astype(np.float32)
    return _case(np.nextafter(p, np.float32(-np.inf)), rng.integers(0, 300, (200, 3)), FALLBACK_VOXEL, FALLBACK_ORIGIN,
                 drop=False)


SIMPLIFY_CASES = {
    "plane_fine": lambda: _plane(0.05, attrs=True),                    # below spacing / sqrt(3): nothing merges
    "plane_3": lambda: _plane(0.3, attrs=True),
    "plane_3_bare": lambda: _plane(0.3),
    "plane_one_cell": lambda: _plane(100.0, origin=(-50.0, -50.0, -50.0)),
    "plane_one_cell_keep": lambda: _plane(100.0, origin=(-50.0, -50.0, -50.0), drop=False, attrs=True),
    "crease": lambda: _case(*crease()[:2], CREASE_VOXEL),
    "cube_origin": lambda: _case(*cube(), 0.4, origin=(0.13, -0.29, 0.071), attrs=True),
    "duplicates": _duplicates,
    "bad_faces": _bad_faces,
    "nonfinite": _nonfinite,
    "on_boundaries": _on_boundaries,
    "loose_vertices": lambda: _loose_vertices(True),
    "loose_vertices_keep": lambda: _loose_vertices(False),
    "no_faces_keep": lambda: _case(soup(13, 70, 1)[0], np.zeros((0, 3), np.int64), 0.8, drop=False, attrs=True),
    "faces_1": lambda: _faces_n(1), "faces_255": lambda: _faces_n(255), "faces_256": lambda: _faces_n(256),
    "faces_257": lambda: _faces_n(257),
    "clusters_1": lambda: _clusters_n(1), "clusters_255": lambda: _clusters_n(255),
    "clusters_256": lambda: _clusters_n(256), "clusters_257": lambda: _clusters_n(257),
    "many_equal": _many_equal,
    "soup_1": lambda: _case(*soup(1), 1.0, attrs=True),
    "soup_2": lambda: _case(*soup(2), 1.0),
    "soup_coarse_1": lambda: _case(*soup(3), 2.0, attrs=True),         # 8 clusters, 112 classes: most faces collide
    "soup_coarse_2": lambda: _case(*soup(4), 2.0),
    "fallback": _fallback,
}
PLACEMENTS = ("mean", "quadric")


@functools.lru_cache(maxsize=None)
def simplify_case(name):
    """The named case: vertices, faces, voxel_size, origin, drop, normals, colors.  Made once, never modified."""
    return SIMPLIFY_CASES[name]()


@functools.lru_cache(maxsize=None)
def simplify_case_reference(name, placement):
    c = simplify_case(name)
    return simplify_reference(c["vertices"], c["faces"], c["voxel_size"], c["origin"], placement, c["normals"],
                              c["colors"], c["drop"])
