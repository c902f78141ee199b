"""numpy restatement, and the definition, of an oriented cloud added to the TSDF volume
(multi_view_stereonet_amd/tsdf.py: integrate_cloud, csrc/mvsn_tsdf_cloud.hip).

The brute force over every (voxel, row) pair in chunks, one numpy operation per stated fp32 step (numpy rounds each
once, as the device does), plain int64 sums and the fp64 update rounded once: the state is the device's byte for byte
and no margin is needed.  No grid and no brick is used to find the pairs; the grid appears only where the contract
names it: a finite point outside its range raises (cloud_reference.target_cells)."""
import functools

import numpy as np

from cloud_reference import CHUNK_ELEMENTS, radius_scalars, squared_distances, target_cells
from tsdf_reference import CASES, SPHERE, tsdf_integrate_reference

MAX_WEIGHT = np.float32(256.0)
MAX_ROWS = 2 ** 19 - 1                # accepted rows of one voxel; above, the voxel is left unchanged
A_QUANTUM, T_QUANTUM = np.float32(2.0 ** 16), np.float32(2.0 ** 20)


def centres_f32(dims, voxel_size, origin):
    """The centres x = origin + float32(i) * voxel_size, a multiply and then an add: (x (Nx), y (Ny), z (Nz)) fp32."""
    vs, o = np.float32(voxel_size), np.asarray(origin, np.float32)
    out = [o[a] + np.arange(dims[a]).astype(np.float32) * vs for a in range(3)]
    assert all(c.dtype == np.float32 for c in out)
    return out


def rows_taking_part(points, normals, weights):
    """(N,) bool: the point is finite, the normal is finite and not (0,0,0), the weight is finite and in (0, 256]."""
    p, n = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    ok = np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)
    if weights is not None:
        w = np.asarray(weights, np.float32)
        with np.errstate(invalid="ignore"):
            ok &= (w > 0) & (w <= MAX_WEIGHT)               # a NaN compares false
    return ok


def tsdf_cloud_reference(points, normals, radius, dims, voxel_size, origin, trunc, *, weights=None, colors=None, state=None):
    """points, normals (N,3) fp32, weights (N,) fp32 or None, colors (N,3) uint8 or None, dims (Nx,Ny,Nz); state =
    (sdf_sum, weight, color_sum) fp32 arrays to start from (zeros without; color_sum None without colours).  Returns a
    dict of (Nz,Ny,Nx) arrays: sdf_sum, weight fp32, color_sum (3,Nz,Ny,Nx) fp32 or None: the new state; count, sum_a,
    sum_at int64 (sum_ac (3,...) with colours); updated bool."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    n = p.shape[0]
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    tr = np.float32(trunc)
    _, _, r2 = radius_scalars(radius)
    if state is None:
        s0, w0 = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        c0 = np.zeros((3,) + shape, np.float32) if colors is not None else None
    else:
        s0, w0 = (np.array(a, np.float32) for a in state[:2])
        c0 = np.array(state[2], np.float32) if state[2] is not None else None
    assert (c0 is None) == (colors is None) and s0.shape == w0.shape == shape
    V = nx * ny * nz
    count, sa, sat = np.zeros(V, np.int64), np.zeros(V, np.int64), np.zeros(V, np.int64)
    sac = np.zeros((3, V), np.int64)
    if n:
        target_cells(p, radius)                              # (raises where a finite point has no cell)
        part = rows_taking_part(p, nr, weights)
        w = np.asarray(weights, np.float32) if weights is not None else np.ones(n, np.float32)
        rgb = np.asarray(colors, np.uint8).astype(np.int64) if colors is not None else None
        cx, cy, cz = centres_f32(dims, voxel_size, origin)
        gz, gy, gx = np.meshgrid(cz, cy, cx, indexing="ij")
        x = np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], axis=1)
        chunk = max(1, CHUNK_ELEMENTS // n)
        for a in range(0, V, chunk):
            q = x[a:a + chunk]
            with np.errstate(all="ignore"):
                dx, dy, dz = (q[:, None, k] - p[None, :, k] for k in range(3))
                d2 = (dx * dx + dy * dy) + dz * dz
                ok = (d2 <= r2) & part[None, :]
                u = d2 / r2
                b = np.float32(1.0) - u
                phi = b * b
                A = np.rint((phi * w[None, :]) * A_QUANTUM)
                s = (dx * nr[None, :, 0] + dy * nr[None, :, 1]) + dz * nr[None, :, 2]
                t = np.fmin(np.fmax(s, -tr), tr)             # (C's fmaxf / fminf: a NaN s gives -trunc)
                T = np.rint((t / tr) * T_QUANTUM)
            assert d2.dtype == phi.dtype == A.dtype == s.dtype == T.dtype == np.float32
            assert np.array_equal(d2, squared_distances(q, p), equal_nan=True)
            A = np.where(ok, A, 0).astype(np.int64)
            T = np.where(ok, T, 0).astype(np.int64)
            count[a:a + chunk] = ok.sum(axis=1)
            sa[a:a + chunk] = A.sum(axis=1)
            sat[a:a + chunk] = (A * T).sum(axis=1)
            if rgb is not None:
                for ch in range(3):
                    sac[ch, a:a + chunk] = (A * rgb[None, :, ch]).sum(axis=1)
    count, sa, sat, sac = count.reshape(shape), sa.reshape(shape), sat.reshape(shape), sac.reshape((3,) + shape)
    upd = (sa > 0) & (count <= MAX_ROWS)
    wsum = sa.astype(np.float64) * 2.0 ** -16
    with np.errstate(all="ignore"):
        weight = np.where(upd, (w0.astype(np.float64) + wsum).astype(np.float32), w0)
        sdf = np.where(upd, (s0.astype(np.float64) + sat.astype(np.float64) * (np.float64(tr) * 2.0 ** -36)).astype(np.float32), s0)
        col = None
        if c0 is not None:
            add = (sac.astype(np.float64) * 2.0 ** -16) / 127.5
            col = np.where(upd[None], ((c0.astype(np.float64) + add) - wsum[None]).astype(np.float32), c0)
    # (np.where copies bits: an untouched voxel keeps a NaN's payload)
    weight, sdf = _keep_bits(weight, w0, upd), _keep_bits(sdf, s0, upd)
    if col is not None:
        col = _keep_bits(col, c0, np.broadcast_to(upd[None], col.shape))
    return {"sdf_sum": sdf, "weight": weight, "color_sum": col, "count": count, "sum_a": sa, "sum_at": sat,
            "sum_ac": sac if c0 is not None else None, "updated": upd}


def _keep_bits(new, old, upd):
    out = old.copy().view(np.uint32)
    out[upd] = new.view(np.uint32)[upd]
    return out.view(np.float32)


def state_bytes(r):
    """The three state arrays of a result (or a (sdf_sum, weight, color_sum) tuple) as one bytes object."""
    s, w, c = (r["sdf_sum"], r["weight"], r["color_sum"]) if isinstance(r, dict) else r
    return np.asarray(s, np.float32).tobytes() + np.asarray(w, np.float32).tobytes() + \
        (np.asarray(c, np.float32).tobytes() if c is not None else b"")


# ---- the named cases ------------------------------------------------------------------------------------------------------
def fibonacci_sphere(n, centre, radius):
    """(points (n,3) fp32, outward unit normals (n,3) fp32) of the Fibonacci lattice on a sphere."""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    rho = np.sqrt(1.0 - z * z)
    ang = np.pi * (3.0 - np.sqrt(5.0)) * i
    nrm = np.stack([rho * np.cos(ang), rho * np.sin(ang), z], axis=1)
    return (np.asarray(centre, np.float64) + radius * nrm).astype(np.float32), nrm.astype(np.float32)


SPHERE_RADIUS, SPHERE_TRUNC, SPHERE_POINTS = 0.25, 0.3, 2000
SMALL = dict(dims=(11, 10, 9), voxel_size=0.1, origin=(-0.52, -0.43, -0.41), centre=(0.0, 0.02, -0.01), radius=0.33)
SMALL_RADIUS, SMALL_TRUNC, SMALL_POINTS = 0.2, 0.25, 300
PLANE = dict(dims=(9, 10, 11), voxel_size=0.1, origin=(-0.43, -0.47, -0.52), normal=(0.3, -0.5, 0.8), offset=0.013)
PLANE_RADIUS, PLANE_TRUNC = 0.2, 0.25
PRIOR_CASE = 1                        # of tsdf_reference.CASES


def _case(points, normals, radius, dims, voxel_size, origin, trunc, weights=None, colors=None, state=None):
    return dict(points=np.ascontiguousarray(points, np.float32).reshape(-1, 3),
                normals=np.ascontiguousarray(normals, np.float32).reshape(-1, 3), radius=radius, dims=tuple(dims),
                voxel_size=voxel_size, origin=tuple(origin), trunc=trunc, weights=weights, colors=colors, state=state)


def _small(**kw):
    p, n = fibonacci_sphere(SMALL_POINTS, SMALL["centre"], SMALL["radius"])
    a = dict(points=p, normals=n, radius=SMALL_RADIUS, dims=SMALL["dims"], voxel_size=SMALL["voxel_size"],
             origin=SMALL["origin"], trunc=SMALL_TRUNC)
    a.update(kw)
    return _case(**a)


def plane_cloud():
    """(points, unit normals, weights) of the tilted plane: a jittered lattice that reaches past the volume."""
    nrm = np.asarray(PLANE["normal"], np.float64)
    nrm /= np.linalg.norm(nrm)
    u = np.cross(nrm, [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(nrm, u)
    rng = np.random.default_rng(301)
    g = np.arange(-24, 25) * 0.05
    a, b = (m.reshape(-1) + rng.uniform(-0.02, 0.02, m.size) for m in np.meshgrid(g, g))
    dims, vs, o = PLANE["dims"], PLANE["voxel_size"], np.asarray(PLANE["origin"], np.float64)
    mid = o + 0.5 * vs * (np.asarray(dims) - 1)
    p = mid + PLANE["offset"] * nrm + a[:, None] * u + b[:, None] * v
    return p.astype(np.float32), np.broadcast_to(nrm, p.shape).astype(np.float32), rng.uniform(0.5, 2.0, len(p)).astype(np.float32)


BAD_ROWS = 12


def bad_rows():
    """(points, normals, weights) of rows that take no part, each inside the small volume but for what makes it bad."""
    p = np.tile(np.asarray([[0.1, 0.05, -0.02]], np.float32), (BAD_ROWS, 1))
    n = np.tile(np.asarray([[0.0, 0.6, 0.8]], np.float32), (BAD_ROWS, 1))
    w = np.ones(BAD_ROWS, np.float32)
    p[0, 0], p[1, 1], p[2, 2], p[3, 0] = np.nan, np.inf, -np.inf, np.nan
    p[3, 1] = np.inf
    n[4, 2], n[5] = np.nan, 0.0
    n[6, 0] = np.inf
    w[7], w[8], w[9], w[10], w[11] = 0.0, -1.0, np.nan, 300.0, np.inf
    return p, n, w


@functools.lru_cache(maxsize=None)
def _prior_state():
    from multi_view_stereonet_amd import synthetic
    shape, dims, vs, origin, trunc = CASES[PRIOR_CASE]
    sc = synthetic.fusion_scene(*shape)
    ref = tsdf_integrate_reference(sc["depth"][:, 0].numpy(), sc["K"].numpy(), sc["T_cam_in_world"].numpy(), dims, vs, origin,
                                   trunc, images=sc["images"].numpy())
    return tuple(ref[k].astype(np.float32) for k in ("sdf_sum", "weight", "color_sum"))


def prior_cloud():
    """A patch of points facing the cameras (normals -z) inside the volume of CASES[PRIOR_CASE], with colours."""
    _, dims, vs, origin, _ = CASES[PRIOR_CASE]
    rng = np.random.default_rng(302)
    o = np.asarray(origin, np.float64)
    ext = vs * (np.asarray(dims) - 1)
    p = o + rng.uniform(0.1, 0.9, (400, 3)) * ext
    p[:, 2] = o[2] + 0.5 * ext[2] + 0.1 * np.sin(p[:, 0])
    n = np.tile([0.0, 0.0, -1.0], (len(p), 1))
    return p.astype(np.float32), n.astype(np.float32), rng.integers(0, 256, (len(p), 3)).astype(np.uint8)


CASE_IDS = ("sphere", "plane", "one_1x1x1", "one_3x2x1", "one_8x8x8", "outside", "brick_border", "bad_rows", "duplicates",
            "non_unit", "overflow", "colours", "prior", "offset", "limit", "empty")


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a named case: made once, never modified."""
    if name == "sphere":
        p, n = fibonacci_sphere(SPHERE_POINTS, SPHERE["centre"], SPHERE["radius"])
        return _case(p, n, SPHERE_RADIUS, SPHERE["dims"], SPHERE["voxel_size"], SPHERE["origin"], SPHERE_TRUNC)
    if name == "plane":
        p, n, w = plane_cloud()
        return _case(p, n, PLANE_RADIUS, PLANE["dims"], PLANE["voxel_size"], PLANE["origin"], PLANE_TRUNC, weights=w)
    if name.startswith("one_"):
        dims = tuple(int(d) for d in name[4:].split("x"))
        return _case([[0.11, 0.07, 0.02]], [[0.6, 0.0, 0.8]], 0.3, dims, 0.1, (-0.03, -0.02, -0.01), 0.2)
    if name == "outside":                                    # 0.21 below the first plane of voxels, reach 0.3
        return _case([[0.2, 0.3, -0.21], [5.0, 5.0, 5.0]], [[0.0, 0.0, -1.0], [1.0, 0.0, 0.0]], 0.3, (5, 6, 7), 0.1, (0, 0, 0), 0.2)
    if name == "brick_border":
        # voxel_size 2^-3 and radius 2^-2 are exact: the first point's reach box starts exactly on voxel 8 of x, the first
        # of brick 1, at d2 == r2 (accepted, phi = 0); the second point's ends exactly on voxel 7, the last of brick 0;
        # the third sits at d2 == r2 from voxel (3, 8, 4) along y
        p = [[1.25, 0.5, 0.5], [0.625, 0.625, 0.5], [0.375, 1.25, 0.5]]
        n = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.6, 0.8]]
        return _case(p, n, 0.25, (17, 12, 9), 0.125, (0, 0, 0), 0.25)
    if name == "bad_rows":
        c = _small()
        bp, bn, bw = bad_rows()
        w = np.concatenate([np.linspace(0.25, 256.0, SMALL_POINTS).astype(np.float32), bw])
        order = np.random.default_rng(303).permutation(SMALL_POINTS + BAD_ROWS)
        return _small(points=np.concatenate([c["points"], bp])[order], normals=np.concatenate([c["normals"], bn])[order],
                      weights=w[order])
    if name == "duplicates":
        c = _small()
        rep = np.concatenate([np.arange(SMALL_POINTS), np.arange(0, SMALL_POINTS, 3), np.zeros(40, np.int64)])
        return _small(points=c["points"][rep], normals=c["normals"][rep])
    if name == "non_unit":
        c = _small()
        scale = np.where(np.arange(SMALL_POINTS) % 3 == 0, 50.0, np.where(np.arange(SMALL_POINTS) % 3 == 1, 1e30, 0.01))
        return _small(normals=(c["normals"].astype(np.float64) * scale[:, None]).astype(np.float32))
    if name == "overflow":                                   # dx nx = +inf and dy ny = -inf: s is a NaN, t = -trunc
        return _case([[-1.5, -1.25, 0.0], [0.5, 0.5, 0.25]], [[3e38, -3e38, 0.0], [0.0, 0.0, 1.0]], 2.5, (3, 2, 1), 1.0, (0, 0, 0), 0.5)
    if name == "colours":
        rng = np.random.default_rng(304)
        return _small(weights=rng.uniform(0.1, 3.0, SMALL_POINTS).astype(np.float32),
                      colors=rng.integers(0, 256, (SMALL_POINTS, 3)).astype(np.uint8))
    if name == "prior":
        _, dims, vs, origin, trunc = CASES[PRIOR_CASE]
        p, n, c = prior_cloud()
        return _case(p, n, 0.5, dims, vs, origin, trunc, colors=c, state=_prior_state())
    if name == "offset":
        shift = np.asarray([1000.0, -1000.0, 1000.0])
        c = _small()
        return _small(points=(c["points"].astype(np.float64) + shift).astype(np.float32),
                      origin=tuple(np.asarray(SMALL["origin"]) + shift))
    if name == "limit":
        # voxel 0 has 2^19 - 1 rows within reach and is updated; voxel 1 has 2^19 and keeps its bits
        rng = np.random.default_rng(305)
        k = MAX_ROWS
        p = np.concatenate([rng.uniform(-0.05, 0.05, (k, 3)), rng.uniform(-0.05, 0.05, (k + 1, 3)) + [1.0, 0.0, 0.0]])
        n = np.tile([0.0, 0.0, 1.0], (len(p), 1))
        return _case(p, n, 0.25, (2, 1, 1), 1.0, (0, 0, 0), 0.1)
    if name == "empty":
        s = (np.arange(24, dtype=np.float32).reshape(2, 3, 4), np.ones((2, 3, 4), np.float32), None)
        return _case(np.zeros((0, 3)), np.zeros((0, 3)), 0.3, (4, 3, 2), 0.1, (0, 0, 0), 0.2, state=s)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """Made once per case, never modified."""
    c = case(name)
    return tsdf_cloud_reference(c["points"], c["normals"], c["radius"], c["dims"], c["voxel_size"], c["origin"], c["trunc"],
                                weights=c["weights"], colors=c["colors"], state=c["state"])


def sphere_mesh_bound():
    """How far a vertex of the sphere case's mesh can lie from the sphere: the level set lies outside by at most
    radius^2 / (2 r) (the closed form in test_tsdf_cloud_reference_cpu.py), Surface Nets adds tsdf_reference.sphere_bound."""
    from tsdf_reference import sphere_bound
    return SPHERE_RADIUS ** 2 / (2.0 * SPHERE["radius"]) + sphere_bound(SPHERE["voxel_size"], SPHERE["radius"])
