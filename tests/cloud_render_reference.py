"""numpy restatement of the cloud render and of the visibility test (csrc/mvsn_cloud_render.hip;
multi_view_stereonet_amd/fusion.py: cloud_render, cloud_visibility, cloud_colorize).

Every fp32 step of the kernels is one fp32 operation here, in the same order, so the outputs are compared byte for byte:
the camera P = K T^-1 in fp64 with the kernel's own operations and one rounding; the three nested fused multiply-adds
of a row (`fmaf` below is a correctly rounded one); the two divisions; floor(u + 0.5).  The render is the brute force over
(point, view, splat pixel) with np.minimum.at on uint64 keys: it shares neither the kernel's clipping of the square nor
its skipped atomics.

The named cases of tests/test_cloud_render_gpu.py are data here (`case(name)`), and
tests/test_cloud_render_reference_cpu.py asserts on the CPU that each of them exercises what its name says."""
import functools

import numpy as np

f32 = np.float32
MAX_RADIUS = 8
MAX_CHANNELS = 16
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
RENDER_OUTPUTS = ("depth", "index", "colors", "normals")
VISIBILITY_OUTPUTS = ("visible", "count", "values")


def fmaf(a, b, c):
    """The fp32 fused multiply-add, correctly rounded.  The product of two fp32 numbers is exact in fp64; the fp64 sum
    with c is rounded to odd (the error of the addition is known exactly: TwoSum), which makes the second rounding, to
    fp32, the only one that counts."""
    a, b, c = (np.atleast_1d(np.asarray(t, f32)).astype(np.float64) for t in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def cameras(K, T):
    """(V,12) fp32: P = K T^-1 as a row-major 3x4, formed in fp64 from the float32 values with the kernel's operations
    (the adjugate inverse of T's top-left 3x3, -R^-1 t summed left to right, K's first two rows times it summed left
    to right, K's bottom row taken to be (0,0,1)) and rounded once."""
    K, T = np.asarray(K, f32).astype(np.float64), np.asarray(T, f32).astype(np.float64)
    out = np.empty((K.shape[0], 12), f32)
    with np.errstate(all="ignore"):
        for v in range(K.shape[0]):
            a, b, c, d, e, f, g, h, i = T[v, :3, :3].reshape(-1)
            A_, B_, C_ = e * i - f * h, -(d * i - f * g), d * h - e * g
            r = 1.0 / (a * A_ + b * B_ + c * C_)
            Ai = [A_ * r, -(b * i - c * h) * r, (b * f - c * e) * r, B_ * r, (a * i - c * g) * r, -(a * f - c * d) * r,
                  C_ * r, -(a * h - b * g) * r, (a * e - b * d) * r]
            Ti = np.empty(12)
            for m in range(3):
                Ti[m * 4:m * 4 + 3] = Ai[m * 3:m * 3 + 3]
                Ti[m * 4 + 3] = -(Ai[m * 3] * T[v, 0, 3] + Ai[m * 3 + 1] * T[v, 1, 3] + Ai[m * 3 + 2] * T[v, 2, 3])
            for n in range(4):
                out[v, n] = (K[v, 0, 0] * Ti[n] + K[v, 0, 1] * Ti[4 + n]) + K[v, 0, 2] * Ti[8 + n]
                out[v, 4 + n] = (K[v, 1, 0] * Ti[n] + K[v, 1, 1] * Ti[4 + n]) + K[v, 1, 2] * Ti[8 + n]
                out[v, 8 + n] = Ti[8 + n]
    return out


def project(Pm, points):
    """(z, fc, fr) fp32 arrays (N,): the depth and the nearest pixel, as floats, of every point in the camera Pm (12,)."""
    x, y, z = (np.ascontiguousarray(points[:, k], f32) for k in range(3))
    with np.errstate(all="ignore"):
        a0 = fmaf(Pm[0], x, fmaf(Pm[1], y, fmaf(Pm[2], z, Pm[3])))
        a1 = fmaf(Pm[4], x, fmaf(Pm[5], y, fmaf(Pm[6], z, Pm[7])))
        zc = fmaf(Pm[8], x, fmaf(Pm[9], y, fmaf(Pm[10], z, Pm[11])))
        u, v = a0 / zc, a1 / zc
        fc, fr = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
    assert zc.dtype == fc.dtype == fr.dtype == f32
    return zc, fc, fr


def takes_part(points, zc, fc, fr, rows, cols, radius, min_depth, max_depth):
    """The rule of section 25, with the pixel compared exactly (fp64 holds every fp32 and every bound; a NaN fails)."""
    with np.errstate(all="ignore"):
        c, r = fc.astype(np.float64), fr.astype(np.float64)
        return (np.isfinite(points).all(axis=1) & np.isfinite(zc) & (zc > f32(min_depth)) & (zc <= f32(max_depth)) &
                (c >= -radius) & (c < cols + radius) & (r >= -radius) & (r < rows + radius))


def render_keys(points, K, T, rows, cols, radius=0, min_depth=0.0, max_depth=np.inf):
    """(V, rows*cols) uint64: per pixel the least (bits of z << 32) | row over every point and every pixel of its
    square, EMPTY where none."""
    points = np.asarray(points, f32).reshape(-1, 3)
    P = cameras(K, T)
    keys = np.full((P.shape[0], rows * cols), EMPTY, np.uint64)
    for v in range(P.shape[0]):
        zc, fc, fr = project(P[v], points)
        at = np.nonzero(takes_part(points, zc, fc, fr, rows, cols, radius, min_depth, max_depth))[0]
        c, r = fc[at].astype(np.int64), fr[at].astype(np.int64)
        key = (zc[at].view(np.uint32).astype(np.uint64) << np.uint64(32)) | at.astype(np.uint64)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                rr, cc = r + dy, c + dx
                m = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
                np.minimum.at(keys[v], rr[m] * cols + cc[m], key[m])
    return keys


def render_reference(points, K, T, rows, cols, radius=0, colors=None, normals=None, min_depth=0.0, max_depth=np.inf):
    """depth (V,rows,cols) fp32, index (V,rows,cols) int64, colors (V,3,rows,cols) uint8 or None, normals
    (V,3,rows,cols) fp32 or None."""
    keys = render_keys(points, K, T, rows, cols, radius, min_depth, max_depth)
    V = keys.shape[0]
    hit = keys != EMPTY
    row = np.where(hit, keys & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)
    out = {"depth": depth.reshape(V, rows, cols), "index": np.where(hit, row, -1).reshape(V, rows, cols),
           "colors": None, "normals": None}
    for name, src, dtype in (("colors", colors, np.uint8), ("normals", normals, f32)):
        if src is not None:
            g = np.where(hit[:, :, None], np.asarray(src, dtype)[row], np.zeros((), dtype))       # (V, P, 3)
            out[name] = np.ascontiguousarray(g.transpose(0, 2, 1)).reshape(V, 3, rows, cols)
    return out


def visibility_reference(points, depth, K, T, rel_tol=0.01, maps=None, min_depth=0.0):
    """visible (N,V) uint8, count (N,) int32, values (N,C) fp32 or None; depth (V,rows,cols), maps (V,C,rows,cols)."""
    points, depth = np.asarray(points, f32).reshape(-1, 3), np.asarray(depth, f32)
    V, rows, cols = depth.shape
    P = cameras(K, T)
    N = len(points)
    visible = np.zeros((N, V), np.uint8)
    C = None if maps is None else np.asarray(maps).shape[1]
    total = np.zeros((N, C or 0), f32)
    with np.errstate(all="ignore"):
        for v in range(V):
            zc, fc, fr = project(P[v], points)
            ok = takes_part(points, zc, fc, fr, rows, cols, 0, min_depth, np.inf)
            c, r = np.where(ok, fc, 0).astype(np.int64), np.where(ok, fr, 0).astype(np.int64)
            D = depth[v][r, c]
            vis = ok & np.isfinite(D) & (D > 0) & (zc <= fmaf(f32(rel_tol), D, D))
            visible[:, v] = vis
            if C:
                sample = np.asarray(maps, f32)[v][:, r, c].T                               # (N, C)
                total = np.where(vis[:, None], total + sample, total).astype(f32)          # plain fp32 additions
        count = visible.sum(axis=1).astype(np.int32)
        values = None
        if C:
            values = np.where(count[:, None] > 0, total / count.astype(f32)[:, None], f32(0)).astype(f32)
    return {"visible": visible, "count": count, "values": values}


def colorize_reference(values, count):
    """(N,3) uint8 of cloud_colorize: rint((c + 1) * 127.5) in fp64, clamped; (0,0,0) where no view sees the point."""
    with np.errstate(all="ignore"):
        q = np.rint((np.asarray(values, f32).astype(np.float64) + 1.0) * 127.5)
        q = np.where(np.isnan(q), 0.0, np.clip(q, 0.0, 255.0))
    return np.where(np.asarray(count)[:, None] > 0, q, 0.0).astype(np.uint8)


# ---- cameras and clouds of the cases -----------------------------------------------------------------------------------
def straight_camera(focal, cx, cy, views=1):
    """K, T (views,4,4) fp32: cameras at the origin looking down +z (T = identity: P = K's top rows exactly, z is the
    point's own z, u = (focal x + cx z) / z)."""
    K = np.tile(np.eye(4, dtype=f32), (views, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = focal
    K[:, 0, 2], K[:, 1, 2] = cx, cy
    return K, np.tile(np.eye(4, dtype=f32), (views, 1, 1))


def at_pixels(K, px, py, z):
    """(N,3) fp32 points of a straight camera that project to (px, py) (fp64 arrays, not necessarily integers) at depth
    z; exact where the numbers are dyadic."""
    px, py, z = (np.asarray(t, np.float64) for t in np.broadcast_arrays(px, py, z))
    f, cx, cy = float(K[0, 0, 0]), float(K[0, 0, 2]), float(K[0, 1, 2])
    return np.stack([(px - cx) * z / f, (py - cy) * z / f, z], -1).astype(f32)


def arc_cameras(views, rows, cols, seed):
    """K, T (views,4,4) fp32 in general position: cameras on an arc about (0,0,4) looking at it, each with a roll, a
    focal length and a principal point of its own."""
    rng = np.random.default_rng(seed)
    K = np.tile(np.eye(4), (views, 1, 1))
    T = np.tile(np.eye(4), (views, 1, 1))
    for v in range(views):
        th, roll = rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3)
        s, c = np.sin(th), np.cos(th)
        Ry = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
        Rz = np.array([[np.cos(roll), -np.sin(roll), 0], [np.sin(roll), np.cos(roll), 0], [0, 0, 1]])
        T[v, :3, :3] = Ry @ Rz
        T[v, :3, 3] = np.array([0, 0, 4.0]) - T[v, :3, 2] * rng.uniform(3.5, 4.5) + rng.uniform(-0.1, 0.1, 3)
        K[v, 0, 0], K[v, 1, 1] = 0.8 * cols * rng.uniform(0.9, 1.1), 0.8 * cols * rng.uniform(0.9, 1.1)
        K[v, 0, 2], K[v, 1, 2] = (cols - 1) / 2 + rng.uniform(-1, 1), (rows - 1) / 2 + rng.uniform(-1, 1)
    return K.astype(f32), T.astype(f32)


def _attributes(n, seed):
    rng = np.random.default_rng(seed)
    normals = rng.standard_normal((n, 3)).astype(f32)
    return rng.integers(0, 256, (n, 3)).astype(np.uint8), normals


def permutation(n, seed=97):
    return np.random.default_rng(seed).permutation(n)


CONTENTION_N = 4099
EDGE_SIZES = [(n, rows, cols, dv) for n in (255, 256, 257) for rows, cols in ((5, 7), (33, 65)) for dv in (-1, 0, 1)]
NONPART_MIN, NONPART_MAX = 1.5, 6.0


def _edge(n, rows, cols, views):
    rng = np.random.default_rng(n * 1000 + cols * 10 + views)
    K, T = arc_cameras(views, rows, cols, seed=n + views)
    # a box about the point the cameras look at, wider than their view: some points miss
    points = (rng.uniform(-1, 1, (n, 3)) * [0.9, 0.9, 0.6] + [0, 0, 4.0]).astype(f32)
    colors, normals = _attributes(n, n)
    return dict(points=points, K=K, T=T, rows=rows, cols=cols, radius=1, colors=colors, normals=normals)


def _contention(order):
    rows, cols = 5, 7
    K, T = straight_camera(64.0, 3.0, 2.0)
    i = np.arange(CONTENTION_N)
    z = {"distinct": 2.0 + permutation(CONTENTION_N, 5) * 2.0 ** -10, "equal": np.full(CONTENTION_N, 2.5),
         "ascending": 2.0 + i * 2.0 ** -10, "descending": 2.0 + i[::-1] * 2.0 ** -10}[order]
    colors, normals = _attributes(CONTENTION_N, 11)
    return dict(points=at_pixels(K, 3.0, 2.0, z), K=K, T=T, rows=rows, cols=cols, radius=0, colors=colors,
                normals=normals)


NONPART_ROWS = {}     # name -> (row, the pixel (r, c) it would land on, takes part)


def _nonpart():
    """One point per pixel of row 1 of a 5 x 16 map, each a special row; rows 3 holds ordinary points behind them."""
    rows, cols = 5, 16
    K, T = straight_camera(64.0, 0.0, 0.0)
    nan, inf = np.nan, np.inf
    special = [
        ("plain", at_pixels(K, 0, 1, 2.0)[None], True),
        ("nan_x", np.array([[nan, 1 / 32, 2.0]]), False), ("nan_z", np.array([[1 / 32, 1 / 32, nan]]), False),
        ("inf_x", np.array([[inf, 1 / 32, 2.0]]), False), ("minus_inf_y", np.array([[3 / 32, -inf, 2.0]]), False),
        ("inf_z", np.array([[4 / 32, 1 / 32, inf]]), False),
        ("behind", at_pixels(K, 5, 1, -2.0)[None], False), ("z_zero", np.array([[0.0, 0.0, 0.0]]), False),
        ("at_min_depth", at_pixels(K, 7, 1, NONPART_MIN)[None], False),
        ("at_max_depth", at_pixels(K, 8, 1, NONPART_MAX)[None], True),
        ("past_max_depth", at_pixels(K, 9, 1, np.nextafter(f32(NONPART_MAX), f32(np.inf)))[None], False),
        ("huge_pixel", np.array([[1e30, 1 / 32, 2.0]]), False),
        ("half_up", at_pixels(K, 10.5, 1, 2.0)[None], True),            # u + 0.5 = 11 exactly: column 11
        ("minus_half", at_pixels(K, -0.5, 2, 2.0)[None], True),         # u + 0.5 = 0 exactly: column 0
        ("below_minus_half", at_pixels(K, -0.5 - 2.0 ** -10, 3, 2.0)[None], False),
        ("last_column_half", at_pixels(K, 15.5, 1, 2.0)[None], False),  # u + 0.5 = 16: column 16 is outside
    ]
    points = np.concatenate([np.asarray(p, np.float64).reshape(1, 3) for _, p, _ in special]).astype(f32)
    for row, (name, _, part) in enumerate(special):
        NONPART_ROWS[name] = (row, part)
    back = at_pixels(K, np.arange(16.0), 4, 3.0)                        # a full row of ordinary points
    points = np.concatenate([points, back]).astype(f32)
    colors, normals = _attributes(len(points), 3)
    return dict(points=points, K=K, T=T, rows=rows, cols=cols, radius=0, colors=colors, normals=normals,
                min_depth=NONPART_MIN, max_depth=NONPART_MAX)


def _radius(radius):
    """33 x 65: points at the four borders and the four corners, points one pixel outside each border, a far point whose
    centre pixel a nearer point's square covers, and 300 random ones, two views."""
    rows, cols = 33, 65
    K, T = straight_camera(64.0, 32.0, 16.0, views=2)
    K[1, 0, 2], K[1, 1, 2] = 30.0, 17.0                                 # the second view sees them shifted
    rng = np.random.default_rng(40)                                     # (the same cloud at every radius)
    px = [0, 64, 20, 40, 0, 64, 0, 64, -1, 65, 30, 31, 10, 11]
    py = [10, 20, 0, 32, 0, 0, 32, 32, 5, 6, -1, 33, 16, 16]
    z = [2.0, 2.25, 2.5, 2.75, 3.0, 3.25, 3.5, 3.75, 2.0, 2.0, 2.0, 2.0, 4.0, 2.0]      # (10,16) far, (11,16) near
    fixed = at_pixels(K, np.array(px, float), np.array(py, float), np.array(z))
    loose = at_pixels(K, rng.uniform(-9, 74, 300), rng.uniform(-9, 42, 300), rng.uniform(2, 5, 300))
    points = np.concatenate([fixed, loose]).astype(f32)
    colors, normals = _attributes(len(points), 7)
    return dict(points=points, K=K, T=T, rows=rows, cols=cols, radius=radius, colors=colors, normals=normals)


RADIUS_OUTSIDE_ROWS = (8, 9, 10, 11)        # the rows of _radius one pixel outside the map
RADIUS_FAR_ROW, RADIUS_NEAR_ROW = 12, 13


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a render case: points, K, T, rows, cols, radius, colors, normals (and min_depth, max_depth)."""
    if name == "one_hit" or name == "one_miss":
        K, T = straight_camera(64.0, 0.0, 0.0)
        x = 0.0 if name == "one_hit" else 5.0
        return dict(points=np.array([[x, 0.0, 2.0]], f32), K=K, T=T, rows=1, cols=1, radius=0,
                    colors=np.array([[7, 8, 9]], np.uint8), normals=np.array([[0.0, 0.6, -0.8]], f32))
    kind, _, rest = name.partition("_")
    if kind == "edge":
        n, rows, cols, dv = (int(t) for t in rest.split("_"))
        return _edge(n, rows, cols, CAMERA_BATCH + dv)
    if kind == "contention":
        return _contention(rest)
    if kind == "nonpart":
        return _nonpart()
    if kind == "radius":
        return _radius(int(rest))
    raise KeyError(name)


CAMERA_BATCH = 32         # mvsn_cloud_render_camera_batch(), asserted where the library is loaded
EDGE_CASES = ["edge_%d_%d_%d_%d" % s for s in EDGE_SIZES]
CONTENTION_CASES = ["contention_" + o for o in ("distinct", "equal", "ascending", "descending")]
RADIUS_CASES = ["radius_%d" % r for r in (0, 1, 2, 8)]
RENDER_CASES = ["one_hit", "one_miss"] + EDGE_CASES + CONTENTION_CASES + ["nonpart"] + RADIUS_CASES


def render_args(c, gathers=True):
    return dict(radius=c["radius"], colors=c["colors"] if gathers else None, normals=c["normals"] if gathers else None,
                min_depth=c.get("min_depth", 0.0), max_depth=c.get("max_depth", np.inf))


@functools.lru_cache(maxsize=None)
def case_reference(name, gathers=True):
    """Made once per case, never modified."""
    c = case(name)
    return render_reference(c["points"], c["K"], c["T"], c["rows"], c["cols"], **render_args(c, gathers))


# ---- visibility cases --------------------------------------------------------------------------------------------------
OCCLUSION_HOLE = (8, 20, 5, 12)      # columns [8, 20) and rows [5, 12) of the near plane are missing


def _occlusion():
    """Two fronto-parallel planes seen by one straight camera, 24 x 32: the near one (z = 2) fills the map but for a
    rectangular hole, the far one (z = 4) is sampled at points a quarter of a pixel off the pixel centres, well inside
    their pixels.  The depth map is the near plane's where it exists and the far plane's in the hole."""
    rows, cols = 24, 32
    K, T = straight_camera(32.0, 15.5, 11.5)
    c0, c1, r0, r1 = OCCLUSION_HOLE
    depth = np.full((1, rows, cols), 2.0, f32)
    depth[0, r0:r1, c0:c1] = 4.0
    ys, xs = np.meshgrid(np.arange(rows) + 0.25, np.arange(cols) - 0.25, indexing="ij")
    far = at_pixels(K, xs.reshape(-1), ys.reshape(-1), 4.0)
    maps = np.random.default_rng(8).standard_normal((1, 3, rows, cols)).astype(f32)
    return dict(points=far, depth=depth, K=K, T=T, rel_tol=0.01, maps=maps, pixel_x=xs.reshape(-1),
                pixel_y=ys.reshape(-1))


def _rel_tol():
    """One pixel per point, D = 3 everywhere; z = fma(rel_tol, D, D) exactly (visible), its next fp32 up (not), its next
    down (visible)."""
    rows, cols = 2, 4
    K, T = straight_camera(64.0, 0.0, 0.0)
    tol = f32(0.0123)
    D = f32(3.0)
    edge = fmaf(tol, D, D)[0]
    z = np.array([edge, np.nextafter(edge, f32(np.inf)), np.nextafter(edge, f32(0)), 2.0], f32)
    points = at_pixels(K, np.arange(4.0), 1, z.astype(np.float64))
    return dict(points=points, depth=np.full((1, rows, cols), D, f32), K=K, T=T, rel_tol=float(tol), maps=None,
                edge=edge)


def _bad_depth():
    """Depth maps holding 0, a negative value, NaN and +inf under points that would otherwise be visible; three views,
    maps with NaN where nothing may read them."""
    rows, cols = 3, 8
    K, T = straight_camera(64.0, 0.0, 0.0, views=3)
    points = at_pixels(K, np.arange(8.0), 1, 2.0)
    depth = np.full((3, rows, cols), 2.0, f32)
    depth[0, 1, :4] = [0.0, -2.0, np.nan, np.inf]
    depth[1, 1, 2:6] = [-0.0, 1.0, 2.0, np.inf]                        # (1.0: the point is behind it)
    depth[2, 1, 7] = np.nan
    maps = np.random.default_rng(9).standard_normal((3, 3, rows, cols)).astype(f32)
    maps[:, :, 0, :] = np.nan
    return dict(points=points, depth=depth, K=K, T=T, rel_tol=0.0, maps=maps)


def _channels(C):
    """257 points in 33 arc cameras, the depth maps an R = 1 render of the cloud itself, maps of C channels."""
    base = case("edge_257_33_65_1")
    ref = case_reference("edge_257_33_65_1", False)
    V = base["K"].shape[0]
    maps = np.random.default_rng(C).standard_normal((V, C, base["rows"], base["cols"])).astype(f32)
    return dict(points=base["points"], depth=ref["depth"], K=base["K"], T=base["T"], rel_tol=0.01, maps=maps)


def _exact(name):
    """The exact property: an R = 0 render's own depth, rel_tol = 0."""
    base = dict(case(name))
    ref = render_reference(base["points"], base["K"], base["T"], base["rows"], base["cols"], radius=0,
                           min_depth=base.get("min_depth", 0.0), max_depth=base.get("max_depth", np.inf))
    return dict(points=base["points"], depth=ref["depth"], K=base["K"], T=base["T"], rel_tol=0.0, maps=None,
                min_depth=base.get("min_depth", 0.0), index=ref["index"])


EXACT_CASES = ["exact:edge_257_33_65_1", "exact:edge_255_5_7_-1", "exact:radius_0", "exact:contention_equal",
               "exact:nonpart"]
VISIBILITY_CASES = EXACT_CASES + ["occlusion", "rel_tol", "bad_depth", "channels_1", "channels_3", "channels_16"]


@functools.lru_cache(maxsize=None)
def visibility_case(name):
    """points, depth (V,rows,cols), K, T, rel_tol, maps (and min_depth)."""
    if name.startswith("exact:"):
        return _exact(name[6:])
    if name.startswith("channels_"):
        return _channels(int(name[9:]))
    return {"occlusion": _occlusion, "rel_tol": _rel_tol, "bad_depth": _bad_depth}[name]()


@functools.lru_cache(maxsize=None)
def visibility_case_reference(name, with_maps=True):
    c = visibility_case(name)
    return visibility_reference(c["points"], c["depth"], c["K"], c["T"], c["rel_tol"], c["maps"] if with_maps else None,
                                c.get("min_depth", 0.0))
