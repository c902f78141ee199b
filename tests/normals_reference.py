"""numpy restatement of the normals from depth maps and of the voxel mean direction (DESIGN.md section 13;
multi_view_stereonet_amd/fusion.py: depth_normals, voxel_normals).

Which neighbours count is decided with the kernel's own fp32 operations (a subtract, a multiply, a comparison, and the
test that the difference is finite: numpy rounds each once, as the device does), so the defined mask and the choice
between the central and the one-sided difference are the device's exactly.  Everything else is float64: K^-1, the rays,
the tangents, the cross product, the rotation, the normalisation.  The device does those in fp32, so each pixel comes
with a bound on the angle between the two, derived from the roundings of the fp32 evaluation (EPS = 2^-24, the unit
roundoff):

    bound = EPS * (8 |X| (|t_u| + |t_v|) + 3 |t_u| |t_v|) / |t_v x t_u| + 8 EPS

each back-projected X carries at most 4 relative roundings (the rounded K^-1, two fused multiply-adds, the product with
the depth) and each tangent is the difference of two such X: the first term; the cross product's own roundings: the
second; the rotation (three roundings per component) and the normalisation: the last.

The voxel restatement forms q exactly as specified, in fp32, sums in int64 and finalises in float64."""
import numpy as np

EPS = 2.0 ** -24
QUANT = np.float32(2.0 ** 20)
SHIFTS = ((0, -1), (0, 1), (-1, 0), (1, 0))          # (dy, dx) of the left, right, upper and lower neighbour


def _shifted(a, dy, dx, fill):
    """a[..., y + dy, x + dx, ...] on the (V,H,W,...) array `a`, `fill` where that lies outside the image."""
    out = np.full_like(a, fill)
    H, W = a.shape[1:3]
    ys = slice(max(0, -dy), H - max(0, dy))
    xs = slice(max(0, -dx), W - max(0, dx))
    yd = slice(max(0, dy), H - max(0, -dy))
    xd = slice(max(0, dx), W - max(0, -dx))
    out[:, ys, xs] = a[:, yd, xd]
    return out


def usable_neighbours(depth, valid, max_rel_step):
    """(ok (V,H,W) bool, flags (4,V,H,W) bool in SHIFTS order) of fp32 `depth` (V,H,W): the pixel is usable; the
    neighbour counts.  fp32 throughout: diff = d' - d, bound = step * d, |diff| <= bound and diff finite."""
    d = np.ascontiguousarray(depth, dtype=np.float32)
    step = np.float32(max_rel_step)
    with np.errstate(all="ignore"):
        ok = d > 0
        if valid is not None:
            ok = ok & (np.asarray(valid).reshape(d.shape) != 0)
        bound = step * d
        flags = []
        for dy, dx in SHIFTS:
            dn = _shifted(d, dy, dx, np.float32(0))
            okn = _shifted(ok, dy, dx, False)
            diff = dn - d
            assert diff.dtype == bound.dtype == np.float32
            flags.append(ok & okn & (np.abs(diff) <= bound) & np.isfinite(diff))
    return ok, np.stack(flags)


def normals_reference(depth, K, valid=None, T_cam_in_world=None, max_rel_step=0.05):
    """dict of normals (V,3,H,W) f64 (zeros where undefined), defined (V,H,W) bool, usable (4,V,H,W) bool (left, right,
    up, down), bound (V,H,W) f64 radians (inf where undefined) and X (V,H,W,3) f64 camera-frame points, for depth
    (V,H,W) or (V,1,H,W) fp32, K (V,4,4) and optional valid (like depth) and T_cam_in_world (V,4,4)."""
    d32 = np.ascontiguousarray(np.asarray(depth), dtype=np.float32)
    if d32.ndim == 4:
        d32 = d32[:, 0]
    V, H, W = d32.shape
    ok, flags = usable_neighbours(d32, None if valid is None else np.asarray(valid).reshape(V, H, W), max_rel_step)
    left, right, up, down = flags
    Kd = np.asarray(K, dtype=np.float64)[:, :3, :3]
    Ki = np.linalg.inv(Kd)
    ys, xs = np.mgrid[0:H, 0:W]
    pix = np.stack([xs, ys, np.ones_like(xs)], -1).astype(np.float64)               # (H,W,3)
    ray = np.einsum("vij,hwj->vhwi", Ki, pix)
    with np.errstate(all="ignore"):
        X = d32.astype(np.float64)[..., None] * ray
        Xs = [_shifted(X, dy, dx, 0.0) for dy, dx in SHIFTS]
        tu = np.where(right[..., None], Xs[1], X) - np.where(left[..., None], Xs[0], X)
        tv = np.where(down[..., None], Xs[3], X) - np.where(up[..., None], Xs[2], X)
        c = np.cross(tv, tu)
        cross_len = np.linalg.norm(c, axis=-1)
        if T_cam_in_world is not None:
            R = np.asarray(T_cam_in_world, dtype=np.float64)[:, :3, :3]
            c = np.einsum("vij,vhwj->vhwi", R, c)
        length = np.linalg.norm(c, axis=-1)
        defined = ok & (left | right) & (up | down) & np.isfinite(length) & (length > 0) & np.isfinite(c).all(-1)
        n = np.where(defined[..., None], c / np.where(defined, length, 1.0)[..., None], 0.0)
        a, b = np.linalg.norm(tu, axis=-1), np.linalg.norm(tv, axis=-1)
        bound = EPS * (8.0 * np.linalg.norm(X, axis=-1) * (a + b) + 3.0 * a * b) / np.where(defined, cross_len, 1.0) \
            + 8.0 * EPS
    return {"normals": np.ascontiguousarray(n.transpose(0, 3, 1, 2)), "defined": defined, "usable": flags,
            "bound": np.where(defined, bound, np.inf), "X": X}


def angle(a, b):
    """Angle in radians between the unit vectors a and b (..., 3), float64: atan2(|a x b|, a . b)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))


def quantise(normals):
    """(counts (N,) bool, q (N,3) int64) of fp32 `normals` (N,3): clamp to [-1,1], times 2^20 (exact), rint (half to
    even); a point counts when every component is finite and q != (0,0,0)."""
    n = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    finite = np.isfinite(n).all(axis=1)
    with np.errstate(all="ignore"):
        scaled = np.clip(np.where(finite[:, None], n, np.float32(0)), np.float32(-1), np.float32(1)) * QUANT
    assert scaled.dtype == np.float32
    q = np.rint(scaled).astype(np.int64)
    return finite & (q != 0).any(axis=1), q


def voxel_normals_reference(normals, inverse, m):
    """(out (m,3) f32, sums (m,3) int64): per row of `inverse` the direction of the integer sum of the q of its points."""
    counts, q = quantise(normals)
    inverse = np.asarray(inverse, dtype=np.int64).reshape(-1)
    counts = counts & (inverse >= 0) & (inverse < m)
    S = np.zeros((m, 3), np.int64)
    np.add.at(S, inverse[counts], q[counts])
    s = S.astype(np.float64)
    length = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
    zero = (S == 0).all(axis=1)
    out = np.where(zero[:, None], 0.0, s / np.where(zero, 1.0, length)[:, None]).astype(np.float32)
    return out, S
