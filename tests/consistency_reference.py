"""float64 restatement of the two-view consistency and depth-metric kernels (csrc/mvsn_consistency.hip: reproject_kernel,
occlusion_kernel, masked_l1_kernel; csrc/mvsn_metrics.hip), the bounds their fp32 evaluation has to keep -- derived from
the kernels' roundings, not measured -- and the scenes and inputs tests/test_consistency_*.py run.

Two kinds of statement:
  * bounded: the projection, the bilinear gather, the per-block partial sums, the means;
  * exact: every term that holds no multiply followed by an add (which the compiler may contract into an fma) is the
    same bits in numpy float32: |sampled - idepth'|, the occlusion predicate and its threshold, the masked-L1 terms,
    every per-pixel term of the depth metrics but the logarithm.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24                       # unit roundoff of fp32 (round to nearest)
EDGE = 16 * 2.0 ** -23               # |n| within this of 1: the out-of-image flag may differ (as test_homography_warp)
UV_RTOL, UV_ATOL = 1e-5, 2e-6        # the projector tolerances of test_two_view_consistency_ops_golden
ID_RTOL, ID_ATOL = 1e-5, 1e-7
RP_THREADS = 256                     # pixels per block of the reprojection / occlusion kernels
PARTIAL_ADDS = 8                     # longest chain of additions in a block's sum: 6 butterfly steps + (r0+r1)+(r2+r3)
MT_BLOCK_PIXELS, MT_BLOCK_CAP = 8192, 64


# ---- the projection ------------------------------------------------------------------------------------------------
def project(K, T_right_in_left, idepth):
    """x' ~ K (R K^-1 [x y 1]^T / idepth + t), (R, t) = inverse(T_right_in_left), in float64 from first principles, with the
    guards of the operation under test (depth = 1 / (idepth + 1e-6), idepth' = 1 / (z' + 1e-6), a divisor of z' + 1e-7;
    stereo/image_predictor.py:538-576): normalised right-image coordinate (B,rows,cols,2), idepth' (B,1,rows,cols), and the
    out-of-image mask |n| > 1."""
    K, T, idp = K.cpu().double(), T_right_in_left.cpu().double(), idepth.cpu().double()
    B, _, rows, cols = idp.shape
    Tl, Ki = torch.linalg.inv(T), torch.linalg.inv(K[:, :3, :3])
    ys, xs = torch.meshgrid(torch.arange(rows, dtype=torch.float64), torch.arange(cols, dtype=torch.float64), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(rows * cols, dtype=torch.float64)], 0)
    X = (Ki @ pix) / (idp.reshape(B, 1, -1) + 1e-6)
    Xr = Tl[:, :3, :3] @ X + Tl[:, :3, 3:4]
    id_prime = (1.0 / (Xr[:, 2] + 1e-6)).view(B, 1, rows, cols)
    cam = K[:, :3, :3] @ Xr
    u, v = cam[:, 0] / (cam[:, 2] + 1e-7), cam[:, 1] / (cam[:, 2] + 1e-7)
    uv = torch.stack([(u + 0.5) * 2.0 / cols - 1.0, (v + 0.5) * 2.0 / rows - 1.0], -1).view(B, rows, cols, 2)
    return uv, id_prime, ((uv[..., 0].abs() > 1.0) | (uv[..., 1].abs() > 1.0)).unsqueeze(1)


def edge_distance(uv64):
    """Distance of a normalised coordinate from the |n| = 1 predicate, (B,1,rows,cols)."""
    uv64 = torch.as_tensor(uv64)
    return torch.minimum((uv64[..., 0].abs() - 1.0).abs(), (uv64[..., 1].abs() - 1.0).abs()).unsqueeze(1)


# ---- the border-clamped bilinear gather ----------------------------------------------------------------------------
def _pixel_coordinate(n, size):
    """grid_sample's un-normalisation with align_corners=False and its border clip, in float64.  A NaN leaves as 0 (the
    clip's operand order, see bilinear_taps in csrc/mvsn_common.h), an infinity at the nearer border."""
    with np.errstate(invalid="ignore"):
        i = ((n + 1.0) * size - 1.0) * 0.5
        return np.where(i > 0.0, np.minimum(i, size - 1.0), 0.0)


def _coordinate_error(n, size):
    """Bound on |device ix - exact ix| given the SAME fp32 n, before the clip (which is 1-Lipschitz).

    ix = ((n + 1) * size - 1) * 0.5 is three roundings and an exact halving: a = fl(n + 1) is off by at most U |a|, and
    that error is scaled by size; b = fl(a * size) adds U |b|; c = fl(b - 1) adds U |c|, |c| <= |b| + 1.  (Should the
    compiler contract a * size - 1 into one fma, b's rounding disappears and the bound only has room.)  To first order
    in U the three sum to U (3 |n + 1| size + 1), halved: 1.5 U (|n + 1| size + 1) -- 3 U size at the far border of an
    image, 2e-5 of a pixel at 96 columns.  A non-finite n is clipped to an exact texel on both sides: no error."""
    with np.errstate(invalid="ignore"):
        d = 1.5 * U * (np.abs(n + 1.0) * size + 1.0)
    return np.where(np.isfinite(n), d, 0.0)


def tap_table(uv, rows, cols):
    """Per pixel of uv (..., 2) float64: the four tap indices y * cols + x in the order (y0,x0), (y0,x1), (y1,x0), (y1,x1)
    as int64 (..., 4), and their float64 weights (..., 4)."""
    uv = np.asarray(uv, np.float64)
    ix, iy = _pixel_coordinate(uv[..., 0], cols), _pixel_coordinate(uv[..., 1], rows)
    x0, y0 = np.floor(ix), np.floor(iy)
    fx, fy = ix - x0, iy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, cols - 1), np.minimum(y0 + 1, rows - 1)
    idx = np.stack([y0 * cols + x0, y0 * cols + x1, y1 * cols + x0, y1 * cols + x1], -1)
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], -1)
    return idx, w


def _gather(flat, idx):
    """flat (B, P) at idx (B, ..., 4) -> (B, ..., 4)."""
    B = flat.shape[0]
    return np.take_along_axis(flat, idx.reshape(B, -1), axis=1).reshape(idx.shape)


def sample(image, uv):
    """grid_sample(image, uv, bilinear, border, align_corners=False) in float64: image (B,1,rows,cols), uv (B,r,c,2) ->
    (B,1,r,c).  The four products are summed in the kernel's order."""
    image = np.asarray(image, np.float64)
    B, _, rows, cols = image.shape
    idx, w = tap_table(uv, rows, cols)
    taps = _gather(image.reshape(B, -1), idx)
    return (((taps[..., 0] * w[..., 0] + taps[..., 1] * w[..., 1]) + taps[..., 2] * w[..., 2]) + taps[..., 3] * w[..., 3])[:, None]


def _hull(uv32, rows, cols):
    """The texel rectangle [xlo, xhi] x [ylo, yhi] (inclusive, int64, per pixel) that holds every tap the device can
    read: its coordinate lies within _coordinate_error of the float64 one, both are clipped, and the taps of a
    coordinate i are floor(i) and floor(i) + 1 (clipped).  At most 3 texels wide: the error is far below 1."""
    uv = np.asarray(uv32, np.float64)
    out = []
    for n, size in ((uv[..., 0], cols), (uv[..., 1], rows)):
        d = _coordinate_error(n, size)
        with np.errstate(invalid="ignore"):
            raw = ((n + 1.0) * size - 1.0) * 0.5
        raw = np.where(np.isnan(raw), 0.0, raw)
        lo = np.floor(np.clip(raw - d, 0.0, size - 1.0)).astype(np.int64)
        hi = np.minimum(np.floor(np.clip(raw + d, 0.0, size - 1.0)).astype(np.int64) + 1, size - 1)
        out += [lo, hi, d]
    (xlo, xhi, dx), (ylo, yhi, dy) = out[:3], out[3:]
    return xlo, xhi, ylo, yhi, dx, dy


def _hull_reduce(image, hull, op, init):
    """op-reduction of image (B,rows,cols) over each pixel's hull (B,r,c); the hull is at most `span` texels a side."""
    xlo, xhi, ylo, yhi = hull
    B, rows, cols = image.shape
    flat = image.reshape(B, -1)
    span_x, span_y = int((xhi - xlo).max()) + 1, int((yhi - ylo).max()) + 1
    acc = np.full(xlo.shape, init, dtype=image.dtype)
    for j in range(span_y):
        for i in range(span_x):
            y, x = np.minimum(ylo + j, yhi), np.minimum(xlo + i, xhi)
            acc = op(acc, np.take_along_axis(flat, (y * cols + x).reshape(B, -1), axis=1).reshape(xlo.shape))
    return acc


def sample_bound(image, uv32, rows, cols):
    """Per-pixel bound (B,1,r,c) on |device sampled - sample(image, float64(device uv))|.

    Coordinate part.  The bilinear interpolant with border clip is continuous and piecewise linear in (ix, iy); its
    partial derivative along x is a convex combination of differences of horizontally adjacent texels, along y of
    vertically adjacent ones, each at most D = max - min over the texel hull the coordinate can reach (_hull: 3x3 at the
    most).  So moving the coordinate by (dx, dy) = _coordinate_error moves the sample by at most (dx + dy) D -- also
    across a cell face, where floor() picks other taps -- and never by more than D.
    Arithmetic part.  fx = ix - floor(ix) is exact.  A weight is two subtractions from 1 and a product: 3 U relative.
    Each tap * weight rounds once (U relative), and the three additions round at most U of a partial sum that
    M = max |tap| bounds, the weights summing to 1: (3 + 1) U M + 3 U M = 7 U M, 8 U M with room for second order."""
    image = np.asarray(image, np.float64)
    B = image.shape[0]
    img = image.reshape(B, rows, cols)
    xlo, xhi, ylo, yhi, dx, dy = _hull(uv32, rows, cols)
    hull = (xlo, xhi, ylo, yhi)
    D = _hull_reduce(img, hull, np.maximum, -np.inf) - _hull_reduce(img, hull, np.minimum, np.inf)
    M = _hull_reduce(np.abs(img), hull, np.maximum, 0.0)
    return (np.minimum(dx + dy, 1.0) * D + 8.0 * U * M)[:, None]


def mask_sampled_sandwich(mask, uv32, rows, cols):
    """(must_set, may_set), bool (B,1,r,c), for the device flag `sum(mask[tap] * weight) > 0` at the device's own uv.

    The weight of texel j along an axis is the tent max(0, 1 - |i - j|) (the border clip merges two taps onto one texel,
    which adds their weights): 1-Lipschitz in the coordinate, whatever cell floor() picks.  A product of two such
    weights in [0, 1] moves by at most dx + dy under the coordinate error, and the fp32 weight (3 U relative) stays
    positive when the exact one is.  must_set: a set tap whose float64 weight exceeds dx + dy + 4 U.  may_set: a set
    texel anywhere in the hull of reachable taps.  must_set <= flag <= may_set, for every pixel."""
    m = np.asarray(mask).astype(bool)
    B = m.shape[0]
    m = m.reshape(B, rows, cols)
    idx, w = tap_table(uv32, rows, cols)
    xlo, xhi, ylo, yhi, dx, dy = _hull(uv32, rows, cols)
    taps = _gather(m.reshape(B, -1), idx)
    must = (taps & (w > (dx + dy + 4.0 * U)[..., None])).any(-1)
    may = _hull_reduce(m, (xlo, xhi, ylo, yhi), np.logical_or, False)
    return must[:, None], may[:, None]


def centre_slack(image, uv, rows, cols):
    """What the projector tolerance lets a coordinate that should be a pixel centre move the sample by: the uv tolerance
    in pixels (half the size per unit of n) times the range of the hull, as in sample_bound.  (B,1,r,c)."""
    uv = np.asarray(uv, np.float64)
    px = 0.5 * ((UV_ATOL + UV_RTOL * np.abs(uv[..., 0])) * cols + (UV_ATOL + UV_RTOL * np.abs(uv[..., 1])) * rows)
    img = np.asarray(image, np.float64).reshape(-1, rows, cols)
    hull = _hull(uv, rows, cols)[:4]
    D = _hull_reduce(img, hull, np.maximum, -np.inf) - _hull_reduce(img, hull, np.minimum, np.inf)
    return (px * D)[:, None]


def reachable_values(mask, uv32, rows, cols):
    """(sees_set, sees_clear), bool (B,1,r,c): the hull of reachable taps holds a set / a clear texel."""
    m = np.asarray(mask).astype(bool)
    m = m.reshape(m.shape[0], rows, cols)
    hull = _hull(uv32, rows, cols)[:4]
    return _hull_reduce(m, hull, np.logical_or, False)[:, None], _hull_reduce(~m, hull, np.logical_or, False)[:, None]


# ---- exact restatements ----------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def absdiff_terms(sampled, idp):
    """|float32(sampled) - float32(idp)| in fp32: the kernel's term, bit for bit."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(_f32(sampled) - _f32(idp))


def block_sums(terms, B):
    """float64 sums of the fp32 terms (B, P) per block of RP_THREADS pixels, and the sums of their magnitudes: two
    (B, nblocks) arrays.  The last block may be partly filled."""
    t = np.asarray(terms, np.float32).reshape(B, -1).astype(np.float64)
    P = t.shape[1]
    nb = (P + RP_THREADS - 1) // RP_THREADS
    pad = np.zeros((B, nb * RP_THREADS))
    pad[:, :P] = t
    pad = pad.reshape(B, nb, RP_THREADS)
    with np.errstate(invalid="ignore", over="ignore"):
        return pad.sum(-1), np.abs(pad).sum(-1)


def occlusion_threshold(partials, P):
    """float32(sequential float64 sum of partials[b, :] / P), (B,) fp32."""
    partials = np.asarray(partials, np.float32)
    out = np.empty(partials.shape[0], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(partials.shape[0]):
            s = np.float64(0.0)
            for v in partials[b]:
                s = s + np.float64(v)
            out[b] = np.float32(s / np.float64(P))
    return out


def occlusion_mask(idp, sampled, invalid, partials):
    """((sampled - idp) > thr) | invalid in fp32, per element: bool (B, P).  A NaN threshold or difference compares
    false, so the mask is `invalid` there."""
    B = np.asarray(partials).shape[0]
    idp, sampled = _f32(idp).reshape(B, -1), _f32(sampled).reshape(B, -1)
    thr = occlusion_threshold(partials, idp.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        return ((sampled - idp) > thr[:, None]) | (np.asarray(invalid).reshape(B, -1) != 0)


def masked_l1(a, b, skip_a, skip_b):
    """float32(S / C): S the float64 sum of the fp32 terms |a - b| over elements with neither flag set (math.fsum: the
    exactly rounded sum), C their count.  0 / 0 is NaN.  Also returns S and C."""
    a, b = _f32(a).reshape(-1), _f32(b).reshape(-1)
    keep = (np.asarray(skip_a).reshape(-1) == 0) & (np.asarray(skip_b).reshape(-1) == 0)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.abs(a[keep] - b[keep]).astype(np.float64)
    S = math.fsum(terms) if np.isfinite(terms).all() else float(terms.sum())
    C = int(keep.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(np.float64(S) / np.float64(C)), S, C


def ulp32(x):
    """Spacing of fp32 at |x| (towards the larger magnitude)."""
    x = np.abs(np.float32(x))
    return float(np.nextafter(x, np.float32(np.inf)) - x)


def depth_metric_terms(idepth, truth, baseline, lo, hi):
    """The kernel's per-pixel terms of one image in numpy float32 (IEEE division, no multiply feeds an add): a dict of
    `truth` and `sel` masks and, over the selected pixels, t, e, abs_rel, sq_rel, sq terms and the three ratio flags."""
    t = _f32(truth).reshape(-1)
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        scaled = _f32(idepth).reshape(-1) / np.float32(baseline)
        e = np.where(scaled > 0, np.float32(1.0) / scaled, scaled).astype(np.float32)
        tr = (t > lo) & (t < hi)
        sel = tr & (e > lo) & (e < hi)
        ts, es = t[sel], e[sel]
        diff = ts - es
        ratio = np.maximum(ts / es, es / ts)
    return {"truth": tr, "sel": sel, "scaled": scaled, "e_all": e, "t": ts, "e": es, "abs_rel": np.abs(diff) / ts,
            "sq_rel": (diff * diff) / ts, "sq": diff * diff, "ratio": ratio,
            "a": [ratio < np.float32(1.25), ratio < np.float32(1.5625), ratio < np.float32(1.953125)]}


def depth_metric_rows64(idepth, truth, baseline, lo, hi):
    """The device rows from the exact fp32 terms summed in float64 (math.fsum: exactly rounded), image by image.
    idepth, truth (B, P); baseline (B,).  A dict:
      rows      (B, 9) float64 {n_truth, n_sel, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3}, NaN without a selected pixel;
                rmse_log takes log in float64 on the fp32 t and e (the device's logf is the one term not restated)
      sums      (B, 4) float64: the sums of abs_rel, sq_rel, sq and log_sq terms (all non-negative: also their
                sums of magnitudes)
      a_counts  (B, 3) int64 numerators of a1, a2, a3"""
    idepth, truth = np.asarray(idepth), np.asarray(truth)
    B = idepth.shape[0]
    rows, sums, counts = np.full((B, 9), np.nan), np.zeros((B, 4)), np.zeros((B, 3), np.int64)
    for b in range(B):
        m = depth_metric_terms(idepth[b], truth[b], np.asarray(baseline).reshape(-1)[b], lo, hi)
        n = int(m["sel"].sum())
        rows[b, 0], rows[b, 1] = float(m["truth"].sum()), float(n)
        lg = np.log(m["t"].astype(np.float64)) - np.log(m["e"].astype(np.float64))
        sums[b] = [math.fsum(m[k].astype(np.float64)) for k in ("abs_rel", "sq_rel", "sq")] + [math.fsum(lg * lg)]
        counts[b] = [int(f.sum()) for f in m["a"]]
        if n:
            with np.errstate(all="ignore"):
                rows[b, 2:] = [sums[b, 0] / n, sums[b, 1] / n, np.sqrt(sums[b, 2] / n), np.sqrt(sums[b, 3] / n)] + \
                              [c / n for c in counts[b]]
    return {"rows": rows, "sums": sums, "a_counts": counts}


def metric_blocks(pixels):
    """mvsn_depth_metrics_blocks restated."""
    return 0 if pixels <= 0 else min(MT_BLOCK_CAP, (pixels + MT_BLOCK_PIXELS - 1) // MT_BLOCK_PIXELS)


# ---- the scenes of the reprojection tests ---------------------------------------------------------------------------------
SHAPES = ((3, 5), (16, 16), (1, 257), (9, 1), (37, 53), (64, 96))
SHAPE_IDS = tuple(f"{r}x{c}" for r, c in SHAPES)
BATCH = 3


def _rotation(roll, yaw, pitch):
    cr, sr, cy, sy, cp, sp = math.cos(roll), math.sin(roll), math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1.0]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return Rz @ Ry @ Rx


def _smooth(rng, B, rows, cols):
    """0.06 +- 0.03 of low-frequency sinusoids plus noise of 0.004, (B,1,rows,cols) float64."""
    yy, xx = np.meshgrid(np.arange(rows) / max(rows, 8), np.arange(cols) / max(cols, 8), indexing="ij")
    out = np.zeros((B, 1, rows, cols))
    for b in range(B):
        acc = np.zeros((rows, cols))
        for _ in range(4):
            fx, fy, ph = rng.uniform(0.3, 2.5), rng.uniform(0.3, 2.5), rng.uniform(0, 2 * math.pi)
            acc += rng.uniform(0.3, 1.0) * np.sin(2 * math.pi * (fx * xx + fy * yy) + ph)
        out[b, 0] = 0.06 + 0.03 * acc / max(np.abs(acc).max(), 1e-6) + 0.004 * rng.standard_normal((rows, cols))
    return out


@functools.lru_cache(maxsize=None)
def scene(rows, cols, identity=False):
    """K, T (B,4,4), this view's idepth map L and the other view's R (B,1,rows,cols), float32 torch tensors on the CPU.

    K is hand-built with fx != fy and a principal point off the centre by another amount per element; T is a roll, yaw
    and pitch of a few degrees plus a translation, another per element.  A one-row (one-column) image keeps only the
    rotation about its short axis and the translation along its long one, and a principal point within 0.2 px of the
    single row (column): anything else moves every pixel out of an image one pixel high.  R carries a nearer band (+0.05)
    over the first third of its rows (of its columns when it has fewer than three rows): real occlusions."""
    rng = np.random.RandomState(1000 * rows + cols)
    B = BATCH
    K, T = np.zeros((B, 4, 4)), np.zeros((B, 4, 4))
    thin_rows, thin_cols = rows < 3, cols < 3
    for b in range(B):
        fx, fy = (1.05 + 0.1 * b) * max(cols, 4), (1.3 - 0.12 * b) * max(rows, 4)
        cx = cols / 2.0 + (0.07 * cols * (b - 1) + 0.3 if not thin_cols else (0.1, -0.15, 0.2)[b]) - (0.5 if thin_cols else 0.0)
        cy = rows / 2.0 + (-0.05 * rows * (b - 1) + 0.2 if not thin_rows else (0.1, -0.15, 0.2)[b]) - (0.5 if thin_rows else 0.0)
        K[b] = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
        roll, yaw, pitch = math.radians(2.0 + b), math.radians(-3.0 + 2.5 * b), math.radians(1.5 - 1.0 * b)
        t = np.array([2.4 - 1.9 * b, -1.6 + 1.3 * b, 0.6 * (b - 1)])
        if thin_rows:
            roll, pitch, t = 0.0, 0.0, np.array([2.4 - 1.9 * b, 0.0, 0.4 * (b - 1)])
        if thin_cols:
            roll, yaw, t = 0.0, 0.0, np.array([0.0, 2.4 - 1.9 * b, 0.4 * (b - 1)])
        T[b] = np.eye(4)
        if not identity:
            T[b, :3, :3], T[b, :3, 3] = _rotation(roll, yaw, pitch), t
    L, R = _smooth(rng, B, rows, cols), _smooth(rng, B, rows, cols)
    if not identity:
        if rows >= 3:
            R[:, :, : rows // 3] += 0.05
        else:
            R[:, :, :, : cols // 3] += 0.05
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    return f(K), f(T), f(L), f(R)


@functools.lru_cache(maxsize=None)
def scene_masks(rows, cols):
    """The two masks of the other view the mask_sampled tests use, bool (B,1,rows,cols) numpy: `random` at 30 % density;
    `single` with one set texel per element, the texel nearest to where that element's middle pixel lands."""
    K, T, L, _ = scene(rows, cols)
    rng = np.random.RandomState(7 + 1000 * rows + cols)
    random = rng.uniform(size=(BATCH, 1, rows, cols)) < 0.3
    uv64 = project(K, T, L)[0].numpy()
    single = np.zeros((BATCH, 1, rows, cols), bool)
    for b in range(BATCH):
        inside = (np.abs(uv64[b]) <= 0.9).all(-1).reshape(-1)
        pick = np.flatnonzero(inside)[inside.sum() // 2] if inside.any() else (rows * cols) // 2
        idx, w = tap_table(uv64[b].reshape(-1, 2)[pick], rows, cols)
        single[b].reshape(-1)[idx[int(np.argmax(w))]] = True
    return random, single


# ---- the inputs of the depth-metric tests ---------------------------------------------------------------------------------
METRIC_RANGE = (0.5, 10.0)
METRIC_PIXELS = (1, 255, 256, 257, 8192, 8193, 16385, 524288, 524289, 529920)
METRIC_BASELINES = (1.375, 1.0, 0.8125)     # (image 0 carries the plants: 10 is an estimate fp32 reaches at 1.375)


def _estimates_near(e_target, base):
    """fp32 idepths within a few steps of base / e_target and the estimates 1 / (idepth / base) the device forms of them."""
    base = np.float32(base)
    cands = [np.float32(base / np.float32(e_target))]
    for _ in range(8):
        cands = [np.nextafter(cands[0], np.float32(-np.inf))] + cands + [np.nextafter(cands[-1], np.float32(np.inf))]
    cands = np.array(cands, np.float32)
    return cands, (np.float32(1.0) / (cands / base)).astype(np.float32)


def idepth_for(e_target, base, side=0):
    """An fp32 idepth whose device conversion 1 / (idepth / base) is exactly float32(e_target) (side 0), or the nearest
    estimate above (side +1) / below (side -1) it that a neighbouring idepth reaches; None if there is none."""
    e_target = np.float32(e_target)
    cands, e = _estimates_near(e_target, base)
    ok = e == e_target if side == 0 else (e > e_target if side > 0 else e < e_target)
    if not ok.any():
        return None
    return cands[ok][int(np.argmin(np.abs(e[ok].astype(np.float64) - float(e_target))))]


def metric_plants(base):
    """(t, idepth) pairs planted on predicates: truth and estimate exactly at both range ends and one fp32 step inside (the
    estimate: the nearest value inside that an fp32 idepth reaches), and ratios t / e exactly at 1.25, 1.5625, 1.953125 and
    one fp32 step to either side (e = 2 exactly)."""
    lo, hi = np.float32(METRIC_RANGE[0]), np.float32(METRIC_RANGE[1])
    up, down = np.float32(np.inf), np.float32(-np.inf)
    two, mid = idepth_for(2.0, base), idepth_for(4.0, base)
    pairs = []
    for t in (lo, np.nextafter(lo, up), hi, np.nextafter(hi, down)):
        pairs.append((t, mid))
    for e, side in ((lo, 0), (lo, +1), (hi, 0), (hi, -1)):
        pairs.append((np.float32(4.0), idepth_for(e, base, side)))
    for r in (1.25, 1.5625, 1.953125):
        t = np.float32(2.0 * r)
        pairs += [(np.nextafter(t, down), two), (t, two), (np.nextafter(t, up), two)]
    assert all(i is not None for _, i in pairs), "a planted estimate has no fp32 idepth"
    return pairs


@functools.lru_cache(maxsize=None)
def metric_case(pixels):
    """idepth, truth (3, pixels) and baseline (3,), float32 numpy.  Truth with holes (0) and values past the range,
    estimates with zero and negative idepths; image 1 has no valid truth, image 2 no selected pixel; image 0 carries
    metric_plants at its first and at its last pixels when it has room for both."""
    rng = np.random.RandomState(pixels % 100003)
    B = 3
    truth = (rng.uniform(size=(B, pixels)) * 12.0).astype(np.float32)
    truth[truth < 1.0] = 0.0
    base = np.array(METRIC_BASELINES, np.float32)
    est = np.maximum(truth, np.float32(0.3)) * (0.7 + 0.6 * rng.uniform(size=(B, pixels))).astype(np.float32)
    idepth = (base[:, None] / est).astype(np.float32)
    idepth[:, 3::7] = 0.0
    idepth[:, 5::9] = -0.25
    if pixels == 1:
        truth[0, 0], idepth[0, 0] = 3.0, idepth_for(2.5, base[0])
    plants = metric_plants(base[0])
    if pixels >= 2 * len(plants) + 16:
        for k, (t, i) in enumerate(plants):          # (the image's last pixel is a selected one)
            truth[0, k], idepth[0, k] = t, i
            truth[0, pixels - len(plants) + k], idepth[0, pixels - len(plants) + k] = t, i
    truth[1] = 0.0
    idepth[2] = -1.0
    return idepth, truth, base
