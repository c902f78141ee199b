"""numpy restatement of the nearest-neighbour query between clouds (DESIGN.md section 14;
multi_view_stereonet_amd/fusion.py: cloud_nearest, radius_outlier_mask; metrics.py: cloud_metrics).

The brute force over every (query, target) pair with the same fp32 operations as the kernel (three subtracts, three
multiplies, two adds in the stated order: numpy rounds each once, as the device does), so dist2, index and within are
the device's exactly and no margin class is needed.  No grid is used to find neighbours; the grid appears only where
the contract names it: a finite target outside its range raises, and `cell_range` restates the cells the kernel visits
so that the claim "every accepted pair's target cell is among them" can be tested on the host."""
import numpy as np

CELL_LIMIT = 1 << 20
CHUNK_ELEMENTS = 1 << 22


def radius_scalars(max_dist):
    """(h, 1/h, h*h), each formed once in fp32."""
    h = np.float32(max_dist)
    with np.errstate(all="ignore"):
        return h, np.float32(1) / h, h * h


def target_cells(target, max_dist):
    """(usable (T,) bool, t (T,3) float32, c (T,3) float32 = floor(t)) of the grid of cell size h anchored at 0; raises
    ValueError where a finite target has no cell in [-2^20, 2^20)^3."""
    p = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
    _, inv, _ = radius_scalars(max_dist)
    with np.errstate(all="ignore"):
        t = (p - np.float32(0)) * inv
        c = np.floor(t)
    assert t.dtype == c.dtype == np.float32
    finite = np.isfinite(p).all(axis=1)
    inside = (np.isfinite(t) & (c >= -CELL_LIMIT) & (c < CELL_LIMIT)).all(axis=1)
    if (finite & ~inside).any():
        raise ValueError(f"max_dist too small for the target's extent: point {int(np.argmax(finite & ~inside))}")
    return finite, t, c


def cell_range(tq, r2):
    """(lo, hi) float32 arrays, inclusive: the cells of one axis the kernel visits for a query at t = q * inv, before
    the clip to the grid: floor((t - reach) - e) .. floor((t + reach) + e), e = 2^-19 + |t| 2^-20, every step fp32;
    reach is 1 cell, 2 where r2 < 2^-100."""
    t = np.asarray(tq, dtype=np.float32)
    reach = np.float32(2.0 if np.float32(r2) < np.float32(2.0 ** -100) else 1.0)
    with np.errstate(all="ignore"):                          # (a non-finite t has no range: the kernel visits nothing)
        e = np.float32(2.0 ** -19) + np.abs(t) * np.float32(2.0 ** -20)
        lo, hi = np.floor((t - reach) - e), np.floor((t + reach) + e)
    assert e.dtype == lo.dtype == hi.dtype == np.float32
    return lo, hi


def squared_distances(query, target):
    """(N,T) float32: d2 = (dx dx + dy dy) + dz dz of the fp32 differences."""
    q, p = np.asarray(query, np.float32), np.asarray(target, np.float32)
    with np.errstate(all="ignore"):
        dx, dy, dz = (q[:, None, a] - p[None, :, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def cloud_nearest_reference(query, target, max_dist):
    """dict of dist2 (N,) f32 (+inf where no target is within), index (N,) i64 (-1), within (N,) i32."""
    q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1, 3)
    p = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
    _, _, r2 = radius_scalars(max_dist)
    n, m = q.shape[0], p.shape[0]
    dist2 = np.full(n, np.inf, np.float32)
    index = np.full(n, -1, np.int64)
    within = np.zeros(n, np.int32)
    if n == 0 or m == 0:
        return {"dist2": dist2, "index": index, "within": within}
    usable, _, _ = target_cells(p, max_dist)
    chunk = max(1, CHUNK_ELEMENTS // m)
    for a in range(0, n, chunk):
        d2 = squared_distances(q[a:a + chunk], p)
        with np.errstate(invalid="ignore"):
            ok = (d2 <= r2) & usable[None, :]               # a NaN compares false
        masked = np.where(ok, d2, np.float32(np.inf))
        best = masked.argmin(axis=1)                         # the first of equal minima: the lowest row
        rows = np.arange(d2.shape[0])
        found = ok[rows, best]
        dist2[a:a + chunk] = np.where(found, masked[rows, best], np.float32(np.inf))
        index[a:a + chunk] = np.where(found, best, -1)
        within[a:a + chunk] = ok.sum(axis=1)
    return {"dist2": dist2, "index": index, "within": within}


def radius_outlier_reference(points, radius, min_neighbours):
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    ref = cloud_nearest_reference(p, p, radius)
    return (ref["within"].astype(np.int64) - 1 >= int(min_neighbours)) & np.isfinite(p).all(axis=1)


def cloud_metrics_reference(pred, truth, threshold, max_dist=None):
    """The metrics of metrics.cloud_metrics, from the brute force: means in float64, counts as integers."""
    p = np.ascontiguousarray(pred, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(truth, dtype=np.float32).reshape(-1, 3)
    tau = np.float32(threshold)
    tau2 = tau * tau
    h = np.float32(threshold if max_dist is None else max_dist)
    assert h >= tau

    def one_way(a, b):
        d2 = cloud_nearest_reference(a, b, h)["dist2"]
        finite = np.isfinite(a).all(axis=1)
        capped = np.minimum(np.sqrt(d2[finite].astype(np.float64)), np.float64(h))
        return int(finite.sum()), float(capped.sum()), int((d2[finite] <= tau2).sum())

    n_p, s_p, k_p = one_way(p, t)
    n_t, s_t, k_t = one_way(t, p)
    precision, recall = k_p / n_p, k_t / n_t
    fscore = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return {"accuracy": s_p / n_p, "completeness": s_t / n_t, "precision": precision, "recall": recall,
            "fscore": fscore, "n_pred": n_p, "n_truth": n_t, "close_pred": k_p, "close_truth": k_t}


# ---- two inputs of tests/test_cloud_gpu.py at a few dozen points, for the kernels that query through the visitor --------
def reach2_clouds():
    """(query (36,3), target (60,3), h) of test_tiny_max_dist_whose_square_is_a_denormal: h = 2^-74, so r2 = 2^-148 is two
    quanta of the denormal range and the kernel reaches two cells; query 0 and target 0 lie in cells 2 and 0 of x, 1.1 h
    apart, and are within."""
    h = 2.0 ** -74
    rng = np.random.default_rng(45)
    t = (rng.uniform(-2, 2, (60, 3)) * h).astype(np.float32)
    q = (rng.uniform(-2.5, 2.5, (36, 3)) * h).astype(np.float32)
    t[0], q[0] = (0.95 * h, 0, 0), (2.05 * h, 0, 0)
    return q, t, h


def grid_edge_clouds():
    """(query (48,3), target (60,3), h) of test_cluster_at_half_a_million_cells_and_at_the_grids_edge, its second half: on
    each axis and on either side ten targets in the last cells of the grid, up to its edge (cell 2^20 - 1 above, cell
    -2^20 below), and eight queries on both sides of the edge."""
    h = 0.25
    edge = np.float32(2.0 ** 20 * h)
    top = np.nextafter(edge, np.float32(0))                  # the largest coordinate of cell 2^20 - 1
    rng = np.random.default_rng(44)
    q, t = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            shift = np.zeros(3, np.float32)
            shift[axis] = sign * (edge - 0.5)
            width = np.full(3, 0.25)
            width[axis] = 0.5
            tt = rng.uniform(-width, width, (10, 3)).astype(np.float32) + shift
            tt[:, axis] = np.clip(tt[:, axis], -edge, top)   # (-edge is in cell -2^20, the lowest)
            t.append(tt)
            q.append(rng.uniform(-1.2 * width, 1.2 * width, (8, 3)).astype(np.float32) + shift)
    return np.concatenate(q), np.concatenate(t), h
