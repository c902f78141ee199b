"""numpy restatement of the voxel-grid merge (multi_view_stereonet_amd/fusion.py: voxel_merge).

The cell and the in-cell fraction of a point are formed with the same fp32 operations as the kernels (a subtract, a
multiply, a floor, a subtract, a multiply by 2^16: numpy rounds each once, as the device does), so the partition into
voxels is the device's exactly and no margin class is needed.  Sums are integers; the means are the float64 expression
of the contract."""
import numpy as np

CELL_LIMIT = 1 << 20


def cells_and_fractions(points, voxel_size, origin=(0.0, 0.0, 0.0)):
    """(kept (N,) bool, c (N,3) int64, q (N,3) int64) of float32 ``points``; raises ValueError where a finite point's
    cell lies outside [-2^20, 2^20)."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    v = np.float32(voxel_size)
    inv = np.float32(1) / v
    o = np.asarray(origin, dtype=np.float64).astype(np.float32)
    with np.errstate(all="ignore"):
        s = p - o
        t = s * inv
        c = np.floor(t)
        f = t - c
        g = f * np.float32(65536)
    assert s.dtype == t.dtype == c.dtype == f.dtype == g.dtype == np.float32
    kept = np.isfinite(p).all(axis=1) & np.isfinite(t).all(axis=1)
    outside = kept & ((c < -CELL_LIMIT) | (c >= CELL_LIMIT)).any(axis=1)
    if outside.any():
        raise ValueError(f"voxel_size too small for the cloud's extent: point {int(np.argmax(outside))}")
    ci = np.where(kept[:, None], c, 0).astype(np.int64)
    qi = np.minimum(65535, np.where(kept[:, None], g, 0).astype(np.int64))
    return kept, ci, qi


def voxel_reference(points, voxel_size, colors=None, origin=(0.0, 0.0, 0.0)):
    """dict of points (M,3) f32, colors (M,3) u8 or None, count (M,) i32, first (M,) i64, inverse (N,) i64 and
    cells (M,3) i64."""
    kept, c, q = cells_and_fractions(points, voxel_size, origin)
    n_pts = kept.shape[0]
    idx = np.nonzero(kept)[0]
    key = ((c[idx, 0] + CELL_LIMIT) << 42) | ((c[idx, 1] + CELL_LIMIT) << 21) | (c[idx, 2] + CELL_LIMIT)
    _, first_k, inv_k = np.unique(key, return_index=True, return_inverse=True)
    inv_k = inv_k.reshape(-1)
    order = np.argsort(first_k, kind="stable")              # rows by their lowest input index
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    first = idx[first_k[order]].astype(np.int64)
    rows = rank[inv_k]
    inverse = np.full(n_pts, -1, np.int64)
    inverse[idx] = rows
    m = first.shape[0]
    count = np.bincount(rows, minlength=m).astype(np.int64)
    sq = np.zeros((m, 3), np.int64)
    np.add.at(sq, rows, q[idx])
    v64 = np.float64(np.float32(voxel_size))
    o64 = np.asarray(origin, dtype=np.float64).astype(np.float32).astype(np.float64)
    cells = c[first]
    n = count[:, None].astype(np.float64)
    pos = o64 + (cells.astype(np.float64) + (sq.astype(np.float64) / n + 0.5) / 65536.0) * v64
    out = {"points": pos.astype(np.float32), "colors": None, "count": count.astype(np.int32), "first": first,
           "inverse": inverse, "cells": cells}
    if colors is not None:
        col = np.asarray(colors, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        sc = np.zeros((m, 3), np.int64)
        np.add.at(sc, rows, col[idx])
        out["colors"] = ((2 * sc + count[:, None]) // (2 * count[:, None])).astype(np.uint8)
    return out
