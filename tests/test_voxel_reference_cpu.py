"""The numpy restatement of the voxel merge (tests/voxel_reference.py) against an independent brute force: a dict keyed
by the cell tuple, float64 means of the member points themselves."""
import numpy as np
import pytest

from voxel_reference import voxel_reference


def _brute_force(points, voxel_size, colors, origin):
    """Point by point in Python.  The cell is formed in fp32 scalars (the contract's partition); the means are plain
    float64 means of the member coordinates and colours, with no quantisation."""
    v = np.float32(voxel_size)
    inv = np.float32(1) / v
    o = [np.float32(x) for x in origin]
    voxels, inverse = {}, []
    for i, p in enumerate(points):
        if not all(np.isfinite(x) for x in p):
            inverse.append(None)
            continue
        cell = tuple(int(np.floor((np.float32(p[a]) - o[a]) * inv)) for a in range(3))
        voxels.setdefault(cell, []).append(i)
        inverse.append(cell)
    cells = sorted(voxels, key=lambda c: voxels[c][0])
    row = {c: r for r, c in enumerate(cells)}
    members = [voxels[c] for c in cells]
    return {"cells": np.array(cells, np.int64).reshape(-1, 3),
            "first": np.array([m[0] for m in members], np.int64),
            "count": np.array([len(m) for m in members], np.int64),
            "inverse": np.array([-1 if c is None else row[c] for c in inverse], np.int64),
            "mean": np.array([points[m].astype(np.float64).mean(axis=0) for m in members]).reshape(-1, 3),
            "colour_mean": None if colors is None else
            np.array([colors[m].astype(np.float64).mean(axis=0) for m in members]).reshape(-1, 3)}


def _cloud(seed, n, span, centre=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    pts = (rng.uniform(-span, span, (n, 3)) + np.asarray(centre)).astype(np.float32)
    cols = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    return pts, cols


CASES = [
    # seed, points, half extent, centre, voxel size, origin
    (0, 600, 1.0, (0.0, 0.0, 0.0), 0.25, (0.0, 0.0, 0.0)),          # ~9 points per voxel, both signs
    (1, 500, 0.5, (3.0, -2.0, 7.5), 0.05, (0.125, -0.3, 0.01)),      # mostly one point per voxel, an origin
    (2, 400, 2.0, (100.0, 50.0, -80.0), 0.7, (-1.0, 2.0, 3.0)),      # coordinates far from the origin
    (3, 300, 0.01, (0.0, 0.0, 0.0), 1.0, (0.0, 0.0, 0.0)),           # eight voxels around the origin
]


@pytest.mark.parametrize("seed, n, span, centre, voxel, origin", CASES)
def test_restatement_matches_the_brute_force(seed, n, span, centre, voxel, origin):
    pts, cols = _cloud(seed, n, span, centre)
    pts[n // 3] = pts[n // 7]                               # an exact duplicate
    pts[n // 2, 1] = np.nan                                 # two dropped points
    pts[n // 5, 2] = np.inf
    ref = voxel_reference(pts, voxel, colors=cols, origin=origin)
    bf = _brute_force(pts, voxel, cols, origin)
    # the partition, exactly
    np.testing.assert_array_equal(ref["cells"], bf["cells"])
    np.testing.assert_array_equal(ref["first"], bf["first"])
    np.testing.assert_array_equal(ref["count"], bf["count"])
    np.testing.assert_array_equal(ref["inverse"], bf["inverse"])
    assert ref["inverse"][n // 2] == -1 and ref["inverse"][n // 5] == -1
    assert ref["inverse"][n // 3] == ref["inverse"][n // 7]
    assert ref["count"].sum() == n - 2 and ref["count"].dtype == np.int32
    assert (np.diff(ref["first"]) > 0).all()
    # positions: v 2^-17 of centred quantisation, doubled, plus the fp32 roundings of s, inv, t and of the result,
    # about 4 * 2^-24 relative to the largest coordinate, doubled
    v = float(np.float32(voxel))
    finite = pts[np.isfinite(pts).all(axis=1)]
    bound = v * 2.0 ** -16 + 2.0 ** -21 * float(np.abs(finite).max())
    err = np.abs(ref["points"].astype(np.float64) - bf["mean"])
    assert err.max() <= bound, (err.max(), bound)
    assert ref["points"].dtype == np.float32
    # colours: round-half-up of the exact mean
    np.testing.assert_array_equal(ref["colors"], np.floor(bf["colour_mean"] + 0.5).astype(np.uint8))


def test_restatement_colour_rounds_half_up_and_position_is_order_free():
    pts = np.array([[0.1, 0.2, 0.3], [0.15, 0.25, 0.35], [0.4, 0.1, 0.2], [0.3, 0.3, 0.3]], np.float32)
    cols = np.array([[0, 1, 255], [1, 2, 255], [0, 0, 254], [1, 0, 255]], np.uint8)
    ref = voxel_reference(pts, 1.0, colors=cols)
    assert ref["count"].tolist() == [4] and ref["first"].tolist() == [0]
    # means 0.5 -> 1, 0.75 -> 1, 254.75 -> 255
    assert ref["colors"].tolist() == [[1, 1, 255]]
    perm = np.array([2, 0, 3, 1])
    again = voxel_reference(pts[perm], 1.0, colors=cols[perm])
    assert again["points"].tobytes() == ref["points"].tobytes()
    np.testing.assert_array_equal(again["colors"], ref["colors"])


def test_restatement_faces_clamp_and_range():
    v = 0.5
    pts = np.array([[1.0, -1.0, 0.0],            # exactly on faces: t an integer, fraction 0, the upper cell
                    [-1e-10, 0.25, 0.25],         # t = -2e-10: cell -1, fraction rounds to 1.0, q clamps to 65535
                    [-0.25, 0.25, 0.25]], np.float32)
    ref = voxel_reference(pts, v)
    np.testing.assert_array_equal(ref["cells"], [[2, -2, 0], [-1, 0, 0]])
    assert ref["count"].tolist() == [1, 2]
    # the clamped point sits at the cell's last sixteenth-bit, just inside its upper face
    x = ref["points"][1, 0]
    want = (-1 + ((65535 + 32768) / 2 + 0.5) / 65536.0) * v
    assert x == np.float32(want) and x < 0
    with pytest.raises(ValueError, match="voxel_size too small"):
        voxel_reference(np.array([[2.0 ** 20 * v, 0, 0]], np.float32), v)
    with pytest.raises(ValueError, match="voxel_size too small"):
        voxel_reference(np.array([[0, -(2.0 ** 20 + 1) * v, 0]], np.float32), v)
    inside = voxel_reference(np.array([[np.nextafter(np.float32(2.0 ** 20 * v), np.float32(0)), -(2.0 ** 20) * v, 0]],
                                      np.float32), v)
    np.testing.assert_array_equal(inside["cells"], [[2 ** 20 - 1, -2 ** 20, 0]])
    # no finite point kept: an empty cloud, every inverse -1
    none = voxel_reference(np.full((3, 3), np.nan, np.float32), v)
    assert none["points"].shape == (0, 3) and none["inverse"].tolist() == [-1, -1, -1]
