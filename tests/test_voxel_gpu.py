"""voxel_merge on the device (csrc/mvsn_voxel.hip) against the numpy restatement (tests/voxel_reference.py): inverse,
first, count and colours exactly; positions within one fp32 ulp (the device's fp64 expression can differ from numpy's
in its last double bit only, which moves the rounded fp32 by at most one ulp)."""
import numpy as np
import pytest
import torch

from fusion_reference import nearest_neighbours
from multi_view_stereonet_amd import synthetic
from multi_view_stereonet_amd.fusion import VoxelCloud, fuse_depthmaps, voxel_merge
from voxel_reference import cells_and_fractions, voxel_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _merge(pts, voxel, cols=None, origin=(0.0, 0.0, 0.0)):
    return voxel_merge(torch.from_numpy(pts).to(DEV), voxel, colors=None if cols is None else torch.from_numpy(cols).to(DEV),
                       origin=origin)


def _check(got: VoxelCloud, ref):
    np.testing.assert_array_equal(got.inverse.cpu().numpy(), ref["inverse"])
    np.testing.assert_array_equal(got.first.cpu().numpy(), ref["first"])
    np.testing.assert_array_equal(got.count.cpu().numpy(), ref["count"])
    assert got.points.dtype == torch.float32 and got.count.dtype == torch.int32
    assert got.first.dtype == torch.int64 and got.inverse.dtype == torch.int64
    if ref["colors"] is None:
        assert got.colors is None
    else:
        assert got.colors.dtype == torch.uint8
        np.testing.assert_array_equal(got.colors.cpu().numpy(), ref["colors"])
    pts = got.points.cpu().numpy()
    assert pts.shape == ref["points"].shape
    err = np.abs(pts.astype(np.float64) - ref["points"].astype(np.float64))
    assert (err <= np.spacing(np.abs(ref["points"])).astype(np.float64)).all(), err.max()


def _hand_case():
    n, v, origin = 1027, 0.25, (0.125, -0.5, 2.0)
    rng = np.random.default_rng(11)
    pts = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)            # both signs, ~14^3 cells: several per voxel
    cols = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    o = np.asarray(origin, np.float32)
    pts[100:110] = pts[5]                                               # exact duplicates
    pts[500] = pts[499]
    # exactly on cell faces: t an integer on every axis (origin + k v is exact in fp32 here)
    for j, k in enumerate([(-3, 2, 0), (0, 0, 0), (5, -7, 1), (-1, -1, -1)]):
        pts[200 + j] = o + np.asarray(k, np.float32) * np.float32(v)
    # the float just below a face on one axis: t = -2^-25 on x, whose fraction 1 - 2^-25 rounds to 1.0 and must clamp
    # to 65535; t = -2^-22 on y and -2^-21 on z, whose fractions stay below 1 and floor to 65535
    below = np.nextafter(o, np.float32(-np.inf))
    pts[300] = (below[0], o[1] + np.float32(0.1), o[2] + np.float32(0.1))
    pts[301] = (o[0] + np.float32(0.1), below[1], o[2] + np.float32(0.1))
    pts[302] = (o[0] + np.float32(0.5), o[1] + np.float32(0.5), below[2])
    # two members of one voxel at indices 0 and N - 1
    pts[0] = o + np.array([10.0, 10.0, 10.0], np.float32) + np.float32(0.01)
    pts[n - 1] = o + np.array([10.0, 10.0, 10.0], np.float32) + np.float32(0.2)
    return pts, cols, v, origin


def test_hand_case_1027_points():
    pts, cols, v, origin = _hand_case()
    kept, c, q = cells_and_fractions(pts, v, origin)
    assert kept.all()
    assert (q[200:204] == 0).all()                                      # on the faces: fraction 0, the upper cell
    assert q[300, 0] == 65535 and q[301, 1] == 65535 and q[302, 2] == 65535 and (c[[300, 301, 302], [0, 1, 2]] == -1).all()
    t = (pts[300, 0] - np.float32(origin[0])) * (np.float32(1) / np.float32(v))
    assert t == -2.0 ** -25 and t - np.floor(t) == np.float32(1.0)      # the clamp is what keeps q at 65535 here
    ref = voxel_reference(pts, v, colors=cols, origin=origin)
    assert ref["inverse"][0] == ref["inverse"][-1] == 0 and ref["count"][0] == 2
    assert ref["count"][ref["inverse"][5]] >= 11 and 1 < len(ref["first"]) < len(pts)
    _check(_merge(pts, v, cols, origin), ref)
    _check(_merge(pts, v, None, origin), voxel_reference(pts, v, origin=origin))


def test_tiny_negative_coordinates_clamp_into_the_cell_below():
    # t = -4e-10, -4e-20, -4e-30 (all normal floats): cell -1 and a fraction that rounds to 1.0 on every axis
    pts = np.array([[-1e-10, -1e-20, -1e-30], [-0.1, -0.1, -0.1], [1e-10, 1e-20, 1e-30]], np.float32)
    kept, c, q = cells_and_fractions(pts, 0.25)
    assert (c[0] == -1).all() and (q[0] == 65535).all() and (c[2] == 0).all() and (q[2] == 0).all()
    got = _merge(pts, 0.25)
    _check(got, voxel_reference(pts, 0.25))
    assert got.inverse.tolist() == [0, 0, 1] and got.count.tolist() == [2, 1]
    assert (got.points[0] < 0).all() and (got.points[1] > 0).all()


def test_single_point():
    pts = np.array([[-1.3, 0.7, 2.9]], np.float32)
    cols = np.array([[7, 0, 255]], np.uint8)
    got = _merge(pts, 0.1, cols)
    _check(got, voxel_reference(pts, 0.1, colors=cols))
    assert got.count.tolist() == [1] and got.first.tolist() == [0] and got.inverse.tolist() == [0]
    assert got.colors.cpu().tolist() == [[7, 0, 255]]


def test_empty_cloud_on_the_device():
    vc = voxel_merge(torch.zeros(0, 3, device=DEV), 0.1, colors=torch.zeros(0, 3, dtype=torch.uint8, device=DEV))
    assert vc.points.shape == (0, 3) and vc.colors.shape == (0, 3) and vc.inverse.shape == (0,)
    assert vc.points.device.type == "cuda"


def _uniform_cloud():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-2.0, 2.0, (20000, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (20000, 3)).astype(np.uint8)
    return pts, cols


def test_many_voxels_uniform_random():
    # 20 000 points in 400^3 cells: nearly every point its own voxel, so the table (65 536 slots) takes ~20 000 keys:
    # collisions, probe sequences, and sequences that run over the table's end
    pts, cols = _uniform_cloud()
    ref = voxel_reference(pts, 0.01, colors=cols)
    assert len(ref["first"]) > 0.99 * 20000
    _check(_merge(pts, 0.01, cols), ref)


def test_more_workgroup_counts_than_scan_threads():
    # 2^20 + 5 points: ceil(N / 1024) = 1025 first-point counts for the scan's 1024 threads, so every thread owns a run
    # of 2 counts and the threads from 513 on own none; 80^3 cells for a million points: several hundred thousand voxels
    n = 2 ** 20 + 5
    rng = np.random.default_rng(8)
    pts = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    ref = voxel_reference(pts, 0.05, colors=cols)
    assert -(-n // 1024) > 1024 and 300000 < len(ref["first"]) < 512000
    _check(_merge(pts, 0.05, cols), ref)


def _line_cloud(axis):
    rng = np.random.default_rng(4)
    k = rng.permutation(4096).astype(np.float32) - 2048.0
    pts = np.full((4096, 3), 0.05, np.float32)
    pts[:, axis] = (k + np.float32(0.5)) * np.float32(0.1)
    return pts


def test_many_voxels_on_a_line_of_consecutive_cells():
    # clustered keys: 4096 consecutive cells along x (then along z: the key's low bits), one point each, shuffled
    for axis in (0, 2):
        pts = _line_cloud(axis)
        ref = voxel_reference(pts, 0.1)
        assert len(ref["first"]) == 4096
        _check(_merge(pts, 0.1), ref)


def _one_voxel_cloud():
    rng = np.random.default_rng(5)
    pts = (rng.uniform(0.0, 1.0, (5000, 3)) * 0.999 + np.array([4.0, -7.0, 1.0])).astype(np.float32)
    cols = rng.integers(0, 256, (5000, 3)).astype(np.uint8)
    return pts, cols


def test_one_voxel_5000_points():
    # maximal contention: every point adds into one accumulator row
    pts, cols = _one_voxel_cloud()
    ref = voxel_reference(pts, 1.0, colors=cols)
    assert ref["count"].tolist() == [5000]
    got = _merge(pts, 1.0, cols)
    assert got.points.shape == (1, 3) and got.count.tolist() == [5000] and got.first.tolist() == [0]
    assert (got.inverse == 0).all()
    _check(got, ref)


def _dropped_cloud():
    rng = np.random.default_rng(6)
    clean = rng.uniform(-1.0, 1.0, (3000, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (3000, 3)).astype(np.uint8)
    bad = np.sort(rng.choice(3000, 40, replace=False))
    bad[0], bad[-1] = 0, 2999                                           # the first and the last point among them
    pts = clean.copy()
    values = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(bad):
        pts[i, j % 3] = values[(j // 3) % 3]
    pts[bad[5]] = np.nan                                                # a whole row
    return pts, cols, clean, bad


def test_dropped_points():
    pts, cols, clean, bad = _dropped_cloud()
    got = _merge(pts, 0.2, cols)
    _check(got, voxel_reference(pts, 0.2, colors=cols))
    inverse = got.inverse.cpu().numpy()
    assert (inverse[bad] == -1).all() and (np.delete(inverse, bad) >= 0).all()
    assert int(got.count.sum()) == 3000 - 40
    assert not np.isin(got.first.cpu().numpy(), bad).any()
    assert torch.isfinite(got.points).all()
    # the other rows: the same cloud without the dropped points gives the same voxels
    keep = np.setdiff1d(np.arange(3000), bad)
    alone = _merge(clean[keep], 0.2, cols[keep])
    assert torch.equal(alone.points, got.points) and torch.equal(alone.colors, got.colors)
    assert torch.equal(alone.count, got.count)
    np.testing.assert_array_equal(keep[alone.first.cpu().numpy()], got.first.cpu().numpy())
    np.testing.assert_array_equal(alone.inverse.cpu().numpy(), inverse[keep])
    # nothing but dropped points: an empty cloud
    none = _merge(np.full((70, 3), np.nan, np.float32), 0.2, cols[:70])
    assert none.points.shape == (0, 3) and none.colors.shape == (0, 3) and (none.inverse == -1).all()


def test_cell_range():
    v = 0.5
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
    far = pts.copy()
    far[123, 0] = 2.0 ** 20 * v                                         # cell 2^20: one past the last
    with pytest.raises(ValueError, match="voxel_size too small for the cloud's extent"):
        _merge(far, v)
    far[123, 0] = -(2.0 ** 20) * v - 1.0                                # below cell -2^20
    with pytest.raises(ValueError, match="voxel_size too small for the cloud's extent"):
        _merge(far, v)
    far[123, 0] = np.nextafter(np.float32(2.0 ** 20 * v), np.float32(0.0))     # cell 2^20 - 1
    far[124, 1] = -(2.0 ** 20) * v                                      # cell -2^20
    ref = voxel_reference(far, v)
    assert ref["cells"][ref["inverse"][123], 0] == 2 ** 20 - 1 and ref["cells"][ref["inverse"][124], 1] == -2 ** 20
    _check(_merge(far, v), ref)
    # the range is counted from the origin: the cloud moved 2^21 cells away needs the origin moved with it
    moved = pts + np.float32(2.0 ** 20)
    with pytest.raises(ValueError, match="voxel_size too small for the cloud's extent"):
        _merge(moved, v)
    _check(_merge(moved, v, origin=(2.0 ** 20,) * 3), voxel_reference(moved, v, origin=(2.0 ** 20,) * 3))
    # a point with a non-finite coordinate, or whose t overflows, is dropped: it is not out of range
    far[125] = (np.inf, 1e30, 0.0)
    far[126] = (3e38, 0.0, 0.0)
    got = _merge(far, v)
    _check(got, voxel_reference(far, v))
    assert got.inverse[125] == -1 and got.inverse[126] == -1


def test_determinism_and_permutation():
    rng = np.random.default_rng(8)
    pts = rng.uniform(-1.0, 1.0, (6000, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (6000, 3)).astype(np.uint8)
    v = 0.15                                                            # ~2400 voxels of a few points each
    a, b = _merge(pts, v, cols), _merge(pts, v, cols)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    perm = rng.permutation(6000)
    p = _merge(pts[perm], v, cols[perm])
    _, cells, _ = cells_and_fractions(pts, v)

    def records(vc, first_original):
        rec = np.concatenate([cells[first_original], vc.count.cpu().numpy()[:, None].astype(np.int64),
                              vc.colors.cpu().numpy().astype(np.int64),
                              vc.points.cpu().numpy().view(np.uint32).astype(np.int64)], axis=1)
        return rec[np.lexsort(rec.T[::-1])]

    first_a, first_p = a.first.cpu().numpy(), p.first.cpu().numpy()
    np.testing.assert_array_equal(records(a, first_a), records(p, perm[first_p]))     # position bits included
    # first and inverse follow the permutation: a permuted point lands in the row of its own cell, and first is the
    # lowest permuted index of the row's members
    inv_a, inv_p = a.inverse.cpu().numpy(), p.inverse.cpu().numpy()
    row_of_cell = {tuple(cells[perm[f]]): r for r, f in enumerate(first_p)}
    assert len(row_of_cell) == len(first_p) == len(first_a)
    want = np.array([row_of_cell[tuple(cells[perm[j]])] for j in range(6000)])
    np.testing.assert_array_equal(inv_p, want)
    lowest = np.full(len(first_p), 6000)
    np.minimum.at(lowest, inv_p, np.arange(6000))
    np.testing.assert_array_equal(first_p, lowest)
    assert (np.diff(first_p) > 0).all()
    # the same partition: two points share a row after the permutation exactly when they did before
    np.testing.assert_array_equal(inv_a[perm][first_p][inv_p], inv_a[perm])


def test_end_to_end_after_the_fusion():
    sc = synthetic.fusion_scene(6, 96, 128, device=DEV)
    res = fuse_depthmaps(sc["depth"], sc["K"], sc["T_cam_in_world"], nearest_neighbours(6, 5), images=sc["images"])
    vc = voxel_merge(res.points, 0.02, colors=res.colors)
    n, m = res.points.shape[0], vc.points.shape[0]
    assert 1 < m < n
    assert int(vc.count.sum()) == n and vc.inverse.shape == (n,) and int(vc.inverse.min()) >= 0
    view = res.view[vc.first]
    assert view.shape == (m,) and int(view.min()) >= 0 and int(view.max()) < 6
    assert torch.equal(vc.inverse[vc.first], torch.arange(m, device=DEV))
    _check(vc, voxel_reference(res.points.cpu().numpy(), 0.02, colors=res.colors.cpu().numpy()))
