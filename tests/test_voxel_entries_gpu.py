"""The voxel entries of the C ABI (csrc/mvsn_voxel.hip: mvsn_voxel_assign, mvsn_voxel_merge) with their inputs in
poisoned buffers and the workspace (the hash table, the slots, the counts), `result`, the 64-byte accumulator rows and
every output between guard bands, on the clouds of tests/test_voxel_gpu.py: the same bits under both poisons, from the
Python entry, and from a workspace and accumulators that a merge of another cloud left dirty."""
import functools

import numpy as np
import pytest
import torch

from guarded_alloc import POISON_FINITE, POISON_NAN, Guard, bits_equal
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd.fusion import VoxelCloud, voxel_merge
from test_voxel_gpu import _check, _dropped_cloud, _hand_case, _line_cloud, _one_voxel_cloud, _uniform_cloud
from voxel_reference import voxel_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _clouds():
    """{name: (points, colors or None, voxel_size, origin)}"""
    hand, hand_cols, v, origin = _hand_case()
    dropped, dropped_cols, _, _ = _dropped_cloud()
    one, one_cols = _one_voxel_cloud()
    uniform, uniform_cols = _uniform_cloud()
    zero = (0.0, 0.0, 0.0)
    return {"hand": (hand, hand_cols, v, origin), "hand_no_colours": (hand, None, v, origin),
            "dropped": (dropped, dropped_cols, 0.2, zero), "all_dropped": (np.full((70, 3), np.nan, np.float32),
                                                                          dropped_cols[:70], 0.2, zero),
            "one_voxel": (one, one_cols, 1.0, zero), "line_x": (_line_cloud(0), None, 0.1, zero),
            "line_z": (_line_cloud(2), None, 0.1, zero), "uniform": (uniform, uniform_cols, 0.01, zero),
            "single": (np.array([[-1.3, 0.7, 2.9]], np.float32), np.array([[7, 0, 255]], np.uint8), 0.1, zero)}


CLOUDS = _clouds()


def _merge_into(guard, lib, ws, ws_bytes, accum_rows, pts, cols, voxel, origin):
    """assign + merge of one cloud into `ws` (and accumulators of at least `accum_rows` rows, carved on first use)."""
    N = pts.shape[0]
    p = guard.poisoned(torch.from_numpy(pts).to(DEV))
    c = guard.poisoned(torch.from_numpy(cols).to(DEV)) if cols is not None else None
    v = np.float32(voxel)
    o = np.asarray(origin, np.float32)
    scalars = (float(v), float(np.float32(1) / v), float(o[0]), float(o[1]), float(o[2]))
    head = guard.empty((2,), torch.int64, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_voxel_assign(_native.ptr(p), N, *scalars, _native.ptr(head), _native.ptr(ws), ws_bytes, st),
                      "mvsn_voxel_assign")
        m, status = head.tolist()
        assert status == 0 and 0 <= m <= N, (m, status)
        out = VoxelCloud(guard.empty((m, 3), torch.float32, DEV),
                         guard.empty((m, 3), torch.uint8, DEV) if cols is not None else None,
                         guard.empty((m,), torch.int32, DEV), guard.empty((m,), torch.int64, DEV),
                         guard.empty((N,), torch.int64, DEV))
        if m == 0:                         # every point dropped: no launch, the caller fills `inverse` (as voxel_merge does)
            out.inverse.fill_(-1)
            return out
        accum = accum_rows(m)
        _native.check(lib.mvsn_voxel_merge(_native.ptr(p), _native.ptr(c), N, *scalars, _native.ptr(ws), ws_bytes, m,
                                           _native.ptr(accum), _native.ptr(out.points), _native.ptr(out.colors),
                                           _native.ptr(out.count), _native.ptr(out.first), _native.ptr(out.inverse), st),
                      "mvsn_voxel_merge")
    return out


def device_merge(name, fill=POISON_NAN, after=None):
    """The cloud `name` through mvsn_voxel_assign and mvsn_voxel_merge between guard bands.  `after`: the name of a
    cloud that is merged first into the same workspace and the same accumulators, which it leaves dirty."""
    lib = _native.load()
    guard = Guard(_alloc, fill)
    order = ([after] if after else []) + [name]
    ws_bytes = max(lib.mvsn_voxel_workspace_bytes(CLOUDS[k][0].shape[0]) for k in order)
    assert ws_bytes > 0
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    rows = max(CLOUDS[k][0].shape[0] for k in order)
    held = []

    def accum_rows(m):                     # 64 bytes per output row, one buffer for both merges
        if not held:
            held.append(guard.empty((rows, 8), torch.int64, DEV))
        return held[0]
    for k in order:
        out = _merge_into(guard, lib, ws, ws_bytes, accum_rows, *CLOUDS[k])
    torch.cuda.synchronize()
    guard.check()
    return out


def _same(a, b):
    for name, x, y in zip(VoxelCloud._fields, a, b):
        assert (x is None and y is None) or bits_equal(x, y), name


@functools.lru_cache(maxsize=None)
def _reference(name):
    pts, cols, v, origin = CLOUDS[name]
    return voxel_reference(pts, v, colors=cols, origin=origin)


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_voxel_entries_between_bands(name):
    pts, cols, v, origin = CLOUDS[name]
    got = device_merge(name, POISON_NAN)
    _same(got, device_merge(name, POISON_FINITE))
    _same(got, voxel_merge(torch.from_numpy(pts).to(DEV), v, origin=origin,
                           colors=None if cols is None else torch.from_numpy(cols).to(DEV)))
    ref = _reference(name)
    if name == "all_dropped":
        assert got.points.shape == (0, 3) and len(ref["first"]) == 0 and (got.inverse == -1).all()
    else:
        _check(got, ref)


# (the cloud, the one merged before it): a fuller table before a sparse one, one row before thousands and the reverse,
# colours before none, a cloud that launches no merge before one that does
DIRTY = [("hand", "uniform"), ("uniform", "one_voxel"), ("one_voxel", "uniform"), ("line_x", "hand"),
         ("dropped", "all_dropped"), ("all_dropped", "dropped"), ("single", "line_z"), ("hand_no_colours", "hand")]


@pytest.mark.parametrize("name,after", DIRTY, ids=[f"{a}_after_{b}" for a, b in DIRTY])
def test_a_dirty_workspace_gives_the_same_bytes(name, after):
    fresh = device_merge(name, POISON_FINITE)
    _same(fresh, device_merge(name, POISON_FINITE, after=after))
    _same(fresh, device_merge(name, POISON_NAN, after=after))
