"""voxel_merge without a GPU: host-side validation (everything is rejected before any launch), the empty cloud, and the
library's voxel entries in the header, the binding and the binary."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multi_view_stereonet_amd import _native, build
from multi_view_stereonet_amd.fusion import VoxelCloud, voxel_merge, write_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvsn_voxel_workspace_bytes", "mvsn_voxel_assign", "mvsn_voxel_merge")


def _points(n=5):
    return torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)


@pytest.mark.parametrize("points, match", [
    (np.zeros((5, 3), np.float32), r"\(N,3\) tensor"),                # not a tensor
    (torch.zeros(5, 4), r"\(N,3\) tensor"),
    (torch.zeros(15), r"\(N,3\) tensor"),
    (torch.zeros(5, 3, 1), r"\(N,3\) tensor"),
    (torch.zeros(5, 3, dtype=torch.float64), "float32"),
    (torch.zeros(5, 3, dtype=torch.float16), "float32"),
])
def test_points_are_validated(points, match):
    with pytest.raises(ValueError, match=match):
        voxel_merge(points, 0.1)


@pytest.mark.parametrize("voxel_size", [0.0, -0.5, float("nan"), float("inf"), 1e-46, 1e39, 1e-39, "thick", None])
def test_voxel_size_must_be_positive_and_finite_in_float32(voxel_size):
    # 1e-46 rounds to 0 in float32, 1e39 to inf, and 1e-39 (a denormal) has no finite float32 inverse
    with pytest.raises(ValueError, match="voxel_size"):
        voxel_merge(_points(), voxel_size)


@pytest.mark.parametrize("colors, match", [
    (torch.zeros(4, 3, dtype=torch.uint8), "colors must be"),
    (torch.zeros(5, 4, dtype=torch.uint8), "colors must be"),
    (torch.zeros(5, 3, dtype=torch.float32), "uint8"),
    (torch.zeros(5, 3, dtype=torch.int32), "uint8"),
    (np.zeros((5, 3), np.uint8), "colors must be"),
    (torch.zeros(5, 3, dtype=torch.uint8, device="meta"), "colors are on meta"),      # another device than the points'
])
def test_colors_are_validated(colors, match):
    with pytest.raises(ValueError, match=match):
        voxel_merge(_points(), 0.1, colors=colors)


@pytest.mark.parametrize("origin", [(0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, float("nan"), 0.0), (float("inf"), 0, 0),
                                    "abc", 1.0])
def test_origin_is_validated(origin):
    with pytest.raises(ValueError, match="origin"):
        voxel_merge(_points(), 0.1, origin=origin)


def test_cpu_tensors_raise_after_validation():
    with pytest.raises(RuntimeError, match="HIP devices only"):
        voxel_merge(_points(), 0.1)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        voxel_merge(_points(), 0.1, colors=torch.zeros(5, 3, dtype=torch.uint8), origin=(1.0, -2.0, 0.5))
    # validation comes first: a bad argument on CPU tensors is a ValueError, not the device error
    with pytest.raises(ValueError, match="voxel_size"):
        voxel_merge(_points(), 0.0)


def test_empty_cloud_returns_empties_without_a_launch(tmp_path):
    # (no launch: this passes on a machine without a device)
    for colors in (None, torch.zeros(0, 3, dtype=torch.uint8)):
        vc = voxel_merge(torch.zeros(0, 3), 0.1, colors=colors)
        assert isinstance(vc, VoxelCloud)
        assert vc.points.shape == (0, 3) and vc.points.dtype == torch.float32
        assert vc.count.shape == (0,) and vc.count.dtype == torch.int32
        assert vc.first.shape == (0,) and vc.first.dtype == torch.int64
        assert vc.inverse.shape == (0,) and vc.inverse.dtype == torch.int64
        if colors is None:
            assert vc.colors is None
        else:
            assert vc.colors.shape == (0, 3) and vc.colors.dtype == torch.uint8
        write_ply(os.path.join(tmp_path, "empty.ply"), vc.points, vc.colors)
    # an empty cloud is still validated
    with pytest.raises(ValueError, match="voxel_size"):
        voxel_merge(torch.zeros(0, 3), -1.0)
    with pytest.raises(ValueError, match="colors must be"):
        voxel_merge(torch.zeros(0, 3), 0.1, colors=torch.zeros(1, 3, dtype=torch.uint8))


def test_voxel_cloud_fields():
    assert VoxelCloud._fields == ("points", "colors", "count", "first", "inverse")


def test_native_carries_the_voxel_signatures():
    from ctypes import c_float, c_int, c_long, c_size_t, c_void_p
    sig = _native.SIGNATURES
    assert sig["mvsn_voxel_workspace_bytes"] == (c_size_t, [c_long])
    assert sig["mvsn_voxel_assign"] == (c_int, [c_void_p, c_long] + [c_float] * 5 + [c_void_p, c_void_p, c_size_t,
                                                                                    c_void_p])
    assert sig["mvsn_voxel_merge"] == (c_int, [c_void_p, c_void_p, c_long] + [c_float] * 5 +
                                       [c_void_p, c_size_t, c_long] + [c_void_p] * 6 + [c_void_p])
    assert _native.ABI_VERSION == 7
    assert "mvsn_voxel.hip" in build.SOURCES


def test_header_declares_and_library_exports_the_voxel_entries():
    header = open(os.path.join(ROOT, "include", "mvsn_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t)\s+(mvsn_[a-z0-9_]+)\s*\(", header, flags=re.M))
    lib = ctypes.CDLL(_native.library_path())
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/mvsn_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+MVSN_VOXEL_STATUS_RANGE\s+1\b", header)
    assert re.search(r"#define\s+MVSN_VOXEL_STATUS_TABLE\s+2\b", header)
    assert re.search(r"#define\s+MVSN_ABI_VERSION\s+7\b", header)


def test_workspace_size_and_argument_checks():
    lib = _native.load()
    ws = lib.mvsn_voxel_workspace_bytes
    assert ws(0) == 0 and ws(-1) == 0 and ws(2 ** 31) == 0              # no plan outside 1 .. 2^31 - 1
    assert ws(1) > 0
    # 16 bytes per slot of a power-of-two table of >= 2 n slots, 4 bytes per point, 12 bytes per 1024 points
    n = 8_350_000
    slots = 1 << 24
    assert slots >= 2 * n > slots // 2
    assert 16 * slots + 4 * n + 12 * (n // 1024) <= ws(n) <= 16 * slots + 4 * n + 12 * (n // 1024 + 1) + 6 * 256
    assert 0 <= ws(2 ** 23) - ws(2 ** 23 - 1) <= 4 + 12 + 3 * 256      # the same table up to 2 n = a power of two ...
    assert ws(2 ** 23 + 1) > ws(2 ** 23) + 16 * 2 ** 23                # ... and twice the table one point later
    # every entry checks its arguments and says what was wrong, before any launch
    bad = lib.mvsn_voxel_assign(None, 4, 0.1, 10.0, 0.0, 0.0, 0.0, None, None, 0, None)
    assert bad == -1 and b"mvsn_voxel_assign" in lib.mvsn_last_error()
    bad = lib.mvsn_voxel_merge(None, None, 4, 0.1, 10.0, 0.0, 0.0, 0.0, None, 0, 1, None, None, None, None, None, None,
                               None)
    assert bad == -1 and b"mvsn_voxel_merge" in lib.mvsn_last_error()
    # a non-null pointer that is never dereferenced: the checks after the null check
    fake = ctypes.c_void_p(4096)
    assert lib.mvsn_voxel_assign(fake, 0, 0.1, 10.0, 0.0, 0.0, 0.0, fake, fake, 1 << 40, None) == -1
    assert lib.mvsn_voxel_assign(fake, 2 ** 31, 0.1, 10.0, 0.0, 0.0, 0.0, fake, fake, 1 << 40, None) == -2
    assert lib.mvsn_voxel_assign(fake, 4, 0.0, 10.0, 0.0, 0.0, 0.0, fake, fake, 1 << 40, None) == -1
    assert lib.mvsn_voxel_assign(fake, 4, 0.1, float("inf"), 0.0, 0.0, 0.0, fake, fake, 1 << 40, None) == -1
    assert lib.mvsn_voxel_assign(fake, 4, 0.1, 10.0, float("nan"), 0.0, 0.0, fake, fake, 1 << 40, None) == -1
    assert lib.mvsn_voxel_assign(fake, 4, 0.1, 10.0, 0.0, 0.0, 0.0, fake, fake, 16, None) == -3
    assert b"workspace" in lib.mvsn_last_error()
    assert lib.mvsn_voxel_merge(fake, None, 4, 0.1, 10.0, 0.0, 0.0, 0.0, fake, 16, 1, fake, fake, None, fake, fake,
                                fake, None) == -3
    assert lib.mvsn_voxel_merge(fake, None, 4, 0.1, 10.0, 0.0, 0.0, 0.0, fake, 1 << 40, 5, fake, fake, None, fake,
                                fake, fake, None) == -1                 # more voxels than points
    assert lib.mvsn_voxel_merge(fake, fake, 4, 0.1, 10.0, 0.0, 0.0, 0.0, fake, 1 << 40, 1, fake, fake, None, fake,
                                fake, fake, None) == -1                 # colours in without colours out
