"""cloud_nearest, radius_outlier_mask and cloud_metrics without a GPU: host-side validation (everything is rejected
before any launch), the empties, the library's cloud entries in the header, the binding and the binary, and the host
path of cloud_metrics against the numpy restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cloud_reference import cloud_metrics_reference
from multi_view_stereonet_amd import _native, build
from multi_view_stereonet_amd.fusion import CloudNeighbours, cloud_nearest, radius_outlier_mask
from multi_view_stereonet_amd.metrics import cloud_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvsn_cloud_workspace_bytes", "mvsn_cloud_index_build", "mvsn_cloud_nearest")


def _points(n=5):
    return torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)


BAD_CLOUDS = [
    (np.zeros((5, 3), np.float32), r"\(N,3\) tensor"),                # not a tensor
    (torch.zeros(5, 4), r"\(N,3\) tensor"),
    (torch.zeros(15), r"\(N,3\) tensor"),
    (torch.zeros(5, 3, 1), r"\(N,3\) tensor"),
    (torch.zeros(5, 3, dtype=torch.float64), "float32"),
    (torch.zeros(5, 3, dtype=torch.float16), "float32"),
]
# 1e-46 rounds to 0 in float32, 1e39 to inf; 1e-39 (a denormal) has no finite float32 inverse; the square of 1e-23 is 0
# and the square of 1e20 is inf in float32
BAD_RADII = [0.0, -0.5, float("nan"), float("inf"), 1e-46, 1e39, 1e-39, 1e-23, 1e20, "far", None]


@pytest.mark.parametrize("cloud, match", BAD_CLOUDS)
def test_clouds_are_validated(cloud, match):
    with pytest.raises(ValueError, match="query must be"):
        cloud_nearest(cloud, _points(), 0.1)
    with pytest.raises(ValueError, match="target must be"):
        cloud_nearest(_points(), cloud, 0.1)
    with pytest.raises(ValueError, match="points must be"):
        radius_outlier_mask(cloud, 0.1, 2)
    with pytest.raises(ValueError, match="pred must be"):
        cloud_metrics(cloud, _points(), 0.1)
    with pytest.raises(ValueError, match="truth must be"):
        cloud_metrics(_points(), cloud, 0.1)


def test_clouds_on_two_devices():
    with pytest.raises(ValueError, match="query is on cpu, target on meta"):
        cloud_nearest(_points(), torch.zeros(5, 3, device="meta"), 0.1)
    with pytest.raises(ValueError, match="pred is on meta, truth on cpu"):
        cloud_metrics(torch.zeros(5, 3, device="meta"), _points(), 0.1)


@pytest.mark.parametrize("max_dist", BAD_RADII)
def test_max_dist_must_be_positive_and_finite_in_float32_with_its_inverse_and_square(max_dist):
    with pytest.raises(ValueError, match="max_dist"):
        cloud_nearest(_points(), _points(), max_dist)
    with pytest.raises(ValueError, match="radius"):
        radius_outlier_mask(_points(), max_dist, 1)
    with pytest.raises(ValueError, match="threshold"):
        cloud_metrics(_points(), _points(), max_dist)
    if max_dist is not None:                                            # (None: the cap defaults to the threshold)
        with pytest.raises(ValueError, match="max_dist"):
            cloud_metrics(_points(), _points(), 0.1, max_dist)


def test_min_neighbours_must_be_an_integer():
    for bad in (1.5, "two", None, True):
        with pytest.raises(ValueError, match="min_neighbours"):
            radius_outlier_mask(_points(), 0.1, bad)


def test_cpu_tensors_raise_after_validation():
    with pytest.raises(RuntimeError, match="HIP devices only"):
        cloud_nearest(_points(), _points(7), 0.1)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        radius_outlier_mask(_points(), 0.1, 1)
    # validation comes first: a bad argument on CPU tensors is a ValueError, not the device error
    with pytest.raises(ValueError, match="max_dist"):
        cloud_nearest(_points(), _points(), 0.0)
    with pytest.raises(ValueError, match="target must be"):
        cloud_nearest(_points(), torch.zeros(5, 2), 0.1)


def test_empties_without_a_launch():
    # (no launch: this passes on a machine without a device)
    nn = cloud_nearest(torch.zeros(0, 3), _points(), 0.1)
    assert isinstance(nn, CloudNeighbours) and CloudNeighbours._fields == ("dist2", "index", "within")
    assert nn.dist2.shape == (0,) and nn.dist2.dtype == torch.float32
    assert nn.index.shape == (0,) and nn.index.dtype == torch.int64
    assert nn.within.shape == (0,) and nn.within.dtype == torch.int32
    nn = cloud_nearest(_points(4), torch.zeros(0, 3), 0.1)
    assert nn.dist2.tolist() == [float("inf")] * 4 and nn.dist2.dtype == torch.float32
    assert nn.index.tolist() == [-1] * 4 and nn.index.dtype == torch.int64
    assert nn.within.tolist() == [0] * 4 and nn.within.dtype == torch.int32
    nn = cloud_nearest(torch.zeros(0, 3), torch.zeros(0, 3), 0.1)
    assert nn.dist2.shape == nn.index.shape == nn.within.shape == (0,)
    mask = radius_outlier_mask(torch.zeros(0, 3), 0.1, 3)
    assert mask.shape == (0,) and mask.dtype == torch.bool
    # the empties are still validated
    with pytest.raises(ValueError, match="max_dist"):
        cloud_nearest(torch.zeros(0, 3), _points(), -1.0)
    with pytest.raises(ValueError, match="target must be"):
        cloud_nearest(torch.zeros(0, 3), torch.zeros(0, 4), 0.1)


def test_native_carries_the_cloud_signatures():
    from ctypes import c_float, c_int, c_long, c_size_t, c_void_p
    sig = _native.SIGNATURES
    assert sig["mvsn_cloud_workspace_bytes"] == (c_size_t, [c_long])
    assert sig["mvsn_cloud_index_build"] == (c_int, [c_void_p, c_long, c_float, c_float, c_void_p, c_void_p, c_size_t,
                                                     c_void_p])
    assert sig["mvsn_cloud_nearest"] == (c_int, [c_void_p, c_long, c_float, c_float, c_void_p, c_size_t, c_long,
                                                 c_void_p, c_void_p, c_void_p, c_void_p])
    assert _native.ABI_VERSION == 7
    assert "mvsn_cloud.hip" in build.SOURCES and "mvsn_voxel.hip" in build.SOURCES
    assert "mvsn_voxel.h" in build.HEADERS                              # the shared cell / key / hash: part of the digest


def test_header_declares_and_library_exports_the_cloud_entries():
    header = open(os.path.join(ROOT, "include", "mvsn_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t)\s+(mvsn_[a-z0-9_]+)\s*\(", header, flags=re.M))
    lib = ctypes.CDLL(_native.library_path())
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/mvsn_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+MVSN_CLOUD_STATUS_RANGE\s+1\b", header)
    assert re.search(r"#define\s+MVSN_CLOUD_STATUS_TABLE\s+2\b", header)
    assert re.search(r"#define\s+MVSN_ABI_VERSION\s+7\b", header)


def test_workspace_size_and_argument_checks():
    lib = _native.load()
    ws = lib.mvsn_cloud_workspace_bytes
    assert ws(0) == 0 and ws(-1) == 0 and ws(2 ** 31) == 0              # no plan outside 1 .. 2^31 - 1
    assert ws(1) > 0 and ws(1) % 256 == 0
    # 20 bytes per slot of a power-of-two table of >= 2 n slots (key, population, start, cursor), 20 bytes per point
    # (slot, record), 12 bytes per 1024 slots (count, offset); eight 256-byte aligned sections
    n = 8_350_000
    slots = 1 << 24
    assert slots >= 2 * n > slots // 2
    exact = 20 * slots + 20 * n + 12 * (slots // 1024)
    assert exact <= ws(n) <= exact + 8 * 256
    assert 0 <= ws(2 ** 23) - ws(2 ** 23 - 1) <= 20 + 2 * 256          # the same table up to 2 n = a power of two ...
    assert ws(2 ** 23 + 1) > ws(2 ** 23) + 20 * 2 ** 23                # ... and twice the table one point later
    # every entry checks its arguments and says what was wrong, before any launch
    bad = lib.mvsn_cloud_index_build(None, 4, 0.1, 10.0, None, None, 0, None)
    assert bad == -1 and b"mvsn_cloud_index_build" in lib.mvsn_last_error()
    bad = lib.mvsn_cloud_nearest(None, 4, 10.0, 0.01, None, 0, 4, None, None, None, None)
    assert bad == -1 and b"mvsn_cloud_nearest" in lib.mvsn_last_error()
    # a non-null pointer that is never dereferenced: the checks after the null check
    fake = ctypes.c_void_p(4096)
    big = 1 << 40
    assert lib.mvsn_cloud_index_build(fake, 0, 0.1, 10.0, fake, fake, big, None) == -1
    assert lib.mvsn_cloud_index_build(fake, 2 ** 31, 0.1, 10.0, fake, fake, big, None) == -2
    assert b"mvsn_cloud_index_build" in lib.mvsn_last_error()
    assert lib.mvsn_cloud_index_build(fake, 4, 0.0, 10.0, fake, fake, big, None) == -1
    assert lib.mvsn_cloud_index_build(fake, 4, 0.1, float("inf"), fake, fake, big, None) == -1
    assert lib.mvsn_cloud_index_build(fake, 4, float("nan"), 10.0, fake, fake, big, None) == -1
    assert lib.mvsn_cloud_index_build(fake, 4, 0.1, 10.0, fake, fake, 16, None) == -3
    assert b"workspace" in lib.mvsn_last_error()
    assert lib.mvsn_cloud_index_build(fake, 4, 0.1, 10.0, fake, ctypes.c_void_p(4100), big, None) == -1   # alignment
    assert lib.mvsn_cloud_nearest(fake, 0, 10.0, 0.01, fake, big, 4, fake, fake, fake, None) == -1
    assert lib.mvsn_cloud_nearest(fake, 4, 10.0, 0.01, fake, big, 0, fake, fake, fake, None) == -1
    assert lib.mvsn_cloud_nearest(fake, 2 ** 31, 10.0, 0.01, fake, big, 4, fake, fake, fake, None) == -2
    assert lib.mvsn_cloud_nearest(fake, 4, 10.0, 0.01, fake, big, 2 ** 31, fake, fake, fake, None) == -2
    assert b"mvsn_cloud_nearest" in lib.mvsn_last_error()
    assert lib.mvsn_cloud_nearest(fake, 4, 0.0, 0.01, fake, big, 4, fake, fake, fake, None) == -1
    assert lib.mvsn_cloud_nearest(fake, 4, 10.0, float("nan"), fake, big, 4, fake, fake, fake, None) == -1
    assert lib.mvsn_cloud_nearest(fake, 4, 10.0, 0.01, fake, big, 4, fake, None, fake, None) == -1
    assert lib.mvsn_cloud_nearest(fake, 4, 10.0, 0.01, fake, 16, 4, fake, fake, fake, None) == -3


# ---- cloud_metrics on the host -------------------------------------------------------------------------------------
def test_cloud_metrics_arguments():
    p = _points()
    with pytest.raises(ValueError, match="must not be below threshold"):
        cloud_metrics(p, p, 0.5, 0.25)
    for cloud in (torch.zeros(0, 3), torch.full((4, 3), float("nan")), torch.tensor([[0.0, float("inf"), 0.0]])):
        with pytest.raises(ValueError, match="no finite point"):
            cloud_metrics(cloud, p, 0.5)
        with pytest.raises(ValueError, match="no finite point"):
            cloud_metrics(p, cloud, 0.5)
    with pytest.raises(ValueError, match="max_dist too small for the target's extent"):
        cloud_metrics(p, p * 1e6, 0.5)


def _compare(got, ref):
    assert set(got) == {"accuracy", "completeness", "precision", "recall", "fscore", "n_pred", "n_truth"}
    assert got["n_pred"] == ref["n_pred"] and got["n_truth"] == ref["n_truth"]
    assert got["precision"] == ref["precision"] and got["recall"] == ref["recall"] and got["fscore"] == ref["fscore"]
    for key in ("accuracy", "completeness"):
        assert abs(got[key] - ref[key]) <= 1e-12 * ref[key], key


def test_cloud_metrics_on_the_host_against_numpy():
    # the line of tests/test_cloud_reference_cpu.py, whose numbers are worked out there
    truth = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    pred = np.array([[0.125, 0, 0], [1, 0, 0], [np.nan, 0, 0], [2.5, 0, 0], [10, 0, 0]], np.float32)
    got = cloud_metrics(torch.from_numpy(pred), torch.from_numpy(truth), 0.25, 1.0)
    assert got == {"accuracy": 1.625 / 4, "completeness": 0.625 / 3, "precision": 0.5, "recall": 2 / 3,
                   "fscore": got["fscore"], "n_pred": 4, "n_truth": 3} and abs(got["fscore"] - 4 / 7) < 1e-15
    # two noisy samplings of a sheet, with holes, non-finite rows and more rows than one chunk of the brute force
    rng = np.random.default_rng(31)
    truth = np.concatenate([rng.uniform(-1, 1, (3000, 2)), np.zeros((3000, 1))], 1).astype(np.float32)
    pred = (truth[rng.permutation(3000)[:2500]] + rng.normal(0, 0.02, (2500, 3))).astype(np.float32)
    pred[7], truth[11], truth[12, 2] = np.nan, np.inf, -np.inf
    pred[pred[:, 0] > 0.7, 2] += 1.0                                    # a part of pred far off the sheet
    for threshold, max_dist in ((0.03, None), (0.03, 0.2), (0.01, 0.01)):
        got = cloud_metrics(torch.from_numpy(pred), torch.from_numpy(truth), threshold, max_dist)
        ref = cloud_metrics_reference(pred, truth, threshold, max_dist)
        assert 0 < ref["precision"] < 1 and 0 < ref["recall"] < 1 and ref["n_pred"] == 2499 and ref["n_truth"] == 2998
        _compare(got, ref)
