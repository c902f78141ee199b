"""depth_normals, point_normals, voxel_normals and write_ply(normals=) without a GPU: the three library entries in the
header, the binding and the binary; their argument checks (nothing is launched); the host-side validation of the Python
functions (every ValueError before the device error); empty inputs; the PLY layout."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multi_view_stereonet_amd import _native, build
from multi_view_stereonet_amd.fusion import (FusionResult, VoxelCloud, depth_normals, point_normals, voxel_normals,
                                             write_ply)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvsn_depth_normals", "mvsn_normals_gather", "mvsn_voxel_normals")
FAKE = ctypes.c_void_p(4096)            # a non-null pointer that is never dereferenced: the checks after the null check
INF, NAN = float("inf"), float("nan")


def test_native_carries_the_normals_signatures():
    from ctypes import c_float, c_int, c_long, c_void_p
    sig = _native.SIGNATURES
    assert sig["mvsn_depth_normals"] == (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_float, c_void_p, c_void_p])
    assert sig["mvsn_normals_gather"] == (c_int, [c_void_p] * 3 + [c_int, c_long, c_long, c_void_p, c_void_p])
    assert sig["mvsn_voxel_normals"] == (c_int, [c_void_p, c_void_p, c_long, c_long, c_void_p, c_void_p, c_void_p])
    assert _native.ABI_VERSION == 7
    assert "mvsn_normals.hip" in build.SOURCES


def test_header_declares_and_library_exports_the_normals_entries():
    header = open(os.path.join(ROOT, "include", "mvsn_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t)\s+(mvsn_[a-z0-9_]+)\s*\(", header, flags=re.M))
    lib = ctypes.CDLL(_native.library_path())
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/mvsn_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+MVSN_ABI_VERSION\s+7\b", header)
    assert _native.load().mvsn_abi_version() == 7
    source = open(os.path.join(ROOT, "multi_view_stereonet_amd", "csrc", "mvsn_normals.hip")).read()
    assert re.search(r"^#pragma clang fp contract\(off\)", source, flags=re.M)


def _refused(rc, lib, entry, code=-1):
    assert rc == code, rc
    assert entry.encode() in lib.mvsn_last_error(), lib.mvsn_last_error()


def test_depth_normals_entry_checks_its_arguments():
    lib = _native.load()
    fn = lib.mvsn_depth_normals
    _refused(fn(None, None, None, None, 1, 4, 4, 0.05, None, None), lib, "mvsn_depth_normals")
    _refused(fn(None, None, FAKE, None, 1, 4, 4, 0.05, FAKE, None), lib, "mvsn_depth_normals")      # no depth
    _refused(fn(FAKE, None, None, None, 1, 4, 4, 0.05, FAKE, None), lib, "mvsn_depth_normals")      # no K
    _refused(fn(FAKE, None, FAKE, None, 1, 4, 4, 0.05, None, None), lib, "mvsn_depth_normals")      # no output
    for V, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4)):
        _refused(fn(FAKE, None, FAKE, None, V, H, W, 0.05, FAKE, None), lib, "mvsn_depth_normals")
    for step in (-0.01, -INF, NAN):
        _refused(fn(FAKE, None, FAKE, None, 1, 4, 4, step, FAKE, None), lib, "mvsn_depth_normals")
        assert b"max_rel_step" in lib.mvsn_last_error()
    _refused(fn(FAKE, None, FAKE, None, 65536, 4, 4, 0.05, FAKE, None), lib, "mvsn_depth_normals", -2)
    _refused(fn(FAKE, None, FAKE, None, 1, 65536, 32768, 0.05, FAKE, None), lib, "mvsn_depth_normals", -2)


def test_normals_gather_entry_checks_its_arguments():
    lib = _native.load()
    fn = lib.mvsn_normals_gather
    _refused(fn(None, None, None, 1, 16, 4, None, None), lib, "mvsn_normals_gather")
    _refused(fn(FAKE, FAKE, None, 1, 16, 4, FAKE, None), lib, "mvsn_normals_gather")
    _refused(fn(FAKE, FAKE, FAKE, 1, 16, 4, None, None), lib, "mvsn_normals_gather")
    for V, HW, M in ((0, 16, 4), (1, 0, 4), (1, 16, -1), (1, 2 ** 31, 4)):
        _refused(fn(FAKE, FAKE, FAKE, V, HW, M, FAKE, None), lib, "mvsn_normals_gather")
    assert fn(None, None, None, 1, 16, 0, None, None) == 0             # no points: no launch, nothing is touched


def test_voxel_normals_entry_checks_its_arguments():
    lib = _native.load()
    fn = lib.mvsn_voxel_normals
    _refused(fn(None, None, 4, 2, None, None, None), lib, "mvsn_voxel_normals")
    _refused(fn(FAKE, None, 4, 2, FAKE, FAKE, None), lib, "mvsn_voxel_normals")
    _refused(fn(FAKE, FAKE, 4, 2, None, FAKE, None), lib, "mvsn_voxel_normals")
    _refused(fn(FAKE, FAKE, 4, 2, FAKE, None, None), lib, "mvsn_voxel_normals")
    _refused(fn(FAKE, FAKE, -1, 2, FAKE, FAKE, None), lib, "mvsn_voxel_normals")
    _refused(fn(FAKE, FAKE, 4, -2, FAKE, FAKE, None), lib, "mvsn_voxel_normals")
    _refused(fn(FAKE, FAKE, 4, 2, ctypes.c_void_p(4100), FAKE, None), lib, "mvsn_voxel_normals")   # accumulators' alignment
    _refused(fn(FAKE, FAKE, 2 ** 31, 2, FAKE, FAKE, None), lib, "mvsn_voxel_normals", -2)
    _refused(fn(FAKE, FAKE, 4, 2 ** 31, FAKE, FAKE, None), lib, "mvsn_voxel_normals", -2)
    assert fn(None, None, 4, 0, None, None, None) == 0                  # no rows: no launch


# ---- the Python functions: every ValueError on CPU tensors, before the device error --------------------------------
def _maps(V=2, H=5, W=7):
    depth = torch.ones(V, 1, H, W)
    K = torch.eye(4).repeat(V, 1, 1)
    return depth, K


@pytest.mark.parametrize("depth, match", [
    (np.ones((2, 1, 5, 7), np.float32), r"\(V,1,H,W\) tensor"),
    (torch.ones(2, 5, 7), r"\(V,1,H,W\) tensor"),
    (torch.ones(2, 3, 5, 7), r"\(V,1,H,W\) tensor"),
    (torch.ones(0, 1, 5, 7), "at least one view"),
    (torch.ones(2, 1, 0, 7), "at least one view"),
    (torch.ones(2, 1, 5, 7, dtype=torch.float64), "float32"),
    (torch.ones(2, 1, 5, 7, dtype=torch.float16), "float32"),
])
def test_depth_is_validated(depth, match):
    with pytest.raises(ValueError, match=match):
        depth_normals(depth, torch.eye(4).repeat(2, 1, 1))


def test_depth_normals_arguments_are_validated_before_the_device():
    depth, K = _maps()
    for bad in (None, K.numpy(), K[:1], K[:, :3, :3], torch.eye(4)):
        with pytest.raises(ValueError, match="K must be"):
            depth_normals(depth, bad)
    with pytest.raises(ValueError, match="K is on meta"):
        depth_normals(depth, K.to("meta"))
    for bad in (K.numpy(), K[:1], K[:, :3]):
        with pytest.raises(ValueError, match="T_cam_in_world must be"):
            depth_normals(depth, K, T_cam_in_world=bad)
    with pytest.raises(ValueError, match="T_cam_in_world is on meta"):
        depth_normals(depth, K, T_cam_in_world=K.to("meta"))
    for bad, match in ((torch.ones(2, 1, 5, 6, dtype=torch.bool), "valid must be"),
                       (torch.ones(2, 5, 7, dtype=torch.bool), "valid must be"),
                       (torch.ones(2, 1, 5, 7), "valid must be torch.bool or torch.uint8"),
                       (np.ones((2, 1, 5, 7), bool), "valid must be a tensor"),
                       (torch.ones(2, 1, 5, 7, dtype=torch.bool, device="meta"), "valid is on meta")):
        with pytest.raises(ValueError, match=match):
            depth_normals(depth, K, valid=bad)
    for bad in (-0.01, NAN, -INF, "wide", None):
        with pytest.raises(ValueError, match="max_rel_step"):
            depth_normals(depth, K, max_rel_step=bad)
    # ... and only then the device: good arguments on CPU tensors
    for kwargs in ({}, {"max_rel_step": INF}, {"max_rel_step": 0}, {"T_cam_in_world": K},
                   {"valid": torch.ones(2, 1, 5, 7, dtype=torch.uint8)}):
        with pytest.raises(RuntimeError, match="HIP devices only"):
            depth_normals(depth, K, **kwargs)


def _result(M=4, V=2, H=5, W=7):
    return FusionResult(torch.zeros(M, 3), None, torch.zeros(M, dtype=torch.int32), torch.zeros(M, dtype=torch.int32),
                        torch.zeros(V, 1, H, W), torch.zeros(V, 1, H, W, dtype=torch.uint8))


def test_point_normals_arguments_are_validated_before_the_device():
    res = _result()
    for bad, match in ((np.zeros((2, 3, 5, 7), np.float32), r"\(V,3,H,W\) tensor"),
                       (torch.zeros(2, 1, 5, 7), r"\(V,3,H,W\) tensor"),
                       (torch.zeros(2, 5, 7, 3), r"\(V,3,H,W\) tensor"),
                       (torch.zeros(2, 3, 5, 7, dtype=torch.float64), "float32"),
                       (torch.zeros(2, 3, 5, 8), "the fusion ran on"),
                       (torch.zeros(2, 3, 5, 7, device="meta"), "normals are on meta")):
        with pytest.raises(ValueError, match=match):
            point_normals(res, bad)
    with pytest.raises(ValueError, match="reference views"):
        point_normals(res, torch.zeros(2, 3, 5, 7), ref_views=[1, 0, 2])
    with pytest.raises(ValueError, match="integers"):
        point_normals(res, torch.zeros(2, 3, 5, 7), ref_views=[0.5, 1.0])
    with pytest.raises(RuntimeError, match="HIP devices only"):
        point_normals(res, torch.zeros(2, 3, 5, 7))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        point_normals(res, torch.zeros(2, 3, 5, 7), ref_views=[1, 0])


def _cloud(N=6, M=3):
    return VoxelCloud(torch.zeros(M, 3), None, torch.ones(M, dtype=torch.int32), torch.zeros(M, dtype=torch.int64),
                      torch.zeros(N, dtype=torch.int64))


def test_voxel_normals_arguments_are_validated_before_the_device():
    vc = _cloud()
    for bad, match in ((np.zeros((6, 3), np.float32), r"\(6,3\) tensor"),
                       (torch.zeros(5, 3), r"\(6,3\) tensor"),
                       (torch.zeros(6, 4), r"\(6,3\) tensor"),
                       (torch.zeros(18), r"\(6,3\) tensor"),
                       (torch.zeros(6, 3, dtype=torch.float64), "float32"),
                       (torch.zeros(6, 3, device="meta"), "normals are on meta")):
        with pytest.raises(ValueError, match=match):
            voxel_normals(vc, bad)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        voxel_normals(vc, torch.zeros(6, 3))


def test_empty_inputs_return_empties_without_a_launch():
    # (no launch: this passes on a machine without a device)
    out = point_normals(_result(M=0), torch.zeros(2, 3, 5, 7))
    assert out.shape == (0, 3) and out.dtype == torch.float32
    out = point_normals(_result(M=0), torch.zeros(1, 3, 5, 7), ref_views=[1])
    assert out.shape == (0, 3) and out.dtype == torch.float32
    with pytest.raises(ValueError, match="float32"):                    # an empty cloud is still validated
        point_normals(_result(M=0), torch.zeros(2, 3, 5, 7, dtype=torch.float64))
    out = voxel_normals(_cloud(N=0, M=0), torch.zeros(0, 3))
    assert out.shape == (0, 3) and out.dtype == torch.float32
    out = voxel_normals(_cloud(N=5, M=0), torch.zeros(5, 3))            # every point dropped by the merge
    assert out.shape == (0, 3) and out.dtype == torch.float32
    out = voxel_normals(_cloud(N=0, M=2), torch.zeros(0, 3))
    assert out.shape == (2, 3) and out.dtype == torch.float32 and (out == 0).all()
    with pytest.raises(ValueError, match=r"\(0,3\) tensor"):
        voxel_normals(_cloud(N=0, M=0), torch.zeros(1, 3))


# ---- write_ply ---------------------------------------------------------------------------------------------------
def _parent_ply_bytes(points, colors=None, confidence=None):
    """The file write_ply wrote before it knew normals, restated: header and records."""
    n = points.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = "property float x\nproperty float y\nproperty float z\n"
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    if confidence is not None:
        fields += [("confidence", "<f4")]
        props += "property float confidence\n"
    rec = np.empty(n, dtype=fields)
    for i, k in enumerate("xyz"):
        rec[k] = points[:, i]
    if colors is not None:
        for i, k in enumerate(("red", "green", "blue")):
            rec[k] = colors[:, i]
    if confidence is not None:
        rec["confidence"] = confidence
    return f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\n{props}end_header\n".encode("ascii") + rec.tobytes()


def _ply_data():
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(11, 3)).astype(np.float32)
    nrm = rng.normal(size=(11, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    col = rng.integers(0, 256, (11, 3)).astype(np.uint8)
    conf = rng.uniform(size=11).astype(np.float32)
    return pts, nrm, col, conf


def test_write_ply_without_normals_is_the_parents_file(tmp_path):
    pts, _, col, conf = _ply_data()
    for colors, confidence in ((None, None), (col, None), (None, conf), (col, conf)):
        path = os.path.join(tmp_path, "plain.ply")
        write_ply(path, torch.from_numpy(pts), None if colors is None else torch.from_numpy(colors),
                  None if confidence is None else torch.from_numpy(confidence))
        assert open(path, "rb").read() == _parent_ply_bytes(pts, colors, confidence)
        write_ply(path, pts, colors, confidence=confidence, normals=None)
        assert open(path, "rb").read() == _parent_ply_bytes(pts, colors, confidence)


@pytest.mark.parametrize("with_colors, with_confidence", [(False, False), (True, False), (True, True), (False, True)])
def test_write_ply_with_normals_round_trips(tmp_path, with_colors, with_confidence):
    pts, nrm, col, conf = _ply_data()
    path = os.path.join(tmp_path, "oriented.ply")
    write_ply(path, torch.from_numpy(pts), torch.from_numpy(col) if with_colors else None,
              confidence=torch.from_numpy(conf) if with_confidence else None, normals=torch.from_numpy(nrm))
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 11"]
    want = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    want += [("red", "u1"), ("green", "u1"), ("blue", "u1")] if with_colors else []
    want += [("confidence", "<f4")] if with_confidence else []
    assert lines[3:] == [f"property {'float' if t == '<f4' else 'uchar'} {k}" for k, t in want]
    rec = np.frombuffer(body, dtype=want)
    assert rec.shape == (11,)
    np.testing.assert_array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), pts)
    np.testing.assert_array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], 1), nrm)
    if with_colors:
        np.testing.assert_array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), col)
    if with_confidence:
        np.testing.assert_array_equal(rec["confidence"], conf)


def test_write_ply_rejects_wrong_shaped_normals(tmp_path):
    pts, nrm, _, _ = _ply_data()
    path = os.path.join(tmp_path, "bad.ply")
    for bad in (nrm[:10], nrm[:, :2], nrm.reshape(-1), nrm.T, torch.zeros(11, 3, 1)):
        with pytest.raises(ValueError, match="normals must be"):
            write_ply(path, pts, normals=bad)
    write_ply(path, np.zeros((0, 3), np.float32), normals=np.zeros((0, 3), np.float32))     # an empty oriented cloud
    assert open(path, "rb").read().endswith(b"property float nz\nend_header\n")
