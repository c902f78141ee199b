"""CPU-side checks of the confidence feature's boundary: the four C entries validate before any device work, the engine
option, fuse_depthmaps' argument checks (all before the device check), write_ply's extra property.  No GPU."""
import numpy as np
import pytest
import torch

from multi_view_stereonet_amd import MultiViewStereoNet, _native
from multi_view_stereonet_amd.fusion import fuse_depthmaps, write_ply
from multi_view_stereonet_amd.multi_view_stereonet import EngineOptions

ONE = 0x1000          # a non-null address that is never dereferenced: every call below fails its size checks first


def _fails(rc, lib, word):
    assert rc == -1 and word in lib.mvsn_last_error(), (rc, lib.mvsn_last_error())


def test_new_entries_validate_before_any_device_work():
    lib = _native.load()
    _fails(lib.mvsn_soft_argmin_confidence(None, None, 1, 4, 16, None, None, None), lib, b"null")
    _fails(lib.mvsn_soft_argmin_confidence(ONE, ONE, 1, 4, 16, ONE, None, None), lib, b"null")
    for n, D, P in ((0, 4, 16), (1, 0, 16), (1, 4, 0), (65536, 4, 16)):
        _fails(lib.mvsn_soft_argmin_confidence(ONE, ONE, n, D, P, ONE, ONE, None), lib, b"bad sizes")
    _fails(lib.mvsn_confidence_fuse_sources(None, 2, 1, 16, None, None), lib, b"null")
    for S, B, P in ((0, 1, 16), (2, 0, 16), (2, 1, 0), (2, 65536, 16)):
        _fails(lib.mvsn_confidence_fuse_sources(ONE, S, B, P, ONE, None), lib, b"bad sizes")
    _fails(lib.mvsn_confidence_mask(None, None, 16, 0.5, None, None), lib, b"null")
    _fails(lib.mvsn_confidence_mask(ONE, None, 0, 0.5, ONE, None), lib, b"bad sizes")
    _fails(lib.mvsn_confidence_mask(ONE, None, 16, float("nan"), ONE, None), lib, b"NaN")
    _fails(lib.mvsn_fusion_gather(None, None, None, 1, 16, 4, None, None), lib, b"null")
    _fails(lib.mvsn_fusion_gather(ONE, ONE, None, 1, 16, 4, ONE, None), lib, b"null")
    for V, HW, M in ((0, 16, 4), (1, 0, 4), (1, 16, 0), (1, 1 << 31, 4)):
        _fails(lib.mvsn_fusion_gather(ONE, ONE, ONE, V, HW, M, ONE, None), lib, b"bad sizes")
    assert lib.mvsn_abi_version() == 7


def test_confidence_is_an_engine_option_off_by_default():
    assert "confidence" in EngineOptions.NAMES
    assert EngineOptions().confidence is False
    assert MultiViewStereoNet().options.confidence is False


def _scene(V=3, H=4, W=5):
    depth = torch.ones(V, 1, H, W)
    eye = torch.eye(4).repeat(V, 1, 1)
    nb = np.array([[1, 2], [0, 2], [0, 1]])
    return depth, eye, eye.clone(), nb


def test_fuse_depthmaps_confidence_validation_comes_before_the_device_check():
    depth, K, T, nb = _scene()
    conf = torch.rand(3, 1, 4, 5)
    with pytest.raises(ValueError, match="min_confidence needs"):
        fuse_depthmaps(depth, K, T, nb, min_confidence=0.5)
    with pytest.raises(ValueError, match="confidence must be"):
        fuse_depthmaps(depth, K, T, nb, confidence=conf[:, :, :3], min_confidence=0.5)
    with pytest.raises(ValueError, match="confidence must be"):
        fuse_depthmaps(depth, K, T, nb, confidence=conf[:, 0], min_confidence=0.5)
    with pytest.raises(ValueError, match="confidence must be torch.float32"):
        fuse_depthmaps(depth, K, T, nb, confidence=conf.double(), min_confidence=0.5)
    with pytest.raises(ValueError, match="confidence must be a tensor"):
        fuse_depthmaps(depth, K, T, nb, confidence=conf.numpy(), min_confidence=0.5)
    with pytest.raises(ValueError, match="confidence is on meta"):
        fuse_depthmaps(depth, K, T, nb, confidence=conf.to("meta"), min_confidence=0.5)
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="min_confidence must be"):
            fuse_depthmaps(depth, K, T, nb, confidence=conf, min_confidence=bad)
    # valid arguments reach the device check (CPU tensors: no CPU implementation)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        fuse_depthmaps(depth, K, T, nb, confidence=conf, min_confidence=0.5)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        fuse_depthmaps(depth, K, T, nb, confidence=conf)


def _ply(tmp_path, name, *args, **kw):
    path = str(tmp_path / name)
    write_ply(path, *args, **kw)
    with open(path, "rb") as f:
        return f.read()


def test_write_ply_confidence_property(tmp_path):
    g = torch.Generator().manual_seed(3)
    pts = torch.randn(7, 3, generator=g)
    col = torch.randint(0, 256, (7, 3), generator=g, dtype=torch.uint8)
    conf = torch.rand(7, generator=g)
    raw = _ply(tmp_path, "c.ply", pts, col, confidence=conf)
    header, body = raw.split(b"end_header\n", 1)
    assert header.decode("ascii") == ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\n"
                                      "property float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
                                      "property uchar blue\nproperty float confidence\n")
    rec = np.frombuffer(body, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"),
                                     ("blue", "u1"), ("confidence", "<f4")])
    assert rec.shape == (7,)
    np.testing.assert_array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), pts.numpy())
    np.testing.assert_array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), col.numpy())
    np.testing.assert_array_equal(rec["confidence"], conf.numpy())
    # without colours the property follows z
    raw = _ply(tmp_path, "n.ply", pts, confidence=conf.numpy())
    header, body = raw.split(b"end_header\n", 1)
    assert header.endswith(b"property float z\nproperty float confidence\n")
    rec = np.frombuffer(body, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("confidence", "<f4")])
    np.testing.assert_array_equal(rec["confidence"], conf.numpy())
    with pytest.raises(ValueError, match="confidence must be"):
        write_ply(str(tmp_path / "bad.ply"), pts, col, confidence=conf[:5])


def test_write_ply_without_confidence_is_unchanged(tmp_path):
    """Byte for byte what the writer produced before the keyword existed: the header and packed records, put together here
    from the PLY layout."""
    g = torch.Generator().manual_seed(4)
    pts = torch.randn(5, 3, generator=g)
    col = torch.randint(0, 256, (5, 3), generator=g, dtype=torch.uint8)
    rec = np.empty(5, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = pts.numpy()[:, 0], pts.numpy()[:, 1], pts.numpy()[:, 2]
    rec["red"], rec["green"], rec["blue"] = col.numpy()[:, 0], col.numpy()[:, 1], col.numpy()[:, 2]
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\n"
            "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert _ply(tmp_path, "a.ply", pts, col) == head.encode("ascii") + rec.tobytes()
    assert _ply(tmp_path, "b.ply", pts, col, confidence=None) == head.encode("ascii") + rec.tobytes()
    bare = ("ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\n"
            "property float z\nend_header\n")
    assert _ply(tmp_path, "d.ply", pts) == bare.encode("ascii") + pts.numpy().astype("<f4").tobytes()
