"""CPU-side checks of the boundary of the two-view consistency and depth-metric entries: every argument check of the C
entries fails before any device work, the two block-count functions, the wrappers' refusal of CPU tensors, the mask
conversion for every dtype, and the loss of an empty pyramid.  No GPU."""
import pytest
import torch

import consistency_reference as cr
from multi_view_stereonet_amd import _native, losses

ONE = 0x1000          # a non-null address that is never dereferenced: every call below fails a check first


def _fails(rc, lib, word):
    assert rc == -1 and word in lib.mvsn_last_error(), (rc, lib.mvsn_last_error())


def test_reproject_validates_before_any_device_work():
    lib = _native.load()
    good = [ONE, ONE, ONE, ONE, ONE, 2, 4, 5, ONE, ONE, ONE, ONE, ONE, ONE, None]
    for required in (0, 1, 2, 3, 8, 9, 11):           # K, T, idepth, other_idepth, idepth_in_other, other_sampled, invalid
        args = list(good)
        args[required] = None
        _fails(lib.mvsn_idepth_reproject(*args), lib, b"null pointer")
    args = list(good)
    args[4] = None                                    # other_mask_sampled asked for, no other_mask to sample
    _fails(lib.mvsn_idepth_reproject(*args), lib, b"mask output without mask input")
    for batch, rows, cols in ((0, 4, 5), (65536, 4, 5), (-1, 4, 5), (2, 0, 5), (2, 4, 0), (2, -4, 5)):
        args = list(good)
        args[5:8] = [batch, rows, cols]
        _fails(lib.mvsn_idepth_reproject(*args), lib, b"bad sizes")
    assert lib.mvsn_abi_version() == 7


def test_occlusion_mask_validates_before_any_device_work():
    lib = _native.load()
    good = [ONE, ONE, ONE, ONE, 2, 20, ONE, None]
    for required in (0, 1, 2, 3, 6):
        args = list(good)
        args[required] = None
        _fails(lib.mvsn_occlusion_mask(*args), lib, b"null pointer")
    for batch, pixels in ((0, 20), (65536, 20), (2, 0), (2, -1)):
        args = list(good)
        args[4:6] = [batch, pixels]
        _fails(lib.mvsn_occlusion_mask(*args), lib, b"bad sizes")


def test_masked_l1_validates_before_any_device_work():
    lib = _native.load()
    good = [ONE, ONE, ONE, ONE, 20, 0, ONE, None]
    for required in (0, 1, 2, 3, 6):
        args = list(good)
        args[required] = None
        _fails(lib.mvsn_masked_l1(*args), lib, b"null pointer")
    for n in (0, -1):
        args = list(good)
        args[4] = n
        _fails(lib.mvsn_masked_l1(*args), lib, b"bad size")


def test_depth_metrics_validates_before_any_device_work():
    lib = _native.load()
    good = [ONE, ONE, ONE, 2, 20, 0.5, 10.0, ONE, ONE, None]
    for required in (0, 1, 2, 7, 8):
        args = list(good)
        args[required] = None
        _fails(lib.mvsn_depth_metrics(*args), lib, b"null pointer")
    for batch, pixels in ((0, 20), (65536, 20), (2, 0), (2, -1)):
        args = list(good)
        args[3:5] = [batch, pixels]
        _fails(lib.mvsn_depth_metrics(*args), lib, b"bad sizes")


def test_block_counts():
    lib = _native.load()
    cases = (0, 1, 8192, 8193, 524288, 524289, -5)
    assert [lib.mvsn_idepth_reproject_blocks(p) for p in cases] == [0, 1, 32, 33, 2048, 2049, 0]
    assert [lib.mvsn_depth_metrics_blocks(p) for p in cases] == [0, 1, 1, 2, 64, 64, 0]
    assert [cr.metric_blocks(p) for p in cases] == [0, 1, 1, 2, 64, 64, 0]
    assert [lib.mvsn_idepth_reproject_blocks(p) for p in (255, 256, 257)] == [1, 1, 2]


def test_wrappers_raise_on_cpu_tensors():
    K, T, L, R = cr.scene(3, 5)
    occ = torch.zeros(L.shape, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        losses.idepthmap_projector(K, T, L)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        losses.get_occlusion_mask(K, T, L, None, R, None)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        losses.left_right_idepthmap_consistency_losses(T, T, [K], [L], [occ], [R], [occ])


@pytest.mark.parametrize("mask", [
    torch.tensor([[True, False], [False, True]]),
    torch.tensor([[0, 1], [2, 255]], dtype=torch.uint8),
    torch.tensor([[0, 1], [-3, 1 << 20]], dtype=torch.int32),
    torch.tensor([[0, 1], [-3, 1 << 40]], dtype=torch.int64),          # (nothing in its low byte)
    torch.tensor([[0.0, -0.0], [0.5, float("nan")]], dtype=torch.float32),
    torch.arange(12, dtype=torch.uint8).view(3, 4)[:, ::2],            # a non-contiguous view
    torch.tensor([[True, False, True], [False, False, True]]).t(),
], ids=["bool", "uint8", "int32", "int64", "float32", "uint8-strided", "bool-transposed"])
def test_as_flag_bytes_is_mask_not_equal_zero(mask):
    got = losses._as_flag_bytes(mask)
    assert got.dtype == torch.bool and got.is_contiguous() and got.shape == mask.shape
    assert got.element_size() == 1 and torch.equal(got, mask != 0)
    assert set(got.view(torch.uint8).unique().tolist()) <= {0, 1}       # the bytes the kernels read


def test_loss_of_a_pyramid_without_levels_is_a_host_zero():
    """Every level None: the reference returns the Python float 0.0 it started from (losses.py:116, 160), a value without
    a device; here the same zero as a 0-dim float32 tensor on the CPU -- no input is there to name a device."""
    K, T, _, _ = cr.scene(3, 5)
    loss = losses.left_right_idepthmap_consistency_losses(T, T, [K, K], [None, None], [None, None], [None, None], [None, None])
    assert isinstance(loss, torch.Tensor) and loss.dim() == 0 and loss.dtype == torch.float32
    assert loss.device.type == "cpu" and float(loss) == 0.0
    empty = losses.left_right_idepthmap_consistency_losses(T, T, [], [], [], [], [])
    assert empty.dim() == 0 and float(empty) == 0.0
