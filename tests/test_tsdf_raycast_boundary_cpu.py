"""The ray-cast of the TSDF volume without a GPU: host-side validation (everything is rejected before any launch), CPU
tensors, degenerate volumes, and the library's two entries in the header, the binding and the binary."""
import ctypes
import os
import re

import pytest
import torch

from multi_view_stereonet_amd import _native, build
from multi_view_stereonet_amd.tsdf import TSDFRender, TSDFVolume, raycast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvsn_tsdf_raycast_workspace_bytes", "mvsn_tsdf_raycast")
V, H, W = 2, 4, 6


def volume(**kw):
    args = dict(dims=(5, 4, 3), voxel_size=0.1, origin=(0.0, 0.0, 1.0), trunc=0.3, device="cpu")
    args.update(kw)
    return TSDFVolume(**args)


def call(vol=None, **kw):
    a = dict(K=torch.eye(4).repeat(V, 1, 1), T_cam_in_world=torch.eye(4).repeat(V, 1, 1), size=(H, W))
    a.update(kw)
    return (vol or volume()).raycast(a.pop("K"), a.pop("T_cam_in_world"), a.pop("size"), **a)


@pytest.mark.parametrize("kw, match", [
    (dict(K=None), "K must be"), (dict(K=torch.eye(4)), "K must be"), (dict(K=torch.eye(3).repeat(V, 1, 1)), "K must be"),
    (dict(K=torch.eye(4).repeat(V, 1, 1).numpy()), "K must be"), (dict(K=torch.zeros(0, 4, 4), T_cam_in_world=torch.zeros(0, 4, 4)), "at least one view"),
    (dict(T_cam_in_world=None), "T_cam_in_world must be"), (dict(T_cam_in_world=torch.eye(4).repeat(V + 1, 1, 1)), "T_cam_in_world must be"),
    (dict(K=torch.eye(4, dtype=torch.int64).repeat(V, 1, 1)), "K must be a floating-point"),
    (dict(T_cam_in_world=torch.eye(4, dtype=torch.int32).repeat(V, 1, 1)), "T_cam_in_world must be a floating-point"),
    (dict(K=torch.eye(4).repeat(V, 1, 1).to("meta")), "K is on"),
    (dict(T_cam_in_world=torch.eye(4).repeat(V, 1, 1).to("meta")), "T_cam_in_world is on"),
    (dict(K=torch.eye(4).repeat(65536, 1, 1), T_cam_in_world=torch.eye(4).repeat(65536, 1, 1)), "65535 views"),
    (dict(size=(H,)), "size"), (dict(size=(H, W, 1)), "size"), (dict(size=(0, W)), "size"), (dict(size=(H, -1)), "size"),
    (dict(size=(2.5, W)), "size"), (dict(size="big"), "size"), (dict(size=None), "size"), (dict(size=(True, W)), "size"),
    (dict(size=(2 ** 24 + 1, 1)), r"2\^24 rows or columns"), (dict(size=(1, 2 ** 24 + 4)), r"2\^24 rows or columns"),
    (dict(size=(2 ** 16, 2 ** 15)), r"2\^31 - 1 pixels"),
    (dict(step=0.0), "step"), (dict(step=-0.1), "step"), (dict(step=float("nan")), "step"), (dict(step=float("inf")), "step"),
    (dict(step=1e-46), "step"), (dict(step=1e39), "step"), (dict(step="small"), "step"),
    (dict(min_weight=0.0), "min_weight"), (dict(min_weight=-1.0), "min_weight"), (dict(min_weight=float("nan")), "min_weight"),
    (dict(min_weight=float("inf")), "min_weight"), (dict(min_weight=None), "min_weight"),
    (dict(min_depth=float("nan")), "min_depth"), (dict(min_depth=float("inf")), "min_depth"), (dict(min_depth="near"), "min_depth"),
    (dict(max_depth=0.0), "max_depth"), (dict(max_depth=-1.0), "max_depth"), (dict(min_depth=2.0, max_depth=2.0), "max_depth"),
    (dict(min_depth=2.0, max_depth=1.0), "max_depth"), (dict(max_depth=float("nan")), "max_depth"),
    (dict(max_depth=float("inf")), "max_depth"), (dict(max_depth="far"), "max_depth"),
    (dict(step=5e-7), r"at most 2\^20"),                 # 0.1 * |(4,3,2)| / 5e-7 + 2 = 1.08e6 samples
])
def test_raycast_arguments_are_validated(kw, match):
    with pytest.raises(ValueError, match=match):
        call(**kw)
    if not {"K", "T_cam_in_world", "size"} & set(kw) and "2^20" not in match.replace("\\", ""):   # (a shorter diagonal)
        with pytest.raises(ValueError, match=match):      # (validated before the degenerate volume's zero maps)
            call(volume(dims=(1, 4, 3)), **kw)


def test_the_sample_bound_is_the_diagonal_over_the_step():
    # 0.1 * |(4,3,2)| / step + 2 <= 2^20 exactly when step >= 5.1357e-7
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call(step=5.2e-7)
    with pytest.raises(ValueError, match=r"at most 2\^20"):
        call(step=5.1e-7)


def test_raycast_state_is_validated():
    s, w = torch.zeros(3, 4, 5), torch.zeros(3, 4, 5)
    K = T = torch.eye(4)[None]
    for args, match in (((s[0], w, None), "sdf_sum"), ((s.double(), w, None), "sdf_sum"), ((s, w[:2], None), "weight"),
                        ((s, w.double(), None), "weight"), ((s, w.to("meta"), None), "weight is on"),
                        ((s, w, torch.zeros(3, 4, 5)), "color_sum"), ((s, w, torch.zeros(3, 3, 4, 5).to("meta")), "color_sum is on")):
        with pytest.raises(ValueError, match=match):
            raycast(*args, 0.1, (0, 0, 0), K, T, (H, W))
    with pytest.raises(ValueError, match="voxel_size"):
        raycast(s, w, None, 0.0, (0, 0, 0), K, T, (H, W))
    with pytest.raises(ValueError, match="origin"):
        raycast(s, w, None, 0.1, (0, 0), K, T, (H, W))
    with pytest.raises(ValueError, match="is on"):
        raycast(s.to("meta"), w.to("meta"), None, 0.1, (0, 0, 0), K, T, (H, W))


def test_cpu_tensors_raise_the_usual_runtime_error():
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call(volume(color=True), K=torch.eye(4, dtype=torch.float64).repeat(V, 1, 1), max_depth=9.0, step=0.05)
    s, w = torch.zeros(3, 4, 5), torch.zeros(3, 4, 5)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        raycast(s, w, None, 0.1, (0, 0, 0), torch.eye(4)[None], torch.eye(4)[None], (H, W))


@pytest.mark.parametrize("dims", [(1, 4, 3), (5, 1, 3), (5, 4, 1), (1, 1, 1)])
@pytest.mark.parametrize("color", [False, True])
def test_degenerate_volumes_return_zero_maps(dims, color):
    vol = volume(dims=dims, color=color)
    vol.sdf_sum.fill_(-1.0)
    vol.weight.fill_(2.0)
    r = call(vol)
    assert isinstance(r, TSDFRender)
    assert r.depth.shape == r.weight.shape == (V, 1, H, W) and r.normals.shape == (V, 3, H, W)
    assert (r.colors is None) != color
    for t in r:
        if t is not None:
            assert t.dtype == torch.float32 and t.device == vol.sdf_sum.device and not t.any()
    if color:
        assert r.colors.shape == (V, 3, H, W)


def test_entries_in_header_binding_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_tsdf_raycast.hip") == 1
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SIGNATURES
    lib = ctypes.CDLL(_native.library_path())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    lib.mvsn_tsdf_raycast_workspace_bytes.restype = ctypes.c_size_t
    lib.mvsn_tsdf_raycast_workspace_bytes.argtypes = [ctypes.c_int] * 3
    size = lib.mvsn_tsdf_raycast_workspace_bytes
    assert size(0, 4, 4) == 0 and size(2048, 2048, 512) == 0 and size(2 ** 24 + 4, 2, 2) == 0
    assert size(2 ** 24, 2, 2) >= 4 * 2 ** 26
    n = 21 * 19 * 17
    assert 4 * n <= size(21, 19, 17) < 4 * n + 256 and size(21, 19, 17) % 256 == 0


def test_c_entries_check_their_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    ok = dict(sdf_sum=one, weight=one, color_sum=None, nx=4, ny=4, nz=4, voxel_size=0.1, origin_x=0.0, K=one, T=one,
              n_views=1, rows=4, cols=4, min_weight=1.0, min_depth=0.0, max_depth=float("inf"), step=0.1, ws=one,
              ws_bytes=1 << 20, depth=one, normals=one, colors=None, weight_out=one)

    def cast(**kw):
        a = dict(ok, **kw)
        return lib.mvsn_tsdf_raycast(a["sdf_sum"], a["weight"], a["color_sum"], a["nx"], a["ny"], a["nz"], a["voxel_size"],
                                     a["origin_x"], 0.0, 0.0, a["K"], a["T"], a["n_views"], a["rows"], a["cols"],
                                     a["min_weight"], a["min_depth"], a["max_depth"], a["step"], a["ws"], a["ws_bytes"],
                                     a["depth"], a["normals"], a["colors"], a["weight_out"], None)
    # (nothing passes: the last checks are the workspace's, and its size is asked for below)
    for name in ("sdf_sum", "weight", "K", "T", "depth", "normals", "weight_out"):
        assert cast(**{name: None}) == -1, name
    assert b"mvsn_tsdf_raycast" in lib.mvsn_last_error()
    assert cast(color_sum=one) == -1 and cast(colors=one) == -1
    assert cast(n_views=0) == -1 and cast(rows=0) == -1 and cast(cols=-3) == -1
    assert cast(n_views=65536) == -2 and cast(rows=2 ** 16, cols=2 ** 15) == -2
    assert cast(rows=2 ** 24 + 1, cols=1) == -2 and cast(cols=2 ** 24 + 4, rows=1) == -2
    assert cast(nx=1) == -1 and cast(ny=0) == -1 and cast(nz=1) == -1
    assert cast(nx=2048, ny=2048, nz=512) == -2 and cast(nx=2 ** 24 + 4, ny=2, nz=2) == -2
    assert cast(voxel_size=0.0) == -1 and cast(voxel_size=float("nan")) == -1 and cast(voxel_size=float("inf")) == -1
    assert cast(min_weight=0.0) == -1 and cast(min_weight=float("nan")) == -1
    assert cast(step=0.0) == -1 and cast(step=-1.0) == -1 and cast(step=float("inf")) == -1
    assert cast(origin_x=float("inf")) == -1 and cast(min_depth=float("nan")) == -1 and cast(min_depth=float("-inf")) == -1
    assert cast(max_depth=0.0) == -1 and cast(max_depth=float("nan")) == -1 and cast(min_depth=1.0, max_depth=0.5) == -1
    assert cast(step=4e-7) == -2                                 # 0.1 * |(3,3,3)| / 4e-7 + 2 = 1.3e6 samples
    need = lib.mvsn_tsdf_raycast_workspace_bytes(4, 4, 4)
    assert need == 256
    assert cast(ws=None) == -3 and cast(ws_bytes=need - 1) == -3 and cast(ws_bytes=0) == -3
    assert cast(ws=ctypes.c_void_p(8)) == -1                     # not 16-byte aligned
