"""The alignment to the TSDF volume without a GPU: host-side validation (everything is rejected before any launch), CPU
tensors, degenerate volumes, and the library's three entries in the header, the binding and the binary."""
import ctypes
import os
import re

import pytest
import torch

from multi_view_stereonet_amd import _native, build, tsdf
from multi_view_stereonet_amd.tsdf import TSDFAlignment, TSDFVolume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvsn_tsdf_align_workspace_bytes", "mvsn_tsdf_align_system", "mvsn_tsdf_align")
V, H, W = 2, 4, 6


def volume(**kw):
    args = dict(dims=(5, 4, 3), voxel_size=0.1, origin=(0.0, 0.0, 1.0), trunc=0.3, device="cpu")
    args.update(kw)
    return TSDFVolume(**args)


def inputs(**kw):
    a = dict(depth=torch.ones(V, 1, H, W), K=torch.eye(4).repeat(V, 1, 1), T_cam_in_world=torch.eye(4).repeat(V, 1, 1))
    a.update(kw)
    return a


def call(vol=None, **kw):
    a = inputs(**kw)
    return (vol or volume()).align(a.pop("depth"), a.pop("K"), a.pop("T_cam_in_world"), **a)


def call_system(vol=None, **kw):
    vol = vol or volume()
    a = inputs(**kw)
    a.setdefault("band", 0.15)
    return tsdf.align_system(vol.sdf_sum, vol.weight, vol.voxel_size, vol.origin, a.pop("depth"), a.pop("K"),
                             a.pop("T_cam_in_world"), **a)


SHARED = [
    (dict(depth=None), "depth must be"), (dict(depth=torch.ones(V, H, W)), "depth must be"),
    (dict(depth=torch.ones(V, 2, H, W)), "depth must be"), (dict(depth=torch.ones(V, 1, H, W, dtype=torch.float64)), "depth must be float32"),
    (dict(depth=torch.ones(0, 1, H, W), K=torch.zeros(0, 4, 4), T_cam_in_world=torch.zeros(0, 4, 4)), "at least one view"),
    (dict(depth=torch.ones(V, 1, H, W).to("meta")), "depth is on"),
    (dict(K=None), "K must be"), (dict(K=torch.eye(4)), "K must be"), (dict(K=torch.eye(3).repeat(V, 1, 1)), "K must be"),
    (dict(K=torch.eye(4, dtype=torch.int64).repeat(V, 1, 1)), "K must be a floating-point"),
    (dict(K=torch.eye(4).repeat(V, 1, 1).to("meta")), "K is on"),
    (dict(T_cam_in_world=None), "T_cam_in_world must be"), (dict(T_cam_in_world=torch.eye(4).repeat(V + 1, 1, 1)), "T_cam_in_world must be"),
    (dict(T_cam_in_world=torch.eye(4, dtype=torch.int32).repeat(V, 1, 1)), "T_cam_in_world must be a floating-point"),
    (dict(T_cam_in_world=torch.eye(4).repeat(V, 1, 1).to("meta")), "T_cam_in_world is on"),
    (dict(valid=torch.ones(V, 1, H, W)), "valid must be"), (dict(valid=torch.ones(V, 1, H, W + 1, dtype=torch.bool)), "valid must be"),
    (dict(valid=torch.ones(V, 1, H, W, dtype=torch.bool).to("meta")), "valid is on"), (dict(valid=3), "valid must be"),
    (dict(weights=torch.ones(V, 1, H, W, dtype=torch.float64)), "weights must be"), (dict(weights=torch.ones(V, H, W)), "weights must be"),
    (dict(weights=torch.ones(V, 1, H, W).to("meta")), "weights is on"),
    (dict(min_weight=0.0), "min_weight"), (dict(min_weight=-1.0), "min_weight"), (dict(min_weight=float("nan")), "min_weight"),
    (dict(min_weight=float("inf")), "min_weight"), (dict(min_weight=None), "min_weight"),
    (dict(band=0.0), "band"), (dict(band=-0.1), "band"), (dict(band=float("nan")), "band"), (dict(band=float("inf")), "band"),
    (dict(band=1e-46), "band"), (dict(band="wide"), "band"),
    (dict(stride=0), "stride"), (dict(stride=-2), "stride"), (dict(stride=1.5), "stride"), (dict(stride=True), "stride"),
    (dict(stride=None), "stride"), (dict(stride="two"), "stride"),
]
LOOP_ONLY = [
    (dict(iterations=-1), "iterations"), (dict(iterations=1001), "iterations"), (dict(iterations=2.5), "iterations"),
    (dict(iterations=None), "iterations"), (dict(iterations=True), "iterations"),
    (dict(min_pixels=0), "min_pixels"), (dict(min_pixels=-3), "min_pixels"), (dict(min_pixels=6.5), "min_pixels"),
    (dict(min_pixels=None), "min_pixels"),
    (dict(min_pivot=0.0), "min_pivot"), (dict(min_pivot=1.0), "min_pivot"), (dict(min_pivot=-1e-9), "min_pivot"),
    (dict(min_pivot=float("nan")), "min_pivot"), (dict(min_pivot="small"), "min_pivot"), (dict(min_pivot=None), "min_pivot"),
]


@pytest.mark.parametrize("kw, match", SHARED + LOOP_ONLY)
def test_align_arguments_are_validated(kw, match):
    with pytest.raises(ValueError, match=match):
        call(**kw)
    with pytest.raises(ValueError, match=match):          # (validated before the degenerate volume's answer)
        call(volume(dims=(1, 4, 3)), **kw)


@pytest.mark.parametrize("kw, match", SHARED)
def test_align_system_arguments_are_validated(kw, match):
    with pytest.raises(ValueError, match=match):
        call_system(**kw)
    with pytest.raises(ValueError, match=match):
        call_system(volume(dims=(5, 1, 3)), **kw)


def test_size_limits():
    big = torch.ones(1, 1, 1, 1).expand(65536, 1, H, W)
    eye = torch.eye(4).expand(65536, 4, 4)
    with pytest.raises(ValueError, match="65535 views"):
        volume().align(big, eye, eye)
    row = torch.ones(1, 1, 1, 1).expand(1, 1, 1, 2 ** 24 + 4)
    with pytest.raises(ValueError, match=r"2\^24 rows or columns"):
        volume().align(row, torch.eye(4)[None], torch.eye(4)[None])
    area = torch.ones(1, 1, 1, 1).expand(1, 1, 2 ** 16, 2 ** 15)
    with pytest.raises(ValueError, match=r"2\^31 - 1 pixels"):
        volume().align(area, torch.eye(4)[None], torch.eye(4)[None])


def test_the_state_is_validated_and_the_band_is_required():
    s, w = torch.zeros(3, 4, 5), torch.zeros(3, 4, 5)
    a = inputs()
    rest = (a["depth"], a["K"], a["T_cam_in_world"])
    for fn in (tsdf.align, tsdf.align_system):
        for state, match in (((s[0], w), "sdf_sum"), ((s.double(), w), "sdf_sum"), ((s, w[:2]), "weight"),
                             ((s, w.double()), "weight"), ((s, w.to("meta")), "weight is on")):
            with pytest.raises(ValueError, match=match):
                fn(*state, 0.1, (0, 0, 0), *rest, band=0.1)
        with pytest.raises(ValueError, match="voxel_size"):
            fn(s, w, 0.0, (0, 0, 0), *rest, band=0.1)
        with pytest.raises(ValueError, match="origin"):
            fn(s, w, 0.1, (0, 0), *rest, band=0.1)
        with pytest.raises(ValueError, match="depth is on"):
            fn(s.to("meta"), w.to("meta"), 0.1, (0, 0, 0), *rest, band=0.1)
        with pytest.raises(TypeError, match="band"):
            fn(s, w, 0.1, (0, 0, 0), *rest)
    with pytest.raises(TypeError):
        tsdf.align_system(s, w, 0.1, (0, 0, 0), *rest, band=0.1, iterations=3)


def test_cpu_tensors_raise_the_usual_runtime_error():
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call(K=torch.eye(4, dtype=torch.float64).repeat(V, 1, 1), valid=torch.ones(V, 1, H, W, dtype=torch.bool),
             weights=torch.ones(V, 1, H, W), band=0.1, iterations=0, stride=10 ** 9, min_pixels=10 ** 12, min_pivot=0.5)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call_system(with_residual=True)


@pytest.mark.parametrize("dims", [(1, 4, 3), (5, 1, 3), (5, 4, 1), (1, 1, 1)])
@pytest.mark.parametrize("iterations", [0, 3])
def test_degenerate_volumes_are_answered_without_a_launch(dims, iterations):
    vol = volume(dims=dims)
    vol.sdf_sum.fill_(-1.0)
    vol.weight.fill_(2.0)
    T = torch.eye(4, dtype=torch.float64).repeat(V, 1, 1)
    T[:, 0, 3] = 1.0 / 3.0
    r = call(vol, T_cam_in_world=T, iterations=iterations)
    assert isinstance(r, TSDFAlignment)
    assert r.T_cam_in_world.dtype == torch.float32 and torch.equal(r.T_cam_in_world, T.float())
    assert r.history.shape == (V, iterations + 1, 3) and r.history.dtype == torch.float64 and not r.history.any()
    assert r.status.dtype == torch.int32 and r.status.tolist() == [1] * V
    assert r.information.shape == (V, 6, 6) and r.information.dtype == torch.float64 and not r.information.any()
    Hm, b, count, sw, swr2, res = call_system(vol, with_residual=True)
    assert Hm.shape == (V, 6, 6) and b.shape == (V, 6) and Hm.dtype == b.dtype == sw.dtype == swr2.dtype == torch.float64
    assert count.dtype == torch.int64 and count.tolist() == [0] * V and not Hm.any() and not b.any() and not sw.any() and not swr2.any()
    assert res.shape == (V, 1, H, W) and res.dtype == torch.float32 and torch.isnan(res).all()
    assert call_system(vol)[5] is None


def test_the_default_band_is_half_the_truncation():
    doc = TSDFVolume.align.__doc__
    assert "trunc / 2" in doc and "not a measured constant" in doc


def test_entries_in_header_binding_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_tsdf_align.hip") == 1 and build.HEADERS.count("mvsn_tsdf_sample.h") == 1
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SIGNATURES
    # the binding's argument counts are the header's
    for name in ENTRIES:
        decl = re.search(r"^(?:size_t|int) %s\(([^;]*)\);" % name, header, re.M).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]), name
    lib = ctypes.CDLL(_native.library_path())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    size = lib.mvsn_tsdf_align_workspace_bytes
    size.restype, size.argtypes = ctypes.c_size_t, [ctypes.c_int] * 7
    assert size(0, 4, 4, 1, 4, 4, 1) == 0 and size(2048, 2048, 512, 1, 4, 4, 1) == 0 and size(4, 4, 4, 0, 4, 4, 1) == 0
    assert size(4, 4, 4, 1, 0, 4, 1) == 0 and size(4, 4, 4, 1, 4, 4, 0) == 0 and size(4, 4, 4, 65536, 4, 4, 1) == 0
    assert size(4, 4, 4, 1, 2 ** 24 + 1, 1, 1) == 0 and size(4, 4, 4, 1, 2 ** 16, 2 ** 15, 1) == 0
    # the plane, the poses and one record of 30 doubles per workgroup of 32 x 32 lattice pixels, each on 256 bytes
    n = 21 * 19 * 17

    def up(x):
        return (x + 255) // 256 * 256
    assert size(21, 19, 17, 3, 37, 61, 1) == up(4 * n) + up(3 * 96) + up(3 * 2 * 2 * 240)
    assert size(21, 19, 17, 3, 37, 61, 2) == up(4 * n) + up(3 * 96) + up(3 * 1 * 1 * 240)
    assert size(21, 19, 17, 1, 1, 1029, 1) == up(4 * n) + up(96) + up(33 * 240)


def test_c_entries_check_their_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    ok = dict(sdf_sum=one, weight=one, nx=4, ny=4, nz=4, voxel_size=0.1, origin_x=0.0, depth=one, valid=None, weights=None,
              K=one, T=one, n_views=1, rows=4, cols=4, stride=1, min_weight=1.0, band=0.1, ws=one, ws_bytes=1 << 20)

    def head(a):
        return (a["sdf_sum"], a["weight"], a["nx"], a["ny"], a["nz"], a["voxel_size"], a["origin_x"], 0.0, 0.0, a["depth"],
                a["valid"], a["weights"], a["K"], a["T"], a["n_views"], a["rows"], a["cols"], a["stride"], a["min_weight"],
                a["band"])

    def system(**kw):
        a = dict(ok, H=one, b=one, sums=one)
        a.update(kw)
        return lib.mvsn_tsdf_align_system(*head(a), a["ws"], a["ws_bytes"], a["H"], a["b"], a["sums"], None, None)

    def loop(**kw):
        a = dict(ok, iterations=2, min_pixels=6, min_pivot=1e-9, T_out=one, history=one, status=one, information=one)
        a.update(kw)
        return lib.mvsn_tsdf_align(*head(a), a["iterations"], a["min_pixels"], a["min_pivot"], a["ws"], a["ws_bytes"],
                                   a["T_out"], a["history"], a["status"], a["information"], None)
    # (nothing passes: the last checks are the workspace's, and its size is asked for below)
    for fn in (system, loop):
        for name in ("sdf_sum", "weight", "depth", "K", "T"):
            assert fn(**{name: None}) == -1, name
        assert fn(n_views=0) == -1 and fn(rows=0) == -1 and fn(cols=-3) == -1
        assert fn(n_views=65536) == -2 and fn(rows=2 ** 16, cols=2 ** 15) == -2
        assert fn(rows=2 ** 24 + 1, cols=1) == -2 and fn(cols=2 ** 24 + 4, rows=1) == -2
        assert fn(stride=0) == -1 and fn(stride=-1) == -1 and fn(stride=2 ** 24 + 1) == -1
        assert fn(nx=1) == -1 and fn(ny=0) == -1 and fn(nz=1) == -1
        assert fn(nx=2048, ny=2048, nz=512) == -2 and fn(nx=2 ** 24 + 4, ny=2, nz=2) == -2
        assert fn(voxel_size=0.0) == -1 and fn(voxel_size=float("nan")) == -1 and fn(voxel_size=float("inf")) == -1
        assert fn(min_weight=0.0) == -1 and fn(min_weight=float("nan")) == -1
        assert fn(band=0.0) == -1 and fn(band=-1.0) == -1 and fn(band=float("inf")) == -1 and fn(band=float("nan")) == -1
        assert fn(origin_x=float("inf")) == -1 and fn(origin_x=float("nan")) == -1
        need = lib.mvsn_tsdf_align_workspace_bytes(4, 4, 4, 1, 4, 4, 1)
        assert need == 3 * 256
        assert fn(ws=None) == -3 and fn(ws_bytes=need - 1) == -3 and fn(ws_bytes=0) == -3
        assert fn(ws=ctypes.c_void_p(8)) == -1                   # not 16-byte aligned
    assert b"mvsn_tsdf_align" in lib.mvsn_last_error()
    for name in ("H", "b", "sums"):
        assert system(**{name: None}) == -1, name
    for name in ("T_out", "history", "status", "information"):
        assert loop(**{name: None}) == -1, name
    assert loop(iterations=-1) == -1 and loop(iterations=1001) == -1
    assert loop(min_pixels=0) == -1 and loop(min_pivot=0.0) == -1 and loop(min_pivot=1.0) == -1 and loop(min_pivot=float("nan")) == -1
