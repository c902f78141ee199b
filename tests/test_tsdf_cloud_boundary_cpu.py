"""integrate_cloud, TSDFVolume.around and read_ply without a GPU: host-side validation (everything is rejected before
any launch, with the library unreachable), the empty cloud, CPU tensors, the library's entries in the header, the
binding, the build list and the binary, and the PLY reader against the writer."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from multi_view_stereonet_amd import _native, build, fusion, tsdf
from multi_view_stereonet_amd.fusion import PlyData, read_ply, write_ply
from multi_view_stereonet_amd.tsdf import TSDFVolume, integrate_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, BYTES = "mvsn_tsdf_cloud_integrate", "mvsn_tsdf_cloud_workspace_bytes"
N, DIMS = 5, (4, 3, 2)
NAN, INF = float("nan"), float("inf")


@pytest.fixture
def no_library(monkeypatch):
    """The library unreachable: whatever passes under it was decided on the host, before any launch."""
    def unreachable():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load", unreachable)


def volume(color=False, device="cpu"):
    return TSDFVolume(DIMS, 0.1, (0.0, 0.0, 0.0), 0.3, device=device, color=color)


def call(color=False, **kw):
    a = dict(points=torch.zeros(N, 3), normals=torch.ones(N, 3), radius=0.25)
    a.update(kw)
    return volume(color).integrate_cloud(a.pop("points"), a.pop("normals"), a.pop("radius"), **a)


def call_state(**kw):
    v = volume()
    a = dict(sdf_sum=v.sdf_sum, weight=v.weight, color_sum=None, voxel_size=0.1, origin=(0, 0, 0), trunc=0.3,
             points=torch.zeros(N, 3), normals=torch.ones(N, 3), radius=0.25)
    a.update(kw)
    pos = [a.pop(k) for k in ("sdf_sum", "weight", "color_sum", "voxel_size", "origin", "trunc", "points", "normals", "radius")]
    return integrate_cloud(*pos, **a)


BAD = [
    (dict(points=None), "points must be"), (dict(points=torch.zeros(N, 4)), "points must be"),
    (dict(points=torch.zeros(N, 3, dtype=torch.float64)), "points must be float32"),
    (dict(points=torch.zeros(N, 3).to("meta")), "points is on"),
    (dict(normals=None), "normals must be"), (dict(normals=torch.ones(N + 1, 3)), "normals must be"),
    (dict(normals=torch.ones(N, 3, dtype=torch.float64)), "normals must be"), (dict(normals=torch.ones(N, 3).to("meta")), "normals is on"),
    (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=NAN), "radius"), (dict(radius=INF), "radius"),
    (dict(radius=1e-30), "radius"), (dict(radius="far"), "radius"),
    (dict(weights=torch.ones(N, 1)), "weights must be"), (dict(weights=torch.ones(N, dtype=torch.float64)), "weights must be"),
    (dict(weights=torch.ones(N + 1)), "weights must be"), (dict(weights=[1.0] * N), "weights must be"),
    (dict(weights=torch.ones(N).to("meta")), "weights is on"),
    (dict(colors=torch.zeros(N, 3, dtype=torch.uint8)), "colors need a volume made with color=True"),
    (dict(color=True), "colors need a volume made with color=True"),
    (dict(color=True, colors=torch.zeros(N, 3)), "colors must be"), (dict(color=True, colors=torch.zeros(N, dtype=torch.uint8)), "colors must be"),
    (dict(color=True, colors=torch.zeros(N, 3, dtype=torch.uint8).to("meta")), "colors is on"),
]
BAD_STATE = [
    (dict(sdf_sum=torch.zeros(2, 3)), "sdf_sum must be"), (dict(weight=torch.zeros(2, 3, 5)), "weight must be"),
    (dict(color_sum=torch.zeros(2, 2, 3, 4)), "color_sum must be"),
    (dict(sdf_sum=torch.zeros(2, 3, 8)[:, :, ::2]), "sdf_sum must be contiguous"),
    (dict(weight=torch.zeros(2, 3, 8)[:, :, ::2]), "weight must be contiguous"),
    (dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=NAN), "voxel_size"), (dict(trunc=-1.0), "trunc"), (dict(trunc=INF), "trunc"),
    (dict(origin=(0, 0)), "origin"), (dict(origin=(0, NAN, 0)), "origin"), (dict(points=torch.zeros(N, 2)), "points must be"),
    (dict(radius=0), "radius"),
]


@pytest.mark.parametrize("kw, match", BAD)
def test_arguments_are_validated_before_any_launch(no_library, kw, match):
    with pytest.raises(ValueError, match=match):
        call(**kw)


@pytest.mark.parametrize("kw, match", BAD_STATE)
def test_the_state_call_validates_the_state_too(no_library, kw, match):
    with pytest.raises(ValueError, match=match):
        call_state(**kw)


def test_sizes_are_limited_and_the_options_are_keywords(no_library):
    big = torch.zeros(1, 3).expand(2 ** 31, 3)
    with pytest.raises(ValueError, match=r"2\^31 - 1 points"):
        call(points=big, normals=big)
    with pytest.raises(TypeError):
        volume().integrate_cloud(torch.zeros(N, 3), torch.ones(N, 3), 0.25, torch.ones(N))     # weights is a keyword
    with pytest.raises(TypeError):
        volume().integrate_cloud(torch.zeros(N, 3), torch.ones(N, 3))                         # radius is required


def test_an_empty_cloud_is_answered_without_a_launch(no_library):
    for color in (False, True):
        v = volume(color)
        v.sdf_sum.fill_(2.5)
        v.weight.fill_(1.5)
        colors = torch.zeros(0, 3, dtype=torch.uint8) if color else None
        assert v.integrate_cloud(torch.zeros(0, 3), torch.zeros(0, 3), 0.25, weights=torch.zeros(0), colors=colors) is None
        assert bool((v.sdf_sum == 2.5).all()) and bool((v.weight == 1.5).all())
        with pytest.raises(ValueError, match="radius"):          # (validated before the empty cloud's answer)
            v.integrate_cloud(torch.zeros(0, 3), torch.zeros(0, 3), 0.0, colors=colors)
    assert call_state(points=torch.zeros(0, 3), normals=torch.zeros(0, 3)) is None


def test_cpu_tensors_raise_the_usual_runtime_error(no_library):
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call(color=True, colors=torch.zeros(N, 3, dtype=torch.uint8), weights=torch.ones(N))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        call_state()


def test_the_docstrings_say_what_the_call_does():
    doc = integrate_cloud.__doc__
    assert "order of the rows" in doc and "bitwise reproducible" in doc and "not bit-identical" in doc
    assert "2^19 - 1" in doc and "(0, 256]" in doc and "blend" in doc and "cloud_nearest" in doc
    assert "integrate_cloud" in tsdf.__doc__ and "read_ply" in fusion.__doc__
    assert "depth maps and clouds" in TSDFVolume.integrate_cloud.__doc__


# ---- TSDFVolume.around ---------------------------------------------------------------------------------------------------
def test_around_is_the_smallest_lattice_volume_that_holds_the_points_and_the_padding(no_library):
    p = torch.tensor([[0.13, -0.42, 1.0], [0.71, 0.2, 1.3], [NAN, 0.0, 0.0], [0.0, INF, 0.0], [5.0, 5.0, -INF]])
    for vs, trunc, pad in ((0.1, 0.3, None), (0.25, 0.5, 0.0), (0.07, 0.2, 1.0)):
        v = TSDFVolume.around(p, vs, trunc, padding=pad, color=pad is not None)
        assert isinstance(v, TSDFVolume) and (v.color_sum is not None) == (pad is not None) and v.sdf_sum.device == p.device
        assert v.voxel_size == np.float32(vs) and v.trunc == np.float32(trunc) and not v.weight.any()
        pd = float(np.float32(trunc if pad is None else pad))
        lo, hi = p[:2].min(0).values.double().numpy() - pd, p[:2].max(0).values.double().numpy() + pd
        o, step = v.origin.astype(np.float64), float(v.voxel_size)
        top = o + step * (np.asarray(v.dims) - 1)
        assert (o <= lo).all() and (top >= hi).all()                      # holds the finite points plus the padding
        assert (o + 2 * step > lo).all() and (top - 2 * step < hi).all()  # ... and no more than the lattice needs
        assert (np.abs(o / step - np.rint(o / step)) < 1e-3).all()        # on the lattice of multiples of voxel_size
    one = TSDFVolume.around(torch.tensor([[0.2, 0.2, 0.2]]), 0.1, 0.3, padding=0)
    assert max(one.dims) <= 2


@pytest.mark.parametrize("args, kw, match", [
    ((torch.zeros(0, 3), 0.1, 0.3), {}, "no finite row"), ((torch.full((4, 3), NAN), 0.1, 0.3), {}, "no finite row"),
    ((torch.tensor([[0.0, 0.0, INF]]), 0.1, 0.3), {}, "no finite row"),
    ((torch.zeros(3, 2), 0.1, 0.3), {}, "points must be"), ((torch.zeros(3, 3, dtype=torch.float64), 0.1, 0.3), {}, "float32"),
    ((torch.zeros(3, 3), 0.0, 0.3), {}, "voxel_size"), ((torch.zeros(3, 3), 0.1, NAN), {}, "trunc"),
    ((torch.zeros(3, 3), 0.1, 0.3), dict(padding=-0.1), "padding"), ((torch.zeros(3, 3), 0.1, 0.3), dict(padding=NAN), "padding"),
    ((torch.zeros(3, 3), 0.1, 0.3), dict(padding="wide"), "padding"),
    ((torch.tensor([[0.0, 0.0, 0.0], [1e6, 0.0, 0.0]]), 0.01, 0.3), {}, r"at most 2\^31 - 1 voxels and 2\^24 along an axis"),
    ((torch.tensor([[0.0, 0.0, 0.0], [200.0, 200.0, 200.0]]), 0.1, 0.3), {}, r"at most 2\^31 - 1 voxels"),
])
def test_around_refuses(no_library, args, kw, match):
    with pytest.raises(ValueError, match=match):
        TSDFVolume.around(*args, **kw)


# ---- the entries ------------------------------------------------------------------------------------------------------------
def test_entries_in_header_binding_build_list_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_tsdf_cloud.hip") == 1 and build.HEADERS.count("mvsn_cloud.h") == 1
    for name in build.SOURCES + build.HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    lib = ctypes.CDLL(_native.library_path())
    for name, kind, count in ((ENTRY, "int", 24), (BYTES, "size_t", 3)):
        assert name in _native.SIGNATURES and hasattr(lib, name)
        decl = re.search(r"^%s %s\(([^;]*)\);" % (kind, name), header, re.M).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]) == count, name
    with open(os.path.join(build.CSRC, "mvsn_tsdf_cloud.hip")) as f:
        source = f.read()
    assert '#include "mvsn_cloud.h"' in source and "#pragma clang fp contract(off)" in source and not re.search(r"\batomic[A-Z]", source)


def test_the_workspace_is_a_flag_byte_per_brick():
    lib = _native.load()
    fn = lib.mvsn_tsdf_cloud_workspace_bytes
    assert fn(1, 1, 1) == 256 and fn(8, 8, 8) == 256 and fn(21, 19, 17) == 256 and fn(64, 64, 64) == 512
    assert fn(65, 64, 64) == 9 * 8 * 8 + (-(9 * 8 * 8) % 256) and fn(2 ** 24, 1, 1) == 2 ** 21
    for dims in ((0, 1, 1), (1, -1, 1), (2 ** 24 + 1, 1, 1), (2 ** 16, 2 ** 15, 1), (2 ** 11, 2 ** 10, 2 ** 10)):
        assert fn(*dims) == 0, dims
    assert fn(2 ** 11, 2 ** 10, 2 ** 10 - 1) > 0


def test_the_c_entry_checks_its_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    need, flags = lib.mvsn_cloud_workspace_bytes(N), lib.mvsn_tsdf_cloud_workspace_bytes(*DIMS)
    ok = dict(points=one, normals=one, weights=None, colors=None, n=N, iws=one, iws_bytes=need - 1, cell=0.5, inv=2.0, r2=0.25,
              nx=DIMS[0], ny=DIMS[1], nz=DIMS[2], vs=0.1, ox=0.0, oy=0.0, oz=0.0, trunc=0.3, sdf=one, weight=one, color=None,
              ws=one, ws_bytes=flags)

    def fn(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.mvsn_tsdf_cloud_integrate(*(a[k] for k in ok), None)
    # (nothing passes: the index workspace is one byte short throughout, or another check fails first)
    assert fn() == -3 and ENTRY.encode() in lib.mvsn_last_error() and b"index workspace" in lib.mvsn_last_error()
    assert fn(weights=one) == -3                                  # weights are optional
    for name in ("points", "normals", "sdf", "weight"):
        assert fn(**{name: None}) == -1, name
    assert ENTRY.encode() in lib.mvsn_last_error()
    assert fn(colors=one) == -1 and fn(color=one) == -1 and fn(colors=one, color=one) == -3
    assert fn(n=0) == -1 and fn(n=-5) == -1 and fn(n=2 ** 31) == -2
    for name in ("cell", "inv", "r2", "vs", "trunc"):
        assert fn(**{name: 0.0}) == -1 and fn(**{name: NAN}) == -1 and fn(**{name: INF}) == -1 and fn(**{name: -1.0}) == -1, name
    for name in ("ox", "oy", "oz"):
        assert fn(**{name: NAN}) == -1 and fn(**{name: INF}) == -1 and fn(**{name: -1e30}) == -3, name
    assert fn(nx=0) == -1 and fn(ny=-1) == -1 and fn(nz=0) == -1
    assert fn(nx=2 ** 24 + 1) == -2 and fn(nx=2 ** 16, ny=2 ** 16) == -2 and fn(nx=2 ** 11, ny=2 ** 10, nz=2 ** 10) == -2
    assert fn(iws=None) == -3 and fn(iws_bytes=0) == -3
    assert fn(iws=ctypes.c_void_p(24), iws_bytes=need) == -1      # not 16-byte aligned
    # the index workspace passes: now the flag workspace is looked at
    assert fn(iws_bytes=need, ws=None) == -3 and b"workspace" in lib.mvsn_last_error()
    assert fn(iws_bytes=need, ws_bytes=flags - 1) == -3 and fn(iws_bytes=need, ws=ctypes.c_void_p(24)) == -1
    # the codes in their order: a null pointer before the size, the size before the workspace
    assert fn(points=None, n=2 ** 31, iws=None) == -1 and fn(n=2 ** 31, iws=None) == -2


# ---- read_ply ------------------------------------------------------------------------------------------------------------------
def _cloud(n, f, normals, colors, confidence, faces, seed=0):
    rng = np.random.default_rng(seed)
    return dict(points=rng.normal(size=(n, 3)).astype(np.float32),
                normals=rng.normal(size=(n, 3)).astype(np.float32) if normals else None,
                colors=rng.integers(0, 256, (n, 3)).astype(np.uint8) if colors else None,
                confidence=rng.random(n).astype(np.float32) if confidence else None,
                faces=(rng.integers(0, n, (f, 3)) if n else np.zeros((0, 3), np.int64)) if faces else None)


@pytest.mark.parametrize("n, f", [(7, 4), (7, 0), (0, 0), (1, 1)])
def test_read_ply_returns_everything_write_ply_can_write_byte_for_byte(tmp_path, n, f):
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    for flags in itertools.product((False, True), repeat=4):
        c = _cloud(n, f, *flags)
        write_ply(a, c["points"], colors=c["colors"], confidence=c["confidence"], normals=c["normals"], faces=c["faces"])
        r = read_ply(a)
        assert isinstance(r, PlyData) and PlyData._fields == ("points", "normals", "colors", "confidence", "faces")
        for k, dtype, shape in (("points", torch.float32, (n, 3)), ("normals", torch.float32, (n, 3)),
                                ("colors", torch.uint8, (n, 3)), ("confidence", torch.float32, (n,)),
                                ("faces", torch.int64, (0 if c["faces"] is None else len(c["faces"]), 3))):
            got = getattr(r, k)
            if c[k] is None:
                assert got is None, k
                continue
            assert torch.is_tensor(got) and got.device.type == "cpu" and got.dtype == dtype and tuple(got.shape) == shape, k
            assert got.numpy().tobytes() == np.ascontiguousarray(c[k]).astype(got.numpy().dtype).tobytes(), k
        write_ply(b, r.points, colors=r.colors, confidence=r.confidence, normals=r.normals, faces=r.faces)
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read()


ASCII = """ply
format ascii 1.0
comment a ground-truth cloud
element vertex 3
property uchar red
property uchar green
property uchar blue
property float32 x
property float y
property float z
property float confidence
property float nx
property float ny
property float nz
element face 2
property list uint8 uint vertex_index
end_header
1 2 3 0 0.5 -1 0.25 0 0 1
255 0 9 1.5 2e-3 -2.5e3 1 0 1 0
0 0 0 nan inf -inf 0 1 0 0
3 0 1 2
3 2 1 0
"""


def _write(tmp_path, content, name="x.ply"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(content if isinstance(content, bytes) else content.encode("ascii"))
    return path


def test_read_ply_reads_ascii_with_the_properties_in_any_order(tmp_path):
    r = read_ply(_write(tmp_path, ASCII))
    assert r.points.dtype == torch.float32 and r.colors.dtype == torch.uint8 and r.faces.dtype == torch.int64
    want = np.array([[0, 0.5, -1], [1.5, 2e-3, -2.5e3], [np.nan, np.inf, -np.inf]], np.float32)
    assert r.points.numpy().tobytes() == want.tobytes()
    assert r.colors.tolist() == [[1, 2, 3], [255, 0, 9], [0, 0, 0]] and r.confidence.tolist() == [0.25, 1.0, 0.0]
    assert r.normals.tolist() == [[0, 0, 1], [0, 1, 0], [1, 0, 0]] and r.faces.tolist() == [[0, 1, 2], [2, 1, 0]]
    # binary, the same properties in that order
    path = str(tmp_path / "bin.ply")
    write_ply(path, r.points, faces=r.faces)
    with open(path, "rb") as f:
        data = f.read()
    moved = data.replace(b"property float x\nproperty float y\nproperty float z\n", b"property float z\nproperty float y\nproperty float x\n")
    back = read_ply(_write(tmp_path, moved.replace(b" int vertex_indices", b" uint vertex_indices"), "moved.ply"))
    assert back.points.numpy().tobytes() == want[:, ::-1].tobytes() and back.faces.tolist() == r.faces.tolist()


def _binary(tmp_path, n=3, f=2):
    path = str(tmp_path / "ok.ply")
    c = _cloud(n, f, True, True, True, True)
    write_ply(path, c["points"], colors=c["colors"], confidence=c["confidence"], normals=c["normals"], faces=c["faces"])
    with open(path, "rb") as fh:
        return fh.read()


REFUSALS = [
    (lambda d: d.replace(b"ply\n", b"plx\n", 1), "not a PLY file"),
    (lambda d: d.replace(b"end_header\n", b"end\n"), "not a PLY file"),
    (lambda d: d.replace(b"binary_little_endian", b"binary_big_endian"), "binary_big_endian"),
    (lambda d: d.replace(b"format binary_little_endian 1.0\n", b""), "no format line"),
    (lambda d: d.replace(b"property float x\n", b"property double x\n"), "double x"),
    (lambda d: d.replace(b"property uchar red\n", b"property float red\n"), "float red"),
    (lambda d: d.replace(b"property float confidence\n", b"property float intensity\n"), "intensity"),
    (lambda d: d.replace(b"property float nz\n", b""), "nx, ny, nz go together"),
    (lambda d: d.replace(b"property float x\n", b""), "x, y, z go together"),
    (lambda d: d.replace(b"property float y\n", b"property float x\n"), "appears twice"),
    (lambda d: d.replace(b"element face", b"element edge"), "element 'edge'"),
    (lambda d: d.replace(b"element vertex 3\n", b"element material 1\nproperty float x\nelement vertex 3\n"), "element 'material'"),
    (lambda d: d.replace(b"list uchar int vertex_indices", b"list uchar short vertex_indices"), "short vertex_indices"),
    (lambda d: d.replace(b"list uchar int vertex_indices", b"list int int vertex_indices"), "int int vertex_indices"),
    (lambda d: d.replace(b"property list uchar int vertex_indices\n", b""), "no vertex_indices"),
    (lambda d: d.replace(b"end_header\n", b"property float quality\nend_header\n"), "quality"),
    (lambda d: d[:-1], "truncated"), (lambda d: d[:d.index(b"end_header\n") + 11 + 20], "truncated"),
    (lambda d: d + b"\0", "1 bytes after the last element"),
    (lambda d: d[:-13] + b"\4" + d[-12:], "face 1 has 4 vertices"),
    (lambda d: d[:-4] + b"\3\0\0\0", "indexes outside the 3 vertices"),
    (lambda d: d[:-4] + b"\xff\xff\xff\xff", "indexes outside the 3 vertices"),
]


@pytest.mark.parametrize("index", range(len(REFUSALS)))
def test_read_ply_names_what_it_did_not_understand(tmp_path, index):
    change, match = REFUSALS[index]
    good = _binary(tmp_path)
    assert read_ply(_write(tmp_path, good, "good.ply")).faces.shape == (2, 3)
    bad = change(good)
    assert bad != good
    with pytest.raises(ValueError, match=match):
        read_ply(_write(tmp_path, bad, "bad.ply"))


@pytest.mark.parametrize("change, match", [
    (lambda s: s.replace("3 2 1 0\n", ""), "truncated"), (lambda s: s[:s.index("0 0 0 nan")], "truncated"),
    (lambda s: s.replace("3 2 1 0\n", "4 2 1 0 0\n"), "only triangles"), (lambda s: s + "7\n", "after the last element"),
    (lambda s: s.replace("255 0 9", "256 0 9"), "not an integer in"), (lambda s: s.replace("255 0 9", "2.5 0 9"), "not an integer in"),
    (lambda s: s.replace("0.5 -1 0.25", "0.5 abc 0.25"), "not a number"), (lambda s: s.replace("3 2 1 0\n", "3 2 1 3\n"), "indexes outside"),
    (lambda s: s.replace("format ascii 1.0", "format ascii 2.0"), "ascii 2.0"),
])
def test_read_ply_refuses_broken_ascii_too(tmp_path, change, match):
    with pytest.raises(ValueError, match=match):
        read_ply(_write(tmp_path, change(ASCII)))
