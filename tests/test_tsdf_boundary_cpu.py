"""The TSDF volume without a GPU: host-side validation (everything is rejected before any launch), CPU tensors,
degenerate volumes, write_ply(faces=), and the library's tsdf entries in the header, the binding and the binary."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multi_view_stereonet_amd import _native, build
from multi_view_stereonet_amd.fusion import write_ply
from multi_view_stereonet_amd.tsdf import TSDFMesh, TSDFVolume, extract_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvsn_tsdf_camera_batch", "mvsn_tsdf_integrate", "mvsn_tsdf_workspace_bytes", "mvsn_tsdf_classify",
           "mvsn_tsdf_extract")
V, H, W = 2, 4, 6


def volume(**kw):
    args = dict(dims=(5, 4, 3), voxel_size=0.1, origin=(0.0, 0.0, 1.0), trunc=0.3, device="cpu")
    args.update(kw)
    return TSDFVolume(**args)


def views(**kw):
    a = dict(depth=torch.ones(V, 1, H, W), K=torch.eye(4).repeat(V, 1, 1), T_cam_in_world=torch.eye(4).repeat(V, 1, 1))
    a.update(kw)
    return a


@pytest.mark.parametrize("kw, match", [
    (dict(dims=(5, 4)), "dims"), (dict(dims=(5, 4, 0)), "dims"), (dict(dims=(5.5, 4, 3)), "dims"),
    (dict(dims="big"), "dims"), (dict(dims=(2048, 2048, 512)), r"2\^31 - 1 voxels"),
    (dict(dims=(2 ** 24 + 4, 2, 2)), r"2\^24"), (dict(dims=(2, 1, 2 ** 24 + 1)), r"2\^24"),
    (dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=-1.0), "voxel_size"), (dict(voxel_size=float("nan")), "voxel_size"),
    (dict(voxel_size=float("inf")), "voxel_size"), (dict(voxel_size=1e-46), "voxel_size"), (dict(voxel_size=1e39), "voxel_size"),
    (dict(voxel_size="thin"), "voxel_size"), (dict(voxel_size=None), "voxel_size"),
    (dict(trunc=0.0), "trunc"), (dict(trunc=-0.1), "trunc"), (dict(trunc=float("nan")), "trunc"),
    (dict(trunc=float("inf")), "trunc"), (dict(trunc=None), "trunc"),
    (dict(origin=(0.0, 0.0)), "origin"), (dict(origin=(0.0, float("nan"), 0.0)), "origin"),
    (dict(origin=(0.0, float("inf"), 0.0)), "origin"), (dict(origin="here"), "origin"),
])
def test_volume_arguments_are_validated(kw, match):
    with pytest.raises(ValueError, match=match):
        volume(**kw)


def test_volume_layout_reset_and_values():
    vol = volume(color=True)
    assert vol.sdf_sum.shape == vol.weight.shape == (3, 4, 5) and vol.color_sum.shape == (3, 3, 4, 5)
    assert vol.sdf_sum.dtype == vol.weight.dtype == vol.color_sum.dtype == torch.float32
    assert volume().color_sum is None
    assert vol.voxel_size == np.float32(0.1) and vol.trunc == np.float32(0.3) and vol.origin.dtype == np.float32
    vol.sdf_sum[1, 2, 3], vol.weight[1, 2, 3] = 3.0, 2.0
    vals = vol.values()
    assert float(vals[1, 2, 3]) == 1.5 and int(torch.isnan(vals).sum()) == 59
    vol.color_sum.fill_(1.0)
    vol.reset()
    assert not vol.sdf_sum.any() and not vol.weight.any() and not vol.color_sum.any()


@pytest.mark.parametrize("kw, match", [
    (dict(depth=np.ones((V, 1, H, W), np.float32)), r"\(V,1,H,W\)"),
    (dict(depth=torch.ones(V, H, W)), r"\(V,1,H,W\)"), (dict(depth=torch.ones(V, 2, H, W)), r"\(V,1,H,W\)"),
    (dict(depth=torch.ones(V, 1, H, W, dtype=torch.float64)), "float32"),
    (dict(depth=torch.ones(0, 1, H, W)), "at least one view"),
    (dict(depth=torch.ones(V, 1, H, W, device="meta")), "is on meta"),
    (dict(depth=torch.ones(65536, 1, 1, 1), K=torch.eye(4).repeat(65536, 1, 1),
          T_cam_in_world=torch.eye(4).repeat(65536, 1, 1)), "65535 views"),
    (dict(K=torch.eye(4).repeat(V + 1, 1, 1)), "K must be"), (dict(K=torch.eye(3).repeat(V, 1, 1)), "K must be"),
    (dict(K=torch.eye(4).repeat(V, 1, 1).to("meta")), "K is on"),
    (dict(K=torch.eye(4, dtype=torch.int64).repeat(V, 1, 1)), "K must be a floating-point"),
    (dict(T_cam_in_world=torch.eye(4, dtype=torch.int32).repeat(V, 1, 1)), "T_cam_in_world must be a floating-point"),
    (dict(depth=torch.ones(1, 1, 1, 2 ** 24 + 4, device="meta"), K=torch.eye(4)[None].to("meta"),
          T_cam_in_world=torch.eye(4)[None].to("meta")), r"2\^24 rows or columns"),
    (dict(T_cam_in_world=torch.eye(4)), "T_cam_in_world must be"), (dict(T_cam_in_world=None), "T_cam_in_world must be"),
    (dict(images=torch.zeros(V, 3, H, W)), "color=True"),
    (dict(valid=torch.ones(V, 1, H, W)), "valid must be"), (dict(valid=torch.ones(V, 1, H, W + 1, dtype=torch.bool)), "valid must be"),
    (dict(weights=torch.ones(V, H, W)), "weights must be"), (dict(weights=torch.ones(V, 1, H, W + 1)), "weights must be"),
    (dict(weights=torch.ones(V, 3, H, W)), "weights must be"),
    (dict(weights=torch.ones(V, 1, H, W, dtype=torch.float64)), "weights must be"),
    (dict(min_depth=float("nan")), "min_depth"), (dict(min_depth=float("inf")), "min_depth"), (dict(min_depth="near"), "min_depth"),
])
def test_integrate_arguments_are_validated(kw, match):
    with pytest.raises(ValueError, match=match):
        volume().integrate(**views(**kw))


def test_colour_and_images_go_together():
    with pytest.raises(ValueError, match="color=True"):
        volume(color=True).integrate(**views())
    with pytest.raises(ValueError, match="images must be"):
        volume(color=True).integrate(**views(images=torch.zeros(V, 1, H, W)))
    with pytest.raises(ValueError, match="images must be"):
        volume(color=True).integrate(**views(images=torch.zeros(V, 3, H, W, dtype=torch.float16)))


def test_cpu_tensors_raise_the_usual_runtime_error():
    with pytest.raises(RuntimeError, match="HIP devices only"):
        volume().integrate(**views())
    with pytest.raises(RuntimeError, match="HIP devices only"):
        volume(color=True).integrate(**views(images=torch.zeros(V, 3, H, W)))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        volume().extract_mesh()


@pytest.mark.parametrize("min_weight", [0.0, -1.0, float("nan"), float("inf"), 1e-46, 1e39, "some", None])
def test_min_weight_must_be_positive_and_finite(min_weight):
    with pytest.raises(ValueError, match="min_weight"):
        volume().extract_mesh(min_weight)
    with pytest.raises(ValueError, match="min_weight"):
        volume(dims=(1, 4, 3)).extract_mesh(min_weight)          # (validated before the degenerate volume's empties)


def test_extract_state_is_validated():
    s, w = torch.zeros(3, 4, 5), torch.zeros(3, 4, 5)
    for args, match in (((s[0], w, None), "sdf_sum"), ((s.double(), w, None), "sdf_sum"), ((s, w[:2], None), "weight"),
                        ((s, w.double(), None), "weight"), ((s, w.to("meta"), None), "weight is on"),
                        ((s, w, torch.zeros(3, 4, 5)), "color_sum"), ((s, w, torch.zeros(3, 3, 4, 5).to("meta")), "color_sum is on")):
        with pytest.raises(ValueError, match=match):
            extract_mesh(*args, 0.1, (0, 0, 0))
    with pytest.raises(ValueError, match="voxel_size"):
        extract_mesh(s, w, None, 0.0, (0, 0, 0))
    with pytest.raises(ValueError, match="origin"):
        extract_mesh(s, w, None, 0.1, (0, 0))


@pytest.mark.parametrize("dims", [(1, 4, 3), (5, 1, 3), (5, 4, 1), (1, 1, 1)])
@pytest.mark.parametrize("color", [False, True])
def test_degenerate_volumes_return_empties(dims, color):
    m = volume(dims=dims, color=color).extract_mesh()
    assert isinstance(m, TSDFMesh)
    assert m.vertices.shape == (0, 3) and m.normals.shape == (0, 3) and m.faces.shape == (0, 3) and m.cell.shape == (0,)
    assert m.vertices.dtype == m.normals.dtype == torch.float32 and m.faces.dtype == m.cell.dtype == torch.int64
    assert (m.colors is None) != color
    if color:
        assert m.colors.shape == (0, 3) and m.colors.dtype == torch.uint8


def read_ply(path):
    """A numpy reader of the binary PLY files write_ply makes: (vertex record array, faces (F,3) or None)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    n = int(re.match(r"element vertex (\d+)", lines[2]).group(1))
    fields, k = [], 3
    while lines[k].startswith("property ") and not lines[k].startswith("property list"):
        _, typ, name = lines[k].split()
        fields.append((name, {"float": "<f4", "uchar": "u1"}[typ]))
        k += 1
    verts = np.frombuffer(data, dtype=fields, count=n, offset=end)
    faces = None
    if lines[k].startswith("element face"):
        F = int(lines[k].split()[2])
        assert lines[k + 1] == "property list uchar int vertex_indices" and lines[k + 2] == "end_header"
        rec = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=F, offset=end + verts.nbytes)
        assert (rec["n"] == 3).all() and end + verts.nbytes + rec.nbytes == len(data)
        faces = rec["v"].astype(np.int64)
    else:
        assert lines[k] == "end_header" and end + verts.nbytes == len(data)
    return verts, faces


def test_write_ply_faces_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((7, 3)).astype(np.float32)
    nrm = rng.standard_normal((7, 3)).astype(np.float32)
    col = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    faces = rng.integers(0, 7, (5, 3))
    p = str(tmp_path / "mesh.ply")
    write_ply(p, torch.from_numpy(pts), colors=torch.from_numpy(col), normals=torch.from_numpy(nrm),
              faces=torch.from_numpy(faces))
    verts, got = read_ply(p)
    np.testing.assert_array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), pts)
    np.testing.assert_array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), nrm)
    np.testing.assert_array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), col)
    np.testing.assert_array_equal(got, faces)
    write_ply(p, pts, faces=np.zeros((0, 3), np.int64))         # no faces: an empty face element
    verts, got = read_ply(p)
    assert verts.shape == (7,) and got.shape == (0, 3)


@pytest.mark.parametrize("faces", [[[0, 1, 7]], [[-1, 0, 1]], [[0, 1]], [[0.0, 1.0, 2.0]], [0, 1, 2]])
def test_write_ply_refuses_bad_faces(tmp_path, faces):
    with pytest.raises(ValueError, match="faces"):
        write_ply(str(tmp_path / "bad.ply"), np.zeros((7, 3), np.float32), faces=np.asarray(faces))


def test_write_ply_without_faces_is_unchanged(tmp_path):
    # the layout the function had before `faces`: header, then the packed vertex records, nothing else
    rng = np.random.default_rng(1)
    pts = rng.standard_normal((4, 3)).astype(np.float32)
    nrm = rng.standard_normal((4, 3)).astype(np.float32)
    col = rng.integers(0, 256, (4, 3)).astype(np.uint8)
    conf = rng.random(4).astype(np.float32)
    p = str(tmp_path / "cloud.ply")
    write_ply(p, pts, colors=col, confidence=conf, normals=nrm)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\n" +
              "".join(f"property float {n}\n" for n in ("x", "y", "z", "nx", "ny", "nz")) +
              "".join(f"property uchar {n}\n" for n in ("red", "green", "blue")) +
              "property float confidence\nend_header\n").encode("ascii")
    body = b"".join(pts[i].tobytes() + nrm[i].tobytes() + col[i].tobytes() + conf[i].tobytes() for i in range(4))
    with open(p, "rb") as f:
        assert f.read() == header + body
    write_ply(p, pts)
    with open(p, "rb") as f:
        assert f.read() == b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\n" \
                            b"property float z\nend_header\n" + pts.tobytes()


def test_entries_in_header_binding_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        header = f.read()
    assert build.SOURCES.count("mvsn_tsdf.hip") == 1
    assert _native.ABI_VERSION == 7 and "#define MVSN_ABI_VERSION 7" in header.replace("  ", " ")
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SIGNATURES
    lib = ctypes.CDLL(_native.library_path())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    lib.mvsn_tsdf_workspace_bytes.restype = ctypes.c_size_t
    lib.mvsn_tsdf_workspace_bytes.argtypes = [ctypes.c_int] * 3
    assert lib.mvsn_tsdf_workspace_bytes(0, 4, 4) == 0 and lib.mvsn_tsdf_workspace_bytes(2048, 2048, 512) == 0
    assert lib.mvsn_tsdf_workspace_bytes(2 ** 24 + 4, 2, 2) == 0 and lib.mvsn_tsdf_workspace_bytes(2 ** 24, 2, 2) > 0
    n = 21 * 19 * 17
    assert lib.mvsn_tsdf_workspace_bytes(21, 19, 17) >= 5 * n
    assert lib.mvsn_tsdf_camera_batch() == 32


def test_c_entries_check_their_own_arguments():
    lib = _native.load()
    one = ctypes.c_void_p(16)                                    # (never dereferenced: every call fails its checks first)
    ok = dict(n_views=1, rows=4, cols=4, nx=4, ny=4, nz=4, voxel_size=0.1, trunc=0.3)

    def integrate(depth=one, images=None, color_sum=None, min_depth=0.0, origin_x=0.0, **kw):
        a = dict(ok, **kw)
        return lib.mvsn_tsdf_integrate(depth, None, None, images, one, one, a["n_views"], a["rows"], a["cols"], a["nx"],
                                       a["ny"], a["nz"], a["voxel_size"], origin_x, 0.0, 0.0, a["trunc"], min_depth, one,
                                       one, color_sum, None)
    assert integrate(depth=None) == -1 and b"mvsn_tsdf_integrate" in lib.mvsn_last_error()
    assert integrate(images=one) == -1 and integrate(color_sum=one) == -1
    assert integrate(n_views=0) == -1 and integrate(rows=0) == -1 and integrate(nx=0) == -1
    assert integrate(n_views=65536) == -2 and integrate(nx=2048, ny=2048, nz=512) == -2
    assert integrate(cols=2 ** 24 + 4, rows=2) == -2 and integrate(rows=2 ** 24 + 1, cols=2) == -2
    assert integrate(nx=2 ** 24 + 4, ny=2, nz=2) == -2 and integrate(nx=2 ** 24, ny=2, nz=2, depth=None) == -1
    assert integrate(voxel_size=0.0) == -1 and integrate(voxel_size=float("nan")) == -1 and integrate(trunc=float("inf")) == -1
    assert integrate(min_depth=float("nan")) == -1 and integrate(origin_x=float("inf")) == -1
    assert lib.mvsn_tsdf_classify(None, one, 4, 4, 4, 1.0, one, one, 1 << 20, None) == -1
    assert lib.mvsn_tsdf_classify(one, one, 1, 4, 4, 1.0, one, one, 1 << 20, None) == -1
    assert lib.mvsn_tsdf_classify(one, one, 4, 4, 4, 0.0, one, one, 1 << 20, None) == -1
    assert lib.mvsn_tsdf_classify(one, one, 4, 4, 4, 1.0, one, one, 8, None) == -3
    assert lib.mvsn_tsdf_classify(one, one, 4, 4, 4, 1.0, one, ctypes.c_void_p(8), 1 << 20, None) == -1
    extract = lambda **kw: lib.mvsn_tsdf_extract(one, one, kw.get("color_sum"), 4, 4, kw.get("nz", 4), 0.1, 0.0, 0.0, 0.0,  # noqa: E731
                                                 1.0, one, kw.get("ws", 1 << 20), kw.get("m", 1), kw.get("q", 1), one, one,
                                                 None, one, one, None)
    assert extract(color_sum=one) == -1 and extract(nz=1) == -1 and extract(m=65) == -1 and extract(q=193) == -1
    assert extract(ws=8) == -3
