"""mesh_render on the device (csrc/mvsn_mesh_render.hip) against the numpy restatement
(tests/mesh_render_reference.py).  Every case goes through the C ABI with the inputs in poisoned buffers of their own and
the workspace and every output between guard bands, under both poisons.  The restatement performs the kernels' operations
one for one: depth, face, weights, normals, colours and clipped are compared byte for byte and no tolerance applies
anywhere.

Figures of one MI355X run are in DESIGN.md section 27."""
import functools

import numpy as np
import pytest
import torch

import mesh_render_reference as mr
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd.mesh import MeshRender, mesh_render
from multi_view_stereonet_amd.tsdf import TSDFVolume

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _render(vertices, faces, K, T, rows, cols, *, normals=None, colors=None, min_depth=0.0, max_depth=np.inf,
            fill=POISON_NAN):
    """mvsn_mesh_render: numpy arrays of the six outputs (None for a gather that was not asked for)."""
    M, F, V = len(vertices), len(faces), len(K)
    guard = Guard(_alloc, fill)
    v, f, Kd, Td = (guard.poisoned(_to(a)) for a in (vertices, faces, K, T))
    nor = guard.poisoned(_to(normals)) if normals is not None else None
    col = guard.poisoned(_to(colors)) if colors is not None else None
    lib = _native.load()
    ws_bytes = lib.mvsn_mesh_render_workspace_bytes(V, rows, cols)
    assert ws_bytes == 8 * V * (rows * cols + 1)
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    depth, face = guard.empty((V, rows, cols), torch.float32, DEV), guard.empty((V, rows, cols), torch.int64, DEV)
    weights = guard.empty((V, 3, rows, cols), torch.float32, DEV)
    out_nor = guard.empty((V, 3, rows, cols), torch.float32, DEV) if normals is not None else None
    out_col = guard.empty((V, 3, rows, cols), torch.uint8, DEV) if colors is not None else None
    clipped = guard.empty((V,), torch.int64, DEV)
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_mesh_render(
            _native.ptr(v), M, _native.ptr(f), F, _native.ptr(nor), _native.ptr(col), _native.ptr(Kd), _native.ptr(Td), V,
            rows, cols, float(min_depth), float(max_depth), _native.ptr(ws), ws_bytes, _native.ptr(depth),
            _native.ptr(face), _native.ptr(weights), _native.ptr(out_nor), _native.ptr(out_col), _native.ptr(clipped),
            _native.stream()), "mvsn_mesh_render")
    torch.cuda.synchronize()
    guard.check()
    host = lambda t: t.cpu().numpy() if t is not None else None   # noqa: E731
    return {"depth": host(depth), "face": host(face), "weights": host(weights), "normals": host(out_nor),
            "colors": host(out_col), "clipped": host(clipped)}


def _case(name, gathers=True, fill=POISON_NAN):
    c = mr.case(name)
    return _render(c["vertices"], c["faces"], c["K"], c["T"], c["rows"], c["cols"], fill=fill, **mr.render_args(c, gathers))


@functools.lru_cache(maxsize=None)
def _device(name, gathers=True, fill=POISON_NAN):
    """Made once per (case, gathers, poison), never modified."""
    return _case(name, gathers, fill)


def _same_bits(a, b, keys=mr.OUTPUTS):
    for key in keys:
        if b[key] is None:
            assert a[key] is None, key
            continue
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


def test_the_constants_are_the_restatements():
    lib = _native.load()
    assert lib.mvsn_mesh_render_small_pixels() == mr.SMALL_PIXELS
    assert lib.mvsn_cloud_render_camera_batch() == mr.CAMERA_BATCH


# ---- one face on a 1 x 1 map (a hit, and a miss that still writes 0 / -1 / zeros); the workgroup and wave edges (63 .. 257
# ---- faces; 5 x 7 and 33 x 65 pixels; one camera less than a batch, a batch, one more); boxes at the threshold between the
# ---- two raster paths; a whole-map face among 300 small ones; 64 large faces in one wave; large and small interleaved;
# ---- 4099 coincident faces in four orders; the faces that take no part; clipping; the depth limits; the borders; the
# ---- gathers' special values; the watertight sheets ------------------------------------------------------------------
@pytest.mark.parametrize("name", mr.CASES)
def test_cases_match_the_restatement_byte_for_byte(name):
    _same_bits(_device(name), mr.case_reference(name))


@pytest.mark.parametrize("name", mr.CASES)
def test_buffers_under_both_poisons(name):
    # (the guard bands of every buffer are checked inside _render; an element nobody writes, or a read of foreign memory
    # or of the uninitialised workspace that reaches a result, differs between the two fills)
    _same_bits(_device(name, True, POISON_NAN), _device(name, True, POISON_FINITE))
    _same_bits(_device(name, True, POISON_FINITE), mr.case_reference(name))


@pytest.mark.parametrize("name", ["one_hit", "one_miss", "edge_257_33_65_1", "edge_63_5_7_-1", "whole_map", "nonpart",
                                  "gathers"])
def test_the_gathers_are_optional(name):
    got = _device(name, False)
    assert got["colors"] is None and got["normals"] is None
    _same_bits(got, mr.case_reference(name, False))
    c = mr.case(name)
    args = (c["vertices"], c["faces"], c["K"], c["T"], c["rows"], c["cols"])
    only = _render(*args, **dict(mr.render_args(c), normals=None))
    assert only["normals"] is None and only["colors"].tobytes() == mr.case_reference(name)["colors"].tobytes()
    only = _render(*args, **dict(mr.render_args(c), colors=None))
    assert only["colors"] is None and only["normals"].tobytes() == mr.case_reference(name)["normals"].tobytes()


def test_the_smallest_render_writes_every_output_on_a_miss():
    miss = _device("one_miss")
    assert miss["depth"].tolist() == [[[0.0]]] and miss["face"].tolist() == [[[-1]]] and miss["clipped"].tolist() == [0]
    assert miss["weights"].tobytes() == np.zeros(3, np.float32).tobytes()
    assert miss["colors"].reshape(-1).tolist() == [0, 0, 0] and miss["normals"].tobytes() == np.zeros(3, np.float32).tobytes()
    hit = _device("one_hit")
    assert hit["depth"].tolist() == [[[2.0]]] and hit["face"].tolist() == [[[0]]]
    assert hit["colors"].reshape(-1).tolist() == [7, 8, 9] and hit["weights"].sum() == 1.0


@pytest.mark.parametrize("name", mr.CONTENTION_CASES + ["edge_256_33_65_0", "whole_map", "wave_large", "wave_mixed"])
def test_calling_twice_gives_the_same_bytes(name):
    _same_bits(_case(name), _device(name))


def test_the_lowest_row_wins_a_tie_and_the_nearest_face_wins_otherwise():
    r, c = mr.CONTENTION_PIXEL
    assert _device("contention_equal")["face"][0, r, c] == 0
    for order in ("ascending", "descending", "shuffled"):
        z = mr.case("contention_" + order)["vertices"][::3, 2]
        got = _device("contention_" + order)
        assert got["face"][0, r, c] == np.argmin(z) and got["depth"][0, r, c] == z.min()


def test_permuted_faces_give_the_same_depth_bytes():
    for name in ("edge_257_33_65_1", "whole_map", "wave_mixed", "contention_shuffled"):
        c = mr.case(name)
        perm = mr.permutation(len(c["faces"]))
        moved = _render(c["vertices"], c["faces"][perm], c["K"], c["T"], c["rows"], c["cols"])
        base = _device(name)
        assert moved["depth"].tobytes() == base["depth"].tobytes(), name
        assert moved["clipped"].tobytes() == base["clipped"].tobytes()
        same = perm[moved["face"]] == base["face"]
        assert same[base["face"] >= 0].mean() > 0.99 and (moved["face"] >= 0).tobytes() == (base["face"] >= 0).tobytes()


def test_a_flipped_face_gives_the_same_bytes_apart_from_the_order_of_the_weights():
    a, b = _device("nonpart", False), _device("nonpart_flipped", False)
    _same_bits(a, b, ("depth", "face", "clipped"))
    assert a["weights"][:, [0, 2, 1]].tobytes() == b["weights"].tobytes() and (a["face"] >= 0).all()


def test_faces_that_take_no_part_leave_the_face_behind_them():
    got = _device("nonpart")
    back = mr.NONPART_ROWS["back"][0]
    for name, (row, covers) in mr.NONPART_ROWS.items():
        assert (got["face"] == row).any() == covers, name
    assert set(np.unique(got["face"]).tolist()) == {mr.NONPART_ROWS["plain"][0], mr.NONPART_ROWS["flipped_twin"][0], back}


def test_clipped_counts_and_the_guard_band():
    got = _device("clipping")
    counted = sum(c for _, _, c in mr.CLIP_ROWS.values())
    assert got["clipped"][0] == counted == 5
    for name, (row, part, _) in mr.CLIP_ROWS.items():
        assert (got["face"][0] == row).any() == part, name


def test_the_depth_limits_are_open_below_and_closed_above():
    got = _device("depth_limits")
    seen = {name: (got["face"][0] == row).any() for row, name in enumerate(mr.LIMIT_ROWS)}
    assert seen == {"at_min": False, "above_min": True, "at_max": True, "past_max": False, "between": True}
    d = got["depth"][got["face"] >= 0]
    assert (d > np.float32(mr.LIMIT_MIN)).all() and d.max() == np.float32(mr.LIMIT_MAX)


# ---- the Python interface ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    s = synthetic.fusion_scene(3, 48, 64)
    dev = {k: v.to(DEV) for k, v in s.items()}
    vol = TSDFVolume((128, 128, 128), 0.04, (-2.56, -2.56, 3.2), 0.16, device=DEV, color=True)
    vol.integrate(dev["depth"], dev["K"], dev["T_cam_in_world"], images=dev["images"])
    return s, dev, vol.extract_mesh()


def test_the_python_call_is_the_library_call_on_the_tsdf_mesh():
    s, dev, mesh = _scene()
    F = int(mesh.faces.shape[0])
    assert F > 3000 and mesh.colors is not None
    K, T = s["K"].numpy(), s["T_cam_in_world"].numpy()
    r = mesh_render(mesh.vertices, mesh.faces, dev["K"].double(), dev["T_cam_in_world"].double(), (48, 64),
                    normals=mesh.normals, colors=mesh.colors, min_depth=0.5, max_depth=50.0)
    assert isinstance(r, MeshRender) and MeshRender._fields == mr.OUTPUTS
    assert r.depth.shape == (3, 1, 48, 64) and r.face.shape == (3, 48, 64) and r.weights.shape == (3, 3, 48, 64)
    ref = mr.render_reference(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), K, T, 48, 64,
                              mesh.normals.cpu().numpy(), mesh.colors.cpu().numpy(), 0.5, 50.0)
    got = {"depth": r.depth[:, 0].cpu().numpy(), "face": r.face.cpu().numpy(), "weights": r.weights.cpu().numpy(),
           "normals": r.normals.cpu().numpy(), "colors": r.colors.cpu().numpy(), "clipped": r.clipped.cpu().numpy()}
    _same_bits(got, ref)
    # (a sanity check that the picture is not empty: the volume holds a part of what the three views see)
    assert (got["face"] >= 0).mean() > 0.25 and (got["face"] >= 0).sum() == (ref["cover"] > 0).sum()
    bare = mesh_render(mesh.vertices, mesh.faces, dev["K"], dev["T_cam_in_world"], (48, 64))
    assert bare.normals is None and bare.colors is None and bare.clipped.dtype == torch.int64
    wide = mesh_render(mesh.vertices, mesh.faces, dev["K"], dev["T_cam_in_world"], (48, 64), min_depth=0.5, max_depth=50.0)
    assert torch.equal(wide.depth, r.depth) and torch.equal(wide.face, r.face) and torch.equal(wide.weights, r.weights)
