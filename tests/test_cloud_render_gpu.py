"""cloud_render, cloud_visibility and cloud_colorize on the device (csrc/mvsn_cloud_render.hip) against the numpy
restatement (tests/cloud_render_reference.py).  Every case goes through the C ABI with the inputs in poisoned buffers of
their own and the workspace and every output between guard bands, under both poisons.  The restatement performs the
kernels' fp32 operations one for one, and everything on top of them is integer work: depth, index, colours, normals,
visible, count and values are compared byte for byte and no tolerance applies anywhere.

Figures of one MI355X run are in DESIGN.md section 25."""
import functools

import numpy as np
import pytest
import torch

import cloud_render_reference as cr
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd.fusion import (CloudRender, CloudVisibility, cloud_colorize, cloud_render,
                                             cloud_visibility, fuse_depthmaps)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISONS = (POISON_NAN, POISON_FINITE)


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _render(points, K, T, rows, cols, *, radius=0, colors=None, normals=None, min_depth=0.0, max_depth=np.inf,
            fill=POISON_NAN):
    """mvsn_cloud_render: numpy arrays of the four outputs (None for a gather that was not asked for)."""
    n, V = len(points), len(K)
    guard = Guard(_alloc, fill)
    p, Kd, Td = guard.poisoned(_to(points)), guard.poisoned(_to(K)), guard.poisoned(_to(T))
    col = guard.poisoned(_to(colors)) if colors is not None else None
    nor = guard.poisoned(_to(normals)) if normals is not None else None
    lib = _native.load()
    ws_bytes = lib.mvsn_cloud_render_workspace_bytes(V, rows, cols)
    assert ws_bytes == 8 * V * rows * cols
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    depth, index = guard.empty((V, rows, cols), torch.float32, DEV), guard.empty((V, rows, cols), torch.int64, DEV)
    out_col = guard.empty((V, 3, rows, cols), torch.uint8, DEV) if colors is not None else None
    out_nor = guard.empty((V, 3, rows, cols), torch.float32, DEV) if normals is not None else None
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_cloud_render(_native.ptr(p), n, _native.ptr(col), _native.ptr(nor), _native.ptr(Kd),
                                            _native.ptr(Td), V, rows, cols, int(radius), float(min_depth), float(max_depth),
                                            _native.ptr(ws), ws_bytes, _native.ptr(depth), _native.ptr(index),
                                            _native.ptr(out_col), _native.ptr(out_nor), _native.stream()),
                      "mvsn_cloud_render")
    torch.cuda.synchronize()
    guard.check()
    host = lambda t: t.cpu().numpy() if t is not None else None   # noqa: E731
    return {"depth": host(depth), "index": host(index), "colors": host(out_col), "normals": host(out_nor)}


def _visibility(points, depth, K, T, rel_tol, maps=None, min_depth=0.0, fill=POISON_NAN):
    """mvsn_cloud_visibility: numpy arrays of the three outputs."""
    n, (V, rows, cols) = len(points), depth.shape
    guard = Guard(_alloc, fill)
    p, d, Kd, Td = (guard.poisoned(_to(a)) for a in (points, depth, K, T))
    m = guard.poisoned(_to(maps)) if maps is not None else None
    C = maps.shape[1] if maps is not None else 0
    visible, count = guard.empty((n, V), torch.uint8, DEV), guard.empty((n,), torch.int32, DEV)
    values = guard.empty((n, C), torch.float32, DEV) if C else None
    lib = _native.load()
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_cloud_visibility(_native.ptr(p), n, _native.ptr(d), _native.ptr(m), C, _native.ptr(Kd),
                                                _native.ptr(Td), V, rows, cols, float(rel_tol), float(min_depth),
                                                _native.ptr(visible), _native.ptr(count), _native.ptr(values),
                                                _native.stream()), "mvsn_cloud_visibility")
    torch.cuda.synchronize()
    guard.check()
    return {"visible": visible.cpu().numpy(), "count": count.cpu().numpy(),
            "values": values.cpu().numpy() if C else None}


@functools.lru_cache(maxsize=None)
def _device(name, gathers=True, fill=POISON_NAN):
    """Made once per (case, gathers, poison), never modified."""
    c = cr.case(name)
    return _render(c["points"], c["K"], c["T"], c["rows"], c["cols"], fill=fill, **cr.render_args(c, gathers))


@functools.lru_cache(maxsize=None)
def _device_visibility(name, with_maps=True, fill=POISON_NAN):
    c = cr.visibility_case(name)
    return _visibility(c["points"], c["depth"], c["K"], c["T"], c["rel_tol"], c["maps"] if with_maps else None,
                       c.get("min_depth", 0.0), fill)


def _same_bits(a, b, keys):
    for key in keys:
        if b[key] is None:
            assert a[key] is None, key
            continue
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


def test_the_camera_batch_is_the_restatements():
    assert _native.load().mvsn_cloud_render_camera_batch() == cr.CAMERA_BATCH


# ---- the render: one point on a 1 x 1 map (a hit, and a miss that still writes 0 / -1 everywhere), the workgroup edge
# ---- (255, 256, 257 points; 5 x 7 and 33 x 65 pixels; one camera less than a batch, a batch, one more), 4099 rows on one
# ---- pixel in four orders, the rows that take no part, radius 0, 1, 2, 8 with clipped squares ---------------------------
@pytest.mark.parametrize("name", cr.RENDER_CASES)
def test_cases_match_the_restatement_byte_for_byte(name):
    _same_bits(_device(name), cr.case_reference(name), cr.RENDER_OUTPUTS)


@pytest.mark.parametrize("name", cr.RENDER_CASES)
def test_buffers_under_both_poisons(name):
    # (the guard bands of every buffer are checked inside _render; an element nobody writes, or a read of foreign memory
    # or of the uninitialised workspace that reaches a result, differs between the two fills)
    _same_bits(_device(name, True, POISON_NAN), _device(name, True, POISON_FINITE), cr.RENDER_OUTPUTS)


@pytest.mark.parametrize("name", ["one_hit", "one_miss", "edge_257_33_65_1", "edge_255_5_7_-1", "radius_2", "nonpart"])
def test_the_gathers_are_optional(name):
    got = _device(name, False)
    assert got["colors"] is None and got["normals"] is None
    _same_bits(got, cr.case_reference(name, False), cr.RENDER_OUTPUTS)
    c = cr.case(name)
    only = _render(c["points"], c["K"], c["T"], c["rows"], c["cols"], **dict(cr.render_args(c), normals=None))
    assert only["normals"] is None and only["colors"].tobytes() == cr.case_reference(name)["colors"].tobytes()
    only = _render(c["points"], c["K"], c["T"], c["rows"], c["cols"], **dict(cr.render_args(c), colors=None))
    assert only["colors"] is None and only["normals"].tobytes() == cr.case_reference(name)["normals"].tobytes()


def test_the_smallest_render_writes_every_output_on_a_miss():
    miss = _device("one_miss")
    assert miss["depth"].tolist() == [[[0.0]]] and miss["index"].tolist() == [[[-1]]]
    assert miss["colors"].reshape(-1).tolist() == [0, 0, 0] and miss["normals"].tobytes() == np.zeros(3, np.float32).tobytes()
    hit = _device("one_hit")
    assert hit["depth"].tolist() == [[[2.0]]] and hit["index"].tolist() == [[[0]]] and hit["colors"].reshape(-1).tolist() == [7, 8, 9]


@pytest.mark.parametrize("name", cr.CONTENTION_CASES + ["edge_256_33_65_0", "radius_8"])
def test_calling_twice_gives_the_same_bytes(name):
    c = cr.case(name)
    again = _render(c["points"], c["K"], c["T"], c["rows"], c["cols"], **cr.render_args(c))
    _same_bits(again, _device(name), cr.RENDER_OUTPUTS)


def test_the_lowest_row_wins_a_tie_and_the_nearest_point_wins_otherwise():
    assert _device("contention_equal")["index"][0, 2, 3] == 0
    for order in ("distinct", "ascending", "descending"):
        z = cr.case("contention_" + order)["points"][:, 2]
        got = _device("contention_" + order)
        assert got["index"][0, 2, 3] == np.argmin(z) and got["depth"][0, 2, 3] == z.min()
    near = _device("radius_1")
    assert near["index"][0, 16, 10] == cr.RADIUS_NEAR_ROW and _device("radius_0")["index"][0, 16, 10] == cr.RADIUS_FAR_ROW


def test_a_permuted_cloud_gives_the_same_depth_bytes():
    for name in ("edge_257_33_65_1", "radius_2", "contention_distinct"):
        c = cr.case(name)
        perm = cr.permutation(len(c["points"]))
        moved = _render(c["points"][perm], c["K"], c["T"], c["rows"], c["cols"], radius=c["radius"])
        base = _device(name)
        assert moved["depth"].tobytes() == base["depth"].tobytes(), name
        same = perm[moved["index"]] == base["index"]
        assert same[base["index"] >= 0].mean() > 0.99 and (moved["index"] >= 0).tobytes() == (base["index"] >= 0).tobytes()


# ---- the visibility ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.VISIBILITY_CASES)
def test_visibility_matches_the_restatement_byte_for_byte(name):
    got, ref = _device_visibility(name), cr.visibility_case_reference(name)
    _same_bits(got, ref, cr.VISIBILITY_OUTPUTS)
    assert set(np.unique(got["visible"]).tolist()) <= {0, 1}
    assert got["count"].tolist() == got["visible"].sum(axis=1).tolist()             # count = the row sums of visible


@pytest.mark.parametrize("name", cr.VISIBILITY_CASES)
def test_visibility_buffers_under_both_poisons(name):
    _same_bits(_device_visibility(name, True, POISON_NAN), _device_visibility(name, True, POISON_FINITE),
               cr.VISIBILITY_OUTPUTS)


@pytest.mark.parametrize("name", ["occlusion", "channels_16", "bad_depth"])
def test_visibility_without_maps_is_the_same_visibility(name):
    got = _device_visibility(name, False)
    assert got["values"] is None
    _same_bits(got, cr.visibility_case_reference(name), ("visible", "count"))


@pytest.mark.parametrize("name", ["edge_257_33_65_1", "edge_255_5_7_-1", "radius_0", "contention_equal", "nonpart"])
def test_every_rendered_row_is_visible_against_its_own_render_with_no_tolerance(name):
    """The exact property, on the device end to end: the visibility kernel forms the bits of z that the render stored."""
    c = cr.case(name)
    lo, hi = c.get("min_depth", 0.0), c.get("max_depth", np.inf)
    rendered = _render(c["points"], c["K"], c["T"], c["rows"], c["cols"], radius=0, min_depth=lo, max_depth=hi)
    vis = _visibility(c["points"], rendered["depth"], c["K"], c["T"], 0.0, min_depth=lo)
    assert (rendered["index"] >= 0).any()
    for v in range(len(c["K"])):
        rows = rendered["index"][v][rendered["index"][v] >= 0]
        assert vis["visible"][rows, v].all(), v


def test_the_far_plane_is_visible_exactly_inside_the_hole():
    c, got = cr.visibility_case("occlusion"), _device_visibility("occlusion")
    c0, c1, r0, r1 = cr.OCCLUSION_HOLE
    col, row = np.floor(c["pixel_x"] + 0.5), np.floor(c["pixel_y"] + 0.5)
    inside = (col >= c0) & (col < c1) & (row >= r0) & (row < r1)
    assert got["visible"][:, 0].astype(bool).tolist() == inside.tolist() and got["count"].sum() == inside.sum() > 0


def test_the_tolerance_boundary_and_the_bad_depths():
    assert _device_visibility("rel_tol")["visible"][:, 0].tolist() == [1, 0, 1, 1]
    bad = _device_visibility("bad_depth")
    assert bad["visible"].tolist() == [[0, 1, 1], [0, 1, 1], [0, 0, 1], [0, 0, 1], [1, 1, 1], [1, 0, 1], [1, 1, 1], [1, 1, 0]]
    assert np.isfinite(bad["values"]).all()


# ---- the Python interface ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    s = synthetic.fusion_scene(3, 48, 64)
    nb = np.array([[1, 2], [0, 2], [0, 1]])
    dev = {k: v.to(DEV) for k, v in s.items()}
    # (min_consistent = 0 keeps the pixels that no other view confirms: the points that only their own view sees)
    res = fuse_depthmaps(dev["depth"], dev["K"], dev["T_cam_in_world"], nb, images=dev["images"], min_consistent=0)
    return s, dev, res


def test_the_python_calls_are_the_library_calls_on_the_scene():
    s, dev, res = _scene()
    points = res.points.cpu().numpy()
    assert len(points) > 3000
    K, T = s["K"].numpy(), s["T_cam_in_world"].numpy()
    normals = np.random.default_rng(2).standard_normal(points.shape).astype(np.float32)
    for radius in (0, 1):
        r = cloud_render(res.points, dev["K"], dev["T_cam_in_world"], (48, 64), radius=radius, colors=res.colors,
                         normals=_to(normals), min_depth=0.5, max_depth=50.0)
        assert isinstance(r, CloudRender) and r.depth.shape == (3, 1, 48, 64) and r.index.shape == (3, 48, 64)
        ref = cr.render_reference(points, K, T, 48, 64, radius, res.colors.cpu().numpy(), normals, 0.5, 50.0)
        got = {"depth": r.depth[:, 0].cpu().numpy(), "index": r.index.cpu().numpy(), "colors": r.colors.cpu().numpy(),
               "normals": r.normals.cpu().numpy()}
        _same_bits(got, ref, cr.RENDER_OUTPUTS)
        assert (got["index"] >= 0).mean() > 0.5
    bare = cloud_render(res.points, dev["K"].double(), dev["T_cam_in_world"].double(), (48, 64))
    assert bare.colors is None and bare.normals is None
    # the visibility against the scene's own depth maps, with the images as maps
    vis = cloud_visibility(res.points, dev["depth"], dev["K"], dev["T_cam_in_world"], maps=dev["images"])
    assert isinstance(vis, CloudVisibility) and vis.visible.dtype == torch.bool and vis.visible.shape == (len(points), 3)
    ref = cr.visibility_reference(points, s["depth"][:, 0].numpy(), K, T, 0.01, s["images"].numpy())
    got = {"visible": vis.visible.cpu().numpy().view(np.uint8), "count": vis.count.cpu().numpy(),
           "values": vis.values.cpu().numpy()}
    _same_bits(got, ref, cr.VISIBILITY_OUTPUTS)
    assert cloud_visibility(res.points, dev["depth"], dev["K"], dev["T_cam_in_world"]).values is None
    # every row of an R = 0 render is visible against it with no tolerance
    own = cloud_visibility(res.points, bare.depth, dev["K"], dev["T_cam_in_world"], rel_tol=0.0)
    for v in range(3):
        rows = bare.index[v][bare.index[v] >= 0]
        assert bool(own.visible[rows, v].all())


def test_colorize_reproduces_the_fusions_colours_where_the_points_own_view_sees_them():
    s, dev, res = _scene()
    colors, count = cloud_colorize(res.points, dev["images"], dev["depth"], dev["K"], dev["T_cam_in_world"])
    assert colors.shape == res.colors.shape and colors.dtype == torch.uint8 and count.dtype == torch.int32
    vis = cloud_visibility(res.points, dev["depth"], dev["K"], dev["T_cam_in_world"], maps=dev["images"])
    want = cr.colorize_reference(vis.values.cpu().numpy(), vis.count.cpu().numpy())
    assert colors.cpu().numpy().tobytes() == want.tobytes() and torch.equal(count, vis.count)
    # count == 1 and the one view is the point's own: the same nearest pixel, the same conversion, a mean of one sample
    rows = torch.arange(len(res.points), device=DEV)
    mine = (count == 1) & vis.visible[rows, res.view.long()]
    assert int(mine.sum()) > 0
    assert torch.equal(colors[mine], res.colors[mine])
    assert not colors[count == 0].any()
