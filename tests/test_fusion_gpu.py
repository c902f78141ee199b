"""Depth-map fusion on the device (csrc/mvsn_fusion.hip) against the float64 restatement (tests/fusion_reference.py),
and reconstruct() against its own composition.  The scenes also go through the C ABI with their inputs in poisoned
buffers and the workspace and every output between guard bands (`device_fuse`, `fuse_between_bands`); the exact
scenes, the planted values and mvsn_fusion_gather are in tests/test_fusion_entries_gpu.py."""
import numpy as np
import pytest
import torch

from fusion_reference import fuse_reference, nearest_neighbours
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard, bits_equal
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd.fusion import FusionResult, frame_pair_poses, fuse_depthmaps, reconstruct

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _compare(got: FusionResult, ref, images, T_cam_in_world, views, max_margin):
    count = got.count.cpu().numpy().astype(np.int64)
    margin = ref["margin"]
    diff = count != ref["count"]
    assert not (diff & ~margin).any(), np.argwhere(diff & ~margin)[:10]
    # margin pixels: a decision of the restatement within 1e-4 (relative) of flipping
    assert margin.sum() <= max_margin * margin.size, margin.sum()
    same = ~diff & ref["keep"]
    fused = got.depth.cpu().numpy().astype(np.float64)
    assert (fused[~ref["keep"] & ~diff] == 0).all()
    rel = np.abs(fused[same] - ref["fused"][same]) / ref["fused"][same]
    assert rel.max() < 1e-5, rel.max()
    # points by their (view, pixel) key: the key lists agree but for margin pixels, in the same order
    H, W = count.shape[-2:]
    key_g = got.view.cpu().numpy().astype(np.int64) * H * W + got.pixel.cpu().numpy()
    key_r = ref["view"] * H * W + ref["pixel"]
    shared, ig, ir = np.intersect1d(key_g, key_r, return_indices=True)
    order_g, order_r = np.argsort(ig, kind="stable"), np.argsort(ir, kind="stable")
    assert (order_g == order_r).all()                       # the shared entries come in the same order
    extra = np.setdiff1d(np.union1d(key_g, key_r), shared)
    row = {v: i for i, v in enumerate(views)}
    for k in extra:
        v, p = divmod(int(k), H * W)
        assert margin[row[v], 0].reshape(-1)[p], (v, p)
    # (points of margin pixels whose count differs are left out: one more or one fewer depth in their average)
    rows_ = np.array([row[int(v)] for v in ref["view"][ir]], np.int64)
    agree = ~diff.reshape(len(views), -1)[rows_, ref["pixel"][ir]]
    ig, ir = ig[agree], ir[agree]
    pts = got.points.cpu().numpy().astype(np.float64)[ig]
    # within 1e-5 of the point's distance from its camera (= depth times the ray's length: the fused depth's 1e-5)
    centres = np.stack([cam[:3, 3] for cam in T_cam_in_world.double().numpy()])[ref["view"][ir]]
    err = np.linalg.norm(pts - ref["points"][ir], axis=1) / np.linalg.norm(ref["points"][ir] - centres, axis=1)
    print(f"fusion against the restatement: {len(shared)} shared points, {int(margin.sum())} margin pixels of "
          f"{margin.size}, {int(diff.sum())} counts differ, fused depth error / 1e-5 max {rel.max() / 1e-5:.3f}, "
          f"point error / 1e-5 max {err.max() / 1e-5:.3f}")
    assert err.max() < 1e-5, err.max()
    if images is not None:
        np.testing.assert_array_equal(got.colors.cpu().numpy()[ig], ref["colors"][ir])
    else:
        assert got.colors is None
    return len(shared)


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def device_fuse(depth, K, T_cam_in_world, neighbours, *, images=None, valid=None, ref_views=None, max_reproj_px=1.0,
                max_rel_depth=0.01, min_consistent=2, fill=POISON_NAN):
    """mvsn_fusion_consistency then mvsn_fusion_emit through the C ABI: every input in a poisoned buffer of its own
    (16-byte aligned only), the workspace, `total` and every output carved between guard bands, the bands checked after
    the emit.  Arguments as fuse_depthmaps' (tensors or arrays, on the host); a FusionResult of device tensors."""
    depth = torch.as_tensor(depth)
    V, _, H, W = depth.shape
    nb = np.asarray(neighbours, np.int64)
    R, M = nb.shape
    refs = np.arange(V) if ref_views is None else np.asarray(ref_views, np.int64)
    assert refs.shape == (R,) and 1 <= M <= 32 and ((0 <= refs) & (refs < V)).all() and ((-1 <= nb) & (nb < V)).all()
    guard = Guard(_alloc, fill)
    put = lambda a, dtype: guard.poisoned(torch.as_tensor(a).to(dtype).contiguous().to(DEV))   # noqa: E731
    d, k, t = put(depth, torch.float32), put(K, torch.float32), put(T_cam_in_world, torch.float32)
    m = put(valid, torch.uint8) if valid is not None else None
    im = put(images, torch.float32) if images is not None else None
    rv, nbd = put(refs, torch.int32), put(nb, torch.int32)
    lib = _native.load()
    ws_bytes = lib.mvsn_fusion_workspace_bytes(R, M, H, W)
    assert ws_bytes > 0
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    fused, count = guard.empty((R, 1, H, W), torch.float32, DEV), guard.empty((R, 1, H, W), torch.uint8, DEV)
    total = guard.empty((1,), torch.int64, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_fusion_consistency(
            _native.ptr(d), _native.ptr(m), _native.ptr(k), _native.ptr(t), _native.ptr(rv), _native.ptr(nbd), V, R, M, H,
            W, float(max_reproj_px), float(max_rel_depth), int(min_consistent), _native.ptr(fused), _native.ptr(count),
            _native.ptr(total), _native.ptr(ws), ws_bytes, st), "mvsn_fusion_consistency")
        n = int(total.item())
        assert 0 <= n <= R * H * W, n
        points = guard.empty((n, 3), torch.float32, DEV)
        colors = guard.empty((n, 3), torch.uint8, DEV) if images is not None else None
        view, pixel = guard.empty((n,), torch.int32, DEV), guard.empty((n,), torch.int32, DEV)
        _native.check(lib.mvsn_fusion_emit(
            _native.ptr(fused), _native.ptr(im), _native.ptr(rv), R, H, W, M, _native.ptr(ws), ws_bytes, n,
            _native.ptr(points), _native.ptr(colors), _native.ptr(view), _native.ptr(pixel), st), "mvsn_fusion_emit")
    torch.cuda.synchronize()
    guard.check()
    return FusionResult(points, colors, view, pixel, fused, count)


def same_bits(a: FusionResult, b: FusionResult):
    for name, x, y in zip(FusionResult._fields, a, b):
        assert (x is None and y is None) or bits_equal(x, y), name


def fuse_between_bands(*args, **kwargs):
    """device_fuse under both poisons (an element nobody writes, or a read of foreign memory that reaches a result,
    differs between them) and the Python entry on the same inputs: one result, the same bits three times."""
    a = device_fuse(*args, fill=POISON_NAN, **kwargs)
    same_bits(a, device_fuse(*args, fill=POISON_FINITE, **kwargs))
    dev = lambda x: None if x is None else torch.as_tensor(x).to(DEV)   # noqa: E731
    depth, K, T, nb = args
    py = {k: (dev(v) if k in ("images", "valid") else v) for k, v in kwargs.items()}
    same_bits(a, fuse_depthmaps(dev(depth).float(), dev(K).float(), dev(T).float(), nb, **py))
    return a


def test_fusion_matches_the_restatement_on_the_analytic_scene():
    sc = synthetic.fusion_scene(6, 96, 128)
    nb = nearest_neighbours(6, 5)
    ref = fuse_reference(sc["depth"], sc["K"], sc["T_cam_in_world"], nb, images=sc["images"])
    got = fuse_depthmaps(sc["depth"].to(DEV), sc["K"].to(DEV), sc["T_cam_in_world"].to(DEV), nb,
                         images=sc["images"].to(DEV))
    # (59 margin pixels of 73728 here: projections within 1e-4 * u of an integer column next to the image edge)
    assert _compare(got, ref, sc["images"], sc["T_cam_in_world"], range(6), 1e-3) > 0.8 * 6 * 96 * 128
    banded = fuse_between_bands(sc["depth"], sc["K"], sc["T_cam_in_world"], nb, images=sc["images"])
    _compare(banded, ref, sc["images"], sc["T_cam_in_world"], range(6), 1e-3)


def anisotropic_scene(V=6, H=90, W=150, device="cpu"):
    """The analytic scene through cameras real calibrations have: fy = 1.137 fx (0.83 fx for the odd views), principal
    points well off the centre and different from view to view, a non-square image -- a kernel that read fx for fy,
    cx for cy, W for H or one view's K for another's would project to other pixels."""
    K = synthetic.fusion_scene_intrinsics(V, H, W)
    for v in range(V):
        K[v, 1, 1] = K[v, 0, 0] * (1.137 if v % 2 == 0 else 0.83)
        K[v, 0, 2] += 13.25 - 3.5 * v
        K[v, 1, 2] += -7.6 + 2.25 * v
    return synthetic.fusion_scene(V, H, W, device=device, K=K)


def test_fusion_with_anisotropic_off_centre_cameras_matches_the_restatement():
    sc = anisotropic_scene()
    assert (sc["K"][:, 0, 0] != sc["K"][:, 1, 1]).all() and not torch.equal(sc["K"][0], sc["K"][1])
    nb = nearest_neighbours(6, 5)
    ref = fuse_reference(sc["depth"], sc["K"], sc["T_cam_in_world"], nb, images=sc["images"])
    got = fuse_depthmaps(sc["depth"].to(DEV), sc["K"].to(DEV), sc["T_cam_in_world"].to(DEV), nb,
                         images=sc["images"].to(DEV))
    shared = _compare(got, ref, sc["images"], sc["T_cam_in_world"], range(6), 1e-3)
    print(f"anisotropic fusion: {shared} shared points, {int(ref['margin'].sum())} margin pixels of {ref['margin'].size}, "
          f"{int((got.count.cpu().numpy() != ref['count']).sum())} counts differ")
    assert shared > 0.6 * 6 * 90 * 150
    banded = fuse_between_bands(sc["depth"], sc["K"], sc["T_cam_in_world"], nb, images=sc["images"])
    _compare(banded, ref, sc["images"], sc["T_cam_in_world"], range(6), 1e-3)


def test_fusion_odd_size_padding_valid_mask_and_ref_subset():
    V, H, W = 6, 97, 131
    sc = synthetic.fusion_scene(V, H, W)
    gen = torch.Generator().manual_seed(7)
    valid = torch.rand(V, 1, H, W, generator=gen) > 0.05
    depth = sc["depth"].clone()
    depth[1, :, 40:50, 60:80] = 0.0                               # a hole: taps with no depth
    refs = [4, 1, 3]
    nb = np.array([[3, 5, -1, 2], [-1, 0, 2, 3], [2, -1, 4, -1]])
    ref = fuse_reference(depth, sc["K"], sc["T_cam_in_world"], nb, images=sc["images"], valid=valid, ref_views=refs)
    got = fuse_depthmaps(depth.to(DEV), sc["K"].to(DEV), sc["T_cam_in_world"].to(DEV), nb, images=sc["images"].to(DEV),
                         valid=valid.to(DEV), ref_views=refs)
    assert got.depth.shape == (3, 1, H, W) and got.count.dtype == torch.uint8
    # (444 margin pixels of 38121: with 5 % of the pixels invalid, most integer crossings of (u, v) change whether
    # all four taps are valid)
    assert _compare(got, ref, sc["images"], sc["T_cam_in_world"], refs, 0.02) > 0.3 * 3 * H * W
    # without images: no colours, the same points
    bare = fuse_depthmaps(depth.to(DEV), sc["K"].to(DEV), sc["T_cam_in_world"].to(DEV), nb, valid=valid.to(DEV),
                          ref_views=refs)
    assert bare.colors is None and torch.equal(bare.points, got.points)
    for images in (sc["images"], None):
        banded = fuse_between_bands(depth, sc["K"], sc["T_cam_in_world"], nb, images=images, valid=valid, ref_views=refs)
        _compare(banded, ref, images, sc["T_cam_in_world"], refs, 0.02)


def test_fusion_more_workgroup_counts_than_scan_threads():
    # 88 references x ceil(96 * 128 / 1024) = 88 x 12 = 1056 kept-pixel counts for the scan's 1024 threads: every thread
    # owns a run of ceil(1056 / 1024) = 2 counts and the last 496 threads own none.  Many views of the first test's
    # size, not a few large ones: _compare's 1e-5 on the fused depth is a bound for images of this size (the fp32 error
    # of a projected coordinate grows with the coordinate, and an interpolated depth moves by its slope times that:
    # 3 views of 600 x 600 reach 1.8e-5 at the sphere's silhouette).  The cameras span the usual arc, so the neighbours
    # are 17 and 34 views away: the angles of the first test's views.
    V, H, W = 88, 96, 128
    sc = synthetic.fusion_scene(V, H, W)
    nb = np.array([[v + 17, v + 34] if v < V // 2 else [v - 17, v - 34] for v in range(V)])
    ref = fuse_reference(sc["depth"], sc["K"], sc["T_cam_in_world"], nb, images=sc["images"])
    got = fuse_depthmaps(sc["depth"].to(DEV), sc["K"].to(DEV), sc["T_cam_in_world"].to(DEV), nb,
                         images=sc["images"].to(DEV))
    assert got.depth.shape == (V, 1, H, W) and V * (-(-H * W // 1024)) == 1056
    assert got.points.shape[0] == int((got.depth > 0).sum())
    # (368 margin pixels of 1081344 in the restatement)
    shared = _compare(got, ref, sc["images"], sc["T_cam_in_world"], range(V), 1e-3)
    print(f"1056 counts: {shared} shared points of {got.points.shape[0]}, {int(ref['margin'].sum())} margin pixels")
    assert shared > 0.8 * V * H * W
    banded = fuse_between_bands(sc["depth"], sc["K"], sc["T_cam_in_world"], nb, images=sc["images"])
    _compare(banded, ref, sc["images"], sc["T_cam_in_world"], range(V), 1e-3)


def test_fusion_is_deterministic():
    sc = synthetic.fusion_scene(6, 96, 128, device=DEV)
    nb = nearest_neighbours(6, 4)
    a = fuse_depthmaps(sc["depth"], sc["K"], sc["T_cam_in_world"], nb, images=sc["images"])
    b = fuse_depthmaps(sc["depth"], sc["K"], sc["T_cam_in_world"], nb, images=sc["images"])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_fusion_empty_result():
    sc = synthetic.fusion_scene(4, 64, 96, device=DEV)
    nb = nearest_neighbours(4, 2)
    got = fuse_depthmaps(sc["depth"], sc["K"], sc["T_cam_in_world"], nb, images=sc["images"], min_consistent=3)
    torch.cuda.synchronize()
    assert got.points.shape == (0, 3) and got.colors.shape == (0, 3)
    assert got.view.shape == (0,) and got.pixel.shape == (0,)
    assert float(got.depth.abs().sum()) == 0.0 and int(got.count.max()) <= 2


@pytest.fixture(scope="module")
def net():
    from multi_view_stereonet_amd import MultiViewStereoNet
    from multi_view_stereonet_amd.weights import load_weights
    torch.set_grad_enabled(False)
    m = MultiViewStereoNet()
    m.load_state_dict(load_weights("gta_sfm_150epochs"), strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("batch", [2, 6])     # 2 x 3 sources: recorded plans; 6 x 3 = 18 chains: eager forward
def test_reconstruct_is_its_composition(net, batch):
    from multi_view_stereonet_amd import metrics
    from multi_view_stereonet_amd import multi_view_stereonet_utils as snu
    V, S, D = 6, 3, 16
    sc = synthetic.fusion_scene(V, 64, 128, device=DEV)
    nb = nearest_neighbours(V, S)
    res, depth = reconstruct(net, sc["images"], sc["K"], sc["T_cam_in_world"], nb, num_idepth_samples=D, batch=batch,
                             max_rel_depth=0.05, min_consistent=1)
    # by hand: DataLoader-style batches, unpack, the 7-argument forward, idepth -> depth, one fusion
    depths = []
    for lo in range(0, V, batch):
        ref = list(range(lo, min(lo + batch, V)))
        frames = {"left_image": sc["images"][ref], "right_image": [sc["images"][nb[ref, s].tolist()] for s in range(S)],
                  "K": sc["K"].cpu()[ref].unsqueeze(1).contiguous(),
                  "T_right_in_left": [frame_pair_poses(sc["T_cam_in_world"], ref, nb[ref, s]) for s in range(S)]}
        inputs = snu.multi_view_unpack_batch(frames, DEV, net.num_levels)
        out = net(inputs["left_image_pyr"], inputs["K_pyr"], inputs["T_right_in_left"], inputs["right_image_pyr"], D,
                  True, [True] * 5)
        depths.append(metrics.idepth_to_depth(out["left_idepthmap_pyr"][0], inputs["baseline"]))
    want_depth = torch.cat(depths, 0)
    assert torch.equal(depth, want_depth)
    want = fuse_depthmaps(want_depth, sc["K"], sc["T_cam_in_world"], nb, images=sc["images"], max_rel_depth=0.05,
                          min_consistent=1)
    for x, y in zip(res, want):
        assert torch.equal(x, y)
    assert res.points.shape[0] > 0


def test_reconstruct_rejects_a_zero_baseline(net):
    sc = synthetic.fusion_scene(3, 64, 128, device=DEV)
    T = sc["T_cam_in_world"].clone()
    T[1] = T[0]                                   # view 1 sits on view 0: zero baseline for view 0's first source
    with pytest.raises(AssertionError, match="baseline"):
        reconstruct(net, sc["images"], sc["K"], T, np.array([[1, 2], [0, 2], [1, 0]]), num_idepth_samples=8)
