"""Normals from depth maps on the device (csrc/mvsn_normals.hip) against the numpy restatement (tests/normals_reference.py):
the defined mask exactly, unit length, the angle within the derived per-pixel bound; inputs in poisoned buffers and the
output between guard bands; point_normals against plain indexing, voxel_normals against the integer restatement, and
reconstruct(with_normals=True) against its own composition."""
import functools

import numpy as np
import pytest
import torch

from fusion_reference import nearest_neighbours
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard, bits_equal
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd.fusion import (depth_normals, fuse_depthmaps, point_normals, reconstruct, voxel_merge,
                                             voxel_normals)
from normals_reference import EPS, angle, normals_reference, voxel_normals_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# W = 61: no multiple of 4; (1,3,5): one short row per thread; (2,2,1029): a workgroup boundary (1024 pixels) inside a row
SHAPES = [(3, 37, 61), (4, 48, 64), (1, 3, 5), (2, 2, 1029)]
INF = float("inf")


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


@functools.lru_cache(maxsize=None)
def _scene(shape, own_K=False):
    """depth (V,H,W), K, T_cam_in_world as numpy arrays: made once per shape, never modified."""
    V, H, W = shape
    K = None
    if W < 16:                                                          # (the scene's focal length of 0.8 W would put
        K = synthetic.fusion_scene_intrinsics(V, H, W)                  # neighbouring rays of a 5-pixel row more than
        K[:, 0, 0] = K[:, 1, 1] = 51.2                                  # max_rel_step apart in depth)
    if own_K:                                                           # fx != fy, off-centre, a camera per view
        K = synthetic.fusion_scene_intrinsics(V, H, W)
        for v in range(V):
            K[v, 0, 0] *= 1.0 + 0.07 * (v + 1)
            K[v, 1, 1] *= 0.9 - 0.04 * v
            K[v, 0, 2] += 2.25 + v
            K[v, 1, 2] -= 1.5 + 0.5 * v
    sc = synthetic.fusion_scene(V, H, W, K=K)
    return sc["depth"][:, 0].numpy(), sc["K"].numpy(), sc["T_cam_in_world"].numpy()


def _holes(shape):
    """A checkerboard with holes: the checkerboard (top-left part) leaves a valid pixel without any neighbour, the
    seeded holes elsewhere take one, two or three of them."""
    V, H, W = shape
    ys, xs = np.mgrid[0:H, 0:W]
    valid = np.random.default_rng(V * 1000 + W).random((V, H, W)) > 0.3
    board = (ys < (H + 1) // 2) & (xs < (W + 1) // 2)
    valid[:, board] = ((ys + xs) % 2 == 0)[board]
    return valid


def _device_normals(depth, K, valid=None, T=None, step=0.05, fill=POISON_NAN):
    """mvsn_depth_normals on inputs that sit in poisoned buffers of their own (16-byte aligned only), into an output
    carved between guard bands and poisoned too: a pixel that is not written keeps the poison."""
    V, H, W = depth.shape
    guard = Guard(_alloc, fill)
    put = lambda a, dtype: guard.poisoned(torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV))   # noqa: E731
    d, k = put(depth, torch.float32), put(K, torch.float32)
    m = put(valid, torch.uint8) if valid is not None else None
    t = put(T, torch.float32) if T is not None else None
    out = guard.empty((V, 3, H, W), torch.float32, DEV)
    lib = _native.load()
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_depth_normals(_native.ptr(d), _native.ptr(m), _native.ptr(k), _native.ptr(t), V, H, W,
                                             float(step), _native.ptr(out), _native.stream()), "mvsn_depth_normals")
    torch.cuda.synchronize()
    guard.check()
    return out.cpu().numpy()


def _compare(got, ref, what=""):
    assert not np.isnan(got).any() and np.isfinite(got).all(), "a pixel was not written, or a NaN came through"
    defined = (got != 0).any(axis=1)
    np.testing.assert_array_equal(defined, ref["defined"])              # exactly: no margin class
    if not defined.any():
        return 0.0
    n = got.transpose(0, 2, 3, 1)[defined].astype(np.float64)
    length = np.linalg.norm(n, axis=-1)
    err = angle(n, ref["normals"].transpose(0, 2, 3, 1)[defined])
    ratio = err / ref["bound"][defined]
    print(f"{what}: {defined.sum()} defined of {defined.size}, | |n| - 1 | max {np.abs(length - 1).max():.2e}, "
          f"angle max {err.max():.2e} rad, angle / bound max {ratio.max():.3f}")
    assert np.abs(length - 1).max() <= 4 * EPS, np.abs(length - 1).max()
    assert (err <= ref["bound"][defined]).all(), ratio.max()
    return ratio.max()


@pytest.mark.parametrize("posed", [False, True], ids=["camera", "world"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "holes"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_depth_normals_match_the_restatement(shape, masked, posed):
    depth, K, T = _scene(shape)
    valid = _holes(shape) if masked else None
    ref = normals_reference(depth, K, valid, T if posed else None, 0.05)
    if masked and shape[1] >= 37:
        # a condition on the mask: every combination of counting neighbours occurs at a usable pixel
        usable = (depth > 0) & valid
        codes = (ref["usable"] * np.array([1, 2, 4, 8])[:, None, None, None]).sum(0)[usable]
        assert set(np.unique(codes)) == set(range(16)), np.unique(codes)
    if not masked and shape[1] >= 37:
        assert ref["defined"].sum() >= 0.99 * (depth > 0).sum()
    got = _device_normals(depth, K, valid, T if posed else None, 0.05)
    _compare(got, ref, f"{shape} masked={masked} posed={posed}")


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 7), (2, 7, 1)], ids=lambda s: "x".join(map(str, s)))
def test_degenerate_shapes_give_zeros(shape):
    V, H, W = shape
    depth = np.full(shape, 2.0, np.float32)
    K = synthetic.fusion_scene_intrinsics(V, 8, 8).numpy()
    for step in (0.05, INF):
        got = _device_normals(depth, K, step=step)
        assert got.shape == (V, 3, H, W) and (got == 0).all()


def test_depth_normals_with_a_camera_of_its_own_per_view():
    shape = (3, 37, 61)
    depth, K, T = _scene(shape, True)
    assert (K[:, 0, 0] != K[:, 1, 1]).all() and len(set(K[:, 0, 2])) == 3
    for posed in (False, True):
        ref = normals_reference(depth, K, None, T if posed else None, 0.05)
        assert ref["defined"].sum() >= 0.99 * (depth > 0).sum()
        _compare(_device_normals(depth, K, None, T if posed else None, 0.05), ref, f"own K posed={posed}")


def test_holes_nan_and_infinite_depths():
    shape = (3, 37, 61)
    depth, K, T = _scene(shape)
    depth = depth.copy()
    spots = {"zero": (0, 10, 20), "negative": (1, 5, 7), "nan": (2, 30, 40), "inf": (0, 20, 33), "corner": (1, 0, 0),
             "last": (2, 36, 60)}
    depth[spots["zero"]], depth[spots["negative"]], depth[spots["nan"]] = 0.0, -3.0, np.nan
    depth[spots["inf"]], depth[spots["corner"]], depth[spots["last"]] = np.inf, np.nan, 0.0
    for step in (0.05, INF):
        ref = normals_reference(depth, K, None, T, step)
        got = _device_normals(depth, K, None, T, step)
        _compare(got, ref, f"holes step={step}")
        for v, y, x in spots.values():
            assert (got[v, :, y, x] == 0).all()
        # beside a hole the tangent is one-sided, as restated, and the normal is still there
        for name in ("zero", "negative", "nan", "inf"):
            v, y, x = spots[name]
            left, right, up, down = ref["usable"][:, v]
            assert not right[y, x - 1] and left[y, x - 1] and not left[y, x + 1] and right[y, x + 1], name
            assert not down[y - 1, x] and up[y - 1, x] and not up[y + 1, x] and down[y + 1, x], name
            for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                assert ref["defined"][v, yy, xx] and (got[v, :, yy, xx] != 0).any(), (name, yy, xx)


@pytest.mark.parametrize("fill", [POISON_NAN, POISON_FINITE], ids=["nan", "finite"])
def test_step_infinite_and_zero(fill):
    # with step = inf every usable neighbour counts: under the finite poison (1.3e36, a usable depth) a tap outside
    # the payload would count too, and change a border pixel
    shape = (3, 37, 61)
    depth, K, T = _scene(shape)
    valid = _holes(shape)
    ref = normals_reference(depth, K, valid, T, INF)
    assert (ref["usable"].sum(0)[ref["defined"]] >= 2).all()
    r_inf = _compare(_device_normals(depth, K, valid, T, INF, fill), ref, "step=inf")
    # step = 0: only a neighbour of exactly the same depth counts; terraces of constant depth have such neighbours
    terraces = (np.round(depth * 4.0) / 4.0).astype(np.float32)
    ref = normals_reference(terraces, K, None, None, 0.0)
    inside = ref["defined"].sum()
    assert 0.3 * terraces.size < inside < 0.99 * terraces.size
    r_zero = _compare(_device_normals(terraces, K, None, None, 0.0, fill), ref, "step=0")
    assert r_inf > 0 and r_zero >= 0
    # and on the analytic depth nearly nothing is defined at step = 0
    ref = normals_reference(depth, K, None, None, 0.0)
    _compare(_device_normals(depth, K, None, None, 0.0, fill), ref, "step=0 analytic")


def test_the_python_call_is_the_library_call():
    shape = (3, 37, 61)
    depth, K, T = _scene(shape)
    valid = _holes(shape)
    d = torch.from_numpy(depth).unsqueeze(1).to(DEV)
    k, t, m = torch.from_numpy(K).to(DEV), torch.from_numpy(T).to(DEV), torch.from_numpy(valid).unsqueeze(1).to(DEV)
    for kwargs, args in (({}, (None, None, 0.05)), ({"valid": m}, (valid, None, 0.05)),
                         ({"valid": m.to(torch.uint8), "T_cam_in_world": t, "max_rel_step": 0.1}, (valid, T, 0.1))):
        got = depth_normals(d, k, **kwargs)
        assert got.shape == (3, 3, 37, 61) and got.dtype == torch.float32 and got.device.type == "cuda"
        want = _device_normals(depth, K, *args)
        assert bits_equal(got.cpu(), torch.from_numpy(want))
    assert bits_equal(depth_normals(d, k), depth_normals(d, k))


# ---- point_normals, voxel_normals: a fused (4,48,64) scene, made once ----------------------------------------------
@pytest.fixture(scope="module")
def fused():
    sc = synthetic.fusion_scene(4, 48, 64, device=DEV)
    nb = nearest_neighbours(4, 3)
    res = fuse_depthmaps(sc["depth"], sc["K"], sc["T_cam_in_world"], nb, images=sc["images"])
    maps = depth_normals(sc["depth"], sc["K"], T_cam_in_world=sc["T_cam_in_world"])
    assert res.points.shape[0] > 4000
    return sc, nb, res, maps


def _indexed(maps, view, pixel):
    HW = maps.shape[2] * maps.shape[3]
    return maps.permute(0, 2, 3, 1).reshape(-1, 3)[view.long() * HW + pixel.long()]


def test_point_normals_are_the_maps_at_view_and_pixel(fused):
    sc, nb, res, maps = fused
    got = point_normals(res, maps)
    assert got.shape == (res.points.shape[0], 3) and got.dtype == torch.float32
    assert bits_equal(got, _indexed(maps, res.view, res.pixel))
    assert (got != 0).any(dim=1).float().mean() > 0.95
    # a subset of the views, in another order: the maps hold those views only
    refs = [2, 0]
    sub = fuse_depthmaps(sc["depth"], sc["K"], sc["T_cam_in_world"], nb[refs], images=sc["images"], ref_views=refs)
    assert set(sub.view.unique().tolist()) == {0, 2}
    got = point_normals(sub, maps[refs].contiguous(), ref_views=refs)
    assert bits_equal(got, _indexed(maps, sub.view, sub.pixel))
    # an index outside the maps: a NaN row, the others untouched
    view, pixel = res.view.clone(), res.pixel.clone()
    view[3], view[4], pixel[5], pixel[6] = 4, -1, 48 * 64, -1
    got = point_normals(res._replace(view=view, pixel=pixel), maps)
    bad = torch.zeros(len(view), dtype=torch.bool, device=DEV)
    bad[3:7] = True
    assert torch.isnan(got[bad]).all() and bits_equal(got[~bad], _indexed(maps, res.view, res.pixel)[~bad])


def test_voxel_normals_match_the_integer_restatement(fused):
    _, _, res, maps = fused
    pn = point_normals(res, maps)
    vc = voxel_merge(res.points, 0.25, colors=res.colors)
    n, m = pn.shape[0], vc.points.shape[0]
    assert 1 < m < n / 2
    got = voxel_normals(vc, pn)
    assert got.shape == (m, 3) and got.dtype == torch.float32
    want, sums = voxel_normals_reference(pn.cpu().numpy(), vc.inverse.cpu().numpy(), m)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64))
    print(f"{n} points, {m} voxels, max component difference {err.max():.3e}")
    assert err.max() <= 2.0 ** -22, err.max()
    assert bits_equal(got, voxel_normals(vc, pn))                       # two calls
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(9)).to(DEV)
    assert bits_equal(got, voxel_normals(vc._replace(inverse=vc.inverse[perm].contiguous()), pn[perm].contiguous()))
    # what does not count: the rows of three voxels zeroed, points taken out of the merge or sent to a row that is
    # not there, non-finite normals; a component beyond 1 is clamped
    pn2, inverse = pn.clone(), vc.inverse.clone()
    rows = torch.tensor([0, m // 2, m - 1], device=DEV)
    pn2[torch.isin(inverse, rows)] = 0.0
    inverse[10:20] = -1
    inverse[20:25] = m + 5
    pn2[30], pn2[31], pn2[32, 1], pn2[33] = float("nan"), float("inf"), float("-inf"), torch.tensor([5.0, -7.0, 0.25])
    got2 = voxel_normals(vc._replace(inverse=inverse), pn2)
    want2, sums2 = voxel_normals_reference(pn2.cpu().numpy(), inverse.cpu().numpy(), m)
    assert (sums2[rows.cpu().numpy()] == 0).all() and (got2[rows] == 0).all()
    assert np.abs(got2.cpu().numpy().astype(np.float64) - want2.astype(np.float64)).max() <= 2.0 ** -22
    assert torch.isfinite(got2).all()


def test_voxel_normals_entry_stays_inside_its_buffers():
    rng = np.random.default_rng(13)
    n, m = 5000, 37                                                     # m * 3 words: no multiple of the block
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    inverse = rng.integers(-1, m + 1, n)                                # -1 and m among them
    inverse[rng.random(n) < 0.5] = 7                                    # half of the points in one row: contention
    guard = Guard(_alloc, POISON_NAN)
    a = guard.poisoned(torch.from_numpy(nrm).to(DEV))
    i = guard.poisoned(torch.from_numpy(inverse).to(DEV))
    accum = guard.empty((m, 3), torch.int64, DEV)
    out = guard.empty((m, 3), torch.float32, DEV)
    lib = _native.load()
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_voxel_normals(_native.ptr(a), _native.ptr(i), n, m, _native.ptr(accum), _native.ptr(out),
                                             _native.stream()), "mvsn_voxel_normals")
    torch.cuda.synchronize()
    guard.check()
    want, sums = voxel_normals_reference(nrm, inverse, m)
    np.testing.assert_array_equal(accum.cpu().numpy(), sums)            # the integer sums are exact
    assert np.abs(out.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -22


# ---- reconstruct(with_normals=True) ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    from multi_view_stereonet_amd import MultiViewStereoNet
    from multi_view_stereonet_amd.weights import load_weights
    torch.set_grad_enabled(False)
    m = MultiViewStereoNet()
    m.load_state_dict(load_weights("gta_sfm_150epochs"), strict=True)
    return m.to(DEV).eval()


def test_reconstruct_with_normals_is_its_composition(net):
    V, S, D = 4, 2, 8
    sc = synthetic.fusion_scene(V, 64, 128, device=DEV)
    nb = nearest_neighbours(V, S)
    kwargs = dict(num_idepth_samples=D, batch=2, max_rel_depth=0.05, min_consistent=1)
    plain = reconstruct(net, sc["images"], sc["K"], sc["T_cam_in_world"], nb, **kwargs)
    got = reconstruct(net, sc["images"], sc["K"], sc["T_cam_in_world"], nb, with_normals=True,
                      normals_max_rel_step=0.1, **kwargs)
    assert len(plain) == 2 and len(got) == 3
    for x, y in zip(got[0], plain[0]):
        assert bits_equal(x, y)
    assert bits_equal(got[1], plain[1])
    res, depth, normals = got
    assert res.points.shape[0] > 0 and normals.shape == (res.points.shape[0], 3)
    want = point_normals(res, depth_normals(depth, sc["K"], T_cam_in_world=sc["T_cam_in_world"], max_rel_step=0.1))
    assert bits_equal(normals, want)
    # after the confidence: still the last element
    conf = reconstruct(net, sc["images"], sc["K"], sc["T_cam_in_world"], nb, with_confidence=True, with_normals=True,
                       **kwargs)
    assert len(conf) == 4 and conf[2].shape == (V, 1, 64, 128)
    assert bits_equal(conf[3], point_normals(conf[0], depth_normals(conf[1], sc["K"],
                                                                    T_cam_in_world=sc["T_cam_in_world"])))
