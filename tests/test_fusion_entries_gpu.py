"""The fusion entries of the C ABI (csrc/mvsn_fusion.hip: mvsn_fusion_consistency, mvsn_fusion_emit; mvsn_fusion_gather)
between guard bands, under both poisons and against the Python entry (test_fusion_gpu.py's harness), on the exact scenes
of tests/fusion_exact_cases.py -- counts equal, fused depths and points bit-equal to the closed form, no margin class --
and on values that are not depths."""
import functools

import numpy as np
import pytest
import torch

import fusion_exact_cases as fx
from fusion_reference import fuse_reference
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard, bits_equal
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd.fusion import FusionResult, point_values
from test_fusion_gpu import _alloc, _compare, fuse_between_bands

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fuse(case):
    K, T = fx.cameras(case)
    return fuse_between_bands(case.depth[:, None], K, T, case.neighbours, ref_views=case.ref_views,
                              valid=None if case.valid is None else case.valid[:, None],
                              max_reproj_px=case.max_reproj_px, max_rel_depth=case.max_rel_depth,
                              min_consistent=case.min_consistent)


def _equal(got: FusionResult, exp, what=""):
    """Equality with the closed form, everywhere: counts, the bits of the fused depths, the kept pixels in order, the
    bits of their points.  Two planted values are depths (> 0) and are kept under min_consistent = 0: a point of the
    infinite one has no position and only has to be non-finite; of the denormal one's point the z, the depth itself,
    is pinned (x and y are sums of products below the smallest denormal, whose rounding depends on the order)."""
    np.testing.assert_array_equal(got.count.cpu().numpy()[:, 0], exp["count"], err_msg=what)
    np.testing.assert_array_equal(_bits(got.depth.cpu().numpy()[:, 0]), _bits(exp["fused"]), err_msg=what)
    np.testing.assert_array_equal(got.view.cpu().numpy(), exp["view"], err_msg=what)
    np.testing.assert_array_equal(got.pixel.cpu().numpy(), exp["pixel"], err_msg=what)
    pts = got.points.cpu().numpy()
    f = exp["fused"][exp["keep"]]
    finite = np.isfinite(f)
    normal = finite & (f >= 2.0 ** -126)
    np.testing.assert_array_equal(_bits(pts[normal]), _bits(exp["points"][normal]), err_msg=what)
    np.testing.assert_array_equal(_bits(pts[finite, 2]), _bits(f[finite]), err_msg=what)
    assert not np.isfinite(pts[~finite]).all(1).any(), what
    assert got.colors is None


@pytest.mark.parametrize("name", sorted(fx.CASES))
def test_exact_scene_equals_its_closed_form(name):
    case = fx.CASES[name]
    got = _fuse(case)
    _equal(got, fx.closed_form(case), name)
    if name.endswith("threshold_zero") or name == "min_consistent_M_plus_1":
        assert got.points.shape == (0, 3) and float(got.depth.abs().sum()) == 0.0      # (the emit is not launched)
    if name == "slots_32":
        assert int(got.count.max()) == 32


def test_65535_references():
    # the scan owns 65535 kept-pixel counts, 64 per thread (one workgroup per reference: 3 x 5 pixels); the expected
    # output is the two-reference result, itself equal to its closed form (above), tiled
    case = fx.CASES["two_references"]
    R = fx.MANY_REFERENCES
    many = case._replace(ref_views=np.resize(case.ref_views, R), neighbours=np.resize(case.neighbours, (R, 1)))
    exp = fx.closed_form(case)
    got = _fuse(many)
    reps = lambda a: np.resize(a, (R,) + a.shape[1:])   # noqa: E731  (rows 0, 1, 0, 1, ... 0)
    np.testing.assert_array_equal(got.count.cpu().numpy()[:, 0], reps(exp["count"]))
    np.testing.assert_array_equal(_bits(got.depth.cpu().numpy()[:, 0]), _bits(reps(exp["fused"])))
    n = [int(exp["keep"][i].sum()) for i in range(2)]
    assert n[0] > 0 and n[1] > 0 and n[0] != n[1]
    split = np.cumsum([n[0], n[1]])
    per_view = [np.split(exp[k], split)[:2] for k in ("view", "pixel", "points")]
    for k, parts in zip(("view", "pixel", "points"), per_view):
        want = np.concatenate([parts[i % 2] for i in range(R)])
        g = getattr(got, k).cpu().numpy()
        if k == "points":
            np.testing.assert_array_equal(_bits(g), _bits(want))
        else:
            np.testing.assert_array_equal(g, want)


# ---- values that are not depths --------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_consistent", [0, 1])
@pytest.mark.parametrize("name", ["baseline_x", "shifted", "shape_25x41_baseline"])
def test_planted_values_in_the_exact_scenes(name, min_consistent):
    case = fx.CASES[name]._replace(min_consistent=min_consistent)
    for what, view, pixel, planted in fx.plants(case):
        _equal(_fuse(planted), fx.closed_form(planted), what)


@functools.lru_cache(maxsize=None)
def _analytic(what):
    sc = fx.analytic_scene()
    depth = sc["depth"] if what is None else fx.analytic_plants()[what][0]
    ref = fuse_reference(depth, sc["K"], sc["T_cam_in_world"], sc["neighbours"], images=sc["images"])
    got = fuse_between_bands(depth, sc["K"], sc["T_cam_in_world"], sc["neighbours"], images=sc["images"])
    return ref, got


@pytest.mark.parametrize("what", sorted(fx.NOT_DEPTHS))
def test_planted_values_in_the_analytic_scene(what):
    sc = fx.analytic_scene()
    ref, got = _analytic(what)
    print(what, end=": ")
    _compare(got, ref, sc["images"], sc["T_cam_in_world"], range(4), 1e-3)
    _, base = _analytic(None)
    spots = fx.analytic_plants()[what][1]
    reach = torch.from_numpy(fx.analytic_reach(spots)).to(DEV)
    assert bits_equal(got.depth[~reach], base.depth[~reach]) and torch.equal(got.count[~reach], base.count[~reach])
    assert torch.isfinite(got.depth).all() and torch.isfinite(got.points).all()
    for view, pixel in spots:
        assert int(got.count[view].view(-1)[pixel]) == 0 and float(got.depth[view].view(-1)[pixel]) == 0.0


def test_the_analytic_scene_without_plants():
    sc = fx.analytic_scene()
    ref, got = _analytic(None)
    assert _compare(got, ref, sc["images"], sc["T_cam_in_world"], range(4), 1e-3) > 0.5 * 4 * 48 * 64


# ---- mvsn_fusion_gather ----------------------------------------------------------------------------------------------
def _device_gather(maps, view, pixel, fill):
    guard = Guard(_alloc, fill)
    m = guard.poisoned(torch.from_numpy(maps).to(DEV))
    v, p = guard.poisoned(torch.from_numpy(view).to(DEV)), guard.poisoned(torch.from_numpy(pixel).to(DEV))
    out = guard.empty((len(view),), torch.float32, DEV)
    with torch.cuda.device(DEV):
        _native.check(_native.load().mvsn_fusion_gather(_native.ptr(m), _native.ptr(v), _native.ptr(p), maps.shape[0],
                                                        maps.shape[2] * maps.shape[3], len(view), _native.ptr(out),
                                                        _native.stream()), "mvsn_fusion_gather")
    torch.cuda.synchronize()
    guard.check()
    return out


@pytest.mark.parametrize("count", [1, 255, 256, 257, 1000])
def test_gather_between_bands(count):
    V, H, W = 3, 5, 7
    HW = H * W
    rng = np.random.default_rng(count)
    maps = rng.standard_normal((V, 1, H, W)).astype(np.float32)
    maps[1, 0, 2, 3], maps[2, 0, 4, 6] = np.nan, np.inf                  # values come through as they are
    view, pixel = rng.integers(0, V, count).astype(np.int32), rng.integers(0, HW, count).astype(np.int32)
    view[0], pixel[0], view[-1], pixel[-1] = 0, 0, V - 1, HW - 1         # the first and the last element of the maps
    outside = [(-1, 0), (V, 0), (2 ** 31 - 1, 0), (-2 ** 31, 0), (0, -1), (V - 1, HW), (0, 2 ** 31 - 1), (1, -2 ** 31),
               (-1, -1), (V, HW), (2 ** 31 - 1, 2 ** 31 - 1)]
    rows = rng.choice(np.arange(1, count - 1), min(len(outside), max(count - 2, 0)), replace=False)
    for i, (v, p) in zip(rows, outside):
        view[i], pixel[i] = v, p
    want = np.full(count, np.nan, np.float32)
    inside = (view >= 0) & (view < V) & (pixel >= 0) & (pixel < HW)
    want[inside] = maps.reshape(V, HW)[view[inside], pixel[inside]]
    assert inside[0] and (count < 3 or (~inside).sum() == len(rows))
    a = _device_gather(maps, view, pixel, POISON_NAN)
    b = _device_gather(maps, view, pixel, POISON_FINITE)                 # an out-of-bounds read would give 1.3e36 here
    assert bits_equal(a, b)
    got = a.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(_bits(got[inside]), _bits(want[inside]))
    # the Python entry on the rows it accepts (every index inside: it is given the fusion's own view and pixel)
    res = FusionResult(None, None, torch.from_numpy(view[inside]).to(DEV), torch.from_numpy(pixel[inside]).to(DEV),
                       torch.empty((V, 1, H, W), device=DEV), None)
    assert bits_equal(point_values(res, torch.from_numpy(maps).to(DEV)), a[torch.from_numpy(inside).to(DEV)])
