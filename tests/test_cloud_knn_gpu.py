"""cloud_knn and statistical_outlier_mask on the device (csrc/mvsn_cloud_knn.hip) against the numpy restatement
(tests/cloud_knn_reference.py).  Every case goes through the C ABI with every input, the workspace and every output
between guard bands under both poisons.  dist2, index and within are compared bit for bit: they are exact by construction
(the same fp32 operations, an integer order), so no tolerance applies.

`mean`, the bound.  The device and numpy both form s_1 = sqrt(d_0) (0 + x is exact), s_(j+1) = fl(s_j + fl(sqrt(d_j))) and
m = fl(s_k / k), with d_j the same fp64 numbers (the fp32 dist2 widened, which is exact).  Let an fp64 square root, add or
divide of the device differ from numpy's correctly rounded one by at most one unit in the last place of its result,
e = 2^-52 relative.  Every term is non-negative, so every partial sum is at most s_k.  The k square roots move their terms
by at most e each, and the terms add up to s_k: e s_k in all.  Each of the k - 1 adds that round moves its partial sum by
at most e s_j <= e s_k: (k - 1) e s_k.  The divide adds e.  Together (k + 1) e to first order, and (k + 2) 2^-52 with the
second-order terms.  The NaN pattern is exact.  test_mean_bit_for_bit then asserts the stronger statement, that the bits are
equal: DESIGN.md section 22 records that the device's fp64 sqrt, add and divide round as numpy's do.

mvsn_cloud_mean_stats, the bound: cloud_knn_reference.mean_stats_bounds derives it (a length-n fp64 sum in any order).

Figures of one MI355X run are in DESIGN.md section 22."""
import functools

import numpy as np
import pytest
import torch

import cloud_knn_reference as ck
from cloud_reference import radius_scalars
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd.fusion import cloud_knn, cloud_nearest, radius_outlier_mask, statistical_outlier_mask

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISONS = (POISON_NAN, POISON_FINITE)


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _entry(query, target, k, h, *, exclude_self=False, fill=POISON_NAN, mean=True, nearest=False):
    """mvsn_cloud_index_build, then mvsn_cloud_knn (and mvsn_cloud_nearest on the same index with `nearest`), every input
    in a poisoned buffer of its own (16-byte aligned only), the workspace, the status word and every output carved between
    guard bands and poisoned too: numpy arrays."""
    hf, inv, r2 = radius_scalars(h)
    target = query if target is None else target
    n, m = len(query), len(target)
    guard = Guard(_alloc, fill)
    q, t = guard.poisoned(_to(query)), guard.poisoned(_to(target))
    lib = _native.load()
    ws_bytes = lib.mvsn_cloud_workspace_bytes(m)
    ws, status = guard.empty((ws_bytes,), torch.uint8, DEV), guard.empty((1,), torch.int64, DEV)
    dist2, index = guard.empty((n, k), torch.float32, DEV), guard.empty((n, k), torch.int64, DEV)
    within = guard.empty((n,), torch.int32, DEV)
    mu = guard.empty((n,), torch.float64, DEV) if mean else None
    if nearest:
        nd, ni, nw = guard.empty((n,), torch.float32, DEV), guard.empty((n,), torch.int64, DEV), guard.empty((n,), torch.int32, DEV)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_cloud_index_build(_native.ptr(t), m, float(hf), float(inv), _native.ptr(status),
                                                 _native.ptr(ws), ws_bytes, st), "mvsn_cloud_index_build")
        _native.check(lib.mvsn_cloud_knn(_native.ptr(q), n, k, int(exclude_self), float(hf), float(inv), float(r2),
                                         _native.ptr(ws), ws_bytes, m, _native.ptr(dist2), _native.ptr(index),
                                         _native.ptr(within), _native.ptr(mu), st), "mvsn_cloud_knn")
        if nearest:
            _native.check(lib.mvsn_cloud_nearest(_native.ptr(q), n, float(inv), float(r2), _native.ptr(ws), ws_bytes, m,
                                                 _native.ptr(nd), _native.ptr(ni), _native.ptr(nw), st), "mvsn_cloud_nearest")
    torch.cuda.synchronize()
    guard.check()
    assert int(status.item()) == 0
    out = {"dist2": dist2.cpu().numpy(), "index": index.cpu().numpy(), "within": within.cpu().numpy()}
    if mean:
        out["mean"] = mu.cpu().numpy()
    if nearest:
        out["nearest"] = {"dist2": nd.cpu().numpy(), "index": ni.cpu().numpy(), "within": nw.cpu().numpy()}
    return out


@functools.lru_cache(maxsize=None)
def _device(name, k, exclude_self=False, fill=POISON_NAN):
    """Made once per (case, k, exclude_self, poison), never modified."""
    c = ck.case(name)
    return _entry(c["query"], c["target"], k, c["h"], exclude_self=exclude_self, fill=fill)


def _same_bits(a, b, keys=None):
    for key in keys or sorted(set(a) | set(b)):
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


def _mean_agrees(got, want, k, what):
    """The NaN pattern exactly, the values within (k + 2) 2^-52 relative (the module's docstring); returns whether the bits
    are equal too."""
    assert (np.isnan(got) == np.isnan(want)).all(), what
    has = ~np.isnan(want)
    err = np.abs(got[has] - want[has])
    bound = (k + 2) * 2.0 ** -52 * np.abs(want[has])
    worst = float((err / np.where(bound > 0, bound, 1.0)).max()) if has.any() else 0.0
    same = got.tobytes() == want.tobytes()
    print(f"{what}: {int(has.sum())} of {len(has)} with a mean; error / bound max {worst:.3g}; bits equal: {same}")
    assert (err <= bound).all(), what
    return same


# ---- every case, every k: the workgroup edge (nq = 1, 255, 256, 257), every capacity's last k and the next one's first,
# ---- ties, duplicates, fewer than k, rows that are not finite, queries beyond the grid, the two-cell reach ----------------
@pytest.mark.parametrize("name, k, exclude_self", ck.RUNS)
def test_cases_match_the_restatement_bit_for_bit(name, k, exclude_self):
    got, ref = _device(name, k, exclude_self), ck.case_reference(name, k, exclude_self)
    _same_bits(got, ref, ("dist2", "index", "within"))
    _mean_agrees(got["mean"], ref["mean"], k, f"{name} k={k} exclude_self={exclude_self}")
    if exclude_self:
        assert (got["index"] != np.arange(len(got["index"]))[:, None]).all()
        base = _device(name, k, False)
        finite = np.isfinite(ck.case(name)["query"]).all(axis=1)
        assert (got["within"][finite] == base["within"][finite] - 1).all()          # the point itself and nothing else
    full = got["index"] >= 0
    assert (full.sum(axis=1) == np.minimum(got["within"], k)).all() and (np.diff(full.astype(int), axis=1) <= 0).all()
    with np.errstate(invalid="ignore"):                                         # (inf - inf behind the last candidate)
        assert (np.diff(got["dist2"], axis=1)[full[:, 1:]] >= 0).all()


@pytest.mark.parametrize("name, k, exclude_self", ck.RUNS)
def test_mean_bit_for_bit(name, k, exclude_self):
    # the stronger statement (DESIGN.md section 22 records that it holds on the MI355X)
    got, ref = _device(name, k, exclude_self), ck.case_reference(name, k, exclude_self)
    assert got["mean"].tobytes() == ref["mean"].tobytes()


@pytest.mark.parametrize("name, k, exclude_self", ck.RUNS)
def test_buffers_under_both_poisons(name, k, exclude_self):
    # (the guard bands of every buffer are checked inside _entry; an element nobody writes, or a read of foreign memory
    # that reaches a result, differs between the two fills)
    _same_bits(_device(name, k, exclude_self, POISON_NAN), _device(name, k, exclude_self, POISON_FINITE))


def test_the_mean_left_out():
    c = ck.case("n257")
    for k in (8, 33):
        for fill in POISONS:
            got = _entry(c["query"], c["target"], k, c["h"], mean=False, fill=fill)
            assert set(got) == {"dist2", "index", "within"}
            _same_bits(got, _device("n257", k), ("dist2", "index", "within"))


@pytest.mark.parametrize("name", ["n257", "self", "tiny", "dense_down"])
def test_k_1_is_mvsn_cloud_nearest(name):
    c = ck.case(name)
    for fill in POISONS:
        got = _entry(c["query"], c["target"], 1, c["h"], fill=fill, nearest=True)
        near = got.pop("nearest")
        for key in near:
            assert got[key].reshape(-1).tobytes() == near[key].tobytes(), key
        _same_bits(got, ck.cloud_knn_reference(c["query"], ck.case_target(name), 1, c["h"]), ("dist2", "index", "within"))


@pytest.mark.parametrize("name, k", [("n257", 8), ("n257", 64), ("dense_up", 8), ("dense_up", 64), ("tiny", 17)])
def test_the_order_of_the_target_reaches_no_distance(name, k):
    c = ck.case(name)
    perm = np.random.default_rng(201).permutation(len(c["target"]))
    base = _device(name, k)
    moved = _entry(c["query"], c["target"][perm], k, c["h"])
    _same_bits(base, moved, ("dist2", "within", "mean"))
    _same_bits(moved, ck.cloud_knn_reference(c["query"], c["target"][perm], k, c["h"]), ("dist2", "index", "within"))
    assert (moved["index"] != base["index"]).any()
    # the same points: where no distance is tied the rows are the permuted ones
    inv = np.argsort(perm)
    untied = np.ones(base["index"].shape, bool)
    with np.errstate(invalid="ignore"):
        step = np.diff(base["dist2"], axis=1) != 0
    untied[:, 1:] &= step
    untied[:, :-1] &= step
    untied &= (base["index"] >= 0) & (np.arange(k)[None, :] < k - 1)            # (the last slot may be tied with the one left out)
    assert (untied.sum() > 20 or name.startswith("dense")) and (moved["index"][untied] == inv[base["index"][untied]]).all()


def test_calling_twice_gives_the_same_bits():
    c = ck.case("self")
    _same_bits(_device("self", 33, True), _entry(c["query"], None, 33, c["h"], exclude_self=True))


# ---- mvsn_cloud_mean_stats ----------------------------------------------------------------------------------------------
def _stats(m, fill):
    guard = Guard(_alloc, fill)
    lib = _native.load()
    n = len(m)
    x = guard.poisoned(_to(m))
    ws_bytes = lib.mvsn_cloud_mean_stats_workspace_bytes(n)
    ws, out = guard.empty((ws_bytes,), torch.uint8, DEV), guard.empty((3,), torch.float64, DEV)
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_cloud_mean_stats(_native.ptr(x), n, _native.ptr(ws), ws_bytes, _native.ptr(out), _native.stream()),
                      "mvsn_cloud_mean_stats")
    torch.cuda.synchronize()
    guard.check()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", ck.STATS_SIZES)
def test_mean_stats_against_float64(n):
    m = ck.stats_input(n)
    count, mu, sigma = ck.mean_stats_reference(m)
    runs = [_stats(m, fill) for fill in POISONS + (POISON_NAN,)]
    assert runs[0].tobytes() == runs[1].tobytes() == runs[2].tobytes()             # both poisons, and twice
    got = runs[0]
    assert got[0] == count
    if count < 2:
        assert got[2] == 0.0 and (got[1] == mu if count == 1 else np.isnan(got[1]))
        return
    b_mu, b_sigma = ck.mean_stats_bounds(m)
    print(f"n = {n}: count {int(count)}; |mu - ref| {abs(got[1] - mu):.3g} (bound {b_mu:.3g}), |sigma - ref| {abs(got[2] - sigma):.3g} "
          f"(bound {b_sigma:.3g})")
    assert abs(got[1] - mu) <= b_mu and abs(got[2] - sigma) <= b_sigma


def test_mean_stats_of_nothing_and_of_one():
    for fill in POISONS:
        none = _stats(np.full(1500, np.nan), fill)
        assert none[0] == 0 and np.isnan(none[1]) and none[2] == 0
        m = np.full(2049, np.nan)
        m[2047] = 0.375
        assert _stats(m, fill).tolist() == [1.0, 0.375, 0.0]
        m[5] = 0.125
        two = _stats(m, fill)
        assert two[:2].tolist() == [2.0, 0.25] and abs(two[2] - np.sqrt(0.03125)) <= 2.0 ** -52 * np.sqrt(0.03125)


# ---- statistical_outlier_mask -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mask(name):
    c = ck.sor_case(name)
    return statistical_outlier_mask(_to(c["points"]), c["k"], c["std_ratio"], c["h"])


@pytest.mark.parametrize("name", ck.SOR_IDS)
def test_statistical_outlier_mask_equals_the_restatement(name):
    # exact, with no point excluded: no point lies within the margin of its threshold (test_cloud_knn_reference_cpu.py)
    c, ref, got = ck.sor_case(name), ck.sor_reference(name), _mask(name)
    assert got.keep.dtype == torch.bool and got.mean_dist.dtype == got.mean.dtype == got.std.dtype == torch.float64
    assert got.keep.shape == got.mean_dist.shape == (len(c["points"]),) and got.mean.shape == got.std.shape == ()
    assert got.keep.is_cuda and got.mean.is_cuda and got.std.is_cuda
    keep, md = got.keep.cpu().numpy(), got.mean_dist.cpu().numpy()
    np.testing.assert_array_equal(keep, ref["keep"])
    _mean_agrees(md, ref["mean_dist"], c["k"], name)
    assert not keep[np.isnan(md)].any()
    b_mu, b_sigma = ck.mean_stats_bounds(ref["mean_dist"])
    assert abs(float(got.mean) - ref["mean"]) <= b_mu + (c["k"] + 2) * 2.0 ** -52 * ref["mean"]
    # (every mean_dist moved by e' = (k + 2) 2^-52 relative moves sigma by at most e' sqrt(sum m^2 / (n - 1)) <= e' (mu + sigma),
    # up to n / (n - 1): twice that)
    assert abs(float(got.std) - ref["std"]) <= b_sigma + 2 * (c["k"] + 2) * 2.0 ** -52 * (ref["mean"] + ref["std"])
    again = statistical_outlier_mask(_to(c["points"]), c["k"], c["std_ratio"], c["h"])
    for a, b in zip(got, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    knn = cloud_knn(_to(c["points"]), _to(c["points"]), c["k"], c["h"], exclude_self=True)
    assert (np.isnan(md) == (knn.within.cpu().numpy() < c["k"])).all()


def test_the_planted_points_are_the_rejected_ones():
    c, got = ck.sor_case("plane"), _mask("plane")
    keep = got.keep.cpu().numpy()
    assert keep[c["kind"] == 0].all() and not keep[c["kind"] != 0].any() and (~keep).sum() == 15


def test_two_densities_the_filter_keeps_what_the_radius_count_drops():
    c, got = ck.sor_case("two_density"), _mask("two_density")
    keep = got.keep.cpu().numpy()
    assert keep.all()                                                           # both sheets, spacings a factor 3 apart
    r = radius_outlier_mask(_to(c["points"]), *ck.RADIUS_COUNT).cpu().numpy()
    assert r[(c["kind"] == 0) & c["interior"]].all() and not r[c["kind"] == 1].any()


# ---- the Python call ----------------------------------------------------------------------------------------------------
def test_the_python_call_is_the_library_call():
    c = ck.case("n257")
    q, t = _to(c["query"]), _to(c["target"])
    for k in (1, 9, 64):
        r = cloud_knn(q, t, k, c["h"])
        assert r.dist2.dtype == torch.float32 and r.index.dtype == torch.int64 and r.within.dtype == torch.int32
        assert r.dist2.shape == r.index.shape == (257, k) and r.within.shape == (257,) and r.dist2.is_cuda
        _same_bits({"dist2": r.dist2.cpu().numpy(), "index": r.index.cpu().numpy(), "within": r.within.cpu().numpy()},
                   _device("n257", k), ("dist2", "index", "within"))
    one, near = cloud_knn(q, t, 1, c["h"]), cloud_nearest(q, t, c["h"])
    assert torch.equal(one.dist2[:, 0].view(torch.int32), near.dist2.view(torch.int32))
    assert torch.equal(one.index[:, 0], near.index) and torch.equal(one.within, near.within)
    s = _to(ck.case("self")["query"])
    own = cloud_knn(s, s, 33, ck.H, exclude_self=True)
    _same_bits({"dist2": own.dist2.cpu().numpy(), "index": own.index.cpu().numpy(), "within": own.within.cpu().numpy()},
               _device("self", 33, True), ("dist2", "index", "within"))
    far = c["target"].copy()
    far[123, 1] = 2.0 ** 20 * c["h"]
    with pytest.raises(ValueError, match="max_dist too small for the target's extent"):
        cloud_knn(q, _to(far), 8, c["h"])
    empty = cloud_knn(q, torch.zeros(0, 3, device=DEV), 8, c["h"])
    assert empty.dist2.is_cuda and torch.isposinf(empty.dist2).all() and (empty.index == -1).all() and not empty.within.any()
