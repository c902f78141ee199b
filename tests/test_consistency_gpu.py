"""The two-view consistency kernels (csrc/mvsn_consistency.hip) and the depth-metric kernels (csrc/mvsn_metrics.hip) on the
device against their restatement (tests/consistency_reference.py): bounded quantities within the
derived bounds, exact ones bit for bit.  Every input sits in a poisoned buffer of its own, every output and workspace
between guard bands, and every case runs under both poisons with identical bits."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import consistency_reference as cr
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native, losses, metrics
from oracle import mvsn_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FILLS = (POISON_NAN, POISON_FINITE)
shapes = pytest.mark.parametrize("rows,cols", cr.SHAPES, ids=cr.SHAPE_IDS)


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _host(x):
    return None if x is None else x.cpu().numpy()


def _same_bits(a, b, keys=None):
    for k in (keys or a.keys()):
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ---- mvsn_idepth_reproject ---------------------------------------------------------------------------------------------
ALWAYS = ("idp", "sampled", "invalid")


def _reproject(K, T, L, R, mask=None, fill=POISON_NAN, want_uv=True, want_partials=True):
    """One guarded launch: CPU tensors in (mask a bool numpy array or None), a dict of numpy arrays out (None for an
    output not asked for).  The mask output is asked for exactly when a mask is given."""
    lib = _native.load()
    B, _, rows, cols = L.shape
    guard = Guard(_alloc, fill)
    put = lambda a: guard.poisoned(a.contiguous().to(DEV))   # noqa: E731
    Kd, Td, Ld, Rd = put(K), put(T), put(L), put(R)
    md = put(torch.from_numpy(np.ascontiguousarray(mask)).to(torch.uint8)) if mask is not None else None
    nb = lib.mvsn_idepth_reproject_blocks(rows * cols)
    assert nb == (rows * cols + cr.RP_THREADS - 1) // cr.RP_THREADS
    idp, sampled = guard.empty((B, 1, rows, cols), torch.float32, DEV), guard.empty((B, 1, rows, cols), torch.float32, DEV)
    invalid = guard.empty((B, 1, rows, cols), torch.uint8, DEV)
    ms = guard.empty((B, 1, rows, cols), torch.uint8, DEV) if mask is not None else None
    uv = guard.empty((B, rows, cols, 2), torch.float32, DEV) if want_uv else None
    partials = guard.empty((B, nb), torch.float32, DEV) if want_partials else None
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_idepth_reproject(_native.ptr(Kd), _native.ptr(Td), _native.ptr(Ld), _native.ptr(Rd),
                                                _native.ptr(md), B, rows, cols, _native.ptr(idp), _native.ptr(sampled),
                                                _native.ptr(ms), _native.ptr(invalid), _native.ptr(uv),
                                                _native.ptr(partials), _native.stream()), "mvsn_idepth_reproject")
    torch.cuda.synchronize()
    guard.check()
    return {"idp": _host(idp), "sampled": _host(sampled), "invalid": _host(invalid), "mask_sampled": _host(ms),
            "uv": _host(uv), "partials": _host(partials)}


@functools.lru_cache(maxsize=None)
def _scene_run(rows, cols, kind="random", fill=POISON_NAN, identity=False):
    """The scene through the kernel with every output, made once per (scene, mask, poison) and never modified."""
    K, T, L, R = cr.scene(rows, cols, identity)
    mask = cr.scene_masks(rows, cols)[0 if kind == "random" else 1]
    return _reproject(K, T, L, R, mask, fill)


def _check_sampled(out, R, rows, cols, extra=None):
    uv = out["uv"]
    want, bound = cr.sample(R.numpy(), uv), cr.sample_bound(R.numpy(), uv, rows, cols)
    if extra is not None:
        bound = bound + extra
    err = np.abs(out["sampled"].astype(np.float64) - want)
    assert np.isfinite(out["sampled"]).all()
    ratio = float((err / bound).max())
    assert ratio <= 1, (ratio, float(err.max()))
    return ratio


def _check_sandwich(out, mask, rows, cols):
    flag = out["mask_sampled"]
    assert set(np.unique(flag).tolist()) <= {0, 1}
    must, may = cr.mask_sampled_sandwich(mask, out["uv"], rows, cols)
    assert not (must & (flag == 0)).any(), f"{int((must & (flag == 0)).sum())} flags clear under a set tap with weight"
    assert not ((flag != 0) & ~may).any(), f"{int(((flag != 0) & ~may).sum())} flags set without a set texel in reach"
    return int(must.sum()), int(may.sum())


def _check_partials(out, B):
    """Every block's sum within PARTIAL_ADDS roundings of the float64 sum of its exact fp32 terms, the terms taken from the
    device's own `sampled` and `idp`; a block holding a non-finite term has a non-finite sum."""
    terms = cr.absdiff_terms(out["sampled"], out["idp"]).reshape(B, -1)
    sums, mags = cr.block_sums(terms, B)
    got = out["partials"].astype(np.float64)
    assert got.shape == sums.shape
    finite = np.isfinite(sums)
    np.testing.assert_array_equal(np.isfinite(got), finite)
    bound = cr.PARTIAL_ADDS * cr.U * mags
    err = np.abs(got - sums)[finite]
    ok = bound[finite] > 0
    assert (err[~ok] == 0).all()
    ratio = float((err[ok] / bound[finite][ok]).max()) if ok.any() else 0.0
    assert ratio <= 1, ratio
    return ratio


@shapes
def test_reproject_against_the_restatement(rows, cols):
    K, T, L, R = cr.scene(rows, cols)
    out = _scene_run(rows, cols)
    _same_bits(out, _scene_run(rows, cols, fill=POISON_FINITE))
    uv64, idp64, inv64 = cr.project(K, T, L)
    e_uv = float(((torch.from_numpy(out["uv"]).double() - uv64).abs() / (cr.UV_ATOL + cr.UV_RTOL * uv64.abs())).max())
    e_id = float(((torch.from_numpy(out["idp"]).double() - idp64).abs() / (cr.ID_ATOL + cr.ID_RTOL * idp64.abs())).max())
    assert set(np.unique(out["invalid"]).tolist()) <= {0, 1}
    differ = torch.from_numpy(out["invalid"] != 0) != inv64
    on_edge = cr.edge_distance(uv64) < cr.EDGE
    r_s = _check_sampled(out, R, rows, cols)
    must, may = _check_sandwich(out, cr.scene_masks(rows, cols)[0], rows, cols)
    r_p = _check_partials(out, cr.BATCH)
    print(f"{rows}x{cols}: uv / idepth' error over tolerance {e_uv:.3f} / {e_id:.3f}; {int(differ.sum())} invalid flags differ, "
          f"{int(on_edge.sum())} pixels on the predicate; sampled error over bound {r_s:.3f}; partial sums over bound "
          f"{r_p:.3f}; mask flags: {must} must, {may} may, {int((out['mask_sampled'] != 0).sum())} set")
    assert e_uv <= 1 and e_id <= 1
    assert bool(on_edge[differ].all())


@shapes
def test_mask_holding_one_texel(rows, cols):
    mask = cr.scene_masks(rows, cols)[1]
    out = _scene_run(rows, cols, "single")
    _same_bits(out, _scene_run(rows, cols, "single", POISON_FINITE))
    must, may = _check_sandwich(out, mask, rows, cols)
    assert must >= cr.BATCH and (out["mask_sampled"].reshape(cr.BATCH, -1) != 0).any(1).all()
    _same_bits(out, _scene_run(rows, cols), ALWAYS + ("uv", "partials"))          # the mask changes nothing else


@shapes
def test_optional_outputs_leave_the_others_unchanged(rows, cols):
    K, T, L, R = cr.scene(rows, cols)
    mask = cr.scene_masks(rows, cols)[0]
    full = _scene_run(rows, cols)
    for want_uv in (False, True):
        for with_mask in (False, True):
            for want_partials in (False, True):
                for fill in FILLS:
                    out = _reproject(K, T, L, R, mask if with_mask else None, fill, want_uv, want_partials)
                    _same_bits(out, full, ALWAYS + (("uv",) if want_uv else ()) + (("mask_sampled",) if with_mask else ())
                               + (("partials",) if want_partials else ()))


@shapes
def test_batch_element_alone_equals_it_in_company(rows, cols):
    K, T, L, R = cr.scene(rows, cols)
    mask = cr.scene_masks(rows, cols)[0]
    full = _scene_run(rows, cols)
    for b in range(cr.BATCH):
        s = slice(b, b + 1)
        alone = _reproject(K[s], T[s], L[s], R[s], mask[s])
        _same_bits(alone, {k: v[s] for k, v in full.items()})


def test_non_finite_idepth_stays_in_its_pixel():
    """A NaN and a -1e-6f (depth = 1 / 0) in element 1: the other elements and every other pixel keep their bits, the two
    pixels' blocks keep what their terms hold, nothing is read out of range, the flags are the oracle's."""
    rows, cols = 37, 53
    K, T, L, R = cr.scene(rows, cols)
    mask = cr.scene_masks(rows, cols)[0]
    clean = _scene_run(rows, cols)
    dirty_L = L.clone()
    spots = (300, 1500)                                        # blocks 1 and 5 of the 8
    dirty_L[1].view(-1)[spots[0]] = float("nan")
    dirty_L[1].view(-1)[spots[1]] = -1e-6
    assert float(dirty_L[1].view(-1)[spots[1]] + torch.tensor(1e-6)) == 0.0
    out = _reproject(K, T, dirty_L, R, mask, POISON_NAN)
    _same_bits(out, _reproject(K, T, dirty_L, R, mask, POISON_FINITE))
    other = np.ones(rows * cols, bool)
    other[list(spots)] = False
    for k in ("idp", "sampled", "invalid", "mask_sampled"):
        a, b = out[k].reshape(3, -1), clean[k].reshape(3, -1)
        assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes(), k
        assert a[1][other].tobytes() == b[1][other].tobytes(), k
    a, b = out["uv"].reshape(3, -1, 2), clean["uv"].reshape(3, -1, 2)
    assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes() and a[1][other].tobytes() == b[1][other].tobytes()
    blocks = [s // cr.RP_THREADS for s in spots]
    keep = np.ones(out["partials"].shape[1], bool)
    keep[blocks] = False
    assert out["partials"][[0, 2]].tobytes() == clean["partials"][[0, 2]].tobytes()
    assert out["partials"][1][keep].tobytes() == clean["partials"][1][keep].tobytes()
    _check_partials(out, 3)                                    # a non-finite term <=> a non-finite block sum
    assert np.isnan(out["idp"].reshape(3, -1)[1, spots[0]]) and np.isnan(out["partials"][1, blocks[0]])
    uv_o, idp_o, inv_o = oracle.idepthmap_projector(K, T, dirty_L)
    for s in spots:
        assert not np.isfinite(out["uv"].reshape(3, -1, 2)[1, s]).all()
        assert bool(out["invalid"].reshape(3, -1)[1, s]) == bool(inv_o.reshape(3, -1)[1, s])
        assert np.isnan(out["idp"].reshape(3, -1)[1, s]) == bool(torch.isnan(idp_o.reshape(3, -1)[1, s]))
    _check_sampled(out, R, rows, cols)                         # a NaN coordinate reads texel 0, an infinite one the border
    _check_sandwich(out, mask, rows, cols)


@pytest.mark.parametrize("rows,cols", [(16, 16), (37, 53)])
def test_identity_pose_samples_the_map_itself(rows, cols):
    K, T, L, R = cr.scene(rows, cols, identity=True)
    out = _scene_run(rows, cols, identity=True)
    _same_bits(out, _scene_run(rows, cols, fill=POISON_FINITE, identity=True))
    ratio = _check_sampled(out, R, rows, cols)
    err = np.abs(out["sampled"].astype(np.float64) - R.numpy().astype(np.float64))
    slack = cr.sample_bound(R.numpy(), out["uv"], rows, cols) + cr.centre_slack(R.numpy(), out["uv"], rows, cols)
    print(f"identity {rows}x{cols}: sampled error over bound {ratio:.3f}, against the map itself {float((err / slack).max()):.3f}")
    assert (err <= slack).all()
    assert not out["invalid"].any()
    _check_sandwich(out, cr.scene_masks(rows, cols)[0], rows, cols)
    _check_partials(out, cr.BATCH)


# ---- mvsn_occlusion_mask -----------------------------------------------------------------------------------------------
def _occlusion(idp, sampled, invalid, partials, fill):
    """numpy (B, P) arrays in, the mask bytes (B, P) out."""
    lib = _native.load()
    B, P = idp.shape
    guard = Guard(_alloc, fill)
    put = lambda a: guard.poisoned(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))   # noqa: E731
    a, s, i, p = put(idp), put(sampled), put(invalid), put(partials)
    assert partials.shape == (B, lib.mvsn_idepth_reproject_blocks(P))
    mask = guard.empty((B, P), torch.uint8, DEV)
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_occlusion_mask(_native.ptr(a), _native.ptr(s), _native.ptr(i), _native.ptr(p), B, P,
                                              _native.ptr(mask), _native.stream()), "mvsn_occlusion_mask")
    torch.cuda.synchronize()
    guard.check()
    return mask.cpu().numpy()


def _occlusion_both(idp, sampled, invalid, partials):
    a, b = (_occlusion(idp, sampled, invalid, partials, f) for f in FILLS)
    assert a.tobytes() == b.tobytes() and set(np.unique(a).tolist()) <= {0, 1}
    return a


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1961])
def test_occlusion_mask_alone_is_exact(P):
    """Arrays that never saw the reprojection: differences planted at the threshold and one fp32 step to either side,
    arbitrary invalid bytes, another threshold per element."""
    rng = np.random.RandomState(P)
    B, nb = 3, (P + 255) // 256
    idp = rng.uniform(0.0, 0.2, (B, P)).astype(np.float32)
    sampled = rng.uniform(0.0, 0.2, (B, P)).astype(np.float32)
    invalid = rng.choice(np.array([0, 0, 0, 0, 1, 2, 255], np.uint8), (B, P))
    partials = (rng.uniform(0.5, 1.5, (B, nb)) * 0.02 * np.arange(1, B + 1)[:, None] * P / nb).astype(np.float32)
    thr = cr.occlusion_threshold(partials, P)
    assert len(set(thr.tolist())) == B
    for b in range(B):                                        # idp = 0: the difference is `sampled` exactly
        plants = [thr[b], np.nextafter(thr[b], np.float32(1)), np.nextafter(thr[b], np.float32(0))]
        for k, v in enumerate(plants[(b % 3):] + plants[:(b % 3)]):
            if k < P:
                idp[b, k], sampled[b, k], invalid[b, k] = 0.0, v, 0
    want = cr.occlusion_mask(idp, sampled, invalid, partials)
    got = _occlusion_both(idp, sampled, invalid, partials)
    np.testing.assert_array_equal(got != 0, want)
    assert P < 3 or (want[:, :3].sum() == B and (~want[:, :3]).sum() == 2 * B)      # one step above is set, on it and below clear
    # a NaN among one element's partials: that element's mask is `invalid`, the others keep theirs
    partials[1, nb - 1] = np.nan
    nan = _occlusion_both(idp, sampled, invalid, partials)
    np.testing.assert_array_equal(nan[1] != 0, invalid[1] != 0)
    assert nan[[0, 2]].tobytes() == got[[0, 2]].tobytes()


@functools.lru_cache(maxsize=None)
def _chained(rows, cols):
    out = _scene_run(rows, cols)
    P = rows * cols
    return _occlusion_both(out["idp"].reshape(-1, P), out["sampled"].reshape(-1, P), out["invalid"].reshape(-1, P),
                           out["partials"])


@shapes
def test_occlusion_mask_after_the_reprojection(rows, cols):
    """Exact on the device's own intermediates; against float64 a differing pixel sits on its predicate (the argument of
    test_two_view_projection_and_occlusion_through_changed_cameras)."""
    K, T, L, R = cr.scene(rows, cols)
    out, B = _scene_run(rows, cols), cr.BATCH
    got = _chained(rows, cols) != 0
    np.testing.assert_array_equal(got, cr.occlusion_mask(out["idp"], out["sampled"], out["invalid"], out["partials"]))
    uv64, idp64, inv64 = cr.project(K, T, L)
    sample = lambda at: F.grid_sample(R.double(), at, mode="bilinear", padding_mode="border", align_corners=False)  # noqa: E731
    at = sample(uv64)
    id_diff = at - idp64
    thr = id_diff.view(B, -1).abs().mean(1).view(B, 1, 1, 1)
    ref = (id_diff > thr) | inv64
    differ = torch.from_numpy(got).view(B, 1, rows, cols) != ref
    print(f"{rows}x{cols}: {int(differ.sum())} occlusion flags differ from float64 of {ref.numel()} ({float(ref.double().mean()):.3f} set)")
    if differ.any():
        duv = cr.UV_ATOL + cr.UV_RTOL * uv64.abs()
        slack = cr.ID_ATOL + cr.ID_RTOL * idp64.abs()
        for axis in (0, 1):
            step = torch.zeros_like(uv64)
            step[..., axis] = duv[..., axis]
            slack = slack + torch.maximum((sample(uv64 + step) - at).abs(), (sample(uv64 - step) - at).abs())
        bound = slack + slack.view(B, -1).mean(1).view(B, 1, 1, 1) + 1e-6 * thr
        on_predicate = ((id_diff - thr).abs() <= bound) | (cr.edge_distance(uv64) < cr.EDGE)
        assert bool(on_predicate[differ].all())


# ---- mvsn_masked_l1 ----------------------------------------------------------------------------------------------------
def _masked_l1(a, b, skip_a, skip_b, fill=POISON_NAN, previous=None):
    """The loss word as a (1,) float32 numpy array; `previous` is put into the word and accumulate set."""
    lib = _native.load()
    guard = Guard(_alloc, fill)
    put = lambda x: guard.poisoned(torch.from_numpy(np.ascontiguousarray(x)).to(DEV))   # noqa: E731
    ad, bd, sa, sb = put(a), put(b), put(skip_a), put(skip_b)
    loss = guard.empty((1,), torch.float32, DEV)
    if previous is not None:
        loss.fill_(float(previous))
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_masked_l1(_native.ptr(ad), _native.ptr(bd), _native.ptr(sa), _native.ptr(sb), a.size,
                                         0 if previous is None else 1, _native.ptr(loss), _native.stream()), "mvsn_masked_l1")
    torch.cuda.synchronize()
    guard.check()
    return loss.cpu().numpy()


def _l1_inputs(n):
    rng = np.random.RandomState(n)
    a, b = rng.uniform(0.0, 0.2, n).astype(np.float32), rng.uniform(0.0, 0.2, n).astype(np.float32)
    skip_a, skip_b = (rng.uniform(size=n) < 0.4).astype(np.uint8), (rng.uniform(size=n) < 0.3).astype(np.uint8)
    skip_a[skip_a != 0] = rng.choice(np.array([1, 2, 255], np.uint8), int((skip_a != 0).sum()))   # any non-zero byte skips
    return a, b, skip_a, skip_b


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 5000, 98304])
def test_masked_l1(n):
    a, b, skip_a, skip_b = _l1_inputs(n)
    if n == 1:
        skip_a[0] = skip_b[0] = 0
    want, S, C = cr.masked_l1(a, b, skip_a, skip_b)
    assert C > 0
    got = _masked_l1(a, b, skip_a, skip_b)
    assert got.tobytes() == _masked_l1(a, b, skip_a, skip_b, POISON_FINITE).tobytes()
    assert got.tobytes() == _masked_l1(a, b, skip_a, skip_b).tobytes()                       # deterministic
    err = abs(float(got[0]) - float(want))
    print(f"n {n}: {C} selected, loss {float(got[0]):.9g}, error {err / cr.ulp32(want):.2f} ulp")
    assert err <= cr.ulp32(want)
    # accumulate adds in fp32 to what the word held; a NaN there stays
    acc = _masked_l1(a, b, skip_a, skip_b, previous=0.37)
    assert acc.tobytes() == _masked_l1(a, b, skip_a, skip_b, POISON_FINITE, previous=0.37).tobytes()
    total = float(np.float32(0.37)) + float(want)
    assert abs(float(acc[0]) - total) <= 2 * cr.ulp32(total) and acc[0] != got[0]
    assert np.isnan(_masked_l1(a, b, skip_a, skip_b, previous=float("nan"))[0])
    # nothing selected: 0 / 0
    ones = np.ones(n, np.uint8)
    assert np.isnan(_masked_l1(a, b, ones, skip_b)[0]) and np.isnan(_masked_l1(a, b, skip_a * 0, ones)[0])
    assert np.isnan(cr.masked_l1(a, b, ones, skip_b)[0])
    # exactly one element selected: its term, exactly; a NaN under every skipped element does not reach the loss
    for index in sorted({0, n - 1} | ({1024} if n > 1024 else set())):
        only = np.ones(n, np.uint8)
        only[index] = 0
        poisoned_a = np.where(only != 0, np.float32(np.nan), a).astype(np.float32)
        for sa, sb in ((only, only * 0), (only * 0, only)):
            one = _masked_l1(poisoned_a, b, sa, sb)
            assert one[0] == np.abs(a[index] - b[index]) and one.dtype == np.float32, (index, one)
    nan_a, nan_b = a.copy(), b.copy()
    nan_a[skip_a != 0], nan_b[(skip_b != 0) & (skip_a == 0)] = np.nan, np.inf
    assert _masked_l1(nan_a, nan_b, skip_a, skip_b).tobytes() == got.tobytes()


# ---- the wrappers ---------------------------------------------------------------------------------------------------------
LEVELS = ((64, 96), (37, 53), (32, 48), (16, 16), (3, 5))


def test_consistency_loss_wrapper_and_mask_dtypes():
    """left_right_idepthmap_consistency_losses over a five-level pyramid: one bit pattern whatever dtype carries the masks,
    and the restatement's loss on the device's own masks and intermediates within the bound of the ten calls (the first
    within 1 ulp of its float32(S / C), each of the nine accumulations within 2 ulps of the running value)."""
    T = cr.scene(*LEVELS[0])[1]
    Ti = torch.linalg.inv(T.double()).float()
    Ks, Ls, Rs = ([cr.scene(r, c)[i] for r, c in LEVELS] for i in (0, 2, 3))
    dev = lambda xs: [x.to(DEV) for x in xs]   # noqa: E731
    Td, Tid, Kd, Ld, Rd = T.to(DEV), Ti.to(DEV), dev(Ks), dev(Ls), dev(Rs)
    lo = [losses.get_occlusion_mask(Kd[i], Td, Ld[i], None, Rd[i], None) for i in range(5)]
    ro = [losses.get_occlusion_mask(Kd[i], Tid, Rd[i], None, Ld[i], None) for i in range(5)]
    for m in lo + ro:
        assert m.dtype == torch.bool and 0 < int(m.sum()) < m.numel()
    got = losses.left_right_idepthmap_consistency_losses(Td, Tid, Kd, Ld, lo, Rd, ro)
    assert got.is_cuda and got.dim() == 0 and got.dtype == torch.float32
    sevens = lambda m: m.to(torch.uint8) * (1 + 6 * (torch.arange(m.numel(), device=DEV).view(m.shape) % 2)).to(torch.uint8)   # noqa: E731
    for name, conv in (("uint8", sevens), ("int64", lambda m: m.to(torch.int64) * -(1 << 40)), ("float32", lambda m: m.float() * 0.25)):
        other = losses.left_right_idepthmap_consistency_losses(Td, Tid, Kd, Ld, [conv(m) for m in lo], Rd, [conv(m) for m in ro])
        assert other.view(torch.int32).item() == got.view(torch.int32).item(), name
    assert set(sevens(lo[0]).unique().tolist()) == {0, 1, 7}
    running, bound = 0.0, 0.0
    for i in range(5):
        for Tx, a, a_occ, b, b_occ in ((Td, Ld[i], lo[i], Rd[i], ro[i]), (Tid, Rd[i], ro[i], Ld[i], lo[i])):
            projected, sampled, occ_sampled, _, _, _ = losses._reproject(Kd[i], Tx, a, b, other_mask=b_occ)
            want, S, C = cr.masked_l1(projected.cpu().numpy(), sampled.cpu().numpy(), a_occ.cpu().numpy(), occ_sampled.cpu().numpy())
            assert C > 0
            first = running == 0.0 and bound == 0.0
            running += float(want)
            bound += cr.ulp32(want) if first else 2 * cr.ulp32(running)
    print(f"loss {float(got):.9g}, restated {running:.9g}, error over bound {abs(float(got) - running) / bound:.3f}")
    assert abs(float(got) - running) <= bound


@shapes
def test_get_occlusion_mask_is_the_chained_kernels(rows, cols):
    K, T, L, R = cr.scene(rows, cols)
    got = losses.get_occlusion_mask(K.to(DEV), T.to(DEV), L.to(DEV), None, R.to(DEV), None)
    assert got.dtype == torch.bool and got.shape == L.shape
    np.testing.assert_array_equal(got.cpu().numpy().reshape(cr.BATCH, -1), _chained(rows, cols) != 0)
    uv, idp, inv = losses.idepthmap_projector(K.to(DEV), T.to(DEV), L.to(DEV))
    out = _scene_run(rows, cols)
    assert uv.cpu().numpy().tobytes() == out["uv"].tobytes() and idp.cpu().numpy().tobytes() == out["idp"].tobytes()
    np.testing.assert_array_equal(inv.cpu().numpy(), out["invalid"] != 0)


# ---- mvsn_depth_metrics ------------------------------------------------------------------------------------------------
# rmse_log is the one metric whose terms are not restated bit for bit (the device's logf against numpy's float64 log on the
# same fp32 t and e).  The ROCm installation documents no error bound for logf, so the bound is the largest relative error
# measured over METRIC_PIXELS on an MI355X (2.65e-7, at one pixel; 3.3e-8 at the most from 255 pixels up), times 4 as a
# margin for other inputs.
RMSE_LOG_REL_BOUND = 4 * 2.65e-7


def _depth_metrics(idepth, truth, base, fill):
    lib = _native.load()
    B, pixels = idepth.shape
    blocks = lib.mvsn_depth_metrics_blocks(pixels)
    assert blocks == cr.metric_blocks(pixels)
    guard = Guard(_alloc, fill)
    put = lambda x: guard.poisoned(torch.from_numpy(np.ascontiguousarray(x)).to(DEV))   # noqa: E731
    est, tru, bas = put(idepth), put(truth), put(base)
    partials = guard.empty((B * blocks * 9,), torch.float64, DEV)      # exactly B * blocks * 9 doubles between the bands
    rows = guard.empty((B, 9), torch.float64, DEV)
    lo, hi = cr.METRIC_RANGE
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_depth_metrics(_native.ptr(est), _native.ptr(tru), _native.ptr(bas), B, pixels, lo, hi,
                                             _native.ptr(partials), _native.ptr(rows), _native.stream()), "mvsn_depth_metrics")
    torch.cuda.synchronize()
    guard.check()
    return rows.cpu().numpy(), partials.cpu().numpy()


@pytest.mark.parametrize("pixels", cr.METRIC_PIXELS)
def test_depth_metrics(pixels):
    idepth, truth, base = cr.metric_case(pixels)
    got, partials = _depth_metrics(idepth, truth, base, POISON_NAN)
    again, partials2 = _depth_metrics(idepth, truth, base, POISON_FINITE)
    assert got.tobytes() == again.tobytes() and partials.tobytes() == partials2.tobytes()
    assert np.isfinite(partials).all()
    ref = cr.depth_metric_rows64(idepth, truth, base, *cr.METRIC_RANGE)
    want = ref["rows"]
    np.testing.assert_array_equal(got[:, :2], want[:, :2])                                  # both counts, exactly
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    assert got[1, 0] == 0 and np.isnan(got[1, 2:]).all()                                    # no valid truth
    assert np.isnan(got[2, 2:]).all() and got[2, 1] == 0                                    # truth, nothing selected
    r = pixels * 2.0 ** -53
    figures = {}
    for b in range(3):
        n = want[b, 1]
        if n == 0:
            continue
        for k in range(3):                                                                  # a_k n_valid is the integer
            assert got[b, 6 + k] == ref["a_counts"][b, k] / n and round(got[b, 6 + k] * n) == ref["a_counts"][b, k]
        # abs_rel, sq_rel, rmse^2: float64 sums of the same fp32 terms in another order, within pixels 2^-53 relative of
        # the exactly rounded sum S.  Division and square root are correctly rounded and monotone, so a device sum inside
        # [S (1 - r), S (1 + r)] gives a mean (a root mean) between the images of the two ends.
        for k, name, root in ((2, "abs_rel", False), (3, "sq_rel", False), (4, "rmse", True)):
            S = ref["sums"][b, k - 2]
            ends = [S * (1.0 - r) / n, S * (1.0 + r) / n]
            ends = np.sqrt(ends) if root else ends
            assert ends[0] <= got[b, k] <= ends[1], (name, got[b, k], want[b, k])
            figures[name] = abs(got[b, k] - want[b, k]) / (r * want[b, k] * (0.5 if root else 1.0)) if want[b, k] else 0.0
        figures["rmse_log"] = abs(got[b, 5] - want[b, 5]) / want[b, 5] if want[b, 5] else 0.0
        assert figures["rmse_log"] <= RMSE_LOG_REL_BOUND
    assert figures, "no image with a selected pixel"
    print(f"pixels {pixels}: error over bound " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items() if k != "rmse_log")
          + f"; rmse_log relative error {figures['rmse_log']:.3e}")
    # an image alone gives the bits it gives in the batch
    for b in range(3):
        s = slice(b, b + 1)
        alone, _ = _depth_metrics(idepth[s], truth[s], base[s], POISON_NAN)
        assert alone.tobytes() == got[s].tobytes(), b


def test_depth_metric_rows_wrapper_is_the_kernel():
    idepth, truth, base = cr.metric_case(16385)
    rows = metrics.depth_metric_rows(torch.from_numpy(idepth).view(3, 1, 1, -1).to(DEV), torch.from_numpy(truth).view(3, 1, 1, -1).to(DEV),
                                     torch.from_numpy(base).to(DEV), *cr.METRIC_RANGE)
    assert rows.cpu().numpy().tobytes() == _depth_metrics(idepth, truth, base, POISON_NAN)[0].tobytes()
