"""The restatement of the consistency and depth-metric kernels (tests/consistency_reference.py) checked without a GPU:
against the fp32 oracle and the recorded fixtures (g7, g9), and the conditions that keep the GPU cases from being vacuous
or unsatisfiable -- the fp32 oracle's own outputs must keep every bound the device is held to."""
import numpy as np
import pytest
import torch

import consistency_reference as cr
from conftest import load_golden, t
from multi_view_stereonet_amd import metrics
from oracle import mvsn_oracle as oracle
from test_oracle_golden import _consistency_inputs


def _close(a, b, rtol, atol):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b).abs() / (atol + rtol * b.abs())).max())


@pytest.mark.parametrize("rows,cols", cr.SHAPES, ids=cr.SHAPE_IDS)
def test_projection_and_sample_against_the_fp32_oracle(rows, cols):
    K, T, L, R = cr.scene(rows, cols)
    uv, idp, inv = oracle.idepthmap_projector(K, T, L)
    uv64, idp64, inv64 = cr.project(K, T, L)
    e_uv, e_id = _close(uv, uv64, cr.UV_RTOL, cr.UV_ATOL), _close(idp, idp64, cr.ID_RTOL, cr.ID_ATOL)
    differ = inv != inv64
    print(f"{rows}x{cols}: oracle uv / idepth' error over tolerance {e_uv:.3f} / {e_id:.3f}, {int(differ.sum())} flags differ")
    assert e_uv <= 1 and e_id <= 1
    assert bool((cr.edge_distance(uv64)[differ] < cr.EDGE).all())
    # the gather at the oracle's own uv: within the derived bound of the float64 one (grid_sample rounds as the kernel
    # does: one un-normalisation, four weights, four products)
    got = oracle._sample(R, uv).numpy().astype(np.float64)
    want, bound = cr.sample(R.numpy(), uv.numpy()), cr.sample_bound(R.numpy(), uv.numpy(), rows, cols)
    ratio = float((np.abs(got - want) / bound).max())
    print(f"{rows}x{cols}: oracle sample error {float(np.abs(got - want).max()):.2e}, over bound {ratio:.3f}")
    assert ratio <= 1


@pytest.mark.parametrize("rows,cols", cr.SHAPES, ids=cr.SHAPE_IDS)
def test_scene_conditions(rows, cols):
    """No GPU case is vacuous: enough pixels land inside the other image, enough are occluded without leaving it, few sit
    on the |n| = 1 predicate, and the masks show both values to enough pixels."""
    K, T, L, R = cr.scene(rows, cols)
    uv64, idp64, inv64 = cr.project(K, T, L)
    inside = float((~inv64).double().mean())
    occ = oracle.get_occlusion_mask(K, T, L, R)
    occluded = float((occ & ~inv64).double().mean())
    on_edge = float((cr.edge_distance(uv64) < cr.EDGE).double().mean())
    uv32 = oracle.idepthmap_projector(K, T, L)[0].numpy()
    random, single = cr.scene_masks(rows, cols)
    sees_set, sees_clear = cr.reachable_values(random, uv32, rows, cols)
    both = float((sees_set & sees_clear).mean())
    print(f"{rows}x{cols}: inside {inside:.3f}, occluded and inside {occluded:.3f}, on the predicate {on_edge:.4f}, "
          f"random mask shows both values to {both:.3f}")
    assert 0.30 <= inside <= 0.97 and occluded >= 0.10 and on_edge < 0.005 and both >= 0.05
    # the single-texel mask cannot show its texel to 5 % of a large image: it must be seen, with weight, by some pixel
    must, may = cr.mask_sampled_sandwich(single, uv32, rows, cols)
    for b in range(cr.BATCH):
        assert single[b].sum() == 1 and must[b].any() and not may[b].all()


@pytest.mark.parametrize("rows,cols", cr.SHAPES, ids=cr.SHAPE_IDS)
def test_sandwich_holds_for_the_fp32_oracle(rows, cols):
    K, T, L, R = cr.scene(rows, cols)
    uv = oracle.idepthmap_projector(K, T, L)[0]
    for mask in cr.scene_masks(rows, cols):
        flag = (oracle._sample(torch.from_numpy(mask).float(), uv) > 0).numpy()
        must, may = cr.mask_sampled_sandwich(mask, uv.numpy(), rows, cols)
        assert not (must & ~flag).any() and not (flag & ~may).any()
        assert (must <= may).all()


def test_identity_pose_lands_on_pixel_centres():
    for rows, cols in ((16, 16), (37, 53)):
        K, T, L, R = cr.scene(rows, cols, identity=True)
        uv = oracle.idepthmap_projector(K, T, L)[0].numpy()
        got = cr.sample(R.numpy(), uv)
        slack = cr.sample_bound(R.numpy(), uv, rows, cols) + cr.centre_slack(R.numpy(), uv, rows, cols)
        assert (np.abs(got - R.numpy().astype(np.float64)) <= slack).all()
        mask = cr.scene_masks(rows, cols)[0]
        flag = (oracle._sample(torch.from_numpy(mask).float(), torch.from_numpy(uv)) > 0).numpy()
        must, may = cr.mask_sampled_sandwich(mask, uv, rows, cols)
        assert not (must & ~flag).any() and not (flag & ~may).any()


def test_occlusion_and_loss_restatements_against_g9():
    fix = load_golden("g9_two_view_consistency.npz")
    T, Ti, Ks, L, R = _consistency_inputs(fix)
    total, per_level = 0.0, []
    for lvl in range(5):
        level = 0.0
        for Tx, a, b, key, okey in ((T, L[lvl], R[lvl], "left", "right"), (Ti, R[lvl], L[lvl], "right", "left")):
            B, _, rows, cols = a.shape
            uv, idp, inv = oracle.idepthmap_projector(Ks[lvl], Tx, a)
            sampled = oracle._sample(b, uv)
            partials, _ = cr.block_sums(cr.absdiff_terms(sampled.numpy(), idp.numpy()).reshape(B, -1), B)
            mask = cr.occlusion_mask(idp.numpy(), sampled.numpy(), inv.numpy(), partials.astype(np.float32))
            bad = int((mask.reshape(B, 1, rows, cols) != fix[f"{key}_occlusion_{lvl}"]).sum())
            assert bad == 0, (lvl, key, bad)      # (the threshold from block sums, not torch's fp32 mean: no pixel of g9 sits between)
            a_occ, b_occ = t(fix[f"{key}_occlusion_{lvl}"]), t(fix[f"{okey}_occlusion_{lvl}"])
            occ_sampled = (oracle._sample(b_occ.float(), uv) > 0).numpy()
            loss, S, C = cr.masked_l1(idp.numpy(), sampled.numpy(), a_occ.numpy(), occ_sampled)
            assert C > 0
            level += float(loss)
        per_level.append(level)
        assert abs(level - float(fix["left_right_loss_per_level"][lvl])) < 1e-6
        total += level
    assert abs(total - float(fix["left_right_loss"])) < 2e-6


def test_depth_metric_rows64_against_g7_and_the_host_path():
    fix = load_golden("g7_depth_metrics.npz")
    tt, ee = fix["depth_true"].reshape(1, -1), fix["depth_est"].reshape(1, -1)
    with np.errstate(divide="ignore"):
        out = cr.depth_metric_rows64(np.float32(1.0) / ee, tt, np.ones(1, np.float32), 0.0, 1e9)
    for i, k in enumerate(metrics.METRIC_KEYS):
        assert abs(out["rows"][0, 2 + i] - float(fix[k])) <= 2e-6 * max(1.0, abs(float(fix[k]))), k
    for pixels in (1, 255, 257, 8193, 16385):
        idepth, truth, base = cr.metric_case(pixels)
        got = cr.depth_metric_rows64(idepth, truth, base, *cr.METRIC_RANGE)
        want = metrics.depth_metric_rows(torch.from_numpy(idepth).view(3, 1, 1, -1), torch.from_numpy(truth).view(3, 1, 1, -1),
                                         torch.from_numpy(base), *cr.METRIC_RANGE).numpy()
        np.testing.assert_array_equal(got["rows"][:, :2], want[:, :2])
        np.testing.assert_array_equal(np.isnan(got["rows"]), np.isnan(want))
        ok = ~np.isnan(want)
        assert (np.abs(got["rows"][ok] - want[ok]) <= 1e-6 * np.maximum(np.abs(want[ok]), 1e-12)).all()   # numpy's fp32 means
        assert np.isnan(got["rows"][1, 2:]).all() and got["rows"][1, 0] == 0
        assert np.isnan(got["rows"][2, 2:]).all() and got["rows"][2, 0] > 0 or pixels == 1
        for k in range(3):
            assert got["rows"][0, 6 + k] * got["rows"][0, 1] == got["a_counts"][0, k]


def test_metric_plants_sit_on_their_predicates():
    idepth, truth, base = cr.metric_case(255)
    m = cr.depth_metric_terms(idepth[0], truth[0], base[0], *cr.METRIC_RANGE)
    lo, hi = np.float32(0.5), np.float32(10.0)
    e, tr = m["e_all"], truth[0]
    for v in (lo, np.nextafter(lo, np.float32(9)), hi, np.nextafter(hi, np.float32(0))):
        assert (tr == v).any()
    assert (e == lo).any() and (e == hi).any()
    assert ((e > lo) & (e < lo + 4 * cr.ulp32(lo))).any() and ((e < hi) & (e > hi - 4 * cr.ulp32(hi))).any()
    for r in (1.25, 1.5625, 1.953125):
        r = np.float32(r)
        for v in (np.nextafter(r, np.float32(0)), r, np.nextafter(r, np.float32(9))):
            assert (m["ratio"] == v).any(), v
    # a value exactly on a range end is outside, one step inside is selected
    assert not m["truth"][tr == lo].any() and not m["truth"][tr == hi].any() and m["truth"][tr == np.nextafter(lo, hi)].all()
    assert not m["sel"][e == lo].any() and not m["sel"][e == hi].any()
    assert cr.metric_blocks(524288) == 64 and cr.metric_blocks(524289) == 64 and cr.metric_blocks(8193) == 2


def test_exact_restatements_on_hand_values():
    # a NaN threshold compares false: the mask is `invalid`
    idp, smp = np.array([[0.1, 0.2, 0.3]], np.float32), np.array([[0.4, 0.1, 0.35]], np.float32)
    inv = np.array([[0, 1, 0]], np.uint8)
    assert cr.occlusion_mask(idp, smp, inv, np.array([[0.3]], np.float32)).tolist() == [[True, True, False]]
    assert cr.occlusion_mask(idp, smp, inv, np.array([[np.nan]], np.float32)).tolist() == [[False, True, False]]
    assert cr.occlusion_threshold(np.array([[1.0, 2.0], [3.0, 0.5]], np.float32), 4).tolist() == [0.75, 0.875]
    loss, S, C = cr.masked_l1([1.0, 5.0, np.nan], [0.5, 1.0, 0.0], [0, 1, 0], [0, 0, 1])
    assert loss == np.float32(0.5) and C == 1
    assert np.isnan(cr.masked_l1([1.0], [0.0], [1], [0])[0])
    sums, mags = cr.block_sums(np.arange(257, dtype=np.float32)[None], 1)
    assert sums.tolist() == [[255 * 128.0, 256.0]] and mags.tolist() == sums.tolist()
