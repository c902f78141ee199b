"""tests/confidence_reference.py against the literal float32 formula of the confidence in ATen on the CPU (MVSNet's
prob_sum4 gathered at depth_index.long()):

    p    = softmin(cost, 1)
    idx  = (p * arange(D)).sum(1)
    conf = 4 * avg_pool3d(pad(p[:, None], (0,0,0,0,1,2)), (4,1,1), 1)  gathered at  idx.long().clamp(0, D-1)

on the seeded inputs the GPU test uses, under the ambiguity rule of confidence_reference.compare.  Measured here, on
ATen's own float32 results over all 108 cases: the confidence is at most 0.062 of conf_bound(D) from the restatement and
the index at most 0.041 of idx_margin(D) (the caps asserted below are 0.1 and 0.1); at scale 1.0 the ambiguous share is
at most 0.30 % for D >= 3."""
import pytest
import torch
import torch.nn.functional as F

import confidence_reference as cr

CONF_CAP = 0.1      # measured 0.062: see the docstring
IDX_CAP = 0.1       # measured 0.041


def literal_fp32(cost):
    D = cost.shape[1]
    p = F.softmin(cost, 1)
    idx = (p * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)).sum(1)
    sum4 = 4 * F.avg_pool3d(F.pad(p[:, None], (0, 0, 0, 0, 1, 2)), (4, 1, 1), 1)
    at = torch.nan_to_num(idx, nan=0.0).long().clamp(0, D - 1)          # (a NaN is never converted)
    return sum4.squeeze(1).gather(1, at.unsqueeze(1)), idx


@pytest.mark.parametrize("D", cr.CONF_D)
def test_literal_formula_within_the_bounds(D):
    worst_conf = worst_idx = 0.0
    for n, rows, cols in cr.CONF_SHAPES:
        for scale in cr.CONF_SCALES:
            cost, _ = cr.conf_inputs(n, D, rows, cols, scale)
            got, idx32 = literal_fp32(cost)
            frac, share = cr.compare(got, cost)
            _, idx64 = cr.confidence_ref(cost)
            ifrac = float((idx32.double() - idx64).abs().max()) / cr.idx_margin(D) if D > 1 else 0.0
            print(f"D={D} {n}x{rows}x{cols} scale {scale:g}: conf {frac:.4f} of conf_bound, idx {ifrac:.4f} of idx_margin, "
                  f"ambiguous {share:.4%}")
            worst_conf, worst_idx = max(worst_conf, frac), max(worst_idx, ifrac)
            assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 + cr.conf_bound(D)
            if scale == 1.0 and D >= 3 and n * rows * cols > 1:
                # the single-window check carries the case: a formula that rounds instead of floors cannot pass
                assert share < 0.01, (D, n, rows, cols, share)
    assert worst_conf <= CONF_CAP and worst_idx <= IDX_CAP, (worst_conf, worst_idx)


def test_rounding_instead_of_flooring_is_caught():
    """The comparison can tell floor from rint at scale 1.0 (where nearly no pixel is ambiguous)."""
    cost, _ = cr.conf_inputs(3, 17, 7, 37, 1.0)
    _, idx64 = cr.confidence_ref(cost)
    wrong = cr.confidence_for_floor(cost, torch.round(idx64)).float()
    frac, _ = cr.compare(wrong, cost)
    assert frac > 1.0


@pytest.mark.parametrize("D", cr.CONF_D)
def test_constant_cost(D):
    """All costs equal: p = 1/D, idx = (D-1)/2; for every D of the list the window lies inside the range or covers it."""
    cost = torch.full((2, D, 3, 5), 3.0)
    conf, idx = cr.confidence_ref(cost)
    assert float((idx - (D - 1) / 2).abs().max()) < 1e-12
    assert float((conf - min(D, 4) / D).abs().max()) < 1e-12
    got, _ = literal_fp32(cost)
    assert cr.compare(got, cost)[0] <= 1.0
    if D == 1:
        assert bool((got == 1.0).all())


@pytest.mark.parametrize("D,d_nan", [(17, 16), (33, 16), (5, 0)])
def test_nan_stays_in_its_pixel(D, d_nan):
    cost, _ = cr.conf_inputs(3, D, 7, 37, 50.0)
    clean, _ = cr.confidence_ref(cost)
    cost[1, d_nan, 2, 5] = float("nan")
    conf, idx = cr.confidence_ref(cost)
    assert bool(conf[1, 0, 2, 5].isnan()) and int(conf.isnan().sum()) == 1 and int(idx.isnan().sum()) == 1
    keep = ~conf.isnan()
    assert torch.equal(conf[keep], clean[keep])
    got, _ = literal_fp32(cost)
    assert cr.compare(got, cost)[0] <= 1.0


def test_fuse_min_ref():
    conf = cr.fuse_min_inputs(3, 2, 4, 5)
    conf[3, 0, 1, 1] = float("nan")                    # chain s=1, b=1
    out = cr.fuse_min_ref(conf, 3, 2)
    assert out.shape == (2, 1, 4, 5) and bool(out[1, 0, 1, 1].isnan()) and int(out.isnan().sum()) == 1
    assert out[0, 0, 2, 3] == min(conf[0, 0, 2, 3], conf[2, 0, 2, 3], conf[4, 0, 2, 3])
    other = cr.fuse_min_ref(conf, 3, 2, chain=cr.chain_bs)
    assert not torch.equal(torch.nan_to_num(out, nan=-1.0), torch.nan_to_num(other, nan=-1.0))
