"""The restatements of tests/tail_reference.py against ATen on the CPU, at the shapes and on the inputs of
tests/test_tail_kernels_gpu.py: the reference alone -- ATen's float32 result standing in for a correct kernel -- stays
inside every bound and every cap the GPU tests use.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import tail_reference as tr
from oracle import mvsn_oracle as oracle

torch.set_grad_enabled(False)


def test_resize_taps_at_the_borders():
    i0, i1, l0, l1 = tr.resize_taps(8, 15)
    assert i0[0] == 0 and l1[0] == 0.0 and l0[0] == 1.0           # source index clamped at 0
    assert i0[-1] == 7 and i1[-1] == 7                              # the +1 tap clamped to the last index
    assert (i0 >= 0).all() and (i1 <= 7).all() and ((i1 - i0) >= 0).all() and ((i1 - i0) <= 1).all()
    assert ((l0 >= 0) & (l1 >= 0) & (l1 < 1)).all()
    i0, i1, l0, l1 = tr.resize_taps(1, 2)                           # one input row: both taps are row 0
    assert (i0 == 0).all() and (i1 == 0).all()


def test_bilinear_ref_against_aten():
    worst = 0.0
    cases = [(x, out) for x, out in tr.bilinear_inputs()] + [(x, out) for x, _, out in tr.prior_inputs()]
    assert len(cases) == 3 * len(tr.BILINEAR_SIZES)
    for x, out in cases:
        ref = tr.bilinear_ref(x, out)
        assert ref.shape == x.shape[:2] + tuple(out) and ref.dtype == torch.float64
        got = F.interpolate(x, size=out, mode="bilinear", align_corners=False)
        err = float((got.double() - ref).abs().max()) / (tr.EPS * float(x.abs().max()))
        worst = max(worst, err)
        assert err <= tr.BILINEAR_FACTOR, (tuple(x.shape), out, err)
    print(f"bilinear: ATen float32 at most {worst:.2f} * 2^-24 * max|x| from bilinear_ref (bound {tr.BILINEAR_FACTOR})")


def test_bilinear_mask_ref_against_the_oracle():
    near = 0
    for planes in tr.BILINEAR_PLANES:
        for size, out in tr.BILINEAR_SIZES:
            m = tr.mask_input(planes, size)
            ref, blend = tr.bilinear_mask_ref(m, out)
            got = oracle.upsample_mask(m, out)
            decided = (blend - 0.5).abs() > 2.0 ** -20
            near += int((~decided).sum())
            assert torch.equal(got[decided], ref[decided]), (size, out)
            assert 0.2 < float(ref.float().mean()) < 0.8
    print(f"mask resize: {near} pixels within 2^-20 of 0.5")


def test_area_downsample_ref_against_aten():
    worst = 0.0
    for planes in tr.AREA_PLANES:
        for rows, cols in tr.AREA_SIZES:
            x = tr.image_input(planes, rows, cols)
            ref = tr.area_downsample_ref(x)
            size = ((rows + 1) // 2, (cols + 1) // 2)
            assert ref.shape[-2:] == size
            got = F.interpolate(x, size, mode="area")
            err = float((got.double() - ref).abs().max()) / (tr.EPS * float(x.abs().max()))
            worst = max(worst, err)
            assert err <= tr.AREA_FACTOR, (rows, cols, err)
            assert torch.equal(got, F.adaptive_avg_pool2d(x, size))
    print(f"area: ATen float32 at most {worst:.2f} * 2^-24 * max|x| from area_downsample_ref (bound {tr.AREA_FACTOR})")


def test_pyramid_ref_levels():
    for rows, cols, levels in tr.PYRAMID_CASES + tr.PYRAMID_UNSUPPORTED:
        x = tr.image_input(2, rows, cols)
        pyr = tr.pyramid_ref(x, levels)
        assert len(pyr) == levels and pyr[0] is not None and torch.equal(pyr[0], x)
        for l in range(1, levels):
            h, w = pyr[l - 1].shape[-2:]
            assert pyr[l].shape[-2:] == ((h + 1) // 2, (w + 1) // 2) and pyr[l].dtype == torch.float32
            err = float((pyr[l].double() - tr.area_downsample_ref(pyr[l - 1])).abs().max())
            assert err <= tr.AREA_FACTOR * tr.EPS * float(pyr[l - 1].abs().max())


@pytest.mark.parametrize("D", tr.SOFT_ARGMIN_D)
def test_soft_argmin_ref_against_the_oracle(D):
    worst = 0.0
    for n, rows, cols in tr.SOFT_ARGMIN_SHAPES:
        for scale in tr.SOFT_ARGMIN_SCALES:
            cost, samples = tr.soft_argmin_inputs(n, D, rows, cols, scale)
            assert n == 1 or not torch.equal(samples[0], samples[1])
            ref = tr.soft_argmin_ref(cost, samples)
            got = oracle.soft_argmin(cost, samples)
            assert ref.shape == (n, 1, rows, cols) == got.shape
            for i in range(n):
                frac = float((got[i].double() - ref[i]).abs().max()) / tr.soft_argmin_bound(D, samples[i])
                worst = max(worst, frac)
                assert frac <= 1.0, (D, n, rows, cols, scale, frac)
    print(f"soft-argmin D={D}: ATen float32 at most {worst:.3f} of the bound")


def test_soft_argmin_ref_constant_cost_and_nan():
    cost, samples = tr.soft_argmin_inputs(3, 17, 7, 37, 1.0)
    flat = tr.soft_argmin_ref(torch.full_like(cost, 3.0), samples)
    assert torch.allclose(flat, samples.double().mean(1).view(3, 1, 1, 1).expand_as(flat), rtol=1e-14, atol=0)
    cost[1, 4, 2, 5] = float("nan")
    ref = tr.soft_argmin_ref(cost, samples)
    assert bool(ref[1, 0, 2, 5].isnan()) and int(ref.isnan().sum()) == 1


@pytest.mark.parametrize("alias", [False, True])
def test_fuse_ref32_against_float64(alias):
    worst = 0.0
    for S in tr.FUSE_S:
        for B in tr.FUSE_B:
            for D in tr.FUSE_D:
                for rows, cols in tr.FUSE_GRIDS:
                    raw, refined, baseline, mask = tr.fuse_inputs(S, B, D, rows, cols)
                    assert len(set(baseline.tolist())) == S * B and 0.3 < float(baseline.min()) and float(baseline.max()) < 2
                    refined = None if alias else refined
                    r32, f32, m32 = tr.fuse_ref32(raw, refined, baseline, mask, S, B)
                    r64, f64 = tr.fuse_ref64(raw, refined, baseline, S, B)
                    for a, b in ((r32, r64), (f32, f64)):
                        err = float(((a.double() - b).abs() / b).max()) / tr.EPS
                        worst = max(worst, err)
                        assert err <= tr.FUSE_FACTOR, (S, B, D, rows, cols, err)
                    if alias:
                        assert torch.equal(r32, f32)
                    assert torch.equal(m32, mask.view(S, B, D, rows, cols).sum(0) * 2 > S)
    print(f"fusion (alias={alias}): float32 chain at most {worst:.2f} * 2^-24 relative from the float64 means")


def test_fuse_ref32_mask_ties():
    for S, n_set, want in ((2, 1, False), (4, 2, False), (4, 3, True), (3, 2, True), (3, 1, False), (1, 1, True), (5, 3, True),
                           (5, 2, False)):
        raw, refined, baseline, _ = tr.fuse_inputs(S, 3, 3, 7, 37)
        mask = tr.tie_mask(S, 3, 3, 7, 37, n_set)
        assert (mask.view(S, -1).sum(0) == n_set).all() and (S == n_set or not mask.view(S, -1)[0].all())
        out = tr.fuse_ref32(raw, refined, baseline, mask, S, 3)[2]
        assert out.dtype == torch.bool and bool((out == want).all()), (S, n_set)


def test_fuse_ref32_sees_the_chain_order():
    raw, refined, baseline, mask = tr.fuse_inputs(2, 3, 3, 7, 37)
    a = tr.fuse_ref32(raw, refined, baseline, mask, 2, 3)
    b = tr.fuse_ref32(raw, refined, baseline, mask, 2, 3, chain=tr.chain_bs)
    assert not any(torch.equal(x, y) for x, y in zip(a, b))
