"""The two consumers of GroupNorm statistics, called directly through _native: mvsn_groupnorm_lrelu_apply
(csrc/mvsn_groupnorm.hip) and mvsn_conv_to1_block (csrc/mvsn_conv_to1.hip) take `stats, stat_tiles` -- finalised (N,4,2)
statistics with stat_tiles = 0, or the producer's records (N,T,4,3) with stat_tiles = T, finalised inside the launch by
mvsn_groupnorm_finalize's own code.  Both forms are the same arithmetic, so every comparison is torch.equal.

Two samples everywhere: the per-sample stride of `stats` differs between the forms (8 against 12 T floats), and one sample
hides that.  The records come from ONE real convolution launch on a 32-channel 8 x 12 input; what matters to the consumers
is the pair (records, their finalised statistics), not which tensor they normalise, so the same pair serves every case."""
import pytest
import torch

from test_hip_parity import net_for
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd.multi_view_stereonet import _Records

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
GN_APPLY_MAX_N = 65535 // 32          # samples per launch of the apply pass (grid.y = sample * 32 + channel)
P = _native.ptr
_SHARED = {}


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator(DEV).manual_seed(seed), device=DEV)


def finalize(lib, records):
    n, tiles = records.shape[0], records.shape[1]
    stats = torch.empty(n, 4, 2, device=DEV)
    _native.check(lib.mvsn_groupnorm_finalize(P(records), n, tiles, P(stats), _native.stream()), "finalize")
    return stats


def shared():
    """(lib, raw conv output (2,32,8,12), its records (2,T,4,3), their statistics, gamma, beta, a second finalised set)."""
    if not _SHARED:
        eng = net_for("gta_sfm_150epochs").engine()
        conv, norm = eng.refiners[0]["res"][0]
        raw, rec = eng.conv(conv, randn(1, 2, 32, 8, 12), want_stats=True, lazy_stats=True)
        assert isinstance(rec, _Records) and rec.partials.shape == (2, rec.tiles, 4, 3) and rec.tiles >= 1
        g = torch.Generator().manual_seed(2)
        st0 = torch.stack([torch.randn(2, 4, generator=g) * 0.1, 1.0 + torch.rand(2, 4, generator=g)], -1).contiguous().to(DEV)
        _SHARED.update(lib=eng.lib, raw=raw, rec=rec.partials, stats=finalize(eng.lib, rec.partials), gamma=norm.gamma,
                       beta=norm.beta, st0=st0, gamma0=randn(3, 32) * 0.2 + 1.0, beta0=randn(4, 32) * 0.1)
        assert not torch.equal(_SHARED["stats"][0], _SHARED["stats"][1])       # (a wrong sample stride would show)
    return _SHARED


def apply(lib, x, stats, tiles, gamma, beta, residual=None, r=None):
    n, spatial = x.shape[0], x.shape[2]
    out = torch.full_like(x, float("nan"))
    r_stats, r_gamma, r_beta = r if r else (None, None, None)
    _native.check(lib.mvsn_groupnorm_lrelu_apply(P(x), P(stats), tiles, P(gamma), P(beta), P(residual), P(r_stats), P(r_gamma),
                                                 P(r_beta), n, spatial, P(out), _native.stream()), "apply")
    return out


@pytest.mark.parametrize("residual", ["none", "plain", "raw"])
@pytest.mark.parametrize("spatial", [96, 63])        # 16-byte path, scalar path
def test_apply_from_records_equals_apply_from_finalised_statistics(spatial, residual):
    s = shared()
    x = s["raw"].reshape(2, 32, 96)[:, :, :spatial].contiguous()
    res = randn(5, 2, 32, spatial) if residual != "none" else None
    r = (s["st0"], s["gamma0"], s["beta0"]) if residual == "raw" else None
    tiles = s["rec"].shape[1]
    want = apply(s["lib"], x, s["stats"], 0, s["gamma"], s["beta"], res, r)
    got = apply(s["lib"], x, s["rec"], tiles, s["gamma"], s["beta"], res, r)
    assert torch.isfinite(want).all() and torch.equal(got, want)
    # and the pass is what it says: LReLU(GN(x)) [+ residual | + LReLU(GN_0(residual))], to fp32 rounding
    def lrelu_gn(t, st, gamma, beta):
        mean, rstd = st[:, :, 0].repeat_interleave(8, 1)[:, :, None], st[:, :, 1].repeat_interleave(8, 1)[:, :, None]
        return torch.nn.functional.leaky_relu((t - mean) * rstd * gamma[None, :, None] + beta[None, :, None], 0.2)
    ref = lrelu_gn(x, s["stats"], s["gamma"], s["beta"])
    if residual == "plain":
        ref = ref + res
    elif residual == "raw":
        ref = ref + lrelu_gn(res, *r)
    torch.testing.assert_close(want, ref, rtol=1e-5, atol=1e-5)


def test_apply_across_the_launchers_sample_chunks():
    """n = GN_APPLY_MAX_N + 1: the last sample runs in a second launch, whose `stats` pointer is advanced by the host --
    by 8 floats per sample for finalised statistics, by 12 stat_tiles for records."""
    lib = shared()["lib"]
    n, spatial = GN_APPLY_MAX_N + 1, 4
    assert n == 2048
    g = torch.Generator().manual_seed(7)
    cnt = torch.full((n, 1, 4, 1), 32.0)                       # one record per sample: {count, mean, M2} per group
    mean = torch.randn(n, 1, 4, 1, generator=g) * 0.5 + 0.3
    m2 = (torch.rand(n, 1, 4, 1, generator=g) + 0.1) * 32.0
    rec = torch.cat([cnt, mean, m2], 3).contiguous().to(DEV)
    x, gamma, beta = randn(8, n, 32, spatial), randn(9, 32) * 0.2 + 1.0, randn(10, 32) * 0.1
    stats = finalize(lib, rec)
    want = apply(lib, x, stats, 0, gamma, beta)
    got = apply(lib, x, rec, 1, gamma, beta)
    assert torch.isfinite(want).all() and torch.equal(got, want)
    # the second launch's sample on its own: its statistics are row n - 1 of either array
    for st, tiles in ((stats, 0), (rec, 1)):
        alone = apply(lib, x[n - 1:].contiguous(), st[n - 1:].contiguous(), tiles, gamma, beta)
        assert torch.equal(alone[0], want[n - 1])
    assert not torch.equal(want[n - 1], apply(lib, x[n - 1:].contiguous(), stats[:1].contiguous(), 0, gamma, beta)[0])


def to1_shapes():
    """The smallest pair of images either side of to1_wide_tiles for two samples -- wide (16 x 64) tiles once
    n * ceil(rows / 16) * ceil(cols / 64) >= 4 compute units' worth --: 68 columns are two wide or three narrow tiles, the
    last of either ragged; the wide image also ends in a one-row tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row_tiles = -(-4 * cus // (2 * 2))                          # n = 2 samples x 2 wide column tiles
    wide = lambda rows: 2 * -(-rows // 16) * 2 >= 4 * cus
    narrow_rows, wide_rows = 16 * (row_tiles - 1), 16 * (row_tiles - 1) + 1
    assert not wide(narrow_rows) and wide(wide_rows)
    return {"narrow": (narrow_rows, 68), "wide": (wide_rows, 68)}


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("tiles_form", ["narrow", "wide"])
def test_conv_to1_block_from_records_equals_from_finalised_statistics(tiles_form, with_res, with_prior):
    s = shared()
    lib = s["lib"]
    rows, cols = to1_shapes()[tiles_form]
    key = ("to1", rows)
    if key not in _SHARED:                                      # (inputs: once per shape, never written)
        _SHARED[key] = (randn(11, 2, 32, rows, cols) * 1.5 + 0.3, randn(12, 2, 32, rows, cols),
                        randn(13, 2, 1, rows, cols).abs() * 2.0,
                        torch.tensor([37.5, 32.5], device=DEV), randn(14, 1, 32, 3, 3) * 0.1, randn(15, 1) * 0.1)
    r, x, prior, fx, weight, bias = _SHARED[key]

    def run(stats, tiles):
        out = torch.full((2, 1, rows, cols), float("nan"), device=DEV)
        _native.check(lib.mvsn_conv_to1_block(P(r), P(stats), tiles, P(s["gamma"]), P(s["beta"]), P(x) if with_res else None,
                                              P(weight), P(bias), P(prior) if with_prior else None,
                                              P(fx) if with_prior else None, 2, rows, cols, P(out), _native.stream()),
                      "conv_to1_block")
        return out
    want, got = run(s["stats"], 0), run(s["rec"], s["rec"].shape[1])
    assert torch.isfinite(want).all() and torch.equal(got, want)
