"""Row-phase items of the dilated Winograd layers (conv_wino_kernel's RP form): the same outputs and the same
GroupNorm statistics as the square tiles, bit for bit, plain and carrying a normalise / activate / add job.

mvsn_debug_set_wino_rowphase picks the form per call: 2 = square tiles only, 1 = row-phase items on every dilated
layer (also heights below 16 x dilation, where the default stays on the square tiles), 0 = the default choice.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
BLOCK = {2: 1, 4: 2, 8: 3}   # refiner residual block of each dilation (weights of the level-0 refiner)
_ENG = []


def engine():
    if not _ENG:
        from multi_view_stereonet_amd import MultiViewStereoNet
        from multi_view_stereonet_amd.weights import load_weights
        net = MultiViewStereoNet()
        net.load_state_dict(load_weights("gta_sfm_150epochs"), strict=True)
        _ENG.append((net.to(DEV).eval(), net.engine()))
    return _ENG[0][1]


def in_form(eng, mode, fn):
    old = eng.lib.mvsn_debug_set_wino_rowphase(mode)
    try:
        r = fn()
        torch.cuda.synchronize()
        return r
    finally:
        eng.lib.mvsn_debug_set_wino_rowphase(old)


def gn_stats(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randn(n, 4, generator=g) * 0.1, 1.0 + torch.rand(n, 4, generator=g)], -1).contiguous().to(DEV)


@pytest.mark.parametrize("dil", [2, 4, 8])
@pytest.mark.parametrize("mode1", [False, True])
@pytest.mark.parametrize("rows,cols,n", [(256, 64, 2), (128, 96, 2), (64, 64, 3), (32, 64, 2), (37, 68, 2), (131, 36, 1),
                                         (9, 12, 1)])
def test_rowphase_conv_is_the_square_tile_conv(dil, mode1, rows, cols, n):
    """Values and statistics equal the square-tile form's bits and ATen's conv2d within rounding, with and without the
    previous layer's LReLU(GN(.)) applied on load (MODE 1); ragged heights and heights below 16 x dilation included."""
    from multi_view_stereonet_amd.multi_view_stereonet import _Conv
    eng = engine()
    norm0 = eng.refiners[0]["bn0"]
    g = torch.Generator().manual_seed(rows * 10 + dil)
    w = torch.randn(32, 32, 3, 3, generator=g) * 0.1
    b = torch.randn(32, generator=g) * 0.1
    conv = _Conv(eng.lib, w.to(DEV), b.to(DEV), dilation=dil)
    x = torch.randn(n, 32, rows, cols, generator=g).to(DEV)
    ist = gn_stats(n, rows) if mode1 else None
    kw = dict(in_stats=ist, in_norm=norm0 if mode1 else None, want_stats=True, prefer_fp32_wino=True)
    sq_out, sq_st = in_form(eng, 2, lambda: eng.conv(conv, x, **kw))
    rp_out, rp_st = in_form(eng, 1, lambda: eng.conv(conv, x, **kw))
    auto_out, auto_st = in_form(eng, 0, lambda: eng.conv(conv, x, **kw))
    assert torch.equal(rp_out, sq_out) and torch.equal(rp_st, sq_st)
    assert torch.equal(auto_out, sq_out) and torch.equal(auto_st, sq_st)
    xin = x.cpu()
    if mode1:
        mean, rstd = ist[..., 0].cpu(), ist[..., 1].cpu()
        xg = (xin.reshape(n, 4, 8, rows, cols) - mean[:, :, None, None, None]) * rstd[:, :, None, None, None]
        xin = F.leaky_relu(xg.reshape(n, 32, rows, cols) * norm0.gamma.cpu()[None, :, None, None] +
                           norm0.beta.cpu()[None, :, None, None], 0.2)
    ref = F.conv2d(xin.double(), w.double(), b.double(), padding=dil, dilation=dil)
    torch.testing.assert_close(rp_out.cpu().double(), ref, rtol=1e-4, atol=2e-4)
    rg = ref.reshape(n, 4, -1)
    torch.testing.assert_close(rp_st[:, :, 0].cpu().double(), rg.mean(2), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rp_st[:, :, 1].cpu().double(), 1.0 / (rg.var(2, unbiased=False) + 1e-5).sqrt(),
                               rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("dil", [2, 4, 8])
@pytest.mark.parametrize("mode1,add2", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("rows,cols,n,jn", [(256, 64, 2, 2), (64, 64, 3, 2), (40, 64, 2, 2)])
def test_rowphase_carrying_launch_is_the_square_tile_launch(dil, mode1, add2, rows, cols, n, jn):
    """A row-phase launch carrying a job (two k-steps per step at dilations 2 and 4, one at 8) covers the whole job:
    the layer's outputs and statistics and the job's output equal the square-tile launch's bits."""
    from multi_view_stereonet_amd.multi_view_stereonet import _Job
    eng = engine()
    conv, norm = eng.refiners[0]["res"][BLOCK[dil]]
    assert conv.dilation == dil
    norm0 = eng.refiners[0]["bn0"]
    g = torch.Generator().manual_seed(1000 + rows + dil)
    x = torch.randn(n, 32, rows, cols, generator=g).to(DEV)
    jr = torch.randn(jn, 32, rows, cols, generator=g).to(DEV)
    jres = torch.randn(jn, 32, rows, cols, generator=g).to(DEV)
    st, st0, ist = gn_stats(jn, 1), gn_stats(jn, 2), gn_stats(n, 3)
    kw = dict(in_stats=ist if mode1 else None, in_norm=norm0 if mode1 else None, want_stats=True)
    if add2:
        want_job = eng.gn_lrelu_add2(jr, st, norm, jres, st0, norm0)
    else:
        want_job = eng.gn_lrelu(jr, st, norm, residual=jres)
    got = {}
    for mode in (2, 1):
        jr2 = jr.clone()
        job = _Job(jr2, st, norm, jres, st0 if add2 else None, norm0 if add2 else None)
        before = eng.carried_jobs
        out, stats = in_form(eng, mode, lambda: eng.conv(conv, x, carry=job, **kw))
        assert eng.carried_jobs - before == 1, mode
        assert torch.equal(jr2, want_job), mode
        got[mode] = (out, stats)
    assert torch.equal(got[1][0], got[2][0]) and torch.equal(got[1][1], got[2][1])
