"""The layer kernels held to their buffers (tests/guarded_alloc.py): every case runs the same call three ways --

  (P) plain, as every other test and production run it;
  (A) with every allocation of the engine inside 64 KiB guard bands, everything poisoned with 0xFF (NaN words), and every
      test-built input copied into a poisoned buffer of its own;
  (B) the same under 0x7B (finite ~1.3e36 words)

-- and asserts that the bands are intact in A and B and that every returned tensor is BIT-identical across P, A and B.  An
output element or record slot nobody writes differs between A and B; a load of unwritten or foreign memory that reaches a
result differs between A and P (or is NaN in A); a store outside a tensor breaks a band.  No tolerance is involved: the
library's determinism and address independence are the only premise.  Payloads are 16-byte aligned and not 32-byte
aligned, which is all include/mvsn_hip.h promises to need.  Workspaces are checked for their bands only.

The shapes are the edge rows of the value tests' parametrisations (test_hip_parity.py, test_wino_rowphase.py): the
smallest at which each kernel can still go wrong."""
import numpy as np
import pytest
import torch

from guarded_alloc import POISON_FINITE, POISON_NAN, bits_equal, guarded
from test_hip_parity import net_for, _motion_family
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd import multi_view_stereonet_utils as snu
from multi_view_stereonet_amd.multi_view_stereonet import PlaneSweepEngine, _Conv, _Job, _Norm, _Records

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
WNAME = "gta_sfm_150epochs"
_ENGINES = []          # every engine a case patched: the last test of the module looks at all of them
_CONVS = {}


def engine():
    eng = net_for(WNAME).engine()
    if not any(e is eng for e in _ENGINES):
        _ENGINES.append(eng)
    return eng


def leaves(x):
    """The tensors of a wrapper's return value, in order (records count as their partials)."""
    if x is None:
        return []
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, _Records):
        return [x.partials]
    if isinstance(x, dict):
        return [t for k in x for t in leaves(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for y in x for t in leaves(y)]
    return []          # (counters, flags)


def _move(v, put):
    if isinstance(v, torch.Tensor):
        return put(v)
    if isinstance(v, (list, tuple)):
        return [_move(y, put) for y in v]
    return v


def _difference(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / dtype {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    wa, wb = a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)
    bad = (wa != wb).nonzero().reshape(-1)
    es = a.element_size()
    first = int(bad[0]) // es
    idx = tuple(int(i) for i in np.unravel_index(first, tuple(a.shape))) if a.dim() else ()
    return (f"{int(torch.unique(bad // es).numel())} of {a.numel()} elements differ, the first at {idx}: "
            f"{a.reshape(-1)[first].item()!r} against {b.reshape(-1)[first].item()!r}")


def three_ways(eng, inputs, call, what, min_allocations=1):
    """call(**inputs on the device) plain and under the two fills; returns the plain run's leaves."""
    got = {}
    dev = {k: _move(v, lambda t: t.to(DEV)) for k, v in inputs.items()}
    got["plain"] = leaves(call(**dev))
    torch.cuda.synchronize()
    for name, fill in (("0xFF", POISON_NAN), ("0x7B", POISON_FINITE)):
        with guarded(eng, fill) as g:          # (asserts the bands of allocations and inputs on exit)
            dev = {k: _move(v, lambda t: g.poisoned(t.to(DEV))) for k, v in inputs.items()}
            n_inputs = len(g.allocations)
            got[name] = leaves(call(**dev))
        assert len(g.allocations) - n_inputs >= min_allocations, f"{what}: the call allocated nothing through the engine"
    assert "empty" not in vars(eng)
    assert len(got["plain"]) == len(got["0xFF"]) == len(got["0x7B"]) and got["plain"], what
    for i, (p, a, b) in enumerate(zip(got["plain"], got["0xFF"], got["0x7B"])):
        assert bits_equal(a, b), f"{what}: output {i} depends on the fill (0xFF against 0x7B): {_difference(a, b)}"
        assert bits_equal(p, a), f"{what}: output {i} under the guard differs from the plain run: {_difference(p, a)}"
    return got["plain"]


def conv_for(cout, cin, k, stride=1, dil=1, dims=2, bias=True):
    """A layer with seeded random weights (packed once, outside the engine's allocations)."""
    key = (cout, cin, k, stride, dil, dims, bias)
    if key not in _CONVS:
        g = torch.Generator().manual_seed(cout * 1000 + cin * 10 + k + dil)
        w = torch.randn((cout, cin) + (k,) * dims, generator=g) * (0.1 if dims == 2 else 0.06)
        b = torch.randn(cout, generator=g) * 0.1 if bias else None
        _CONVS[key] = _Conv(engine().lib, w.to(DEV), b.to(DEV) if bias else None, stride=stride, dilation=dil)
    return _CONVS[key]


def gn_stats(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randn(n, 4, generator=g) * 0.1, 1.0 + torch.rand(n, 4, generator=g)], -1).contiguous()


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def norm0(eng):
    return eng.refiners[0]["bn0"]


class _Form:
    """mvsn_debug_set_wino_rowphase for the duration of a block (2 = square tiles, 1 = row-phase items, 0 = default)."""

    def __init__(self, eng, mode):
        self.eng, self.mode = eng, mode

    def __enter__(self):
        self.old = self.eng.lib.mvsn_debug_set_wino_rowphase(self.mode)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.eng.lib.mvsn_debug_set_wino_rowphase(self.old)


# ---- eng.conv: Winograd 2-D ----------------------------------------------------------------------------------------
WINO_2D = [(32, 16, 32, 2, 1), (32, 37, 68, 2, 1), (36, 40, 72, 1, 1), (4, 24, 40, 3, 1), (32, 5, 4, 2, 1),
           (32, 37, 68, 2, 2), (32, 41, 76, 3, 4), (32, 37, 68, 2, 8), (32, 9, 12, 1, 8)]


@pytest.mark.parametrize("cin,rows,cols,n,dil", WINO_2D)
def test_conv_winograd_2d(cin, rows, cols, n, dil):
    """Statistics on the way out, and (32-channel inputs: GroupNorm has four groups of eight) the previous layer's
    LReLU(GN(.)) on the way in; the dilated layers as square tiles and as row-phase items."""
    eng = engine()
    c = conv_for(32, cin, 3, dil=dil)
    assert c.packed_wino is not None and eng.winograd
    inputs = dict(x=randn(cin * 10 + rows + dil, n, cin, rows, cols), ist=gn_stats(n, rows))
    for mode in ((2, 1) if dil > 1 else (0,)):
        with _Form(eng, mode):
            three_ways(eng, inputs, lambda x, ist: eng.conv(c, x, want_stats=True), f"conv wino mode {mode}", 2)
            if cin == 32:
                three_ways(eng, inputs, lambda x, ist: eng.conv(c, x, in_stats=ist, in_norm=norm0(eng), want_stats=True),
                           f"conv wino + input transform, mode {mode}", 2)


@pytest.mark.parametrize("split,rows,cols,n", [((3, 32, 1), 40, 72, 2), ((4, 4, 4), 33, 52, 2)])
def test_conv_channel_blocks(split, rows, cols, n):
    eng = engine()
    c = conv_for(32, sum(split), 3)
    g = torch.Generator().manual_seed(sum(split) + rows)
    inputs = dict(blocks=[torch.randn(n, c_, rows, cols, generator=g) for c_ in split])

    def call(blocks):
        res = eng.conv_blocks(c, blocks, want_stats=True)
        assert res is not None, "16-byte aligned blocks must take the cat-free path"
        return res
    three_ways(eng, inputs, call, "conv_blocks", 2)


# ---- the volume form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,rows,cols,n", [(8, 16, 32, 2), (5, 9, 36, 1), (1, 16, 32, 2), (6, 30, 40, 2), (3, 23, 36, 1),
                                               (9, 30, 40, 2), (5, 13, 40, 1), (7, 12, 36, 3), (1, 30, 40, 2), (4, 10, 40, 1)])
def test_conv_winograd_volume(depth, rows, cols, n):
    eng = engine()
    c = conv_for(32, 32, 3, dims=3)
    assert c.packed_wino is not None and eng.winograd_volume
    inputs = dict(x=randn(depth * 100 + rows, n, 32, depth, rows, cols), ist=gn_stats(n, depth))
    nrm = eng.vf_norms[0]
    three_ways(eng, inputs, lambda x, ist: eng.conv(c, x, want_stats=True), "conv3d wino", 2)
    three_ways(eng, inputs, lambda x, ist: eng.conv(c, x, in_stats=ist, in_norm=nrm, want_stats=True),
               "conv3d wino + input transform", 2)


# ---- stride-2 layers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wino", [True, False])
@pytest.mark.parametrize("n,rows,cols", [(2, 37, 72), (5, 8, 16)])
def test_conv_5x5_stride2(n, rows, cols, wino):
    eng = engine()
    c = conv_for(32, 32, 5, stride=2)
    inputs = dict(x=randn(rows * 5 + cols, n, 32, rows, cols))
    eng.winograd_stride2 = wino
    try:
        three_ways(eng, inputs, lambda x: eng.conv(c, x), f"conv 5x5 s2 wino={wino}")
    finally:
        eng.winograd_stride2 = True


@pytest.mark.parametrize("n,rows,cols", [(2, 37, 72), (1, 1, 8), (1, 50, 136)])
def test_conv_5x5_stride2_head(n, rows, cols):
    eng = engine()
    c = conv_for(32, 3, 5, stride=2)
    three_ways(eng, dict(x=randn(rows * 11 + cols, n, 3, rows, cols)), lambda x: eng.conv(c, x), "conv 5x5 s2 head")


def test_conv_5x5_stride2_direct_on_odd_columns():
    eng = engine()
    c = conv_for(32, 32, 5, stride=2, bias=False)
    three_ways(eng, dict(x=randn(15, 1, 32, 15, 23)), lambda x: eng.conv(c, x), "conv 5x5 s2 direct 15x23")


# ---- direct kernels on ragged shapes (rows of CONV_CASES with cols % 4 != 0 or an odd channel count) ---------------------
@pytest.mark.parametrize("cin,cout,k,stride,dil,rows,cols,n", [(32, 32, 3, 1, 4, 33, 47, 1), (35, 32, 3, 1, 1, 4, 8, 1),
                                                               (32, 1, 3, 1, 1, 9, 5, 1), (4, 32, 3, 1, 1, 40, 70, 1)])
def test_conv_direct_on_ragged_shapes(cin, cout, k, stride, dil, rows, cols, n):
    eng = engine()
    c = conv_for(cout, cin, k, stride=stride, dil=dil)
    inputs = dict(x=randn(cin * 1000 + rows, n, cin, rows, cols))
    three_ways(eng, inputs, lambda x: eng.conv(c, x, want_stats=(cout == 32)), "conv direct", 2 if cout == 32 else 1)


# ---- folded residual block ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_residual", [True, False])
@pytest.mark.parametrize("rows,cols,dil,cout", [(40, 50, 2, 32), (70, 33, 8, 32), (9, 20, 1, 1)])
def test_conv_with_folded_residual_block(rows, cols, dil, cout, with_residual):
    eng = engine()
    c = conv_for(cout, 32, 3, dil=dil)
    inputs = dict(r=randn(rows + dil, 2, 32, rows, cols) * 1.5 + 0.3, x=randn(rows + dil + 1, 2, 32, rows, cols),
                  ist=gn_stats(2, rows))

    def call(r, x, ist):
        return eng.conv(c, r, in_stats=ist, in_norm=norm0(eng), in_residual=x if with_residual else None, write_staged=True)
    three_ways(eng, inputs, call, "folded residual block", 2)


# ---- carried passes -------------------------------------------------------------------------------------------------
def _carry_case(eng, conv, norm, x, jr, jres, jn, n, mode1, add2, expect, what):
    inputs = dict(x=x, jr=jr, jres=jres, st=gn_stats(jn, 1), st0=gn_stats(jn, 2), ist=gn_stats(n, 3))
    carried = []

    def call(x, jr, jres, st, st0, ist):
        job = _Job(jr, st, norm, jres, st0 if add2 else None, norm0(eng) if add2 else None)      # in place, as the towers run it
        before = eng.carried_jobs
        out, stats = eng.conv(conv, x, in_stats=ist if mode1 else None, in_norm=norm0(eng) if mode1 else None,
                              want_stats=True, carry=job)
        carried.append(eng.carried_jobs - before)
        return out, stats, jr
    three_ways(eng, inputs, call, what, 2)
    assert carried == [expect] * 3, (what, carried)


@pytest.mark.parametrize("block,mode1,add2,n,jn,rows,cols,expect", [
    (0, False, False, 2, 2, 32, 64, 1),      # the job travels inside the launch
    (4, False, False, 2, 2, 40, 72, 0)])     # 2880 pixels per plane: the job runs as a launch of its own
def test_conv_forward_carry(block, mode1, add2, n, jn, rows, cols, expect):
    eng = engine()
    conv, norm = eng.refiners[0]["res"][block]
    _carry_case(eng, conv, norm, randn(100 + block, n, 32, rows, cols), randn(200 + block, jn, 32, rows, cols),
                randn(300 + block, jn, 32, rows, cols), jn, n, mode1, add2, expect, "conv + carried pass")


def test_conv3d_forward_carry():
    eng = engine()
    conv, norm = eng.vf_convs[1], eng.vf_norms[0]
    n, depth, rows, cols = 2, 8, 16, 32
    inputs = dict(x=randn(31, n, 32, depth, rows, cols), jr=randn(32, n, 32, depth, rows, cols), st=gn_stats(n, 4))
    carried = []

    def call(x, jr, st):
        before = eng.carried_jobs
        out, stats = eng.conv(conv, x, want_stats=True, carry=_Job(jr, st, norm))
        carried.append(eng.carried_jobs - before)
        return out, stats, jr
    three_ways(eng, inputs, call, "conv3d + carried pass", 2)
    assert carried == [1, 1, 1]


def test_rowphase_conv_forward_carry():
    eng = engine()
    conv, norm = eng.refiners[0]["res"][1]
    assert conv.dilation == 2
    rows, cols, n, jn = 64, 64, 3, 2
    with _Form(eng, 1):
        _carry_case(eng, conv, norm, randn(1066, n, 32, rows, cols), randn(1067, jn, 32, rows, cols),
                    randn(1068, jn, 32, rows, cols), jn, n, False, True, 1, "row-phase conv + carried pass")


# ---- 32 -> 1 layers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("rows,cols,n", [(37, 68, 1), (5, 4, 3)])
def test_conv_to1_2d(rows, cols, n, with_prior):
    eng = engine()
    c = conv_for(1, 32, 3)
    inputs = dict(x=randn(rows * 7, n, 32, rows, cols), prior=rand(rows, n, 1, rows, cols) * 3.0, fx=rand(cols, n) * 50 + 10)

    def call(x, prior, fx):
        out = eng.conv_to1(c, x, prior, fx) if with_prior else eng.conv_to1(c, x)
        assert out is not None
        return out
    three_ways(eng, inputs, call, "conv_to1 2-D")


@pytest.mark.parametrize("depth,rows,cols,n", [(8, 4, 8, 2), (5, 30, 40, 1), (33, 17, 36, 1)])
def test_conv_to1_3d(depth, rows, cols, n):
    eng = engine()
    c = conv_for(1, 32, 3, dims=3)

    def call(x):
        out = eng.conv_to1(c, x)
        assert out is not None
        return out
    three_ways(eng, dict(x=randn(rows * 7 + depth, n, 32, depth, rows, cols)), call, "conv_to1 3-D")


def test_conv_to1_volume_norm():
    eng = engine()
    n, depth, rows, cols = 2, 5, 30, 40
    inputs = dict(x=randn(8, n, 32, depth, rows, cols), st=gn_stats(n, 8))
    three_ways(eng, inputs, lambda x, st: eng.conv_to1_volume_norm(eng.vf_convs[4], x, st, eng.vf_norms[3]),
               "conv_to1_volume_norm")


@pytest.mark.parametrize("rows,cols,n,with_res", [(37, 68, 1, True), (5, 4, 3, False)])
def test_conv_to1_block(rows, cols, n, with_res):
    eng = engine()
    c = conv_for(1, 32, 3)
    inputs = dict(r=randn(rows * 3 + cols, n, 32, rows, cols) * 1.5 + 0.3, x=randn(rows * 3 + cols + 1, n, 32, rows, cols),
                  st=gn_stats(n, rows), prior=rand(rows, n, 1, rows, cols) * 3.0, fx=rand(cols, n) * 50 + 10)
    three_ways(eng, inputs, lambda r, x, st, prior, fx: eng.conv_to1_block(c, r, st, norm0(eng), x if with_res else None,
                                                                           prior, fx), "conv_to1_block")


def test_conv_to1_block_from_records_through_the_level3_refiner():
    eng = engine()
    n, rows, cols = 2, 32, 64
    cin = eng.refiners[3]["conv0"].cin
    inputs = dict(guide=rand(21, n, cin - 1, rows, cols), prior=rand(22, n, 1, rows, cols) * 0.5,
                  fx=torch.tensor([300.0 / 8, 260.0 / 8]))
    keep = (eng.lazy_stats_max_samples, eng.lazy_stats_max_records)
    eng.lazy_stats_max_samples, eng.lazy_stats_max_records = 8, 1 << 20
    eng.timeline = []
    try:
        eng.idepth_refiner(3, *[inputs[k].to(DEV) for k in ("guide", "prior", "fx")])
        names = [e[0] for e in eng.timeline]
    finally:
        eng.timeline = None
    try:
        # (records are handed over: only the head's statistics are finalised by a launch of their own)
        assert sum(1 for k in names if k == "mvsn_groupnorm_finalize") == 1, names
        three_ways(eng, inputs, lambda guide, prior, fx: eng.idepth_refiner(3, guide, prior, fx), "refiner 3 from records", 8)
    finally:
        eng.lazy_stats_max_samples, eng.lazy_stats_max_records = keep


# ---- GroupNorm passes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(5, 4), (37, 68), (64, 128)])
def test_groupnorm_passes(rows, cols):
    eng = engine()
    n = 2
    conv, norm = eng.refiners[0]["res"][0]
    inputs = dict(r=randn(rows, n, 32, rows, cols), res=randn(rows + 1, n, 32, rows, cols), st=gn_stats(n, 1),
                  st0=gn_stats(n, 2))
    nrm0 = norm0(eng)
    three_ways(eng, inputs, lambda r, res, st, st0: eng.gn_lrelu(r, st, norm), "gn_lrelu")
    three_ways(eng, inputs, lambda r, res, st, st0: eng.gn_lrelu(r, st, norm, residual=res), "gn_lrelu + residual")
    three_ways(eng, inputs, lambda r, res, st, st0: eng.gn_lrelu(r, st, norm, residual=res, out=r), "gn_lrelu in place", 0)
    three_ways(eng, inputs, lambda r, res, st, st0: eng.gn_lrelu_add2(r, st, norm, res, st0, nrm0), "gn_lrelu_add2")

    def from_records(r, res, st, st0):
        raw, rec = eng.conv(conv, r, want_stats=True, lazy_stats=True)
        assert isinstance(rec, _Records), "the layer must hand its records over at this size"
        one = eng.gn_lrelu(raw, rec, norm, residual=res)
        two = eng.gn_lrelu_add2(raw, rec, norm, res, st0, nrm0)
        return raw, rec, one, two, eng.gn_lrelu(raw, rec, norm, out=raw)
    three_ways(eng, inputs, from_records, "gn passes from records", 4)


@pytest.mark.parametrize("records", [1, 257, 2049])
def test_finalize_stats(records):
    eng = engine()
    n = 2
    g = torch.Generator().manual_seed(records)
    cnt = torch.randint(0, 3, (n, records, 4, 1), generator=g).float() * 64.0
    cnt[:, 0] = 64.0
    mean = torch.randn(n, records, 4, 1, generator=g) * 0.5 + 0.3
    m2 = torch.rand(n, records, 4, 1, generator=g) * cnt * 0.7
    split = eng.lib.mvsn_groupnorm_finalize_split_workspace_bytes(n, records) > 0
    assert split == (records > 2048) and eng.split_finalize
    three_ways(eng, dict(part=torch.cat([cnt, mean, m2], 3).contiguous()), lambda part: eng.finalize_stats(part),
               "finalize_stats", 2 if split else 1)


# ---- towers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
def test_tower_extractor_tail(n):
    eng = engine()

    def call(x):
        out = eng.tower_extractor_tail(x)
        assert out is not None
        return out
    three_ways(eng, dict(x=randn(17 + n, n, 32, 16, 32)), call, "tower_extractor_tail")


@pytest.mark.parametrize("B,S", [(1, 1), (2, 3)])
def test_tower_refiner4(B, S):
    eng = engine()
    inputs = dict(img=rand(1, B, 3, 16, 32) * 2 - 1, feats=randn(2, B, 32, 16, 32),
                  prior=0.02 + 0.2 * rand(3, S * B, 1, 16, 32), fx=20.0 + 10.0 * rand(4, B))

    def call(img, feats, prior, fx):
        out = eng.tower_refiner4(img, feats, prior, fx)
        assert out is not None
        return out
    three_ways(eng, inputs, call, "tower_refiner4")


# ---- homography_warp ------------------------------------------------------------------------------------------------
def _warp_inputs(B, C, n, rows, cols):
    g = torch.Generator().manual_seed(rows * cols + n)
    img = torch.rand(B, C, rows, cols, generator=g) * 2 - 1
    H = torch.eye(3).repeat(B, n, 1, 1) + 0.04 * (torch.rand(B, n, 3, 3, generator=g) - 0.5)
    H[..., 0, 2] += (torch.rand(B, n, generator=g) - 0.5) * cols * 0.5
    H[..., 1, 2] += (torch.rand(B, n, generator=g) - 0.5) * rows * 0.5
    H[..., 2, :2] *= 0.02
    return dict(image=img, H=H)


@pytest.mark.parametrize("B,C,n,rows,cols,many", [(1, 3, 16, 4, 8, False), (1, 5, 4, 7, 9, False),        # one pixel per thread
                                                  (32, 3, 1, 256, 512, True), (40, 3, 3, 61, 576, True)])  # four, >= 32 frames
def test_homography_warp(B, C, n, rows, cols, many):
    eng = engine()
    threads = (rows * cols + 255) // 256 * 256 * n * B
    assert (cols % 4 == 0 and threads // 4 >= 16 * 64 * 4 * 256) == many     # (csrc/mvsn_warp.hip: warp_launch, 256 CUs)
    three_ways(eng, _warp_inputs(B, C, n, rows, cols), lambda image, H: eng.homography_warp(image, H), "homography_warp", 2)


# ---- incremental_cost_volume ----------------------------------------------------------------------------------------
FORMS = {"direct": _native.CHAIN_DIRECT, "winograd": _native.CHAIN_WINOGRAD, "stepwise": _native.CHAIN_STEPWISE,
         "banded": _native.CHAIN_BANDED}


def _chain_inputs(N, D, grid):
    r4, c4 = grid
    g = torch.Generator().manual_seed(41 + N)
    H, Hinc = _motion_family(N, D, "mixed", seed=3)
    return dict(src4=torch.rand(N, 3, r4, c4, generator=g) * 2 - 1, H=H.contiguous(), Hinc=Hinc.contiguous(),
                F0=torch.randn(N, 32, r4, c4, generator=g), FL=torch.randn(N, 32, r4, c4, generator=g))


def _chain_case(grid, D, N, form, bf16=False, slab=False):
    net = net_for(WNAME)
    eng = engine()
    r4, c4 = grid
    status = []

    def call(src4, H, Hinc, F0, FL):
        cost, mask, fvol = eng.incremental_cost_volume(src4, H, Hinc, F0, FL, want_features=True, cost_bf16=bf16)
        torch.cuda.synchronize()
        assert eng.last_chain_form == FORMS[form], (eng.last_chain_form, form)
        status.append(eng.chain_status())
        return cost, mask, fvol
    net.options.chain_form = form
    try:
        if form == "banded":
            groups = eng.lib.mvsn_incremental_cost_volume_banded_groups(N, r4, c4)
            assert (groups == {(30, 40): 3, (32, 64): 4}.get(grid)) == slab, (groups, "the plan query")
        cost, mask, fvol = three_ways(eng, _chain_inputs(N, D, grid), call, f"chain[{form}] {r4}x{c4} D={D} N={N}", 3)
    finally:
        net.options.chain_form = "auto"
    assert status == [0, 0, 0], status
    assert cost.dtype == (torch.bfloat16 if bf16 else torch.float32)
    assert bool(torch.isfinite(cost.float()).all()) and bool(torch.isfinite(fvol).all())


@pytest.mark.parametrize("grid,D,N,form", [((16, 32), 3, 2, "winograd"), ((16, 32), 3, 2, "banded"), ((16, 32), 3, 2, "direct"),
                                           ((30, 40), 3, 2, "banded"), ((30, 40), 3, 2, "stepwise"), ((30, 40), 3, 2, "direct"),
                                           ((32, 64), 2, 2, "banded"), ((15, 30), 3, 1, "direct")])
def test_incremental_cost_volume(grid, D, N, form):
    _chain_case(grid, D, N, form)


def test_incremental_cost_volume_slab_plan():
    _chain_case((30, 40), 2, 18, "banded", slab=True)


def test_incremental_cost_volume_bf16_cost():
    _chain_case((16, 32), 3, 2, "winograd", bf16=True)


# ---- tails through the engine wrappers ------------------------------------------------------------------------------
def test_tails():
    eng = engine()
    N, D, rows, cols = 3, 7, 9, 13
    cost, samples = randn(1, N, D, rows, cols) * 3, rand(2, N, D) + 0.01
    three_ways(eng, dict(cost=cost, samples=samples), lambda cost, samples: eng.soft_argmin(cost, samples), "soft_argmin")
    three_ways(eng, dict(cost=cost, samples=samples), lambda cost, samples: eng.soft_argmin_confidence(cost, samples),
               "soft_argmin_confidence", 2)
    x = rand(3, 2, 3, 5, 7)
    three_ways(eng, dict(x=x), lambda x: eng.upsample(x, (9, 13)), "upsample")
    three_ways(eng, dict(x=x[:, :1].contiguous(), fx=rand(4, 2) * 50 + 10), lambda x, fx: eng.upsample_prior(x, fx, (9, 13)),
               "upsample_prior", 2)
    three_ways(eng, dict(m=rand(5, 2, 12, 5, 7) > 0.5), lambda m: eng.upsample_mask(m, (9, 13)), "upsample_mask")
    S, B = 3, 2
    inputs = dict(raw=rand(6, S * B, 1, rows, cols), refined=rand(7, S * B, 1, rows, cols), baseline=rand(8, S * B) + 0.1,
                  mask=rand(9, S * B, D, rows, cols) > 0.5)
    three_ways(eng, inputs, lambda raw, refined, baseline, mask: eng.fuse_sources(raw, refined, baseline, mask, S, B, False),
               "fuse_sources", 3)


# ---- whole forwards -------------------------------------------------------------------------------------------------
def _forward_case(rows, cols, S, B, D, planned, seed, jitter=0.0):
    net = net_for(WNAME)
    eng = engine()
    batch = synthetic.make_batch(rows, cols, S, batch=B, seed=seed, pose_jitter=jitter, smooth=True)
    inp = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
    inputs = dict(lp=list(inp["left_image_pyr"]), kp=list(inp["K_pyr"]), ts=list(inp["T_right_in_left"]),
                  rp=[list(p) for p in inp["right_image_pyr"]])
    recorded = []

    def call(lp, kp, ts, rp):
        eng.plans.clear()                 # (planned: every one of the three is the first -- recording -- forward of its shape)
        before = eng.replays
        out = net(lp, kp, ts, rp, D, True, [True] * 5)
        assert net.engine() is eng and eng.replays == before
        recorded.append(sum(1 for p in eng.plans.values() if p is not None))
        return out
    old, plans = net.options.plan_max_chains, dict(eng.plans)
    net.options.plan_max_chains = 16 if planned else 0
    try:
        out = three_ways(eng, inputs, call, f"forward {rows}x{cols} S={S} B={B} D={D} planned={planned}", 50)
    finally:
        net.options.plan_max_chains = old
        eng.plans.clear()                 # the plans recorded under the guard go; the ones from before come back
        eng.plans.update(plans)
    assert recorded == [1 if planned else 0] * 3, recorded
    assert len(out) == 15 and all(bool(torch.isfinite(t.float()).all()) for t in out)


@pytest.mark.parametrize("planned", [False, True])
def test_forward_64x128(planned):
    _forward_case(64, 128, 2, 1, 8, planned, seed=123)


def test_forward_ragged_eager():
    _forward_case(131, 277, 2, 2, 8, False, seed=131 + 277, jitter=0.2)


# ---- the last test of the module ------------------------------------------------------------------------------------
def test_engine_empty_is_the_class_method_again():
    assert _ENGINES, "no case ran"
    for eng in _ENGINES + [net_for(WNAME).engine()]:
        assert "empty" not in vars(eng)
        assert eng.empty.__func__ is PlaneSweepEngine.empty
    assert engine().lib.mvsn_debug_set_wino_rowphase(0) == 0          # (no case left a kernel form pinned)
