"""The volume form (3x3x3 regulariser layer, conv_wino_kernel<.., VOL, RIDE = 1>) carrying an in-place LReLU(GN(.)) pass
over another volume.  Those launches load the carried units by inline assembly and guard them, like the DMA ring, with ONE
hand-counted `s_waitcnt vmcnt(N)` per step (mvsn_conv_wino.hip rd_issue / do_step; the static side of the guard is
tools/check_dma_isa.py).  A miscounted wait shows as a rare stale word, a wrong unit index as a word outside the job: so
every case compares every word -- the layer's output, its statistics and the carried pass -- with `torch.equal` against the
two-call reference (plain `eng.conv` + `eng.gn_lrelu`), with the job and the output inside larger buffers whose other words
must not change."""
import pytest
import torch

from test_hip_parity import net_for
from multi_view_stereonet_amd.multi_view_stereonet import _Job

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
WNAME = "gta_sfm_150epochs"
BAND = 16384          # guard words on either side (64 KiB: the size of one tile's share of a job)
_REF = {}             # (n, jn, depth, rows, cols, mode1) -> inputs and the two-call reference, computed once


def _gn_stats(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randn(n, 4, generator=g) * 0.1, 1.0 + torch.rand(n, 4, generator=g)], -1).contiguous().to(DEV)


def _layer():
    eng = net_for(WNAME).engine()
    return eng, eng.vf_convs[1], eng.vf_norms[0]


def _reference(n, jn, depth, rows, cols, mode1):
    key = (n, jn, depth, rows, cols, mode1)
    if key not in _REF:
        eng, conv, norm = _layer()
        g = torch.Generator().manual_seed(1000 * n + 100 * jn + depth + rows)
        x = torch.randn(n, 32, depth, rows, cols, generator=g).to(DEV)
        jr = torch.randn(jn, 32, depth, rows, cols, generator=g).to(DEV)
        st, ist = _gn_stats(jn, 4), _gn_stats(n, 5)
        kw = dict(in_stats=ist, in_norm=norm) if mode1 else {}
        want_out, want_st = eng.conv(conv, x, want_stats=True, **kw)
        want_job = eng.gn_lrelu(jr, st, norm)
        torch.cuda.synchronize()
        _REF[key] = dict(x=x, jr=jr, st=st, kw=kw, want_out=want_out, want_st=want_st, want_job=want_job)
    return _REF[key]


class Banded:
    """A tensor inside a larger buffer of NaN words (0xFFFFFFFF), 16-byte aligned like the library asks."""

    def __init__(self, shape):
        numel = 1
        for s in shape:
            numel *= s
        self.flat = torch.full((BAND + numel + BAND,), -1, dtype=torch.int32, device=DEV)
        self.view = self.flat[BAND:BAND + numel].view(torch.float32).view(shape)

    def bands_intact(self):
        return bool((self.flat[:BAND] == -1).all() and (self.flat[-BAND:] == -1).all())


def _launch(r, job_buf, out_buf, reverse=0):
    """One carrying call on fresh copies; returns (carried launches, everything equal, bands intact)."""
    eng, conv, norm = _layer()
    job_buf.view.copy_(r["jr"])
    job = _Job(job_buf.view, r["st"], norm)
    job.job.reverse = reverse
    before = eng.carried_jobs
    got_out, got_st = eng.conv(conv, r["x"], want_stats=True, carry=job, out=out_buf.view, **r["kw"])
    ok = torch.equal(got_out, r["want_out"]) and torch.equal(got_st, r["want_st"]) and torch.equal(job_buf.view, r["want_job"])
    return eng.carried_jobs - before, ok, job_buf.bands_intact() and out_buf.bands_intact()


# (n, jn, depth, rows, cols, mode1, reverse, carried)
CASES = [
    pytest.param(2, 2, 4, 16, 32, False, 0, 1, id="exact-fit"),
    pytest.param(2, 2, 4, 16, 32, False, 1, 1, id="exact-fit-reverse"),
    pytest.param(2, 2, 4, 16, 32, True, 0, 1, id="exact-fit-input-transform"),
    pytest.param(1, 1, 1, 16, 32, False, 0, 1, id="one-plane"),            # every step has a zero plane
    pytest.param(1, 1, 2, 16, 32, False, 0, 1, id="two-planes"),           # a tile's first / last step
    pytest.param(1, 1, 3, 16, 32, False, 0, 1, id="three-planes"),         # (the issue's capacity-edge row: 192 of 288 units)
    pytest.param(2, 3, 3, 16, 32, False, 0, 1, id="capacity-edge"),        # 576 units on 6 items x 96: the last index that fits
    pytest.param(2, 3, 3, 16, 32, False, 1, 1, id="capacity-edge-reverse"),
    pytest.param(1, 2, 4, 16, 32, False, 0, 0, id="job-too-large"),        # 512 units > 384: own launch, same result
    pytest.param(3, 1, 4, 16, 32, False, 0, 1, id="short-job"),            # most steps have no unit
    pytest.param(6, 6, 64, 16, 32, False, 0, 1, id="more-items-than-cus"),   # 384 work items, ragged last round
    pytest.param(6, 6, 64, 16, 32, False, 1, 1, id="more-items-than-cus-reverse"),
    pytest.param(6, 6, 64, 16, 32, True, 1, 1, id="more-items-than-cus-input-transform"),
    pytest.param(2, 2, 3, 32, 64, False, 0, 1, id="tiles-32x64"),          # 2 x 2 tiles of 16 x 32 per plane (not full-width)
    pytest.param(2, 2, 3, 32, 64, True, 1, 1, id="tiles-32x64-input-transform-reverse"),
    pytest.param(2, 2, 3, 30, 40, False, 0, 0, id="wide-30x40-three-planes"),   # 3 x 1200 % 256 != 0: own launch
    pytest.param(2, 2, 16, 30, 40, False, 0, 1, id="wide-30x40"),          # the wide-tile / rolling-strip carriers
    pytest.param(2, 2, 16, 30, 40, True, 1, 1, id="wide-30x40-input-transform-reverse"),
]


@pytest.mark.parametrize("n,jn,depth,rows,cols,mode1,reverse,carried", CASES)
def test_volume_carrier_is_bit_identical_and_stays_inside(n, jn, depth, rows, cols, mode1, reverse, carried):
    r = _reference(n, jn, depth, rows, cols, mode1)
    job_buf, out_buf = Banded(r["jr"].shape), Banded(r["want_out"].shape)
    count, ok, intact = _launch(r, job_buf, out_buf, reverse)
    assert count == carried, "the pass travelled inside the launch" if count else "the pass did not travel inside the launch"
    assert ok, "output, statistics or carried pass differ from the two-call reference"
    assert intact, "words outside the job or the output were written"


@pytest.mark.parametrize("n,jn,depth", [pytest.param(2, 2, 4, id="exact-fit"), pytest.param(6, 6, 64, id="more-items-than-cus")])
def test_volume_carrier_stress(n, jn, depth):
    """200 launches per shape, the walk direction changing every third launch, every word compared each time."""
    r = _reference(n, jn, depth, 16, 32, False)
    job_buf, out_buf = Banded(r["jr"].shape), Banded(r["want_out"].shape)
    bad = carried = 0
    for it in range(200):
        count, ok, intact = _launch(r, job_buf, out_buf, reverse=0 if it % 3 else 1)
        carried += count
        bad += 0 if (ok and intact) else 1
    assert carried == 200, "the pass did not travel inside the launch: nothing was stressed"
    assert bad == 0, f"{bad} of 200 launches differed from the two-call reference"


@pytest.mark.parametrize("n,depth,grow", [(2, 4, 6), (3, 5, 3), (5, 8, 6)])
def test_sliced_filter_equals_unsliced(n, depth, grow):
    """cost_volume_filter_sliced against the one-batch filter.  Six passes (three layers x two slices) ride for even n; at
    n = 3 slice A (two chains, 128 units per plane) does not fit the launches of slice B (one chain, capacity 96) and runs
    on its own; at n = 5 slice A's three chains (192) fit slice B's two (capacity 192) exactly."""
    net = net_for(WNAME)
    eng = net.engine()
    g = torch.Generator().manual_seed(60 + n)
    cost = torch.rand(n, 32, depth, 16, 32, generator=g).to(DEV)
    old = (net.options.carry_passes, net.options.carry_min_bytes, net.options.carry_volume_passes)
    try:
        net.options.carry_volume_passes = True
        net.options.carry_passes = False
        want = eng.cost_volume_filter(cost)
        net.options.carry_passes, net.options.carry_min_bytes = True, 0
        before = eng.carried_jobs
        got = eng.cost_volume_filter(cost)
        torch.cuda.synchronize()
        assert eng.carried_jobs - before == grow
        assert torch.equal(got, want)
    finally:
        net.options.carry_passes, net.options.carry_min_bytes, net.options.carry_volume_passes = old
