"""The small kernels either side of the cost-volume regulariser (csrc/mvsn_misc.hip,
mvsn_image_pyramid of csrc/mvsn_prepare.hip) against the restatements of tests/tail_reference.py, at the shapes where
such kernels go wrong: ragged widths, D % 16 != 0, pixel counts off the block size, partial tiles, S = 3, unaligned
copies.  Every tolerance is a bound of tail_reference.py, which tests/test_tail_reference_cpu.py shows ATen's own float32
results to keep on the same inputs."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import tail_reference as tr
from test_hip_parity import net_for
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd import multi_view_stereonet_utils as snu

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
SENTINEL = -7777.0
PAD = 64            # sentinel elements either side of an output


def engine():
    return net_for("gta_sfm_150epochs").engine()


def guarded(numel, dtype=torch.float32, fill=SENTINEL):
    """A buffer of PAD + numel + PAD elements filled with the sentinel, and the address of element PAD."""
    buf = torch.full((numel + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return buf, buf.data_ptr() + PAD * buf.element_size()


def guards_intact(buf, numel, fill=SENTINEL):
    host = buf.cpu()
    return bool((host[:PAD] == fill).all()) and bool((host[PAD + numel:] == fill).all())


def same_or_both_nan(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


# ---- soft-argmin -----------------------------------------------------------------------------------------------------
def _soft_argmin_within_bound(got, ref, samples, D, what):
    worst = 0.0
    for i in range(ref.shape[0]):
        ok = ~ref[i].isnan()
        assert torch.equal(got[i].isnan(), ref[i].isnan()), what
        frac = float((got[i].double() - ref[i])[ok].abs().max()) / tr.soft_argmin_bound(D, samples[i]) if bool(ok.any()) else 0.0
        worst = max(worst, frac)
    print(f"soft-argmin {what}: {worst:.3f} of the bound")
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("n,rows,cols", tr.SOFT_ARGMIN_SHAPES)
@pytest.mark.parametrize("D", tr.SOFT_ARGMIN_D)
def test_soft_argmin(D, n, rows, cols):
    eng = engine()
    for scale in tr.SOFT_ARGMIN_SCALES:
        cost, samples = tr.soft_argmin_inputs(n, D, rows, cols, scale)
        got = eng.soft_argmin(cost.to(DEV), samples.to(DEV)).cpu()
        assert got.shape == (n, 1, rows, cols)
        _soft_argmin_within_bound(got, tr.soft_argmin_ref(cost, samples), samples, D, f"D={D} {n}x{rows}x{cols} scale {scale:g}")
    # all costs equal: the mean of the samples
    flat = torch.full((n, D, rows, cols), 3.0)
    got = eng.soft_argmin(flat.to(DEV), samples.to(DEV)).cpu()
    mean = samples.double().mean(1).view(n, 1, 1, 1).expand(n, 1, rows, cols)
    _soft_argmin_within_bound(got, mean, samples, D, f"D={D} {n}x{rows}x{cols} constant cost")


@pytest.mark.parametrize("D,d_nan", [(17, 16), (33, 5), (5, 0)])     # the NaN in the scalar tail, in a vector round, first
def test_soft_argmin_nan_stays_in_its_pixel(D, d_nan):
    eng = engine()
    cost, samples = tr.soft_argmin_inputs(3, D, 7, 37, 50.0)
    cost[1, d_nan, 2, 5] = float("nan")
    ref = tr.soft_argmin_ref(cost, samples)
    assert int(ref.isnan().sum()) == 1
    got = eng.soft_argmin(cost.to(DEV), samples.to(DEV)).cpu()
    assert bool(got[1, 0, 2, 5].isnan()) and int(got.isnan().sum()) == 1
    _soft_argmin_within_bound(got, ref, samples, D, f"D={D} NaN at d={d_nan}")


# ---- bilinear resize -------------------------------------------------------------------------------------------------
def _bilinear_within_bound(got, x, out, what):
    ref = tr.bilinear_ref(x, out)
    bound = tr.BILINEAR_FACTOR * tr.EPS * float(x.abs().max())
    err = float((got.double() - ref).abs().max())
    print(f"bilinear {what} {tuple(x.shape)} -> {tuple(out)}: {err / bound * tr.BILINEAR_FACTOR:.2f} * 2^-24 * max|x|")
    assert got.shape == ref.shape and err <= bound, (what, tuple(x.shape), out, err / bound)
    # corners and edges against the clamped taps.  Output 0 of an axis has source index 0 and weights (1, 0): pixel
    # (0, 0) is input (0, 0), exactly.  The last output of an axis has both taps on the last input index, so the last
    # row / column is the 1-D resize of the input's last row / column alone (and the first likewise).
    assert torch.equal(got[..., 0, 0], x[..., 0, 0])

    def row_alone(r):           # output row r (0 or -1) from input row r alone
        return float((got[..., r, :].double() - tr.bilinear_ref(x[..., r:, :][..., :1, :], (1, out[1]))[..., 0, :]).abs().max())

    def col_alone(c):
        return float((got[..., :, c].double() - tr.bilinear_ref(x[..., :, c:][..., :, :1], (out[0], 1))[..., :, 0]).abs().max())

    for edge_err in (row_alone(0), row_alone(-1), col_alone(0), col_alone(-1)):
        assert edge_err <= bound, (what, tuple(x.shape), out)
    for cy, cx in ((0, -1), (-1, 0), (-1, -1)):
        assert float((got[..., cy, cx].double() - x[..., cy, cx].double()).abs().max()) <= bound


def test_upsample_bilinear():
    eng = engine()
    for x, out in tr.bilinear_inputs():
        got = eng.upsample(x.to(DEV), out).cpu()
        _bilinear_within_bound(got, x, out, "upsample")


def test_upsample_prior_two_outputs():
    eng = engine()
    for x, fx, out in tr.prior_inputs():
        assert x.shape[0] == tr.PRIOR_N and len(set(fx.tolist())) == tr.PRIOR_N
        first, scaled = eng.upsample_prior(x.to(DEV), fx.to(DEV), out)
        first, scaled = first.cpu(), scaled.cpu()
        _bilinear_within_bound(first, x, out, "upsample_prior")
        assert torch.equal(scaled, first * fx.view(-1, 1, 1, 1))
        plain = eng.upsample(x.to(DEV), out).cpu()
        print(f"upsample / upsample_prior {tuple(x.shape[-2:])} -> {tuple(out)}: bit-identical = {torch.equal(plain, first)}")


def test_upsample_mask_against_the_blend():
    eng = engine()
    for planes in tr.BILINEAR_PLANES:
        for size, out in tr.BILINEAR_SIZES:
            m = tr.mask_input(planes, size)
            ref, blend = tr.bilinear_mask_ref(m, out)
            decided = (blend - 0.5).abs() > 2.0 ** -20
            got = eng.upsample_mask(m.to(DEV), out).cpu()
            assert got.dtype == torch.bool and torch.equal(got[decided], ref[decided]), (size, out)


# ---- area downsample and the one-launch pyramid ----------------------------------------------------------------------------
def _area_downsample(lib, x_dev, out_ptr=None):
    n, c, rows, cols = x_dev.shape
    out = None
    if out_ptr is None:
        out = torch.empty(n, c, (rows + 1) // 2, (cols + 1) // 2, device=DEV)
        out_ptr = out.data_ptr()
    _native.check(lib.mvsn_area_downsample(_native.ptr(x_dev), n, c, rows, cols, out_ptr, _native.stream()), "area")
    return out


@pytest.mark.parametrize("planes", tr.AREA_PLANES)
def test_area_downsample(planes):
    lib = _native.load()
    for rows, cols in tr.AREA_SIZES:
        x = tr.image_input(planes, rows, cols)
        ro, co = (rows + 1) // 2, (cols + 1) // 2
        buf, ptr = guarded(planes * ro * co)
        _area_downsample(lib, x.to(DEV), ptr)
        got = buf[PAD:PAD + planes * ro * co].view(1, planes, ro, co).cpu()
        assert guards_intact(buf, planes * ro * co), (rows, cols)
        err = float((got.double() - tr.area_downsample_ref(x)).abs().max()) / (tr.EPS * float(x.abs().max()))
        print(f"area {rows}x{cols} x{planes}: {err:.2f} * 2^-24 * max|x|")
        assert err <= tr.AREA_FACTOR, (rows, cols, err)
        if rows % 2 == 0 and cols % 2 == 0:
            assert torch.equal(got, F.interpolate(x, (ro, co), mode="area")), (rows, cols)


@pytest.mark.parametrize("planes", tr.AREA_PLANES)
@pytest.mark.parametrize("rows,cols,levels", tr.PYRAMID_CASES)
def test_image_pyramid_one_launch(rows, cols, levels, planes):
    lib = _native.load()
    assert lib.mvsn_image_pyramid_supported(rows, cols, levels) == 1
    x = tr.image_input(planes, rows, cols)
    xd = x.to(DEV)
    sizes = [(rows >> l, cols >> l) for l in range(1, levels)]
    bufs = [guarded(planes * r * c) for r, c in sizes]
    ptrs = (ctypes.c_void_p * len(bufs))(*[p for _, p in bufs])
    _native.check(lib.mvsn_image_pyramid(_native.ptr(xd), 1, planes, rows, cols, levels, ptrs, _native.stream()), "pyramid")
    ref = tr.pyramid_ref(x, levels)
    chain = xd
    for l, ((r, c), (buf, _)) in enumerate(zip(sizes, bufs), start=1):
        numel = planes * r * c
        assert guards_intact(buf, numel), f"level {l}: the sentinel either side of the level did not survive"
        got = buf[PAD:PAD + numel].view(1, planes, r, c)
        assert ref[l].shape == got.shape
        assert torch.equal(got.cpu(), ref[l]), f"level {l} of {rows}x{cols}"
        chain = _area_downsample(lib, chain)
        assert torch.equal(got, chain), f"level {l} of {rows}x{cols} against the per-level kernel"
    # the wrapper takes this launch
    pyr = snu.build_image_pyramid(xd, levels)
    assert len(pyr) == levels and all(torch.equal(a.cpu(), b) for a, b in zip(pyr, ref))


@pytest.mark.parametrize("rows,cols,levels", tr.PYRAMID_UNSUPPORTED)
def test_image_pyramid_sizes_that_do_not_halve_exactly(rows, cols, levels, monkeypatch):
    lib = _native.load()
    assert lib.mvsn_image_pyramid_supported(rows, cols, levels) == 0
    x = tr.image_input(7, rows, cols)
    xd = x.to(DEV)
    outs = [torch.empty(1, 7, max(rows >> l, 1), max(cols >> l, 1), device=DEV) for l in range(1, levels)]
    ptrs = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    assert lib.mvsn_image_pyramid(_native.ptr(xd), 1, 7, rows, cols, levels, ptrs, _native.stream()) != 0
    assert b"not divisible" in lib.mvsn_last_error()
    calls = []
    one_launch, per_level = lib.mvsn_image_pyramid, lib.mvsn_area_downsample
    monkeypatch.setattr(lib, "mvsn_image_pyramid", lambda *a: calls.append("pyramid") or one_launch(*a))
    monkeypatch.setattr(lib, "mvsn_area_downsample", lambda *a: calls.append("level") or per_level(*a))
    pyr = snu.build_image_pyramid(xd, levels)
    assert calls == ["level"] * (levels - 1)
    ref = tr.pyramid_ref(x, levels)
    assert len(pyr) == levels
    for a, b in zip(pyr, ref):
        assert a.shape == b.shape and torch.allclose(a.cpu(), b, rtol=1e-6, atol=1e-6)


# ---- multi-source fusion ---------------------------------------------------------------------------------------------
def _fuse(eng, raw, refined, baseline, mask, S, B):
    out = eng.fuse_sources(raw.to(DEV), None if refined is None else refined.to(DEV), baseline.to(DEV), mask.to(DEV), S, B,
                           alias=refined is None)
    return [o.cpu() for o in out]


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("S", tr.FUSE_S)
def test_fuse_sources(S, alias):
    eng = engine()
    for B in tr.FUSE_B:
        for D in tr.FUSE_D:
            for rows, cols in tr.FUSE_GRIDS:
                raw, refined, baseline, mask = tr.fuse_inputs(S, B, D, rows, cols)
                refined = None if alias else refined
                got_raw, got_ref, got_mask = _fuse(eng, raw, refined, baseline, mask, S, B)
                want_raw, want_ref, want_mask = tr.fuse_ref32(raw, refined, baseline, mask, S, B)
                what = (S, B, D, rows, cols, alias)
                assert got_raw.shape == (B, 1, rows, cols) and got_mask.shape == (B, D, rows, cols)
                assert torch.equal(got_raw, want_raw) and torch.equal(got_ref, want_ref), what
                assert got_mask.dtype == torch.bool and torch.equal(got_mask, want_mask), what
                mean_raw, mean_ref = tr.fuse_ref64(raw, refined, baseline, S, B)      # alias: raw / base^2, averaged
                for got, mean in ((got_raw, mean_raw), (got_ref, mean_ref)):
                    assert float(((got.double() - mean).abs() / mean).max()) <= tr.FUSE_FACTOR * tr.EPS, what
                if alias:
                    assert torch.equal(got_raw, got_ref), what


@pytest.mark.parametrize("S,n_set,want", [(2, 1, False), (4, 2, False), (4, 3, True), (3, 2, True), (3, 1, False),
                                          (1, 1, True), (5, 3, True), (5, 2, False)])
def test_fuse_sources_mask_ties(S, n_set, want):
    eng = engine()
    B, D, rows, cols = 3, 3, 7, 37
    raw, refined, baseline, _ = tr.fuse_inputs(S, B, D, rows, cols)
    mask = tr.tie_mask(S, B, D, rows, cols, n_set)
    got = _fuse(eng, raw, refined, baseline, mask, S, B)[2]
    assert torch.equal(got, tr.fuse_ref32(raw, refined, baseline, mask, S, B)[2])
    assert bool((got == want).all())


def test_fuse_sources_comparison_sees_the_chain_order():
    """Against the reference with chain b*S + s in place of s*B + b every output must differ: the test sees the layout."""
    eng = engine()
    S, B, D, rows, cols = 2, 3, 3, 7, 37
    raw, refined, baseline, mask = tr.fuse_inputs(S, B, D, rows, cols)
    for ref_in in (refined, None):
        got = _fuse(eng, raw, ref_in, baseline, mask, S, B)
        right = tr.fuse_ref32(raw, ref_in, baseline, mask, S, B)
        wrong = tr.fuse_ref32(raw, ref_in, baseline, mask, S, B, chain=tr.chain_bs)
        assert all(torch.equal(a, b) for a, b in zip(got, right))
        assert not any(torch.equal(a, b) for a, b in zip(got, wrong))


# ---- mvsn_copy_many ------------------------------------------------------------------------------------------------------
GUARD_BYTE = 0xA5


def _copy_many(lib, pairs):
    """pairs: (dst address, src address, bytes)."""
    n = len(pairs)
    dp = (ctypes.c_void_p * n)(*[p[0] for p in pairs])
    sp = (ctypes.c_void_p * n)(*[p[1] for p in pairs])
    nb = (ctypes.c_size_t * n)(*[p[2] for p in pairs])
    return lib.mvsn_copy_many(dp, sp, nb, n, _native.stream())


def _run_copies(lib, specs, seed):
    """specs: (bytes, dst misalignment, src misalignment) per pair.  Every pair gets a 16-byte aligned slot of its own in
    one source buffer of random bytes and one destination buffer of guard bytes, moved by its misalignment; afterwards
    the WHOLE destination buffer must be the guard bytes with the sources laid in: no byte either side of a destination
    is touched."""
    g = torch.Generator().manual_seed(seed)
    slots, at = [], 64
    for nbytes, doff, soff in specs:
        slots.append(at)
        at += (nbytes + 15) // 16 * 16 + 64
    src = torch.randint(0, 256, (at,), dtype=torch.uint8, generator=g)
    want = torch.full((at,), GUARD_BYTE, dtype=torch.uint8)
    src_d, dst_d = src.to(DEV), want.to(DEV)
    assert src_d.data_ptr() % 16 == 0 and dst_d.data_ptr() % 16 == 0
    pairs = []
    for (nbytes, doff, soff), slot in zip(specs, slots):
        pairs.append((dst_d.data_ptr() + slot + doff, src_d.data_ptr() + slot + soff, nbytes))
        want[slot + doff:slot + doff + nbytes] = src[slot + soff:slot + soff + nbytes]
    _native.check(_copy_many(lib, pairs), "mvsn_copy_many")
    got = dst_d.cpu()
    for (nbytes, doff, soff), slot in zip(specs, slots):
        assert torch.equal(got[slot + doff:slot + doff + nbytes], src[slot + soff:slot + soff + nbytes]), (nbytes, doff, soff)
    assert torch.equal(got, want), "a byte outside the destinations changed"


def test_copy_many_alignment_paths():
    lib = _native.load()
    assert lib.mvsn_copy_many(None, None, None, 0, _native.stream()) == 0          # nothing to do
    _run_copies(lib, [(4096, 0, 0)], 1)                                             # one pair, 16-byte accesses
    _run_copies(lib, [(16, 0, 0)], 2)
    seed = 3
    for k in (1, 4, 8):         # one pair of three off the 16-byte path by its size, its destination or its source
        for odd in ((1024 + k, 0, 0), (1024, k, 0), (1024, 0, k), (1024 - k, k, k)):
            _run_copies(lib, [(2048, 0, 0), odd, (528, 0, 0)], seed)
            seed += 1
    _run_copies(lib, [(1024, 0, 0), (0, 0, 0), (777, 0, 0)], 20)                    # a zero-length pair between two others
    _run_copies(lib, [(0, 0, 0), (0, 0, 0)], 21)                                    # only zero-length pairs: no launch


@pytest.mark.parametrize("count", [9, 17])
def test_copy_many_beyond_one_launch(count):
    lib = _native.load()
    specs = [(16 * (3 + 5 * i) + (i % 3 == 1) * (i % 7), (i % 4 == 2) * 4, (i % 5 == 3) * 8) for i in range(count)]
    specs[8] = (4000, 0, 0)          # the first pair of the second launch
    assert any(s[0] % 16 for s in specs) and any(s[1] for s in specs) and any(s[2] for s in specs)
    _run_copies(lib, specs, 30 + count)


@pytest.mark.parametrize("extra", [16, 3])      # 16-byte accesses / bytes
def test_copy_many_past_the_grid(extra):
    """6 MB: more 16-byte pieces than 1024 blocks of 256 threads hold, so the stride loop turns."""
    lib = _native.load()
    _run_copies(lib, [(6 * 1024 * 1024 + extra, 0, 0), (48, 0, 0)], 40 + extra)


def test_copy_many_rejects_null_pointers():
    lib = _native.load()
    before = torch.cat([torch.zeros(32, dtype=torch.uint8), torch.arange(1, 33, dtype=torch.uint8)])
    buf = before.to(DEV)          # a valid pair would copy the pattern of the second half over the zeros of the first
    for pairs in ([(None, buf.data_ptr(), 16)], [(buf.data_ptr(), None, 16)],
                  [(buf.data_ptr(), buf.data_ptr() + 32, 16), (None, None, 1)]):
        assert _copy_many(lib, pairs) != 0
        assert b"mvsn_copy_many" in lib.mvsn_last_error()
    assert lib.mvsn_copy_many(None, None, None, 2, _native.stream()) != 0
    assert b"mvsn_copy_many" in lib.mvsn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), before), "a launch went out before the null pair was rejected"


# ---- gathers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 70])
@pytest.mark.parametrize("levels", [1, 5, 8])
def test_gather_focal(levels, batch):
    eng = engine()
    g = torch.Generator().manual_seed(levels * 100 + batch)
    K_pyr = [torch.randn(batch, 4, 4, generator=g) for _ in range(levels)]
    got = eng.focal_pyramid([k.to(DEV) for k in K_pyr]).cpu()
    assert torch.equal(got, torch.stack([k[:, 0, 0] for k in K_pyr]))
    # the raw entry point, with sentinels either side of its output
    lib = _native.load()
    Kd = [k.to(DEV) for k in K_pyr]
    buf, ptr = guarded(levels * batch)
    ptrs = (ctypes.c_void_p * levels)(*[k.data_ptr() for k in Kd])
    _native.check(lib.mvsn_gather_focal(ptrs, levels, batch, ptr, _native.stream()), "gather_focal")
    assert torch.equal(buf[PAD:PAD + levels * batch].cpu(), torch.stack([k[:, 0, 0] for k in K_pyr]).reshape(-1))
    assert guards_intact(buf, levels * batch)


@pytest.mark.parametrize("stride", [1, 16, 4099])
@pytest.mark.parametrize("count", [1, 300])
def test_gather_strided(count, stride):
    lib = _native.load()
    g = torch.Generator().manual_seed(count + stride)
    src = torch.randn((count - 1) * stride + 1, generator=g)
    sd = src.to(DEV)
    buf, ptr = guarded(count)
    _native.check(lib.mvsn_gather_strided(_native.ptr(sd), count, stride, ptr, _native.stream()), "gather_strided")
    assert torch.equal(buf[PAD:PAD + count].cpu(), src[::stride])
    assert guards_intact(buf, count)
    if stride == 16:        # the wrapper: K[:, 0, 0] of (B, 4, 4)
        K = torch.randn(count, 4, 4, generator=g)
        assert torch.equal(engine().focal(K.to(DEV)).cpu(), K[:, 0, 0])


# ---- elementwise entry points ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", [1, 257])
def test_refiner_epilogue_nan_stays_in_its_pixel(pixels):
    """relu(prior * fx + delta) / fx with a NaN in delta or in prior: NaN at that pixel only, as torch.relu gives, every
    other pixel exact."""
    lib = _native.load()
    g = torch.Generator().manual_seed(pixels)
    n = 3
    prior = torch.rand(n, pixels, generator=g) * 2
    delta = torch.randn(n, pixels, generator=g) * 40
    fx = torch.tensor([410.0, 25.6, 51.2])
    delta[1, pixels // 2] = float("nan")
    prior[2, pixels - 1] = float("nan")
    sc = fx.view(-1, 1)
    want = torch.relu(prior * sc + delta) / sc
    assert int(want.isnan().sum()) == 2 and bool(want[1, pixels // 2].isnan()) and bool(want[2, pixels - 1].isnan())
    pd, fd, dd = prior.to(DEV), fx.to(DEV), delta.to(DEV)
    buf, ptr = guarded(n * pixels)
    _native.check(lib.mvsn_refiner_epilogue(_native.ptr(pd), _native.ptr(fd), _native.ptr(dd), n, pixels, ptr,
                                            _native.stream()), "epilogue")
    got = buf[PAD:PAD + n * pixels].view(n, pixels).cpu()
    assert torch.equal(got.isnan(), want.isnan()) and same_or_both_nan(got, want)
    assert guards_intact(buf, n * pixels)
    if pixels > 1:
        assert bool((got == 0).any()) and bool((got > 0).any())
