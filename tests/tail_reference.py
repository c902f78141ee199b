"""Plain restatements of the small kernels either side of the cost-volume regulariser (csrc/mvsn_misc.hip,
mvsn_image_pyramid of csrc/mvsn_prepare.hip): soft-argmin, bilinear resize of idepth maps and masks,
the area pyramid, multi-source fusion.

Written from the operations, not from the kernels, in float64 arithmetic -- except where float32 IS the operation:
  * the tap choice and the weights of the bilinear resize.  ATen forms them in float32.  At ragged ratios such as
    8x12 -> 15x23 a weight formed in float64 is another weight, and where the source coordinate falls next to an
    integer it can be another tap;
  * the pyramid: the reference interpolates the previous level's ROUNDED values;
  * the literal restatement of the reference's fusion lines.
No device code.

The shapes and the seeded inputs of tests/test_tail_reference_cpu.py and tests/test_tail_kernels_gpu.py live here, so
the bounds the GPU tests use are shown on the CPU, on the same inputs, to hold for ATen's own float32 results.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24          # half an ulp of 1.0 in float32: the relative rounding error of one float32 operation

# ---- shapes ------------------------------------------------------------------------------------------------------
SOFT_ARGMIN_D = (1, 5, 16, 17, 33, 64)                  # 16: one vector round, no tail; 17, 33: a tail of one; 64: four rounds
SOFT_ARGMIN_SHAPES = ((1, 1, 1), (3, 7, 37), (2, 16, 32), (2, 5, 103))      # (n, rows, cols): 1, 259, 512, 515 pixels
SOFT_ARGMIN_SCALES = (1.0, 50.0, 1e4)

BILINEAR_SIZES = (((16, 32), (32, 64)), ((8, 12), (15, 23)), ((5, 7), (9, 13)), ((1, 8), (2, 16)), ((3, 1), (6, 2)),
                  ((4, 130), (8, 260)),                  # 260 output columns: a second 256-column block
                  ((30, 40), (60, 80)))
BILINEAR_PLANES = (1, 6)
BILINEAR_OFFSET_CASE = ((8, 12), (15, 23))               # the case whose values carry an offset of 100
BILINEAR_FACTOR = 8.0                                    # |got - bilinear_ref| <= BILINEAR_FACTOR * EPS * max|x|
PRIOR_N = 5
PRIOR_FX = (410.0, 25.6, 51.2, 102.4, 7.3)

AREA_SIZES = ((5, 7), (1, 9), (9, 1), (37, 53), (3, 515), (2, 2), (6, 10))     # (2,2), (6,10): even, exact 2x2 means
AREA_PLANES = (1, 7)
AREA_FACTOR = 6.0                                        # see area_downsample_ref
PYRAMID_CASES = ((2, 2, 2), (16, 16, 5), (32, 32, 6), (48, 80, 5), (96, 544, 6), (40, 24, 4), (64, 160, 3))
PYRAMID_UNSUPPORTED = ((48, 80, 6), (30, 40, 3))

FUSE_S = (1, 2, 3, 4, 5)
FUSE_B = (1, 3)
FUSE_D = (1, 3)
FUSE_GRIDS = ((1, 1), (7, 37), (16, 32))
FUSE_FACTOR = 4.0                                        # see fuse_ref64


def soft_argmin_bound(D, samples_n):
    """D terms of a few ulp each in numerator and denominator, with weights that sum to 1."""
    return 2.0 * (D + 8) * EPS * float(samples_n.abs().max())


# ---- seeded inputs -------------------------------------------------------------------------------------------------
def soft_argmin_inputs(n, D, rows, cols, scale, seed=0):
    g = torch.Generator().manual_seed(1000 * D + 10 * rows + n + seed)
    cost = torch.randn(n, D, rows, cols, generator=g) * scale
    # per-sample sample vectors: increasing inverse depths on a different range for every n
    samples = torch.sort(torch.rand(n, D, generator=g), dim=1).values * (1.0 + torch.arange(n).view(n, 1)) + 0.01
    return cost, samples


def bilinear_input(planes, size, seed=0):
    g = torch.Generator().manual_seed(100 * size[0] + size[1] + 7 * planes + seed)
    x = torch.randn(1, planes, size[0], size[1], generator=g) * 5
    return x


def bilinear_inputs():
    """(x, out size) for every resize case: N(0,1) * 5, plus an offset of 100 in one case."""
    for planes in BILINEAR_PLANES:
        for size, out in BILINEAR_SIZES:
            x = bilinear_input(planes, size)
            if (size, out) == BILINEAR_OFFSET_CASE:
                x = x + 100.0
            yield x, out


def prior_inputs():
    """(x (5,1,h,w), fx (5,), out size) for mvsn_upsample_prior: every sample with a focal length of its own."""
    fx = torch.tensor(PRIOR_FX)
    for size, out in BILINEAR_SIZES:
        x = bilinear_input(PRIOR_N, size, seed=3).transpose(0, 1).contiguous()
        if (size, out) == BILINEAR_OFFSET_CASE:
            x = x + 100.0
        yield x, fx, out


def mask_input(planes, size, seed=0):
    g = torch.Generator().manual_seed(100 * size[0] + size[1] + 7 * planes + 50 + seed)
    return torch.rand(1, planes, size[0], size[1], generator=g) > 0.5


def image_input(planes, rows, cols, seed=0):
    g = torch.Generator().manual_seed(100 * rows + cols + 7 * planes + seed)
    return torch.randn(1, planes, rows, cols, generator=g)


def fuse_inputs(S, B, D, rows, cols, seed=0):
    """raw, refined (S*B,1,rows,cols) positive inverse depths, baseline (S*B,) in (0.3, 2) distinct per chain, a random
    mask (S*B,D,rows,cols)."""
    g = torch.Generator().manual_seed(10000 * S + 1000 * B + 100 * D + rows + cols + seed)
    N = S * B
    raw = torch.rand(N, 1, rows, cols, generator=g) * 2 + 0.05
    refined = torch.rand(N, 1, rows, cols, generator=g) * 2 + 0.05
    baseline = 0.3 + 1.7 * (torch.randperm(N, generator=g).float() + torch.rand(N, generator=g) * 0.9) / N
    mask = torch.rand(N, D, rows, cols, generator=g) > 0.5
    return raw, refined, baseline, mask


def tie_mask(S, B, D, rows, cols, n_set, seed=0):
    """A mask with exactly n_set of the S sources set at every (b, d, pixel), which sources varying from pixel to pixel."""
    g = torch.Generator().manual_seed(77 + 10 * S + n_set + seed)
    order = torch.rand(S, B, D, rows, cols, generator=g).argsort(dim=0)
    return (order < n_set).reshape(S * B, D, rows, cols)


# ---- soft-argmin ---------------------------------------------------------------------------------------------------
def soft_argmin_ref(cost, samples):
    """float64 max-subtracted softmax of -cost over D, dotted with samples[n]: (N,D,rows,cols), (N,D) -> (N,1,rows,cols)."""
    c = -cost.double()
    m = c.max(dim=1, keepdim=True).values
    e = torch.exp(c - m)
    s = samples.double()[:, :, None, None]
    return (e * s).sum(1, keepdim=True) / e.sum(1, keepdim=True)


# ---- bilinear resize, align_corners=False ---------------------------------------------------------------------------
def resize_taps(in_size, out_size):
    """Taps and weights of one axis, every step rounded to float32 as ATen does (area_pixel_compute_source_index)."""
    f = np.float32
    scale = f(in_size) / f(out_size)
    dst = np.arange(out_size, dtype=np.float32)
    src = (dst + f(0.5)) * scale - f(0.5)
    src = np.maximum(src, f(0.0))
    assert src.dtype == np.float32
    i0 = src.astype(np.int64)
    i1 = np.minimum(i0 + 1, in_size - 1)
    l1 = src - i0.astype(np.float32)
    l0 = f(1.0) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    return i0, i1, l0, l1


def bilinear_ref(x, size):
    """F.interpolate(x, size, mode="bilinear", align_corners=False): float32 taps and weights, float64 four-tap blend."""
    v = x.detach().cpu().double().numpy()
    y0, y1, ly0, ly1 = resize_taps(v.shape[-2], int(size[0]))
    x0, x1, lx0, lx1 = resize_taps(v.shape[-1], int(size[1]))
    ly0, ly1 = ly0.astype(np.float64)[:, None], ly1.astype(np.float64)[:, None]
    lx0, lx1 = lx0.astype(np.float64)[None, :], lx1.astype(np.float64)[None, :]
    top = lx0 * v[..., y0[:, None], x0[None, :]] + lx1 * v[..., y0[:, None], x1[None, :]]
    bot = lx0 * v[..., y1[:, None], x0[None, :]] + lx1 * v[..., y1[:, None], x1[None, :]]
    return torch.from_numpy(ly0 * top + ly1 * bot)


def bilinear_mask_ref(m, size):
    """MaskUpsampler: float -> bilinear -> "> 0.5".  Returns (mask, the float64 blend): the blend tells which pixels
    sit so close to 0.5 that a float32 blend may decide the other way."""
    blend = bilinear_ref(m.double(), size)
    return blend > 0.5, blend


# ---- area downsample and the pyramid ----------------------------------------------------------------------------------
def area_downsample_ref(x):
    """One pyramid level in float64: output ceil(h/2) x ceil(w/2), window [floor(i*in/out), ceil((i+1)*in/out)).

    A float32 row-major sum of a window of k <= 9 values errs by at most sum_{j=2..k} j * EPS * max|x| (the j-th partial
    sum is at most j * max|x|), i.e. 44/9 * EPS * max|x| after the division, which adds one rounding of its own:
    below AREA_FACTOR = 6."""
    v = x.detach().cpu().double()
    h, w = v.shape[-2:]
    ho, wo = (h + 1) // 2, (w + 1) // 2
    out = torch.empty(v.shape[:-2] + (ho, wo), dtype=torch.float64)
    for i in range(ho):
        r0, r1 = (i * h) // ho, -((-(i + 1) * h) // ho)
        for j in range(wo):
            c0, c1 = (j * w) // wo, -((-(j + 1) * w) // wo)
            out[..., i, j] = v[..., r0:r1, c0:c1].sum((-2, -1)) / ((r1 - r0) * (c1 - c0))
    return out


def pyramid_ref(x, levels):
    """The float32 chain the reference runs (utils/image_utils.py:118-126): one interpolate(mode="area") per level on the
    previous level's rounded values, on the CPU."""
    pyr = [x.detach().cpu().float()]
    for _ in range(1, levels):
        prev = pyr[-1]
        pyr.append(F.interpolate(prev, ((prev.shape[2] + 1) // 2, (prev.shape[3] + 1) // 2), mode="area"))
    return pyr


# ---- multi-source fusion -----------------------------------------------------------------------------------------------
def chain_sb(s, b, S, B):
    return s * B + b            # the forward's chain order


def chain_bs(s, b, S, B):
    return b * S + s            # the other order: what a test must be able to tell from chain_sb


def fuse_ref32(raw, refined, baseline, mask, S, B, chain=chain_sb):
    """multi_view_stereonet.py:615-627 literally, in float32 on the CPU, looping over the sources; chain n = s*B + b.
    refined None: the level-4 refiner is off and the refined map IS the raw map (:613), which the two in-place
    divisions of :618-619 then divide by the baseline twice."""
    raw, baseline = raw.detach().cpu().float(), baseline.detach().cpu().float()
    rows, cols = raw.shape[-2:]
    raw_sum = torch.zeros(B, 1, rows, cols)
    ref_sum = torch.zeros(B, 1, rows, cols)
    mask_sum = torch.zeros((B,) + tuple(mask.shape[1:]))
    for s in range(S):
        idx = [chain(s, b, S, B) for b in range(B)]
        left_raw = raw[idx].clone()
        left = left_raw if refined is None else refined.detach().cpu().float()[idx].clone()
        baselinehw = baseline[idx].unsqueeze(1).unsqueeze(2).unsqueeze(3).repeat(1, 1, rows, cols)
        left_raw /= baselinehw
        left /= baselinehw
        raw_sum += left_raw
        ref_sum += left
        mask_sum += mask.detach().cpu()[idx].float()
    return raw_sum / S, ref_sum / S, (mask_sum / S) > 0.5


def fuse_ref64(raw, refined, baseline, S, B, chain=chain_sb):
    """The two means in float64.  The float32 chain is one division per source (two on the alias path), S - 1 additions
    of positive terms and the division by S.  Inverse depths are positive, so every partial sum is below the total and
    each rounding is at most EPS of the result: (S + 2) * EPS in the worst case, 7 * EPS at S = 5.
    FUSE_FACTOR = 4 is the figure the tests were specified with, not that worst case.  On the seeded inputs of
    fuse_inputs the float32 chain fuse_ref32 is at most 3.32 * EPS from these means (measured by
    tests/test_tail_reference_cpu.py, which asserts the cap); other inputs may take the chain itself past 4, so the
    seeds are part of the check.  The GPU test also asks for torch.equal with fuse_ref32, which is the tighter check."""
    r, base = raw.detach().cpu().double(), baseline.detach().cpu().double()
    f = None if refined is None else refined.detach().cpu().double()
    rows, cols = r.shape[-2:]
    raw_mean = torch.zeros(B, 1, rows, cols, dtype=torch.float64)
    ref_mean = torch.zeros(B, 1, rows, cols, dtype=torch.float64)
    for s in range(S):
        for b in range(B):
            n = chain(s, b, S, B)
            if f is None:
                raw_mean[b] += r[n] / base[n] / base[n]
                ref_mean[b] += r[n] / base[n] / base[n]
            else:
                raw_mean[b] += r[n] / base[n]
                ref_mean[b] += f[n] / base[n]
    return raw_mean / S, ref_mean / S
