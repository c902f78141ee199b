"""Plain restatement of the per-pixel confidence (mvsn_soft_argmin_confidence and
mvsn_confidence_fuse_sources of csrc/mvsn_misc.hip), written from the definition, not from the kernels, in float64.
No device code.

Definition, per chain n and pixel, c_d the filtered cost of hypothesis d = 0 .. D-1:
    p_d  = softmax(-c)_d                                  (the weights of the soft-argmin)
    idx  = sum_d p_d * d                                  (expected hypothesis INDEX, not idepth)
    i    = clamp(floor(idx), 0, D-1)
    conf = p_{i-1} + p_i + p_{i+1} + p_{i+2}              (terms outside [0, D-1] are 0)
A NaN cost makes the pixel's confidence NaN.  Per reference image the fused confidence is the minimum over the S sources
of the per-chain confidences (chain n = s*B + b); a NaN in any source gives NaN.

The bounds (EPS = 2^-24, as tail_reference.soft_argmin_bound is derived)
  A float32 evaluation forms e_d = exp(-c_d - m), m = max_d(-c_d), so the largest term is exactly 1 and den >= 1.
  * each e_d: the subtraction -c_d - m rounds its result x (|x| < 104, else e_d = 0) by at most EPS |x|, which moves
    e_d by EPS |x| e^{-|x|} <= EPS / e; a one-ulp expf adds 2 EPS e_d.  Absolute error of a term: at most 2.4 EPS.
  * den = sum of D such terms, summed in sequence: D * 2.4 EPS from the terms and (D - 1) EPS den from the additions.
  * the window W = sum of at most four terms: 4 * 2.4 EPS + 3 EPS W.
  * conf = W / den <= 1 and den >= 1:  |d conf| <= dW + conf * d den / den + EPS conf
                                                <= (9.6 + 3 + 2.4 D + (D - 1) + 1) EPS = (3.4 D + 12.6) EPS.
    A softmax that divides every term by den first (ATen's softmin) adds one EPS per window term.
  conf_bound(D) = 4 (D + 8) EPS covers both.
  * idx = sum_d p_d d: every weight d <= D - 1, so the same argument with the terms weighted by at most D - 1 gives
    idx_margin(D) = conf_bound(D) * (D - 1).
  tests/test_confidence_reference_cpu.py measures both on ATen's own float32 results on the seeded inputs below: the
  literal float32 formula stays within 0.062 of conf_bound and its index within 0.041 of idx_margin (the caps the test
  asserts: 0.1 and 0.1), so the bounds are loose by design, not tuned to any implementation.

The ambiguity rule (used by every comparison, compare() below): floor(idx) is discontinuous at the integers.  Where
|idx64 - rint(idx64)| <= idx_margin(D) a float32 evaluation may land on either side: the value may match either of
the two admissible windows, floor = rint - 1 or floor = rint.  Everywhere else it must match the single window of
floor(idx64).  No pixel is left out.
"""
import torch

import tail_reference as tr
from tail_reference import EPS, chain_bs, chain_sb, soft_argmin_inputs  # noqa: F401  (the seeded inputs are shared)

# ---- shapes --------------------------------------------------------------------------------------------------------
# D: 1, 2: the window covers everything; 3, 4, 5: cut at either end; 16: one vector round, no tail; 17, 33: a tail of
# one; 64: four rounds.  Shapes: 1, 259, 512 and 515 pixels (no full block, a second 256-pixel block).
CONF_D = (1, 2, 3, 4, 5, 16, 17, 33, 64)
CONF_SHAPES = ((1, 1, 1), (3, 7, 37), (2, 16, 32), (2, 5, 103))
CONF_SCALES = (1.0, 50.0, 1e4)
FUSE_S = (1, 2, 3, 5)
FUSE_B = (1, 3)
FUSE_GRIDS = ((1, 1), (7, 37))


def conf_bound(D):
    return 4.0 * (D + 8) * EPS


def idx_margin(D):
    return conf_bound(D) * (D - 1)


def conf_inputs(n, D, rows, cols, scale, seed=0):
    """The seeded cost volumes (and sample vectors) of tail_reference.soft_argmin_inputs."""
    return tr.soft_argmin_inputs(n, D, rows, cols, scale, seed)


# ---- the restatement -------------------------------------------------------------------------------------------------
def _weights(cost):
    c = -cost.double()
    m = c.max(dim=1, keepdim=True).values
    e = torch.exp(c - m)
    return e / e.sum(1, keepdim=True)


def confidence_for_floor(cost, i):
    """Window sum p_{i-1} + .. + p_{i+2} in float64 at the stated floor index i (N,rows,cols) integer, clamped to
    [0, D-1] first; terms outside [0, D-1] are 0.  -> (N,1,rows,cols)"""
    p = _weights(cost)
    D = p.shape[1]
    i = i.long().clamp(0, D - 1)
    out = torch.zeros(p.shape[0], 1, p.shape[2], p.shape[3], dtype=torch.float64)
    for k in (-1, 0, 1, 2):
        d = i + k
        inside = (d >= 0) & (d <= D - 1)
        term = p.gather(1, d.clamp(0, D - 1).unsqueeze(1))
        out = out + torch.where(inside.unsqueeze(1), term, torch.zeros_like(term))
    return out


def confidence_ref(cost, samples=None):
    """(conf64 (N,1,rows,cols), idx64 (N,rows,cols)) of cost (N,D,rows,cols).  `samples` takes no part: the index is
    taken in index space (the argument keeps the call shaped like soft_argmin_ref's)."""
    p = _weights(cost)
    D = p.shape[1]
    idx = (p * torch.arange(D, dtype=torch.float64).view(1, D, 1, 1)).sum(1)
    nan = idx.isnan()
    conf = confidence_for_floor(cost, torch.floor(torch.nan_to_num(idx, nan=0.0)))
    conf = torch.where(nan.unsqueeze(1), torch.full_like(conf, float("nan")), conf)
    return conf, idx


def compare(got, cost):
    """`got` (N,1,rows,cols) float32 against the restatement under the ambiguity rule.  Returns (the worst error as a
    fraction of conf_bound(D), the share of ambiguous pixels); asserts that NaNs sit in the same pixels.  Every pixel
    takes part."""
    D = cost.shape[1]
    conf64, idx64 = confidence_ref(cost)
    nan = conf64.isnan()
    assert torch.equal(got.isnan(), nan), "NaN pixels differ"
    safe = torch.nan_to_num(idx64, nan=0.0)
    r = torch.round(safe)                                  # rint
    ambiguous = ((safe - r).abs() <= idx_margin(D)) & ~nan.squeeze(1)
    g = got.double()
    err_single = (g - conf64).abs()
    err_either = torch.minimum((g - confidence_for_floor(cost, r - 1)).abs(), (g - confidence_for_floor(cost, r)).abs())
    err = torch.where(ambiguous.unsqueeze(1), err_either, err_single)
    err = torch.where(nan, torch.zeros_like(err), err)
    return float(err.max()) / conf_bound(D), float(ambiguous.double().mean())


# ---- minimum over the sources ----------------------------------------------------------------------------------------
def fuse_min_inputs(S, B, rows, cols, seed=0):
    g = torch.Generator().manual_seed(500 * S + 50 * B + rows + cols + seed)
    return torch.rand(S * B, 1, rows, cols, generator=g)


def fuse_min_ref(conf, S, B, chain=chain_sb):
    """(S*B,1,rows,cols) -> (B,1,rows,cols): the minimum over the sources, NaN where any source is NaN.  A minimum
    rounds nothing, so a float32 result must be these bits."""
    out = []
    for b in range(B):
        stack = torch.stack([conf[chain(s, b, S, B)] for s in range(S)], 0)
        low = torch.nan_to_num(stack, nan=float("inf")).amin(0)
        out.append(torch.where(stack.isnan().any(0), torch.full_like(low, float("nan")), low))
    return torch.stack(out, 0)
