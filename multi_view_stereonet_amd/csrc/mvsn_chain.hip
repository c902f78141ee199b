// The fused incremental chain (see include/mvsn_hip.h: mvsn_incremental_cost_volume).
//
// One 1024-thread workgroup (16 waves, 4 per SIMD) owns one (reference image, source view)
// chain for all D-1 sequential steps.  Per step: homography gather of the previous plane's
// features out of LDS, three 3x3 convolutions as implicit GEMMs on v_mfma_f32_16x16x4_f32
// (A = weights 16 couts x 4 cins, B = activations 4 cins x 16 pixels), two GroupNorm(4)
// reductions, and the cost-volume slice written straight to HBM.  Nothing but the cost / mask
// slices (and the optional feature volume) leaves the CU between steps.
//
// LDS plan (floats), P = rows*cols, RS = cols+1, G = RS+1, CS = rows*RS+G rounded to 16 mod 32:
//   wbuf   [10368]      weight fragments of the conv that runs next, [tap][cin/4][cout/16][lane]
//   sparams[224]        biases and GroupNorm affine
//   red    [4][16][4]   cross-wave reduction scratch (one slab per reduction of a step)
//   maskb  [P]          out-of-image flag of the current plane
//   act    G + 36*CS    activation planes.  Each channel is rows x RS with one zero column
//                       closing every row (it doubles as the left halo of the next row) and G
//                       zeros between channels (top/bottom halo), so every 3x3 tap of every
//                       pixel is a plain offset read with no bounds test.  CS = 16 (mod 32)
//                       makes the 16-pixel x 4-channel B-fragment read conflict-free.
//                       ch 0..2 image plane d, ch 3..34 features, ch 35 zero (K padding).
// When that exceeds 160 KiB the activation planes move to a per-chain global workspace
// (L2-resident); the code path is otherwise identical.
#include <type_traits>
#include <utility>

#include "mvsn_chain.h"
#include "mvsn_resident.h"
#include "mvsn_conv_wino.h"

namespace mvsn {

constexpr int CH_THREADS = 1024;
constexpr int CH_WAVES = 16;
constexpr int W0_FLOATS = CH_W0_FLOATS;
constexpr int W1_FLOATS = CH_W1_FLOATS;
constexpr int SP_FLOATS = CH_SP_FLOATS;
constexpr int PACKED_FLOATS = CH_PACKED_FLOATS;
constexpr int RED_FLOATS = 4 * CH_WAVES * 4;

// ---------------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------------
__global__ void pack_refiner_kernel(const float *c0w, const float *c0b, const float *g0w, const float *g0b,
                                    const float *c1w, const float *c1b, const float *g1w, const float *g1b,
                                    const float *c2w, const float *c2b, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= CH_STEPS_OFFSET) return;   // (the stepwise form's region is written by wino_pack_2d)
  if (i >= CH_DIRECT_FLOATS) {
    // Winograd form (mvsn_chain_wino.hip): U = G g G^T, [conv][k-step][cout tile][xi quad][lane][4 xi];
    // lane = k*16 + c holds U_xi[cout = t*16 + c][cin = 4*kstep + k] (the A fragment of the MFMA)
    int rel = i - CH_DIRECT_FLOATS, cin_total = 35;
    const float *w = c0w;
    if (rel >= CW_U0_FLOATS) {
      rel -= CW_U0_FLOATS, cin_total = 32, w = c1w;
      if (rel >= CW_U1_FLOATS) rel -= CW_U1_FLOATS, w = c2w;
    }
    const int j = rel & 3, lane = (rel >> 2) & 63, xq = (rel >> 8) & 3, t = (rel >> 10) & 1, c4 = rel >> 11;
    const int xi = xq * 4 + j, cout = t * 16 + (lane & 15), cin = c4 * 4 + (lane >> 4);
    float u = 0.0f;
    if (cin < cin_total) {
      const float *g = w + ((size_t)cout * cin_total + cin) * 9;
      const float G[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
      const int gi = xi >> 2, gj = xi & 3;
      for (int aa = 0; aa < 3; ++aa)
        for (int bb = 0; bb < 3; ++bb) u += G[gi][aa] * g[aa * 3 + bb] * G[gj][bb];
    }
    out[i] = u;
  } else if (i < W0_FLOATS + 2 * W1_FLOATS) {
    int conv, rel, cin_total, nc;
    const float *w;
    if (i < W0_FLOATS) {
      conv = 0, rel = i, cin_total = 35, nc = 9, w = c0w;
    } else if (i < W0_FLOATS + W1_FLOATS) {
      conv = 1, rel = i - W0_FLOATS, cin_total = 32, nc = 8, w = c1w;
    } else {
      conv = 2, rel = i - W0_FLOATS - W1_FLOATS, cin_total = 32, nc = 8, w = c2w;
    }
    (void)conv;
    const int lane = rel & 63;
    const int t = (rel >> 6) & 1;
    const int c4 = (rel >> 7) % nc;
    const int tap = (rel >> 7) / nc;
    const int cout = t * 16 + (lane & 15);
    const int cin = c4 * 4 + (lane >> 4);
    out[i] = cin < cin_total ? w[((size_t)cout * cin_total + cin) * 9 + tap] : 0.0f;
  } else {
    const int r = i - (W0_FLOATS + 2 * W1_FLOATS);
    const int which = r / 32, c = r % 32;
    const float *srcs[7] = {c0b, g0w, g0b, c1b, g1w, g1b, c2b};
    out[i] = srcs[which][c];
  }
}

// ---------------------------------------------------------------------------------------------
// pieces of the step
// ---------------------------------------------------------------------------------------------
template <int TP, int NC>
__device__ __forceinline__ void conv3x3_mfma(const float *__restrict__ act, const float *__restrict__ wbuf, int CS,
                                             int RS, const int (&qb)[TP], int lane, floatx4 (&acc)[TP][2]) {
#pragma unroll
  for (int j = 0; j < TP; ++j) {
    acc[j][0] = floatx4{0.f, 0.f, 0.f, 0.f};
    acc[j][1] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  const float *abase = act + (lane >> 4) * CS;
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {
    const int off = (tap / 3 - 1) * RS + (tap % 3 - 1);
    const float *wt = wbuf + tap * NC * 128 + lane;
    const float *ab = abase + off;
#pragma unroll
    for (int c4 = 0; c4 < NC; ++c4) {
      const float w0 = wt[c4 * 128];
      const float w1 = wt[c4 * 128 + 64];
#pragma unroll
      for (int j = 0; j < TP; ++j) {
        const float b = ab[c4 * 4 * CS + qb[j]];
        acc[j][0] = mfma16x16x4(w0, b, acc[j][0]);
        acc[j][1] = mfma16x16x4(w1, b, acc[j][1]);
      }
    }
  }
}

// Same convolution when the activation planes live in the global workspace (coarse grids that do not
// fit LDS): each 4-channel slab (with its halo guards) is staged into one of two LDS buffers while the
// previous slab's 9 taps run, so the MFMA loop still reads its B fragments from LDS.  One barrier per
// slab.  `slab` holds 2 x slab_floats, slab_floats = G + 4*CS.
template <int TP, int NC>
__device__ __forceinline__ void conv3x3_mfma_slab(const float *__restrict__ act, const float *__restrict__ wbuf,
                                                  float *__restrict__ slab, int CS, int RS, const int (&qb)[TP],
                                                  int tid, floatx4 (&acc)[TP][2]) {
  const int lane = tid & 63;
  const int G = RS + 1;
  const int slab_floats = G + 4 * CS;
  constexpr int PER = 9;  // staged floats per thread per slab (<= 9216 floats per slab)
#pragma unroll
  for (int j = 0; j < TP; ++j) {
    acc[j][0] = floatx4{0.f, 0.f, 0.f, 0.f};
    acc[j][1] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  float stage[PER];
  auto fetch = [&](int c4) {
    const float *src = act + c4 * 4 * CS - G;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * CH_THREADS;
      stage[k] = i < slab_floats ? src[i] : 0.0f;
    }
  };
  auto commit = [&](int buf) {
    float *dst = slab + buf * slab_floats;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * CH_THREADS;
      if (i < slab_floats) dst[i] = stage[k];
    }
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int c4 = 0; c4 < NC; ++c4) {
    if (c4 + 1 < NC) fetch(c4 + 1);
    const float *sb = slab + (c4 & 1) * slab_floats + G + (lane >> 4) * CS;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int off = (tap / 3 - 1) * RS + (tap % 3 - 1);
      const float *wt = wbuf + (tap * NC + c4) * 128 + lane;
      const float w0 = wt[0];
      const float w1 = wt[64];
#pragma unroll
      for (int j = 0; j < TP; ++j) {
        const float b = sb[qb[j] + off];
        acc[j][0] = mfma16x16x4(w0, b, acc[j][0]);
        acc[j][1] = mfma16x16x4(w1, b, acc[j][1]);
      }
    }
    if (c4 + 1 < NC) commit((c4 + 1) & 1);
    __syncthreads();
  }
}

// Sum `v[t]` (t = 0,1: the two cout tiles) over the whole workgroup, per GroupNorm group.
// Lanes 0..31 of a wave hold channels of group 2t, lanes 32..63 of group 2t+1.
__device__ __forceinline__ void block_group_sum(float (&v)[2], float *red_slab, int lane, int wave) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float s = v[t];
    s += dpp_mov<0xB1>(s);    // quad_perm [1, 0, 3, 2]
    s += dpp_mov<0x4E>(s);    // quad_perm [2, 3, 0, 1]
    s += dpp_mov<0x141>(s);   // row_half_mirror: the other quad of the half row
    s += dpp_mov<0x140>(s);   // row_mirror: the other half of the 16-lane row
    s += __shfl_xor(s, 16, 64);
    v[t] = s;
  }
  if ((lane & 31) == 0) {
    const int hi = lane >> 5;
    red_slab[wave * 4 + 0 + hi] = v[0];
    red_slab[wave * 4 + 2 + hi] = v[1];
  }
  __syncthreads();
  const int hi = lane >> 5;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int w = 0; w < CH_WAVES; ++w) {
    s0 += red_slab[w * 4 + 0 + hi];
    s1 += red_slab[w * 4 + 2 + hi];
  }
  v[0] = s0;
  v[1] = s1;
}

// acc(+bias) -> LeakyReLU(GroupNorm(.)) in place.
template <int TP>
__device__ __forceinline__ void groupnorm_lrelu(floatx4 (&acc)[TP][2], const bool (&valid)[TP],
                                                const float *__restrict__ bias, const float *__restrict__ gamma,
                                                const float *__restrict__ beta, float *red_a, float *red_b,
                                                float inv_count, int lane, int wave) {
  const int cbase = (lane >> 4) * 4;
  float s[2] = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < TP; ++j)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[j][t][r] += bias[t * 16 + cbase + r];
        if (valid[j]) s[t] += acc[j][t][r];
      }
  block_group_sum(s, red_a, lane, wave);
  const float mean[2] = {s[0] * inv_count, s[1] * inv_count};
  float q[2] = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < TP; ++j)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dv = acc[j][t][r] - mean[t];
        if (valid[j]) q[t] += dv * dv;
      }
  block_group_sum(q, red_b, lane, wave);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float rstd = 1.0f / sqrtf(q[t] * inv_count + MVSN_GN_EPS);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = t * 16 + cbase + r;
      const float sc = rstd * gamma[c];
      const float sh = beta[c] - mean[t] * sc;
#pragma unroll
      for (int j = 0; j < TP; ++j) acc[j][t][r] = lrelu02(acc[j][t][r] * sc + sh);
    }
  }
}

template <int WFLOATS>
__device__ __forceinline__ void load_weights_to_regs(const float *__restrict__ g, floatx4 (&wreg)[3], int tid) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int idx = (tid + k * CH_THREADS) * 4;
    if (idx < WFLOATS) wreg[k] = *reinterpret_cast<const floatx4 *>(g + idx);
  }
}
template <int WFLOATS>
__device__ __forceinline__ void store_weights_to_lds(float *wbuf, const floatx4 (&wreg)[3], int tid) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int idx = (tid + k * CH_THREADS) * 4;
    if (idx < WFLOATS) *reinterpret_cast<floatx4 *>(wbuf + idx) = wreg[k];
  }
}

template <int TP, bool LDS_ACT, bool C16 = false>   // C16: cost volume stored as bf16 (ChainArgs::cost_bf16, bf16 feature tier)
__global__ __launch_bounds__(CH_THREADS) void chain_kernel(ChainArgs a, MVSN_VIS10) {   // (MVSN_VIS10: mvsn_common.h)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (chain_gate_closed(a)) return;   // repair launch with nothing to repair (mvsn_chain.h)
  int tid = threadIdx.x;              // (made opaque at the top of every step, see the step loop)
  const int lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x;
  const int rows = a.rows, cols = a.cols, P = rows * cols, RS = cols + 1, G = RS + 1, CS = a.CS, D = a.D;
  constexpr int IMG_IT = (TP * 256 + CH_THREADS - 1) / CH_THREADS;

  float *wbuf = smem;
  float *sparams = wbuf + W0_FLOATS;
  float *red = sparams + SP_FLOATS;
  float *maskb = red + RED_FLOATS;
  const int Ppad = (P + 3) & ~3;
  float *act;
  float *slab = nullptr;
  const int act_floats = G + 36 * CS;
  // moved features of the step (the epilogue adds the refiner's output to them): 32 x P floats per chain in the global
  // workspace, written and read back by the same thread -- held in registers across the three convolutions they cost
  // 8 VGPRs per tile, which a 1024-thread workgroup (128 registers per lane) does not have
  float *mv;
  if constexpr (LDS_ACT) {
    act = maskb + Ppad + G;
    mv = a.workspace + (size_t)n * 32 * P;
  } else {
    act = a.workspace + (size_t)n * (act_floats + 32 * P) + G;
    mv = a.workspace + (size_t)n * (act_floats + 32 * P) + act_floats;
    slab = maskb + Ppad;   // 2 x (G + 4*CS) floats
  }

  // ---- one-time set-up ---------------------------------------------------------------------
  for (int i = tid; i < act_floats; i += CH_THREADS) act[i - G] = 0.0f;
  for (int i = tid; i < SP_FLOATS; i += CH_THREADS) sparams[i] = a.packed[W0_FLOATS + 2 * W1_FLOATS + i];
  const float *bias0 = sparams, *gn0w = sparams + 32, *gn0b = sparams + 64, *bias1 = sparams + 96,
              *gn1w = sparams + 128, *gn1b = sparams + 160, *bias2 = sparams + 192;

  int pb[TP], qb[TP];
  bool valid[TP];
  int cbase;   // this lane's channels: t*16 + cbase + r
  auto tile_indices = [&](int t_) {   // this thread's pixels of its wave's TP tiles (recomputed per step, see the loop)
    const int lane_ = t_ & 63, wave_ = t_ >> 6;
#pragma unroll
    for (int j = 0; j < TP; ++j) {
      const int p = (wave_ * TP + j) * 16 + (lane_ & 15);
      valid[j] = p < P;
      pb[j] = valid[j] ? p : 0;
      qb[j] = (pb[j] / cols) * RS + (pb[j] % cols);
    }
    cbase = (lane_ >> 4) * 4;
  };
  tile_indices(tid);
  __syncthreads();

  const float *f0 = a.f0 + (size_t)n * 32 * P;
  const float *flp = a.fl + (size_t)(n % a.B) * 32 * P;
#pragma unroll
  for (int j = 0; j < TP; ++j)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = t * 16 + cbase + r;
        if (valid[j]) act[(3 + c) * CS + qb[j]] = f0[(size_t)c * P + pb[j]];
      }

  const float *Hn = a.H + (size_t)n * D * 9;
  const float *Hin = a.Hinc + (size_t)n * D * 9;
  const float *src = a.src + (size_t)n * 3 * P;
  uint8_t *maskg = a.mask + (size_t)n * D * P;
  typedef typename ChainCost<C16>::type cost_t;
  cost_t *costg = reinterpret_cast<cost_t *>(a.cost) + (size_t)n * 32 * D * P;
  float *fvolg = a.fvol ? a.fvol + (size_t)n * 32 * D * P : nullptr;

  // ---- plane 0: mask and cost from the extractor's features ---------------------------------
  {
    float Hl[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Hl[i] = Hn[i];
    for (int p = tid; p < P; p += CH_THREADS) {
      WarpCoord c = warp_coord(Hl, (float)(p % cols), (float)(p / cols), (float)rows, (float)cols);
      maskb[p] = c.outside ? 1.0f : 0.0f;
      maskg[p] = c.outside ? 1 : 0;
    }
  }
  __syncthreads();

  // Cost-volume slice of plane `dd` from the LDS-resident features: coalesced 16-byte HBM traffic
  // (left features in, cost out), rows of the padded plane read back as 4 scalars.  Runs while the
  // plane's features and mask are still in place, i.e. before barrier B1 of the following step.
  auto write_cost_slice = [&](int dd) {
    if ((cols & 3) == 0) {
      const int quads = P >> 2;
      for (int i = tid; i < 32 * quads; i += CH_THREADS) {
        const int c = i / quads, p4 = (i - c * quads) * 4;
        const int y = p4 / cols, x = p4 - y * cols;
        const float *fr = act + (3 + c) * CS + y * RS + x;
        const floatx4 l = *reinterpret_cast<const floatx4 *>(flp + (size_t)c * P + p4);
        const floatx4 m = *reinterpret_cast<const floatx4 *>(maskb + p4);
        floatx4 cst, ftr;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float f = fr[k];
          cst[k] = m[k] != 0.0f ? 0.0f : fabsf(l[k] - f);
          ftr[k] = m[k] != 0.0f ? 0.0f : f;
        }
        chain_cost_st(costg + ((size_t)c * D + dd) * P + p4, cst);
        if (fvolg) *reinterpret_cast<floatx4 *>(fvolg + ((size_t)c * D + dd) * P + p4) = ftr;
      }
    } else {
      for (int i = tid; i < 32 * P; i += CH_THREADS) {
        const int c = i / P, p = i - c * P;
        const float f = act[(3 + c) * CS + (p / cols) * RS + (p % cols)];
        const bool out = maskb[p] != 0.0f;
        chain_cost_st(costg + ((size_t)c * D + dd) * P + p, out ? 0.0f : fabsf(flp[(size_t)c * P + p] - f));
        if (fvolg) fvolg[((size_t)c * D + dd) * P + p] = out ? 0.0f : f;
      }
    }
  };
  const float inv_count = 1.0f / (8.0f * (float)P);

  // ---- the recurrence ------------------------------------------------------------------------
#define MVSN_STAMP(i)                                                                   \
  do {                                                                                  \
    if (a.dbg && blockIdx.x == 0 && tid == 0 && d <= 4) a.dbg[(d - 1) * 16 + (i)] = __builtin_readcyclecounter(); \
  } while (0)
  for (int d = 1; d < D; ++d) {
    // Per-thread addresses are recomputed every step from an opaque copy of the thread id: hoisted out of the loop
    // (72 of them in the smallest instantiation) they do not fit the 128 registers of a 1024-thread workgroup and go
    // to scratch -- and every reload in front of a load is an s_waitcnt vmcnt(0) (HISTORY 11.9, same disease).
    asm volatile("" : "+v"(tid));
    tile_indices(tid);
    const int lane = tid & 63, wave = tid >> 6;
    MVSN_STAMP(0);
    floatx4 wreg[3];
    load_weights_to_regs<W0_FLOATS>(a.packed, wreg, tid);
    write_cost_slice(d - 1);

    // A1: image plane d and its mask (global gathers; the 6 KB source image stays in L1/L2)
    float img[IMG_IT][3];
    float mk[IMG_IT];
    {
      float Hl[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) Hl[i] = Hn[d * 9 + i];
#pragma unroll
      for (int it = 0; it < IMG_IT; ++it) {
        const int p = tid + it * CH_THREADS;
        if (p < P) {
          WarpCoord c = warp_coord(Hl, (float)(p % cols), (float)(p / cols), (float)rows, (float)cols);
          Bilinear b = bilinear_taps(c.ix, c.iy, rows, cols);
          const float keep = c.outside ? 0.0f : 1.0f;
          mk[it] = c.outside ? 1.0f : 0.0f;
          const int o00 = b.y0 * cols + b.x0, o01 = b.y0 * cols + b.x1, o10 = b.y1 * cols + b.x0,
                    o11 = b.y1 * cols + b.x1;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const float *ic = src + (size_t)ch * P;
            img[it][ch] = keep * (ic[o00] * b.w00 + ic[o01] * b.w01 + ic[o10] * b.w10 + ic[o11] * b.w11);
          }
        }
      }
    }

    // A2: previous plane's features moved by the incremental homography (gather from the activation planes) -> mv
    {
      float Hl[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) Hl[i] = Hin[d * 9 + i];
#pragma unroll
      for (int j = 0; j < TP; ++j) {
        WarpCoord c = warp_coord(Hl, (float)(pb[j] % cols), (float)(pb[j] / cols), (float)rows, (float)cols);
        Bilinear b = bilinear_taps(c.ix, c.iy, rows, cols);
        const float keep = c.outside ? 0.0f : 1.0f;
        const int o00 = b.y0 * RS + b.x0, o01 = b.y0 * RS + b.x1, o10 = b.y1 * RS + b.x0, o11 = b.y1 * RS + b.x1;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float *fc = act + (3 + t * 16 + cbase + r) * CS;
            const float v = keep * (fc[o00] * b.w00 + fc[o01] * b.w01 + fc[o10] * b.w10 + fc[o11] * b.w11);
            if (valid[j]) mv[(size_t)(t * 16 + cbase + r) * P + pb[j]] = v;
          }
        __builtin_amdgcn_sched_barrier(0);   // one tile's 32 taps in flight at a time
      }
    }
    MVSN_STAMP(1);
    __syncthreads();  // B1: every gather of plane d-1 is done
    MVSN_STAMP(2);

    // A3: lay out the refiner input [image(3) | moved features(32)]
#pragma unroll
    for (int j = 0; j < TP; ++j)
      if (valid[j]) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            act[(3 + t * 16 + cbase + r) * CS + qb[j]] = mv[(size_t)(t * 16 + cbase + r) * P + pb[j]];
      }
#pragma unroll
    for (int it = 0; it < IMG_IT; ++it) {
      const int p = tid + it * CH_THREADS;
      if (p < P) {
        const int q = (p / cols) * RS + (p % cols);
        act[0 * CS + q] = img[it][0];
        act[1 * CS + q] = img[it][1];
        act[2 * CS + q] = img[it][2];
        maskb[p] = mk[it];
        maskg[(size_t)d * P + p] = mk[it] != 0.0f ? 1 : 0;
      }
    }
    store_weights_to_lds<W0_FLOATS>(wbuf, wreg, tid);
    __syncthreads();  // B2
    MVSN_STAMP(3);

    floatx4 acc[TP][2];
    load_weights_to_regs<W1_FLOATS>(a.packed + W0_FLOATS, wreg, tid);  // in flight behind the MFMAs
    if constexpr (LDS_ACT) conv3x3_mfma<TP, 9>(act, wbuf, CS, RS, qb, lane, acc);
    else conv3x3_mfma_slab<TP, 9>(act, wbuf, slab, CS, RS, qb, tid, acc);
    MVSN_STAMP(4);
    __syncthreads();  // B3: act and wbuf free
    MVSN_STAMP(5);

    groupnorm_lrelu<TP>(acc, valid, bias0, gn0w, gn0b, red, red + 64, inv_count, lane, wave);
#pragma unroll
    for (int j = 0; j < TP; ++j)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (valid[j]) {
#pragma unroll
          for (int r = 0; r < 4; ++r) act[(t * 16 + cbase + r) * CS + qb[j]] = acc[j][t][r];
        }
      }
    store_weights_to_lds<W1_FLOATS>(wbuf, wreg, tid);
    __syncthreads();  // B6
    MVSN_STAMP(6);

    load_weights_to_regs<W1_FLOATS>(a.packed + W0_FLOATS + W1_FLOATS, wreg, tid);
    if constexpr (LDS_ACT) conv3x3_mfma<TP, 8>(act, wbuf, CS, RS, qb, lane, acc);
    else conv3x3_mfma_slab<TP, 8>(act, wbuf, slab, CS, RS, qb, tid, acc);
    MVSN_STAMP(7);
    __syncthreads();  // B7
    MVSN_STAMP(8);

    groupnorm_lrelu<TP>(acc, valid, bias1, gn1w, gn1b, red + 128, red + 192, inv_count, lane, wave);
#pragma unroll
    for (int j = 0; j < TP; ++j)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (valid[j]) {
#pragma unroll
          for (int r = 0; r < 4; ++r) act[(t * 16 + cbase + r) * CS + qb[j]] += acc[j][t][r];  // x2 = x1 + ...
        }
      }
    store_weights_to_lds<W1_FLOATS>(wbuf, wreg, tid);
    __syncthreads();  // B10
    MVSN_STAMP(9);

    if constexpr (LDS_ACT) conv3x3_mfma<TP, 8>(act, wbuf, CS, RS, qb, lane, acc);
    else conv3x3_mfma_slab<TP, 8>(act, wbuf, slab, CS, RS, qb, tid, acc);
    MVSN_STAMP(10);
    __syncthreads();  // B11
    MVSN_STAMP(11);

    // epilogue: the new features become the next step's gather source; their cost slice is
    // written (coalesced) at the top of the next step / after the loop
#pragma unroll
    for (int j = 0; j < TP; ++j) {
      if (!valid[j]) continue;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = t * 16 + cbase + r;
          act[(3 + c) * CS + qb[j]] = mv[(size_t)c * P + pb[j]] + (acc[j][t][r] + bias2[c]);
        }
    }
    MVSN_STAMP(12);
    __syncthreads();  // B12
    MVSN_STAMP(13);
  }
#undef MVSN_STAMP
  write_cost_slice(D - 1);
}

static size_t chain_lds_bytes(int P, int act_floats, bool lds_act, int slab_floats = 0) {
  const int Ppad = (P + 3) & ~3;
  size_t f = (size_t)W0_FLOATS + SP_FLOATS + RED_FLOATS + Ppad;
  if (lds_act) f += act_floats;
  else f += 2 * (size_t)slab_floats;
  return f * sizeof(float);
}

static int chain_cs(int rows, int cols) {
  const int RS = cols + 1, G = RS + 1;
  int cs = rows * RS + G;
  while ((cs & 31) != 16) ++cs;
  return cs;
}

// ---- host side: the direct form's plan ----------------------------------------------------------------------------
struct DirectPlan {
  int TP;             // 16-pixel tiles per wave
  bool lds_act, ok;   // activation planes in LDS (else in the global workspace, staged by slabs); the form runs this grid
  size_t lds_bytes;
};

static DirectPlan chain_direct_plan(int rows, int cols) {
  const int P = rows * cols, CS = chain_cs(rows, cols);
  const int act_floats = (cols + 2) + 36 * CS, slab_floats = (cols + 2) + 4 * CS;
  DirectPlan p;
  p.TP = ((P + 15) / 16 + CH_WAVES - 1) / CH_WAVES;
  p.lds_act = chain_lds_bytes(P, act_floats, true) <= 160 * 1024;
  p.lds_bytes = chain_lds_bytes(P, act_floats, p.lds_act, slab_floats);
  p.ok = p.TP <= 8 && (p.lds_act ? p.TP <= 3 : slab_floats <= 9 * CH_THREADS);
  return p;
}

// per chain: the step's moved features (32 x P, always) + the activation planes where they do not fit LDS
static size_t chain_direct_bytes(int n_chains, int rows, int cols) {
  const size_t act_floats = (cols + 2) + 36 * (size_t)chain_cs(rows, cols), mv_floats = (size_t)32 * rows * cols;
  return (size_t)n_chains * (mv_floats + (chain_direct_plan(rows, cols).lds_act ? 0 : act_floats)) * sizeof(float);
}

// ---- the resolver: what a call runs ---------------------------------------------------------------------------------
struct ChainPlan {
  bool ok;                  // the form has a plan for this grid (the entry points refuse the call otherwise)
  bool redirected;          // `redirect` replaced the requested form (see chain_resolve)
  int form;                 // the form that runs (never AUTO once the sizes are valid)
  int repair_form;          // the gated single-launch form behind a guarded banded call; 0: no repair launch
  int groups;               // banded: workgroups per chain of the plan that runs
  size_t workspace_bytes, repair_workspace_bytes;
  size_t status_offset;     // banded: byte offset of the status word inside the workspace
};

// THE place that decides which form a call runs and what it needs -- the entry points, the planning exports and the
// module all ask here.  `guarded`: a gated repair launch follows a banded call (mvsn_incremental_cost_volume_guarded /
// _bf16); `coresident_allowed`: AUTO may pick a form whose workgroups must be co-resident (false: lanes on several
// streams, a latched module, another process owning the device's co-resident launches); `redirect`: the module's
// rule for an explicit Winograd / stepwise request on a grid without that plan -- the direct form runs (the C entry
// points pass false and refuse such a call).
// MVSN_CHAIN_AUTO:
//   16x32 (plane-resident plan): banded -- several workgroups per chain -- only while all chains fit the chip in ONE
//     pass (beyond 64 chains the plane-resident kernel is faster), then Winograd;
//   30x40 / 32x64 (no plane-resident plan), guarded: banded for any number of chains -- thin bands while they fit one
//     pass, the slab plan beyond; the stepwise form, which sends the plane through HBM every step, is no longer AUTO's
//     choice there;
//   ... unguarded (the PLAIN entry point): the multi-pass slab launches need the device to themselves for milliseconds
//     at a stretch and a time-out without repair would leave a NaN-poisoned cost slice, so beyond ONE thin-band pass
//     AUTO stays on the co-residency-free forms (the round-4 policy; a caller that wants the slab plan asks for
//     MVSN_CHAIN_BANDED or uses the guarded entry);
//   otherwise Winograd, then stepwise -- one plane per round of full-chip launches, whatever the number of chains
//     (re-measured in round 3 with tools/chain_bench.py: 30x40, 256 / 512 chains 25.4 / 48.0 ms against the direct
//     form's 41.5 / 86.8) --, then direct (one workgroup per chain, planes in a global workspace: cols % 4 != 0).
static ChainPlan chain_resolve(int n_chains, int D, int rows, int cols, int requested, bool guarded, bool coresident_allowed,
                               bool redirect = false) {
  ChainPlan p = {};
  p.form = requested;
  if (n_chains <= 0 || rows <= 0 || cols <= 0 || requested < MVSN_CHAIN_AUTO || requested > MVSN_CHAIN_BANDED) return p;
  const bool wino = chain_wino_supported(rows, cols), steps = chain_steps_supported(rows, cols);
  if (requested == MVSN_CHAIN_AUTO) {
    const int cap = chain_band_chains_per_pass(rows, cols);
    const bool banded = coresident_allowed && cap > 0 && (n_chains <= cap || (guarded && !wino));
    p.form = banded ? MVSN_CHAIN_BANDED : wino ? MVSN_CHAIN_WINOGRAD : steps ? MVSN_CHAIN_STEPWISE : MVSN_CHAIN_DIRECT;
  } else if (redirect && ((requested == MVSN_CHAIN_WINOGRAD && !wino) || (requested == MVSN_CHAIN_STEPWISE && !steps))) {
    p.form = MVSN_CHAIN_DIRECT, p.redirected = true;
  }
  switch (p.form) {
    case MVSN_CHAIN_WINOGRAD: p.ok = wino; break;
    case MVSN_CHAIN_STEPWISE: p.ok = steps, p.workspace_bytes = chain_steps_workspace_bytes(n_chains, D, rows, cols); break;
    case MVSN_CHAIN_BANDED:
      p.ok = chain_band_layout(n_chains, rows, cols, &p.groups, &p.status_offset);
      if (p.ok) p.workspace_bytes = p.status_offset + 64;
      if (guarded) {   // repaired by the plane-resident Winograd kernel where the grid has that plan (16x32), the direct kernel elsewhere
        p.repair_form = wino ? MVSN_CHAIN_WINOGRAD : MVSN_CHAIN_DIRECT;
        p.repair_workspace_bytes = wino ? 0 : chain_direct_bytes(n_chains, rows, cols);
      }
      break;
    default: p.ok = chain_direct_plan(rows, cols).ok, p.workspace_bytes = chain_direct_bytes(n_chains, rows, cols); break;
  }
  return p;
}

#ifdef MVSN_CHAIN_STAMPS
static unsigned long long *g_chain_stamps = nullptr;
#endif

// f(integral_constant<TP>) for the TP == tp of the list: the fold that turns the run-time tile count into a compile-time one
template <class F, int... TPS>
static int chain_with_tp(int tp, std::integer_sequence<int, TPS...>, F &&f) {
  int rc = MVSN_E_TOOLARGE;
  (void)((tp == TPS && ((rc = f(std::integral_constant<int, TPS>{})), true)) || ...);
  return rc;
}

static int chain_direct_launch(const char *entry, ChainArgs a, int n_chains, void *workspace, size_t workspace_bytes,
                               hipStream_t stream) {
  const DirectPlan plan = chain_direct_plan(a.rows, a.cols);
  MVSN_REQUIRE(plan.TP <= 8, MVSN_E_TOOLARGE, "%s: %dx%d coarse grid (%d px) exceeds the 2048 px plan", entry, a.rows, a.cols,
               a.rows * a.cols);
  const size_t need = chain_direct_bytes(n_chains, a.rows, a.cols);
  MVSN_REQUIRE(workspace && workspace_bytes >= need, MVSN_E_WORKSPACE, "%s: workspace of %zu bytes required", entry, need);
  MVSN_REQUIRE(plan.ok, MVSN_E_TOOLARGE, "%s: coarse grid too large for the slab staging plan", entry);
  a.workspace = (float *)workspace;
  // the kernel of (TP, LDS_ACT, C16): instantiated here, once per combination, with its own LdsOptIn
  auto launch = [&](auto tp, auto lds_act, auto c16) -> int {
    const auto kernel = chain_kernel<decltype(tp)::value, decltype(lds_act)::value, decltype(c16)::value>;
    static LdsOptIn opt;
    if (int rc = ensure_lds(opt, (const void *)kernel, plan.lds_bytes, entry)) return rc;
    hipLaunchKernelGGL(kernel, dim3(n_chains), dim3(CH_THREADS), plan.lds_bytes, stream, a, CHAIN_VISIBLE_G(a));
    return 0;
  };
  auto tiled = [&](auto tp, auto lds_act) -> int {   // (bf16 feature tier: its own instantiations)
    return a.cost_bf16 ? launch(tp, lds_act, std::true_type{}) : launch(tp, lds_act, std::false_type{});
  };
  if (int rc = plan.lds_act
                   ? chain_with_tp(plan.TP, std::integer_sequence<int, 1, 2, 3>{}, [&](auto tp) { return tiled(tp, std::true_type{}); })
                   : chain_with_tp(plan.TP, std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8>{},
                                   [&](auto tp) { return tiled(tp, std::false_type{}); }))
    return rc;
  return check_launch(entry);
}

// One resolved form of the chain; a.gate != null: as a gated repair launch (one of the single-launch forms).
static int chain_launch(const char *entry, const ChainArgs &a, int n_chains, void *workspace, size_t workspace_bytes,
                        const ChainPlan &p, hipStream_t stream) {
  switch (p.form) {
    case MVSN_CHAIN_WINOGRAD:
      MVSN_REQUIRE(p.ok, MVSN_E_TOOLARGE, "%s: no Winograd plan for a %dx%d coarse grid", entry, a.rows, a.cols);
      return chain_wino_launch(a, n_chains, stream);
    case MVSN_CHAIN_STEPWISE:
      MVSN_REQUIRE(!a.cost_bf16, MVSN_E_BADARG, "%s: the stepwise form has no bf16 cost-volume variant", entry);
      return chain_steps_launch(a, n_chains, workspace, workspace_bytes, stream);
    case MVSN_CHAIN_BANDED:
      MVSN_REQUIRE(p.ok, MVSN_E_TOOLARGE, "%s: the banded form has no plan for a %dx%d coarse grid (16x32, 30x40, 32x64)",
                   entry, a.rows, a.cols);
      return chain_band_launch(a, n_chains, workspace, workspace_bytes, 0, stream);
    default: return chain_direct_launch(entry, a, n_chains, workspace, workspace_bytes, stream);
  }
}

// The C arguments of an entry point as the kernels take them.
static ChainArgs chain_args(const float *src_image_lvl4, const float *H_lvl4, const float *H_inc, const float *plane0_features,
                            const float *left_features, const float *refiner_packed, int batch, int num_idepth_samples,
                            int rows, int cols, void *cost_volume, bool cost_bf16, uint8_t *mask_volume,
                            float *feature_volume) {
  ChainArgs a = {};
  a.src = src_image_lvl4, a.H = H_lvl4, a.Hinc = H_inc, a.f0 = plane0_features, a.fl = left_features;
  a.packed = refiner_packed, a.cost = (float *)cost_volume, a.mask = mask_volume, a.fvol = feature_volume;
  a.B = batch, a.D = num_idepth_samples, a.rows = rows, a.cols = cols, a.CS = chain_cs(rows, cols);
  a.cost_bf16 = cost_bf16 ? 1 : 0;
#ifdef MVSN_CHAIN_STAMPS   // tuning builds only (tools/chain_phases.py): device pointer to 64 x u64 cycle stamps
  a.dbg = g_chain_stamps;
#endif
  return a;
}

// The body of the three entry points: the resolved form and, behind a guarded banded call, its gated repair launch.
static int chain_entry(const char *entry, ChainArgs a, int n_chains, void *workspace, size_t workspace_bytes, int form,
                       bool guarded, void *repair_workspace, size_t repair_workspace_bytes, unsigned *sticky_status,
                       mvsn_stream_t stream) {
  MVSN_REQUIRE(a.src && a.H && a.Hinc && a.f0 && a.fl && a.packed && a.cost && a.mask, MVSN_E_BADARG, "%s: null pointer", entry);
  MVSN_REQUIRE(n_chains > 0 && a.B > 0 && a.D >= 1 && a.rows > 0 && a.cols > 0, MVSN_E_BADARG, "%s: bad sizes", entry);
  MVSN_REQUIRE(form >= 0 && form <= 4, MVSN_E_BADARG, "%s: form must be 0 .. 4", entry);
  const ChainPlan p = chain_resolve(n_chains, a.D, a.rows, a.cols, form, guarded, true);
  // everything the repair launch needs is validated BEFORE the banded launch is enqueued: an error return must not
  // leave an unrepaired banded chain (NaN on a time-out) behind on the stream
  MVSN_REQUIRE(!p.repair_workspace_bytes || (repair_workspace && repair_workspace_bytes >= p.repair_workspace_bytes),
               MVSN_E_WORKSPACE, "%s: repair workspace of %zu bytes required", entry, p.repair_workspace_bytes);
  if (int rc = chain_launch(entry, a, n_chains, workspace, workspace_bytes, p, (hipStream_t)stream)) return rc;
  if (!p.repair_form) return 0;   // (the other forms have no inter-workgroup hand-offs to time out)
  a.gate = reinterpret_cast<const unsigned *>(static_cast<const char *>(workspace) + p.status_offset);
  a.sticky = sticky_status;
  return chain_launch(entry, a, n_chains, repair_workspace, repair_workspace_bytes,
                      chain_resolve(n_chains, a.D, a.rows, a.cols, p.repair_form, false, true), (hipStream_t)stream);
}

}  // namespace mvsn

extern "C" size_t mvsn_feature_refiner_packed_floats(void) { return mvsn::PACKED_FLOATS; }

extern "C" int mvsn_pack_feature_refiner(const float *conv0_w, const float *conv0_b, const float *bn0_w,
                                         const float *bn0_b, const float *res0_w, const float *res0_b,
                                         const float *res0_bn_w, const float *res0_bn_b, const float *final_w,
                                         const float *final_b, float *packed, mvsn_stream_t stream) {
  MVSN_REQUIRE(conv0_w && conv0_b && bn0_w && bn0_b && res0_w && res0_b && res0_bn_w && res0_bn_b && final_w &&
                   final_b && packed,
               MVSN_E_BADARG, "mvsn_pack_feature_refiner: null pointer");
  hipLaunchKernelGGL(mvsn::pack_refiner_kernel, dim3((mvsn::CH_STEPS_OFFSET + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, conv0_w, conv0_b, bn0_w, bn0_b, res0_w, res0_b, res0_bn_w, res0_bn_b,
                     final_w, final_b, packed);
  if (int rc = mvsn::check_launch("mvsn_pack_feature_refiner")) return rc;
  // the same three layers in the convolution kernels' Winograd layout (stepwise form)
  float *u = packed + mvsn::CH_STEPS_OFFSET;
  if (int rc = mvsn::wino_pack_2d(conv0_w, 35, u, (hipStream_t)stream)) return rc;
  if (int rc = mvsn::wino_pack_2d(res0_w, 32, u + mvsn::CS_U0_FLOATS, (hipStream_t)stream)) return rc;
  return mvsn::wino_pack_2d(final_w, 32, u + mvsn::CS_U0_FLOATS + mvsn::CS_U1_FLOATS, (hipStream_t)stream);
}

// ---- planning exports: calls into chain_resolve ---------------------------------------------------------------------
extern "C" int mvsn_incremental_cost_volume_resolve(int n_chains, int num_idepth_samples, int rows, int cols, int form,
                                                    int coresident_allowed, int guarded, size_t out[8]) {
  if (!out) return 0;
  const mvsn::ChainPlan p =
      mvsn::chain_resolve(n_chains, num_idepth_samples, rows, cols, form, guarded != 0, coresident_allowed != 0, true);
  out[0] = (size_t)p.form, out[1] = (size_t)p.repair_form, out[2] = p.workspace_bytes, out[3] = p.repair_workspace_bytes;
  out[4] = p.status_offset, out[5] = (size_t)p.groups, out[6] = p.redirected ? 1 : 0, out[7] = 0;
  return p.ok ? 1 : 0;
}

extern "C" int mvsn_incremental_cost_volume_form(int rows, int cols) {
  return mvsn::chain_resolve(1, 1, rows, cols, MVSN_CHAIN_WINOGRAD, false, true).ok ? MVSN_CHAIN_WINOGRAD : MVSN_CHAIN_DIRECT;
}

extern "C" size_t mvsn_incremental_cost_volume_workspace_bytes(int n_chains, int rows, int cols) {
  return mvsn::chain_resolve(n_chains, 1, rows, cols, MVSN_CHAIN_DIRECT, false, true).workspace_bytes;
}

extern "C" int mvsn_incremental_cost_volume_form_for(int n_chains, int rows, int cols) {
  if (n_chains <= 0 || rows <= 0 || cols <= 0) return MVSN_CHAIN_DIRECT;
  return mvsn::chain_resolve(n_chains, 1, rows, cols, MVSN_CHAIN_AUTO, true, true).form;
}

extern "C" size_t mvsn_incremental_cost_volume_workspace_bytes_for(int n_chains, int num_idepth_samples, int rows,
                                                                   int cols, int form) {
  if (num_idepth_samples <= 0) return 0;
  const size_t g = mvsn::chain_resolve(n_chains, num_idepth_samples, rows, cols, form, true, true).workspace_bytes;
  if (form != MVSN_CHAIN_AUTO) return g;
  // AUTO: enough for whichever entry point resolves it (the plain one differs beyond one thin-band pass)
  const size_t u = mvsn::chain_resolve(n_chains, num_idepth_samples, rows, cols, form, false, true).workspace_bytes;
  return g > u ? g : u;
}

extern "C" size_t mvsn_incremental_cost_volume_status_offset(int n_chains, int rows, int cols) {
  return mvsn::chain_resolve(n_chains, 1, rows, cols, MVSN_CHAIN_BANDED, false, true).status_offset;
}

extern "C" int mvsn_incremental_cost_volume_banded_groups(int n_chains, int rows, int cols) {
  return mvsn::chain_resolve(n_chains, 1, rows, cols, MVSN_CHAIN_BANDED, false, true).groups;
}

extern "C" size_t mvsn_incremental_cost_volume_repair_workspace_bytes(int n_chains, int rows, int cols) {
  return mvsn::chain_resolve(n_chains, 1, rows, cols, MVSN_CHAIN_BANDED, true, true).repair_workspace_bytes;
}

extern "C" int mvsn_debug_set_band_flags(int flags) {
  mvsn::chain_band_debug_flags(flags);
  return 0;
}

#ifdef MVSN_CHAIN_STAMPS
extern "C" int mvsn_debug_set_chain_stamps(void *buf) {
  mvsn::g_chain_stamps = (unsigned long long *)buf;
  return 0;
}
#endif

// ---- the entry points (include/mvsn_hip.h) --------------------------------------------------------------------------
extern "C" int mvsn_incremental_cost_volume(const float *src_image_lvl4, const float *H_lvl4, const float *H_inc,
                                            const float *plane0_features, const float *left_features,
                                            const float *refiner_packed, int n_chains, int batch,
                                            int num_idepth_samples, int rows, int cols, float *cost_volume,
                                            uint8_t *mask_volume, float *feature_volume, void *workspace,
                                            size_t workspace_bytes, int form, mvsn_stream_t stream) {
  const mvsn::ChainArgs a = mvsn::chain_args(src_image_lvl4, H_lvl4, H_inc, plane0_features, left_features, refiner_packed,
                                             batch, num_idepth_samples, rows, cols, cost_volume, false, mask_volume, feature_volume);
  return mvsn::chain_entry("mvsn_incremental_cost_volume", a, n_chains, workspace, workspace_bytes, form, false, nullptr, 0,
                           nullptr, stream);
}

extern "C" int mvsn_incremental_cost_volume_guarded(const float *src_image_lvl4, const float *H_lvl4, const float *H_inc,
                                                    const float *plane0_features, const float *left_features,
                                                    const float *refiner_packed, int n_chains, int batch,
                                                    int num_idepth_samples, int rows, int cols, float *cost_volume,
                                                    uint8_t *mask_volume, float *feature_volume, void *workspace,
                                                    size_t workspace_bytes, int form, void *repair_workspace,
                                                    size_t repair_workspace_bytes, unsigned *sticky_status,
                                                    mvsn_stream_t stream) {
  const mvsn::ChainArgs a = mvsn::chain_args(src_image_lvl4, H_lvl4, H_inc, plane0_features, left_features, refiner_packed,
                                             batch, num_idepth_samples, rows, cols, cost_volume, false, mask_volume, feature_volume);
  return mvsn::chain_entry("mvsn_incremental_cost_volume_guarded", a, n_chains, workspace, workspace_bytes, form, true,
                           repair_workspace, repair_workspace_bytes, sticky_status, stream);
}

// The guarded call with the cost volume stored as bf16 (the bf16 feature tier, BASELINE config 5; include/mvsn_hip.h).
extern "C" int mvsn_incremental_cost_volume_bf16(const float *src_image_lvl4, const float *H_lvl4, const float *H_inc,
                                                    const float *plane0_features, const float *left_features,
                                                    const float *refiner_packed, int n_chains, int batch,
                                                    int num_idepth_samples, int rows, int cols, void *cost_volume_bf16,
                                                    uint8_t *mask_volume, float *feature_volume, void *workspace,
                                                    size_t workspace_bytes, int form, void *repair_workspace,
                                                    size_t repair_workspace_bytes, unsigned *sticky_status,
                                                    mvsn_stream_t stream) {
  const mvsn::ChainArgs a = mvsn::chain_args(src_image_lvl4, H_lvl4, H_inc, plane0_features, left_features, refiner_packed,
                                             batch, num_idepth_samples, rows, cols, cost_volume_bf16, true, mask_volume, feature_volume);
  return mvsn::chain_entry("mvsn_incremental_cost_volume_bf16", a, n_chains, workspace, workspace_bytes, form, true,
                           repair_workspace, repair_workspace_bytes, sticky_status, stream);
}
