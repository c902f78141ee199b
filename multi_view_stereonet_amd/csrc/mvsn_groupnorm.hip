// GroupNorm(4 groups of 8 channels) behind every convolution tier: the producers (direct, Winograd, bf16 and tower
// kernels) leave per-tile records (count, mean, M2); here they become (mean, rstd) per (sample, group) -- in one
// workgroup per sample or in slices -- and the stand-alone normalise / activate / add pass reads them (see
// include/mvsn_hip.h: mvsn_groupnorm_finalize, mvsn_groupnorm_lrelu_apply).  The reductions themselves
// (gn_finalize_block, gn_partial_block, gn_stats_here) are in mvsn_common.h: the kernels that consume records share them.
#include "mvsn_common.h"

namespace mvsn {

// One workgroup per sample: gn_finalize_block (mvsn_common.h).
__global__ __launch_bounds__(256) void gn_finalize_kernel(const float *__restrict__ partials, int tiles,
                                                          float *__restrict__ stats) {
  const int n = blockIdx.x;
  gn_finalize_block(partials + (size_t)n * tiles * 12, tiles, stats + (size_t)n * 8);
}

// Split finalize: slice k of sample n's records -> 12 double sums; then one thread per (sample, group) adds the K slices in
// order.  (A level-0 layer of a 1024x512 frame leaves 32768 records = 1.5 MB per sample: one workgroup per sample read
// them in ~45 us -- 14 such launches per batch-1 forward, and at 32 samples 32 of the 256 CUs were at work.)
__global__ __launch_bounds__(256) void gn_partial_kernel(const float *__restrict__ partials, int tiles, int per, int K,
                                                         double *__restrict__ scratch) {
  const int k = blockIdx.x, n = blockIdx.y;
  const int lo = k * per, cnt = tiles - lo < per ? tiles - lo : per;
  gn_partial_block(partials + ((size_t)n * tiles + lo) * 12, cnt, scratch + ((size_t)n * K + k) * 12);
}
__global__ __launch_bounds__(256) void gn_combine_kernel(const double *__restrict__ scratch, int n, int K,
                                                         float *__restrict__ stats) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 4) return;
  const int s = t >> 2, g = t & 3;
  double N = 0.0, S = 0.0, Q = 0.0;
  for (int k = 0; k < K; ++k) {
    const double *p = scratch + ((size_t)s * K + k) * 12 + g * 3;
    N += p[0], S += p[1], Q += p[2];
  }
  const double mean = S / N;
  double var = Q / N - mean * mean;
  if (var < 0.0) var = 0.0;
  stats[(size_t)s * 8 + g * 2 + 0] = (float)mean;
  stats[(size_t)s * 8 + g * 2 + 1] = (float)(1.0 / sqrt(var + (double)GN_FINALIZE_EPS));
}
// slices per sample: a function of the records per sample ALONE (a sample's statistics must not depend on the batch it
// travels in); 1 up to 2048 records -- the range in which consumers may form the statistics themselves (gn_stats_here)
static inline int gn_split_slices(int tiles) { return tiles <= 2048 ? 1 : (tiles + 2047) / 2048 < 16 ? (tiles + 2047) / 2048 : 16; }

// out = [residual +] LeakyReLU(GroupNorm(x)), (N,32,spatial), float4 per thread.
constexpr int GN_APPLY_MAX_N = 65535 / 32;   // samples per launch (grid.y = sample * 32 + channel)

// RRAW: the residual is itself a raw conv output whose LeakyReLU(GroupNorm(.)) was never materialised
// (the head of a refiner): out = LReLU(GN(x)) + LReLU(GN_r(residual)).
template <bool RRAW>
__global__ __launch_bounds__(256) void gn_apply_kernel(const float *__restrict__ x, const float *__restrict__ stats,
                                                       const float *__restrict__ gamma,
                                                       const float *__restrict__ beta,
                                                       const float *__restrict__ residual,
                                                       const float *__restrict__ r_stats,
                                                       const float *__restrict__ r_gamma,
                                                       const float *__restrict__ r_beta, long spatial,
                                                       int stat_tiles, float *__restrict__ out) {
  const int plane = blockIdx.y;  // n*32 + c
  const int n = plane >> 5, c = plane & 31;
  __shared__ float gst[8];
  const float *st = gn_stats_here<true>(stats, stat_tiles, n, gst, c >> 3);   // (stat_tiles > 0: x's statistics from its records)
  const float mean = st[(c >> 3) * 2 + 0];
  const float rstd = st[(c >> 3) * 2 + 1];
  const float sc = rstd * gamma[c];
  const float sh = beta[c] - mean * sc;
  float rsc = 1.0f, rsh = 0.0f;
  if constexpr (RRAW) {
    const float rm = r_stats[((size_t)n * 4 + (c >> 3)) * 2 + 0];
    rsc = r_stats[((size_t)n * 4 + (c >> 3)) * 2 + 1] * r_gamma[c];
    rsh = r_beta[c] - rm * rsc;
  }
  auto res = [&](float v) { return RRAW ? lrelu02(v * rsc + rsh) : v; };
  const float *xp = x + (size_t)plane * spatial;
  const float *rp = residual ? residual + (size_t)plane * spatial : nullptr;
  float *op = out + (size_t)plane * spatial;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  const bool vec_ok = (spatial & 3) == 0;
  if (vec_ok) {
    // streaming pass: non-temporal 16-byte accesses, four independent iterations in flight per thread
    long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    for (; i + 3 * stride < spatial; i += 4 * stride) {
      floatx4 v[4], o[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const floatx4 *>(xp + i + u * stride));
      if (rp) {
        floatx4 rv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) rv[u] = __builtin_nontemporal_load(reinterpret_cast<const floatx4 *>(rp + i + u * stride));
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int k = 0; k < 4; ++k) o[u][k] = lrelu02(v[u][k] * sc + sh) + res(rv[u][k]);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int k = 0; k < 4; ++k) o[u][k] = lrelu02(v[u][k] * sc + sh);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(o[u], reinterpret_cast<floatx4 *>(op + i + u * stride));
    }
    for (; i < spatial; i += stride) {
      floatx4 v = *reinterpret_cast<const floatx4 *>(xp + i);
      floatx4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = lrelu02(v[k] * sc + sh);
      if (rp) {
        floatx4 rv = *reinterpret_cast<const floatx4 *>(rp + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] += res(rv[k]);
      }
      *reinterpret_cast<floatx4 *>(op + i) = o;
    }
  } else {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < spatial; i += (long)gridDim.x * blockDim.x) {
      float o = lrelu02(xp[i] * sc + sh);
      if (rp) o += res(rp[i]);
      op[i] = o;
    }
  }
}

}  // namespace mvsn

extern "C" int mvsn_groupnorm_finalize(const float *partials, int n, int tiles, float *stats, mvsn_stream_t stream) {
  MVSN_REQUIRE(partials && stats && n > 0 && tiles > 0, MVSN_E_BADARG, "mvsn_groupnorm_finalize: bad argument");
  hipLaunchKernelGGL(mvsn::gn_finalize_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, partials, tiles, stats);
  return mvsn::check_launch("mvsn_groupnorm_finalize");
}

extern "C" size_t mvsn_groupnorm_finalize_split_workspace_bytes(int n, int tiles) {
  if (n <= 0 || tiles <= 0) return 0;
  const int K = mvsn::gn_split_slices(tiles);
  return K == 1 ? 0 : (size_t)n * K * 12 * sizeof(double);
}

extern "C" int mvsn_groupnorm_finalize_split(const float *partials, int n, int tiles, float *stats, void *workspace,
                                             size_t workspace_bytes, mvsn_stream_t stream) {
  MVSN_REQUIRE(partials && stats && n > 0 && tiles > 0, MVSN_E_BADARG, "mvsn_groupnorm_finalize_split: bad argument");
  const int K = mvsn::gn_split_slices(tiles);
  if (K == 1) return mvsn_groupnorm_finalize(partials, n, tiles, stats, stream);
  const size_t need = mvsn_groupnorm_finalize_split_workspace_bytes(n, tiles);
  MVSN_REQUIRE(workspace && workspace_bytes >= need && ((size_t)workspace & 7) == 0, MVSN_E_WORKSPACE,
               "mvsn_groupnorm_finalize_split: 8-byte aligned workspace of %zu bytes required", need);
  MVSN_REQUIRE(n <= 65535, MVSN_E_TOOLARGE, "mvsn_groupnorm_finalize_split: batch too large for one launch");
  const int per = (tiles + K - 1) / K;
  hipLaunchKernelGGL(mvsn::gn_partial_kernel, dim3(K, n), dim3(256), 0, (hipStream_t)stream, partials, tiles, per, K,
                     (double *)workspace);
  hipLaunchKernelGGL(mvsn::gn_combine_kernel, dim3((n * 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const double *)workspace, n, K, stats);
  return mvsn::check_launch("mvsn_groupnorm_finalize_split");
}

// stat_tiles == 0: `stats` is the finalised (N,4,2) array; > 0: the producer's records (N, stat_tiles, 4, 3), finalised by
// every workgroup of the pass itself (gn_stats_here)
extern "C" int mvsn_groupnorm_lrelu_apply(const float *x, const float *stats, int stat_tiles, const float *gamma,
                                          const float *beta, const float *residual, const float *r_stats,
                                          const float *r_gamma, const float *r_beta, int n, long spatial, float *out,
                                          mvsn_stream_t stream) {
  MVSN_REQUIRE(x && stats && stat_tiles >= 0 && gamma && beta && out && n > 0 && spatial > 0, MVSN_E_BADARG,
               "mvsn_groupnorm_lrelu_apply: bad argument");
  MVSN_REQUIRE(!r_stats || (residual && r_gamma && r_beta), MVSN_E_BADARG,
               "mvsn_groupnorm_lrelu_apply: a raw residual needs its statistics, gamma and beta");
  long per = (spatial + 4095) / 4096;   // 4 float4 per thread per pass
  int gx = (int)(per < 1 ? 1 : (per > 32 ? 32 : per));
  const long sstride = stat_tiles > 0 ? (long)stat_tiles * 12 : 8;
  for (int n0 = 0; n0 < n; n0 += mvsn::GN_APPLY_MAX_N) {   // grid.y carries (sample, channel): 2047 samples per launch
    const int nn = n - n0 < mvsn::GN_APPLY_MAX_N ? n - n0 : mvsn::GN_APPLY_MAX_N;
    const long off = (long)n0 * 32 * spatial;
    if (r_stats)
      hipLaunchKernelGGL(mvsn::gn_apply_kernel<true>, dim3(gx, nn * 32), dim3(256), 0, (hipStream_t)stream, x + off,
                         stats + (long)n0 * sstride, gamma, beta, residual + off, r_stats + (long)n0 * 8, r_gamma, r_beta,
                         spatial, stat_tiles, out + off);
    else
      hipLaunchKernelGGL(mvsn::gn_apply_kernel<false>, dim3(gx, nn * 32), dim3(256), 0, (hipStream_t)stream, x + off,
                         stats + (long)n0 * sstride, gamma, beta, residual ? residual + off : residual,
                         (const float *)nullptr, (const float *)nullptr, (const float *)nullptr, spatial, stat_tiles,
                         out + off);
  }
  return mvsn::check_launch("mvsn_groupnorm_lrelu_apply");
}
