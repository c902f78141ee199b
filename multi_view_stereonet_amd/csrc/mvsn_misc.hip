// Small HBM-bound kernels either side of the cost-volume regulariser: soft-argmin, bilinear
// resize of idepth maps and hypothesis masks, multi-source fusion, the per-pixel confidence.
#include "mvsn_geom.h"

namespace mvsn {

// ---- soft-argmin over D -----------------------------------------------------------------
// cost (N,D,P): one thread per pixel walks D with stride P, so every load is a coalesced row
// segment; max-subtracted softmax of -cost (what torch.softmin computes).
__global__ __launch_bounds__(256) void soft_argmin_kernel(const float *__restrict__ cost,
                                                          const float *__restrict__ samples, int D, int P,
                                                          float *__restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = blockIdx.y;
  if (p >= P) return;
  const float *c = cost + (size_t)n * D * P + p;
  const float *s = samples + (size_t)n * D;
  // (sixteen independent loads in flight per round: at batch 1 the kernel is one latency chain per pixel)
  float m = -INFINITY;
  int d0 = 0;
  for (; d0 + 16 <= D; d0 += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = c[(size_t)(d0 + j) * P];
#pragma unroll
    for (int j = 0; j < 16; ++j) m = fmaxf(m, -v[j]);
  }
  for (int d = d0; d < D; ++d) m = fmaxf(m, -c[(size_t)d * P]);
  float den = 0.0f, num = 0.0f;
  for (d0 = 0; d0 + 16 <= D; d0 += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = c[(size_t)(d0 + j) * P];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float e = expf(-v[j] - m);
      den += e;
      num += e * s[d0 + j];
    }
  }
  for (int d = d0; d < D; ++d) {
    float e = expf(-c[(size_t)d * P] - m);
    den += e;
    num += e * s[d];
  }
  out[(size_t)n * P + p] = num / den;
}

// ---- soft-argmin that keeps the distribution's sharpness -------------------------
// The same walk and, for m, den and num, the same operations in the same order as soft_argmin_kernel (the idepth
// output is the same bits); the second pass also accumulates sum e * d.  Third step: the expected hypothesis index
// idx = (sum e d) / den, i = clamp(floor(idx), 0, D - 1), confidence = (e[i-1] + e[i] + e[i+1] + e[i+2]) / den with
// the terms outside [0, D) left out.  Its four loads re-read costs this workgroup has just read twice (cache hits);
// neighbouring pixels peak on neighbouring hypotheses, so they are still mostly row segments across the wave.
// A NaN cost makes den NaN: tested before anything is converted to an int, and written as NaN.
__global__ __launch_bounds__(256) void soft_argmin_confidence_kernel(const float *__restrict__ cost,
                                                                     const float *__restrict__ samples, int D, int P,
                                                                     float *__restrict__ out,
                                                                     float *__restrict__ confidence) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = blockIdx.y;
  if (p >= P) return;
  const float *c = cost + (size_t)n * D * P + p;
  const float *s = samples + (size_t)n * D;
  float m = -INFINITY;
  int d0 = 0;
  for (; d0 + 16 <= D; d0 += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = c[(size_t)(d0 + j) * P];
#pragma unroll
    for (int j = 0; j < 16; ++j) m = fmaxf(m, -v[j]);
  }
  for (int d = d0; d < D; ++d) m = fmaxf(m, -c[(size_t)d * P]);
  float den = 0.0f, num = 0.0f, idx = 0.0f;
  for (d0 = 0; d0 + 16 <= D; d0 += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = c[(size_t)(d0 + j) * P];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float e = expf(-v[j] - m);
      den += e;
      num += e * s[d0 + j];
      idx += e * (float)(d0 + j);
    }
  }
  for (int d = d0; d < D; ++d) {
    float e = expf(-c[(size_t)d * P] - m);
    den += e;
    num += e * s[d];
    idx += e * (float)d;
  }
  out[(size_t)n * P + p] = num / den;
  const float expected = idx / den;
  float conf = NAN;
  if (expected == expected) {   // (false for NaN: never converted)
    int i = (int)floorf(expected);
    i = i < 0 ? 0 : (i > D - 1 ? D - 1 : i);
    float w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d = i - 1 + k;
      const bool in = d >= 0 && d < D;
      w[k] = in ? c[(size_t)(in ? d : 0) * P] : INFINITY;   // exp(-inf) = 0: a term outside the range
    }
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += expf(-w[k] - m);
    conf = sum / den;
  }
  confidence[(size_t)n * P + p] = conf;
}

// min over the S sources of the per-chain confidences (chain n = s * B + b); a NaN in any source gives NaN
__global__ __launch_bounds__(256) void confidence_fuse_kernel(const float *__restrict__ conf, int S, int B, int P,
                                                              float *__restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (p >= P) return;
  float acc = conf[(size_t)b * P + p];
  for (int s = 1; s < S; ++s) {
    const float v = conf[((size_t)s * B + b) * P + p];
    acc = (v != v || v < acc) ? v : acc;   // (acc NaN: v < acc is false, it stays)
  }
  out[(size_t)b * P + p] = acc;
}

// out = (conf >= thr) && (valid == null || valid) as 0 / 1 bytes; NaN compares false
__global__ __launch_bounds__(256) void confidence_mask_kernel(const float *__restrict__ conf,
                                                              const uint8_t *__restrict__ valid, long count, float thr,
                                                              uint8_t *__restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const bool keep = conf[i] >= thr && (valid == nullptr || valid[i] != 0);
  out[i] = keep ? 1 : 0;
}

// ---- elementwise steps of the flag branches -----------------------------------------------------
__global__ __launch_bounds__(256) void channel_l2_norm_kernel(const float *__restrict__ x, int channels, long P,
                                                              float *__restrict__ out) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float *xp = x + (size_t)blockIdx.y * channels * P + p;
  float acc = 0.0f;
  for (int c = 0; c < channels; ++c) {
    const float v = xp[(size_t)c * P];
    acc += v * v;
  }
  out[(size_t)blockIdx.y * P + p] = sqrtf(acc);
}

// EPI false: out = prior * fx;  EPI true: out = relu(prior * fx + delta) / fx
template <bool EPI>
__global__ __launch_bounds__(256) void idepth_gain_kernel(const float *__restrict__ prior, const float *__restrict__ fx,
                                                          const float *__restrict__ delta, long P,
                                                          float *__restrict__ out) {
#pragma clang fp contract(off)   // prior*fx and the add are two separately rounded ATen ops in the reference
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float f = fx[blockIdx.y];
  const size_t i = (size_t)blockIdx.y * P + p;
  const float scaled = prior[i] * f;
  if constexpr (EPI) out[i] = relu_nan(scaled + delta[i]) / f;
  else out[i] = scaled;
}

// ---- bilinear resize, align_corners=False ------------------------------------------------
// src = (dst + 0.5) * (in/out) - 0.5, clamped at 0; the +1 tap is clamped to the last index
// (ATen upsample_bilinear2d, area_pixel_compute_source_index).
struct ResizeTap {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ ResizeTap resize_tap(int dst, int in_size, int out_size) {
  float scale = (float)in_size / (float)out_size;
  float src = ((float)dst + 0.5f) * scale - 0.5f;
  if (src < 0.0f) src = 0.0f;
  ResizeTap t;
  t.i0 = (int)src;
  if (t.i0 > in_size - 1) t.i0 = in_size - 1;
  t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.0f - t.l1;
  return t;
}

template <typename TIn, typename TOut, bool THRESH>
__global__ __launch_bounds__(256) void upsample_kernel(const TIn *__restrict__ in, int hin, int win, int hout,
                                                       int wout, TOut *__restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  const size_t plane = blockIdx.z;  // n*C + c
  if (x >= wout) return;
  ResizeTap ty = resize_tap(y, hin, hout);
  ResizeTap tx = resize_tap(x, win, wout);
  const TIn *ip = in + plane * hin * win;
  float v00 = (float)ip[ty.i0 * win + tx.i0], v01 = (float)ip[ty.i0 * win + tx.i1];
  float v10 = (float)ip[ty.i1 * win + tx.i0], v11 = (float)ip[ty.i1 * win + tx.i1];
  float v = ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
  if (THRESH)
    out[(plane * hout + y) * wout + x] = (TOut)(v > 0.5f ? 1 : 0);
  else
    out[(plane * hout + y) * wout + x] = (TOut)v;
}

// The coarse-to-fine step's prior: the upsampled idepth map AND its fx-scaled copy (the refiner's input channel,
// multi_view_stereonet.py:607-611) from one pass -- the scaling no longer costs a launch per level.
__global__ __launch_bounds__(256) void upsample_gain_kernel(const float *__restrict__ in, const float *__restrict__ gain,
                                                            int hin, int win, int hout, int wout,
                                                            float *__restrict__ out, float *__restrict__ out_scaled) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  const size_t plane = blockIdx.z;
  if (x >= wout) return;
  ResizeTap ty = resize_tap(y, hin, hout);
  ResizeTap tx = resize_tap(x, win, wout);
  const float *ip = in + plane * hin * win;
  float v00 = ip[ty.i0 * win + tx.i0], v01 = ip[ty.i0 * win + tx.i1];
  float v10 = ip[ty.i1 * win + tx.i0], v11 = ip[ty.i1 * win + tx.i1];
  float v = ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
  out[(plane * hout + y) * wout + x] = v;
  out_scaled[(plane * hout + y) * wout + x] = v * gain[plane];
}

// Mask variant: each thread produces 16 consecutive output columns of one row and stores them as
// one 128-bit word (the D-channel masks are the largest HBM stream of a forward; byte stores waste
// most of every write transaction).  1-D grid over (plane, row, 16-column group).
__global__ __launch_bounds__(256) void upsample_mask16_kernel(const uint8_t *__restrict__ in, int hin, int win,
                                                              int hout, int wout, int groups_per_row,
                                                              size_t total_groups, uint8_t *__restrict__ out) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total_groups) return;
  const int gx = (int)(gid % groups_per_row);
  const size_t rowid = gid / groups_per_row;  // plane * hout + y
  const int y = (int)(rowid % hout);
  const size_t plane = rowid / hout;
  const int x16 = gx * 16;
  ResizeTap ty = resize_tap(y, hin, hout);
  const uint8_t *r0 = in + (plane * hin + ty.i0) * win;
  const uint8_t *r1 = in + (plane * hin + ty.i1) * win;
  uint32_t w[4] = {0, 0, 0, 0};
  uint8_t vals[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int x = x16 + k < wout ? x16 + k : wout - 1;
    ResizeTap tx = resize_tap(x, win, wout);
    const float v00 = (float)r0[tx.i0], v01 = (float)r0[tx.i1], v10 = (float)r1[tx.i0], v11 = (float)r1[tx.i1];
    const float v = ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
    vals[k] = v > 0.5f ? 1 : 0;
    w[k >> 2] |= (uint32_t)vals[k] << (8 * (k & 3));
  }
  uint8_t *orow = out + rowid * wout;
  if (x16 + 15 < wout && (((size_t)(orow + x16)) & 15) == 0) {
    *reinterpret_cast<uint4 *>(orow + x16) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (x16 + k < wout) orow[x16 + k] = vals[k];
  }
}

// Exact 2x mask upsampling.  The masks are boolean (bytes 0 / 1): with the 2x bilinear weights an output pixel is
// (9 a + 3 b + 3 c + d) / 16 of its nearest input pixel a and three neighbours, and "> 0.5" of that is a itself
// (a = 1: at least 9/16; a = 0: at most 7/16), also where the clamped edge taps coincide -- so the float -> bilinear
// -> threshold of MaskUpsampler (:389-396) is a 2 x 2 replication.  One thread: 8 input bytes -> 2 rows x 16 bytes.
__global__ __launch_bounds__(256) void upsample_mask2x_kernel(const uint8_t *__restrict__ in, int hin, int win,
                                                              int groups_per_row, size_t total_groups,
                                                              uint8_t *__restrict__ out) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // (plane, input row, 8-column group)
  if (gid >= total_groups) return;
  const int gx = (int)(gid % groups_per_row);
  const size_t rowid = gid / groups_per_row;                           // plane * hin + y
  const uint2 w = *reinterpret_cast<const uint2 *>(in + rowid * win + gx * 8);
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  u32x4 o;
  o[0] = __builtin_amdgcn_perm(w.x, w.x, 0x01010000u);   // bytes b0 b0 b1 b1
  o[1] = __builtin_amdgcn_perm(w.x, w.x, 0x03030202u);   //       b2 b2 b3 b3
  o[2] = __builtin_amdgcn_perm(w.y, w.y, 0x01010000u);
  o[3] = __builtin_amdgcn_perm(w.y, w.y, 0x03030202u);
  uint8_t *dst = out + (rowid * 2) * (size_t)(win * 2) + gx * 16;
  __builtin_nontemporal_store(o, reinterpret_cast<u32x4 *>(dst));
  __builtin_nontemporal_store(o, reinterpret_cast<u32x4 *>(dst + win * 2));
}

// ---- area (adaptive average) downsample: one pyramid level ---------------------------------
// out size ((h+1)/2, (w+1)/2); window [floor(i*in/out), ceil((i+1)*in/out)) as ATen's
// adaptive_avg_pool2d (= interpolate(mode="area"), utils/image_utils.py:118-126): an exact 2x2
// mean for even sizes, overlapping windows for odd ones.
__global__ __launch_bounds__(256) void area_downsample_kernel(const float *__restrict__ in, int hin, int win,
                                                              int hout, int wout, float *__restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  const size_t plane = blockIdx.z;
  if (x >= wout) return;
  const int y0 = (y * hin) / hout, y1 = ((y + 1) * hin + hout - 1) / hout;
  const int x0 = (x * win) / wout, x1 = ((x + 1) * win + wout - 1) / wout;
  const float *ip = in + plane * hin * win;
  float sum = 0.0f;
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx) sum += ip[yy * win + xx];
  out[(plane * hout + y) * wout + x] = sum / (float)((y1 - y0) * (x1 - x0));
}

// ---- multi-source fusion -------------------------------------------------------------------
__global__ __launch_bounds__(256) void fuse_idepth_kernel(const float *__restrict__ raw,
                                                          const float *__restrict__ refined,
                                                          const float *__restrict__ baseline, int S, int B, int P,
                                                          int alias, float *__restrict__ raw_out,
                                                          float *__restrict__ refined_out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (p >= P) return;
  float sr = 0.0f, sf = 0.0f;
  for (int s = 0; s < S; ++s) {
    const size_t n = (size_t)s * B + b;
    const float base = baseline[n];
    float r = raw[n * P + p] / base;
    float f;
    if (alias) {  // reference quirk: refined aliases raw, which is divided in place twice
      r = r / base;
      f = r;
    } else {
      f = refined[n * P + p] / base;
    }
    sr += r;
    sf += f;
  }
  raw_out[(size_t)b * P + p] = sr / (float)S;
  refined_out[(size_t)b * P + p] = sf / (float)S;
}

__global__ __launch_bounds__(256) void fuse_mask_kernel(const uint8_t *__restrict__ mask, int S, int B, size_t DP,
                                                        uint8_t *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= DP) return;
  float acc = 0.0f;
  for (int s = 0; s < S; ++s) acc += (float)mask[((size_t)s * B + b) * DP + i];
  out[(size_t)b * DP + i] = (acc / (float)S) > 0.5f ? 1 : 0;
}

}  // namespace mvsn

extern "C" int mvsn_soft_argmin(const float *cost, const float *idepth_samples, int n, int D, int pixels,
                                float *idepth, mvsn_stream_t stream) {
  MVSN_REQUIRE(cost && idepth_samples && idepth, MVSN_E_BADARG, "mvsn_soft_argmin: null pointer");
  MVSN_REQUIRE(n > 0 && D > 0 && pixels > 0 && n <= 65535, MVSN_E_BADARG, "mvsn_soft_argmin: bad sizes");
  hipLaunchKernelGGL(mvsn::soft_argmin_kernel, dim3((pixels + 255) / 256, n), dim3(256), 0, (hipStream_t)stream,
                     cost, idepth_samples, D, pixels, idepth);
  return mvsn::check_launch("mvsn_soft_argmin");
}

extern "C" int mvsn_soft_argmin_confidence(const float *cost, const float *idepth_samples, int n, int D, int pixels,
                                           float *idepth, float *confidence, mvsn_stream_t stream) {
  MVSN_REQUIRE(cost && idepth_samples && idepth && confidence, MVSN_E_BADARG, "mvsn_soft_argmin_confidence: null pointer");
  MVSN_REQUIRE(n > 0 && D > 0 && pixels > 0 && n <= 65535, MVSN_E_BADARG, "mvsn_soft_argmin_confidence: bad sizes");
  hipLaunchKernelGGL(mvsn::soft_argmin_confidence_kernel, dim3((pixels + 255) / 256, n), dim3(256), 0,
                     (hipStream_t)stream, cost, idepth_samples, D, pixels, idepth, confidence);
  return mvsn::check_launch("mvsn_soft_argmin_confidence");
}

extern "C" int mvsn_confidence_fuse_sources(const float *confidence, int n_sources, int batch, int pixels, float *out,
                                            mvsn_stream_t stream) {
  MVSN_REQUIRE(confidence && out, MVSN_E_BADARG, "mvsn_confidence_fuse_sources: null pointer");
  MVSN_REQUIRE(n_sources > 0 && batch > 0 && batch <= 65535 && pixels > 0, MVSN_E_BADARG,
               "mvsn_confidence_fuse_sources: bad sizes");
  hipLaunchKernelGGL(mvsn::confidence_fuse_kernel, dim3((pixels + 255) / 256, batch), dim3(256), 0, (hipStream_t)stream,
                     confidence, n_sources, batch, pixels, out);
  return mvsn::check_launch("mvsn_confidence_fuse_sources");
}

extern "C" int mvsn_confidence_mask(const float *confidence, const uint8_t *valid, long count, float min_confidence,
                                    uint8_t *out, mvsn_stream_t stream) {
  MVSN_REQUIRE(confidence && out, MVSN_E_BADARG, "mvsn_confidence_mask: null pointer");
  MVSN_REQUIRE(count > 0 && (count + 255) / 256 <= 2147483647L, MVSN_E_BADARG, "mvsn_confidence_mask: bad sizes");
  MVSN_REQUIRE(min_confidence == min_confidence, MVSN_E_BADARG, "mvsn_confidence_mask: the threshold is NaN");
  hipLaunchKernelGGL(mvsn::confidence_mask_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, confidence, valid, count, min_confidence, out);
  return mvsn::check_launch("mvsn_confidence_mask");
}

namespace mvsn {
__global__ void gather_strided_kernel(const float *__restrict__ src, int count, long stride, float *__restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) dst[i] = src[(size_t)i * stride];
}
}  // namespace mvsn

namespace mvsn {
struct FocalSrc {
  const float *K[8];
};
__global__ void gather_focal_kernel(FocalSrc src, int levels, int batch, float *__restrict__ out, MVSN_VIS10) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < levels * batch) out[i] = src.K[i / batch][(size_t)(i % batch) * 16];
}
}  // namespace mvsn

extern "C" int mvsn_gather_focal(const float *const *K_pyr, int levels, int batch, float *fx, mvsn_stream_t stream) {
  MVSN_REQUIRE(K_pyr && fx && levels >= 1 && levels <= 8 && batch > 0, MVSN_E_BADARG, "mvsn_gather_focal: bad arguments");
  mvsn::FocalSrc src = {};
  for (int l = 0; l < levels; ++l) {
    MVSN_REQUIRE(K_pyr[l], MVSN_E_BADARG, "mvsn_gather_focal: null pointer");
    src.K[l] = K_pyr[l];
  }
  const int total = levels * batch;
  hipLaunchKernelGGL(mvsn::gather_focal_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, levels,
                     batch, fx, (const void *)src.K[0], (const void *)src.K[1], (const void *)src.K[2],
                     (const void *)src.K[3], (const void *)src.K[4], (const void *)src.K[5], (const void *)src.K[6],
                     (const void *)src.K[7], (const void *)nullptr, (const void *)nullptr);   // MVSN_VIS10
  return mvsn::check_launch("mvsn_gather_focal");
}

extern "C" int mvsn_copy(void *dst, const void *src, size_t nbytes, mvsn_stream_t stream) {
  MVSN_REQUIRE(dst && src, MVSN_E_BADARG, "mvsn_copy: null pointer");
  if (nbytes == 0) return 0;
  hipError_t e = hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e != hipSuccess) {
    mvsn::set_error("mvsn_copy: %s", hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

namespace mvsn {
// Up to eight independent device-to-device copies in ONE launch, every buffer a plain pointer argument (the runtime
// sees what is written and read: MVSN_VIS10's rule; ATen's multi-tensor copy carries its pointers inside a struct).
// grid.y = pair; 16-byte accesses where both pointers and the size allow it, bytes otherwise.
struct CopySizes {
  size_t n[8];
};
__global__ __launch_bounds__(256) void copy8_kernel(void *d0, const void *s0, void *d1, const void *s1, void *d2,
                                                    const void *s2, void *d3, const void *s3, void *d4, const void *s4,
                                                    void *d5, const void *s5, void *d6, const void *s6, void *d7,
                                                    const void *s7, CopySizes sz) {
  void *const d[8] = {d0, d1, d2, d3, d4, d5, d6, d7};
  const void *const s[8] = {s0, s1, s2, s3, s4, s5, s6, s7};
  const int k = blockIdx.y;
  char *dst = nullptr;
  const char *src = nullptr;
  size_t n = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (i == k) dst = (char *)d[i], src = (const char *)s[i], n = sz.n[i];
  const size_t stride = (size_t)gridDim.x * 256, t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if ((((size_t)dst | (size_t)src | n) & 15) == 0) {
    for (size_t i = t; i < n / 16; i += stride) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
  } else {
    for (size_t i = t; i < n; i += stride) dst[i] = src[i];
  }
}
}  // namespace mvsn

extern "C" int mvsn_copy_many(void *const *dst, const void *const *src, const size_t *nbytes, int count,
                              mvsn_stream_t stream) {
  MVSN_REQUIRE(count >= 0 && (count == 0 || (dst && src && nbytes)), MVSN_E_BADARG, "mvsn_copy_many: bad arguments");
  for (int at = 0; at < count; at += 8) {
    const int m = count - at < 8 ? count - at : 8;
    void *d[8] = {};
    const void *s[8] = {};
    mvsn::CopySizes sz = {};
    size_t largest = 0;
    for (int i = 0; i < m; ++i) {
      MVSN_REQUIRE(nbytes[at + i] == 0 || (dst[at + i] && src[at + i]), MVSN_E_BADARG, "mvsn_copy_many: null pointer");
      d[i] = dst[at + i], s[i] = src[at + i], sz.n[i] = nbytes[at + i];
      if (sz.n[i] > largest) largest = sz.n[i];
    }
    if (largest == 0) continue;
    size_t blocks = (largest / 16 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    hipLaunchKernelGGL(mvsn::copy8_kernel, dim3((unsigned)blocks, m), dim3(256), 0, (hipStream_t)stream, d[0], s[0], d[1],
                       s[1], d[2], s[2], d[3], s[3], d[4], s[4], d[5], s[5], d[6], s[6], d[7], s[7], sz);
  }
  return mvsn::check_launch("mvsn_copy_many");
}

extern "C" int mvsn_gather_strided(const float *src, int count, long stride, float *dst, mvsn_stream_t stream) {
  MVSN_REQUIRE(src && dst && count > 0 && stride > 0, MVSN_E_BADARG, "mvsn_gather_strided: bad arguments");
  hipLaunchKernelGGL(mvsn::gather_strided_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, count,
                     stride, dst);
  return mvsn::check_launch("mvsn_gather_strided");
}

extern "C" int mvsn_channel_l2_norm(const float *x, int n, int channels, long pixels, float *out,
                                    mvsn_stream_t stream) {
  MVSN_REQUIRE(x && out, MVSN_E_BADARG, "mvsn_channel_l2_norm: null pointer");
  MVSN_REQUIRE(n > 0 && n <= 65535 && channels > 0 && pixels > 0, MVSN_E_BADARG, "mvsn_channel_l2_norm: bad sizes");
  hipLaunchKernelGGL(mvsn::channel_l2_norm_kernel, dim3((unsigned)((pixels + 255) / 256), n), dim3(256), 0,
                     (hipStream_t)stream, x, channels, pixels, out);
  return mvsn::check_launch("mvsn_channel_l2_norm");
}

extern "C" int mvsn_idepth_scale(const float *prior, const float *fx, int n, long pixels, float *out,
                                 mvsn_stream_t stream) {
  MVSN_REQUIRE(prior && fx && out, MVSN_E_BADARG, "mvsn_idepth_scale: null pointer");
  MVSN_REQUIRE(n > 0 && n <= 65535 && pixels > 0, MVSN_E_BADARG, "mvsn_idepth_scale: bad sizes");
  hipLaunchKernelGGL(mvsn::idepth_gain_kernel<false>, dim3((unsigned)((pixels + 255) / 256), n), dim3(256), 0,
                     (hipStream_t)stream, prior, fx, (const float *)nullptr, pixels, out);
  return mvsn::check_launch("mvsn_idepth_scale");
}

extern "C" int mvsn_refiner_epilogue(const float *prior, const float *fx, const float *delta, int n, long pixels,
                                     float *out, mvsn_stream_t stream) {
  MVSN_REQUIRE(prior && fx && delta && out, MVSN_E_BADARG, "mvsn_refiner_epilogue: null pointer");
  MVSN_REQUIRE(n > 0 && n <= 65535 && pixels > 0, MVSN_E_BADARG, "mvsn_refiner_epilogue: bad sizes");
  hipLaunchKernelGGL(mvsn::idepth_gain_kernel<true>, dim3((unsigned)((pixels + 255) / 256), n), dim3(256), 0,
                     (hipStream_t)stream, prior, fx, delta, pixels, out);
  return mvsn::check_launch("mvsn_refiner_epilogue");
}

extern "C" int mvsn_upsample_bilinear(const float *in, int n, int channels, int rows_in, int cols_in, int rows_out,
                                      int cols_out, float *out, mvsn_stream_t stream) {
  MVSN_REQUIRE(in && out, MVSN_E_BADARG, "mvsn_upsample_bilinear: null pointer");
  MVSN_REQUIRE(n > 0 && channels > 0 && rows_in > 0 && cols_in > 0 && rows_out > 0 && cols_out > 0, MVSN_E_BADARG,
               "mvsn_upsample_bilinear: bad sizes");
  MVSN_REQUIRE((long)n * channels <= 65535 && rows_out <= 65535, MVSN_E_TOOLARGE, "mvsn_upsample_bilinear: grid");
  dim3 grid((cols_out + 255) / 256, rows_out, n * channels);
  hipLaunchKernelGGL((mvsn::upsample_kernel<float, float, false>), grid, dim3(256), 0, (hipStream_t)stream, in,
                     rows_in, cols_in, rows_out, cols_out, out);
  return mvsn::check_launch("mvsn_upsample_bilinear");
}

extern "C" int mvsn_upsample_prior(const float *in, const float *fx, int n, int rows_in, int cols_in, int rows_out,
                                   int cols_out, float *out, float *out_scaled, mvsn_stream_t stream) {
  MVSN_REQUIRE(in && fx && out && out_scaled, MVSN_E_BADARG, "mvsn_upsample_prior: null pointer");
  MVSN_REQUIRE(n > 0 && rows_in > 0 && cols_in > 0 && rows_out > 0 && cols_out > 0, MVSN_E_BADARG,
               "mvsn_upsample_prior: bad sizes");
  MVSN_REQUIRE(n <= 65535 && rows_out <= 65535, MVSN_E_TOOLARGE, "mvsn_upsample_prior: grid");
  dim3 grid((cols_out + 255) / 256, rows_out, n);
  hipLaunchKernelGGL(mvsn::upsample_gain_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, fx, rows_in, cols_in,
                     rows_out, cols_out, out, out_scaled);
  return mvsn::check_launch("mvsn_upsample_prior");
}

extern "C" int mvsn_upsample_mask(const uint8_t *in, int n, int channels, int rows_in, int cols_in, int rows_out,
                                  int cols_out, uint8_t *out, mvsn_stream_t stream) {
  MVSN_REQUIRE(in && out, MVSN_E_BADARG, "mvsn_upsample_mask: null pointer");
  MVSN_REQUIRE(n > 0 && channels > 0 && rows_in > 0 && cols_in > 0 && rows_out > 0 && cols_out > 0, MVSN_E_BADARG,
               "mvsn_upsample_mask: bad sizes");
  const int groups_per_row = (cols_out + 15) / 16;
  const size_t total = (size_t)n * channels * rows_out * groups_per_row;
  MVSN_REQUIRE((total + 255) / 256 < 2147483647ull, MVSN_E_TOOLARGE, "mvsn_upsample_mask: grid");
  if (rows_out == 2 * rows_in && cols_out == 2 * cols_in && cols_in % 8 == 0 && (((size_t)in | (size_t)out) & 15) == 0) {
    const size_t groups = (size_t)n * channels * rows_in * (cols_in / 8);
    hipLaunchKernelGGL(mvsn::upsample_mask2x_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, in, rows_in, cols_in, cols_in / 8, groups, out);
    return mvsn::check_launch("mvsn_upsample_mask(2x)");
  }
  hipLaunchKernelGGL(mvsn::upsample_mask16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, in, rows_in, cols_in, rows_out, cols_out, groups_per_row, total, out);
  return mvsn::check_launch("mvsn_upsample_mask");
}

extern "C" int mvsn_area_downsample(const float *in, int n, int channels, int rows_in, int cols_in, float *out,
                                    mvsn_stream_t stream) {
  MVSN_REQUIRE(in && out, MVSN_E_BADARG, "mvsn_area_downsample: null pointer");
  MVSN_REQUIRE(n > 0 && channels > 0 && rows_in > 0 && cols_in > 0, MVSN_E_BADARG, "mvsn_area_downsample: bad sizes");
  const int rows_out = (rows_in + 1) / 2, cols_out = (cols_in + 1) / 2;
  MVSN_REQUIRE((long)n * channels <= 65535 && rows_out <= 65535, MVSN_E_TOOLARGE, "mvsn_area_downsample: grid");
  dim3 grid((cols_out + 255) / 256, rows_out, n * channels);
  hipLaunchKernelGGL(mvsn::area_downsample_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, rows_in, cols_in,
                     rows_out, cols_out, out);
  return mvsn::check_launch("mvsn_area_downsample");
}

extern "C" int mvsn_fuse_sources(const float *raw, const float *refined, const float *baseline, const uint8_t *mask,
                                 int n_sources, int batch, int D, int pixels, int refined_aliases_raw,
                                 float *raw_out, float *refined_out, uint8_t *mask_out, mvsn_stream_t stream) {
  MVSN_REQUIRE(raw && baseline && mask && raw_out && refined_out && mask_out, MVSN_E_BADARG,
               "mvsn_fuse_sources: null pointer");
  MVSN_REQUIRE(refined || refined_aliases_raw, MVSN_E_BADARG, "mvsn_fuse_sources: refined is null");
  MVSN_REQUIRE(n_sources > 0 && batch > 0 && batch <= 65535 && D > 0 && pixels > 0, MVSN_E_BADARG,
               "mvsn_fuse_sources: bad sizes");
  hipLaunchKernelGGL(mvsn::fuse_idepth_kernel, dim3((pixels + 255) / 256, batch), dim3(256), 0, (hipStream_t)stream,
                     raw, refined, baseline, n_sources, batch, pixels, refined_aliases_raw, raw_out, refined_out);
  int rc = mvsn::check_launch("mvsn_fuse_sources(idepth)");
  if (rc) return rc;
  const size_t DP = (size_t)D * pixels;
  hipLaunchKernelGGL(mvsn::fuse_mask_kernel, dim3((unsigned)((DP + 255) / 256), batch), dim3(256), 0,
                     (hipStream_t)stream, mask, n_sources, batch, DP, mask_out);
  return mvsn::check_launch("mvsn_fuse_sources(mask)");
}

extern "C" int mvsn_fusion_gather(const float *maps, const int *view, const int *pixel, int n_views, long pixels_per_view,
                                  long count, float *out, mvsn_stream_t stream) {
  MVSN_REQUIRE(maps && view && pixel && out, MVSN_E_BADARG, "mvsn_fusion_gather: null pointer");
  MVSN_REQUIRE(n_views > 0 && pixels_per_view > 0 && pixels_per_view <= 2147483647L && count > 0 &&
                   (count + 255) / 256 <= 2147483647L,
               MVSN_E_BADARG, "mvsn_fusion_gather: bad sizes");
  hipLaunchKernelGGL(mvsn::gather_kernel<1>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     maps, view, pixel, n_views, pixels_per_view, count, out);
  return mvsn::check_launch("mvsn_fusion_gather");
}
