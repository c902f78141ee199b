// ---------------------------------------------------------------------------------------------
// 32 -> 1 channel 3x3 / 3x3x3 convolution (the last layer of every refiner and of the regulariser)
// ---------------------------------------------------------------------------------------------
// At 128 input bytes per output the layer is HBM-bound.  One output channel has no cout dimension to put
// on MFMA directly; the 3-D layer (27 taps) instead puts the TAPS on it (tap GEMM, further down), the 2-D
// layer (9 taps) runs on the vector ALUs: each thread owns 4 consecutive output
// columns of one row, reads the three neighbouring input rows of every channel as aligned
// float4 and takes the two halo columns from its lane neighbours with wave shuffles (a 16-lane group
// spans 64 columns; only the group's edge lanes touch memory for the halo).  Weights are wave-uniform
// (scalar loads).  Optional refiner epilogue: relu(prior*fx + conv + bias) / fx
// (multi_view_stereonet.py:482 with the gain trick of :607-611).
#include "mvsn_resident.h"

namespace mvsn {

// ---- 32 -> 1 channel 3x3x3 as a tap GEMM ------------------------------------------------------------------
// out[z][y][x] = sum_tap P[tap][z + dz - 1][y + dy - 1][x + dx - 1],  P[tap][v] = sum_c w[c][tap] in[c][v].
// P is a (27 x 32) by (32 x voxels) product: it runs on the fp32 matrix cores, every input element is read
// from HBM exactly once (one 16-byte load feeds four MFMAs), and the 27-tap shift-and-add reads P back from
// LDS.  A workgroup owns a 16 x 32 pixel tile and a slab of planes and streams through the slab: per input
// plane it forms P over the haloed tile (18 rows x 40 columns from the aligned column x0 - 4 = 720 slots),
// then every thread adds the plane's contribution to the three output planes it touches for its two pixels
// (rolling accumulators) and writes the plane that just became complete.
//   A = taps (16 per MFMA, 2 tiles) x 4 cins, held in registers for the whole kernel
//   B = 4 cins x 16 slots: lane (k, i) loads slots 64g + 4i .. + 3 of channel 4 ks + k with one dwordx4;
//       register p of that load is the B fragment of "slot tile p" = slots {64g + 4i + p}, so the four
//       accumulators of a lane are four CONSECUTIVE slots of one tap row -> one 16-byte LDS write.
constexpr int T3_TY = 16, T3_TX = 32;
constexpr int T3_HY = T3_TY + 2, T3_XS = 40;          // haloed rows, row stride in slots
constexpr int T3_SLOTS = T3_HY * T3_XS;               // 720
constexpr int T3_GROUPS = (T3_SLOTS + 63) / 64;       // 12 groups of 64 slots, 3 per wave
constexpr int T3_LDS_FLOATS = 27 * T3_SLOTS;          // 77,760 bytes: two workgroups per CU

// XF: the input is a raw convolution output whose LeakyReLU(GroupNorm(.)) is applied on load (two VALU per
// element behind an HBM-bound stream) -- the regulariser's last normalise/activate pass never touches HBM.
// WHOLE: the plane IS the tile (16 x 32, the headline's coarse grid): the 208 halo slots of the 720 lie outside the
// volume for every plane -- their rows of P are zeroed once and never written, the products cover the 512 real slots
// only (two full 64-slot groups per wave instead of three partly idle ones: a third fewer multiplies -- at 22 flop per
// input byte the tap GEMM needs most of the fp32 matrix pipe at the HBM rate -- and every lane of every load carries
// data), and a plane's two groups are requested while the previous plane is gathered.
template <bool XF, bool WHOLE>
__global__ __launch_bounds__(256, 2) void conv_to1_3d_mfma_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                                  const float *__restrict__ bias,
                                                                  const float *__restrict__ in_stats,
                                                                  const float *__restrict__ in_gamma,
                                                                  const float *__restrict__ in_beta, int D, int H, int W,
                                                                  int ntx, int zslab, float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float P[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.z;
  const int tile = xcd_tile_index(blockIdx.x, gridDim.x);
  const int tyi = tile / ntx, txi = tile - tyi * ntx;
  const int y0 = tyi * T3_TY, x0 = txi * T3_TX;
  const int zb = blockIdx.y * zslab, ze = min(D, zb + zslab);   // output planes [zb, ze)
  const size_t plane = (size_t)H * W, chan = (size_t)D * plane;
  const float *inn = in + (size_t)n * 32 * chan + (size_t)(lane >> 4) * chan;   // this lane's k (cin within a k-step)

  // tap weights as A fragments: a[t][ks] = w[cin = 4 ks + (lane>>4)][tap = 16 t + (lane&15)]
  float a[2][8];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int tap = t * 16 + (lane & 15), c = ks * 4 + (lane >> 4);
      a[t][ks] = tap < 27 ? w[c * 27 + tap] : 0.0f;
    }

  float xsc[8], xsh[8];   // XF: per k-step scale / shift of this lane's channel 4 ks + (lane>>4) (group ks >> 1)
  if constexpr (XF) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int c = ks * 4 + (lane >> 4);
      const float mean = in_stats[((size_t)n * 4 + (ks >> 1)) * 2], rstd = in_stats[((size_t)n * 4 + (ks >> 1)) * 2 + 1];
      xsc[ks] = rstd * in_gamma[c];
      xsh[ks] = in_beta[c] - mean * xsc[ks];
    }
  }

  // this lane's slots: group g = wave + 4 u, slots 64 g + 4 (lane&15) .. + 3
  constexpr int GPW = WHOLE ? 2 : T3_GROUPS / 4;   // 3 (WHOLE: 8 groups of 64 REAL slots, 2 per wave)
  int goff[GPW];   // global offset of the lane's four slots inside a plane (-1: outside the volume)
  int lslot[GPW];  // their first slot in P (-1: beyond the tile)
#pragma unroll
  for (int u = 0; u < GPW; ++u) {
    const int s0 = (wave + 4 * u) * 64 + 4 * (lane & 15);
    if constexpr (WHOLE) {   // H == 16, W == 32, one tile: pixel index == plane offset
      goff[u] = s0;
      lslot[u] = ((s0 >> 5) + 1) * T3_XS + (s0 & 31) + 4;
    } else {
      const int row = s0 / T3_XS, col = s0 - row * T3_XS;
      const int gy = y0 - 1 + row, gx = x0 - 4 + col;
      goff[u] = (s0 < T3_SLOTS && gy >= 0 && gy < H && gx >= 0 && gx < W) ? gy * W + gx : -1;
      lslot[u] = s0 < T3_SLOTS ? s0 : -1;
    }
  }
  if constexpr (WHOLE) {   // halo slots of every tap row: zero, once
    for (int i = tid * 4; i < T3_LDS_FLOATS; i += 1024) *reinterpret_cast<floatx4 *>(P + i) = floatx4{0.f, 0.f, 0.f, 0.f};
    lds_barrier();
  }

  // gather side: this thread's two output pixels (xx even)
  const int oy = tid >> 4, ox = (tid & 15) * 2;
  const bool o_ok = y0 + oy < H && x0 + ox < W;          // W % 4 == 0: both pixels or neither
  const float *pg = P + oy * T3_XS + ox + 3;             // tap (dy, dx) adds dy * T3_XS + dx
  float acc[3][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // output planes z-1, z, z+1 of the current input plane z
  const float b = bias ? bias[0] : 0.0f;
  float *outn = out + (size_t)n * chan + (size_t)(y0 + oy) * W + x0 + ox;

  // The stream over the slab's planes is software-pipelined ACROSS planes, two slot groups ahead: a group's 64
  // multiplies take ~0.85 us, an HBM round trip under load more than twice that, and with one request burst per plane
  // (round 2) the kernel sat at 27 % of the HBM rate.  Three groups per plane, three register buffers: group u of every
  // plane lives in bfr[u]; while group u multiplies, group u + 2 (of this plane or the next) is requested.
  floatx4 bfr[3][8];
  auto load_group = [&](int z, int u, floatx4 (&dst)[8]) {
    const float *src = inn + (size_t)z * plane + (goff[u] >= 0 ? goff[u] : 0);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
      dst[ks] = goff[u] >= 0 ? __builtin_nontemporal_load(reinterpret_cast<const floatx4 *>(src + (size_t)ks * 4 * chan))
                             : floatx4{0.f, 0.f, 0.f, 0.f};
  };
  auto activate = [&](int u, floatx4 (&dst)[8]) {
    if constexpr (XF) {   // padding stays zero: it pads the ACTIVATED tensor
      if (goff[u] >= 0) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
          for (int p = 0; p < 4; ++p) dst[ks][p] = lrelu02(dst[ks][p] * xsc[ks] + xsh[ks]);
      }
    }
  };
  static_assert(GPW == (WHOLE ? 2 : 3), "the plane pipeline below is written for three (WHOLE: two) slot groups per wave");
  const int zfirst = zb - 1 < 0 ? 0 : zb - 1, zlast = ze < D ? ze : D - 1;   // input planes inside the volume
  if (zfirst <= zlast) {
    load_group(zfirst, 0, bfr[0]);
    load_group(zfirst, 1, bfr[1]);
  }
  auto plane_products = [&](int z) {
#pragma unroll
    for (int u = 0; u < GPW; ++u) {
      if constexpr (!WHOLE) {
        if (u == 0) load_group(z, 2, bfr[2]);
        else if (z + 1 <= zlast) load_group(z + 1, u - 1, bfr[u - 1]);   // next plane: in flight across the barriers below
      }
      activate(u, bfr[u]);
      floatx4 d[2][4];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int p = 0; p < 4; ++p) d[t][p] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          d[0][p] = mfma16x16x4(a[0][ks], bfr[u][ks][p], d[0][p]);
          d[1][p] = mfma16x16x4(a[1][ks], bfr[u][ks][p], d[1][p]);
        }
      // WHOLE: the group's registers are free again -- the same group of the next plane travels during the rest of this
      // plane (the other group's multiplies, the gather and both barriers)
      if constexpr (WHOLE) {
        if (z + 1 <= zlast) load_group(z + 1, u, bfr[u]);
      }
      // lane holds taps 16 t + 4 (lane>>4) + r of slots s0 .. s0 + 3
      const int s0 = lslot[u];
      if (s0 >= 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int tap = t * 16 + (lane >> 4) * 4 + r;
            if (tap < 27)
              *reinterpret_cast<floatx4 *>(P + tap * T3_SLOTS + s0) = floatx4{d[t][0][r], d[t][1][r], d[t][2][r], d[t][3][r]};
          }
      }
    }
  };

  for (int z = zb - 1; z <= ze; ++z) {
    if (z >= 0 && z < D) {   // uniform: planes outside the volume contribute nothing
      // ---- P = taps x slots for plane z
      plane_products(z);
      lds_barrier();   // (LDS only: the next plane's first loads stay in flight across it)
      // ---- shift-and-add: input plane z feeds output planes z + 1 (dz = 0), z (dz = 1), z - 1 (dz = 2)
#pragma unroll
      for (int dz = 0; dz < 3; ++dz)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const float *q = pg + (dz * 9 + dy * 3 + dx) * T3_SLOTS + dy * T3_XS + dx;
            acc[2 - dz][0] += q[0];
            acc[2 - dz][1] += q[1];
          }
    }
    // output plane z - 1 is complete
    if (z - 1 >= zb && z - 1 < ze && o_ok) {
      float2 v = make_float2(acc[0][0] + b, acc[0][1] + b);
      *reinterpret_cast<float2 *>(outn + (size_t)(z - 1) * plane) = v;
    }
    acc[0][0] = acc[1][0], acc[0][1] = acc[1][1];
    acc[1][0] = acc[2][0], acc[1][1] = acc[2][1];
    acc[2][0] = 0.f, acc[2][1] = 0.f;
    lds_barrier();   // everyone is done reading P before the next plane overwrites it
  }
}

// ---- 32 -> 1 channel 3x3 (2-D) the same way: 9 taps = one MFMA row tile ------------------------------------
// One workgroup per 16 x 32 tile.  XFORM: the input is not materialised -- the kernel reads the raw
// output r of the tower's last conv and the block input x and forms x + LeakyReLU(GN(r)) on the B
// fragments in registers (zero outside the image, as the padding of the materialised tensor would be),
// i.e. the last residual block's normalise/activate/add pass is folded into this layer's load.
// Epilogue (optional): the refiner's relu(prior * fx + conv + bias) / fx.
// Output tiles of 16 x TX: 16 x 64 (an 18 x 72-slot haloed tile = 1.27x the outputs) when there are enough tiles to
// fill the chip, 16 x 32 (1.41x, twice the workgroups) otherwise.  The halo lines of a 32-channel x 2-tensor stream
// do not all stay in the 4 MB L2, so the ratio is HBM traffic: level-0 folded block at batch 128 1.36 -> 1.12 ms
// (3.1 -> 3.9 TB/s algorithmic); 16 x 128 tiles 1.18 ms; round 1 measured 8 x 64 (the same 1.41x) within 1 % of 16 x 32.
constexpr int T2_TY = 16;
template <int TX>
struct T2 {
  static constexpr int XS = TX + 8, SLOTS = (T2_TY + 2) * XS, GROUPS = (SLOTS + 63) / 64, LDS_FLOATS = 9 * SLOTS;
};
// wide tiles once they alone give every CU four workgroups
static inline bool to1_wide_tiles(int n, int rows, int cols) {
  return (long)n * ((rows + T2_TY - 1) / T2_TY) * ((cols + 63) / 64) >= 4L * device_cus();
}

template <bool XFORM, int T2_TX>
__global__ __launch_bounds__(256) void conv_to1_2d_mfma_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                               const float *__restrict__ bias,
                                                               const float *__restrict__ in_stats,
                                                               const float *__restrict__ in_gamma,
                                                               const float *__restrict__ in_beta,
                                                               const float *__restrict__ in_residual,
                                                               const float *__restrict__ prior, const float *__restrict__ fx,
                                                               int H, int W, int ntx, int stat_tiles,
                                                               float *__restrict__ out) {
  constexpr int T2_XS = T2<T2_TX>::XS, T2_SLOTS = T2<T2_TX>::SLOTS, T2_GROUPS = T2<T2_TX>::GROUPS;
  __shared__ __attribute__((aligned(16))) float P[T2<T2_TX>::LDS_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.y;
  const int tile = xcd_tile_index(blockIdx.x, gridDim.x);   // neighbouring tiles (shared halo lines) on one XCD's L2
  const int tyi = tile / ntx, txi = tile - tyi * ntx;
  const int y0 = tyi * T2_TY, x0 = txi * T2_TX;
  const size_t plane = (size_t)H * W;
  const int kc = lane >> 4;   // this lane's cin within a k-step
  const float *inn = in + ((size_t)n * 32 + kc) * plane;
  const float *resn = (XFORM && in_residual) ? in_residual + ((size_t)n * 32 + kc) * plane : nullptr;

  float a[8];   // A fragments: w[cin = 4 ks + kc][tap = lane & 15]
  float sc[8], sh[8];
  __shared__ float gst[8];
  const float *st = nullptr;
  if constexpr (XFORM) st = gn_stats_here(in_stats, stat_tiles, n, gst);   // (stat_tiles > 0: from the producer's records)
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const int tap = lane & 15, c = ks * 4 + kc;
    a[ks] = tap < 9 ? w[c * 9 + tap] : 0.0f;
    if constexpr (XFORM) {
      const float mean = st[(c >> 3) * 2 + 0];
      const float rstd = st[(c >> 3) * 2 + 1];
      sc[ks] = rstd * in_gamma[c];
      sh[ks] = in_beta[c] - mean * sc[ks];
    }
  }

  constexpr int GPW = (T2_GROUPS + 3) / 4;   // groups of 64 slots per wave (the last round may be partial)
#pragma unroll
  for (int u = 0; u < GPW; ++u) {
    if ((wave + 4 * u) * 64 >= T2_SLOTS) break;   // wave-uniform
    const int s0 = (wave + 4 * u) * 64 + 4 * (lane & 15);
    const int row = s0 / T2_XS, col = s0 - row * T2_XS;
    const int gy = y0 - 1 + row, gx = x0 - 4 + col;
    const bool ok = s0 < T2_SLOTS && gy >= 0 && gy < H && gx >= 0 && gx < W;
    const size_t off = ok ? (size_t)gy * W + gx : 0;
    floatx4 bfr[8], rfr[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      bfr[ks] = ok ? *reinterpret_cast<const floatx4 *>(inn + (size_t)ks * 4 * plane + off) : floatx4{0.f, 0.f, 0.f, 0.f};
      if constexpr (XFORM)
        rfr[ks] = (ok && resn) ? *reinterpret_cast<const floatx4 *>(resn + (size_t)ks * 4 * plane + off)
                               : floatx4{0.f, 0.f, 0.f, 0.f};
    }
    floatx4 d[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) d[p] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      if constexpr (XFORM) {   // groups outside the image were loaded as zeros and must stay zero: shift masked once
        const float shk = ok ? sh[ks] : 0.0f;
#pragma unroll
        for (int p = 0; p < 4; ++p) bfr[ks][p] = rfr[ks][p] + lrelu02(bfr[ks][p] * sc[ks] + shk);
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) d[p] = mfma16x16x4(a[ks], bfr[ks][p], d[p]);
    }
    if (s0 < T2_SLOTS) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tap = kc * 4 + r;
        if (tap < 9) *reinterpret_cast<floatx4 *>(P + tap * T2_SLOTS + s0) = floatx4{d[0][r], d[1][r], d[2][r], d[3][r]};
      }
    }
  }
  __syncthreads();
  const float b = bias ? bias[0] : 0.0f;
#pragma unroll
  for (int k = 0; k < T2_TY * T2_TX / 512; ++k) {   // two neighbouring outputs per thread and round
    const int idx = tid + 256 * k;
    const int oy = idx / (T2_TX / 2), ox = (idx % (T2_TX / 2)) * 2;
    if (y0 + oy >= H || x0 + ox >= W) continue;
    const float *pg = P + oy * T2_XS + ox + 3;
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const float *q = pg + (dy * 3 + dx) * T2_SLOTS + dy * T2_XS + dx;
        acc0 += q[0];
        acc1 += q[1];
      }
    const size_t o = (size_t)n * plane + (size_t)(y0 + oy) * W + x0 + ox;
    float2 res = make_float2(acc0 + b, acc1 + b);
    if (prior) {
      const float g = fx[n];
      const float2 pv = *reinterpret_cast<const float2 *>(prior + o);
      const float s0v = pv.x * g + res.x, s1v = pv.y * g + res.y;
      res = make_float2(relu_nan(s0v) / g, relu_nan(s1v) / g);
    }
    *reinterpret_cast<float2 *>(out + o) = res;
  }
}

}  // namespace mvsn

static int conv_to1_volume(const float *in, const float *weight, const float *bias, const float *in_stats,
                           const float *in_gamma, const float *in_beta, int n, int depth, int rows, int cols,
                           float *out, mvsn_stream_t stream) {
  using namespace mvsn;
  // tap GEMM on the matrix cores; slabs of planes so that even one chain fills the chip
  const int nty = (rows + T3_TY - 1) / T3_TY, ntx = (cols + T3_TX - 1) / T3_TX;
  int nslab = 1;
  while (nslab < 8 && (long)n * nty * ntx * nslab < 1024 && depth / (nslab * 2) >= 8) nslab *= 2;
  // a handful of chains on a small grid (batch 1: 2 x 1 tile): a plane is ~7 us of dependent load -> multiply -> LDS
  // round trips, so thinner slabs (down to one output plane, its two halo planes re-read) while workgroups < CUs
  while (nslab < depth && (long)n * nty * ntx * nslab * 2 <= device_cus()) nslab *= 2;
  const int zslab = (depth + nslab - 1) / nslab;
  const int nz = (depth + zslab - 1) / zslab;
  MVSN_REQUIRE(n <= 65535 && nz <= 65535, MVSN_E_TOOLARGE, "mvsn_conv_to1: grid");
  const size_t lds = (size_t)T3_LDS_FLOATS * sizeof(float);
  const bool whole = rows == T3_TY && cols == T3_TX;   // the plane is the tile
#define MVSN_TO1_3D_LAUNCH(XF_, WHOLE_)                                                                                \
  do {                                                                                                                 \
    static LdsOptIn opt;                                                                                               \
    if (int rc = ensure_lds(opt, (const void *)conv_to1_3d_mfma_kernel<XF_, WHOLE_>, lds, "mvsn_conv_to1")) return rc; \
    hipLaunchKernelGGL((conv_to1_3d_mfma_kernel<XF_, WHOLE_>), dim3(nty * ntx, nz, n), dim3(256), lds,                 \
                       (hipStream_t)stream, in, weight, bias, in_stats, in_gamma, in_beta, depth, rows, cols, ntx,     \
                       zslab, out);                                                                                    \
  } while (0)
  if (in_stats) {
    if (whole) MVSN_TO1_3D_LAUNCH(true, true);
    else MVSN_TO1_3D_LAUNCH(true, false);
  } else {
    in_gamma = in_beta = nullptr;
    if (whole) MVSN_TO1_3D_LAUNCH(false, true);
    else MVSN_TO1_3D_LAUNCH(false, false);
  }
#undef MVSN_TO1_3D_LAUNCH
  return mvsn::check_launch("mvsn_conv_to1(volume)");
}

extern "C" int mvsn_conv_to1_supported(int rows, int cols) { return (cols % 4 == 0 && rows > 0) ? 1 : 0; }

extern "C" int mvsn_conv_to1(const float *in, const float *weight, const float *bias, const float *prior,
                             const float *fx, int n, int depth, int rows, int cols, int kd, float *out,
                             mvsn_stream_t stream) {
  MVSN_REQUIRE(in && weight && out, MVSN_E_BADARG, "mvsn_conv_to1: null pointer");
  MVSN_REQUIRE(n > 0 && depth > 0 && rows > 0 && cols > 0 && (kd == 1 || kd == 3), MVSN_E_BADARG,
               "mvsn_conv_to1: bad sizes");
  MVSN_REQUIRE(cols % 4 == 0, MVSN_E_BADARG, "mvsn_conv_to1: cols must be a multiple of 4 (use mvsn_conv_forward)");
  MVSN_REQUIRE(!prior || (fx && depth == 1), MVSN_E_BADARG, "mvsn_conv_to1: refiner epilogue needs fx and 2-D input");
  if (kd == 3) {
    return conv_to1_volume(in, weight, bias, nullptr, nullptr, nullptr, n, depth, rows, cols, out, stream);
  } else {
    MVSN_REQUIRE(depth == 1, MVSN_E_BADARG, "mvsn_conv_to1: kd = 1 needs depth = 1");
    MVSN_REQUIRE(n <= 65535, MVSN_E_TOOLARGE, "mvsn_conv_to1: grid");
    const int nty = (rows + mvsn::T2_TY - 1) / mvsn::T2_TY;
    if (mvsn::to1_wide_tiles(n, rows, cols)) {
      const int ntx = (cols + 63) / 64;
      hipLaunchKernelGGL((mvsn::conv_to1_2d_mfma_kernel<false, 64>), dim3(nty * ntx, n), dim3(256), 0,
                         (hipStream_t)stream, in, weight, bias, (const float *)nullptr, (const float *)nullptr,
                         (const float *)nullptr, (const float *)nullptr, prior, fx, rows, cols, ntx, 0, out);
    } else {
      const int ntx = (cols + 31) / 32;
      hipLaunchKernelGGL((mvsn::conv_to1_2d_mfma_kernel<false, 32>), dim3(nty * ntx, n), dim3(256), 0,
                         (hipStream_t)stream, in, weight, bias, (const float *)nullptr, (const float *)nullptr,
                         (const float *)nullptr, (const float *)nullptr, prior, fx, rows, cols, ntx, 0, out);
    }
  }
  return mvsn::check_launch("mvsn_conv_to1");
}

extern "C" int mvsn_conv_to1_volume_norm(const float *in_raw, const float *in_stats, const float *in_gamma,
                                         const float *in_beta, const float *weight, const float *bias, int n, int depth,
                                         int rows, int cols, float *out, mvsn_stream_t stream) {
  MVSN_REQUIRE(in_raw && in_stats && in_gamma && in_beta && weight && out, MVSN_E_BADARG,
               "mvsn_conv_to1_volume_norm: null pointer");
  MVSN_REQUIRE(n > 0 && depth > 0 && rows > 0 && cols > 0, MVSN_E_BADARG, "mvsn_conv_to1_volume_norm: bad sizes");
  MVSN_REQUIRE(cols % 4 == 0, MVSN_E_BADARG, "mvsn_conv_to1_volume_norm: cols must be a multiple of 4");
  return conv_to1_volume(in_raw, weight, bias, in_stats, in_gamma, in_beta, n, depth, rows, cols, out, stream);
}

// stat_tiles == 0: `in_stats` is the finalised (N,4,2) array; > 0: the producer's records (N, stat_tiles, 4, 3), finalised
// by every workgroup of the launch itself (gn_stats_here)
extern "C" int mvsn_conv_to1_block(const float *in_raw, const float *in_stats, int stat_tiles, const float *in_gamma,
                                   const float *in_beta, const float *in_residual, const float *weight,
                                   const float *bias, const float *prior, const float *fx, int n, int rows, int cols,
                                   float *out, mvsn_stream_t stream) {
  MVSN_REQUIRE(in_raw && in_stats && in_gamma && in_beta && weight && out, MVSN_E_BADARG,
               "mvsn_conv_to1_block: null pointer");
  MVSN_REQUIRE(stat_tiles >= 0, MVSN_E_BADARG, "mvsn_conv_to1_block: stat_tiles");
  MVSN_REQUIRE(n > 0 && rows > 0 && cols > 0, MVSN_E_BADARG, "mvsn_conv_to1_block: bad sizes");
  MVSN_REQUIRE(cols % 4 == 0, MVSN_E_BADARG, "mvsn_conv_to1_block: cols must be a multiple of 4");
  MVSN_REQUIRE(!prior || fx, MVSN_E_BADARG, "mvsn_conv_to1_block: refiner epilogue needs fx");
  MVSN_REQUIRE(n <= 65535, MVSN_E_TOOLARGE, "mvsn_conv_to1_block: grid");
  const int nty = (rows + mvsn::T2_TY - 1) / mvsn::T2_TY;
  if (mvsn::to1_wide_tiles(n, rows, cols)) {
    const int ntx = (cols + 63) / 64;
    hipLaunchKernelGGL((mvsn::conv_to1_2d_mfma_kernel<true, 64>), dim3(nty * ntx, n), dim3(256), 0, (hipStream_t)stream,
                       in_raw, weight, bias, in_stats, in_gamma, in_beta, in_residual, prior, fx, rows, cols, ntx,
                       stat_tiles, out);
  } else {
    const int ntx = (cols + 31) / 32;
    hipLaunchKernelGGL((mvsn::conv_to1_2d_mfma_kernel<true, 32>), dim3(nty * ntx, n), dim3(256), 0, (hipStream_t)stream,
                       in_raw, weight, bias, in_stats, in_gamma, in_beta, in_residual, prior, fx, rows, cols, ntx,
                       stat_tiles, out);
  }
  return mvsn::check_launch("mvsn_conv_to1_block");
}
