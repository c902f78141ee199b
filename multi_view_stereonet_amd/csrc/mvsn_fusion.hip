// Depth-map fusion (see include/mvsn_hip.h: mvsn_fusion_*): the geometric-consistency filter every MVS pipeline runs
// after the network, and the back-projection of the kept pixels into one world-space point cloud.
//
// Four launches, one host read between the third and the fourth:
//   pair_setup_kernel   one thread per (reference, slot): the two 3x4 maps of the pair in fp64, rounded once to fp32
//                       (P_rs = K_s T_r_in_s K_r^-1 applied to (x d, y d, d, 1), and the reverse P_sr), plus per
//                       reference the map of a pixel into the world (T_r_in_world K_r^-1)
//   consistency_kernel  grid (pixel blocks, R): FU_PIX consecutive pixels per thread, every slot's map from LDS; per
//                       pixel and slot: project, bilinear-gather the neighbour's depth (four taps through L2/MALL),
//                       project back, test; writes the fused depth (0 = not kept), the count map and one kept-pixel
//                       count per workgroup
//   geom_scan_kernel    one workgroup: exclusive prefix of those counts in a fixed order, and the total (mvsn_geom.h)
//   emit_kernel         the consistency kernel's blocking again: kept pixels ranked inside the workgroup (block_rank
//                       of mvsn_geom.h), written at the workgroup's scanned offset
// No atomics anywhere: every output is a deterministic function of the inputs.  The bottom row of every K is taken to be
// (0, 0, 1) (not checked on the device): the third row of P_rs then yields the neighbour's camera z itself.
#include "mvsn_common.h"
#include "mvsn_geom.h"

namespace mvsn {

constexpr int FU_THREADS = 256;
constexpr int FU_PIX = 4;                               // consecutive pixels per thread: one 16-byte depth load
constexpr int FU_BLOCK_PIX = FU_THREADS * FU_PIX;       // pixels per workgroup
constexpr int FU_MAX_SLOTS = 32;
constexpr int FU_MAP = 24;                              // floats per slot: P_rs (3x4) then P_sr (3x4)

// byte offsets of the workspace sections (each 256-byte aligned)
struct FusionLayout {
  size_t maps, world, counts, offsets, bytes;
  long blocks;   // pixel blocks per reference view
};

inline FusionLayout fusion_layout(int n_ref, int n_slots, int rows, int cols) {
  FusionLayout l;
  const long P = (long)rows * cols;
  l.blocks = (P + FU_BLOCK_PIX - 1) / FU_BLOCK_PIX;
  l.maps = 0;
  l.world = align256(l.maps + sizeof(float) * FU_MAP * (size_t)n_ref * n_slots);
  l.counts = align256(l.world + sizeof(float) * 12 * (size_t)n_ref);
  l.offsets = align256(l.counts + sizeof(int) * (size_t)n_ref * l.blocks);
  l.bytes = align256(l.offsets + sizeof(int64_t) * (size_t)n_ref * l.blocks);
  return l;
}

// top-left 3x3 of a row-major 4x4, inverted in fp64.  Not mvsn_geom.h's inv3_d: this file is compiled with contraction
// allowed, these products fuse, and the fp32 maps pair_setup_kernel rounds from them are pinned bit for bit by the tests.
__device__ inline void inv3_fused_d(const float *K, double *o) {
  const double a = K[0], b = K[1], c = K[2], d = K[4], e = K[5], f = K[6], g = K[8], h = K[9], i = K[10];
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const double det = a * A + b * B + c * C, r = 1.0 / det;
  o[0] = A * r, o[1] = -(b * i - c * h) * r, o[2] = (b * f - c * e) * r;
  o[3] = B * r, o[4] = (a * i - c * g) * r, o[5] = -(a * f - c * d) * r;
  o[6] = C * r, o[7] = -(a * h - b * g) * r, o[8] = (a * e - b * d) * r;
}

// inverse of an affine pose [A t; 0 0 0 1] in fp64: [A^-1, -A^-1 t] (3x4 rows)
__device__ inline void pose_inv_d(const float *T, double *o) {
  double Ai[9];
  inv3_fused_d(T, Ai);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[i * 4 + j] = Ai[i * 3 + j];
    o[i * 4 + 3] = -(Ai[i * 3 + 0] * T[3] + Ai[i * 3 + 1] * T[7] + Ai[i * 3 + 2] * T[11]);
  }
}

// out (3x4) = Ka (3x3, fp32 top-left of a 4x4) * [A (3x4) composed with B (3x4 pose)] * blockdiag(Kinv, 1); Ka NULL = I
__device__ inline void pair_map(const float *Ka, const double *A, const float *B, const double *Kinv, float *out) {
  double AB[12];   // A * [B; 0 0 0 1]
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = j == 3 ? A[i * 4 + 3] : 0.0;
      for (int k = 0; k < 3; ++k) s += A[i * 4 + k] * (double)B[k * 4 + j];
      AB[i * 4 + j] = s;
    }
  double KAB[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += (Ka ? (double)Ka[i * 4 + k] : (double)(i == k)) * AB[k * 4 + j];
      KAB[i * 4 + j] = s;
    }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += KAB[i * 4 + k] * Kinv[k * 3 + j];
      out[i * 4 + j] = (float)s;
    }
    out[i * 4 + 3] = (float)KAB[i * 4 + 3];
  }
}

__global__ __launch_bounds__(64) void pair_setup_kernel(const float *__restrict__ K, const float *__restrict__ T,
                                                        const int *__restrict__ ref_views,
                                                        const int *__restrict__ neighbours, int n_views, int n_ref,
                                                        int n_slots, float *__restrict__ maps,
                                                        float *__restrict__ world) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_ref * (n_slots + 1)) return;
  const int r = t / (n_slots + 1), j = t % (n_slots + 1);
  const int rv = ref_views[r];
  if (rv < 0 || rv >= n_views) return;            // (validated on the host; never read out of bounds)
  const float *Kr = K + (size_t)rv * 16, *Tr = T + (size_t)rv * 16;
  double Krinv[9];
  inv3_fused_d(Kr, Krinv);
  if (j == n_slots) {                               // pixel (x f, y f, f, 1) of the reference -> world
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    pair_map(nullptr, I, Tr, Krinv, world + (size_t)r * 12);
    return;
  }
  const int s = neighbours[(size_t)r * n_slots + j];
  if (s < 0 || s >= n_views) return;
  const float *Ks = K + (size_t)s * 16, *Ts = T + (size_t)s * 16;
  double Ksinv[9], Trinv[12], Tsinv[12];
  inv3_fused_d(Ks, Ksinv);
  pose_inv_d(Tr, Trinv);
  pose_inv_d(Ts, Tsinv);
  float *m = maps + ((size_t)r * n_slots + j) * FU_MAP;
  pair_map(Ks, Tsinv, Tr, Krinv, m);           // T_r_in_s = T_s_in_world^-1 T_r_in_world
  pair_map(Kr, Trinv, Ts, Ksinv, m + 12);      // T_s_in_r = T_r_in_world^-1 T_s_in_world
}

// FU_PIX consecutive values at base[p0..]: one wide load where the address allows it, a scalar tail otherwise
__device__ __forceinline__ void load_pix(const float *base, long p0, long P, float *v) {
  const float *q = base + p0;
  if (p0 + FU_PIX <= P && ((uintptr_t)q & 15) == 0) {
    const float4 w = *reinterpret_cast<const float4 *>(q);
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else {
#pragma unroll
    for (int k = 0; k < FU_PIX; ++k) v[k] = p0 + k < P ? q[k] : 0.0f;
  }
}

__device__ __forceinline__ void load_pix(const uint8_t *base, long p0, long P, bool *v) {
  const uint8_t *q = base + p0;
  if (p0 + FU_PIX <= P && ((uintptr_t)q & 3) == 0) {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(q);
#pragma unroll
    for (int k = 0; k < FU_PIX; ++k) v[k] = ((w >> (8 * k)) & 0xff) != 0;
  } else {
#pragma unroll
    for (int k = 0; k < FU_PIX; ++k) v[k] = p0 + k < P && q[k] != 0;
  }
}

__global__ __launch_bounds__(FU_THREADS) void consistency_kernel(
    const float *__restrict__ depth, const uint8_t *__restrict__ valid, const int *__restrict__ ref_views,
    const int *__restrict__ neighbours, const float *__restrict__ maps, int n_views, int n_slots, int rows, int cols,
    float max_reproj_px, float max_rel_depth, int min_consistent, float *__restrict__ fused,
    uint8_t *__restrict__ count_map, int *__restrict__ block_counts) {
  __shared__ float smap[FU_MAX_SLOTS * FU_MAP];
  __shared__ int snb[FU_MAX_SLOTS];
  __shared__ int swave[FU_THREADS / 64];
  const int r = blockIdx.y;
  const long P = (long)rows * cols;
  const int rv = ref_views[r];
  const bool ref_ok = rv >= 0 && rv < n_views;
  for (int i = threadIdx.x; i < n_slots * FU_MAP; i += FU_THREADS) smap[i] = maps[(size_t)r * n_slots * FU_MAP + i];
  if (threadIdx.x < n_slots) {
    const int s = neighbours[(size_t)r * n_slots + threadIdx.x];
    snb[threadIdx.x] = ref_ok && s >= 0 && s < n_views ? s : -1;
  }
  __syncthreads();

  const long p0 = ((long)blockIdx.x * FU_THREADS + threadIdx.x) * FU_PIX;
  float d[FU_PIX];
  bool cand[FU_PIX];
  if (ref_ok) {
    load_pix(depth + (int64_t)rv * P, p0, P, d);
    if (valid) load_pix(valid + (int64_t)rv * P, p0, P, cand);
  }
#pragma unroll
  for (int k = 0; k < FU_PIX; ++k) {
    if (!ref_ok) d[k] = 0.0f;
    cand[k] = (valid && ref_ok ? cand[k] : true) && p0 + k < P && d[k] > 0.0f;
  }
  float xd[FU_PIX], yd[FU_PIX], px[FU_PIX], py[FU_PIX], sum[FU_PIX];
  int cnt[FU_PIX];
#pragma unroll
  for (int k = 0; k < FU_PIX; ++k) {
    const long p = p0 + k;
    px[k] = (float)(p % cols), py[k] = (float)(p / cols);
    xd[k] = px[k] * d[k], yd[k] = py[k] * d[k];
    sum[k] = 0.0f, cnt[k] = 0;
  }
  const float thr2 = max_reproj_px * max_reproj_px;
  const float fcols = (float)(cols - 1), frows = (float)(rows - 1);

  for (int j = 0; j < n_slots; ++j) {                // slot order: the sums are bitwise reproducible
    const int s = snb[j];
    if (s < 0) continue;                             // (uniform over the workgroup)
    const float *A = smap + j * FU_MAP, *B = A + 12;
    const float *ds = depth + (int64_t)s * P;
    const uint8_t *vs = valid ? valid + (int64_t)s * P : nullptr;
    // all FU_PIX gathers are issued before any is used: the taps' addresses are clamped into the image, and whether
    // the slot may count at all is kept in `ok`
    float u[FU_PIX], v[FU_PIX], t00[FU_PIX], t01[FU_PIX], t10[FU_PIX], t11[FU_PIX];
    bool ok[FU_PIX];
#pragma unroll
    for (int k = 0; k < FU_PIX; ++k) {
      const float c0 = A[0] * xd[k] + A[1] * yd[k] + A[2] * d[k] + A[3];
      const float c1 = A[4] * xd[k] + A[5] * yd[k] + A[6] * d[k] + A[7];
      const float c2 = A[8] * xd[k] + A[9] * yd[k] + A[10] * d[k] + A[11];   // the neighbour's camera z
      u[k] = c0 / c2, v[k] = c1 / c2;
      const float fx0 = floorf(u[k]), fy0 = floorf(v[k]);
      // all four taps inside the image (a NaN fails every comparison)
      ok[k] = cand[k] && c2 > 0.0f && fx0 >= 0.0f && fx0 + 1.0f <= fcols && fy0 >= 0.0f && fy0 + 1.0f <= frows;
      const int x0 = ok[k] ? (int)fx0 : 0, y0 = ok[k] ? (int)fy0 : 0;
      const int x1 = min(x0 + 1, cols - 1), y1 = min(y0 + 1, rows - 1);
      const long i00 = (long)y0 * cols + x0, i01 = (long)y0 * cols + x1;
      const long i10 = (long)y1 * cols + x0, i11 = (long)y1 * cols + x1;
      t00[k] = ds[i00], t01[k] = ds[i01], t10[k] = ds[i10], t11[k] = ds[i11];
      if (vs) ok[k] = ok[k] && vs[i00] && vs[i01] && vs[i10] && vs[i11];
    }
#pragma unroll
    for (int k = 0; k < FU_PIX; ++k) {
      const float ax = u[k] - floorf(u[k]), ay = v[k] - floorf(v[k]);
      const float e = (1.0f - ax) * (1.0f - ay) * t00[k] + ax * (1.0f - ay) * t01[k] + (1.0f - ax) * ay * t10[k] +
                      ax * ay * t11[k];
      const bool taps = t00[k] > 0.0f && t01[k] > 0.0f && t10[k] > 0.0f && t11[k] > 0.0f;
      const float ue = u[k] * e, ve = v[k] * e;
      const float q0 = B[0] * ue + B[1] * ve + B[2] * e + B[3];
      const float q1 = B[4] * ue + B[5] * ve + B[6] * e + B[7];
      const float q2 = B[8] * ue + B[9] * ve + B[10] * e + B[11];            // Y_r.z
      const float dx = q0 / q2 - px[k], dy = q1 / q2 - py[k];
      if (ok[k] && taps && q2 > 0.0f && dx * dx + dy * dy < thr2 && fabsf(q2 - d[k]) < max_rel_depth * d[k]) {
        cnt[k] += 1;
        sum[k] += q2;
      }
    }
  }

  float f[FU_PIX];
  uint32_t packed = 0;
  int kept = 0;
#pragma unroll
  for (int k = 0; k < FU_PIX; ++k) {
    const bool keep = cand[k] && cnt[k] >= min_consistent;
    f[k] = keep ? (d[k] + sum[k]) / (float)(cnt[k] + 1) : 0.0f;
    kept += keep;
    packed |= (uint32_t)cnt[k] << (8 * k);
  }
  {
    float *fo = fused + (int64_t)r * P + p0;
    uint8_t *co = count_map + (int64_t)r * P + p0;
    if (p0 + FU_PIX <= P && ((uintptr_t)fo & 15) == 0 && ((uintptr_t)co & 3) == 0) {
      *reinterpret_cast<float4 *>(fo) = make_float4(f[0], f[1], f[2], f[3]);
      *reinterpret_cast<uint32_t *>(co) = packed;
    } else {
#pragma unroll
      for (int k = 0; k < FU_PIX; ++k)
        if (p0 + k < P) fo[k] = f[k], co[k] = (uint8_t)cnt[k];
    }
  }
  kept = block_sum_256(kept, swave);
  if (threadIdx.x == 0) block_counts[(size_t)r * gridDim.x + blockIdx.x] = kept;
}

__global__ __launch_bounds__(FU_THREADS) void emit_kernel(const float *__restrict__ fused,
                                                          const float *__restrict__ images,
                                                          const int *__restrict__ ref_views,
                                                          const float *__restrict__ world,
                                                          const int64_t *__restrict__ offsets, int rows, int cols,
                                                          long capacity, float *__restrict__ points,
                                                          uint8_t *__restrict__ colors, int *__restrict__ view,
                                                          int *__restrict__ pixel) {
  __shared__ int swave[FU_THREADS / 64];
  __shared__ float sw[12];
  const int r = blockIdx.y;
  const long P = (long)rows * cols;
  if (threadIdx.x < 12) sw[threadIdx.x] = world[(size_t)r * 12 + threadIdx.x];
  const long p0 = ((long)blockIdx.x * FU_THREADS + threadIdx.x) * FU_PIX;
  float f[FU_PIX];
  load_pix(fused + (int64_t)r * P, p0, P, f);
  bool kept[FU_PIX];
#pragma unroll
  for (int k = 0; k < FU_PIX; ++k) kept[k] = p0 + k < P && f[k] > 0.0f;
  // rank among the workgroup's kept pixels, then the pixels of this thread before each one (the barrier inside also
  // publishes sw)
  int64_t idx = offsets[(size_t)r * gridDim.x + blockIdx.x] + block_rank(kept, swave);
  const int rv = ref_views[r];
#pragma unroll
  for (int k = 0; k < FU_PIX; ++k) {
    if (!kept[k]) continue;
    if (idx < capacity) {                           // (capacity = the scanned total: always true)
      const long p = p0 + k;
      const float x = (float)(p % cols) * f[k], y = (float)(p / cols) * f[k];
      points[idx * 3 + 0] = sw[0] * x + sw[1] * y + sw[2] * f[k] + sw[3];
      points[idx * 3 + 1] = sw[4] * x + sw[5] * y + sw[6] * f[k] + sw[7];
      points[idx * 3 + 2] = sw[8] * x + sw[9] * y + sw[10] * f[k] + sw[11];
      if (colors) {
        const float *im = images + (int64_t)rv * 3 * P + p;
#pragma unroll
        for (int c = 0; c < 3; ++c) {   // (c + 1) * 127.5 in fp64, rint with ties to even: numpy's float64 bits
          const double q = rint(((double)im[(int64_t)c * P] + 1.0) * 127.5);
          colors[idx * 3 + c] = (uint8_t)(q < 0.0 ? 0.0 : q > 255.0 ? 255.0 : q);
        }
      }
      view[idx] = rv;
      pixel[idx] = (int)p;
    }
    ++idx;
  }
}

}  // namespace mvsn

extern "C" size_t mvsn_fusion_workspace_bytes(int n_ref, int n_slots, int rows, int cols) {
  if (n_ref <= 0 || n_slots <= 0 || n_slots > mvsn::FU_MAX_SLOTS || rows <= 0 || cols <= 0) return 0;
  return mvsn::fusion_layout(n_ref, n_slots, rows, cols).bytes;
}

extern "C" int mvsn_fusion_consistency(const float *depth, const uint8_t *valid, const float *K,
                                       const float *T_cam_in_world, const int *ref_views, const int *neighbours,
                                       int n_views, int n_ref, int n_slots, int rows, int cols, float max_reproj_px,
                                       float max_rel_depth, int min_consistent, float *fused_depth, uint8_t *count,
                                       int64_t *total, void *workspace, size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(depth && K && T_cam_in_world && ref_views && neighbours && fused_depth && count && total, MVSN_E_BADARG,
               "mvsn_fusion_consistency: null pointer");
  MVSN_REQUIRE(n_views > 0 && n_ref > 0 && n_ref <= 65535 && rows > 0 && cols > 0, MVSN_E_BADARG,
               "mvsn_fusion_consistency: bad sizes (views %d, references %d, %d x %d)", n_views, n_ref, rows, cols);
  MVSN_REQUIRE(n_slots >= 1 && n_slots <= FU_MAX_SLOTS, MVSN_E_BADARG,
               "mvsn_fusion_consistency: %d neighbour slots (1..%d)", n_slots, FU_MAX_SLOTS);
  MVSN_REQUIRE(max_reproj_px >= 0.0f && max_rel_depth >= 0.0f && min_consistent >= 0, MVSN_E_BADARG,
               "mvsn_fusion_consistency: negative threshold");
  MVSN_REQUIRE((long)rows * cols <= 0x7fffffffL, MVSN_E_TOOLARGE, "mvsn_fusion_consistency: %d x %d pixels", rows, cols);
  const FusionLayout l = fusion_layout(n_ref, n_slots, rows, cols);
  MVSN_REQUIRE(workspace && workspace_bytes >= l.bytes, MVSN_E_WORKSPACE,
               "mvsn_fusion_consistency: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
  MVSN_REQUIRE(l.blocks <= 0x7fffffffL, MVSN_E_TOOLARGE, "mvsn_fusion_consistency: image too large");
  char *ws = (char *)workspace;
  float *maps = (float *)(ws + l.maps), *world = (float *)(ws + l.world);
  int *counts = (int *)(ws + l.counts);
  int64_t *offsets = (int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  const int setup_threads = n_ref * (n_slots + 1);
  hipLaunchKernelGGL(pair_setup_kernel, dim3((setup_threads + 63) / 64), dim3(64), 0, st, K, T_cam_in_world, ref_views,
                     neighbours, n_views, n_ref, n_slots, maps, world);
  if (int e = check_launch("mvsn_fusion_consistency: pair set-up")) return e;
  hipLaunchKernelGGL(consistency_kernel, dim3((unsigned)l.blocks, n_ref), dim3(FU_THREADS), 0, st, depth, valid,
                     ref_views, neighbours, maps, n_views, n_slots, rows, cols, max_reproj_px, max_rel_depth,
                     min_consistent, fused_depth, count, counts);
  if (int e = check_launch("mvsn_fusion_consistency: consistency")) return e;
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)counts,
                     (long)n_ref * l.blocks, offsets, total);
  return check_launch("mvsn_fusion_consistency: scan");
}

extern "C" int mvsn_fusion_emit(const float *fused_depth, const float *images, const int *ref_views, int n_ref,
                                int rows, int cols, int n_slots, const void *workspace, size_t workspace_bytes,
                                long capacity, float *points, uint8_t *colors, int *view, int *pixel,
                                mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(fused_depth && ref_views && workspace, MVSN_E_BADARG, "mvsn_fusion_emit: null pointer");
  MVSN_REQUIRE(!colors || images, MVSN_E_BADARG, "mvsn_fusion_emit: colours without images");
  MVSN_REQUIRE(n_ref > 0 && n_ref <= 65535 && rows > 0 && cols > 0 && n_slots >= 1 && n_slots <= FU_MAX_SLOTS &&
                   capacity >= 0,
               MVSN_E_BADARG, "mvsn_fusion_emit: bad sizes");
  if (capacity == 0) return 0;                      // nothing kept: nothing to launch
  MVSN_REQUIRE(points && view && pixel, MVSN_E_BADARG, "mvsn_fusion_emit: null output");
  const FusionLayout l = fusion_layout(n_ref, n_slots, rows, cols);
  MVSN_REQUIRE(workspace_bytes >= l.bytes, MVSN_E_WORKSPACE, "mvsn_fusion_emit: workspace of %zu bytes, %zu needed",
               workspace_bytes, l.bytes);
  const char *ws = (const char *)workspace;
  hipLaunchKernelGGL(emit_kernel, dim3((unsigned)l.blocks, n_ref), dim3(FU_THREADS), 0, (hipStream_t)stream,
                     fused_depth, images, ref_views, (const float *)(ws + l.world), (const int64_t *)(ws + l.offsets),
                     rows, cols, capacity, points, colors, view, pixel);
  return check_launch("mvsn_fusion_emit");
}
