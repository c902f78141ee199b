// Oriented normals from depth maps (see include/mvsn_hip.h: mvsn_depth_normals, mvsn_normals_gather, mvsn_voxel_normals;
// the semantics are DESIGN.md section 13): the normal of every pixel from differences of its back-projected neighbours,
// facing the camera that saw it; the normals of a fused cloud's points read out of those maps; the mean direction of
// the points of a voxel.
//
//   depth_normals_kernel     grid (pixel blocks, V): section 10's blocking, NM_PIX consecutive pixels per thread.  A
//                            5-point stencil: the thread's own pixels and the two beside them, the rows above and below.
//                            Every load is issued before the first use, at an address clamped into the view, with an
//                            in-range flag kept beside it: never a read outside the maps.  K^-1 (fp64, rounded once) and R
//                            are formed by the workgroup's first lanes into LDS while those loads are in flight.
//   gather_kernel<3>         mvsn_geom.h: one thread per point, the three planes of the map at (view, pixel)
//   voxel_normals_*          zero the accumulators / one thread per point: three no-return 64-bit integer atomicAdd of the
//                            components quantised to 2^-20 / one thread per row: the direction of the sum, in fp64
// As in mvsn_voxel.hip every atomic is an integer sum, so every output is a deterministic function of the inputs whatever
// order the points arrive in; no float atomics, no sort, no loop that waits.
//
// Contraction is off for the whole file: the usable-neighbour test |d' - d| <= step * d is three fp32 operations that the
// numpy restatement (tests/normals_reference.py) repeats bit for bit, and the fp64 finalise is one rounding per step.
// Where a fused multiply-add is wanted it is written as fmaf.
#pragma clang fp contract(off)
#include "mvsn_common.h"
#include "mvsn_geom.h"

namespace mvsn {

constexpr int NM_THREADS = 256;
constexpr int NM_PIX = 4;                               // consecutive pixels per thread: one 16-byte depth load
constexpr int NM_BLOCK_PIX = NM_THREADS * NM_PIX;       // pixels per workgroup
constexpr float NM_QUANT = 1048576.0f;                  // 2^20: a unit component is 2^20 steps

// entry `e` of mvsn_geom.h's inv3_d, one rounding per step (mvsn_fusion.hip's own inverse has the same formulas but
// is compiled with contraction allowed: its bits can differ)
__device__ inline double normals_inv3_entry(const float *K, int e) {
  double o[9];
  inv3_d(K, o);
  double v = o[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) v = e == k ? o[k] : v;    // (a select chain: no runtime-indexed array)
  return v;
}

// The wide accesses below are accesses of a native vector (floatx4), not of the float4 struct: a struct copy is taken
// apart into four scalar accesses, the optimiser then finds one of them in common with the scalar branch and moves it
// (for a store, the division behind it too) out of both branches, and what is left is put together again as a 12-byte
// access plus a 4-byte one.
// NM_PIX consecutive floats at base[i0 ..] of a view of P values; i0 may lie outside [0, P): one wide load where all
// four lie inside and the address allows it, scalar loads at addresses clamped into the view otherwise (the caller
// keeps the in-range flags)
__device__ __forceinline__ void normals_load(const float *base, long i0, long P, float *v) {
  const float *q = base + i0;
  if (i0 >= 0 && i0 + NM_PIX <= P && ((uintptr_t)q & 15) == 0) {
    const floatx4 w = *reinterpret_cast<const floatx4 *>(q);
    v[0] = w[0], v[1] = w[1], v[2] = w[2], v[3] = w[3];
  } else {
#pragma unroll
    for (int k = 0; k < NM_PIX; ++k) v[k] = base[min(max(i0 + k, 0L), P - 1)];
  }
}

__device__ __forceinline__ void normals_load(const uint8_t *base, long i0, long P, bool *v) {
  const uint8_t *q = base + i0;
  if (i0 >= 0 && i0 + NM_PIX <= P && ((uintptr_t)q & 3) == 0) {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(q);
#pragma unroll
    for (int k = 0; k < NM_PIX; ++k) v[k] = ((w >> (8 * k)) & 0xff) != 0;
  } else {
#pragma unroll
    for (int k = 0; k < NM_PIX; ++k) v[k] = base[min(max(i0 + k, 0L), P - 1)] != 0;
  }
}

// |dn - d| <= step * d: subtract, multiply, compare.  A NaN difference fails the comparison by itself; an infinite one
// would pass it against an infinite bound (step = inf, or an infinite d), so it is refused by a comparison of its own:
// a non-finite difference never counts.
__device__ __forceinline__ bool normals_step_ok(float dn, float d, float step) {
  const float diff = dn - d;
  const float bound = step * d;
  return fabsf(diff) <= bound && fabsf(diff) <= 3.4028234e38f;
}

__global__ __launch_bounds__(NM_THREADS) void depth_normals_kernel(const float *__restrict__ depth,
                                                                   const uint8_t *__restrict__ valid,
                                                                   const float *__restrict__ K,
                                                                   const float *__restrict__ T, int rows, int cols,
                                                                   float max_rel_step, float *__restrict__ normals) {
  __shared__ float scam[18];                             // K^-1 (9), R (9)
  const int v = blockIdx.y;
  const long P = (long)rows * cols;
  const long p0 = ((long)blockIdx.x * NM_THREADS + threadIdx.x) * NM_PIX;
  const float *dv = depth + (int64_t)v * P;
  const uint8_t *vv = valid ? valid + (int64_t)v * P : nullptr;

  // the taps: the row of the thread's pixels with one pixel either side (dc[k + 1] is pixel p0 + k), the rows above and
  // below.  Whether an index lies inside the view, and whether it is the pixel's neighbour in the IMAGE, is decided below.
  float dc[NM_PIX + 2], du[NM_PIX], dd[NM_PIX];
  bool vc[NM_PIX + 2], vu[NM_PIX], vd[NM_PIX];
  normals_load(dv, p0, P, dc + 1);
  dc[0] = dv[min(max(p0 - 1, 0L), P - 1)];
  dc[NM_PIX + 1] = dv[min(p0 + NM_PIX, P - 1)];
  normals_load(dv, p0 - cols, P, du);
  normals_load(dv, p0 + cols, P, dd);
  if (vv) {
    normals_load(vv, p0, P, vc + 1);
    vc[0] = vv[min(max(p0 - 1, 0L), P - 1)] != 0;
    vc[NM_PIX + 1] = vv[min(p0 + NM_PIX, P - 1)] != 0;
    normals_load(vv, p0 - cols, P, vu);
    normals_load(vv, p0 + cols, P, vd);
  }

  if (threadIdx.x < 9) {
    scam[threadIdx.x] = (float)normals_inv3_entry(K + (size_t)v * 16, threadIdx.x);
  } else if (threadIdx.x < 18) {
    const int e = threadIdx.x - 9;
    scam[threadIdx.x] = T ? T[(size_t)v * 16 + (e / 3) * 4 + e % 3] : (e % 4 == 0 ? 1.0f : 0.0f);
  }
  __syncthreads();
  float ki[9], R[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) ki[e] = scam[e], R[e] = scam[9 + e];

  // usable: inside the view, depth > 0 (a NaN is not), valid
  bool uc[NM_PIX + 2], uu[NM_PIX], ud[NM_PIX];
#pragma unroll
  for (int k = 0; k < NM_PIX + 2; ++k) {
    const long p = p0 - 1 + k;
    uc[k] = p >= 0 && p < P && dc[k] > 0.0f && (!vv || vc[k]);
  }
#pragma unroll
  for (int k = 0; k < NM_PIX; ++k) {
    const long p = p0 + k;
    uu[k] = p - cols >= 0 && p - cols < P && du[k] > 0.0f && (!vv || vu[k]);
    ud[k] = p + cols < P && dd[k] > 0.0f && (!vv || vd[k]);
  }

  float n[3][NM_PIX];
#pragma unroll
  for (int k = 0; k < NM_PIX; ++k) {
    const long p = min(p0 + k, P - 1);                  // (a pixel past the end is computed and not stored)
    const int y = (int)((unsigned)p / (unsigned)cols), x = (int)p - y * cols;      // (P < 2^31: 32-bit division)
    const float fx = (float)x, fy = (float)y, d = dc[k + 1];
    const bool left = uc[k + 1] && x > 0 && uc[k] && normals_step_ok(dc[k], d, max_rel_step);
    const bool right = uc[k + 1] && x < cols - 1 && uc[k + 2] && normals_step_ok(dc[k + 2], d, max_rel_step);
    const bool up = uc[k + 1] && y > 0 && uu[k] && normals_step_ok(du[k], d, max_rel_step);
    const bool down = uc[k + 1] && y < rows - 1 && ud[k] && normals_step_ok(dd[k], d, max_rel_step);
    // X = d * K^-1 (x, y, 1) at the pixel and at the neighbours that count; the pixel itself stands in for one that
    // does not, which turns the central difference into the one-sided one
    float t[2][3];                                      // t[0] = t_u (horizontal), t[1] = t_v (vertical)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float rc = fmaf(ki[3 * a], fx, fmaf(ki[3 * a + 1], fy, ki[3 * a + 2]));
      const float rl = fmaf(ki[3 * a], fx - 1.0f, fmaf(ki[3 * a + 1], fy, ki[3 * a + 2]));
      const float rr = fmaf(ki[3 * a], fx + 1.0f, fmaf(ki[3 * a + 1], fy, ki[3 * a + 2]));
      const float ru = fmaf(ki[3 * a], fx, fmaf(ki[3 * a + 1], fy - 1.0f, ki[3 * a + 2]));
      const float rd = fmaf(ki[3 * a], fx, fmaf(ki[3 * a + 1], fy + 1.0f, ki[3 * a + 2]));
      const float Xc = d * rc;
      t[0][a] = (right ? dc[k + 2] * rr : Xc) - (left ? dc[k] * rl : Xc);
      t[1][a] = (down ? dd[k] * rd : Xc) - (up ? du[k] * ru : Xc);
    }
    // c = t_v x t_u: towards the camera for x right, y down, z forward
    float c[3];
    c[0] = t[1][1] * t[0][2] - t[1][2] * t[0][1];
    c[1] = t[1][2] * t[0][0] - t[1][0] * t[0][2];
    c[2] = t[1][0] * t[0][1] - t[1][1] * t[0][0];
    // |c| zero or not finite <=> its largest component is (a NaN fails the last test); then scale by a power of two so
    // that the largest component lies in [1, 2): exact, and the squares neither overflow nor vanish
    const float big = fmaxf(fabsf(c[0]), fmaxf(fabsf(c[1]), fabsf(c[2])));
    bool defined = (left || right) && (up || down) && big > 0.0f && big <= 3.4028234e38f &&
                   c[0] == c[0] && c[1] == c[1] && c[2] == c[2];
    int ex;
    (void)frexpf(defined ? big : 1.0f, &ex);
    const float s0 = ldexpf(c[0], 1 - ex), s1 = ldexpf(c[1], 1 - ex), s2 = ldexpf(c[2], 1 - ex);
    float w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = fmaf(R[3 * a], s0, fmaf(R[3 * a + 1], s1, R[3 * a + 2] * s2));
    const float len = sqrtf(fmaf(w[0], w[0], fmaf(w[1], w[1], w[2] * w[2])));
    defined = defined && len > 0.0f && len <= 3.4028234e38f;      // (R is assumed to be a rotation; all zeros is not)
#pragma unroll
    for (int a = 0; a < 3; ++a) n[a][k] = defined ? w[a] / len : 0.0f;
  }

  // three planar stores per thread, 16 bytes each where the address allows it
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float *o = normals + ((int64_t)v * 3 + a) * P + p0;
    if (p0 + NM_PIX <= P && ((uintptr_t)o & 15) == 0) {
      *reinterpret_cast<floatx4 *>(o) = floatx4{n[a][0], n[a][1], n[a][2], n[a][3]};
    } else {
#pragma unroll
      for (int k = 0; k < NM_PIX; ++k)
        if (p0 + k < P) o[k] = n[a][k];
    }
  }
}

__global__ __launch_bounds__(256) void voxel_normals_zero_kernel(unsigned long long *__restrict__ accum, long words) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < words) accum[i] = 0ull;
}

__global__ __launch_bounds__(256) void voxel_normals_accumulate_kernel(const float *__restrict__ normals,
                                                                       const int64_t *__restrict__ inverse, long n,
                                                                       long m, unsigned long long *__restrict__ accum) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = inverse[i];
  if (r < 0 || r >= m) return;                        // dropped by the merge (or not a row): never dereferenced
  long long q[3];
  bool finite = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float c = normals[(size_t)i * 3 + a];
    finite = finite && fabsf(c) <= 3.4028234e38f;     // (a NaN compares false)
    const float clamped = fminf(fmaxf(c, -1.0f), 1.0f);
    const float scaled = clamped * NM_QUANT;          // exact: a power of two, no overflow
    q[a] = (long long)rintf(finite ? scaled : 0.0f);  // half to even
  }
  if (!finite || (q[0] == 0 && q[1] == 0 && q[2] == 0)) return;
  unsigned long long *a = accum + (size_t)r * 3;      // two's complement: the unsigned sum is the signed one
  atomicAdd(a + 0, (unsigned long long)q[0]);
  atomicAdd(a + 1, (unsigned long long)q[1]);
  atomicAdd(a + 2, (unsigned long long)q[2]);
}

__global__ __launch_bounds__(256) void voxel_normals_finalise_kernel(const unsigned long long *__restrict__ accum,
                                                                     long m, float *__restrict__ out) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const double sx = (double)(long long)accum[(size_t)r * 3 + 0], sy = (double)(long long)accum[(size_t)r * 3 + 1],
               sz = (double)(long long)accum[(size_t)r * 3 + 2];
  const bool zero = sx == 0.0 && sy == 0.0 && sz == 0.0;
  // |S| <= 2^51 per component: the conversions are exact and the squares far from overflow; one rounding per step
  const double len = sqrt(sx * sx + sy * sy + sz * sz);
  out[(size_t)r * 3 + 0] = zero ? 0.0f : (float)(sx / len);
  out[(size_t)r * 3 + 1] = zero ? 0.0f : (float)(sy / len);
  out[(size_t)r * 3 + 2] = zero ? 0.0f : (float)(sz / len);
}

}  // namespace mvsn

extern "C" int mvsn_depth_normals(const float *depth, const uint8_t *valid, const float *K, const float *T_cam_in_world,
                                  int n_views, int rows, int cols, float max_rel_step, float *normals,
                                  mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(depth && K && normals, MVSN_E_BADARG, "mvsn_depth_normals: null pointer");
  MVSN_REQUIRE(n_views > 0 && rows > 0 && cols > 0, MVSN_E_BADARG, "mvsn_depth_normals: bad sizes (views %d, %d x %d)",
               n_views, rows, cols);
  MVSN_REQUIRE(max_rel_step >= 0.0f, MVSN_E_BADARG, "mvsn_depth_normals: max_rel_step %g is negative or NaN",
               (double)max_rel_step);
  MVSN_REQUIRE(n_views <= 65535 && (long)rows * cols <= 0x7fffffffL, MVSN_E_TOOLARGE,
               "mvsn_depth_normals: %d views of %d x %d pixels (at most 65535 views of 2^31 - 1 pixels)", n_views, rows,
               cols);
  const long blocks = ((long)rows * cols + NM_BLOCK_PIX - 1) / NM_BLOCK_PIX;
  hipLaunchKernelGGL(depth_normals_kernel, dim3((unsigned)blocks, n_views), dim3(NM_THREADS), 0, (hipStream_t)stream,
                     depth, valid, K, T_cam_in_world, rows, cols, max_rel_step, normals);
  return check_launch("mvsn_depth_normals");
}

extern "C" int mvsn_normals_gather(const float *normals, const int *view, const int *pixel, int n_views,
                                   long pixels_per_view, long count, float *out, mvsn_stream_t stream) {
  MVSN_REQUIRE(n_views > 0 && pixels_per_view > 0 && pixels_per_view <= 2147483647L && count >= 0 &&
                   (count + 255) / 256 <= 2147483647L,
               MVSN_E_BADARG, "mvsn_normals_gather: bad sizes");
  if (count == 0) return 0;                           // no points: nothing to launch
  MVSN_REQUIRE(normals && view && pixel && out, MVSN_E_BADARG, "mvsn_normals_gather: null pointer");
  hipLaunchKernelGGL(mvsn::gather_kernel<3>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, normals, view, pixel, n_views, pixels_per_view, count, out);
  return mvsn::check_launch("mvsn_normals_gather");
}

extern "C" int mvsn_voxel_normals(const float *normals, const int64_t *inverse, long n, long m, void *accumulators,
                                  float *out, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(n >= 0 && m >= 0, MVSN_E_BADARG, "mvsn_voxel_normals: %ld rows of %ld points", m, n);
  MVSN_REQUIRE(n <= 0x7fffffffL && m <= 0x7fffffffL, MVSN_E_TOOLARGE,
               "mvsn_voxel_normals: %ld rows of %ld points (at most 2^31 - 1 of either)", m, n);
  if (m == 0) return 0;                               // no rows: nothing to launch
  MVSN_REQUIRE(accumulators && out && (n == 0 || (normals && inverse)), MVSN_E_BADARG,
               "mvsn_voxel_normals: null pointer");
  MVSN_REQUIRE(((uintptr_t)accumulators & 7) == 0, MVSN_E_BADARG, "mvsn_voxel_normals: accumulators not 8-byte aligned");
  unsigned long long *accum = (unsigned long long *)accumulators;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(voxel_normals_zero_kernel, dim3((unsigned)((m * 3 + 255) / 256)), dim3(256), 0, st, accum, m * 3);
  if (int e = check_launch("mvsn_voxel_normals: zero")) return e;
  if (n > 0) {
    hipLaunchKernelGGL(voxel_normals_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, normals,
                       inverse, n, m, accum);
    if (int e = check_launch("mvsn_voxel_normals: accumulate")) return e;
  }
  hipLaunchKernelGGL(voxel_normals_finalise_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, accum, m, out);
  return check_launch("mvsn_voxel_normals: finalise");
}
