// Fast Point Feature Histograms (Rusu et al., ICRA 2009) of an oriented cloud: 33 bins per point (see include/mvsn_hip.h:
// mvsn_cloud_fpfh; the semantics and every step are DESIGN.md section 23).  The neighbours of a point are section 14's
// (mvsn_cloud.h: cloud_visit) on an index that mvsn_cloud_index_build made of the cloud itself with cell size = radius.
//
//   cloud_spfh_kernel  one thread per point.  Per accepted pair the Darboux-frame triple (f1, f2, f3) by single fp32
//                      operations, each binned into 11 bins: f1 and f2 by floor(11 (f + 1) / 2) clamped, f3 (an angle)
//                      by sign tests of 2-D cross products against the ten inner sector boundaries, so that no atan2 is
//                      called.  The 33 counters of a thread live in LDS, bin-major (hist[33][CL_THREADS] int32, 33 KiB):
//                      a thread's accesses fall in its own bank column and there is no dynamically indexed private
//                      array.  Integer counts only: the order of a cell's records reaches no output.
//   cloud_fpfh_kernel  one thread per point, the same walk.  Every contributing neighbour adds
//                      rint(2^20 w spfh_j[b] / K_j) to 33 exact 64-bit integers, w = r2 / max(d2, r2 2^-20) in [1, 2^20]:
//                      each term is at most 2^40, so 2^20 neighbours (FP_MAX_NEIGHBOURS) stay below 2^60 < 2^63.  Then
//                      F[b] = spfh_i[b] / K_i + (A[b] 2^-20) / n' in fp64, each 11-bin block scaled to sum 100, one
//                      rounding to fp32 per output.
// No atomics, nothing waits on another workgroup: every output is a bitwise-reproducible function of the inputs and does
// not depend on the order of the cloud's rows in the index.
//
// Contraction is off for the whole file and nothing here is written as a fused multiply-add: every step of section 23 is
// one operation.
#pragma clang fp contract(off)
#include "mvsn_cloud.h"

namespace mvsn {

constexpr int FP_BINS = 11;
constexpr int FP_DIM = 3 * FP_BINS;
constexpr int FP_MAX_NEIGHBOURS = 1 << 20;                // past it the 64-bit sums could overflow: the row is zero

// the ten inner boundaries of the 11 equal sectors of [-pi, pi]: (cos, sin) of -pi + 2 pi k / 11, k = 1 .. 10
__constant__ float FP_SECTOR[10][2] = {
    {-0.84125353283118117f, -0.54064081745559758f}, {-0.41541501300188643f, -0.90963199535451837f},
    {0.14231483827328514f, -0.98982144188093273f},  {0.65486073394528510f, -0.75574957435425827f},
    {0.95949297361449737f, -0.28173255684142969f},  {0.95949297361449737f, 0.28173255684142969f},
    {0.65486073394528510f, 0.75574957435425827f},   {0.14231483827328514f, 0.98982144188093273f},
    {-0.41541501300188643f, 0.90963199535451837f},  {-0.84125353283118117f, 0.54064081745559758f}};

__device__ __forceinline__ bool fpfh_normal_ok(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z) && !(x == 0.0f && y == 0.0f && z == 0.0f);
}

__device__ __forceinline__ int fpfh_linear_bin(float f) {
  const float x = ((f + 1.0f) * 11.0f) * 0.5f;
  return x >= 10.0f ? 10 : (x >= 0.0f ? (int)floorf(x) : 0);   // (a NaN lands in bin 0)
}

// the sector of the direction (c, s): the lower half plane (s < 0) holds boundaries 1 .. 5, the upper one 6 .. 10; within
// a half plane the sign of the cross product b x (c, s) says on which side of boundary b the direction lies
__device__ __forceinline__ int fpfh_sector_bin(float c, float s) {
  const int first = s < 0.0f ? 0 : 5;
  int bin = first;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float bx = FP_SECTOR[first + k][0], by = FP_SECTOR[first + k][1];
    bin += (bx * s - by * c >= 0.0f) ? 1 : 0;
  }
  return bin;
}

// The three bins of the pair (query i at p with normal n, neighbour `row` with normal m; (dx, dy, dz) = p - p_row as the
// walk forms it, d2 its square).
__device__ __forceinline__ void fpfh_pair_bins(unsigned i, unsigned row, float dx, float dy, float dz, float d2, float nx,
                                               float ny, float nz, float mx, float my, float mz, int *b1, int *b2, int *b3) {
  const float d = sqrtf(d2);
  const float ex = -dx, ey = -dy, ez = -dz;                // p_row - p
  const float ai = (nx * ex + ny * ey) + nz * ez;
  const float aj = (mx * ex + my * ey) + mz * ez;
  const float fi = fabsf(ai), fj = fabsf(aj);
  const bool own = fi > fj || (fi == fj && i < row) || (fi != fi || fj != fj);   // the source is the query (a NaN: the query)
  const float ux = own ? nx : mx, uy = own ? ny : my, uz = own ? nz : mz;       // n_s
  const float tx = own ? mx : nx, ty = own ? my : ny, tz = own ? mz : nz;       // n_t
  const float gx = own ? ex : dx, gy = own ? ey : dy, gz = own ? ez : dz;       // p_t - p_s
  const float lx = gx / d, ly = gy / d, lz = gz / d;
  const float f2 = (ux * lx + uy * ly) + uz * lz;
  const float vx = uy * lz - uz * ly, vy = uz * lx - ux * lz, vz = ux * ly - uy * lx;
  const float wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
  const float f1 = (vx * tx + vy * ty) + vz * tz;
  const float c3 = (ux * tx + uy * ty) + uz * tz;
  const float s3 = (wx * tx + wy * ty) + wz * tz;
  *b1 = fpfh_linear_bin(f1);
  *b2 = fpfh_linear_bin(f2);
  *b3 = fpfh_sector_bin(c3, s3);
}

__global__ __launch_bounds__(CL_THREADS) void cloud_spfh_kernel(const float *__restrict__ points,
                                                                const float *__restrict__ normals, long n, float inv,
                                                                float r2, const unsigned long long *__restrict__ keys,
                                                                const int *__restrict__ pop, const int *__restrict__ start,
                                                                const floatx4 *__restrict__ records, size_t slots,
                                                                int *__restrict__ spfh, int *__restrict__ pairs) {
  __shared__ int hist[FP_DIM][CL_THREADS];
  const int tid = threadIdx.x;
  const long i = (long)blockIdx.x * CL_THREADS + tid;
  if (i >= n) return;                                      // (no barrier below: a thread owns its column)
#pragma unroll
  for (int b = 0; b < FP_DIM; ++b) hist[b][tid] = 0;
  const float px = points[(size_t)i * 3], py = points[(size_t)i * 3 + 1], pz = points[(size_t)i * 3 + 2];
  const float nx = normals[(size_t)i * 3], ny = normals[(size_t)i * 3 + 1], nz = normals[(size_t)i * 3 + 2];
  const CloudIndex ix = {keys, pop, start, slots};
  int count = 0;
  if (fpfh_normal_ok(nx, ny, nz))
    cloud_visit(px, py, pz, inv, r2, ix, records, n,
                [&](float dx, float dy, float dz, float d2, const floatx4 &r) {
                  const unsigned row = __float_as_uint(r[3]);
                  if (row == (unsigned)i || d2 == 0.0f || (long)row >= n) return;
                  const float mx = normals[(size_t)row * 3], my = normals[(size_t)row * 3 + 1], mz = normals[(size_t)row * 3 + 2];
                  if (!fpfh_normal_ok(mx, my, mz)) return;
                  int b1, b2, b3;
                  fpfh_pair_bins((unsigned)i, row, dx, dy, dz, d2, nx, ny, nz, mx, my, mz, &b1, &b2, &b3);
                  ++count;
                  hist[b1][tid] += 1;
                  hist[FP_BINS + b2][tid] += 1;
                  hist[2 * FP_BINS + b3][tid] += 1;
                });
  pairs[i] = count;
#pragma unroll
  for (int b = 0; b < FP_DIM; ++b) spfh[(size_t)i * FP_DIM + b] = hist[b][tid];
}

__global__ __launch_bounds__(CL_THREADS) void cloud_fpfh_kernel(const float *__restrict__ points,
                                                                const float *__restrict__ normals, long n, float inv,
                                                                float r2, long min_neighbours,
                                                                const unsigned long long *__restrict__ keys,
                                                                const int *__restrict__ pop, const int *__restrict__ start,
                                                                const floatx4 *__restrict__ records, size_t slots,
                                                                const int *__restrict__ spfh, const int *__restrict__ pairs,
                                                                float *__restrict__ features) {
  const long i = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= n) return;
  const float px = points[(size_t)i * 3], py = points[(size_t)i * 3 + 1], pz = points[(size_t)i * 3 + 2];
  const float nx = normals[(size_t)i * 3], ny = normals[(size_t)i * 3 + 1], nz = normals[(size_t)i * 3 + 2];
  const int ki = pairs[i];
  const CloudIndex ix = {keys, pop, start, slots};
  float *out = features + (size_t)i * FP_DIM;

  long long acc[FP_DIM];
#pragma unroll
  for (int b = 0; b < FP_DIM; ++b) acc[b] = 0;
  int used = 0;
  const double r2d = (double)r2;
  const double floor_d2 = r2d * 0x1p-20;
  if (ki > 0 && (long)ki >= min_neighbours && fpfh_normal_ok(nx, ny, nz))
    cloud_visit(px, py, pz, inv, r2, ix, records, n,
                [&](float, float, float, float d2, const floatx4 &r) {
                  const unsigned row = __float_as_uint(r[3]);
                  if (row == (unsigned)i || d2 == 0.0f || (long)row >= n) return;
                  const float mx = normals[(size_t)row * 3], my = normals[(size_t)row * 3 + 1], mz = normals[(size_t)row * 3 + 2];
                  if (!fpfh_normal_ok(mx, my, mz)) return;
                  const int kj = pairs[row];
                  if (kj <= 0) return;
                  ++used;
                  if (used > FP_MAX_NEIGHBOURS) return;   // (the row is zero then; nothing more is added)
                  const double dd = (double)d2;
                  const double w = r2d / (dd > floor_d2 ? dd : floor_d2);
                  const double s = w * 0x1p20, kd = (double)kj;
                  const int *sj = spfh + (size_t)row * FP_DIM;
#pragma unroll
                  for (int b = 0; b < FP_DIM; ++b) {
                    const double x = (s * (double)sj[b]) / kd;
                    acc[b] += (long long)rint(x);
                  }
                });
  if (!(ki > 0 && (long)ki >= min_neighbours) || used > FP_MAX_NEIGHBOURS) {
#pragma unroll
    for (int b = 0; b < FP_DIM; ++b) out[b] = 0.0f;
    return;
  }
  const double kd = (double)ki, nd = (double)used;
  const int *si = spfh + (size_t)i * FP_DIM;
#pragma unroll
  for (int block = 0; block < 3; ++block) {
    double f[FP_BINS];
    double sum = 0.0;
#pragma unroll
    for (int b = 0; b < FP_BINS; ++b) {
      const double own = (double)si[block * FP_BINS + b] / kd;
      const double nb = used > 0 ? ((double)acc[block * FP_BINS + b] * 0x1p-20) / nd : 0.0;
      f[b] = own + nb;
      sum = sum + f[b];
    }
#pragma unroll
    for (int b = 0; b < FP_BINS; ++b) out[block * FP_BINS + b] = (float)((f[b] * 100.0) / sum);
  }
}

}  // namespace mvsn

extern "C" int mvsn_cloud_fpfh(const float *points, const float *normals, long n, float cell, float inv_cell, float r2,
                               long min_neighbours, const void *index_workspace, size_t index_workspace_bytes, int *spfh,
                               int *pairs, float *features, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_fpfh";
  MVSN_REQUIRE(points && normals && spfh && pairs && features, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(n > 0, MVSN_E_BADARG, "%s: %ld points", who, n);
  MVSN_REQUIRE(cell > 0.0f && cell <= 3.0e38f && inv_cell > 0.0f && inv_cell <= 3.0e38f && r2 > 0.0f && r2 <= 3.0e38f,
               MVSN_E_BADARG, "%s: cell size %g, its inverse %g or squared radius %g is not a positive finite number", who,
               (double)cell, (double)inv_cell, (double)r2);
  MVSN_REQUIRE(min_neighbours >= 1, MVSN_E_BADARG, "%s: min_neighbours = %ld (at least 1)", who, min_neighbours);
  MVSN_REQUIRE(n <= 0x7fffffffL, MVSN_E_TOOLARGE, "%s: %ld points (at most 2^31 - 1)", who, n);
  CloudLayout l;
  if (int e = cloud_index_check(who, "index workspace", index_workspace, index_workspace_bytes, n, &l)) return e;
  const floatx4 *records;
  const CloudIndex ix = cloud_index(index_workspace, l, &records);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + CL_THREADS - 1) / CL_THREADS)), block(CL_THREADS);
  hipLaunchKernelGGL(cloud_spfh_kernel, grid, block, 0, st, points, normals, n, inv_cell, r2, ix.keys, ix.pop, ix.start,
                     records, ix.slots, spfh, pairs);
  if (int e = check_launch("mvsn_cloud_fpfh: spfh")) return e;
  hipLaunchKernelGGL(cloud_fpfh_kernel, grid, block, 0, st, points, normals, n, inv_cell, r2, min_neighbours, ix.keys,
                     ix.pop, ix.start, records, ix.slots, (const int *)spfh, (const int *)pairs, features);
  return check_launch("mvsn_cloud_fpfh: fpfh");
}
