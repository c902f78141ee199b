// Oriented points into the TSDF volume (see include/mvsn_hip.h: mvsn_tsdf_cloud_integrate; the semantics and every
// step are DESIGN.md section 31): the implicit moving-least-squares distance, Hoppe's weighted tangent planes, added to
// the three state tensors of section 15 on an index that mvsn_cloud_index_build made over the points with cell =
// radius.  The neighbourhood is section 14's query (mvsn_cloud.h: cloud_visit) run from every voxel centre.
//
//   tsdf_cloud_mark_kernel        one thread per row: 1 into the flag byte of every brick of 8 x 8 x 8 voxels that the
//                                 row's reach box touches (widened, clipped to the volume).  Plain byte stores of one
//                                 value: whichever thread stores first, the byte is 1.  The flags are zeroed on the
//                                 stream before the launch.  A superset of the bricks that hold a voxel within reach.
//   tsdf_cloud_integrate_kernel   one workgroup per brick (a grid of TC_MAX_GRID workgroups strides over more); a
//                                 workgroup whose brick's flag is 0 moves on before it touches the state.  Each thread owns TC_VOX voxels consecutive in x and, voxel after voxel, runs
//                                 the walk from the centre: the visitor takes the row from the record's fourth word,
//                                 gathers its normal, weight and colour and adds to exact 64-bit integer sums in
//                                 registers (the order of a cell's records reaches no output); then the voxel's state
//                                 is loaded, updated in fp64, rounded once and stored.
// No atomics, no scratch, nothing waits on another workgroup, every loop bounded: every byte of the state is a
// bitwise-reproducible function of the inputs and does not depend on the order of the rows.
//
// Contraction is off for the whole file and nothing here is written as a fused multiply-add: every step of section 31
// is one operation.
#pragma clang fp contract(off)
#include "mvsn_cloud.h"

namespace mvsn {

constexpr int TC_BRICK = 8;                             // voxels along a brick's edge
constexpr int TC_VOX = 2;                               // voxels of a thread, consecutive in x
constexpr int TC_THREADS = TC_BRICK * TC_BRICK * TC_BRICK / TC_VOX;
constexpr int TC_MAX_EXTENT = 1 << 24;                  // (float)i is exact
constexpr long TC_MAX_VOXELS = 0x7fffffffL;
// A_j <= 2^24 and |T_j| <= 2^20, so a product is at most 2^44 and the sum of 2^19 - 1 of them is below 2^63
constexpr long TC_MAX_ROWS = (1L << 19) - 1;
constexpr float TC_MAX_WEIGHT = 256.0f;
constexpr float TC_A_QUANTUM = 0x1p16f, TC_T_QUANTUM = 0x1p20f;
constexpr float TC_FLT_MAX = 3.0e38f;
constexpr long TC_MAX_GRID = 1L << 22;                   // workgroups of the integrate launch

inline long tc_bricks(int n) { return ((long)n + TC_BRICK - 1) / TC_BRICK; }

// The bricks of one axis that the reach box of coordinate p touches: the voxels from (p - r - o) / v to (p + r - o) / v,
// widened by one voxel and by what the fp32 centres and differences can be off (2^-21 of the magnitudes involved, in
// voxels), clipped to [0, n).  fp64 throughout; lo > hi: none.
__device__ __forceinline__ void tc_brick_range(float p, double r, float o, float v, int n, int *lo, int *hi) {
  const double mag = (fabs((double)o) + fabs((double)p)) + (r + (double)n * (double)v);
  const double slack = 1.0 + (mag * 0x1p-21) / (double)v;
  const double a = (((double)p - r) - (double)o) / (double)v - slack;
  const double b = (((double)p + r) - (double)o) / (double)v + slack;
  // (clamped on both sides before the conversion)
  const int first = (int)fmin(fmax(floor(a), 0.0), (double)n);
  const int last = (int)fmax(fmin(ceil(b), (double)(n - 1)), -1.0);
  *lo = first / TC_BRICK;
  *hi = last < 0 ? -1 : last / TC_BRICK;
}

__global__ __launch_bounds__(CL_THREADS) void tsdf_cloud_mark_kernel(const float *__restrict__ points, long n, double reach,
                                                                     int nx, int ny, int nz, float voxel_size, float ox,
                                                                     float oy, float oz, int bx, int by,
                                                                     unsigned char *__restrict__ flags) {
  const long i = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= n) return;
  const float px = points[(size_t)i * 3], py = points[(size_t)i * 3 + 1], pz = points[(size_t)i * 3 + 2];
  if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return;
  int lo[3], hi[3];
  tc_brick_range(px, reach, ox, voxel_size, nx, lo + 0, hi + 0);
  tc_brick_range(py, reach, oy, voxel_size, ny, lo + 1, hi + 1);
  tc_brick_range(pz, reach, oz, voxel_size, nz, lo + 2, hi + 2);
  for (int c = lo[2]; c <= hi[2]; ++c)                    // (bounded: at most the bricks of the volume)
    for (int b = lo[1]; b <= hi[1]; ++b)
      for (int a = lo[0]; a <= hi[0]; ++a) flags[((size_t)c * by + b) * bx + a] = 1;
}

// One voxel: the walk from its centre (x, y, z), then the update of its state at linear index `at`.
template <bool COLOR>
__device__ __forceinline__ void tsdf_cloud_voxel(float x, float y, float z, size_t at, size_t plane,
                                                 const float *__restrict__ normals, const float *__restrict__ weights,
                                                 const unsigned char *__restrict__ colors, long n, const CloudIndex &ix,
                                                 const floatx4 *__restrict__ records, float inv, float r2, float trunc,
                                                 float *__restrict__ sdf_sum, float *__restrict__ weight,
                                                 float *__restrict__ color_sum) {
  // the sums are unsigned so that a voxel past the limit wraps instead of overflowing; each product is formed from two
  // signed 64-bit numbers and is exact
  int within = 0;
  unsigned long long sa = 0, sat = 0, sc0 = 0, sc1 = 0, sc2 = 0;
  cloud_visit(x, y, z, inv, r2, ix, records, n, [&](float dx, float dy, float dz, float d2, const floatx4 &r) {
    const long row = (long)__float_as_int(r[3]);
    if (row < 0 || row >= n) return;                      // (a built index holds rows of the cloud; any other stays inside too)
    const float ax = normals[(size_t)row * 3], ay = normals[(size_t)row * 3 + 1], az = normals[(size_t)row * 3 + 2];
    const float w = weights ? weights[row] : 1.0f;
    if (!(isfinite(ax) && isfinite(ay) && isfinite(az)) || (ax == 0.0f && ay == 0.0f && az == 0.0f)) return;
    if (!(w > 0.0f && w <= TC_MAX_WEIGHT)) return;        // (a NaN compares false)
    const float q = d2 / r2;
    const float a = 1.0f - q;
    const float phi = a * a;
    const int64_t A = (int64_t)rintf((phi * w) * TC_A_QUANTUM);
    const float s = (dx * ax + dy * ay) + dz * az;
    const float c = fminf(fmaxf(s, -trunc), trunc);       // (a NaN s, from products that overflowed, gives -trunc)
    const int64_t T = (int64_t)rintf((c / trunc) * TC_T_QUANTUM);
    ++within;
    sa += (unsigned long long)A;
    sat += (unsigned long long)(A * T);
    if (COLOR) {
      const unsigned char *rgb = colors + (size_t)row * 3;
      sc0 += (unsigned long long)(A * (int64_t)rgb[0]);
      sc1 += (unsigned long long)(A * (int64_t)rgb[1]);
      sc2 += (unsigned long long)(A * (int64_t)rgb[2]);
    }
  });
  if (within == 0 || (long)within > TC_MAX_ROWS || sa == 0) return;   // the voxel keeps its bits
  const double wsum = (double)(int64_t)sa * 0x1p-16;
  weight[at] = (float)((double)weight[at] + wsum);
  sdf_sum[at] = (float)((double)sdf_sum[at] + (double)(int64_t)sat * ((double)trunc * 0x1p-36));
  if (COLOR) {
    const unsigned long long sc[3] = {sc0, sc1, sc2};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double rgb = ((double)(int64_t)sc[ch] * 0x1p-16) / 127.5;
      color_sum[ch * plane + at] = (float)(((double)color_sum[ch * plane + at] + rgb) - wsum);
    }
  }
}

template <bool COLOR>
__global__ __launch_bounds__(TC_THREADS) void tsdf_cloud_integrate_kernel(
    const float *__restrict__ normals, const float *__restrict__ weights, const unsigned char *__restrict__ colors, long n,
    const unsigned long long *__restrict__ keys, const int *__restrict__ pop, const int *__restrict__ start,
    const floatx4 *__restrict__ records, size_t slots, float inv, float r2, int nx, int ny, int nz, float voxel_size,
    float ox, float oy, float oz, float trunc, int bx, int by, long bricks, const unsigned char *__restrict__ flags,
    float *__restrict__ sdf_sum, float *__restrict__ weight, float *__restrict__ color_sum) {
  const CloudIndex ix = {keys, pop, start, slots};
  const size_t plane = (size_t)nx * ny * nz;
  const int t = threadIdx.x;
  // (one brick per workgroup up to TC_MAX_GRID bricks; a larger volume strides)
  for (long brick = (long)blockIdx.x; brick < bricks; brick += (long)gridDim.x) {
    if (flags[brick] == 0) continue;                      // (the same byte in every thread: the workgroup moves on as one)
    const int ba = (int)(brick % bx), bb = (int)((brick / bx) % by), bc = (int)(brick / ((long)bx * by));
    const int i0 = ba * TC_BRICK + (t % (TC_BRICK / TC_VOX)) * TC_VOX;
    const int j = bb * TC_BRICK + (t / (TC_BRICK / TC_VOX)) % TC_BRICK;
    const int k = bc * TC_BRICK + t / (TC_BRICK / TC_VOX * TC_BRICK);
    if (j >= ny || k >= nz) continue;                     // (the ragged last brick of an axis)
    const float y = oy + (float)j * voxel_size, z = oz + (float)k * voxel_size;
#pragma unroll 1
    for (int i = i0; i < min(i0 + TC_VOX, nx); ++i)
      tsdf_cloud_voxel<COLOR>(ox + (float)i * voxel_size, y, z, ((size_t)k * ny + j) * nx + i, plane, normals, weights,
                              colors, n, ix, records, inv, r2, trunc, sdf_sum, weight, color_sum);
  }
}

}  // namespace mvsn

extern "C" size_t mvsn_tsdf_cloud_workspace_bytes(int nx, int ny, int nz) {
  using namespace mvsn;
  if (nx < 1 || ny < 1 || nz < 1 || nx > TC_MAX_EXTENT || ny > TC_MAX_EXTENT || nz > TC_MAX_EXTENT ||
      (long)nx * ny > TC_MAX_VOXELS || (long)nx * ny * nz > TC_MAX_VOXELS)
    return 0;
  return align256((size_t)(tc_bricks(nx) * tc_bricks(ny) * tc_bricks(nz)));
}

extern "C" int mvsn_tsdf_cloud_integrate(const float *points, const float *normals, const float *weights,
                                         const uint8_t *colors, long n, const void *index_workspace,
                                         size_t index_workspace_bytes, float cell, float inv_cell, float r2, int nx, int ny,
                                         int nz, float voxel_size, float origin_x, float origin_y, float origin_z,
                                         float trunc, float *sdf_sum, float *weight, float *color_sum, void *workspace,
                                         size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_tsdf_cloud_integrate";
  MVSN_REQUIRE(points && normals && sdf_sum && weight, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(!colors == !color_sum, MVSN_E_BADARG, "%s: colors and color_sum go together", who);
  MVSN_REQUIRE(n > 0, MVSN_E_BADARG, "%s: %ld points", who, n);
  MVSN_REQUIRE(cell > 0.0f && cell <= TC_FLT_MAX && inv_cell > 0.0f && inv_cell <= TC_FLT_MAX && r2 > 0.0f &&
                   r2 <= TC_FLT_MAX,
               MVSN_E_BADARG, "%s: cell size %g, its inverse %g or squared radius %g is not a positive finite number", who,
               (double)cell, (double)inv_cell, (double)r2);
  MVSN_REQUIRE(nx > 0 && ny > 0 && nz > 0, MVSN_E_BADARG, "%s: dims %d x %d x %d", who, nx, ny, nz);
  MVSN_REQUIRE(voxel_size > 0.0f && voxel_size <= TC_FLT_MAX && trunc > 0.0f && trunc <= TC_FLT_MAX, MVSN_E_BADARG,
               "%s: voxel size %g or truncation %g is not a positive finite number", who, (double)voxel_size,
               (double)trunc);
  MVSN_REQUIRE(fabsf(origin_x) <= TC_FLT_MAX && fabsf(origin_y) <= TC_FLT_MAX && fabsf(origin_z) <= TC_FLT_MAX,
               MVSN_E_BADARG, "%s: origin is not finite", who);
  MVSN_REQUIRE(n <= 0x7fffffffL, MVSN_E_TOOLARGE, "%s: %ld points (at most 2^31 - 1)", who, n);
  // (float)i must be exact
  MVSN_REQUIRE(nx <= TC_MAX_EXTENT && ny <= TC_MAX_EXTENT && nz <= TC_MAX_EXTENT, MVSN_E_TOOLARGE,
               "%s: %d x %d x %d voxels (at most 2^24 along an axis)", who, nx, ny, nz);
  MVSN_REQUIRE((long)nx * ny <= TC_MAX_VOXELS && (long)nx * ny * nz <= TC_MAX_VOXELS, MVSN_E_TOOLARGE,
               "%s: %d x %d x %d voxels (at most 2^31 - 1)", who, nx, ny, nz);
  CloudLayout l;
  if (int e = cloud_index_check(who, "index workspace", index_workspace, index_workspace_bytes, n, &l)) return e;
  const long bx = tc_bricks(nx), by = tc_bricks(ny), bz = tc_bricks(nz);
  const size_t flag_bytes = (size_t)(bx * by * bz);
  if (int e = workspace_check(who, "workspace", workspace, workspace_bytes, align256(flag_bytes))) return e;
  const floatx4 *records;
  const CloudIndex ix = cloud_index(index_workspace, l, &records);
  unsigned char *flags = (unsigned char *)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (hipError_t e = hipMemsetAsync(flags, 0, flag_bytes, st)) {
    set_error("%s: clearing the brick flags: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  // the reach of a row in world units: r2 is the fp32 square of cell, so neither bounds the other
  const double reach = fmax((double)cell, sqrt((double)r2));
  hipLaunchKernelGGL(tsdf_cloud_mark_kernel, dim3((unsigned)((n + CL_THREADS - 1) / CL_THREADS)), dim3(CL_THREADS), 0, st,
                     points, n, reach, nx, ny, nz, voxel_size, origin_x, origin_y, origin_z, (int)bx, (int)by, flags);
  if (int e = check_launch("mvsn_tsdf_cloud_integrate: mark")) return e;
  const long bricks = bx * by * bz;
  const dim3 grid((unsigned)(bricks < TC_MAX_GRID ? bricks : TC_MAX_GRID));
  if (color_sum)
    hipLaunchKernelGGL(tsdf_cloud_integrate_kernel<true>, grid, dim3(TC_THREADS), 0, st, normals, weights, colors, n,
                       ix.keys, ix.pop, ix.start, records, ix.slots, inv_cell, r2, nx, ny, nz, voxel_size, origin_x,
                       origin_y, origin_z, trunc, (int)bx, (int)by, bricks, flags, sdf_sum, weight, color_sum);
  else
    hipLaunchKernelGGL(tsdf_cloud_integrate_kernel<false>, grid, dim3(TC_THREADS), 0, st, normals, weights, colors, n,
                       ix.keys, ix.pop, ix.start, records, ix.slots, inv_cell, r2, nx, ny, nz, voxel_size, origin_x,
                       origin_y, origin_z, trunc, (int)bx, (int)by, bricks, flags, sdf_sum, weight, color_sum);
  return check_launch("mvsn_tsdf_cloud_integrate: integrate");
}
