// Alignment of depth maps to the dense TSDF volume (see include/mvsn_hip.h: mvsn_tsdf_align, mvsn_tsdf_align_system; the
// semantics are DESIGN.md section 17): Gauss-Newton on the point-to-TSDF residual.  A pixel with depth D is the grid
// point g = fma(D, dir, g0) of section 16's camera; its residual is the trilinear value there over the voxel size, its
// Jacobian under a rigid update about the volume's centre is (n, q x n) with n the analytic gradient and q = g - c0.
//
//   tsdf_values_kernel              (mvsn_tsdf_raycast.hip) the plane d, NaN at an unobserved voxel: once per call
//   tsdf_align_accumulate_kernel    the view on the grid's z; a workgroup of 256 threads owns 32 x 32 pixels of the stride
//                                   lattice, in four passes of 16 x 16 with each wave on a compact 8 x 8 tile.  Thread 0
//                                   forms the camera in fp64 from the current fp64 pose into LDS.  Every thread sums its
//                                   pixels' 30 terms in fp64, the wave adds them by an xor tree, the four waves are added
//                                   in index order through LDS, and the workgroup stores one record of 30 doubles.
//   tsdf_align_solve_kernel         one workgroup of 64 threads per view: thread i < 30 adds term i of the view's records
//                                   in index order; thread 0 writes the history row and, when asked to, scales the 6 x 6
//                                   to a unit diagonal, factors it (Cholesky), solves, and applies the update to the
//                                   fp64 pose in the workspace.  The last launch only reduces: it writes the normal
//                                   matrix, the right-hand side and the fp32 pose.
// No atomics, no scratch, nothing waits on another workgroup: the order of every sum is fixed by the launch geometry, so
// the outputs are bitwise reproducible and a view's results do not depend on the other views of the call.
//
// Contraction is off for the whole file: every fused multiply-add of section 17 is written as fmaf / fma, every other
// step is one operation.
#pragma clang fp contract(off)
#include "mvsn_tsdf_sample.h"
#include "mvsn_pose.h"

namespace mvsn {

constexpr int TA_THREADS = 256;
constexpr int TA_TILE = 32;                             // lattice pixels of a workgroup along each axis
constexpr int TA_PASSES = 4;                            // 2 x 2 passes of 16 x 16: 2 x 2 waves of 8 x 8
constexpr int TA_TERMS = 30;                            // 21 of H (upper triangle, row-major), 6 of b, sum w, sum w r^2, count
constexpr int TA_SOLVE_THREADS = 64;
constexpr int TA_POSE = 12;                             // doubles of a pose in the workspace: R row-major, then t
constexpr int TA_MAX_ITERATIONS = 1000;

// A = R K^-1 / voxel_size (out[0..8]) and g0 = (t - origin) / voxel_size (out[9..11]) from the fp64 pose P (R row-major,
// then t): section 16's camera with its operations in its order, each of the twelve rounded once
__device__ inline void align_camera(const float *K, const double *P, float voxel_size, float ox, float oy, float oz,
                                    float *out) {
  double Ki[9];
  inv3_d(K, Ki);
  const double vs = (double)voxel_size;
  const double o[3] = {(double)ox, (double)oy, (double)oz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
      out[a * 3 + b] = (float)(((P[a * 3 + 0] * Ki[b] + P[a * 3 + 1] * Ki[3 + b]) + P[a * 3 + 2] * Ki[6 + b]) / vs);
    out[9 + a] = (float)((P[9 + a] - o[a]) / vs);
  }
}

// the pose of a view as 12 doubles: the workspace's, or (before the first update) the float32 values of T_cam_in_world
__device__ inline void align_pose(const float *T, const double *pose, double *P) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) P[a * 3 + b] = pose ? pose[a * 3 + b] : (double)T[a * 4 + b];
    P[9 + a] = pose ? pose[9 + a] : (double)T[a * 4 + 3];
  }
}

template <bool RESIDUAL>
__global__ __launch_bounds__(TA_THREADS) void tsdf_align_accumulate_kernel(
    const float *__restrict__ d, int nx, int ny, int nz, float voxel_size, float ox, float oy, float oz,
    const float *__restrict__ depth, const uint8_t *__restrict__ valid, const float *__restrict__ weights,
    const float *__restrict__ K, const float *__restrict__ T, const double *__restrict__ pose, int rows, int cols,
    int stride, int lat_rows, int lat_cols, int tiles_x, float band, double *__restrict__ records,
    float *__restrict__ residual) {
  __shared__ float scam[12];
  __shared__ double swave[TA_THREADS / 64][TA_TERMS];
  const int view = blockIdx.z;
  if (threadIdx.x == 0) {
    double P[TA_POSE];
    align_pose(T + (size_t)view * 16, pose ? pose + (size_t)view * TA_POSE : nullptr, P);
    align_camera(K + (size_t)view * 16, P, voxel_size, ox, oy, oz, scam);
  }
  __syncthreads();
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float top[3] = {(float)(nx - 2), (float)(ny - 2), (float)(nz - 2)};   // the highest lowest corner of a cell
  const float c0[3] = {(float)(nx - 1) * 0.5f, (float)(ny - 1) * 0.5f, (float)(nz - 1) * 0.5f};   // (exact)
  const long lnx = nx, nxy = (long)nx * ny;
  const size_t P = (size_t)rows * cols;

  double acc[TA_TERMS];
#pragma unroll
  for (int i = 0; i < TA_TERMS; ++i) acc[i] = 0.0;
  int count = 0;

#pragma unroll 1
  for (int pass = 0; pass < TA_PASSES; ++pass) {
    const int lx = tile_x * TA_TILE + (pass & 1) * 16 + (wave & 1) * 8 + (lane & 7);
    const int ly = tile_y * TA_TILE + (pass >> 1) * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (lx >= lat_cols || ly >= lat_rows) continue;                 // (no barrier inside the loop)
    const int x = lx * stride, y = ly * stride;                     // < cols, rows: the lattice counts say so
    const size_t pix = (size_t)y * cols + x;
    const float D = depth[view * P + pix];
    const float w = weights ? weights[view * P + pix] : 1.0f;
    bool takes = D > 0.0f && D <= TR_FLT_MAX && w > 0.0f && w <= TR_FLT_MAX && (!valid || valid[view * P + pix] != 0);

    const float xf = (float)x, yf = (float)y;
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float dir = fmaf(scam[a * 3 + 0], xf, fmaf(scam[a * 3 + 1], yf, scam[a * 3 + 2]));
      g[a] = fmaf(D, dir, scam[9 + a]);
    }
    const float cx = floorf(g[0]), cy = floorf(g[1]), cz = floorf(g[2]);
    // in range, compared as floats: a NaN fails
    takes = takes && cx >= 0.0f && cx <= top[0] && cy >= 0.0f && cy <= top[1] && cz >= 0.0f && cz <= top[2];
    float r = NAN;
    if (takes) {                                                    // (nothing is loaded for a point out of range)
      float v[8], grad[3];
      cell_load(d, ((long)cz * ny + (long)cy) * lnx + (long)cx, lnx, nxy, v);
      const float fx = g[0] - cx, fy = g[1] - cy, fz = g[2] - cz;
      const float f = trilinear(v, fx, fy, fz);                     // a NaN: a corner is not observed
      trilinear_gradient(v, fx, fy, fz, grad);
      const float n[3] = {grad[0] / voxel_size, grad[1] / voxel_size, grad[2] / voxel_size};
      takes = fabsf(f) <= band && fabsf(n[0]) <= TR_FLT_MAX && fabsf(n[1]) <= TR_FLT_MAX && fabsf(n[2]) <= TR_FLT_MAX;
      if (takes) {
        r = f / voxel_size;
        const float q[3] = {g[0] - c0[0], g[1] - c0[1], g[2] - c0[2]};
        const float J[6] = {n[0], n[1], n[2], fmaf(q[1], n[2], -(q[2] * n[1])), fmaf(q[2], n[0], -(q[0] * n[2])),
                            fmaf(q[0], n[1], -(q[1] * n[0]))};
        const double wd = (double)w, rd = (double)r;
        int m = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          const double wJ = wd * (double)J[i];
#pragma unroll
          for (int j = i; j < 6; ++j, ++m) acc[m] = acc[m] + wJ * (double)J[j];
          acc[21 + i] = acc[21 + i] + wJ * rd;
        }
        acc[27] = acc[27] + wd;
        acc[28] = acc[28] + (wd * rd) * rd;
        ++count;
      }
    }
    if (RESIDUAL) {                                                 // the lattice pixel and the pixels off the lattice
      float *out = residual + view * P;                             // behind it: every pixel once
      const int x_end = min(x + stride, cols), y_end = min(y + stride, rows);
      for (int yy = y; yy < y_end; ++yy)
        for (int xx = x; xx < x_end; ++xx) out[(size_t)yy * cols + xx] = (yy == y && xx == x) ? r : NAN;
    }
  }
  acc[29] = (double)count;

  // the wave's sum: an xor tree, every lane ends with the same bits (a + b = b + a)
#pragma unroll
  for (int i = 0; i < TA_TERMS; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[i] = acc[i] + __shfl_xor(acc[i], off, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < TA_TERMS; ++i) swave[wave][i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x < TA_TERMS) {                                     // the waves in index order
    const int i = threadIdx.x;
    records[((size_t)view * gridDim.x + blockIdx.x) * TA_TERMS + i] =
        ((swave[0][i] + swave[1][i]) + swave[2][i]) + swave[3][i];
  }
}

// The update of one view from its sums s (TA_TERMS): 0 and the new pose in P, or the status that stops the view (1: fewer
// than min_pixels take part; 2: the scaled normal matrix has a pivot below min_pivot, or a diagonal entry that is not a
// positive finite number) with P untouched.  The solve is mvsn_pose.h's; it hands delta to the update below.
__device__ inline int align_update(const double *s, double min_pixels, double min_pivot, float voxel_size, float ox,
                                   float oy, float oz, int nx, int ny, int nz, double *P) {
  return pose_solve(s, min_pixels, min_pivot, [&](const double *delta) {
    // R <- Rd R, t <- Rd (t - cw) + cw + voxel_size v, cw = origin + voxel_size c0
    double Rd[9], N[TA_POSE];
    align_rotation(delta + 3, Rd);
    const double vs = (double)voxel_size;
    const double cw[3] = {(double)ox + vs * ((double)(nx - 1) * 0.5), (double)oy + vs * ((double)(ny - 1) * 0.5),
                          (double)oz + vs * ((double)(nz - 1) * 0.5)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) N[a * 3 + b] = (Rd[a * 3] * P[b] + Rd[a * 3 + 1] * P[3 + b]) + Rd[a * 3 + 2] * P[6 + b];
      N[9 + a] = (((Rd[a * 3] * (P[9] - cw[0]) + Rd[a * 3 + 1] * (P[10] - cw[1])) + Rd[a * 3 + 2] * (P[11] - cw[2])) + cw[a]) +
                 vs * delta[a];
    }
#pragma unroll
    for (int i = 0; i < TA_POSE; ++i) P[i] = N[i];
    return 0;
  });
}

// One workgroup per view.  `pose_in` null: the pose is the float32 T (before the first update).  `update`: solve and
// write the new pose to pose_out (the old one when the view is stopped); without it the launch only reduces.  Outputs
// that are null are not written.  `status` is read unless `first` (then it is 0) and written with `update`.
__global__ __launch_bounds__(TA_SOLVE_THREADS) void tsdf_align_solve_kernel(
    const double *__restrict__ records, int n_records, const float *__restrict__ T, const double *pose_in,
    double *pose_out, int first, int update, double min_pixels, double min_pivot, float voxel_size, float ox, float oy,
    float oz, int nx, int ny, int nz, int *status, double *__restrict__ history, int history_rows, int history_row,
    double *__restrict__ information, double *__restrict__ rhs, float *__restrict__ T_out) {
  __shared__ double ssum[TA_TERMS];
  const int view = blockIdx.x;
  if (threadIdx.x < TA_TERMS) {
    const double *p = records + (size_t)view * n_records * TA_TERMS + threadIdx.x;
    double sum = 0.0;
    for (int g = 0; g < n_records; ++g) sum = sum + p[(size_t)g * TA_TERMS];   // the workgroups in index order
    ssum[threadIdx.x] = sum;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s[TA_TERMS];
#pragma unroll
  for (int i = 0; i < TA_TERMS; ++i) s[i] = ssum[i];
  if (history) {
    double *h = history + ((size_t)view * history_rows + history_row) * 3;
    h[0] = s[29], h[1] = s[27], h[2] = s[28];
  }
  if (information) {
    int m = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++m) information[(size_t)view * 36 + i * 6 + j] = information[(size_t)view * 36 + j * 6 + i] = s[m];
  }
  if (rhs) {
#pragma unroll
    for (int i = 0; i < 6; ++i) rhs[(size_t)view * 6 + i] = s[21 + i];
  }
  double P[TA_POSE];
  align_pose(T + (size_t)view * 16, pose_in ? pose_in + (size_t)view * TA_POSE : nullptr, P);
  if (first && !update && status) status[view] = 0;                 // no iteration asked for: every view ran them all
  if (update) {
    int st = first ? 0 : status[view];
    if (st == 0) st = align_update(s, min_pixels, min_pivot, voxel_size, ox, oy, oz, nx, ny, nz, P);
    status[view] = st;
#pragma unroll
    for (int i = 0; i < TA_POSE; ++i) pose_out[(size_t)view * TA_POSE + i] = P[i];
  }
  if (T_out) {                                                      // each number rounded once; the bottom row is T's
    float *o = T_out + (size_t)view * 16;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) o[a * 4 + b] = (float)P[a * 3 + b];
      o[a * 4 + 3] = (float)P[9 + a];
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) o[12 + b] = T[(size_t)view * 16 + 12 + b];
  }
}

struct AlignPlan {
  int lat_rows, lat_cols, tiles_x;
  long tiles;                                                       // workgroups, and records, per view
  size_t d_bytes, pose_bytes, record_bytes;
};

inline bool align_sizes_ok(int n_views, int rows, int cols, int stride) {
  return n_views > 0 && rows > 0 && cols > 0 && stride > 0;
}

inline AlignPlan align_plan(int nx, int ny, int nz, int n_views, int rows, int cols, int stride) {
  AlignPlan p;
  p.lat_rows = (rows + stride - 1) / stride, p.lat_cols = (cols + stride - 1) / stride;
  p.tiles_x = (p.lat_cols + TA_TILE - 1) / TA_TILE;
  p.tiles = (long)p.tiles_x * ((p.lat_rows + TA_TILE - 1) / TA_TILE);
  p.d_bytes = align256(sizeof(float) * (size_t)nx * ny * nz);
  p.pose_bytes = align256(sizeof(double) * TA_POSE * (size_t)n_views);
  p.record_bytes = align256(sizeof(double) * TA_TERMS * (size_t)p.tiles * n_views);
  return p;
}

struct AlignArgs {
  const float *sdf_sum, *weight;
  int nx, ny, nz;
  float voxel_size, ox, oy, oz;
  const float *depth;
  const uint8_t *valid;
  const float *weights, *K, *T;
  int n_views, rows, cols, stride;
  float min_weight, band;
  void *workspace;
  size_t workspace_bytes;
};

// the checks both entries share; 0 or the error code
inline int align_check(const char *who, const AlignArgs &a) {
  MVSN_REQUIRE(a.sdf_sum && a.weight && a.depth && a.K && a.T, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(a.n_views > 0 && a.rows > 0 && a.cols > 0, MVSN_E_BADARG, "%s: bad sizes (views %d, %d x %d)", who,
               a.n_views, a.rows, a.cols);
  MVSN_REQUIRE(a.n_views <= 65535 && (long)a.rows * a.cols <= 0x7fffffffL && a.rows <= TR_MAX_EXTENT && a.cols <= TR_MAX_EXTENT,
               MVSN_E_TOOLARGE, "%s: %d views of %d x %d pixels (at most 65535 views of 2^31 - 1 pixels, 2^24 along an axis)",
               who, a.n_views, a.rows, a.cols);
  MVSN_REQUIRE(a.stride >= 1 && a.stride <= TR_MAX_EXTENT, MVSN_E_BADARG, "%s: stride %d (1 to 2^24)", who, a.stride);
  MVSN_REQUIRE(a.nx >= 2 && a.ny >= 2 && a.nz >= 2, MVSN_E_BADARG, "%s: dims %d x %d x %d (at least 2 each)", who, a.nx, a.ny,
               a.nz);
  MVSN_REQUIRE(raycast_dims_ok(a.nx, a.ny, a.nz), MVSN_E_TOOLARGE, "%s: %d x %d x %d voxels (at most 2^31 - 1, 2^24 along an axis)",
               who, a.nx, a.ny, a.nz);
  MVSN_REQUIRE(raycast_positive(a.voxel_size) && raycast_positive(a.min_weight) && raycast_positive(a.band), MVSN_E_BADARG,
               "%s: voxel size %g, min_weight %g or band %g is not a positive finite number", who, (double)a.voxel_size,
               (double)a.min_weight, (double)a.band);
  MVSN_REQUIRE(fabsf(a.ox) <= TR_FLT_MAX && fabsf(a.oy) <= TR_FLT_MAX && fabsf(a.oz) <= TR_FLT_MAX, MVSN_E_BADARG,
               "%s: origin is not finite", who);
  const AlignPlan p = align_plan(a.nx, a.ny, a.nz, a.n_views, a.rows, a.cols, a.stride);
  const size_t need = p.d_bytes + p.pose_bytes + p.record_bytes;
  MVSN_REQUIRE(a.workspace && a.workspace_bytes >= need, MVSN_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who,
               a.workspace_bytes, need);
  MVSN_REQUIRE(((uintptr_t)a.workspace & 15) == 0, MVSN_E_BADARG, "%s: workspace not 16-byte aligned", who);
  return 0;
}

inline int align_values(const AlignArgs &a, float *d, hipStream_t st, const char *what) {
  const long n = (long)a.nx * a.ny * a.nz;
  const long items = (n + TR_VOX - 1) / TR_VOX;
  hipLaunchKernelGGL(tsdf_values_kernel, dim3((unsigned)((items + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, st,
                     a.sdf_sum, a.weight, n, a.min_weight, d);
  return check_launch(what);
}

inline int align_accumulate(const AlignArgs &a, const AlignPlan &p, const float *d, const double *pose, double *records,
                            float *residual, hipStream_t st, const char *what) {
  const dim3 grid((unsigned)p.tiles, 1, (unsigned)a.n_views);
  if (residual)
    hipLaunchKernelGGL(tsdf_align_accumulate_kernel<true>, grid, dim3(TA_THREADS), 0, st, d, a.nx, a.ny, a.nz, a.voxel_size,
                       a.ox, a.oy, a.oz, a.depth, a.valid, a.weights, a.K, a.T, pose, a.rows, a.cols, a.stride, p.lat_rows,
                       p.lat_cols, p.tiles_x, a.band, records, residual);
  else
    hipLaunchKernelGGL(tsdf_align_accumulate_kernel<false>, grid, dim3(TA_THREADS), 0, st, d, a.nx, a.ny, a.nz, a.voxel_size,
                       a.ox, a.oy, a.oz, a.depth, a.valid, a.weights, a.K, a.T, pose, a.rows, a.cols, a.stride, p.lat_rows,
                       p.lat_cols, p.tiles_x, a.band, records, residual);
  return check_launch(what);
}

}  // namespace mvsn

extern "C" size_t mvsn_tsdf_align_workspace_bytes(int nx, int ny, int nz, int n_views, int rows, int cols, int stride) {
  using namespace mvsn;
  if (!raycast_dims_ok(nx, ny, nz) || !align_sizes_ok(n_views, rows, cols, stride) || n_views > 65535 ||
      rows > TR_MAX_EXTENT || cols > TR_MAX_EXTENT || stride > TR_MAX_EXTENT || (long)rows * cols > 0x7fffffffL)
    return 0;
  const AlignPlan p = align_plan(nx, ny, nz, n_views, rows, cols, stride);
  return p.d_bytes + p.pose_bytes + p.record_bytes;
}

extern "C" int mvsn_tsdf_align_system(const float *sdf_sum, const float *weight, int nx, int ny, int nz, float voxel_size,
                                      float origin_x, float origin_y, float origin_z, const float *depth,
                                      const uint8_t *valid, const float *weights, const float *K,
                                      const float *T_cam_in_world, int n_views, int rows, int cols, int stride,
                                      float min_weight, float band, void *workspace, size_t workspace_bytes, double *H,
                                      double *b, double *sums, float *residual, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_tsdf_align_system";
  const AlignArgs a = {sdf_sum, weight, nx, ny, nz, voxel_size, origin_x, origin_y, origin_z, depth, valid, weights, K,
                       T_cam_in_world, n_views, rows, cols, stride, min_weight, band, workspace, workspace_bytes};
  MVSN_REQUIRE(H && b && sums, MVSN_E_BADARG, "%s: null pointer", who);
  if (int e = align_check(who, a)) return e;
  const AlignPlan p = align_plan(nx, ny, nz, n_views, rows, cols, stride);
  float *d = (float *)workspace;
  double *records = (double *)((char *)workspace + p.d_bytes + p.pose_bytes);
  const hipStream_t st = (hipStream_t)stream;
  if (int e = align_values(a, d, st, "mvsn_tsdf_align_system: values")) return e;
  if (int e = align_accumulate(a, p, d, nullptr, records, residual, st, "mvsn_tsdf_align_system: accumulate")) return e;
  hipLaunchKernelGGL(tsdf_align_solve_kernel, dim3((unsigned)n_views), dim3(TA_SOLVE_THREADS), 0, st,
                     (const double *)records, (int)p.tiles, T_cam_in_world, (const double *)nullptr, (double *)nullptr, 1, 0,
                     0.0, 0.0, voxel_size, origin_x, origin_y, origin_z, nx, ny, nz, (int *)nullptr, sums, 1, 0, H, b,
                     (float *)nullptr);
  return check_launch("mvsn_tsdf_align_system: reduce");
}

extern "C" int mvsn_tsdf_align(const float *sdf_sum, const float *weight, int nx, int ny, int nz, float voxel_size,
                               float origin_x, float origin_y, float origin_z, const float *depth, const uint8_t *valid,
                               const float *weights, const float *K, const float *T_cam_in_world, int n_views, int rows,
                               int cols, int stride, float min_weight, float band, int iterations, long min_pixels,
                               double min_pivot, void *workspace, size_t workspace_bytes, float *T_out, double *history,
                               int *status, double *information, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_tsdf_align";
  const AlignArgs a = {sdf_sum, weight, nx, ny, nz, voxel_size, origin_x, origin_y, origin_z, depth, valid, weights, K,
                       T_cam_in_world, n_views, rows, cols, stride, min_weight, band, workspace, workspace_bytes};
  MVSN_REQUIRE(T_out && history && status && information, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(iterations >= 0 && iterations <= TA_MAX_ITERATIONS, MVSN_E_BADARG, "%s: %d iterations (0 to 1000)", who,
               iterations);
  MVSN_REQUIRE(min_pixels >= 1, MVSN_E_BADARG, "%s: min_pixels %ld (at least 1)", who, min_pixels);
  MVSN_REQUIRE(min_pivot > 0.0 && min_pivot < 1.0, MVSN_E_BADARG, "%s: min_pivot %g (inside (0, 1))", who, min_pivot);
  if (int e = align_check(who, a)) return e;
  const AlignPlan p = align_plan(nx, ny, nz, n_views, rows, cols, stride);
  float *d = (float *)workspace;
  double *pose = (double *)((char *)workspace + p.d_bytes);
  double *records = (double *)((char *)workspace + p.d_bytes + p.pose_bytes);
  const hipStream_t st = (hipStream_t)stream;
  if (int e = align_values(a, d, st, "mvsn_tsdf_align: values")) return e;
  for (int it = 0; it <= iterations; ++it) {
    const double *cur = it == 0 ? nullptr : pose;                   // before the first update: the float32 T
    if (int e = align_accumulate(a, p, d, cur, records, nullptr, st, "mvsn_tsdf_align: accumulate")) return e;
    const bool last = it == iterations;
    hipLaunchKernelGGL(tsdf_align_solve_kernel, dim3((unsigned)n_views), dim3(TA_SOLVE_THREADS), 0, st,
                       (const double *)records, (int)p.tiles, T_cam_in_world, cur, pose, it == 0 ? 1 : 0, last ? 0 : 1,
                       (double)min_pixels, min_pivot, voxel_size, origin_x, origin_y, origin_z, nx, ny, nz, status, history,
                       iterations + 1, it, last ? information : (double *)nullptr, (double *)nullptr,
                       last ? T_out : (float *)nullptr);
    if (int e = check_launch("mvsn_tsdf_align: solve")) return e;
  }
  return 0;
}
