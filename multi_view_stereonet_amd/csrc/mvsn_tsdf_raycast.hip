// Ray-cast of the dense TSDF volume (see include/mvsn_hip.h: mvsn_tsdf_raycast; the semantics are DESIGN.md section
// 16): depth, normal, colour and weight maps of the volume's surface as cameras (K, T) see it.
//
//   tsdf_values_kernel    the plane d = sdf_sum / weight (one IEEE division, the quotient the mesh extraction classifies
//                         by) with a NaN where weight < min_weight, into the workspace: 4 bytes per voxel, three plane
//                         passes once per call whatever V is.  A sample of the march is then eight loads and seven
//                         fmas, and "every corner observed" is "the interpolant is not a NaN".
//   tsdf_raycast_kernel   one thread per pixel, 256 threads = 16 x 16 pixels, each wave a compact 8 x 8 tile so that
//                         neighbouring rays fetch their corners from the same cache lines; the view on the grid's z.
//                         The camera (A = R K^-1 / voxel_size, g0 = (t - origin) / voxel_size; fp64, rounded once) is
//                         formed by thread 0 into LDS.  Each ray clips itself against the box in fp64 (the slab test,
//                         widened by two steps at both ends: the widening covers the rounding of t_k = k step), marches
//                         its samples in ascending k and stops at the first sign change; the wave's loop ends when all
//                         its rays have.  Weight, colour and the gradient are read at the hit only, from the state.
// No atomics, no scratch, nothing waits on another workgroup; every pixel of every output is written once by its own
// thread; the march is bounded by the sample count the entry checks.
//
// Contraction is off for the whole file: every fused multiply-add of section 16 is written as fmaf, every other step
// is one fp32 operation.
#pragma clang fp contract(off)
#include "mvsn_tsdf_sample.h"

namespace mvsn {

constexpr int TR_TILE = 16;                             // pixels of a workgroup along each axis: 2 x 2 waves of 8 x 8
constexpr long TR_MAX_SAMPLES = 1L << 20;               // samples of one ray inside the box
constexpr int TR_SLACK = 8;                             // the clip's widening (2 x 2), its floor and ceil, and room

__global__ __launch_bounds__(TR_THREADS) void tsdf_values_kernel(const float *__restrict__ sdf_sum,
                                                                 const float *__restrict__ weight, long n,
                                                                 float min_weight, float *__restrict__ d) {
  const long a = ((long)blockIdx.x * TR_THREADS + threadIdx.x) * TR_VOX;
  if (a >= n) return;
  if (a + TR_VOX <= n && (((uintptr_t)(sdf_sum + a) | (uintptr_t)(weight + a) | (uintptr_t)(d + a)) & 15) == 0) {
    const floatx4 s = *reinterpret_cast<const floatx4 *>(sdf_sum + a);
    const floatx4 w = *reinterpret_cast<const floatx4 *>(weight + a);
    floatx4 q;
#pragma unroll
    for (int m = 0; m < TR_VOX; ++m) q[m] = w[m] >= min_weight ? s[m] / w[m] : NAN;
    *reinterpret_cast<floatx4 *>(d + a) = q;
  } else {
    for (int m = 0; m < TR_VOX && a + m < n; ++m) {
      const float w = weight[a + m];
      d[a + m] = w >= min_weight ? sdf_sum[a + m] / w : NAN;
    }
  }
}

// A = R K^-1 / voxel_size (3x3, out[0..8]) and g0 = (t - origin) / voxel_size (out[9..11]) of one view: fp64, each of
// the twelve rounded once; K's bottom row is taken to be (0,0,1) (the adjugate inverse of the top-left 3x3)
__device__ inline void raycast_camera(const float *K, const float *T, float voxel_size, float ox, float oy, float oz,
                                      float *out) {
  double Ki[9];
  inv3_d(K, Ki);
  const double vs = (double)voxel_size;
  const double o[3] = {(double)ox, (double)oy, (double)oz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
      out[a * 3 + b] = (float)((((double)T[a * 4 + 0] * Ki[b] + (double)T[a * 4 + 1] * Ki[3 + b]) +
                                (double)T[a * 4 + 2] * Ki[6 + b]) / vs);
    out[9 + a] = (float)(((double)T[a * 4 + 3] - o[a]) / vs);
  }
}

template <bool COLOR>
__global__ __launch_bounds__(TR_THREADS) void tsdf_raycast_kernel(
    const float *__restrict__ d, const float *__restrict__ sdf_sum, const float *__restrict__ weight,
    const float *__restrict__ color_sum, int nx, int ny, int nz, float voxel_size, float ox, float oy, float oz,
    const float *__restrict__ K, const float *__restrict__ T, int rows, int cols, int tiles_x, float min_weight,
    float min_depth, float max_depth, float step, int max_count, float *__restrict__ depth,
    float *__restrict__ normals, float *__restrict__ colors, float *__restrict__ weight_out) {
  __shared__ float scam[12];
  const int view = blockIdx.z;
  if (threadIdx.x == 0) raycast_camera(K + (size_t)view * 16, T + (size_t)view * 16, voxel_size, ox, oy, oz, scam);
  __syncthreads();
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = tile_x * TR_TILE + (wave & 1) * 8 + (lane & 7);
  const int y = tile_y * TR_TILE + (wave >> 1) * 8 + (lane >> 3);
  if (x >= cols || y >= rows) return;                               // (after the only barrier)

  const float xf = (float)x, yf = (float)y;
  float dir[3], g0[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    dir[a] = fmaf(scam[a * 3 + 0], xf, fmaf(scam[a * 3 + 1], yf, scam[a * 3 + 2]));
    g0[a] = scam[9 + a];
  }
  const float top[3] = {(float)(nx - 2), (float)(ny - 2), (float)(nz - 2)};   // the highest lowest corner of a cell

  // The slab test in fp64: a sample is in range only where 0 <= g_a < N_a - 1 on every axis, and the sign of
  // fmaf(t, dir, g0) - bound is that of the exact expression, so the exact interval holds every sample in range.
  // t_k = (float)k * step lies within one step of k * step for k < 2^24; the interval is widened by two steps.
  const double sd = (double)step;
  double t_in = fmax((double)min_depth, 0.0), t_out = fmin((double)max_depth, (double)(TR_MAX_EXTENT - 1) * sd);
  bool any = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double lo = -(double)g0[a], hi = (double)top[a] + 1.0 - (double)g0[a];
    if (dir[a] == 0.0f) {                                           // along a grid axis: g_a = g0_a for every t
      any = any && lo <= 0.0 && hi > 0.0;
    } else {
      const double t1 = lo / (double)dir[a], t2 = hi / (double)dir[a];
      t_in = fmax(t_in, fmin(t1, t2));
      t_out = fmin(t_out, fmax(t1, t2));
    }
    any = any && fabsf(dir[a]) <= TR_FLT_MAX && fabsf(g0[a]) <= TR_FLT_MAX;   // (a NaN fails)
  }
  any = any && t_in <= t_out;                                       // (a NaN fails)
  const double k_in = fmax(floor(t_in / sd) - 2.0, 1.0), k_out = fmin(ceil(t_out / sd) + 2.0, (double)(TR_MAX_EXTENT - 1));
  any = any && k_in <= k_out;
  const int k_first = any ? (int)k_in : 1;
  // (the entry has checked that no ray holds more than max_count samples inside the widened box: the clamp is the
  // loop's own bound, whatever the cameras hold)
  const int k_last = any ? (int)fmin(k_out, k_in + (double)(max_count - 1)) : 0;

  const long lnx = nx, nxy = (long)nx * ny;
  float f_prev = NAN, t_prev = 0.0f, t_hit = 0.0f;
  bool hit = false;
  for (int k = k_first; k <= k_last; ++k) {
    const float t = (float)k * step;
    if (!(t > min_depth)) continue;
    if (!(t <= max_depth)) break;                                   // (t_k does not decrease with k)
    const float gx = fmaf(t, dir[0], g0[0]), gy = fmaf(t, dir[1], g0[1]), gz = fmaf(t, dir[2], g0[2]);
    const float cx = floorf(gx), cy = floorf(gy), cz = floorf(gz);
    const bool in = cx >= 0.0f && cx <= top[0] && cy >= 0.0f && cy <= top[1] && cz >= 0.0f && cz <= top[2];
    float f = NAN;                                                  // NaN: not in range, or a corner unobserved
    if (in) {                                                       // (nothing is loaded for a sample out of range)
      float v[8];
      cell_load(d, ((long)cz * ny + (long)cy) * lnx + (long)cx, lnx, nxy, v);
      f = trilinear(v, gx - cx, gy - cy, gz - cz);
    }
    if (f_prev >= 0.0f && f < 0.0f) {
      t_hit = fmaf(step, f_prev / (f_prev - f), t_prev);
      hit = true;
      break;
    }
    if (f_prev < 0.0f && f >= 0.0f) break;                          // seen from behind: the ray ends without a hit
    f_prev = f, t_prev = t;
  }

  float out_n[3] = {0.0f, 0.0f, 0.0f}, out_c[3] = {0.0f, 0.0f, 0.0f}, out_w = 0.0f;
  if (hit) {
    const float gx = fmaf(t_hit, dir[0], g0[0]), gy = fmaf(t_hit, dir[1], g0[1]), gz = fmaf(t_hit, dir[2], g0[2]);
    const float cx = floorf(gx), cy = floorf(gy), cz = floorf(gz);
    const bool in = cx >= 0.0f && cx <= top[0] && cy >= 0.0f && cy <= top[1] && cz >= 0.0f && cz <= top[2];
    const long at = in ? ((long)cz * ny + (long)cy) * lnx + (long)cx : 0;
    const float fx = gx - cx, fy = gy - cy, fz = gz - cz;
    float w[8];
    cell_load(weight, at, lnx, nxy, w);
    bool defined = in;
#pragma unroll
    for (int c = 0; c < 8; ++c) defined = defined && w[c] >= min_weight;
    if (defined) {
      float v[8];
      cell_load(sdf_sum, at, lnx, nxy, v);
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] = v[c] / w[c];
      float grad[3];
      trilinear_gradient(v, fx, fy, fz, grad);
      const float len = sqrtf(fmaf(grad[0], grad[0], fmaf(grad[1], grad[1], grad[2] * grad[2])));
      const bool unit = len > 0.0f && len <= TR_FLT_MAX;
#pragma unroll
      for (int m = 0; m < 3; ++m) out_n[m] = unit ? grad[m] / len : 0.0f;
      out_w = trilinear(w, fx, fy, fz);
      if (COLOR) {
        const size_t plane = (size_t)nxy * nz;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          float c[8];
          cell_load(color_sum + ch * plane, at, lnx, nxy, c);
#pragma unroll
          for (int m = 0; m < 8; ++m) c[m] = c[m] / w[m];
          out_c[ch] = trilinear(c, fx, fy, fz);
        }
      }
    }
  }
  const size_t P = (size_t)rows * cols, pix = (size_t)y * cols + x;
  depth[view * P + pix] = hit ? t_hit : 0.0f;
  weight_out[view * P + pix] = out_w;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    normals[((size_t)view * 3 + m) * P + pix] = out_n[m];
    if (COLOR) colors[((size_t)view * 3 + m) * P + pix] = out_c[m];
  }
}

// no ray holds more samples inside the box than this: its length in depth is at most its metric length (the camera
// ray's z component is 1), which is at most the box's diagonal
inline double raycast_samples(int nx, int ny, int nz, float voxel_size, float step) {
  const double ex = nx - 1, ey = ny - 1, ez = nz - 1;
  return (double)voxel_size * sqrt(ex * ex + ey * ey + ez * ez) / (double)step + 2.0;
}

}  // namespace mvsn

extern "C" size_t mvsn_tsdf_raycast_workspace_bytes(int nx, int ny, int nz) {
  if (!mvsn::raycast_dims_ok(nx, ny, nz)) return 0;
  return mvsn::align256(sizeof(float) * (size_t)nx * ny * nz);
}

extern "C" int mvsn_tsdf_raycast(const float *sdf_sum, const float *weight, const float *color_sum, int nx, int ny,
                                 int nz, float voxel_size, float origin_x, float origin_y, float origin_z,
                                 const float *K, const float *T_cam_in_world, int n_views, int rows, int cols,
                                 float min_weight, float min_depth, float max_depth, float step, void *workspace,
                                 size_t workspace_bytes, float *depth, float *normals, float *colors,
                                 float *weight_out, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(sdf_sum && weight && K && T_cam_in_world && depth && normals && weight_out, MVSN_E_BADARG,
               "mvsn_tsdf_raycast: null pointer");
  MVSN_REQUIRE(!colors == !color_sum, MVSN_E_BADARG, "mvsn_tsdf_raycast: colours and color_sum go together");
  MVSN_REQUIRE(n_views > 0 && rows > 0 && cols > 0, MVSN_E_BADARG, "mvsn_tsdf_raycast: bad sizes (views %d, %d x %d)",
               n_views, rows, cols);
  MVSN_REQUIRE(n_views <= 65535 && (long)rows * cols <= 0x7fffffffL && rows <= TR_MAX_EXTENT && cols <= TR_MAX_EXTENT,
               MVSN_E_TOOLARGE,
               "mvsn_tsdf_raycast: %d views of %d x %d pixels (at most 65535 views of 2^31 - 1 pixels, 2^24 along an axis)",
               n_views, rows, cols);
  MVSN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, MVSN_E_BADARG, "mvsn_tsdf_raycast: dims %d x %d x %d (at least 2 each)", nx,
               ny, nz);
  MVSN_REQUIRE(raycast_dims_ok(nx, ny, nz), MVSN_E_TOOLARGE,
               "mvsn_tsdf_raycast: %d x %d x %d voxels (at most 2^31 - 1, 2^24 along an axis)", nx, ny, nz);
  MVSN_REQUIRE(raycast_positive(voxel_size) && raycast_positive(min_weight) && raycast_positive(step), MVSN_E_BADARG,
               "mvsn_tsdf_raycast: voxel size %g, min_weight %g or step %g is not a positive finite number",
               (double)voxel_size, (double)min_weight, (double)step);
  MVSN_REQUIRE(fabsf(origin_x) <= TR_FLT_MAX && fabsf(origin_y) <= TR_FLT_MAX && fabsf(origin_z) <= TR_FLT_MAX &&
                   fabsf(min_depth) <= TR_FLT_MAX,
               MVSN_E_BADARG, "mvsn_tsdf_raycast: origin or min_depth is not finite");
  MVSN_REQUIRE(max_depth > min_depth, MVSN_E_BADARG, "mvsn_tsdf_raycast: max_depth %g is not above min_depth %g",
               (double)max_depth, (double)min_depth);
  const double samples = raycast_samples(nx, ny, nz, voxel_size, step);
  MVSN_REQUIRE(samples <= (double)TR_MAX_SAMPLES, MVSN_E_TOOLARGE,
               "mvsn_tsdf_raycast: up to %.0f samples on a ray (at most 2^20): a larger step", samples);
  const long n = (long)nx * ny * nz;
  const size_t need = align256(sizeof(float) * (size_t)n);
  MVSN_REQUIRE(workspace && workspace_bytes >= need, MVSN_E_WORKSPACE,
               "mvsn_tsdf_raycast: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  MVSN_REQUIRE(((uintptr_t)workspace & 15) == 0, MVSN_E_BADARG, "mvsn_tsdf_raycast: workspace not 16-byte aligned");
  float *d = (float *)workspace;
  const hipStream_t st = (hipStream_t)stream;
  const long items = (n + TR_VOX - 1) / TR_VOX;
  hipLaunchKernelGGL(tsdf_values_kernel, dim3((unsigned)((items + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, st,
                     sdf_sum, weight, n, min_weight, d);
  if (int e = check_launch("mvsn_tsdf_raycast: values")) return e;
  const int tiles_x = (cols + TR_TILE - 1) / TR_TILE, tiles_y = (rows + TR_TILE - 1) / TR_TILE;
  const dim3 grid((unsigned)((long)tiles_x * tiles_y), 1, (unsigned)n_views);
  const int max_count = (int)samples + TR_SLACK;
  if (color_sum)
    hipLaunchKernelGGL(tsdf_raycast_kernel<true>, grid, dim3(TR_THREADS), 0, st, (const float *)d, sdf_sum, weight,
                       color_sum, nx, ny, nz, voxel_size, origin_x, origin_y, origin_z, K, T_cam_in_world, rows, cols,
                       tiles_x, min_weight, min_depth, max_depth, step, max_count, depth, normals, colors, weight_out);
  else
    hipLaunchKernelGGL(tsdf_raycast_kernel<false>, grid, dim3(TR_THREADS), 0, st, (const float *)d, sdf_sum, weight,
                       color_sum, nx, ny, nz, voxel_size, origin_x, origin_y, origin_z, K, T_cam_in_world, rows, cols,
                       tiles_x, min_weight, min_depth, max_depth, step, max_count, depth, normals, colors, weight_out);
  return check_launch("mvsn_tsdf_raycast: march");
}
