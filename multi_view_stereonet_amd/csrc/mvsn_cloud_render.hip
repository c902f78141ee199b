// A cloud rendered into posed cameras, and the occlusion test of its points against depth maps (see include/mvsn_hip.h:
// mvsn_cloud_render*, mvsn_cloud_visibility; the semantics, every fp32 step and the arguments are DESIGN.md section 25).
//
//   mvsn_cloud_render, three launches on a workspace of one 64-bit key per pixel per view:
//   render_clear_kernel     every key = all ones (the workspace arrives uninitialised)
//   render_splat_kernel     one thread per point, looping over the views; the cameras (P = K T^-1 as a 3x4, fp64,
//                           rounded once: tsdf_camera of mvsn_camera.h, the TSDF integration's) are staged in LDS
//                           RD_CAM_BATCH at a time, so the point's 12 bytes are read once for all views.  For every pixel
//                           of the (2R+1)^2 square around the point's nearest pixel that lies inside the map:
//                           atomicMin(key, (bits of z << 32) | row), skipped when a load of the key shows that it would
//                           not be lowered
//   render_resolve_kernel   one thread per pixel: the winner's z and row, and its colour and normal, or the miss values
//   mvsn_cloud_visibility, one launch, no workspace and no atomics:
//   visibility_kernel       one thread per point, looping over the views in order with the cameras staged the same way:
//                           the point's z against the depth at its nearest pixel; with maps, the mean of their samples
//                           over the views that see the point
//
// The projection is section 15's for a voxel centre, restated here operation for operation (mvsn_tsdf.hip splits each
// row into a part that the four voxels of a thread share and a last fused multiply-add per voxel; a point has nothing
// to share, and the three nested fmaf below are the same three operations in the same order).  Only the camera itself
// is shared code.
//
// The only atomic is the 64-bit integer minimum.  min is associative and commutative and a key is a function of the
// point and the view alone, so a pixel's final key is the least key of the points that reach it whatever the order of
// the points and of the atomics; every output is a function of the final keys.
//
// Contraction is off for the whole file: every fused multiply-add is written as fmaf, every other step is one fp32
// operation.
#pragma clang fp contract(off)
#include "mvsn_common.h"
#include "mvsn_camera.h"
#include "mvsn_geom.h"

namespace mvsn {

constexpr int RD_THREADS = 256;
constexpr int RD_CAM_BATCH = 32;                        // cameras staged in LDS at once
constexpr float RD_FLT_MAX = 3.4028234e38f;
constexpr int RD_MAX_EXTENT = 1 << 24;                  // rows and cols up to here
constexpr float RD_PIXEL_LIMIT = 33554432.0f;           // 2^25: an integer-valued float within it converts exactly
constexpr long RD_MAX_POINTS = 0x7fffffffL;             // a row is the low word of a key
constexpr unsigned RD_MAX_BLOCKS = 1u << 20;            // of the two per-pixel kernels, which stride over the rest
constexpr unsigned long long RD_EMPTY = ~0ull;          // never a real key: z is finite, so its bits are below 0x7f800000

#ifdef MVSN_RENDER_COUNT
// [0] candidates (point, view, pixel inside the map), [1] atomics issued; a debug build's figures, never reset by a call
__device__ unsigned long long render_debug_counts[2];
#endif

// a point's nearest pixel in one staged camera
struct RenderTap {
  float z;
  int row, col;       // valid only when ok
  bool ok;            // takes part: z finite, min_depth < z <= max_depth, the pixel within `radius` of the map
};

// z = P row 2 . (p,1); (u, v) = rows 0, 1 over z; col = floor(u + 0.5), row = floor(v + 0.5): section 15's steps.  The
// pixel is compared as a float first (a NaN fails, 1e30 pixels fail) and, once known to be an exact small integer, against
// the map as an integer: -radius <= col < cols + radius holds exactly, which (float)(cols + radius) could not promise
// above 2^24.
__device__ __forceinline__ RenderTap render_project(const float *Pm, float x, float y, float zw, bool finite,
                                                    float min_depth, float max_depth, int rows, int cols, int radius) {
  RenderTap t;
  const float a0 = fmaf(Pm[0], x, fmaf(Pm[1], y, fmaf(Pm[2], zw, Pm[3])));
  const float a1 = fmaf(Pm[4], x, fmaf(Pm[5], y, fmaf(Pm[6], zw, Pm[7])));
  t.z = fmaf(Pm[8], x, fmaf(Pm[9], y, fmaf(Pm[10], zw, Pm[11])));
  const float u = a0 / t.z, v = a1 / t.z;
  const float fc = floorf(u + 0.5f), fr = floorf(v + 0.5f);
  // (a NaN fails every comparison)
  const bool small = fabsf(fc) <= RD_PIXEL_LIMIT && fabsf(fr) <= RD_PIXEL_LIMIT;
  t.col = small ? (int)fc : 0;
  t.row = small ? (int)fr : 0;
  t.ok = finite && small && t.z > min_depth && t.z <= max_depth && t.z <= RD_FLT_MAX && t.col >= -radius &&
         t.col < cols + radius && t.row >= -radius && t.row < rows + radius;
  return t;
}

__global__ __launch_bounds__(RD_THREADS) void render_clear_kernel(unsigned long long *__restrict__ keys, size_t total) {
  const size_t stride = (size_t)gridDim.x * RD_THREADS;
  for (size_t i = (size_t)blockIdx.x * RD_THREADS + threadIdx.x; i < total; i += stride) keys[i] = RD_EMPTY;
}

__global__ __launch_bounds__(RD_THREADS) void render_splat_kernel(
    const float *__restrict__ points, long n, const float *__restrict__ K, const float *__restrict__ T, int n_views,
    int rows, int cols, int radius, float min_depth, float max_depth, unsigned long long *keys) {
  __shared__ float scam[RD_CAM_BATCH * TS_CAM];
  const long i = (long)blockIdx.x * RD_THREADS + threadIdx.x;
  const long at = min(i, n - 1);                                    // (a thread past the end projects and writes nothing)
  const float x = points[(size_t)at * 3], y = points[(size_t)at * 3 + 1], zw = points[(size_t)at * 3 + 2];
  const bool finite = i < n && fabsf(x) <= RD_FLT_MAX && fabsf(y) <= RD_FLT_MAX && fabsf(zw) <= RD_FLT_MAX;
  const size_t P = (size_t)rows * cols;
#ifdef MVSN_RENDER_COUNT
  unsigned long long candidates = 0, atomics = 0;
#endif

  for (int base = 0; base < n_views; base += RD_CAM_BATCH) {        // bounded: ceil(V / RD_CAM_BATCH) rounds
    const int batch = min(RD_CAM_BATCH, n_views - base);
    __syncthreads();                                                // (the previous batch has been read)
    if (threadIdx.x < batch)
      tsdf_camera(K + (size_t)(base + threadIdx.x) * 16, T + (size_t)(base + threadIdx.x) * 16,
                  scam + threadIdx.x * TS_CAM);
    __syncthreads();
    for (int cam = 0; cam < batch; ++cam) {
      const RenderTap t =
          render_project(scam + cam * TS_CAM, x, y, zw, finite, min_depth, max_depth, rows, cols, radius);
      if (!t.ok) continue;
      // z > 0, so its bits order as unsigned integers the way the values do; a tie on z goes to the lowest row
      const unsigned long long key = ((unsigned long long)__float_as_uint(t.z) << 32) | (unsigned long long)i;
      unsigned long long *view_keys = keys + (size_t)(base + cam) * P;
      const int r0 = max(t.row - radius, 0), r1 = min(t.row + radius, rows - 1);      // the square clipped to the map:
      const int c0 = max(t.col - radius, 0), c1 = min(t.col + radius, cols - 1);      // every index below is inside
      for (int r = r0; r <= r1; ++r) {
        for (int c = c0; c <= c1; ++c) {
          unsigned long long *slot = view_keys + (size_t)r * cols + c;
          // Keys only ever decrease between the clear and the resolve.  A stale value of the load is therefore never
          // below the key's current value: when it is <= ours, so is the current one, and the atomic would change
          // nothing; when it is above ours although the current one is not, the atomic is issued and changes nothing.
          // A stale read can cause a superfluous atomic, never a wrong skip.  The argument needs the value to be one
          // the slot really held: the load is a relaxed device-scope atomic one, which cannot return half of one key and
          // half of another (on a tie in z such a mixture could sort below the true key and drop a winner).  It is served
          // past the CU's L1.  Measured (section 25), an ordinary cached load skips as often and is 0 to 3 % faster.
#if defined(MVSN_RENDER_NO_SKIP)                                   // (the A/Bs of DESIGN.md section 25: every candidate an atomic,
          const unsigned long long seen = RD_EMPTY;
#elif defined(MVSN_RENDER_PLAIN_LOAD)                              // and the skip on an ordinary cached load)
          const unsigned long long seen = *slot;
#else
          const unsigned long long seen = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
#ifdef MVSN_RENDER_COUNT
          ++candidates;
#endif
          if (seen <= key) continue;
          atomicMin(slot, key);
#ifdef MVSN_RENDER_COUNT
          ++atomics;
#endif
        }
      }
    }
  }
#ifdef MVSN_RENDER_COUNT
  if (candidates) atomicAdd(render_debug_counts + 0, candidates);
  if (atomics) atomicAdd(render_debug_counts + 1, atomics);
#endif
}

template <bool COLOR, bool NORMAL>
__global__ __launch_bounds__(RD_THREADS) void render_resolve_kernel(
    const unsigned long long *__restrict__ keys, size_t total, size_t P, long n, const uint8_t *__restrict__ colors,
    const float *__restrict__ normals, float *__restrict__ depth, int64_t *__restrict__ index,
    uint8_t *__restrict__ out_colors, float *__restrict__ out_normals) {
  const size_t stride = (size_t)gridDim.x * RD_THREADS;
  for (size_t i = (size_t)blockIdx.x * RD_THREADS + threadIdx.x; i < total; i += stride) {
    const unsigned long long key = keys[i];
    const long row = (long)(key & 0xffffffffull);
    const bool hit = key != RD_EMPTY && row < n;                    // (a key the splat wrote always names a row)
    depth[i] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
    index[i] = hit ? (int64_t)row : (int64_t)-1;
    if (COLOR || NORMAL) {
      const size_t v = i / P, pix = i - v * P;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        if (COLOR) out_colors[(v * 3 + ch) * P + pix] = hit ? colors[(size_t)row * 3 + ch] : (uint8_t)0;
        if (NORMAL) out_normals[(v * 3 + ch) * P + pix] = hit ? normals[(size_t)row * 3 + ch] : 0.0f;
      }
    }
  }
}

constexpr int VIS_MAX_CHANNELS = 16;

template <bool MAPS>
__global__ __launch_bounds__(RD_THREADS) void visibility_kernel(
    const float *__restrict__ points, long n, const float *__restrict__ depth, const float *__restrict__ maps,
    int channels, const float *__restrict__ K, const float *__restrict__ T, int n_views, int rows, int cols,
    float rel_tol, float min_depth, uint8_t *__restrict__ visible, int *__restrict__ count,
    float *__restrict__ values) {
  __shared__ float scam[RD_CAM_BATCH * TS_CAM];
  const long i = (long)blockIdx.x * RD_THREADS + threadIdx.x;
  const long at = min(i, n - 1);
  const float x = points[(size_t)at * 3], y = points[(size_t)at * 3 + 1], zw = points[(size_t)at * 3 + 2];
  const bool finite = i < n && fabsf(x) <= RD_FLT_MAX && fabsf(y) <= RD_FLT_MAX && fabsf(zw) <= RD_FLT_MAX;
  const size_t P = (size_t)rows * cols;
  int seen = 0;
  float sum[VIS_MAX_CHANNELS];
#pragma unroll
  for (int c = 0; c < VIS_MAX_CHANNELS; ++c) sum[c] = 0.0f;

  for (int base = 0; base < n_views; base += RD_CAM_BATCH) {        // bounded: ceil(V / RD_CAM_BATCH) rounds
    const int batch = min(RD_CAM_BATCH, n_views - base);
    __syncthreads();                                                // (the previous batch has been read)
    if (threadIdx.x < batch)
      tsdf_camera(K + (size_t)(base + threadIdx.x) * 16, T + (size_t)(base + threadIdx.x) * 16,
                  scam + threadIdx.x * TS_CAM);
    __syncthreads();
    for (int cam = 0; cam < batch; ++cam) {                         // view order: the sums are bitwise reproducible
      const int v = base + cam;
      // radius 0: taking part puts the pixel inside the map
      const RenderTap t = render_project(scam + cam * TS_CAM, x, y, zw, finite, min_depth, RD_FLT_MAX, rows, cols, 0);
      const size_t pix = t.ok ? (size_t)t.row * cols + t.col : 0;   // always inside the maps
      const float D = depth[(size_t)v * P + pix];
      const bool vis = t.ok && D > 0.0f && D <= RD_FLT_MAX && t.z <= fmaf(rel_tol, D, D);
      if (i < n) visible[(size_t)i * n_views + v] = vis ? 1 : 0;
      seen += vis;
      if (MAPS && vis) {
        const float *m = maps + (size_t)v * channels * P + pix;
#pragma unroll
        for (int c = 0; c < VIS_MAX_CHANNELS; ++c)
          if (c < channels) sum[c] = sum[c] + m[(size_t)c * P];     // (a sample that is not finite is added like any other)
      }
    }
  }
  if (i >= n) return;
  count[i] = seen;
  if (MAPS) {
    const float by = (float)seen;
#pragma unroll
    for (int c = 0; c < VIS_MAX_CHANNELS; ++c)
      if (c < channels) values[(size_t)i * channels + c] = seen > 0 ? sum[c] / by : 0.0f;
  }
}

// the limits that both entries share; who = the entry's name
static int render_check_sizes(const char *who, long n, int n_views, int rows, int cols) {
  MVSN_REQUIRE(n >= 1 && n <= RD_MAX_POINTS, MVSN_E_BADARG, "%s: %ld points (1 to 2^31 - 1)", who, n);
  MVSN_REQUIRE(n_views >= 1 && n_views <= 65535, MVSN_E_BADARG, "%s: %d views (1 to 65535)", who, n_views);
  MVSN_REQUIRE(rows >= 1 && cols >= 1 && rows <= RD_MAX_EXTENT && cols <= RD_MAX_EXTENT &&
                   (long)rows * cols <= 0x7fffffffL,
               MVSN_E_BADARG, "%s: maps of %d x %d pixels (1 to 2^24 along an axis, at most 2^31 - 1 pixels)", who, rows,
               cols);
  return 0;
}

inline size_t render_bytes(int n_views, int rows, int cols) {
  return sizeof(unsigned long long) * (size_t)n_views * (size_t)rows * (size_t)cols;   // one key per pixel per view
}

}  // namespace mvsn

extern "C" int mvsn_cloud_render_camera_batch(void) { return mvsn::RD_CAM_BATCH; }

extern "C" size_t mvsn_cloud_render_workspace_bytes(int n_views, int rows, int cols) {
  using namespace mvsn;
  if (n_views < 1 || n_views > 65535 || rows < 1 || cols < 1 || rows > RD_MAX_EXTENT || cols > RD_MAX_EXTENT ||
      (long)rows * cols > 0x7fffffffL)
    return 0;
  return render_bytes(n_views, rows, cols);
}

extern "C" int mvsn_cloud_render(const float *points, long n, const uint8_t *colors, const float *normals,
                                 const float *K, const float *T_cam_in_world, int n_views, int rows, int cols,
                                 int radius, float min_depth, float max_depth, void *workspace, size_t workspace_bytes,
                                 float *depth, int64_t *index, uint8_t *out_colors, float *out_normals,
                                 mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_render";
  MVSN_REQUIRE(points && K && T_cam_in_world && depth && index, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(!colors == !out_colors && !normals == !out_normals, MVSN_E_BADARG,
               "%s: colors and out_colors go together, and normals and out_normals", who);
  if (int e = render_check_sizes(who, n, n_views, rows, cols)) return e;
  MVSN_REQUIRE(radius >= 0 && radius <= MVSN_RENDER_MAX_RADIUS, MVSN_E_BADARG, "%s: radius %d (0 to %d)", who, radius,
               MVSN_RENDER_MAX_RADIUS);
  // (a NaN fails both)
  MVSN_REQUIRE(min_depth >= 0.0f && min_depth <= RD_FLT_MAX, MVSN_E_BADARG,
               "%s: min_depth %g is not a finite number >= 0", who, (double)min_depth);
  MVSN_REQUIRE(max_depth > 0.0f, MVSN_E_BADARG, "%s: max_depth %g is not a number > 0 (+inf: no limit)", who,
               (double)max_depth);
  const size_t need = render_bytes(n_views, rows, cols);
  MVSN_REQUIRE(workspace && workspace_bytes >= need, MVSN_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who,
               workspace_bytes, need);
  MVSN_REQUIRE(((uintptr_t)workspace & 15) == 0, MVSN_E_BADARG, "%s: workspace not 16-byte aligned", who);
  unsigned long long *keys = (unsigned long long *)workspace;
  const size_t P = (size_t)rows * cols, total = (size_t)n_views * P;
  const size_t pixel_blocks = (total + RD_THREADS - 1) / RD_THREADS;
  const dim3 pixel_grid((unsigned)(pixel_blocks < RD_MAX_BLOCKS ? pixel_blocks : RD_MAX_BLOCKS)), block(RD_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(render_clear_kernel, pixel_grid, block, 0, st, keys, total);
  if (int e = check_launch("mvsn_cloud_render: clear")) return e;
  hipLaunchKernelGGL(render_splat_kernel, dim3((unsigned)((n + RD_THREADS - 1) / RD_THREADS)), block, 0, st, points, n, K,
                     T_cam_in_world, n_views, rows, cols, radius, min_depth, max_depth, keys);
  if (int e = check_launch("mvsn_cloud_render: splat")) return e;
#define MVSN_RESOLVE(C, N)                                                                                              \
  hipLaunchKernelGGL((render_resolve_kernel<C, N>), pixel_grid, block, 0, st, (const unsigned long long *)keys, total, P, \
                     n, colors, normals, depth, index, out_colors, out_normals)
  if (colors && normals) MVSN_RESOLVE(true, true);
  else if (colors) MVSN_RESOLVE(true, false);
  else if (normals) MVSN_RESOLVE(false, true);
  else MVSN_RESOLVE(false, false);
#undef MVSN_RESOLVE
  return check_launch("mvsn_cloud_render: resolve");
}

extern "C" int mvsn_cloud_visibility(const float *points, long n, const float *depth, const float *maps, int channels,
                                     const float *K, const float *T_cam_in_world, int n_views, int rows, int cols,
                                     float rel_tol, float min_depth, uint8_t *visible, int *count, float *values,
                                     mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_visibility";
  MVSN_REQUIRE(points && depth && K && T_cam_in_world && visible && count, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(!maps == !values, MVSN_E_BADARG, "%s: maps and values go together", who);
  MVSN_REQUIRE(maps ? channels >= 1 && channels <= VIS_MAX_CHANNELS : channels == 0, MVSN_E_BADARG,
               "%s: %d channels (1 to %d with maps, 0 without)", who, channels, VIS_MAX_CHANNELS);
  if (int e = render_check_sizes(who, n, n_views, rows, cols)) return e;
  MVSN_REQUIRE(rel_tol >= 0.0f && rel_tol <= RD_FLT_MAX && min_depth >= 0.0f && min_depth <= RD_FLT_MAX, MVSN_E_BADARG,
               "%s: rel_tol %g or min_depth %g is not a finite number >= 0", who, (double)rel_tol, (double)min_depth);
  const dim3 grid((unsigned)((n + RD_THREADS - 1) / RD_THREADS)), block(RD_THREADS);
  if (maps)
    hipLaunchKernelGGL(visibility_kernel<true>, grid, block, 0, (hipStream_t)stream, points, n, depth, maps, channels, K,
                       T_cam_in_world, n_views, rows, cols, rel_tol, min_depth, visible, count, values);
  else
    hipLaunchKernelGGL(visibility_kernel<false>, grid, block, 0, (hipStream_t)stream, points, n, depth, maps, channels, K,
                       T_cam_in_world, n_views, rows, cols, rel_tol, min_depth, visible, count, values);
  return check_launch("mvsn_cloud_visibility");
}

#ifdef MVSN_RENDER_COUNT
// debug builds only (-DMVSN_RENDER_COUNT): out[0] = candidates, out[1] = atomics since the library was loaded
extern "C" int mvsn_cloud_render_debug_counts(unsigned long long *out) {
  const hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(mvsn::render_debug_counts), 2 * sizeof(unsigned long long));
  return e == hipSuccess ? 0 : (int)e;
}
#endif
