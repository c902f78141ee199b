// A triangle mesh rendered into posed cameras: per pixel the z-depth of the nearest face, its row, the perspective-correct
// barycentric weights, and the interpolated vertex normal and colour (see include/mvsn_hip.h: mvsn_mesh_render*; the
// semantics, every operation and the arguments are DESIGN.md section 27).
//
//   mvsn_mesh_render, three launches on a workspace of one 64-bit key per pixel per view and one counter per view:
//   mesh_clear_kernel       every key = all ones, every counter = 0 (the workspace arrives uninitialised)
//   mesh_raster_kernel      one thread per face, looping over the views; the cameras (tsdf_camera of mvsn_camera.h, the
//                           cloud render's) are staged in LDS MR_CAM_BATCH at a time, so the face's three vertices are
//                           read once for all views.  The three vertices are projected with section 25's steps and snapped
//                           to 1/256 of a pixel; coverage is decided on the snapped integers alone.  A face whose clipped
//                           box holds at most MR_SMALL_PIXELS pixels is walked by its own thread; a larger one is handed
//                           to the wave: the wave loops over the ballot of lanes that hold one, broadcasts that lane's six
//                           snapped coordinates and three z, and its 64 lanes stride over the box.  For every covered
//                           pixel whose z lies in (min_depth, max_depth]: atomicMin(key, (bits of z << 32) | face row),
//                           skipped when a load of the key shows that it would not be lowered (section 25's argument)
//   mesh_resolve_kernel     one thread per pixel: the winner's z and row; the winner is projected again in the pixel's view
//                           by the same device functions, which gives the same bits, and the weights, the normal and the
//                           colour are formed from there.  Nothing but keys and counters lives in the workspace
//
// The only atomics are the 64-bit integer minimum and the integer sum of the faces that the near plane or the guard band
// removed.  A key is a function of (face, view, pixel) alone, so a pixel's final key is the least key of the faces that
// cover it whatever the order of the faces and of the atomics, and whichever of the two paths rasterised a face.
//
// Contraction is off for the whole file: every fused multiply-add is written as fmaf, every other step is one operation.
// No scratch, every loop bounded by the clipped box, by 64 (the ballot) or by the number of views.
#pragma clang fp contract(off)
#include "mvsn_common.h"
#include "mvsn_camera.h"
#include "mvsn_geom.h"
#include "mvsn_mesh.h"

namespace mvsn {

constexpr int MR_THREADS = 256;
constexpr int MR_CAM_BATCH = 32;                        // cameras staged in LDS at once
constexpr int MR_SMALL_PIXELS = 32;                     // a clipped box of more pixels goes to the whole wave (tuning only)
constexpr float MR_FLT_MAX = 3.4028234e38f;
constexpr float MR_GUARD = 65536.0f;                    // |u|, |v| up to here: 2^24 once snapped
constexpr float MR_SUBPIXEL = 256.0f;                   // 8 sub-pixel bits
constexpr int MR_MAX_EXTENT = 1 << 15;                  // rows and cols up to here: the guard band is at least a map wide
constexpr unsigned MR_MAX_BLOCKS = 1u << 20;            // of the two per-pixel kernels, which stride over the rest
constexpr unsigned long long MR_EMPTY = ~0ull;          // never a real key: z is finite, so its bits are below 0x7f800000

// a face in one view, in its own vertex order
struct MrSnap {
  int X[3], Y[3];     // rintf(256 u), rintf(256 v): |X|, |Y| <= 2^24; 0 unless part
  float zc[3];
  bool part;          // takes part: valid, every zc finite and > min_depth, every |u|, |v| <= 2^16
  bool clipped;       // valid and takes no part although a vertex has zc > min_depth
};

// section 25's projection of the three vertices (three nested fmaf per row, two divisions), the limit compared as floats
// before any conversion (a NaN fails), the snap
__device__ __forceinline__ MrSnap mr_snap(const float *Pm, const float (*p)[3], bool valid, float min_depth) {
  MrSnap s;
  float u[3], v[3];
  bool all = valid, any = false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float x = p[j][0], y = p[j][1], zw = p[j][2];
    const float a0 = fmaf(Pm[0], x, fmaf(Pm[1], y, fmaf(Pm[2], zw, Pm[3])));
    const float a1 = fmaf(Pm[4], x, fmaf(Pm[5], y, fmaf(Pm[6], zw, Pm[7])));
    s.zc[j] = fmaf(Pm[8], x, fmaf(Pm[9], y, fmaf(Pm[10], zw, Pm[11])));
    u[j] = a0 / s.zc[j], v[j] = a1 / s.zc[j];
    const bool front = s.zc[j] > min_depth;
    any = any || front;
    all = all && front && s.zc[j] <= MR_FLT_MAX && fabsf(u[j]) <= MR_GUARD && fabsf(v[j]) <= MR_GUARD;
  }
  s.part = all;
  s.clipped = valid && !all && any;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    s.X[j] = all ? (int)rintf(u[j] * MR_SUBPIXEL) : 0;               // (the scaling is exact, the rounding to nearest even)
    s.Y[j] = all ? (int)rintf(v[j] * MR_SUBPIXEL) : 0;
  }
  return s;
}

// the pixels whose centres can lie in the face: ceil(min / 256) .. floor(max / 256) per axis (the shifts are arithmetic:
// right for negative values), clipped to the map; n = 0 when the face takes no part or the box is empty
struct MrBox {
  int r0, c0, width, n;
};

__device__ __forceinline__ MrBox mr_box(const int *X, const int *Y, bool part, int rows, int cols) {
  const int c0 = max((min(X[0], min(X[1], X[2])) + 255) >> 8, 0), c1 = min(max(X[0], max(X[1], X[2])) >> 8, cols - 1);
  const int r0 = max((min(Y[0], min(Y[1], Y[2])) + 255) >> 8, 0), r1 = min(max(Y[0], max(Y[1], Y[2])) >> 8, rows - 1);
  MrBox b;
  b.r0 = r0, b.c0 = c0, b.width = c1 - c0 + 1;
  b.n = part && c1 >= c0 && r1 >= r0 ? b.width * (r1 - r0 + 1) : 0;  // (at most 2^30)
  return b;
}

// the oriented face: what a pixel is tested against
struct MrTri {
  long X[3], Y[3];    // vertices 1 and 2 swapped when the area is negative
  long A;             // the oriented area, > 0; 0: the face covers nothing
  double q[3];        // 1 / zc, in the face's own order
  bool swapped;
};

__device__ __forceinline__ MrTri mr_tri(const int *X, const int *Y, const float *zc) {
  MrTri t;
  const long A = (long)(X[1] - X[0]) * (long)(Y[2] - Y[0]) - (long)(Y[1] - Y[0]) * (long)(X[2] - X[0]);
  t.swapped = A < 0;
  t.A = t.swapped ? -A : A;
  const int one = t.swapped ? 2 : 1, two = t.swapped ? 1 : 2;
  t.X[0] = X[0], t.X[1] = X[one], t.X[2] = X[two];
  t.Y[0] = Y[0], t.Y[1] = Y[one], t.Y[2] = Y[two];
#pragma unroll
  for (int k = 0; k < 3; ++k) t.q[k] = 1.0 / (double)zc[k];
  return t;
}

// Whether the centre of pixel (r, c) is covered; if so lq[k] = lambda_k q_k in the face's own order and S their sum.  Every
// edge function is below 2^51 in magnitude: exact in int64, and converts to fp64 exactly.
__device__ __forceinline__ bool mr_pixel(const MrTri &t, int r, int c, double *lq, double &S) {
  const long px = 256L * c, py = 256L * r;
  long E[3];                                                         // E[k]: the edge opposite the oriented vertex k
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int p = (k + 1) % 3, q = (k + 2) % 3;
    const long dx = t.X[q] - t.X[p], dy = t.Y[q] - t.Y[p];
    E[k] = dx * (py - t.Y[p]) - dy * (px - t.X[p]);
    // a centre on an edge belongs to the face that traverses the edge upwards, or leftwards where it is level: the
    // neighbour across the edge traverses it the other way, so exactly one of the two owns the centre
    in = in && (E[k] > 0 || (E[k] == 0 && (dy < 0 || (dy == 0 && dx < 0))));
  }
  if (!in) return false;
  const double A = (double)t.A;
  const double l0 = (double)E[0] / A, la = (double)E[1] / A, lb = (double)E[2] / A;
  lq[0] = l0 * t.q[0];
  lq[1] = (t.swapped ? lb : la) * t.q[1];
  lq[2] = (t.swapped ? la : lb) * t.q[2];
  S = (lq[0] + lq[1]) + lq[2];
  return true;
}

// one candidate (face, view, pixel): r and c lie inside the map
__device__ __forceinline__ void mr_try(const MrTri &t, int r, int c, unsigned long long row, unsigned long long *view_keys,
                                       int cols, float min_depth, float max_depth) {
  double lq[3], S;
  if (!mr_pixel(t, r, c, lq, S)) return;
  const float z = (float)(1.0 / S);
  if (!(z > min_depth && z <= max_depth && z <= MR_FLT_MAX)) return;  // (a NaN fails)
  // z > 0, so its bits order as unsigned integers the way the values do; a tie on z goes to the lowest face row
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | row;
  unsigned long long *slot = view_keys + (size_t)r * cols + c;
  // Keys only ever decrease between the clear and the resolve, so a stale value of this load is never below the current
  // one: it can cost a superfluous atomic, never a wrong skip.  A relaxed agent-scope atomic load cannot return half of
  // one key and half of another (DESIGN.md section 25 has the argument in full).
  const unsigned long long seen = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (seen <= key) return;
  atomicMin(slot, key);
}

__global__ __launch_bounds__(MR_THREADS) void mesh_clear_kernel(unsigned long long *__restrict__ keys, size_t total,
                                                                unsigned long long *__restrict__ clipped, int n_views) {
  const size_t stride = (size_t)gridDim.x * MR_THREADS;
  const size_t first = (size_t)blockIdx.x * MR_THREADS + threadIdx.x;
  for (size_t i = first; i < total; i += stride) keys[i] = MR_EMPTY;
  for (size_t i = first; i < (size_t)n_views; i += stride) clipped[i] = 0ull;
}

__global__ __launch_bounds__(MR_THREADS) void mesh_raster_kernel(
    const float *__restrict__ vertices, long m, const int64_t *__restrict__ faces, long f, const float *__restrict__ K,
    const float *__restrict__ T, int n_views, int rows, int cols, float min_depth, float max_depth,
    unsigned long long *keys, unsigned long long *clipped) {
  __shared__ float scam[MR_CAM_BATCH * TS_CAM];
  const long i = (long)blockIdx.x * MR_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int64_t r3[3];
  float p[3][3] = {};
  // (a thread past the end, and a face that takes no part, stay: every lane of a wave reaches the cooperative loop)
  const bool valid = i < f && face_load(vertices, m, faces, i, r3, p);
  const size_t P = (size_t)rows * cols;

  for (int base = 0; base < n_views; base += MR_CAM_BATCH) {        // bounded: ceil(V / MR_CAM_BATCH) rounds
    const int batch = min(MR_CAM_BATCH, n_views - base);
    __syncthreads();                                                // (the previous batch has been read)
    if (threadIdx.x < batch)
      tsdf_camera(K + (size_t)(base + threadIdx.x) * 16, T + (size_t)(base + threadIdx.x) * 16,
                  scam + threadIdx.x * TS_CAM);
    __syncthreads();
    for (int cam = 0; cam < batch; ++cam) {
      const MrSnap s = mr_snap(scam + cam * TS_CAM, p, valid, min_depth);
      // at most one count per (face, view), summed over the wave first
      const unsigned long long lost = __ballot(s.clipped);
      if (lost != 0 && lane == __ffsll((long long)lost) - 1)
        atomicAdd(clipped + base + cam, (unsigned long long)__popcll(lost));
      unsigned long long *view_keys = keys + (size_t)(base + cam) * P;
      const MrBox b = mr_box(s.X, s.Y, s.part, rows, cols);
      const bool large = b.n > MR_SMALL_PIXELS;
      if (b.n > 0 && !large) {                                      // its own thread walks it: at most MR_SMALL_PIXELS steps
        const MrTri t = mr_tri(s.X, s.Y, s.zc);
        if (t.A != 0)
          for (int j = 0; j < b.n; ++j)
            mr_try(t, b.r0 + j / b.width, b.c0 + j % b.width, (unsigned long long)i, view_keys, cols, min_depth, max_depth);
      }
      unsigned long long todo = __ballot(large);                    // the same word in every lane: the loop is uniform
      while (todo != 0) {                                           // bounded: at most 64 rounds
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        int X[3], Y[3];
        float zc[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          X[k] = __shfl(s.X[k], src, 64);
          Y[k] = __shfl(s.Y[k], src, 64);
          zc[k] = __shfl(s.zc[k], src, 64);
        }
        const MrBox o = mr_box(X, Y, true, rows, cols);             // (the lane's own box again: the same integers)
        const MrTri t = mr_tri(X, Y, zc);
        if (t.A == 0) continue;
        const unsigned long long row = (unsigned long long)(i - lane + src);
        for (int j = lane; j < o.n; j += 64)                        // bounded by the clipped box
          mr_try(t, o.r0 + j / o.width, o.c0 + j % o.width, row, view_keys, cols, min_depth, max_depth);
      }
    }
  }
}

template <bool NORMAL, bool COLOR>
__global__ __launch_bounds__(MR_THREADS) void mesh_resolve_kernel(
    const unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ lost,
    const float *__restrict__ vertices, long m, const int64_t *__restrict__ faces, long f, const float *__restrict__ K,
    const float *__restrict__ T, int rows, int cols, float min_depth, const float *__restrict__ normals,
    const uint8_t *__restrict__ colors, float *__restrict__ depth, int64_t *__restrict__ face,
    float *__restrict__ weights, float *__restrict__ out_normals, uint8_t *__restrict__ out_colors,
    int64_t *__restrict__ clipped) {
  __shared__ float scam[TS_CAM];
  const size_t v = blockIdx.y, P = (size_t)rows * cols;
  if (threadIdx.x == 0) {
    tsdf_camera(K + v * 16, T + v * 16, scam);
    if (blockIdx.x == 0) clipped[v] = (int64_t)lost[v];
  }
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * MR_THREADS;
  for (size_t pix = (size_t)blockIdx.x * MR_THREADS + threadIdx.x; pix < P; pix += stride) {
    const unsigned long long key = keys[v * P + pix];
    const long row = (long)(key & 0xffffffffull);
    int64_t r3[3] = {0, 0, 0};
    double w[3] = {0.0, 0.0, 0.0};
    bool hit = false;
    if (key != MR_EMPTY) {                                          // (a key the raster wrote always names a covering face)
      float p[3][3] = {};
      const bool valid = row < f && face_load(vertices, m, faces, row, r3, p);
      const MrSnap s = mr_snap(scam, p, valid, min_depth);
      if (s.part) {
        const MrTri t = mr_tri(s.X, s.Y, s.zc);
        double lq[3], S;
        const unsigned at = (unsigned)pix;                          // (P <= 2^30)
        hit = t.A != 0 && mr_pixel(t, (int)(at / (unsigned)cols), (int)(at % (unsigned)cols), lq, S);
        if (hit) {
#pragma unroll
          for (int k = 0; k < 3; ++k) w[k] = lq[k] / S;
        }
      }
    }
    depth[v * P + pix] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
    face[v * P + pix] = hit ? (int64_t)row : (int64_t)-1;
#pragma unroll
    for (int k = 0; k < 3; ++k) weights[(v * 3 + k) * P + pix] = hit ? (float)w[k] : 0.0f;
    if (NORMAL) {
      float n[3];
      face_normal(normals, r3, w, hit, n);
#pragma unroll
      for (int k = 0; k < 3; ++k) out_normals[(v * 3 + k) * P + pix] = n[k];
    }
    if (COLOR) {
      uint8_t c[3];
      face_color(colors, r3, w, hit, c);
#pragma unroll
      for (int k = 0; k < 3; ++k) out_colors[(v * 3 + k) * P + pix] = c[k];
    }
  }
}

static bool mesh_render_sizes_ok(int n_views, int rows, int cols) {
  return n_views >= 1 && n_views <= 65535 && rows >= 1 && cols >= 1 && rows <= MR_MAX_EXTENT && cols <= MR_MAX_EXTENT;
}

inline size_t mesh_render_bytes(int n_views, int rows, int cols) {   // one key per pixel per view, one counter per view
  return sizeof(unsigned long long) * (size_t)n_views * ((size_t)rows * (size_t)cols + 1);
}

}  // namespace mvsn

extern "C" int mvsn_mesh_render_small_pixels(void) { return mvsn::MR_SMALL_PIXELS; }

extern "C" size_t mvsn_mesh_render_workspace_bytes(int n_views, int rows, int cols) {
  return mvsn::mesh_render_sizes_ok(n_views, rows, cols) ? mvsn::mesh_render_bytes(n_views, rows, cols) : 0;
}

extern "C" int mvsn_mesh_render(const float *vertices, long n_vertices, const int64_t *faces, long n_faces,
                                const float *normals, const uint8_t *colors, const float *K, const float *T_cam_in_world,
                                int n_views, int rows, int cols, float min_depth, float max_depth, void *workspace,
                                size_t workspace_bytes, float *depth, int64_t *face, float *weights, float *out_normals,
                                uint8_t *out_colors, int64_t *clipped, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_mesh_render";
  MVSN_REQUIRE(vertices && faces && K && T_cam_in_world && depth && face && weights && clipped, MVSN_E_BADARG,
               "%s: null pointer", who);
  MVSN_REQUIRE(!normals == !out_normals && !colors == !out_colors, MVSN_E_BADARG,
               "%s: normals and out_normals go together, and colors and out_colors", who);
  MVSN_REQUIRE(n_vertices >= 1 && n_vertices <= MESH_MAX_ROWS && n_faces >= 1 && n_faces <= MESH_MAX_ROWS, MVSN_E_BADARG,
               "%s: %ld vertices and %ld faces (1 to 2^31 - 1 each)", who, n_vertices, n_faces);
  MVSN_REQUIRE(n_views >= 1 && n_views <= 65535, MVSN_E_BADARG, "%s: %d views (1 to 65535)", who, n_views);
  MVSN_REQUIRE(mesh_render_sizes_ok(n_views, rows, cols), MVSN_E_BADARG,
               "%s: maps of %d x %d pixels (1 to 2^15 along an axis)", who, rows, cols);
  // (a NaN fails both)
  MVSN_REQUIRE(min_depth >= 0.0f && min_depth <= MR_FLT_MAX, MVSN_E_BADARG,
               "%s: min_depth %g is not a finite number >= 0", who, (double)min_depth);
  MVSN_REQUIRE(max_depth > 0.0f, MVSN_E_BADARG, "%s: max_depth %g is not a number > 0 (+inf: no limit)", who,
               (double)max_depth);
  const size_t need = mesh_render_bytes(n_views, rows, cols);
  if (int e = workspace_check(who, "workspace", workspace, workspace_bytes, need)) return e;
  const size_t P = (size_t)rows * cols, total = (size_t)n_views * P;
  unsigned long long *keys = (unsigned long long *)workspace, *lost = keys + total;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(MR_THREADS);
  const size_t all_blocks = (total + MR_THREADS - 1) / MR_THREADS, view_blocks = (P + MR_THREADS - 1) / MR_THREADS;
  hipLaunchKernelGGL(mesh_clear_kernel, dim3((unsigned)(all_blocks < MR_MAX_BLOCKS ? all_blocks : MR_MAX_BLOCKS)), block, 0,
                     st, keys, total, lost, n_views);
  if (int e = check_launch("mvsn_mesh_render: clear")) return e;
  hipLaunchKernelGGL(mesh_raster_kernel, dim3((unsigned)((n_faces + MR_THREADS - 1) / MR_THREADS)), block, 0, st, vertices,
                     n_vertices, faces, n_faces, K, T_cam_in_world, n_views, rows, cols, min_depth, max_depth, keys, lost);
  if (int e = check_launch("mvsn_mesh_render: raster")) return e;
  const dim3 pixel_grid((unsigned)(view_blocks < MR_MAX_BLOCKS ? view_blocks : MR_MAX_BLOCKS), (unsigned)n_views);
#define MVSN_RESOLVE(N, C)                                                                                                \
  hipLaunchKernelGGL((mesh_resolve_kernel<N, C>), pixel_grid, block, 0, st, (const unsigned long long *)keys,              \
                     (const unsigned long long *)lost, vertices, n_vertices, faces, n_faces, K, T_cam_in_world, rows, cols, \
                     min_depth, normals, colors, depth, face, weights, out_normals, out_colors, clipped)
  if (normals && colors) MVSN_RESOLVE(true, true);
  else if (normals) MVSN_RESOLVE(true, false);
  else if (colors) MVSN_RESOLVE(false, true);
  else MVSN_RESOLVE(false, false);
#undef MVSN_RESOLVE
  return check_launch("mvsn_mesh_render: resolve");
}
