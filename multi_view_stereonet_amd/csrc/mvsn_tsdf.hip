// Dense TSDF volume (see include/mvsn_hip.h: mvsn_tsdf_*; the semantics are DESIGN.md section 15): posed depth maps
// integrated into planar fp32 sums (sum w t, sum w, sum w rgb), and a table-free mesh extraction (Surface Nets) from
// those sums.
//
//   tsdf_integrate_kernel   TS_VOX voxels consecutive in x per thread, 16-byte loads and stores of the state where the
//                           row allows it and a scalar tail where not.  The state is loaded once, every view is
//                           accumulated into it in registers in index order, and it is stored once, whatever V is.  The
//                           cameras (P = K T^-1 as a 3x4, fp64, rounded once) are staged in LDS TS_CAM_BATCH at a time;
//                           more views than a batch loop over batches inside the launch.  The depth (validity, weight,
//                           colour) taps are plain gathers through the caches at an index clamped into the map.
//   Extraction, five launches and one 8-byte device copy, one host read (M, quads) between the second and the third:
//   tsdf_classify_kernel    per voxel a: is the cell whose lowest corner is a active, does the grid edge (a, axis) emit a
//                           quad; one code byte per voxel, and the vertices and quads of the workgroup counted
//   geom_scan_kernel        mvsn_geom.h's scan, launched from here over [vertex counts | quad counts]
//   tsdf_rank_kernel        active cells ranked inside the workgroup (block_rank of mvsn_geom.h): the cell -> row int32
//                           map (-1 = no vertex)
//   tsdf_faces_kernel       the quads ranked the same way in (voxel, axis) order; two triangles each
//   tsdf_vertices_kernel    one thread per voxel: the vertex, normal, colour and cell index of an active cell
// No atomics, no scratch, nothing waits on another workgroup; every loop is bounded and every output is a deterministic
// function of the inputs.
//
// Contraction is off for the whole file: every fused multiply-add of section 15 is written as fmaf, every other step
// is one fp32 operation.
#pragma clang fp contract(off)
#include "mvsn_common.h"
#include "mvsn_camera.h"
#include "mvsn_geom.h"

namespace mvsn {

constexpr int TS_THREADS = 256;
constexpr int TS_VOX = 4;                               // voxels per thread, consecutive in x: one 16-byte access
constexpr int TS_CAM_BATCH = 32;                        // cameras staged in LDS at once
constexpr int TS_BLOCK_VOX = TS_THREADS * TS_VOX;       // voxels per workgroup of the classify / rank / faces kernels
constexpr float TS_FLT_MAX = 3.4028234e38f;
constexpr int TS_MAX_EXTENT = 1 << 24;                  // rows, cols and dims up to here: every index is an exact fp32

// (the camera of one view, P = K T^-1 as a 3x4: tsdf_camera of mvsn_camera.h, shared with mvsn_cloud_render.hip)

// TS_VOX floats at p: one 16-byte access when `wide`, the first `n` of them one by one otherwise
__device__ __forceinline__ void tsdf_load(const float *p, bool wide, int n, float *v) {
  if (wide) {
    const floatx4 w = *reinterpret_cast<const floatx4 *>(p);
    v[0] = w[0], v[1] = w[1], v[2] = w[2], v[3] = w[3];
  } else {
#pragma unroll
    for (int k = 0; k < TS_VOX; ++k) v[k] = k < n ? p[k] : 0.0f;
  }
}

__device__ __forceinline__ void tsdf_store(float *p, bool wide, int n, const float *v) {
  if (wide) {
    *reinterpret_cast<floatx4 *>(p) = floatx4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int k = 0; k < TS_VOX; ++k)
      if (k < n) p[k] = v[k];
  }
}

template <bool COLOR>
__global__ __launch_bounds__(TS_THREADS) void tsdf_integrate_kernel(
    const float *__restrict__ depth, const uint8_t *__restrict__ valid, const float *__restrict__ weights,
    const float *__restrict__ images, const float *__restrict__ K, const float *__restrict__ T, int n_views, int rows,
    int cols, int nx, int ny, int nz, float voxel_size, float ox, float oy, float oz, float trunc, float min_depth,
    float *__restrict__ sdf_sum, float *__restrict__ weight, float *__restrict__ color_sum) {
  __shared__ float scam[TS_CAM_BATCH * TS_CAM];
  const int quads = (nx + TS_VOX - 1) / TS_VOX;                     // threads per row of the volume
  const long items = (long)nz * ny * quads;
  const long item = (long)blockIdx.x * TS_THREADS + threadIdx.x;
  const long it = min(item, items - 1);                             // (a thread past the end computes and stores nothing)
  const long line = it / quads;                                     // k * ny + j
  const int i0 = (int)(it - line * quads) * TS_VOX;
  const int k = (int)(line / ny), j = (int)(line - (long)k * ny);
  const int n = item < items ? min(TS_VOX, nx - i0) : 0;            // voxels of this thread
  const size_t at = (size_t)line * nx + i0;
  const size_t plane = (size_t)nz * ny * nx;
  const long P = (long)rows * cols;
  const bool wide = n == TS_VOX && (((uintptr_t)(sdf_sum + at) | (uintptr_t)(weight + at)) & 15) == 0 &&
                    (!COLOR || (((uintptr_t)(color_sum + at) | (uintptr_t)(color_sum + plane + at) |
                                 (uintptr_t)(color_sum + 2 * plane + at)) & 15) == 0);

  float s[TS_VOX], w[TS_VOX], c[3][TS_VOX];
  tsdf_load(sdf_sum + at, wide, n, s);
  tsdf_load(weight + at, wide, n, w);
  if (COLOR) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) tsdf_load(color_sum + ch * plane + at, wide, n, c[ch]);
  }

  float px[TS_VOX];
#pragma unroll
  for (int q = 0; q < TS_VOX; ++q) px[q] = fmaf((float)(i0 + q), voxel_size, ox);
  const float py = fmaf((float)j, voxel_size, oy), pz = fmaf((float)k, voxel_size, oz);
  const float last_col = (float)(cols - 1), last_row = (float)(rows - 1);

  for (int base = 0; base < n_views; base += TS_CAM_BATCH) {        // bounded: ceil(V / TS_CAM_BATCH) rounds
    const int batch = min(TS_CAM_BATCH, n_views - base);
    __syncthreads();                                                // (the previous batch has been read)
    if (threadIdx.x < batch)
      tsdf_camera(K + (size_t)(base + threadIdx.x) * 16, T + (size_t)(base + threadIdx.x) * 16,
                  scam + threadIdx.x * TS_CAM);
    __syncthreads();
    for (int cam = 0; cam < batch; ++cam) {                         // view order: the sums are bitwise reproducible
      const float *Pm = scam + cam * TS_CAM;
      const int v = base + cam;
      // the part of the three rows that the thread's voxels share
      const float b0 = fmaf(Pm[1], py, fmaf(Pm[2], pz, Pm[3]));
      const float b1 = fmaf(Pm[5], py, fmaf(Pm[6], pz, Pm[7]));
      const float b2 = fmaf(Pm[9], py, fmaf(Pm[10], pz, Pm[11]));
      float z[TS_VOX], D[TS_VOX], wt[TS_VOX], rgb[3][TS_VOX];
      bool ok[TS_VOX];
#pragma unroll
      for (int q = 0; q < TS_VOX; ++q) {
        const float a0 = fmaf(Pm[0], px[q], b0), a1 = fmaf(Pm[4], px[q], b1);
        z[q] = fmaf(Pm[8], px[q], b2);
        const float u = a0 / z[q], vv = a1 / z[q];
        const float fc = floorf(u + 0.5f), fr = floorf(vv + 0.5f);
        // (a NaN fails every comparison)
        ok[q] = q < n && z[q] > min_depth && fc >= 0.0f && fc <= last_col && fr >= 0.0f && fr <= last_row;
        const int col = ok[q] ? (int)fc : 0, row = ok[q] ? (int)fr : 0;
        const size_t pix = (size_t)v * P + (size_t)row * cols + col;          // always inside the maps
        D[q] = depth[pix];
        if (valid) ok[q] = ok[q] && valid[pix] != 0;
        wt[q] = weights ? weights[pix] : 1.0f;
        if (COLOR) {
          const float *im = images + (size_t)v * 3 * P + (size_t)row * cols + col;
          rgb[0][q] = im[0], rgb[1][q] = im[P], rgb[2][q] = im[2 * P];
        }
      }
#pragma unroll
      for (int q = 0; q < TS_VOX; ++q) {
        const float sdf = D[q] - z[q];
        const bool upd = ok[q] && D[q] > 0.0f && D[q] <= TS_FLT_MAX && wt[q] > 0.0f && wt[q] <= TS_FLT_MAX &&
                         !(sdf < -trunc);
        const float t = fminf(sdf, trunc);
        s[q] = upd ? fmaf(wt[q], t, s[q]) : s[q];
        w[q] = upd ? w[q] + wt[q] : w[q];
        if (COLOR) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) c[ch][q] = upd ? fmaf(wt[q], rgb[ch][q], c[ch][q]) : c[ch][q];
        }
      }
    }
  }

  tsdf_store(sdf_sum + at, wide, n, s);
  tsdf_store(weight + at, wide, n, w);
  if (COLOR) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) tsdf_store(color_sum + ch * plane + at, wide, n, c[ch]);
  }
}

// ---- extraction ------------------------------------------------------------------------------------------------------
// byte offsets of the workspace sections (each 256-byte aligned)
struct TsdfLayout {
  size_t code, map, counts, offsets, bytes;
  long blocks;    // workgroups of the classify / rank / faces kernels
};

inline TsdfLayout tsdf_layout(long n) {
  TsdfLayout l;
  l.blocks = (n + TS_BLOCK_VOX - 1) / TS_BLOCK_VOX;
  l.code = 0;
  l.map = align256(l.code + (size_t)n);
  l.counts = align256(l.map + sizeof(int) * (size_t)n);
  l.offsets = align256(l.counts + sizeof(int) * 2 * (size_t)l.blocks);
  l.bytes = align256(l.offsets + sizeof(int64_t) * 2 * (size_t)l.blocks);
  return l;
}

// (formed inside each kernel from its plain pointer arguments: a pointer inside a by-value argument struct is invisible
// to a captured graph, mvsn_common.h)
struct TsdfGrid {
  const float *sdf_sum, *weight;
  int nx, ny, nz;
  float min_weight;
};

__device__ __forceinline__ bool tsdf_observed(const TsdfGrid &g, int i, int j, int k) {
  return i >= 0 && j >= 0 && k >= 0 && i < g.nx && j < g.ny && k < g.nz &&
         g.weight[((size_t)k * g.ny + j) * g.nx + i] >= g.min_weight;
}

// d = sdf_sum / weight of an observed voxel: one fp32 division
__device__ __forceinline__ float tsdf_value(const TsdfGrid &g, int i, int j, int k) {
  const size_t a = ((size_t)k * g.ny + j) * g.nx + i;
  return g.sdf_sum[a] / g.weight[a];
}

// the cell whose lowest corner is (i,j,k) exists and all of its 8 corners are observed
__device__ __forceinline__ bool tsdf_cell_observed(const TsdfGrid &g, int i, int j, int k) {
  if (i < 0 || j < 0 || k < 0 || i + 1 >= g.nx || j + 1 >= g.ny || k + 1 >= g.nz) return false;
  bool all = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) all = all && tsdf_observed(g, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2));
  return all;
}

// code of voxel a = (i,j,k): bit 0 = its cell is active, bit 1 + axis = the edge (a, axis) emits a quad
__device__ __forceinline__ int tsdf_code(const TsdfGrid &g, int i, int j, int k) {
  int code = 0;
  if (tsdf_cell_observed(g, i, j, k)) {
    int inside = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) inside += tsdf_value(g, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)) < 0.0f;
    code = inside != 0 && inside != 8;
  }
  if (!tsdf_observed(g, i, j, k)) return code;
  const bool in0 = tsdf_value(g, i, j, k) < 0.0f;
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    const int e[3] = {axis == 0, axis == 1, axis == 2};
    if (!tsdf_observed(g, i + e[0], j + e[1], k + e[2])) continue;
    if ((tsdf_value(g, i + e[0], j + e[1], k + e[2]) < 0.0f) == in0) continue;
    // the 4 cells around the edge all hold it, so each has a sign change: active <=> it exists with every corner observed
    const int u[3] = {axis == 2, axis == 0, axis == 1}, v[3] = {axis == 1, axis == 2, axis == 0};   // the other two axes
    const bool all = tsdf_cell_observed(g, i - u[0] - v[0], j - u[1] - v[1], k - u[2] - v[2]) &&
                     tsdf_cell_observed(g, i - v[0], j - v[1], k - v[2]) && tsdf_cell_observed(g, i, j, k) &&
                     tsdf_cell_observed(g, i - u[0], j - u[1], k - u[2]);
    if (all) code |= 2 << axis;
  }
  return code;
}

__global__ __launch_bounds__(TS_THREADS) void tsdf_classify_kernel(
    const float *__restrict__ sdf_sum, const float *__restrict__ weight, int nx, int ny, int nz,
    float min_weight, long n, uint8_t *__restrict__ code, int *__restrict__ counts, long blocks) {
  const TsdfGrid g = {sdf_sum, weight, nx, ny, nz, min_weight};
  __shared__ int swave[2][TS_THREADS / 64];
  const long a0 = ((long)blockIdx.x * TS_THREADS + threadIdx.x) * TS_VOX;
  int verts = 0, faces = 0;
#pragma unroll
  for (int q = 0; q < TS_VOX; ++q) {
    const long a = a0 + q;
    if (a >= n) break;
    const long line = a / g.nx;
    const int i = (int)(a - line * g.nx), k = (int)(line / g.ny), j = (int)(line - (long)k * g.ny);
    const int cd = tsdf_code(g, i, j, k);
    code[a] = (uint8_t)cd;
    verts += cd & 1;
    faces += __popc(cd >> 1);
  }
  for (int off = 32; off > 0; off >>= 1) {
    verts += __shfl_xor(verts, off, 64);
    faces += __shfl_xor(faces, off, 64);
  }
  if ((threadIdx.x & 63) == 0) swave[0][threadIdx.x >> 6] = verts, swave[1][threadIdx.x >> 6] = faces;
  __syncthreads();
  if (threadIdx.x < 2)
    counts[threadIdx.x * blocks + blockIdx.x] =
        (swave[threadIdx.x][0] + swave[threadIdx.x][1]) + (swave[threadIdx.x][2] + swave[threadIdx.x][3]);
}

__global__ __launch_bounds__(TS_THREADS) void tsdf_rank_kernel(const uint8_t *__restrict__ code,
                                                               const int64_t *__restrict__ offsets, long n,
                                                               int *__restrict__ map) {
  __shared__ int swave[TS_THREADS / 64];
  const long a0 = ((long)blockIdx.x * TS_THREADS + threadIdx.x) * TS_VOX;
  bool act[TS_VOX];
#pragma unroll
  for (int q = 0; q < TS_VOX; ++q) act[q] = a0 + q < n && (code[min(a0 + q, n - 1)] & 1) != 0;
  int64_t idx = offsets[blockIdx.x] + block_rank(act, swave);
#pragma unroll
  for (int q = 0; q < TS_VOX; ++q) {
    if (a0 + q >= n) break;
    map[a0 + q] = act[q] ? (int)idx : -1;
    idx += act[q];
  }
}

__global__ __launch_bounds__(TS_THREADS) void tsdf_faces_kernel(
    const float *__restrict__ sdf_sum, const float *__restrict__ weight, int nx, int ny, int nz,
    float min_weight, const uint8_t *__restrict__ code, const int *__restrict__ map,
    const int64_t *__restrict__ offsets, long blocks, long n, long n_vertices, long n_quads,
    int64_t *__restrict__ faces) {
  const TsdfGrid g = {sdf_sum, weight, nx, ny, nz, min_weight};
  __shared__ int swave[TS_THREADS / 64];
  const long a0 = ((long)blockIdx.x * TS_THREADS + threadIdx.x) * TS_VOX;
  int cd[TS_VOX];
  bool quad[TS_VOX * 3];                                            // in (voxel, axis) order
#pragma unroll
  for (int q = 0; q < TS_VOX; ++q) {
    cd[q] = a0 + q < n ? code[min(a0 + q, n - 1)] >> 1 : 0;
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) quad[q * 3 + axis] = (cd[q] >> axis) & 1;
  }
  // the quad counts follow the vertex counts in the scanned array: their prefix starts at the vertex total
  int64_t idx = offsets[blocks + blockIdx.x] - offsets[blocks] + block_rank(quad, swave);
#pragma unroll
  for (int q = 0; q < TS_VOX; ++q) {
    if (cd[q] == 0) continue;
    const long a = a0 + q;
    const long line = a / g.nx;
    const int i = (int)(a - line * g.nx), k = (int)(line / g.ny), j = (int)(line - (long)k * g.ny);
    const bool in0 = tsdf_value(g, i, j, k) < 0.0f;
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
      if (!((cd[q] >> axis) & 1)) continue;
      // the 4 cells around the edge, counter-clockwise seen from +axis: (-u,-v), (0,-v), (0,0), (-u,0) with
      // (u, v) the two other axes in cyclic order; the outside is +axis when a itself is inside
      const long su = axis == 2 ? 1 : axis == 0 ? (long)g.nx : (long)g.nx * g.ny;
      const long sv = axis == 1 ? 1 : axis == 2 ? (long)g.nx : (long)g.nx * g.ny;
      const long cell[4] = {a - su - sv, a - sv, a, a - su};
      int64_t r[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const long cm = min(max(cell[m], 0L), n - 1);
        const int row = map[cm];
        r[m] = row >= 0 && row < n_vertices ? row : 0;             // (a quad's cells are active: always a row)
      }
      if (idx < n_quads) {                                         // (n_quads = the scanned total: always true)
        int64_t *f = faces + idx * 6;
        f[0] = r[0], f[1] = in0 ? r[1] : r[2], f[2] = in0 ? r[2] : r[1];
        f[3] = r[0], f[4] = in0 ? r[2] : r[3], f[5] = in0 ? r[3] : r[2];
      }
      ++idx;
    }
  }
}

template <bool COLOR>
__global__ __launch_bounds__(TS_THREADS) void tsdf_vertices_kernel(
    const float *__restrict__ sdf_sum, const float *__restrict__ weight, int nx, int ny, int nz,
    float min_weight, const float *__restrict__ color_sum, const uint8_t *__restrict__ code,
    const int *__restrict__ map, long n, long n_vertices, float voxel_size, float ox, float oy, float oz,
    float *__restrict__ vertices, float *__restrict__ normals, uint8_t *__restrict__ colors, int64_t *__restrict__ cell) {
  const TsdfGrid g = {sdf_sum, weight, nx, ny, nz, min_weight};
  const long a = (long)blockIdx.x * TS_THREADS + threadIdx.x;
  if (a >= n || !(code[a] & 1)) return;
  const long row = map[a];
  if (row < 0 || row >= n_vertices) return;                        // (an active cell's row is always inside)
  const long line = a / g.nx;
  const int i = (int)(a - line * g.nx), k = (int)(line / g.ny), j = (int)(line - (long)k * g.ny);
  if (i + 1 >= g.nx || j + 1 >= g.ny || k + 1 >= g.nz) return;     // (never for a code the classify pass wrote)
  const size_t plane = (size_t)g.nx * g.ny * g.nz;
  float d[8], col[3][8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const size_t at = ((size_t)(k + (c >> 2)) * g.ny + (j + ((c >> 1) & 1))) * g.nx + (i + (c & 1));
    const float wgt = g.weight[at];
    d[c] = g.sdf_sum[at] / wgt;
    if (COLOR) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) col[ch][c] = color_sum[ch * plane + at] / wgt;
    }
  }
  // the 12 edges in a fixed order: axis 0, 1, 2; within an axis the low corner's other two offsets (0,0) (1,0) (0,1)
  // (1,1), the lower axis first
  float sum[3] = {0.0f, 0.0f, 0.0f}, csum[3] = {0.0f, 0.0f, 0.0f}, grad[3] = {0.0f, 0.0f, 0.0f};
  int crossings = 0;
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    const int ua = axis == 0 ? 1 : 0, va = axis == 2 ? 1 : 2;       // the other two axes, lower first
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int lo = ((b & 1) << ua) | ((b >> 1) << va), hi = lo | (1 << axis);
      grad[axis] += d[hi] - d[lo];
      if ((d[lo] < 0.0f) == (d[hi] < 0.0f)) continue;
      const float t = d[lo] / (d[lo] - d[hi]);
      float p[3] = {(float)(lo & 1), (float)((lo >> 1) & 1), (float)(lo >> 2)};
      p[axis] = t;
      sum[0] += p[0], sum[1] += p[1], sum[2] += p[2];
      if (COLOR) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) csum[ch] += fmaf(t, col[ch][hi] - col[ch][lo], col[ch][lo]);
      }
      ++crossings;
    }
  }
  const float cnt = (float)crossings;                               // >= 3 for an active cell
  vertices[row * 3 + 0] = fmaf((float)i + sum[0] / cnt, voxel_size, ox);
  vertices[row * 3 + 1] = fmaf((float)j + sum[1] / cnt, voxel_size, oy);
  vertices[row * 3 + 2] = fmaf((float)k + sum[2] / cnt, voxel_size, oz);
  const float len = sqrtf(fmaf(grad[0], grad[0], fmaf(grad[1], grad[1], grad[2] * grad[2])));
  const bool defined = len > 0.0f && len <= TS_FLT_MAX;
#pragma unroll
  for (int m = 0; m < 3; ++m) normals[row * 3 + m] = defined ? grad[m] / len : 0.0f;
  if (COLOR) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {   // (c + 1) * 127.5 in fp64, rint with ties to even, as mvsn_fusion_emit
      const double q = rint(((double)(csum[ch] / cnt) + 1.0) * 127.5);
      colors[row * 3 + ch] = (uint8_t)(q > 255.0 ? 255.0 : q >= 0.0 ? q : 0.0);      // (a NaN gives 0)
    }
  }
  cell[row] = a;
}

inline bool tsdf_dims_ok(int nx, int ny, int nz) {
  return nx > 0 && ny > 0 && nz > 0 && nx <= TS_MAX_EXTENT && ny <= TS_MAX_EXTENT && nz <= TS_MAX_EXTENT &&
         (long)nx * ny <= 0x7fffffffL && (long)nx * ny * nz <= 0x7fffffffL;
}

inline bool tsdf_positive(float x) { return x > 0.0f && x <= TS_FLT_MAX; }

}  // namespace mvsn

extern "C" int mvsn_tsdf_camera_batch(void) { return mvsn::TS_CAM_BATCH; }

extern "C" int mvsn_tsdf_integrate(const float *depth, const uint8_t *valid, const float *weights, const float *images,
                                   const float *K, const float *T_cam_in_world, int n_views, int rows, int cols, int nx,
                                   int ny, int nz, float voxel_size, float origin_x, float origin_y, float origin_z,
                                   float trunc, float min_depth, float *sdf_sum, float *weight, float *color_sum,
                                   mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(depth && K && T_cam_in_world && sdf_sum && weight, MVSN_E_BADARG, "mvsn_tsdf_integrate: null pointer");
  MVSN_REQUIRE(!images == !color_sum, MVSN_E_BADARG, "mvsn_tsdf_integrate: images and color_sum go together");
  MVSN_REQUIRE(n_views > 0 && rows > 0 && cols > 0, MVSN_E_BADARG, "mvsn_tsdf_integrate: bad sizes (views %d, %d x %d)",
               n_views, rows, cols);
  MVSN_REQUIRE(n_views <= 65535 && (long)rows * cols <= 0x7fffffffL, MVSN_E_TOOLARGE,
               "mvsn_tsdf_integrate: %d views of %d x %d pixels (at most 65535 views of 2^31 - 1 pixels)", n_views, rows,
               cols);
  MVSN_REQUIRE(nx > 0 && ny > 0 && nz > 0, MVSN_E_BADARG, "mvsn_tsdf_integrate: dims %d x %d x %d", nx, ny, nz);
  // indices are compared and scaled as floats: (float)(cols - 1) and (float)i must be exact
  MVSN_REQUIRE(rows <= TS_MAX_EXTENT && cols <= TS_MAX_EXTENT && nx <= TS_MAX_EXTENT && ny <= TS_MAX_EXTENT &&
                   nz <= TS_MAX_EXTENT,
               MVSN_E_TOOLARGE, "mvsn_tsdf_integrate: %d x %d pixels, %d x %d x %d voxels (at most 2^24 along an axis)",
               rows, cols, nx, ny, nz);
  MVSN_REQUIRE(tsdf_dims_ok(nx, ny, nz), MVSN_E_TOOLARGE, "mvsn_tsdf_integrate: %d x %d x %d voxels (at most 2^31 - 1)",
               nx, ny, nz);
  MVSN_REQUIRE(tsdf_positive(voxel_size) && tsdf_positive(trunc), MVSN_E_BADARG,
               "mvsn_tsdf_integrate: voxel size %g or truncation %g is not a positive finite number", (double)voxel_size,
               (double)trunc);
  MVSN_REQUIRE(fabsf(origin_x) <= TS_FLT_MAX && fabsf(origin_y) <= TS_FLT_MAX && fabsf(origin_z) <= TS_FLT_MAX &&
                   fabsf(min_depth) <= TS_FLT_MAX,
               MVSN_E_BADARG, "mvsn_tsdf_integrate: origin or min_depth is not finite");
  const long items = (long)nz * ny * ((nx + TS_VOX - 1) / TS_VOX);
  const dim3 grid((unsigned)((items + TS_THREADS - 1) / TS_THREADS));
  if (color_sum)
    hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, dim3(TS_THREADS), 0, (hipStream_t)stream, depth, valid,
                       weights, images, K, T_cam_in_world, n_views, rows, cols, nx, ny, nz, voxel_size, origin_x,
                       origin_y, origin_z, trunc, min_depth, sdf_sum, weight, color_sum);
  else
    hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, dim3(TS_THREADS), 0, (hipStream_t)stream, depth, valid,
                       weights, images, K, T_cam_in_world, n_views, rows, cols, nx, ny, nz, voxel_size, origin_x,
                       origin_y, origin_z, trunc, min_depth, sdf_sum, weight, color_sum);
  return check_launch("mvsn_tsdf_integrate");
}

extern "C" size_t mvsn_tsdf_workspace_bytes(int nx, int ny, int nz) {
  if (!mvsn::tsdf_dims_ok(nx, ny, nz)) return 0;
  return mvsn::tsdf_layout((long)nx * ny * nz).bytes;
}

extern "C" int mvsn_tsdf_classify(const float *sdf_sum, const float *weight, int nx, int ny, int nz, float min_weight,
                                  int64_t *result, void *workspace, size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(sdf_sum && weight && result, MVSN_E_BADARG, "mvsn_tsdf_classify: null pointer");
  MVSN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, MVSN_E_BADARG, "mvsn_tsdf_classify: dims %d x %d x %d (at least 2 each)",
               nx, ny, nz);
  MVSN_REQUIRE(tsdf_dims_ok(nx, ny, nz), MVSN_E_TOOLARGE, "mvsn_tsdf_classify: %d x %d x %d voxels (at most 2^31 - 1)",
               nx, ny, nz);
  MVSN_REQUIRE(tsdf_positive(min_weight), MVSN_E_BADARG, "mvsn_tsdf_classify: min_weight %g is not a positive finite number",
               (double)min_weight);
  const long n = (long)nx * ny * nz;
  const TsdfLayout l = tsdf_layout(n);
  MVSN_REQUIRE(workspace && workspace_bytes >= l.bytes, MVSN_E_WORKSPACE,
               "mvsn_tsdf_classify: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
  MVSN_REQUIRE(((uintptr_t)workspace & 15) == 0, MVSN_E_BADARG, "mvsn_tsdf_classify: workspace not 16-byte aligned");
  char *ws = (char *)workspace;
  int *counts = (int *)(ws + l.counts);
  int64_t *offsets = (int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tsdf_classify_kernel, dim3((unsigned)l.blocks), dim3(TS_THREADS), 0, st, sdf_sum, weight, nx, ny, nz,
                     min_weight, n,
                     (uint8_t *)(ws + l.code), counts, l.blocks);
  if (int e = check_launch("mvsn_tsdf_classify: classify")) return e;
  // one scan over [vertex counts | quad counts]: result[1] = M + quads, and M = the prefix at the first quad count
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)counts, 2 * l.blocks, offsets,
                     result + 1);
  if (int e = check_launch("mvsn_tsdf_classify: scan")) return e;
  const hipError_t e = hipMemcpyAsync(result, offsets + l.blocks, sizeof(int64_t), hipMemcpyDeviceToDevice, st);
  MVSN_REQUIRE(e == hipSuccess, (int)e, "mvsn_tsdf_classify: copy of the vertex total: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int mvsn_tsdf_extract(const float *sdf_sum, const float *weight, const float *color_sum, int nx, int ny,
                                 int nz, float voxel_size, float origin_x, float origin_y, float origin_z,
                                 float min_weight, const void *workspace, size_t workspace_bytes, long n_vertices,
                                 long n_quads, float *vertices, float *normals, uint8_t *colors, int64_t *faces,
                                 int64_t *cell, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(sdf_sum && weight && workspace, MVSN_E_BADARG, "mvsn_tsdf_extract: null pointer");
  MVSN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, MVSN_E_BADARG, "mvsn_tsdf_extract: dims %d x %d x %d (at least 2 each)", nx,
               ny, nz);
  MVSN_REQUIRE(tsdf_dims_ok(nx, ny, nz), MVSN_E_TOOLARGE, "mvsn_tsdf_extract: %d x %d x %d voxels (at most 2^31 - 1)", nx,
               ny, nz);
  const long n = (long)nx * ny * nz;
  MVSN_REQUIRE(n_vertices >= 0 && n_vertices <= n && n_quads >= 0 && n_quads <= 3 * n, MVSN_E_BADARG,
               "mvsn_tsdf_extract: %ld vertices and %ld quads of %ld voxels", n_vertices, n_quads, n);
  MVSN_REQUIRE(!colors == !color_sum, MVSN_E_BADARG, "mvsn_tsdf_extract: colours and color_sum go together");
  MVSN_REQUIRE(tsdf_positive(voxel_size) && tsdf_positive(min_weight), MVSN_E_BADARG,
               "mvsn_tsdf_extract: voxel size %g or min_weight %g is not a positive finite number", (double)voxel_size,
               (double)min_weight);
  const TsdfLayout l = tsdf_layout(n);
  MVSN_REQUIRE(workspace_bytes >= l.bytes, MVSN_E_WORKSPACE, "mvsn_tsdf_extract: workspace of %zu bytes, %zu needed",
               workspace_bytes, l.bytes);
  if (n_vertices == 0) return 0;                    // no active cell: nothing to launch
  MVSN_REQUIRE(vertices && normals && cell && (n_quads == 0 || faces), MVSN_E_BADARG, "mvsn_tsdf_extract: null output");
  char *ws = (char *)workspace;                     // (the map section is written here: the workspace is the caller's)
  const uint8_t *code = (const uint8_t *)(ws + l.code);
  int *map = (int *)(ws + l.map);
  const int64_t *offsets = (const int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tsdf_rank_kernel, dim3((unsigned)l.blocks), dim3(TS_THREADS), 0, st, code, offsets, n, map);
  if (int e = check_launch("mvsn_tsdf_extract: rank")) return e;
  if (n_quads > 0) {
    hipLaunchKernelGGL(tsdf_faces_kernel, dim3((unsigned)l.blocks), dim3(TS_THREADS), 0, st, sdf_sum, weight, nx, ny, nz,
                       min_weight, code, (const int *)map,
                       offsets, l.blocks, n, n_vertices, n_quads, faces);
    if (int e = check_launch("mvsn_tsdf_extract: faces")) return e;
  }
  const dim3 grid((unsigned)((n + TS_THREADS - 1) / TS_THREADS));
  if (color_sum)
    hipLaunchKernelGGL(tsdf_vertices_kernel<true>, grid, dim3(TS_THREADS), 0, st, sdf_sum, weight, nx, ny, nz, min_weight,
                       color_sum, code, (const int *)map, n,
                       n_vertices, voxel_size, origin_x, origin_y, origin_z, vertices, normals, colors, cell);
  else
    hipLaunchKernelGGL(tsdf_vertices_kernel<false>, grid, dim3(TS_THREADS), 0, st, sdf_sum, weight, nx, ny, nz, min_weight,
                       color_sum, code, (const int *)map,
                       n, n_vertices, voxel_size, origin_x, origin_y, origin_z, vertices, normals, colors, cell);
  return check_launch("mvsn_tsdf_extract: vertices");
}
