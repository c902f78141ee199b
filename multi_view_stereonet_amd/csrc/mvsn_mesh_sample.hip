// Area-uniform samples of a triangle mesh's surface (see include/mvsn_hip.h: mvsn_mesh_sample_*; the semantics and every
// operation are DESIGN.md section 26).  The areas become exact integers, their prefix is an integer scan, and every draw
// is integer work up to the two barycentric coordinates: the samples are a bitwise-reproducible function of
// (vertices, faces, n, seed), and sample i does not depend on n.
//
// mvsn_mesh_sample_prefix, the head cleared, three launches and the scan, one host read (total, status) behind them:
//   sample_area_kernel      one thread per face: the area in fp64, 0.5 sqrt(|(b - a) x (c - a)|^2), 0 for a face that
//                           takes no part (an index outside [0, M) or a vertex that is not finite: never dereferenced);
//                           the bits of the largest area by a 64-bit integer atomicMax (areas are >= 0: their bits order
//                           as they do)
//   sample_quantise_kernel  q = (uint64) floor(area 2^(31 - e)) with e = ilogb(A_max), so q < 2^32; the sum of the
//                           workgroup's 256 q
//   sample_scan_kernel      one workgroup: the exclusive prefix of those sums, geom_scan_kernel 64 bits wide; the total
//                           and the status word
//   sample_prefix_kernel    P[f] = the inclusive prefix of q, inside the workgroup by __shfl_up and the waves in order
// mvsn_mesh_sample_draw, one launch:
//   sample_draw_kernel      one thread per sample: three splitmix64 draws, the face by binary search over P, the
//                           barycentric pair, the point, and the interpolated normal and colour where asked for
//
// Integer sums do not depend on their order and the maximum does not either, so P is a pure function of the mesh.  fp64
// with only + - x / sqrt and compares; contraction is off for the whole file and nothing is written as a fused
// multiply-add: every step of section 26 is one operation.  No float atomics, no scratch, every loop bounded.
#pragma clang fp contract(off)
#include "mvsn_common.h"
#include "mvsn_geom.h"
#include "mvsn_mesh.h"

namespace mvsn {

constexpr int SM_THREADS = 256;                         // one face, or one sample, per thread

// byte offsets of the workspace sections (each 256-byte aligned)
struct SampleLayout {
  size_t head, area, sums, offsets, bytes;   // area: the fp64 areas, then q, then P in place (8 bytes per face)
  long blocks;
};

inline SampleLayout sample_layout(long f) {
  SampleLayout l;
  l.blocks = (f + SM_THREADS - 1) / SM_THREADS;
  l.head = 0;                                           // [0] bits of A_max, [1] total, [2] status
  l.area = align256(l.head + 4 * sizeof(uint64_t));
  l.sums = align256(l.area + sizeof(uint64_t) * (size_t)f);
  l.offsets = align256(l.sums + sizeof(uint64_t) * (size_t)l.blocks);
  l.bytes = align256(l.offsets + sizeof(uint64_t) * (size_t)l.blocks);
  return l;
}

__global__ __launch_bounds__(SM_THREADS) void sample_area_kernel(const float *__restrict__ vertices, long m,
                                                                 const int64_t *__restrict__ faces, long f,
                                                                 double *__restrict__ area,
                                                                 unsigned long long *__restrict__ head) {
  const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  double mine = 0.0;
  if (i < f) {
    int64_t r[3];
    double p[3][3], c[3];
    if (face_load(vertices, m, faces, i, r, p)) {
      face_cross(p, c);
      mine = 0.5 * sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    }
    area[i] = mine;
  }
  // the workgroup's largest first: one atomic per wave that holds any area
  unsigned long long bits = (unsigned long long)__double_as_longlong(mine);
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(bits, off, 64);
    bits = o > bits ? o : bits;
  }
  if ((threadIdx.x & 63) == 0 && bits != 0) atomicMax(head, bits);
}

// 2^(31 - e) for the A_max whose bits are `bits` (a normal double: e in [-1022, 1023]), 0 for A_max = 0
__device__ __forceinline__ double sample_scale(unsigned long long bits) {
  const long e = (long)((bits >> 52) & 0x7ff) - 1023;
  const long biased = 1023 + 31 - e;                    // in [31, 2076]
  if (bits == 0 || biased < 1 || biased > 2046) return 0.0;
  return __longlong_as_double((long long)((unsigned long long)biased << 52));
}

__global__ __launch_bounds__(SM_THREADS) void sample_quantise_kernel(unsigned long long *__restrict__ area, long f,
                                                                     const unsigned long long *__restrict__ head,
                                                                     unsigned long long *__restrict__ sums) {
  __shared__ unsigned long long swave[SM_THREADS / 64];
  const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  const double scale = sample_scale(head[0]);
  unsigned long long q = 0;
  if (i < f) {
    const double a = __longlong_as_double((long long)area[i]);
    const double s = floor(a * scale);
    q = s >= 0.0 && s < 4294967296.0 ? (unsigned long long)s : 0ull;   // (area <= A_max < 2^(e+1): always inside)
    area[i] = q;
  }
  unsigned long long sum = q;
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if ((threadIdx.x & 63) == 0) swave[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = (swave[0] + swave[1]) + (swave[2] + swave[3]);
}

// geom_scan_kernel (mvsn_geom.h), 64 bits wide: every thread owns a run of ceil(n / 1024) consecutive sums
__global__ __launch_bounds__(GEOM_SCAN_THREADS) void sample_scan_kernel(const unsigned long long *__restrict__ sums, long n,
                                                                        unsigned long long *__restrict__ offsets,
                                                                        unsigned long long *__restrict__ head) {
  __shared__ unsigned long long swave[GEOM_SCAN_THREADS / 64];
  const long per = (n + GEOM_SCAN_THREADS - 1) / GEOM_SCAN_THREADS;
  const long lo = min((long)threadIdx.x * per, n), hi = min(lo + per, n);
  unsigned long long own = 0;
  for (long i = lo; i < hi; ++i) own += sums[i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = own;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) swave[wave] = incl;
  __syncthreads();
  unsigned long long base = 0;
  for (int w = 0; w < wave; ++w) base += swave[w];
  unsigned long long run = base + incl - own;
  for (long i = lo; i < hi; ++i) {
    offsets[i] = run;
    run += sums[i];
  }
  if (threadIdx.x == GEOM_SCAN_THREADS - 1) {
    head[1] = run;
    head[2] = run == 0 ? (unsigned long long)MVSN_MESH_SAMPLE_STATUS_NO_AREA : 0ull;
  }
}

__global__ __launch_bounds__(SM_THREADS) void sample_prefix_kernel(unsigned long long *__restrict__ area, long f,
                                                                   const unsigned long long *__restrict__ offsets) {
  __shared__ unsigned long long swave[SM_THREADS / 64];
  const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  const unsigned long long own = i < f ? area[i] : 0ull;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = own;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) swave[wave] = incl;
  __syncthreads();
  unsigned long long base = offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) base += swave[w];
  if (i < f) area[i] = base + incl;
}

__device__ __forceinline__ unsigned long long sample_z(unsigned long long seed, unsigned long long c) {
  unsigned long long z = seed + c * 0x9E3779B97F4A7C15ull;   // ransac_draw's finaliser (mvsn_cloud_ransac.hip)
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(SM_THREADS) void sample_draw_kernel(
    const float *__restrict__ vertices, long m, const int64_t *__restrict__ faces, long f,
    const unsigned long long *__restrict__ prefix, long n, unsigned long long seed, const float *__restrict__ normals,
    const uint8_t *__restrict__ colors, float *__restrict__ points, int64_t *__restrict__ face,
    float *__restrict__ weights, float *__restrict__ out_normals, uint8_t *__restrict__ out_colors) {
  const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned long long c = 3ull * (unsigned long long)i;
  const unsigned long long z1 = sample_z(seed, c + 1), z2 = sample_z(seed, c + 2), z3 = sample_z(seed, c + 3);
  const unsigned long long pick = __umul64hi(z1, prefix[f - 1]);
  long lo = 0, hi = f;                                   // the first row with P[row] > pick, f where there is none
  for (int step = 0; step < 32 && lo < hi; ++step) {     // (f < 2^31: at most 31 halvings)
    const long mid = lo + ((hi - lo) >> 1);
    if (prefix[mid] > pick) hi = mid;
    else lo = mid + 1;
  }
  int64_t r[3] = {0, 0, 0};
  double p[3][3] = {};
  // (a chosen face has q > 0, so it takes part: anything else is a workspace that is not this mesh's)
  const bool ok = lo < f && face_load(vertices, m, faces, lo, r, p);
  double u = (double)(z2 >> 11) * 0x1p-53, v = (double)(z3 >> 11) * 0x1p-53;
  if (u + v > 1.0) u = 1.0 - u, v = 1.0 - v;
  const double w[3] = {(1.0 - u) - v, u, v};
  face[i] = ok ? (int64_t)lo : (int64_t)-1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double ab = p[1][k] - p[0][k], ac = p[2][k] - p[0][k];
    const double x = (p[0][k] + u * ab) + v * ac;
    points[i * 3 + k] = ok ? (float)x : 0.0f;
    weights[i * 3 + k] = ok ? (float)w[k] : 0.0f;
  }
  if (out_normals) {
    float nrm[3];
    face_normal(normals, r, w, ok, nrm);
#pragma unroll
    for (int k = 0; k < 3; ++k) out_normals[i * 3 + k] = nrm[k];
  }
  if (out_colors) {
    uint8_t col[3];
    face_color(colors, r, w, ok, col);
#pragma unroll
    for (int k = 0; k < 3; ++k) out_colors[i * 3 + k] = col[k];
  }
}

}  // namespace mvsn

extern "C" size_t mvsn_mesh_sample_workspace_bytes(long n_faces) {
  if (n_faces <= 0 || n_faces > mvsn::MESH_MAX_ROWS) return 0;
  return mvsn::sample_layout(n_faces).bytes;
}

static int sample_check(const char *who, const float *vertices, long n_vertices, const int64_t *faces, long n_faces,
                        const void *workspace, size_t workspace_bytes, mvsn::SampleLayout *l) {
  using namespace mvsn;
  MVSN_REQUIRE(vertices && faces, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(n_vertices > 0 && n_faces > 0, MVSN_E_BADARG, "%s: %ld vertices and %ld faces", who, n_vertices, n_faces);
  MVSN_REQUIRE(n_vertices <= MESH_MAX_ROWS && n_faces <= MESH_MAX_ROWS, MVSN_E_TOOLARGE,
               "%s: %ld vertices and %ld faces (at most 2^31 - 1 each)", who, n_vertices, n_faces);
  *l = sample_layout(n_faces);
  return workspace_check(who, "workspace", workspace, workspace_bytes, l->bytes);
}

extern "C" int mvsn_mesh_sample_prefix(const float *vertices, long n_vertices, const int64_t *faces, long n_faces,
                                       int64_t *result, void *workspace, size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  SampleLayout l;
  if (int e = sample_check("mvsn_mesh_sample_prefix", vertices, n_vertices, faces, n_faces, workspace, workspace_bytes, &l))
    return e;
  MVSN_REQUIRE(result, MVSN_E_BADARG, "mvsn_mesh_sample_prefix: null pointer");
  char *ws = (char *)workspace;
  unsigned long long *head = (unsigned long long *)(ws + l.head), *area = (unsigned long long *)(ws + l.area);
  unsigned long long *sums = (unsigned long long *)(ws + l.sums), *offsets = (unsigned long long *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)l.blocks), block(SM_THREADS);
  const hipError_t cleared = hipMemsetAsync(head, 0, 4 * sizeof(unsigned long long), st);
  MVSN_REQUIRE(cleared == hipSuccess, (int)cleared, "mvsn_mesh_sample_prefix: clearing the head: %s",
               hipGetErrorString(cleared));
  hipLaunchKernelGGL(sample_area_kernel, grid, block, 0, st, vertices, n_vertices, faces, n_faces, (double *)area, head);
  if (int e = check_launch("mvsn_mesh_sample_prefix: area")) return e;
  hipLaunchKernelGGL(sample_quantise_kernel, grid, block, 0, st, area, n_faces, (const unsigned long long *)head, sums);
  if (int e = check_launch("mvsn_mesh_sample_prefix: quantise")) return e;
  hipLaunchKernelGGL(sample_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const unsigned long long *)sums,
                     l.blocks, offsets, head);
  if (int e = check_launch("mvsn_mesh_sample_prefix: scan")) return e;
  hipLaunchKernelGGL(sample_prefix_kernel, grid, block, 0, st, area, n_faces, (const unsigned long long *)offsets);
  if (int e = check_launch("mvsn_mesh_sample_prefix: prefix")) return e;
  const hipError_t e = hipMemcpyAsync(result, head + 1, 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
  MVSN_REQUIRE(e == hipSuccess, (int)e, "mvsn_mesh_sample_prefix: copy of the head: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int mvsn_mesh_sample_draw(const float *vertices, long n_vertices, const int64_t *faces, long n_faces,
                                     const void *workspace, size_t workspace_bytes, long n, uint64_t seed,
                                     const float *normals, const uint8_t *colors, float *points, int64_t *face,
                                     float *weights, float *out_normals, uint8_t *out_colors, mvsn_stream_t stream) {
  using namespace mvsn;
  SampleLayout l;
  if (int e = sample_check("mvsn_mesh_sample_draw", vertices, n_vertices, faces, n_faces, workspace, workspace_bytes, &l))
    return e;
  MVSN_REQUIRE(n > 0, MVSN_E_BADARG, "mvsn_mesh_sample_draw: %ld samples", n);
  MVSN_REQUIRE(n <= MESH_MAX_ROWS, MVSN_E_TOOLARGE, "mvsn_mesh_sample_draw: %ld samples (at most 2^31 - 1)", n);
  MVSN_REQUIRE(points && face && weights, MVSN_E_BADARG, "mvsn_mesh_sample_draw: null output");
  MVSN_REQUIRE(!normals == !out_normals && !colors == !out_colors, MVSN_E_BADARG,
               "mvsn_mesh_sample_draw: normals in and out go together, and colours");
  const char *ws = (const char *)workspace;
  hipLaunchKernelGGL(sample_draw_kernel, dim3((unsigned)((n + SM_THREADS - 1) / SM_THREADS)), dim3(SM_THREADS), 0,
                     (hipStream_t)stream, vertices, n_vertices, faces, n_faces, (const unsigned long long *)(ws + l.area), n,
                     (unsigned long long)seed, normals, colors, points, face, weights, out_normals, out_colors);
  return check_launch("mvsn_mesh_sample_draw: draw");
}
