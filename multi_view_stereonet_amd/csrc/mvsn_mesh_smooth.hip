// Laplacian and Taubin smoothing over the unique edges of a mesh, and its face and vertex normals (see
// include/mvsn_hip.h: mvsn_mesh_smooth, mvsn_mesh_normals; the semantics and every operation are DESIGN.md section 29).
//
// mvsn_mesh_smooth, no host read:
//   smooth_clear_kernel    the six bound keys and the parameters
//   smooth_load_kernel     one thread per vertex: x = (double)v, sums and degree zeroed, the flags (non-finite, pinned),
//                          and per axis atomicMin / atomicMax of an order-preserving key of the float's bits
//   smooth_setup_kernel    one thread: span = the largest per-axis difference in fp64 = m 2^k, m in [0.5, 1); the step
//                          2^(k-30) and its inverse, into the workspace; inactive without a finite vertex or with span 0
//   smooth_degree_kernel   one thread per edge: +1 to the degree of both ends where the edge contributes
//   per step, back to back on the stream:
//   smooth_edge_kernel     one thread per edge (a, b), per axis: d = x_b - x_a, q = rint(d 2^(30-k)) clamped to +-2^31,
//                          64-bit integer atomicAdd of +q at a and of -q at b
//   smooth_vertex_kernel   one thread per vertex: mean = ((double)sum step) / (double)degree, x = x + f mean where the
//                          vertex is free and has a degree; the sum zeroed
//   smooth_store_kernel    (float)x, rounded once; the input's bits for a flagged vertex and for an inactive call
//
// mvsn_mesh_normals:
//   normals_clear_kernel   per vertex: the maximum and the three sums zeroed
//   normals_face_kernel    per face: c = (p1 - p0) x (p2 - p0) in fp64 with the lowest row in front, c / |c| and |c| / 2;
//                          64-bit atomicMax at each corner of the bits of max(|cx|, |cy|, |cz|)
//   normals_sum_kernel     per face and corner: with the corner's maximum = m 2^e, rint(c 2^(31-e)) into its int64 sums
//   normals_vertex_kernel  per vertex: the direction of (double)sum, rounded once; zeros for a zero sum
//
// Every atomic is an integer one (minima, maxima, sums): the outputs do not depend on the order of the edges or faces or
// on any race.  No loop, no wait.  fp64 with + - x / sqrt rint and compares only; contraction is off for the whole file:
// every step of section 29 is one operation, and tests/mesh_smooth_reference.py repeats it in numpy bit for bit.
#pragma clang fp contract(off)
#include "mvsn_common.h"
#include "mvsn_geom.h"
#include "mvsn_mesh.h"

namespace mvsn {

constexpr int SM_THREADS = 256;                         // one vertex, edge or face per thread
constexpr long SM_MAX_ITERATIONS = 10000;
constexpr double SM_CLAMP = 2147483648.0;               // 2^31
constexpr int SM_NONFINITE = 2, SM_PINNED = 1;          // the flags of a vertex
enum { SM_LAPLACIAN = 0, SM_TAUBIN = 1 };

// the head of the workspace: what the setup kernel leaves for the steps
struct SmoothParams {
  unsigned lo[3], hi[3];    // order-preserving keys of the per-axis minimum and maximum over the finite vertices
  int active;               // 0: no finite vertex, or span == 0: the output is the input's bits
  int pad;
  double step, scale;       // 2^(k-30) and 2^(30-k)
};

struct SmoothLayout {
  size_t params, x, sum, degree, flags, bytes;
};

inline SmoothLayout smooth_layout(long m) {
  SmoothLayout l;
  const size_t M = (size_t)m;
  l.params = 0;
  l.x = align256(sizeof(SmoothParams));
  l.sum = align256(l.x + sizeof(double) * 3 * M);
  l.degree = align256(l.sum + sizeof(uint64_t) * 3 * M);
  l.flags = align256(l.degree + sizeof(int) * M);
  l.bytes = align256(l.flags + sizeof(int) * M);
  return l;
}

// a < b as floats (neither a NaN) iff key(a) < key(b) as unsigned; -0 sorts below +0
__device__ __forceinline__ unsigned smooth_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float smooth_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ void smooth_clear_kernel(SmoothParams *__restrict__ p) {
  if (threadIdx.x < 3) {
    p->lo[threadIdx.x] = 0xffffffffu;
    p->hi[threadIdx.x] = 0u;
  }
  if (threadIdx.x == 0) {
    p->active = 0;
    p->pad = 0;
    p->step = 0.0;
    p->scale = 0.0;
  }
}

__global__ __launch_bounds__(SM_THREADS) void smooth_load_kernel(const float *__restrict__ vertices, long m,
                                                                 const uint8_t *__restrict__ pinned,
                                                                 SmoothParams *__restrict__ p, double *__restrict__ x,
                                                                 unsigned long long *__restrict__ sum,
                                                                 int *__restrict__ degree, int *__restrict__ flags) {
  const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= m) return;
  float v[3];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = vertices[i * 3 + k];
    finite = finite && isfinite(v[k]);
    x[i * 3 + k] = (double)v[k];
    sum[i * 3 + k] = 0ull;
  }
  degree[i] = 0;
  flags[i] = (finite ? 0 : SM_NONFINITE) | (pinned && pinned[i] ? SM_PINNED : 0);
  if (finite) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned key = smooth_key(v[k]);
      atomicMin(p->lo + k, key);
      atomicMax(p->hi + k, key);
    }
  }
}

__global__ void smooth_setup_kernel(SmoothParams *__restrict__ p) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (p->lo[0] > p->hi[0]) return;                       // no finite vertex
  double span = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double d = (double)smooth_unkey(p->hi[k]) - (double)smooth_unkey(p->lo[k]);
    span = d > span ? d : span;
  }
  if (!(span > 0.0)) return;
  // span = m 2^k with m in [0.5, 1): a difference of two floats is a normal double
  const int k = (int)((__double_as_longlong(span) >> 52) & 0x7ff) - 1022;
  p->step = __longlong_as_double((long long)(k - 30 + 1023) << 52);
  p->scale = __longlong_as_double((long long)(30 - k + 1023) << 52);
  p->active = 1;
}

// the ends of edge j where it contributes: both inside [0, m), different, and neither non-finite
__device__ __forceinline__ bool smooth_ends(const int64_t *__restrict__ edges, const int *__restrict__ flags, long m,
                                            long j, int64_t *a, int64_t *b) {
  *a = edges[j * 2], *b = edges[j * 2 + 1];
  if (!(*a >= 0 && *a < m && *b >= 0 && *b < m) || *a == *b) return false;
  return ((flags[*a] | flags[*b]) & SM_NONFINITE) == 0;
}

__global__ __launch_bounds__(SM_THREADS) void smooth_degree_kernel(const int64_t *__restrict__ edges, long e, long m,
                                                                   const int *__restrict__ flags,
                                                                   int *__restrict__ degree) {
  const long j = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (j >= e) return;
  int64_t a, b;
  if (!smooth_ends(edges, flags, m, j, &a, &b)) return;
  atomicAdd(degree + a, 1);
  atomicAdd(degree + b, 1);
}

__global__ __launch_bounds__(SM_THREADS) void smooth_edge_kernel(const int64_t *__restrict__ edges, long e, long m,
                                                                 const int *__restrict__ flags,
                                                                 const SmoothParams *__restrict__ p,
                                                                 const double *__restrict__ x,
                                                                 unsigned long long *__restrict__ sum) {
  const long j = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (j >= e || !p->active) return;
  int64_t a, b;
  if (!smooth_ends(edges, flags, m, j, &a, &b)) return;
  const double scale = p->scale;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double d = x[b * 3 + k] - x[a * 3 + k];
    double q = rint(d * scale);                          // half to even
    q = q < -SM_CLAMP ? -SM_CLAMP : q;
    q = q > SM_CLAMP ? SM_CLAMP : q;
    q = q == q ? q : 0.0;                                // (positions that ran away to infinity: inf - inf)
    const long long n = (long long)q;
    if (n != 0) {                                        // two's complement: the unsigned sum is the signed one
      atomicAdd(sum + a * 3 + k, (unsigned long long)n);
      atomicAdd(sum + b * 3 + k, (unsigned long long)(-n));
    }
  }
}

__global__ __launch_bounds__(SM_THREADS) void smooth_vertex_kernel(long m, const int *__restrict__ flags,
                                                                   const int *__restrict__ degree,
                                                                   const SmoothParams *__restrict__ p, double factor,
                                                                   double *__restrict__ x,
                                                                   unsigned long long *__restrict__ sum) {
  const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= m || !p->active) return;
  const int n = degree[i];
  const bool moves = flags[i] == 0 && n > 0;
  const double step = p->step;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (moves) {
      const double mean = ((double)(long long)sum[i * 3 + k] * step) / (double)n;
      x[i * 3 + k] = x[i * 3 + k] + factor * mean;
    }
    sum[i * 3 + k] = 0ull;
  }
}

__global__ __launch_bounds__(SM_THREADS) void smooth_store_kernel(const float *__restrict__ vertices, long m,
                                                                  const int *__restrict__ flags,
                                                                  const SmoothParams *__restrict__ p,
                                                                  const double *__restrict__ x, float *__restrict__ out) {
  const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= m) return;
  const bool kept = !p->active || flags[i] != 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) out[i * 3 + k] = kept ? vertices[i * 3 + k] : (float)x[i * 3 + k];
}

// ---- normals --------------------------------------------------------------------------------------------------------

struct NormalsLayout {
  size_t vmax, nsum, bytes;
};

inline NormalsLayout normals_layout(long m) {
  NormalsLayout l;
  l.vmax = 0;
  l.nsum = align256(sizeof(uint64_t) * (size_t)m);
  l.bytes = align256(l.nsum + sizeof(uint64_t) * 3 * (size_t)m);
  return l;
}

// c = (p1 - p0) x (p2 - p0) of face r with the lowest row rotated to the front (the bits do not depend on which corner
// the face starts with; the winding stays) and len = |c|; false for a corner outside [0, m), a non-finite corner or no
// area.  row: the corners in the rotated order.
__device__ __forceinline__ bool normals_cross(const float *__restrict__ vertices, long m,
                                              const int64_t *__restrict__ faces, long r, int64_t *row, double *c,
                                              double *len) {
  int64_t in[3];
  if (!face_rows(faces, r, m, in)) return false;
  face_lead(in, row);
  double p[3][3];
  if (!face_points(vertices, row, p)) return false;
  face_cross(p, c);
  *len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  return *len > 0.0 && *len <= 1.7e308;
}

__global__ __launch_bounds__(SM_THREADS) void normals_clear_kernel(unsigned long long *__restrict__ vmax,
                                                                   unsigned long long *__restrict__ nsum, long m) {
  const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= m) return;
  vmax[i] = 0ull;
  nsum[i * 3] = nsum[i * 3 + 1] = nsum[i * 3 + 2] = 0ull;
}

__global__ __launch_bounds__(SM_THREADS) void normals_face_kernel(const float *__restrict__ vertices, long m,
                                                                  const int64_t *__restrict__ faces, long f,
                                                                  unsigned long long *__restrict__ vmax,
                                                                  float *__restrict__ face_normals,
                                                                  float *__restrict__ face_area) {
  const long r = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (r >= f) return;
  int64_t row[3];
  double c[3], len;
  float n[3] = {0.0f, 0.0f, 0.0f}, area = 0.0f;
  if (normals_cross(vertices, m, faces, r, row, c, &len)) {
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = (float)(c[k] / len);
    area = (float)(len / 2.0);
    const double ax = fabs(c[0]), ay = fabs(c[1]), az = fabs(c[2]);
    const double big = ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
    const unsigned long long bits = (unsigned long long)__double_as_longlong(big);   // positive doubles order as integers
#pragma unroll
    for (int j = 0; j < 3; ++j) atomicMax(vmax + row[j], bits);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) face_normals[r * 3 + k] = n[k];
  face_area[r] = area;
}

__global__ __launch_bounds__(SM_THREADS) void normals_sum_kernel(const float *__restrict__ vertices, long m,
                                                                 const int64_t *__restrict__ faces, long f,
                                                                 const unsigned long long *__restrict__ vmax,
                                                                 unsigned long long *__restrict__ nsum) {
  const long r = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (r >= f) return;
  int64_t row[3];
  double c[3], len;
  if (!normals_cross(vertices, m, faces, r, row, c, &len)) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // the corner's maximum = m 2^e with m in [0.5, 1) (normal and positive: a valid face wrote it); |c| <= it < 2^e
    const int e = (int)((vmax[row[j]] >> 52) & 0x7ff) - 1022;
    const double scale = __longlong_as_double((long long)(31 - e + 1023) << 52);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long q = (long long)rint(c[k] * scale);
      if (q != 0) atomicAdd(nsum + row[j] * 3 + k, (unsigned long long)q);
    }
  }
}

__global__ __launch_bounds__(SM_THREADS) void normals_vertex_kernel(const unsigned long long *__restrict__ nsum, long m,
                                                                    float *__restrict__ vertex_normals) {
  const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= m) return;
  const double s[3] = {(double)(long long)nsum[i * 3], (double)(long long)nsum[i * 3 + 1],
                       (double)(long long)nsum[i * 3 + 2]};
  const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) vertex_normals[i * 3 + k] = len > 0.0 ? (float)(s[k] / len) : 0.0f;
}

inline unsigned smooth_blocks(long n) { return (unsigned)((n + SM_THREADS - 1) / SM_THREADS); }

}  // namespace mvsn

extern "C" size_t mvsn_mesh_smooth_workspace_bytes(long n_vertices) {
  if (n_vertices <= 0 || n_vertices > mvsn::MESH_MAX_ROWS) return 0;
  return mvsn::smooth_layout(n_vertices).bytes;
}

extern "C" int mvsn_mesh_smooth(const float *vertices, long n_vertices, const int64_t *edges, long n_edges,
                                const uint8_t *pinned, int method, long iterations, double lam, double mu,
                                void *workspace, size_t workspace_bytes, float *out_vertices, mvsn_stream_t stream) {
  using namespace mvsn;
  const long m = n_vertices, e = n_edges;
  MVSN_REQUIRE(vertices && out_vertices && workspace, MVSN_E_BADARG, "mvsn_mesh_smooth: null pointer");
  MVSN_REQUIRE(m > 0 && e >= 0 && (e == 0 || edges), MVSN_E_BADARG, "mvsn_mesh_smooth: %ld vertices, %ld edges", m, e);
  MVSN_REQUIRE(m <= MESH_MAX_ROWS && e <= MESH_MAX_ROWS, MVSN_E_TOOLARGE,   // (mvsn_mesh_edges emits fewer: 3 per face)
               "mvsn_mesh_smooth: %ld vertices, %ld edges (at most 2^31 - 1 of either)", m, e);
  MVSN_REQUIRE(method == SM_LAPLACIAN || method == SM_TAUBIN, MVSN_E_BADARG,
               "mvsn_mesh_smooth: method %d (0 = laplacian, 1 = taubin)", method);
  MVSN_REQUIRE(iterations >= 0 && iterations <= SM_MAX_ITERATIONS, MVSN_E_BADARG,
               "mvsn_mesh_smooth: %ld iterations (0 to 10000)", iterations);
  MVSN_REQUIRE(lam > 0.0 && lam <= 1.0 && mu >= -2.0 && mu < 0.0, MVSN_E_BADARG,
               "mvsn_mesh_smooth: lam %g (0 < lam <= 1), mu %g (-2 <= mu < 0)", lam, mu);
  const SmoothLayout l = smooth_layout(m);
  if (int err = workspace_check("mvsn_mesh_smooth", "workspace", workspace, workspace_bytes, l.bytes)) return err;
  char *ws = (char *)workspace;
  SmoothParams *params = (SmoothParams *)(ws + l.params);
  double *x = (double *)(ws + l.x);
  unsigned long long *sum = (unsigned long long *)(ws + l.sum);
  int *degree = (int *)(ws + l.degree), *flags = (int *)(ws + l.flags);
  const hipStream_t st = (hipStream_t)stream;
  const unsigned vblocks = smooth_blocks(m), eblocks = smooth_blocks(e);
  hipLaunchKernelGGL(smooth_clear_kernel, dim3(1), dim3(64), 0, st, params);
  if (int err = check_launch("mvsn_mesh_smooth: clear")) return err;
  hipLaunchKernelGGL(smooth_load_kernel, dim3(vblocks), dim3(SM_THREADS), 0, st, vertices, m, pinned, params, x, sum,
                     degree, flags);
  if (int err = check_launch("mvsn_mesh_smooth: load")) return err;
  hipLaunchKernelGGL(smooth_setup_kernel, dim3(1), dim3(64), 0, st, params);
  if (int err = check_launch("mvsn_mesh_smooth: setup")) return err;
  if (e > 0) {
    hipLaunchKernelGGL(smooth_degree_kernel, dim3(eblocks), dim3(SM_THREADS), 0, st, edges, e, m, (const int *)flags,
                       degree);
    if (int err = check_launch("mvsn_mesh_smooth: degree")) return err;
    const long steps = method == SM_TAUBIN ? 2 * iterations : iterations;
    for (long s = 0; s < steps; ++s) {                   // back to back: no host read in the loop
      const double factor = method == SM_TAUBIN && (s & 1) ? mu : lam;
      hipLaunchKernelGGL(smooth_edge_kernel, dim3(eblocks), dim3(SM_THREADS), 0, st, edges, e, m, (const int *)flags,
                         (const SmoothParams *)params, (const double *)x, sum);
      hipLaunchKernelGGL(smooth_vertex_kernel, dim3(vblocks), dim3(SM_THREADS), 0, st, m, (const int *)flags,
                         (const int *)degree, (const SmoothParams *)params, factor, x, sum);
    }
    if (int err = check_launch("mvsn_mesh_smooth: steps")) return err;
  }
  hipLaunchKernelGGL(smooth_store_kernel, dim3(vblocks), dim3(SM_THREADS), 0, st, vertices, m, (const int *)flags,
                     (const SmoothParams *)params, (const double *)x, out_vertices);
  return check_launch("mvsn_mesh_smooth: store");
}

extern "C" size_t mvsn_mesh_normals_workspace_bytes(long n_vertices) {
  if (n_vertices <= 0 || n_vertices > mvsn::MESH_MAX_ROWS) return 0;
  return mvsn::normals_layout(n_vertices).bytes;
}

extern "C" int mvsn_mesh_normals(const float *vertices, long n_vertices, const int64_t *faces, long n_faces,
                                 void *workspace, size_t workspace_bytes, float *face_normals, float *face_area,
                                 float *vertex_normals, mvsn_stream_t stream) {
  using namespace mvsn;
  const long m = n_vertices, f = n_faces;
  MVSN_REQUIRE(vertices && vertex_normals && workspace, MVSN_E_BADARG, "mvsn_mesh_normals: null pointer");
  MVSN_REQUIRE(m > 0 && f >= 0 && (f == 0 || (faces && face_normals && face_area)), MVSN_E_BADARG,
               "mvsn_mesh_normals: %ld vertices, %ld faces", m, f);
  MVSN_REQUIRE(m <= MESH_MAX_ROWS && f <= MESH_MAX_ROWS, MVSN_E_TOOLARGE,
               "mvsn_mesh_normals: %ld vertices, %ld faces (at most 2^31 - 1 of either)", m, f);
  const NormalsLayout l = normals_layout(m);
  if (int e = workspace_check("mvsn_mesh_normals", "workspace", workspace, workspace_bytes, l.bytes)) return e;
  char *ws = (char *)workspace;
  unsigned long long *vmax = (unsigned long long *)(ws + l.vmax), *nsum = (unsigned long long *)(ws + l.nsum);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(normals_clear_kernel, dim3(smooth_blocks(m)), dim3(SM_THREADS), 0, st, vmax, nsum, m);
  if (int e = check_launch("mvsn_mesh_normals: clear")) return e;
  if (f > 0) {
    hipLaunchKernelGGL(normals_face_kernel, dim3(smooth_blocks(f)), dim3(SM_THREADS), 0, st, vertices, m, faces, f, vmax,
                       face_normals, face_area);
    if (int e = check_launch("mvsn_mesh_normals: faces")) return e;
    hipLaunchKernelGGL(normals_sum_kernel, dim3(smooth_blocks(f)), dim3(SM_THREADS), 0, st, vertices, m, faces, f,
                       (const unsigned long long *)vmax, nsum);
    if (int e = check_launch("mvsn_mesh_normals: sums")) return e;
  }
  hipLaunchKernelGGL(normals_vertex_kernel, dim3(smooth_blocks(m)), dim3(SM_THREADS), 0, st,
                     (const unsigned long long *)nsum, m, vertex_normals);
  return check_launch("mvsn_mesh_normals: vertices");
}
