// Exact point-to-triangle-mesh distance within a radius (see include/mvsn_hip.h: mvsn_mesh_nearest*; the semantics, the
// distance operation by operation and the proof that the cells visited are enough are DESIGN.md section 26): for every
// query point the nearest face within max_dist (squared distance, row, closest point, barycentric weights) and the number
// of faces within max_dist.  The mesh counterpart of mvsn_cloud.hip, on the same hash grid (mvsn_voxel.h, cell = max_dist).
//
// mvsn_mesh_nearest_count, one launch, one host read (pairs, large faces, status) behind it:
//   nearest_count_kernel    one thread per face: the box of cells floor(min inv) .. floor(max inv) per axis; a face of
//                           at most MVSN_MESH_NEAREST_BOX_CELLS cells adds them to `pairs`, a larger one 1 to `large`;
//                           a face with an index outside [0, M) or a vertex that is not finite takes no part (never
//                           dereferenced); a finite vertex without a cell sets MVSN_MESH_NEAREST_STATUS_RANGE
// mvsn_mesh_nearest_build: mvsn_cloud_index_build's counting sort, over (cell, face) pairs, six launches:
//   cloud_init_kernel       (mvsn_cloud.hip) every key empty, every population and cursor zero
//   nearest_assign_kernel   one thread per face: hash_insert of every cell of its box, 1 added to the cell's population
//   cloud_count_kernel, geom_scan_kernel, cloud_start_kernel   (mvsn_cloud.hip, mvsn_voxel.hip) start[slot]
//   nearest_scatter_kernel  one thread per face: its row into the records of every cell of its box (a returning
//                           atomicAdd on the cell's cursor), or onto the list of large faces
// mvsn_mesh_nearest, one launch:
//   nearest_query_kernel    one thread per query: cloud_cells (mvsn_cloud.h); a face met in cell c is evaluated only
//                           where c is the componentwise maximum of the lower corners of the query's range and of the
//                           face's box (once per query); then every large face; the minimum of (d2 bits, row) as one
//                           64-bit key and the count; the winner's point and weights recomputed once after the walk
//
// A pair record is the face row alone (4 bytes): a face lies in several cells, so a 48-byte record of its vertices would
// multiply the mesh by the pair count, and the box test that rejects most records needs the vertices' fp32 minima only.
// Where a row lands inside its cell's records depends on the order of the scatter's atomics; no output does.  Integer
// atomics only; fp64 with + - x / and compares, contraction off for the whole file; no scratch; every loop bounded.
#pragma clang fp contract(off)
#include "mvsn_cloud.h"
#include "mvsn_mesh.h"

namespace mvsn {

constexpr int MN_THREADS = 256;                         // one face, or one query, per thread
constexpr unsigned long long MN_BOX_CELLS = MVSN_MESH_NEAREST_BOX_CELLS;
enum { MN_NO_PART = 0, MN_BOXED = 1, MN_OUT_OF_RANGE = 2 };

// byte offsets of the workspace sections (each 256-byte aligned)
struct NearestLayout {
  size_t head, keys, pop, start, cursor, records, large, counts, offsets, bytes;
  size_t slots;   // power of two >= 2 pairs (>= pairs above 2^30): no more cells than pairs
  long blocks;
};

inline NearestLayout nearest_layout(long pairs, long large) {
  NearestLayout l;
  l.slots = hash_table_slots(pairs, CL_MIN_SLOTS);
  l.blocks = (long)(l.slots / CL_BLOCK_SLOTS);
  l.head = 0;                                           // [0] the table's status word, [1] the large faces listed
  l.keys = align256(l.head + 2 * sizeof(unsigned long long));
  l.pop = align256(l.keys + sizeof(unsigned long long) * l.slots);
  l.start = align256(l.pop + sizeof(int) * l.slots);
  l.cursor = align256(l.start + sizeof(int) * l.slots);
  l.records = align256(l.cursor + sizeof(int) * l.slots);
  l.large = align256(l.records + sizeof(int) * (size_t)pairs);
  l.counts = align256(l.large + sizeof(int) * (size_t)large);
  l.offsets = align256(l.counts + sizeof(int) * (size_t)l.blocks);
  l.bytes = align256(l.offsets + sizeof(int64_t) * (size_t)l.blocks);
  return l;
}

inline bool nearest_sizes_ok(long pairs, long large) { return pairs >= 0 && pairs <= MESH_MAX_ROWS && large >= 0 && large <= MESH_MAX_ROWS; }

// The vertices of face i and its box of cells, every step one fp32 operation: lo = floor(min inv), hi = floor(max inv)
// per axis.  MN_NO_PART (nothing dereferenced) when an index lies outside [0, m) or a coordinate is not finite;
// MN_OUT_OF_RANGE when a finite vertex has no cell in [-2^20, 2^20).
__device__ __forceinline__ int nearest_face_box(const float *__restrict__ vertices, long m,
                                                const int64_t *__restrict__ faces, long i, float inv, float (*p)[3],
                                                int *lo, int *hi) {
  int64_t r[3];
  if (!face_rows(faces, i, m, r)) return MN_NO_PART;
  bool finite = true, inside = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a = vertices[r[0] * 3 + k], b = vertices[r[1] * 3 + k], c = vertices[r[2] * 3 + k];
    p[0][k] = a, p[1][k] = b, p[2][k] = c;
    finite = finite && isfinite(a) && isfinite(b) && isfinite(c);
    float mn = b < a ? b : a, mx = b > a ? b : a;
    mn = c < mn ? c : mn, mx = c > mx ? c : mx;
    const float tl = mn * inv, th = mx * inv;
    const float fl = floorf(tl), fh = floorf(th);
    const bool in = isfinite(tl) && isfinite(th) && fl >= -(float)VX_CELL_BIAS && fh < (float)VX_CELL_BIAS;
    inside = inside && in;
    lo[k] = in ? (int)fl : 0, hi[k] = in ? (int)fh : 0;
  }
  return !finite ? MN_NO_PART : inside ? MN_BOXED : MN_OUT_OF_RANGE;
}

__device__ __forceinline__ unsigned long long nearest_box_cells(const int *lo, const int *hi) {
  return (unsigned long long)(hi[0] - lo[0] + 1) * (unsigned long long)(hi[1] - lo[1] + 1) *
         (unsigned long long)(hi[2] - lo[2] + 1);         // (at most 2^21 per axis: below 2^63)
}

__global__ __launch_bounds__(MN_THREADS) void nearest_count_kernel(const float *__restrict__ vertices, long m,
                                                                   const int64_t *__restrict__ faces, long f, float inv,
                                                                   unsigned long long *__restrict__ result) {
  const long i = (long)blockIdx.x * MN_THREADS + threadIdx.x;
  unsigned long long pairs = 0, large = 0, status = 0;
  if (i < f) {
    float p[3][3];
    int lo[3], hi[3];
    const int state = nearest_face_box(vertices, m, faces, i, inv, p, lo, hi);
    if (state == MN_BOXED) {
      const unsigned long long cells = nearest_box_cells(lo, hi);
      if (cells > MN_BOX_CELLS) large = 1;
      else pairs = cells;
    } else if (state == MN_OUT_OF_RANGE) {
      status = MVSN_MESH_NEAREST_STATUS_RANGE;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    pairs += __shfl_xor(pairs, off, 64);
    large += __shfl_xor(large, off, 64);
    status |= __shfl_xor(status, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {                          // integer sums: the order of arrival does not show
    if (pairs) atomicAdd(result + 0, pairs);
    if (large) atomicAdd(result + 1, large);
    if (status) atomicOr(result + 2, status);
  }
}

__global__ __launch_bounds__(MN_THREADS) void nearest_assign_kernel(const float *__restrict__ vertices, long m,
                                                                    const int64_t *__restrict__ faces, long f, float inv,
                                                                    unsigned long long *__restrict__ keys,
                                                                    int *__restrict__ pop, size_t slots) {
  const long i = (long)blockIdx.x * MN_THREADS + threadIdx.x;
  if (i >= f) return;
  float p[3][3];
  int lo[3], hi[3];
  if (nearest_face_box(vertices, m, faces, i, inv, p, lo, hi) != MN_BOXED) return;
  if (nearest_box_cells(lo, hi) > MN_BOX_CELLS) return;
  int c[3];
  for (c[0] = lo[0]; c[0] <= hi[0]; ++c[0])
    for (c[1] = lo[1]; c[1] <= hi[1]; ++c[1])
      for (c[2] = lo[2]; c[2] <= hi[2]; ++c[2]) {
        const int found = hash_insert(keys, slots, voxel_key(c));
        if (found >= 0) atomicAdd(pop + found, 1);      // (slots >= pairs >= cells: there is always room)
      }
}

__global__ __launch_bounds__(MN_THREADS) void nearest_scatter_kernel(const float *__restrict__ vertices, long m,
                                                                     const int64_t *__restrict__ faces, long f, float inv,
                                                                     unsigned long long *__restrict__ keys, size_t slots,
                                                                     const int *__restrict__ start, int *__restrict__ cursor,
                                                                     int *__restrict__ records, long pairs,
                                                                     int *__restrict__ large_rows, long large,
                                                                     unsigned long long *__restrict__ listed) {
  const long i = (long)blockIdx.x * MN_THREADS + threadIdx.x;
  if (i >= f) return;
  float p[3][3];
  int lo[3], hi[3];
  if (nearest_face_box(vertices, m, faces, i, inv, p, lo, hi) != MN_BOXED) return;
  if (nearest_box_cells(lo, hi) > MN_BOX_CELLS) {
    const unsigned long long at = atomicAdd(listed, 1ull);
    if (at < (unsigned long long)large) large_rows[at] = (int)i;
    return;
  }
  int c[3];
  for (c[0] = lo[0]; c[0] <= hi[0]; ++c[0])
    for (c[1] = lo[1]; c[1] <= hi[1]; ++c[1])
      for (c[2] = lo[2]; c[2] <= hi[2]; ++c[2]) {
        const int s = hash_insert(keys, slots, voxel_key(c));      // (the key is there since the assign: a lookup)
        if (s < 0) continue;
        const long at = (long)start[s] + (long)atomicAdd(cursor + s, 1);
        if (at >= 0 && at < pairs) records[at] = (int)i;          // (the populations sum to `pairs`: always inside)
      }
}

__device__ __forceinline__ double dot3d(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void cross3d(const double *a, const double *b, double *c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// The closest point of the face p to q (normative): its fp32 position x32, clamped to the face's
// box, the fp64 barycentric weights w, and the fp32 squared distance of q to x32 by cloud_walk's operations.
__device__ __forceinline__ float nearest_closest(const float *q, const float (*p)[3], float *x32, double *w) {
  double P[3][3], qd[3], ab[3], ac[3], aq[3], n[3], x[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    P[0][k] = (double)p[0][k], P[1][k] = (double)p[1][k], P[2][k] = (double)p[2][k], qd[k] = (double)q[k];
    ab[k] = P[1][k] - P[0][k], ac[k] = P[2][k] - P[0][k], aq[k] = qd[k] - P[0][k];
  }
  cross3d(ab, ac, n);
  const double nn = dot3d(n, n);
  bool inside = false;
  if (nn > 0.0) {
    double t1[3], t2[3];
    cross3d(aq, ac, t1);
    cross3d(ab, aq, t2);
    const double wb = dot3d(t1, n) / nn, wc = dot3d(t2, n) / nn;
    const double wa = (1.0 - wb) - wc;
    if (wb >= 0.0 && wc >= 0.0 && wa >= 0.0) {
      inside = true;
      w[0] = wa, w[1] = wb, w[2] = wc;
#pragma unroll
      for (int k = 0; k < 3; ++k) x[k] = (P[0][k] + wb * ab[k]) + wc * ac[k];
    }
  }
  if (!inside) {
    double best = 0.0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {                         // the sides (a,b), (b,c), (c,a): ties to the earlier
      const int s1 = (s + 1) % 3, s2 = (s + 2) % 3;
      double e[3], d[3], xs[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) e[k] = P[s1][k] - P[s][k], d[k] = qd[k] - P[s][k];
      const double ee = dot3d(e, e);
      double t = 0.0;
      if (ee > 0.0) {
        const double r = dot3d(d, e) / ee;
        t = r > 0.0 ? (r < 1.0 ? r : 1.0) : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) xs[k] = P[s][k] + t * e[k], d[k] = qd[k] - xs[k];
      const double dd = dot3d(d, d);
      if (s == 0 || dd < best) {
        best = dd;
        x[0] = xs[0], x[1] = xs[1], x[2] = xs[2];
        w[s] = 1.0 - t, w[s1] = t, w[s2] = 0.0;
      }
    }
  }
  float df[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float mn = p[1][k] < p[0][k] ? p[1][k] : p[0][k], mx = p[1][k] > p[0][k] ? p[1][k] : p[0][k];
    mn = p[2][k] < mn ? p[2][k] : mn, mx = p[2][k] > mx ? p[2][k] : mx;
    const float xf = (float)x[k];
    x32[k] = xf < mn ? mn : (xf > mx ? mx : xf);
    df[k] = q[k] - x32[k];
  }
  return (df[0] * df[0] + df[1] * df[1]) + df[2] * df[2];
}

__global__ __launch_bounds__(MN_THREADS) void nearest_query_kernel(
    const float *__restrict__ query, long nq, const float *__restrict__ vertices, long m,
    const int64_t *__restrict__ faces, long f, float inv, float r2, const unsigned long long *__restrict__ keys,
    const int *__restrict__ pop, const int *__restrict__ start, const int *__restrict__ records, size_t slots, long pairs,
    const int *__restrict__ large_rows, long large, float *__restrict__ dist2, int64_t *__restrict__ face,
    float *__restrict__ point, float *__restrict__ weights, int *__restrict__ within) {
  const long i = (long)blockIdx.x * MN_THREADS + threadIdx.x;
  if (i >= nq) return;
  const float q[3] = {query[i * 3], query[i * 3 + 1], query[i * 3 + 2]};
  const CloudIndex ix = {keys, pop, start, slots};
  int count = 0;
  unsigned long long best = ~0ull;
  const bool visits = cloud_cells(q[0], q[1], q[2], inv, r2, ix, pairs,
                                  [&](const int *c, const int *lo, long from, long to) {
    for (long j = from; j < to; ++j) {
      const long row = (long)records[j];
      if (row < 0 || row >= f) continue;                   // (a built record is a face row: always inside)
      float p[3][3];
      int flo[3], fhi[3];
      if (nearest_face_box(vertices, m, faces, row, inv, p, flo, fhi) != MN_BOXED) continue;
      // once per query: only in the lowest cell that the query's range and the face's box share
      if (c[0] != max(lo[0], flo[0]) || c[1] != max(lo[1], flo[1]) || c[2] != max(lo[2], flo[2])) continue;
      float x32[3];
      double w[3];
      const float d2 = nearest_closest(q, p, x32, w);
      if (d2 <= r2) {
        ++count;
        const unsigned long long k = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)row;
        best = k < best ? k : best;
      }
    }
  });
  // (a query without cells is farther than max_dist from every point of a face that has a box)
  if (visits) {
    for (long j = 0; j < large; ++j) {                     // the large faces: every query tests each directly
      const long row = (long)large_rows[j];
      if (row < 0 || row >= f) continue;
      float p[3][3];
      int flo[3], fhi[3];
      if (nearest_face_box(vertices, m, faces, row, inv, p, flo, fhi) != MN_BOXED) continue;
      float x32[3];
      double w[3];
      const float d2 = nearest_closest(q, p, x32, w);
      if (d2 <= r2) {
        ++count;
        const unsigned long long k = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)row;
        best = k < best ? k : best;
      }
    }
  }
  float x32[3] = {0.0f, 0.0f, 0.0f};
  double w[3] = {0.0, 0.0, 0.0};
  bool any = best != ~0ull;
  if (any) {                                                // the winner again: the same function, the same bits
    float p[3][3];
    int flo[3], fhi[3];
    any = nearest_face_box(vertices, m, faces, (long)(best & 0xffffffffull), inv, p, flo, fhi) == MN_BOXED;
    if (any) nearest_closest(q, p, x32, w);
  }
  dist2[i] = any ? __uint_as_float((unsigned)(best >> 32)) : __builtin_inff();
  face[i] = any ? (int64_t)(best & 0xffffffffull) : (int64_t)-1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    point[i * 3 + k] = any ? x32[k] : 0.0f;
    weights[i * 3 + k] = any ? (float)w[k] : 0.0f;
  }
  within[i] = any ? count : 0;
}

}  // namespace mvsn

extern "C" int mvsn_mesh_nearest_box_cells(void) { return MVSN_MESH_NEAREST_BOX_CELLS; }

extern "C" size_t mvsn_mesh_nearest_workspace_bytes(long n_pairs, long n_large) {
  if (!mvsn::nearest_sizes_ok(n_pairs, n_large)) return 0;
  return mvsn::nearest_layout(n_pairs, n_large).bytes;
}

// the checks the three entries share
static int nearest_check_mesh(const char *who, const float *vertices, long n_vertices, const int64_t *faces, long n_faces,
                              float inv_cell) {
  using namespace mvsn;
  MVSN_REQUIRE(vertices && faces, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(n_vertices > 0 && n_faces > 0, MVSN_E_BADARG, "%s: %ld vertices and %ld faces", who, n_vertices, n_faces);
  MVSN_REQUIRE(n_vertices <= MESH_MAX_ROWS && n_faces <= MESH_MAX_ROWS, MVSN_E_TOOLARGE,
               "%s: %ld vertices and %ld faces (at most 2^31 - 1 each)", who, n_vertices, n_faces);
  MVSN_REQUIRE(inv_cell > 0.0f && inv_cell <= 3.0e38f, MVSN_E_BADARG,
               "%s: inverse cell size %g is not a positive finite number", who, (double)inv_cell);
  return 0;
}

static int nearest_check_workspace(const char *who, long n_pairs, long n_large, const void *workspace,
                                   size_t workspace_bytes, mvsn::NearestLayout *l) {
  using namespace mvsn;
  MVSN_REQUIRE(n_pairs >= 0 && n_large >= 0, MVSN_E_BADARG, "%s: %ld pairs and %ld large faces", who, n_pairs, n_large);
  MVSN_REQUIRE(n_pairs <= MESH_MAX_ROWS && n_large <= MESH_MAX_ROWS, MVSN_E_TOOLARGE,
               "%s: %ld pairs and %ld large faces (at most 2^31 - 1 each)", who, n_pairs, n_large);
  *l = nearest_layout(n_pairs, n_large);
  return workspace_check(who, "workspace", workspace, workspace_bytes, l->bytes);
}

extern "C" int mvsn_mesh_nearest_count(const float *vertices, long n_vertices, const int64_t *faces, long n_faces,
                                       float inv_cell, int64_t *result, mvsn_stream_t stream) {
  using namespace mvsn;
  if (int e = nearest_check_mesh("mvsn_mesh_nearest_count", vertices, n_vertices, faces, n_faces, inv_cell)) return e;
  MVSN_REQUIRE(result, MVSN_E_BADARG, "mvsn_mesh_nearest_count: null pointer");
  const hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(result, 0, 3 * sizeof(int64_t), st);
  MVSN_REQUIRE(e == hipSuccess, (int)e, "mvsn_mesh_nearest_count: clearing the result: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(nearest_count_kernel, dim3((unsigned)((n_faces + MN_THREADS - 1) / MN_THREADS)), dim3(MN_THREADS), 0,
                     st, vertices, n_vertices, faces, n_faces, inv_cell, (unsigned long long *)result);
  return check_launch("mvsn_mesh_nearest_count: count");
}

extern "C" int mvsn_mesh_nearest_build(const float *vertices, long n_vertices, const int64_t *faces, long n_faces,
                                       float inv_cell, long n_pairs, long n_large, void *workspace,
                                       size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  if (int e = nearest_check_mesh("mvsn_mesh_nearest_build", vertices, n_vertices, faces, n_faces, inv_cell)) return e;
  NearestLayout l;
  if (int e = nearest_check_workspace("mvsn_mesh_nearest_build", n_pairs, n_large, workspace, workspace_bytes, &l)) return e;
  char *ws = (char *)workspace;
  unsigned long long *head = (unsigned long long *)(ws + l.head), *keys = (unsigned long long *)(ws + l.keys);
  int *pop = (int *)(ws + l.pop), *start = (int *)(ws + l.start), *cursor = (int *)(ws + l.cursor);
  int *records = (int *)(ws + l.records), *large_rows = (int *)(ws + l.large), *counts = (int *)(ws + l.counts);
  int64_t *offsets = (int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 fgrid((unsigned)((n_faces + MN_THREADS - 1) / MN_THREADS)), block(MN_THREADS);
  const hipError_t e = hipMemsetAsync(head, 0, 2 * sizeof(unsigned long long), st);
  MVSN_REQUIRE(e == hipSuccess, (int)e, "mvsn_mesh_nearest_build: clearing the head: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(cloud_init_kernel, dim3((unsigned)l.blocks), dim3(CL_THREADS), 0, st, keys, pop, cursor, head);
  if (int e = check_launch("mvsn_mesh_nearest_build: table init")) return e;
  hipLaunchKernelGGL(nearest_assign_kernel, fgrid, block, 0, st, vertices, n_vertices, faces, n_faces, inv_cell, keys, pop,
                     l.slots);
  if (int e = check_launch("mvsn_mesh_nearest_build: assign")) return e;
  hipLaunchKernelGGL(cloud_count_kernel, dim3((unsigned)l.blocks), dim3(CL_THREADS), 0, st, (const int *)pop, counts);
  if (int e = check_launch("mvsn_mesh_nearest_build: count")) return e;
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)counts, l.blocks, offsets,
                     (int64_t *)nullptr);
  if (int e = check_launch("mvsn_mesh_nearest_build: scan")) return e;
  hipLaunchKernelGGL(cloud_start_kernel, dim3((unsigned)l.blocks), dim3(CL_THREADS), 0, st, (const int *)pop,
                     (const int64_t *)offsets, start);
  if (int e = check_launch("mvsn_mesh_nearest_build: start")) return e;
  hipLaunchKernelGGL(nearest_scatter_kernel, fgrid, block, 0, st, vertices, n_vertices, faces, n_faces, inv_cell, keys,
                     l.slots, (const int *)start, cursor, records, n_pairs, large_rows, n_large, head + 1);
  return check_launch("mvsn_mesh_nearest_build: scatter");
}

extern "C" int mvsn_mesh_nearest(const float *query, long nq, const float *vertices, long n_vertices,
                                 const int64_t *faces, long n_faces, float inv_cell, float r2, long n_pairs, long n_large,
                                 const void *workspace, size_t workspace_bytes, float *dist2, int64_t *face, float *point,
                                 float *weights, int *within, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(query && dist2 && face && point && weights && within, MVSN_E_BADARG, "mvsn_mesh_nearest: null pointer");
  MVSN_REQUIRE(nq > 0, MVSN_E_BADARG, "mvsn_mesh_nearest: %ld queries", nq);
  MVSN_REQUIRE(nq <= MESH_MAX_ROWS, MVSN_E_TOOLARGE, "mvsn_mesh_nearest: %ld queries (at most 2^31 - 1)", nq);
  if (int e = nearest_check_mesh("mvsn_mesh_nearest", vertices, n_vertices, faces, n_faces, inv_cell)) return e;
  MVSN_REQUIRE(r2 > 0.0f && r2 <= 3.0e38f, MVSN_E_BADARG,
               "mvsn_mesh_nearest: squared radius %g is not a positive finite number", (double)r2);
  NearestLayout l;
  if (int e = nearest_check_workspace("mvsn_mesh_nearest", n_pairs, n_large, workspace, workspace_bytes, &l)) return e;
  const int *records;
  const CloudIndex ix = cloud_index(workspace, l, &records);
  hipLaunchKernelGGL(nearest_query_kernel, dim3((unsigned)((nq + MN_THREADS - 1) / MN_THREADS)), dim3(MN_THREADS), 0,
                     (hipStream_t)stream, query, nq, vertices, n_vertices, faces, n_faces, inv_cell, r2, ix.keys, ix.pop,
                     ix.start, records, ix.slots, n_pairs, (const int *)((const char *)workspace + l.large), n_large, dist2,
                     face, point, weights, within);
  return check_launch("mvsn_mesh_nearest: query");
}
