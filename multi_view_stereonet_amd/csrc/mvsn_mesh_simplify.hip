// Vertex-clustering simplification of a triangle mesh (see include/mvsn_hip.h: mvsn_mesh_simplify_*; the semantics and
// every operation are DESIGN.md section 28): the vertices of one cell of the voxel grid become one vertex, the faces are
// remapped through the clustering, collapsed and repeated faces go, and with the quadric placement the new vertex is the
// point of the cell nearest the planes of the faces around it.
//
// mvsn_mesh_simplify_assign is mvsn_voxel_assign on the vertices (cell, key, slot, first row, count and scan: the
// clusters ARE voxel_merge's voxels); one host read (clusters, status) behind it.
// mvsn_mesh_simplify_mark, one host read (M', F', status, fallbacks) behind it:
//   mvsn_voxel_merge          rank, accumulate, finalise: mean position and colour, count, first and the cluster of
//                             every vertex, into the workspace; mvsn_voxel_normals: the direction of the normals' sum
//   simplify_init_kernel      quadric sums zeroed, cluster flags, the face table emptied, the result words
//   simplify_quadric_kernel   one thread per face: the unit normal in fp64 once, then per distinct cluster of its corners
//                             the terms n n^T, d n and the incidence count, quantised to 2^-30, 64-bit integer atomicAdd
//   simplify_place_kernel     one thread per cluster: (A + lambda k I) x = -b + lambda k u_mean by the closed-form inverse
//                             in fp64, clamped to the cell, mapped back and rounded once; whatever the placement the
//                             position must lie in the cluster's cell by voxel_cell, else it becomes the first member's
//   simplify_insert_kernel    one thread per face: remap, classify, canonical triple, insert into the set of faces (an
//                             int32 table of face rows: compare-and-swap on an empty slot, atomicMin of the row where the
//                             occupant's triple, read through its row, equals mine)
//   simplify_mark_kernel      a face survives iff its slot holds its own row; survivors flag their clusters; count per
//                             workgroup; simplify_cluster_count_kernel the same for the clusters; geom_scan_kernel twice
// mvsn_mesh_simplify_emit: the clusters and the faces compacted in order (block_rank), inverse through the cluster's row.
//
// Every atomic is an integer one whose result does not depend on arrival order (a compare-and-swap that only replaces
// the empty slot, minima, sums): which slot a class of equal faces owns depends on the race, nothing that leaves this
// file does.  Every loop is bounded by the table size; no thread waits for another.  fp64 with + - x / sqrt and
// compares only; contraction is off for the whole file: every step of section 28 is one operation, and
// tests/mesh_simplify_reference.py repeats it in numpy bit for bit.
#pragma clang fp contract(off)
#include "mvsn_common.h"
#include "mvsn_geom.h"
#include "mvsn_mesh.h"
#include "mvsn_voxel.h"

namespace mvsn {

constexpr int MS_THREADS = 256;                         // one vertex, cluster or face per thread
constexpr size_t MS_MIN_SLOTS = 1024;
constexpr int MS_QUAD_WORDS = 10;                       // xx xy xz yy yz zz, dx dy dz, k
constexpr int MS_VOXEL_ROW_WORDS = 8;                   // mvsn_voxel.hip's accumulator row: sum qx qy qz, r g b, count, key
constexpr double MS_QUANT = 1073741824.0;               // 2^30 steps per unit
constexpr double MS_LAMBDA = 1.0 / 1024.0;              // pull towards the mean, per incidence (section 28)
constexpr double MS_CLAMP = 0.5 - 1.0 / 1024.0;         // |x| <= this on every axis: inside the cell, off its faces
enum { MS_MEAN = 0, MS_QUADRIC = 1 };

// byte offsets of the workspace sections (each 256-byte aligned); sized by the vertices, used by the clusters
struct SimplifyLayout {
  size_t voxel, voxel_bytes, accum, cpoints, cnormals, ccolors, ccount, cfirst, cid, quad, nsum, used, crow, ccounts,
      coffsets, ftable, fslot, fcounts, foffsets, bytes;
  size_t fslots;            // power of two >= 2 f; 0 without faces
  long cblocks, fblocks;    // workgroups of the count / rank kernels (cblocks for m clusters, the most there can be)
};

inline SimplifyLayout simplify_layout(long m, long f) {
  SimplifyLayout l;
  const size_t M = (size_t)m, F = (size_t)f;
  l.fslots = f > 0 ? hash_table_slots(f, MS_MIN_SLOTS) : 0;
  l.cblocks = (m + MS_THREADS - 1) / MS_THREADS;
  l.fblocks = (f + MS_THREADS - 1) / MS_THREADS;
  l.voxel = 0;
  l.voxel_bytes = mvsn_voxel_workspace_bytes(m);
  l.accum = align256(l.voxel + l.voxel_bytes);
  l.cpoints = align256(l.accum + sizeof(uint64_t) * MS_VOXEL_ROW_WORDS * M);
  l.cnormals = align256(l.cpoints + sizeof(float) * 3 * M);
  l.ccolors = align256(l.cnormals + sizeof(float) * 3 * M);
  l.ccount = align256(l.ccolors + 3 * M);
  l.cfirst = align256(l.ccount + sizeof(int) * M);
  l.cid = align256(l.cfirst + sizeof(int64_t) * M);
  l.quad = align256(l.cid + sizeof(int64_t) * M);
  l.nsum = align256(l.quad + sizeof(uint64_t) * MS_QUAD_WORDS * M);
  l.used = align256(l.nsum + sizeof(uint64_t) * 3 * M);
  l.crow = align256(l.used + sizeof(int) * M);
  l.ccounts = align256(l.crow + sizeof(int) * M);
  l.coffsets = align256(l.ccounts + sizeof(int) * (size_t)l.cblocks);
  l.ftable = align256(l.coffsets + sizeof(int64_t) * (size_t)l.cblocks);
  l.fslot = align256(l.ftable + sizeof(int) * l.fslots);
  l.fcounts = align256(l.fslot + sizeof(int) * F);
  l.foffsets = align256(l.fcounts + sizeof(int) * (size_t)l.fblocks);
  l.bytes = align256(l.foffsets + sizeof(int64_t) * (size_t)l.fblocks);
  return l;
}

__global__ __launch_bounds__(MS_THREADS) void simplify_init_kernel(unsigned long long *__restrict__ quad, long quad_words,
                                                                   int *__restrict__ used, long clusters, int used_fill,
                                                                   int *__restrict__ ftable, long fslots,
                                                                   int64_t *__restrict__ result) {
  const long i = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  if (i < quad_words) quad[i] = 0ull;
  if (i < clusters) used[i] = used_fill;
  if (i < fslots) ftable[i] = -1;
  if (i < 4) result[i] = 0;
}

// The clusters of face r's corners; false (nothing beyond the face's own row dereferenced) when a corner lies outside
// [0, m) or is a dropped vertex.
__device__ __forceinline__ bool simplify_face_clusters(const int64_t *__restrict__ faces,
                                                       const int64_t *__restrict__ cid, long m, long clusters, long r,
                                                       int *g) {
  int64_t v[3];
  if (!face_rows(faces, r, m, v)) return false;
  const int64_t ga = cid[v[0]], gb = cid[v[1]], gc = cid[v[2]];
  if (!(ga >= 0 && ga < clusters && gb >= 0 && gb < clusters && gc >= 0 && gc < clusters)) return false;
  g[0] = (int)ga, g[1] = (int)gb, g[2] = (int)gc;
  return true;
}

__device__ __forceinline__ unsigned long long simplify_hash(const int *t) {
  return voxel_hash(voxel_hash(((unsigned long long)(unsigned)t[0] << 32) | (unsigned)t[1]) ^ (unsigned)t[2]);
}

__device__ __forceinline__ long long simplify_quantise(double x) { return (long long)rint(x * MS_QUANT); }   // half to even

__device__ __forceinline__ void simplify_add(unsigned long long *a, long long q) {
  if (q != 0) atomicAdd(a, (unsigned long long)q);     // two's complement: the unsigned sum is the signed one
}

__global__ __launch_bounds__(MS_THREADS) void simplify_quadric_kernel(const float *__restrict__ vertices, long m,
                                                                      const int64_t *__restrict__ faces, long f,
                                                                      const int64_t *__restrict__ cid, long clusters,
                                                                      float voxel_size, float inv, float ox, float oy,
                                                                      float oz, unsigned long long *__restrict__ quad) {
  const long r = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  if (r >= f) return;
  int64_t in[3], row[3];
  if (!face_rows(faces, r, m, in)) return;
  face_lead(in, row);                                    // the normal's bits do not depend on the corner the face starts with
  float pf[3][3];
  if (!face_points(vertices, row, pf)) return;
  double p[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) p[j][k] = (double)pf[j][k];
  int g[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int64_t c = cid[row[j]];
    if (c < 0 || c >= clusters) return;                  // (a finite vertex always has a cluster once the status is clear)
    g[j] = (int)c;
  }
  double cr[3];
  face_cross(p, cr);
  const double len = sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
  if (!(len > 0.0 && len <= 1.7e308)) return;            // no area (or no finite normal): adds nothing
  const double n[3] = {cr[0] / len, cr[1] / len, cr[2] / len};
  const long long qa[6] = {simplify_quantise(n[0] * n[0]), simplify_quantise(n[0] * n[1]), simplify_quantise(n[0] * n[2]),
                           simplify_quantise(n[1] * n[1]), simplify_quantise(n[1] * n[2]), simplify_quantise(n[2] * n[2])};
  const float o[3] = {ox, oy, oz};
  const double v = (double)voxel_size;
  long long qb[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    int c[3];
    unsigned q[3];
    voxel_cell(pf[j], inv, o, c, q);
    double u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = (p[j][k] - (double)o[k]) / v - ((double)c[k] + 0.5);
    const double d = -((n[0] * u[0] + n[1] * u[1]) + n[2] * u[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) qb[j][k] = simplify_quantise(d * n[k]);
  }
  // one set of atomics per distinct cluster: the integer terms of its corners summed first (the sums are exact either way)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    bool repeated = false;
#pragma unroll
    for (int l = 0; l < j; ++l) repeated = repeated || g[l] == g[j];
    if (repeated) continue;
    long long count = 0, sb[3] = {0, 0, 0};
#pragma unroll
    for (int l = j; l < 3; ++l)
      if (g[l] == g[j]) {
        ++count;
        sb[0] += qb[l][0], sb[1] += qb[l][1], sb[2] += qb[l][2];
      }
    unsigned long long *a = quad + (size_t)g[j] * MS_QUAD_WORDS;
#pragma unroll
    for (int e = 0; e < 6; ++e) simplify_add(a + e, count * qa[e]);
#pragma unroll
    for (int e = 0; e < 3; ++e) simplify_add(a + 6 + e, sb[e]);
    atomicAdd(a + 9, (unsigned long long)count);
  }
}

__global__ __launch_bounds__(MS_THREADS) void simplify_place_kernel(const float *__restrict__ vertices,
                                                                    const int64_t *__restrict__ cfirst, long clusters,
                                                                    const unsigned long long *__restrict__ accum,
                                                                    const unsigned long long *__restrict__ quad,
                                                                    int placement, float voxel_size, float inv, float ox,
                                                                    float oy, float oz, float *__restrict__ cpoints,
                                                                    int64_t *__restrict__ result) {
  const long c = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  if (c >= clusters) return;
  const float o[3] = {ox, oy, oz};
  const float *head = vertices + (size_t)cfirst[c] * 3;  // the first member: finite and in the cell, by definition
  const float member[3] = {head[0], head[1], head[2]};
  int cell[3];
  unsigned q[3];
  voxel_cell(member, inv, o, cell, q);
  float pos[3] = {cpoints[c * 3], cpoints[c * 3 + 1], cpoints[c * 3 + 2]};   // voxel_merge's mean
  if (placement == MS_QUADRIC) {
    const unsigned long long *s = accum + (size_t)c * MS_VOXEL_ROW_WORDS;
    const double nd = (double)s[6];
    double ub[3], x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = ub[k] = ((double)s[k] / nd + 0.5) / 65536.0 - 0.5;
    const unsigned long long *w = quad + (size_t)c * MS_QUAD_WORDS;
    const long long k_inc = (long long)w[9];
    if (k_inc > 0) {
      const double scale = 1.0 / MS_QUANT;               // a power of two: the products are exact
      const double lk = MS_LAMBDA * (double)k_inc;
      const double m00 = (double)(long long)w[0] * scale + lk, m01 = (double)(long long)w[1] * scale,
                   m02 = (double)(long long)w[2] * scale, m11 = (double)(long long)w[3] * scale + lk,
                   m12 = (double)(long long)w[4] * scale, m22 = (double)(long long)w[5] * scale + lk;
      const double r0 = lk * ub[0] - (double)(long long)w[6] * scale, r1 = lk * ub[1] - (double)(long long)w[7] * scale,
                   r2 = lk * ub[2] - (double)(long long)w[8] * scale;
      const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
      const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
      const double det = (m00 * c00 + m01 * c01) + m02 * c02;
      if (det > 0.0 && det <= 1.7e308) {                 // (A + lambda k I is positive definite: always)
        x[0] = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
        x[1] = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
        x[2] = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
      }
    }
    const double v = (double)voxel_size;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double xk = x[k] == x[k] ? x[k] : ub[k];
      xk = xk < -MS_CLAMP ? -MS_CLAMP : xk;
      xk = xk > MS_CLAMP ? MS_CLAMP : xk;
      pos[k] = (float)((double)o[k] + (((double)cell[k] + 0.5) + xk) * v);
    }
  }
  int got[3];
  const int state = voxel_cell(pos, inv, o, got, q);
  if (state != VX_KEPT || got[0] != cell[0] || got[1] != cell[1] || got[2] != cell[2]) {
    pos[0] = member[0], pos[1] = member[1], pos[2] = member[2];
    atomicAdd(reinterpret_cast<unsigned long long *>(result) + 3, 1ull);
  }
  cpoints[c * 3] = pos[0], cpoints[c * 3 + 1] = pos[1], cpoints[c * 3 + 2] = pos[2];
}

__global__ __launch_bounds__(MS_THREADS) void simplify_insert_kernel(const int64_t *__restrict__ faces, long f, long m,
                                                                     const int64_t *__restrict__ cid, long clusters,
                                                                     int *__restrict__ ftable, size_t fslots,
                                                                     int *__restrict__ fslot,
                                                                     int64_t *__restrict__ result) {
  const long r = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  if (r >= f) return;
  int g[3], mine[3];
  int found = -1;
  if (simplify_face_clusters(faces, cid, m, clusters, r, g) && g[0] != g[1] && g[1] != g[2] && g[0] != g[2]) {
    face_lead(g, mine);                                  // the canonical triple: three distinct ids, the winding stays
    const size_t mask = fslots - 1;
    size_t h = (size_t)simplify_hash(mine) & mask;
    for (size_t probe = 0; probe < fslots; ++probe) {
      int seen = __hip_atomic_load(ftable + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (seen < 0) seen = atomicCAS(ftable + h, -1, (int)r);
      if (seen < 0) {                                    // claimed: the slot's class is mine from now on
        found = (int)h;
        break;
      }
      // occupied, perhaps since the swap just failed: the same slot is examined.  Its row may fall, its class cannot.
      int og[3], theirs[3];
      simplify_face_clusters(faces, cid, m, clusters, (long)seen, og);   // (an inserted face: always true)
      face_lead(og, theirs);
      if (theirs[0] == mine[0] && theirs[1] == mine[1] && theirs[2] == mine[2]) {
        atomicMin(ftable + h, (int)r);
        found = (int)h;
        break;
      }
      h = (h + 1) & mask;
    }
    if (found < 0)
      atomicOr(reinterpret_cast<unsigned long long *>(result) + 2, (unsigned long long)MVSN_MESH_SIMPLIFY_STATUS_TABLE);
  }
  fslot[r] = found;
}

__global__ __launch_bounds__(MS_THREADS) void simplify_mark_kernel(const int64_t *__restrict__ faces, long f,
                                                                   const int64_t *__restrict__ cid,
                                                                   const int *__restrict__ ftable,
                                                                   int *__restrict__ fslot, int *__restrict__ used,
                                                                   int *__restrict__ block_counts) {
  __shared__ int swave[MS_THREADS / 64];
  const long r = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  bool survives = false;
  if (r < f) {
    const int s = fslot[r];
    survives = s >= 0 && (long)ftable[s] == r;
    if (survives) {                                      // (its rows and clusters were checked by the insert)
#pragma unroll
      for (int j = 0; j < 3; ++j) used[cid[faces[r * 3 + j]]] = 1;
    } else {
      fslot[r] = -1;
    }
  }
  const int total = block_sum_256(survives ? 1 : 0, swave);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MS_THREADS) void simplify_cluster_count_kernel(const int *__restrict__ used, long clusters,
                                                                            int *__restrict__ block_counts) {
  __shared__ int swave[MS_THREADS / 64];
  const long c = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  const int total = block_sum_256(c < clusters && used[c] != 0 ? 1 : 0, swave);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MS_THREADS) void simplify_cluster_emit_kernel(
    const int *__restrict__ used, long clusters, const int64_t *__restrict__ offsets, long capacity,
    const float *__restrict__ cpoints, const float *__restrict__ cnormals, const uint8_t *__restrict__ ccolors,
    const int *__restrict__ ccount, const int64_t *__restrict__ cfirst, int *__restrict__ crow,
    float *__restrict__ out_vertices, float *__restrict__ out_normals, uint8_t *__restrict__ out_colors,
    int *__restrict__ out_count, int64_t *__restrict__ out_first) {
  __shared__ int swave[MS_THREADS / 64];
  const long c = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  const bool flag[1] = {c < clusters && used[c] != 0};
  const int64_t row = offsets[blockIdx.x] + block_rank(flag, swave);
  if (c >= clusters) return;
  const bool kept = flag[0] && row < capacity;           // (capacity = the scanned total: always true of a flagged one)
  crow[c] = kept ? (int)row : -1;
  if (!kept) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    out_vertices[row * 3 + k] = cpoints[c * 3 + k];
    if (out_normals) out_normals[row * 3 + k] = cnormals[c * 3 + k];
    if (out_colors) out_colors[row * 3 + k] = ccolors[c * 3 + k];
  }
  out_count[row] = ccount[c];
  out_first[row] = cfirst[c];
}

__global__ __launch_bounds__(MS_THREADS) void simplify_inverse_kernel(const int64_t *__restrict__ cid, long m,
                                                                      long clusters, const int *__restrict__ crow,
                                                                      int64_t *__restrict__ inverse) {
  const long i = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  if (i >= m) return;
  const int64_t c = cid[i];
  inverse[i] = c >= 0 && c < clusters ? (int64_t)crow[c] : -1;
}

__global__ __launch_bounds__(MS_THREADS) void simplify_face_emit_kernel(const int64_t *__restrict__ faces, long f,
                                                                        const int64_t *__restrict__ cid,
                                                                        const int *__restrict__ crow,
                                                                        const int *__restrict__ fslot,
                                                                        const int64_t *__restrict__ offsets,
                                                                        long capacity, int64_t *__restrict__ out_faces,
                                                                        int64_t *__restrict__ face_rows) {
  __shared__ int swave[MS_THREADS / 64];
  const long r = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  const bool flag[1] = {r < f && fslot[r] >= 0};
  const int64_t row = offsets[blockIdx.x] + block_rank(flag, swave);
  if (!flag[0] || row >= capacity) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) out_faces[row * 3 + j] = (int64_t)crow[cid[faces[r * 3 + j]]];
  face_rows[row] = r;
}

inline unsigned simplify_blocks(long n) { return (unsigned)((n + MS_THREADS - 1) / MS_THREADS); }

}  // namespace mvsn

extern "C" size_t mvsn_mesh_simplify_workspace_bytes(long n_vertices, long n_faces) {
  if (n_vertices <= 0 || n_vertices > mvsn::MESH_MAX_ROWS || n_faces < 0 || n_faces > mvsn::MESH_MAX_ROWS) return 0;
  return mvsn::simplify_layout(n_vertices, n_faces).bytes;
}

extern "C" int mvsn_mesh_simplify_assign(const float *vertices, long n_vertices, float voxel_size, float inv_voxel_size,
                                         float origin_x, float origin_y, float origin_z, int64_t *result,
                                         void *workspace, size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(vertices && result, MVSN_E_BADARG, "mvsn_mesh_simplify_assign: null pointer");
  MVSN_REQUIRE(n_vertices > 0, MVSN_E_BADARG, "mvsn_mesh_simplify_assign: %ld vertices", n_vertices);
  MVSN_REQUIRE(n_vertices <= MESH_MAX_ROWS, MVSN_E_TOOLARGE, "mvsn_mesh_simplify_assign: %ld vertices (at most 2^31 - 1)",
               n_vertices);
  const size_t need = mvsn_voxel_workspace_bytes(n_vertices);
  if (int e = workspace_check("mvsn_mesh_simplify_assign", "workspace", workspace, workspace_bytes, need)) return e;
  return mvsn_voxel_assign(vertices, n_vertices, voxel_size, inv_voxel_size, origin_x, origin_y, origin_z, result,
                           workspace, need, stream);
}

extern "C" int mvsn_mesh_simplify_mark(const float *vertices, const float *normals, const uint8_t *colors,
                                       long n_vertices, const int64_t *faces, long n_faces, float voxel_size,
                                       float inv_voxel_size, float origin_x, float origin_y, float origin_z,
                                       int placement, int drop_unreferenced, long clusters, int64_t *result,
                                       void *workspace, size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  const long m = n_vertices, f = n_faces;
  MVSN_REQUIRE(vertices && result && workspace, MVSN_E_BADARG, "mvsn_mesh_simplify_mark: null pointer");
  MVSN_REQUIRE(m > 0 && f >= 0 && clusters > 0 && clusters <= m && (f == 0 || faces), MVSN_E_BADARG,
               "mvsn_mesh_simplify_mark: %ld clusters of %ld vertices, %ld faces", clusters, m, f);
  MVSN_REQUIRE(m <= MESH_MAX_ROWS && f <= MESH_MAX_ROWS, MVSN_E_TOOLARGE,
               "mvsn_mesh_simplify_mark: %ld vertices, %ld faces (at most 2^31 - 1 of either)", m, f);
  MVSN_REQUIRE(placement == MS_MEAN || placement == MS_QUADRIC, MVSN_E_BADARG,
               "mvsn_mesh_simplify_mark: placement %d (0 = mean, 1 = quadric)", placement);
  const SimplifyLayout l = simplify_layout(m, f);
  if (int e = workspace_check("mvsn_mesh_simplify_mark", "workspace", workspace, workspace_bytes, l.bytes)) return e;
  char *ws = (char *)workspace;
  unsigned long long *accum = (unsigned long long *)(ws + l.accum), *quad = (unsigned long long *)(ws + l.quad);
  float *cpoints = (float *)(ws + l.cpoints), *cnormals = (float *)(ws + l.cnormals);
  uint8_t *ccolors = (uint8_t *)(ws + l.ccolors);
  int *ccount = (int *)(ws + l.ccount), *used = (int *)(ws + l.used), *ccounts = (int *)(ws + l.ccounts);
  int64_t *cfirst = (int64_t *)(ws + l.cfirst), *cid = (int64_t *)(ws + l.cid), *coffsets = (int64_t *)(ws + l.coffsets);
  int *ftable = (int *)(ws + l.ftable), *fslot = (int *)(ws + l.fslot), *fcounts = (int *)(ws + l.fcounts);
  int64_t *foffsets = (int64_t *)(ws + l.foffsets);
  const hipStream_t st = (hipStream_t)stream;
  // the vertex side is the voxel merge itself, into the workspace
  if (int e = mvsn_voxel_merge(vertices, colors, m, voxel_size, inv_voxel_size, origin_x, origin_y, origin_z, ws + l.voxel,
                               l.voxel_bytes, clusters, accum, cpoints, colors ? ccolors : nullptr, ccount, cfirst, cid,
                               stream))
    return e;
  if (normals)
    if (int e = mvsn_voxel_normals(normals, cid, m, clusters, ws + l.nsum, cnormals, stream)) return e;
  const long quad_words = clusters * MS_QUAD_WORDS;
  const long init = max(max(quad_words, (long)l.fslots), 4L);
  hipLaunchKernelGGL(simplify_init_kernel, dim3(simplify_blocks(init)), dim3(MS_THREADS), 0, st, quad, quad_words, used,
                     clusters, drop_unreferenced ? 0 : 1, ftable, (long)l.fslots, result);
  if (int e = check_launch("mvsn_mesh_simplify_mark: init")) return e;
  if (placement == MS_QUADRIC && f > 0) {
    hipLaunchKernelGGL(simplify_quadric_kernel, dim3(simplify_blocks(f)), dim3(MS_THREADS), 0, st, vertices, m, faces, f,
                       (const int64_t *)cid, clusters, voxel_size, inv_voxel_size, origin_x, origin_y, origin_z, quad);
    if (int e = check_launch("mvsn_mesh_simplify_mark: quadric")) return e;
  }
  hipLaunchKernelGGL(simplify_place_kernel, dim3(simplify_blocks(clusters)), dim3(MS_THREADS), 0, st, vertices,
                     (const int64_t *)cfirst, clusters, (const unsigned long long *)accum,
                     (const unsigned long long *)quad, placement, voxel_size, inv_voxel_size, origin_x, origin_y,
                     origin_z, cpoints, result);
  if (int e = check_launch("mvsn_mesh_simplify_mark: place")) return e;
  if (f > 0) {
    hipLaunchKernelGGL(simplify_insert_kernel, dim3(simplify_blocks(f)), dim3(MS_THREADS), 0, st, faces, f, m,
                       (const int64_t *)cid, clusters, ftable, l.fslots, fslot, result);
    if (int e = check_launch("mvsn_mesh_simplify_mark: insert")) return e;
    hipLaunchKernelGGL(simplify_mark_kernel, dim3((unsigned)l.fblocks), dim3(MS_THREADS), 0, st, faces, f,
                       (const int64_t *)cid, (const int *)ftable, fslot, used, fcounts);
    if (int e = check_launch("mvsn_mesh_simplify_mark: mark")) return e;
    hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)fcounts, l.fblocks,
                       foffsets, result + 1);
    if (int e = check_launch("mvsn_mesh_simplify_mark: face scan")) return e;
  }
  const long cblocks = (clusters + MS_THREADS - 1) / MS_THREADS;
  hipLaunchKernelGGL(simplify_cluster_count_kernel, dim3((unsigned)cblocks), dim3(MS_THREADS), 0, st, (const int *)used,
                     clusters, ccounts);
  if (int e = check_launch("mvsn_mesh_simplify_mark: cluster count")) return e;
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)ccounts, cblocks, coffsets,
                     result);
  return check_launch("mvsn_mesh_simplify_mark: cluster scan");
}

extern "C" int mvsn_mesh_simplify_emit(const int64_t *faces, long n_vertices, long n_faces, long clusters,
                                       const void *workspace, size_t workspace_bytes, long out_vertices_n,
                                       long out_faces_n, float *out_vertices, int64_t *out_faces, float *out_normals,
                                       uint8_t *out_colors, int *count, int64_t *first, int64_t *inverse,
                                       int64_t *face_rows, mvsn_stream_t stream) {
  using namespace mvsn;
  const long m = n_vertices, f = n_faces;
  MVSN_REQUIRE(workspace && inverse, MVSN_E_BADARG, "mvsn_mesh_simplify_emit: null pointer");
  MVSN_REQUIRE(m > 0 && f >= 0 && clusters > 0 && clusters <= m && out_vertices_n >= 0 && out_vertices_n <= clusters &&
                   out_faces_n >= 0 && out_faces_n <= f,
               MVSN_E_BADARG, "mvsn_mesh_simplify_emit: %ld of %ld clusters of %ld vertices, %ld of %ld faces",
               out_vertices_n, clusters, m, out_faces_n, f);
  MVSN_REQUIRE(m <= MESH_MAX_ROWS && f <= MESH_MAX_ROWS, MVSN_E_TOOLARGE,
               "mvsn_mesh_simplify_emit: %ld vertices, %ld faces (at most 2^31 - 1 of either)", m, f);
  MVSN_REQUIRE(out_vertices_n == 0 || (out_vertices && count && first), MVSN_E_BADARG,
               "mvsn_mesh_simplify_emit: null vertex output");
  MVSN_REQUIRE(out_faces_n == 0 || (faces && out_faces && face_rows), MVSN_E_BADARG,
               "mvsn_mesh_simplify_emit: null face output");
  const SimplifyLayout l = simplify_layout(m, f);
  if (int e = workspace_check("mvsn_mesh_simplify_emit", "workspace", workspace, workspace_bytes, l.bytes)) return e;
  char *ws = (char *)workspace;                          // (crow, a section of it, is written here)
  const hipStream_t st = (hipStream_t)stream;
  const int64_t *cid = (const int64_t *)(ws + l.cid);
  int *crow = (int *)(ws + l.crow);
  const long cblocks = (clusters + MS_THREADS - 1) / MS_THREADS;
  hipLaunchKernelGGL(simplify_cluster_emit_kernel, dim3((unsigned)cblocks), dim3(MS_THREADS), 0, st,
                     (const int *)(ws + l.used), clusters, (const int64_t *)(ws + l.coffsets), out_vertices_n,
                     (const float *)(ws + l.cpoints), (const float *)(ws + l.cnormals),
                     (const uint8_t *)(ws + l.ccolors), (const int *)(ws + l.ccount), (const int64_t *)(ws + l.cfirst),
                     crow, out_vertices, out_normals, out_colors, count, first);
  if (int e = check_launch("mvsn_mesh_simplify_emit: clusters")) return e;
  hipLaunchKernelGGL(simplify_inverse_kernel, dim3(simplify_blocks(m)), dim3(MS_THREADS), 0, st, cid, m, clusters,
                     (const int *)crow, inverse);
  if (int e = check_launch("mvsn_mesh_simplify_emit: inverse")) return e;
  if (f > 0 && out_faces_n > 0) {
    hipLaunchKernelGGL(simplify_face_emit_kernel, dim3((unsigned)l.fblocks), dim3(MS_THREADS), 0, st, faces, f, cid,
                       (const int *)crow, (const int *)(ws + l.fslot), (const int64_t *)(ws + l.foffsets), out_faces_n,
                       out_faces, face_rows);
    if (int e = check_launch("mvsn_mesh_simplify_emit: faces")) return e;
  }
  return 0;
}
