// The unique edges of a triangle mesh (see include/mvsn_hip.h: mvsn_mesh_edges_*; the semantics are DESIGN.md section
// 29).  Side s of face r = (v0, v1, v2) runs from v_s to v_(s+1)%3 and has the index 3 r + s; a face with an index
// outside [0, m) takes no part, nor does a side with equal ends.  An edge is the unordered pair of a side's ends.
//
// mvsn_mesh_edges_mark, one host read (E, status) behind it:
//   edges_init_kernel     the table emptied: keys, minima, counts, windings; the result words
//   edges_insert_kernel   one thread per side: the packed key (low << 32) | high into the set (hash_insert: a
//                         compare-and-swap that only replaces the empty slot), then beside the slot atomicMin of the side
//                         index, atomicAdd of 1 and atomicAdd of +1 (low -> high) or -1 (high -> low)
//   edges_count_kernel    a side owns its edge iff the slot's minimum is its own index; owners per workgroup;
//                         geom_scan_kernel
// mvsn_mesh_edges_emit:
//   edges_vertex_init_kernel   degrees and border flags zeroed
//   edges_emit_kernel     the owners compacted in side order (block_rank): the pair, first, count, winding; the row goes
//                         back to the slot; the edge adds 1 to the degree of both ends and flags them where its count is 1
//   edges_face_kernel     one thread per side: the row of its slot, -1 for a side that takes no part
//
// Every atomic is an integer one whose result does not depend on arrival order: which slot an edge occupies depends on
// the race, nothing that leaves this file does.  Every probe loop is bounded by the table size; no thread waits for
// another.  tests/mesh_smooth_reference.py repeats it in numpy byte for byte.
#pragma clang fp contract(off)
#include "mvsn_common.h"
#include "mvsn_geom.h"
#include "mvsn_mesh.h"
#include "mvsn_voxel.h"

namespace mvsn {

constexpr int ME_THREADS = 256;                         // one side, slot or vertex per thread
constexpr long ME_MAX_FACES = 0x7fffffffL / 3;          // a side index is an int32
constexpr size_t ME_MIN_SLOTS = 1024;
constexpr int ME_NO_SIDE = 0x7fffffff;

// byte offsets of the workspace sections (each 256-byte aligned)
struct EdgesLayout {
  size_t keys, minside, count, wind, row, sslot, counts, offsets, bytes;
  size_t slots;             // power of two >= 6 f
  long sides, sblocks;      // 3 f, and the workgroups of the count / rank kernels
};

inline EdgesLayout edges_layout(long f) {
  EdgesLayout l;
  l.sides = 3 * f;
  l.slots = hash_table_slots(l.sides, ME_MIN_SLOTS);
  l.sblocks = (l.sides + ME_THREADS - 1) / ME_THREADS;
  l.keys = 0;
  l.minside = align256(l.keys + sizeof(uint64_t) * l.slots);
  l.count = align256(l.minside + sizeof(int) * l.slots);
  l.wind = align256(l.count + sizeof(int) * l.slots);
  l.row = align256(l.wind + sizeof(int) * l.slots);
  l.sslot = align256(l.row + sizeof(int) * l.slots);
  l.counts = align256(l.sslot + sizeof(int) * (size_t)l.sides);
  l.offsets = align256(l.counts + sizeof(int) * (size_t)l.sblocks);
  l.bytes = align256(l.offsets + sizeof(int64_t) * (size_t)l.sblocks);
  return l;
}

__global__ __launch_bounds__(ME_THREADS) void edges_init_kernel(unsigned long long *__restrict__ keys,
                                                                int *__restrict__ minside, int *__restrict__ count,
                                                                int *__restrict__ wind, long slots,
                                                                int64_t *__restrict__ result) {
  const long i = (long)blockIdx.x * ME_THREADS + threadIdx.x;
  if (i < slots) {
    keys[i] = VX_EMPTY;
    minside[i] = ME_NO_SIDE;
    count[i] = 0;
    wind[i] = 0;
  }
  if (i < 2) result[i] = 0;
}

// The ends of side i, low first; false (nothing beyond the face's own row dereferenced) when the face has a corner
// outside [0, m) or the side's ends are equal.  up: the side runs low -> high.
__device__ __forceinline__ bool edges_side(const int64_t *__restrict__ faces, long m, long i, int64_t *lo, int64_t *hi,
                                           bool *up) {
  const long r = i / 3;
  const int s = (int)(i - r * 3);
  int64_t v[3];
  if (!face_rows(faces, r, m, v)) return false;
  // (selects, not v[s]: an array indexed by a variable would be placed in LDS)
  const int64_t a = s == 0 ? v[0] : s == 1 ? v[1] : v[2], b = s == 0 ? v[1] : s == 1 ? v[2] : v[0];
  if (a == b) return false;
  *up = a < b;
  *lo = *up ? a : b;
  *hi = *up ? b : a;
  return true;
}

__global__ __launch_bounds__(ME_THREADS) void edges_insert_kernel(const int64_t *__restrict__ faces, long m, long sides,
                                                                  unsigned long long *__restrict__ keys, size_t slots,
                                                                  int *__restrict__ minside, int *__restrict__ count,
                                                                  int *__restrict__ wind, int *__restrict__ sslot,
                                                                  int64_t *__restrict__ result) {
  const long i = (long)blockIdx.x * ME_THREADS + threadIdx.x;
  if (i >= sides) return;
  int64_t lo, hi;
  bool up;
  int found = -1;
  if (edges_side(faces, m, i, &lo, &hi, &up)) {
    found = hash_insert(keys, slots, ((unsigned long long)lo << 32) | (unsigned long long)hi);   // (lo < 2^31: never the empty key)
    if (found >= 0) {
      atomicMin(minside + found, (int)i);
      atomicAdd(count + found, 1);
      atomicAdd(wind + found, up ? 1 : -1);
    } else {
      atomicOr(reinterpret_cast<unsigned long long *>(result) + 1, (unsigned long long)MVSN_MESH_EDGES_STATUS_TABLE);
    }
  }
  sslot[i] = found;
}

__device__ __forceinline__ bool edges_owner(const int *__restrict__ sslot, const int *__restrict__ minside, long sides,
                                            long i) {
  if (i >= sides) return false;
  const int h = sslot[i];
  return h >= 0 && (long)minside[h] == i;
}

__global__ __launch_bounds__(ME_THREADS) void edges_count_kernel(const int *__restrict__ sslot,
                                                                 const int *__restrict__ minside, long sides,
                                                                 int *__restrict__ block_counts) {
  __shared__ int swave[ME_THREADS / 64];
  const long i = (long)blockIdx.x * ME_THREADS + threadIdx.x;
  const int total = block_sum_256(edges_owner(sslot, minside, sides, i) ? 1 : 0, swave);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(ME_THREADS) void edges_vertex_init_kernel(int *__restrict__ degree,
                                                                       uint8_t *__restrict__ boundary, long m) {
  const long i = (long)blockIdx.x * ME_THREADS + threadIdx.x;
  if (i >= m) return;
  degree[i] = 0;
  boundary[i] = 0;
}

__global__ __launch_bounds__(ME_THREADS) void edges_emit_kernel(
    const int *__restrict__ sslot, const int *__restrict__ minside, const unsigned long long *__restrict__ keys,
    const int *__restrict__ count, const int *__restrict__ wind, long sides, long m,
    const int64_t *__restrict__ offsets, long capacity, int *__restrict__ slot_row, int64_t *__restrict__ edges,
    int64_t *__restrict__ first, int *__restrict__ face_count, int *__restrict__ winding, int *__restrict__ degree,
    uint8_t *__restrict__ boundary) {
  __shared__ int swave[ME_THREADS / 64];
  const long i = (long)blockIdx.x * ME_THREADS + threadIdx.x;
  const bool flag[1] = {edges_owner(sslot, minside, sides, i)};
  const int64_t row = offsets[blockIdx.x] + block_rank(flag, swave);
  if (!flag[0] || row >= capacity) return;               // (capacity = the scanned total: always true of an owner)
  const int h = sslot[i];
  const unsigned long long key = keys[h];
  const int64_t lo = (int64_t)(key >> 32), hi = (int64_t)(key & 0xffffffffull);
  if (lo >= m || hi >= m) return;                        // (an inserted key: never)
  const int n = count[h];
  slot_row[h] = (int)row;
  edges[row * 2] = lo;
  edges[row * 2 + 1] = hi;
  first[row] = i;
  face_count[row] = n;
  winding[row] = wind[h];
  atomicAdd(degree + lo, 1);
  atomicAdd(degree + hi, 1);
  if (n == 1) boundary[lo] = 1, boundary[hi] = 1;        // (every writer stores the same byte)
}

__global__ __launch_bounds__(ME_THREADS) void edges_face_kernel(const int *__restrict__ sslot,
                                                                const int *__restrict__ slot_row, long sides,
                                                                long capacity, int64_t *__restrict__ face_edge) {
  const long i = (long)blockIdx.x * ME_THREADS + threadIdx.x;
  if (i >= sides) return;
  const int h = sslot[i];
  int64_t row = -1;
  if (h >= 0) {
    row = (int64_t)slot_row[h];
    if (row >= capacity) row = -1;                       // (never: the owner of every used slot wrote its row)
  }
  face_edge[i] = row;
}

inline unsigned edges_blocks(long n) { return (unsigned)((n + ME_THREADS - 1) / ME_THREADS); }

}  // namespace mvsn

extern "C" size_t mvsn_mesh_edges_workspace_bytes(long n_vertices, long n_faces) {
  if (n_vertices <= 0 || n_vertices > mvsn::MESH_MAX_ROWS || n_faces <= 0 || n_faces > mvsn::ME_MAX_FACES) return 0;
  return mvsn::edges_layout(n_faces).bytes;
}

// the checks of the counts and of the workspace that the two entries share (each has rejected its null pointers, and
// emit its edge count, before); `l` is filled when they pass
static int edges_check(const char *who, long m, long f, const void *workspace, size_t workspace_bytes,
                       mvsn::EdgesLayout *l) {
  using namespace mvsn;
  MVSN_REQUIRE(m <= MESH_MAX_ROWS && f <= ME_MAX_FACES, MVSN_E_TOOLARGE,
               "%s: %ld vertices, %ld faces (at most 2^31 - 1 vertices and (2^31 - 1) / 3 faces)", who, m, f);
  *l = edges_layout(f);
  return workspace_check(who, "workspace", workspace, workspace_bytes, l->bytes);
}

extern "C" int mvsn_mesh_edges_mark(const int64_t *faces, long n_vertices, long n_faces, int64_t *result, void *workspace,
                                    size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  const long m = n_vertices, f = n_faces;
  MVSN_REQUIRE(faces && result && workspace, MVSN_E_BADARG, "mvsn_mesh_edges_mark: null pointer");
  MVSN_REQUIRE(m > 0 && f > 0, MVSN_E_BADARG, "mvsn_mesh_edges_mark: %ld vertices, %ld faces", m, f);
  EdgesLayout l;
  if (int e = edges_check("mvsn_mesh_edges_mark", m, f, workspace, workspace_bytes, &l)) return e;
  char *ws = (char *)workspace;
  unsigned long long *keys = (unsigned long long *)(ws + l.keys);
  int *minside = (int *)(ws + l.minside), *count = (int *)(ws + l.count), *wind = (int *)(ws + l.wind);
  int *sslot = (int *)(ws + l.sslot), *counts = (int *)(ws + l.counts);
  int64_t *offsets = (int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(edges_init_kernel, dim3(edges_blocks((long)l.slots)), dim3(ME_THREADS), 0, st, keys, minside, count,
                     wind, (long)l.slots, result);
  if (int e = check_launch("mvsn_mesh_edges_mark: init")) return e;
  hipLaunchKernelGGL(edges_insert_kernel, dim3((unsigned)l.sblocks), dim3(ME_THREADS), 0, st, faces, m, l.sides, keys,
                     l.slots, minside, count, wind, sslot, result);
  if (int e = check_launch("mvsn_mesh_edges_mark: insert")) return e;
  hipLaunchKernelGGL(edges_count_kernel, dim3((unsigned)l.sblocks), dim3(ME_THREADS), 0, st, (const int *)sslot,
                     (const int *)minside, l.sides, counts);
  if (int e = check_launch("mvsn_mesh_edges_mark: count")) return e;
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)counts, l.sblocks, offsets,
                     result);
  return check_launch("mvsn_mesh_edges_mark: scan");
}

extern "C" int mvsn_mesh_edges_emit(long n_vertices, long n_faces, void *workspace, size_t workspace_bytes, long n_edges,
                                    int64_t *edges, int64_t *first, int *face_count, int *winding, int64_t *face_edge,
                                    int *vertex_degree, uint8_t *vertex_boundary, mvsn_stream_t stream) {
  using namespace mvsn;
  const long m = n_vertices, f = n_faces;
  MVSN_REQUIRE(workspace && face_edge && vertex_degree && vertex_boundary, MVSN_E_BADARG,
               "mvsn_mesh_edges_emit: null pointer");
  MVSN_REQUIRE(m > 0 && f > 0 && n_edges >= 0 && (f > ME_MAX_FACES || n_edges <= 3 * f), MVSN_E_BADARG,
               "mvsn_mesh_edges_emit: %ld vertices, %ld faces, %ld edges", m, f, n_edges);
  MVSN_REQUIRE(n_edges == 0 || (edges && first && face_count && winding), MVSN_E_BADARG,
               "mvsn_mesh_edges_emit: null edge output");
  EdgesLayout l;
  if (int e = edges_check("mvsn_mesh_edges_emit", m, f, workspace, workspace_bytes, &l)) return e;
  char *ws = (char *)workspace;                          // (row, a section of it, is written here)
  const int *sslot = (const int *)(ws + l.sslot);
  int *slot_row = (int *)(ws + l.row);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(edges_vertex_init_kernel, dim3(edges_blocks(m)), dim3(ME_THREADS), 0, st, vertex_degree,
                     vertex_boundary, m);
  if (int e = check_launch("mvsn_mesh_edges_emit: vertices")) return e;
  if (n_edges > 0) {
    hipLaunchKernelGGL(edges_emit_kernel, dim3((unsigned)l.sblocks), dim3(ME_THREADS), 0, st, sslot,
                       (const int *)(ws + l.minside), (const unsigned long long *)(ws + l.keys),
                       (const int *)(ws + l.count), (const int *)(ws + l.wind), l.sides, m,
                       (const int64_t *)(ws + l.offsets), n_edges, slot_row, edges, first, face_count, winding,
                       vertex_degree, vertex_boundary);
    if (int e = check_launch("mvsn_mesh_edges_emit: edges")) return e;
  }
  hipLaunchKernelGGL(edges_face_kernel, dim3((unsigned)l.sblocks), dim3(ME_THREADS), 0, st, sslot, (const int *)slot_row,
                     l.sides, n_edges, face_edge);
  return check_launch("mvsn_mesh_edges_emit: faces");
}
