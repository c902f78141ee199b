// Connected components of a triangle mesh, and the mesh of the components one keeps (see include/mvsn_hip.h:
// mvsn_mesh_*; the semantics, the termination and the visibility argument are DESIGN.md section 18).  The graph has the
// vertex rows as nodes and the sides of the faces as edges; a component's id is its rank among the components ordered by
// their lowest vertex row.
//
//   Labelling, three launches and the scan, one host read (C, status) behind them:
//   mesh_init_kernel         parent[v] = v; the head (C, status) zeroed
//   mesh_hook_kernel         one thread per face: unite (a, b) and (b, c) in a lock-free union-find over `parent`
//                            (mvsn_unionfind.h, shared with mvsn_cloud_cluster.hip).  The
//                            invariant, at every instant: parent[v] <= v, and parent[v] is a vertex of v's component.
//                            A root is hooked under a LOWER root by a compare-and-swap that expects it to be its own
//                            parent still, so the root of a finished component is its lowest vertex
//   mesh_flatten_kernel      one thread per vertex: parent[v] = the root of v; the roots of the workgroup counted
//   geom_scan_kernel         mvsn_geom.h's scan over those counts: the total is C
//   Emission, three launches:
//   mesh_rank_kernel         the roots ranked inside the workgroup (block_rank): root -> dense id, first[id] = root, the
//                            two counters of the id zeroed
//   mesh_vertex_label_kernel vertex_label[v] = id of the root of v, and 1 added to vertex_count[id]
//   mesh_face_label_kernel   face_label[f] = label of its first index (-1 for a face with an index outside [0, M)), and 1
//                            added to face_count
//   Selection (three launches) and compaction (two): the kept vertices and faces flagged from `keep` and the labels,
//   counted per workgroup, scanned, ranked; the vertex row map; the gather.
//
// Integer atomics only: the compare-and-swap on a root, relaxed agent-scope loads and stores of `parent`, integer sums.
// Which trees form in between depends on the race; the partition, and so every output, does not.  No float arithmetic
// (vertices and normals are copied as 32-bit words), no scratch, nothing waits on another thread, and every loop carries
// its bound: a walk that exhausts it, or meets a parent above its vertex, can only mean a corrupted workspace; the thread
// stops and sets MVSN_MESH_STATUS_WORKSPACE in the head.
#include "mvsn_common.h"
#include "mvsn_geom.h"
#include "mvsn_mesh.h"
#include "mvsn_unionfind.h"

namespace mvsn {

constexpr int MS_THREADS = 256;                         // one vertex or one face per thread

// byte offsets of the workspace sections (each 256-byte aligned)
struct MeshLayout {
  size_t head, parent, map, counts, offsets, bytes;
  long vblocks, fblocks;    // workgroups over the vertices and over the faces (at least one: the scan's M' sits there)
};

inline MeshLayout mesh_layout(long m, long f) {
  MeshLayout l;
  l.vblocks = (m + MS_THREADS - 1) / MS_THREADS;
  l.fblocks = f > 0 ? (f + MS_THREADS - 1) / MS_THREADS : 1;
  l.head = 0;
  l.parent = align256(l.head + 2 * sizeof(int64_t));
  l.map = align256(l.parent + sizeof(int) * (size_t)m);
  l.counts = align256(l.map + sizeof(int) * (size_t)m);
  l.offsets = align256(l.counts + sizeof(int) * (size_t)(l.vblocks + l.fblocks));
  l.bytes = align256(l.offsets + sizeof(int64_t) * (size_t)(l.vblocks + l.fblocks));
  return l;
}

inline bool mesh_sizes_ok(long m, long f) { return m > 0 && m <= MESH_MAX_ROWS && f >= 0 && f <= MESH_MAX_ROWS; }

__global__ __launch_bounds__(MS_THREADS) void mesh_init_kernel(int *__restrict__ parent, long m,
                                                               unsigned long long *__restrict__ head) {
  const long v = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  if (v < m) parent[v] = (int)v;
  if (v == 0) head[0] = 0, head[1] = 0;
}

// face_rows narrowed to int; zeros, and false, when a row lies outside [0, m)
__device__ __forceinline__ bool mesh_face(const int64_t *__restrict__ faces, long i, long m, int *r) {
  int64_t v[3];
  const bool ok = face_rows(faces, i, m, v);
  r[0] = ok ? (int)v[0] : 0, r[1] = ok ? (int)v[1] : 0, r[2] = ok ? (int)v[2] : 0;
  return ok;
}

__global__ __launch_bounds__(MS_THREADS) void mesh_hook_kernel(const int64_t *__restrict__ faces, long f, long m,
                                                               int *parent, unsigned long long *head) {
  const long i = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  if (i >= f) return;
  int r[3];
  if (!mesh_face(faces, i, m, r)) return;                           // takes no part: joins nothing
  bool ok = r[0] == r[1] || mesh_unite(parent, r[0], r[1], m);
  ok = ok && (r[1] == r[2] || mesh_unite(parent, r[1], r[2], m));
  if (!ok) atomicOr(head + 1, (unsigned long long)MVSN_MESH_STATUS_WORKSPACE);
}

// No hook runs in this launch, so the roots stand still; the other entries of `parent` are being replaced by roots
// while they are read, and either value is an ancestor.
__global__ __launch_bounds__(MS_THREADS) void mesh_flatten_kernel(int *parent, long m, int *__restrict__ counts,
                                                                  unsigned long long *head) {
  __shared__ int swave[MS_THREADS / 64];
  const long v = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  bool is_root = false;
  if (v < m) {
    int r = (int)v;
    bool found = false;
    for (long step = 0; step <= m; ++step) {                        // strictly downwards: at most m steps
      const int p = mesh_load(parent + r);
      if ((unsigned)p > (unsigned)r) break;
      if (p == r) {
        found = true;
        break;
      }
      r = p;
    }
    if (!found) atomicOr(head + 1, (unsigned long long)MVSN_MESH_STATUS_WORKSPACE);
    else if (r != (int)v) mesh_store(parent + v, r);
    is_root = found && r == (int)v;
  }
  const int roots = block_sum_256(is_root, swave);
  if (threadIdx.x == 0) counts[blockIdx.x] = roots;
}

__global__ __launch_bounds__(MS_THREADS) void mesh_rank_kernel(const int *__restrict__ parent,
                                                               const int64_t *__restrict__ offsets, long m, long c,
                                                               int *__restrict__ id_of, int64_t *__restrict__ first,
                                                               int64_t *__restrict__ vertex_count,
                                                               int64_t *__restrict__ face_count) {
  __shared__ int swave[MS_THREADS / 64];
  const long v = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  const bool is_root[1] = {v < m && (long)parent[min(v, m - 1)] == v};
  const int64_t id = offsets[blockIdx.x] + block_rank(is_root, swave);
  if (!is_root[0]) return;
  id_of[v] = id < c ? (int)id : -1;                                 // (c = the scanned total: always inside)
  if (id < c) first[id] = v, vertex_count[id] = 0, face_count[id] = 0;
}

// the dense id of the component of vertex v, -1 where the workspace holds none for it
__device__ __forceinline__ int mesh_id(const int *__restrict__ parent, const int *__restrict__ id_of, long v, long m,
                                       long c) {
  const int root = parent[v];
  if (root < 0 || root >= m) return -1;
  const int id = id_of[root];
  return id >= 0 && id < c ? id : -1;
}

__global__ __launch_bounds__(MS_THREADS) void mesh_vertex_label_kernel(const int *__restrict__ parent,
                                                                       const int *__restrict__ id_of, long m, long c,
                                                                       int64_t *__restrict__ vertex_label,
                                                                       int64_t *__restrict__ vertex_count) {
  const long v = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  int id = -1;
  if (v < m) {
    id = mesh_id(parent, id_of, v, m, c);
    vertex_label[v] = id;
  }
  mesh_count(vertex_count, id);
}

__global__ __launch_bounds__(MS_THREADS) void mesh_face_label_kernel(const int64_t *__restrict__ faces, long f,
                                                                     const int *__restrict__ parent,
                                                                     const int *__restrict__ id_of, long m, long c,
                                                                     int64_t *__restrict__ face_label,
                                                                     int64_t *__restrict__ face_count) {
  const long i = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  int id = -1;
  if (i < f) {
    int r[3];
    if (mesh_face(faces, i, m, r)) id = mesh_id(parent, id_of, r[0], m, c);
    face_label[i] = id;
  }
  mesh_count(face_count, id);
}

// ---- selection and compaction ----------------------------------------------------------------------------------------
__device__ __forceinline__ bool mesh_kept(const int64_t *__restrict__ label, long i, long n, const uint8_t *__restrict__ keep,
                                          long c) {
  if (i >= n) return false;
  const int64_t id = label[i];
  return id >= 0 && id < c && keep[id] != 0;
}

// workgroups [0, vblocks) count the kept vertices, the ones behind them the kept faces
__global__ __launch_bounds__(MS_THREADS) void mesh_select_count_kernel(const int64_t *__restrict__ vertex_label, long m,
                                                                       const int64_t *__restrict__ face_label, long f,
                                                                       const uint8_t *__restrict__ keep, long c,
                                                                       long vblocks, int *__restrict__ counts) {
  __shared__ int swave[MS_THREADS / 64];
  const bool vertices = (long)blockIdx.x < vblocks;
  const long i = ((long)blockIdx.x - (vertices ? 0 : vblocks)) * MS_THREADS + threadIdx.x;
  const bool kept = vertices ? mesh_kept(vertex_label, i, m, keep, c) : mesh_kept(face_label, i, f, keep, c);
  const int total = block_sum_256(kept, swave);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MS_THREADS) void mesh_select_rank_kernel(const int64_t *__restrict__ vertex_label, long m,
                                                                      const uint8_t *__restrict__ keep, long c,
                                                                      const int64_t *__restrict__ offsets,
                                                                      int *__restrict__ map) {
  __shared__ int swave[MS_THREADS / 64];
  const long v = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  const bool kept[1] = {mesh_kept(vertex_label, v, m, keep, c)};
  const int64_t row = offsets[blockIdx.x] + block_rank(kept, swave);
  if (v < m) map[v] = kept[0] ? (int)row : -1;
}

// vertices and normals travel as 32-bit words: the bits are copied, nothing is computed
__global__ __launch_bounds__(MS_THREADS) void mesh_gather_vertices_kernel(
    const int *__restrict__ map, long m, long m_out, const uint32_t *__restrict__ vertices,
    const uint32_t *__restrict__ normals, const uint8_t *__restrict__ colors, const int64_t *__restrict__ cell,
    uint32_t *__restrict__ out_vertices, uint32_t *__restrict__ out_normals, uint8_t *__restrict__ out_colors,
    int64_t *__restrict__ out_cell, int64_t *__restrict__ vertex_rows) {
  const long v = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  if (v >= m) return;
  const long row = map[v];
  if (row < 0 || row >= m_out) return;                              // dropped (a kept vertex's row is always inside)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    out_vertices[row * 3 + k] = vertices[v * 3 + k];
    out_normals[row * 3 + k] = normals[v * 3 + k];
    if (colors) out_colors[row * 3 + k] = colors[v * 3 + k];
  }
  out_cell[row] = cell[v];
  vertex_rows[row] = v;
}

__global__ __launch_bounds__(MS_THREADS) void mesh_gather_faces_kernel(
    const int64_t *__restrict__ faces, const int64_t *__restrict__ face_label, long f, const uint8_t *__restrict__ keep,
    long c, const int *__restrict__ map, long m, const int64_t *__restrict__ offsets, long vblocks, long f_out,
    int64_t *__restrict__ out_faces, int64_t *__restrict__ face_rows) {
  __shared__ int swave[MS_THREADS / 64];
  const long i = (long)blockIdx.x * MS_THREADS + threadIdx.x;
  const bool kept[1] = {mesh_kept(face_label, i, f, keep, c)};
  // the face counts follow the vertex counts in the scanned array: their prefix starts at the vertex total
  const int64_t row = offsets[vblocks + blockIdx.x] - offsets[vblocks] + block_rank(kept, swave);
  if (!kept[0] || row >= f_out) return;                             // (f_out = the scanned total: a kept face is inside)
  int r[3];
  const bool ok = mesh_face(faces, i, m, r);                        // (a labelled face has its rows inside: always true)
#pragma unroll
  for (int k = 0; k < 3; ++k) out_faces[row * 3 + k] = ok ? (int64_t)map[r[k]] : -1;
  face_rows[row] = i;
}

}  // namespace mvsn

extern "C" size_t mvsn_mesh_workspace_bytes(long n_vertices, long n_faces) {
  if (!mvsn::mesh_sizes_ok(n_vertices, n_faces)) return 0;
  return mvsn::mesh_layout(n_vertices, n_faces).bytes;
}

// the checks the four entries share; `l` is filled when they pass
static int mesh_check(const char *who, long n_vertices, long n_faces, const void *workspace, size_t workspace_bytes,
                      mvsn::MeshLayout *l) {
  using namespace mvsn;
  MVSN_REQUIRE(n_vertices > 0 && n_faces >= 0, MVSN_E_BADARG, "%s: %ld vertices and %ld faces", who, n_vertices, n_faces);
  MVSN_REQUIRE(n_vertices <= MESH_MAX_ROWS && n_faces <= MESH_MAX_ROWS, MVSN_E_TOOLARGE,
               "%s: %ld vertices and %ld faces (at most 2^31 - 1 each)", who, n_vertices, n_faces);
  *l = mesh_layout(n_vertices, n_faces);
  return workspace_check(who, "workspace", workspace, workspace_bytes, l->bytes);
}

extern "C" int mvsn_mesh_components_label(const int64_t *faces, long n_vertices, long n_faces, int64_t *result,
                                          void *workspace, size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(result && (faces || n_faces == 0), MVSN_E_BADARG, "mvsn_mesh_components_label: null pointer");
  MeshLayout l;
  if (int e = mesh_check("mvsn_mesh_components_label", n_vertices, n_faces, workspace, workspace_bytes, &l)) return e;
  char *ws = (char *)workspace;
  unsigned long long *head = (unsigned long long *)(ws + l.head);
  int *parent = (int *)(ws + l.parent), *counts = (int *)(ws + l.counts);
  int64_t *offsets = (int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 vgrid((unsigned)l.vblocks), block(MS_THREADS);
  hipLaunchKernelGGL(mesh_init_kernel, vgrid, block, 0, st, parent, n_vertices, head);
  if (int e = check_launch("mvsn_mesh_components_label: init")) return e;
  if (n_faces > 0) {
    hipLaunchKernelGGL(mesh_hook_kernel, dim3((unsigned)l.fblocks), block, 0, st, faces, n_faces, n_vertices, parent, head);
    if (int e = check_launch("mvsn_mesh_components_label: hook")) return e;
  }
  hipLaunchKernelGGL(mesh_flatten_kernel, vgrid, block, 0, st, parent, n_vertices, counts, head);
  if (int e = check_launch("mvsn_mesh_components_label: flatten")) return e;
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)counts, l.vblocks, offsets,
                     (int64_t *)head);
  if (int e = check_launch("mvsn_mesh_components_label: scan")) return e;
  const hipError_t e = hipMemcpyAsync(result, head, 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
  MVSN_REQUIRE(e == hipSuccess, (int)e, "mvsn_mesh_components_label: copy of the head: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int mvsn_mesh_components_emit(const int64_t *faces, long n_vertices, long n_faces, void *workspace,
                                         size_t workspace_bytes, long n_components, int64_t *vertex_label,
                                         int64_t *face_label, int64_t *vertex_count, int64_t *face_count, int64_t *first,
                                         mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(vertex_label && vertex_count && face_count && first && (n_faces == 0 || (faces && face_label)),
               MVSN_E_BADARG, "mvsn_mesh_components_emit: null pointer");
  MeshLayout l;
  if (int e = mesh_check("mvsn_mesh_components_emit", n_vertices, n_faces, workspace, workspace_bytes, &l)) return e;
  // every vertex belongs to a component and no component is empty: any other count is not this workspace's
  MVSN_REQUIRE(n_components >= 1 && n_components <= n_vertices, MVSN_E_BADARG,
               "mvsn_mesh_components_emit: %ld components of %ld vertices", n_components, n_vertices);
  char *ws = (char *)workspace;
  const int *parent = (const int *)(ws + l.parent);
  int *id_of = (int *)(ws + l.map);
  const int64_t *offsets = (const int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 vgrid((unsigned)l.vblocks), block(MS_THREADS);
  hipLaunchKernelGGL(mesh_rank_kernel, vgrid, block, 0, st, parent, offsets, n_vertices, n_components, id_of, first,
                     vertex_count, face_count);
  if (int e = check_launch("mvsn_mesh_components_emit: rank")) return e;
  hipLaunchKernelGGL(mesh_vertex_label_kernel, vgrid, block, 0, st, parent, (const int *)id_of, n_vertices, n_components,
                     vertex_label, vertex_count);
  if (int e = check_launch("mvsn_mesh_components_emit: vertex labels")) return e;
  if (n_faces > 0) {
    hipLaunchKernelGGL(mesh_face_label_kernel, dim3((unsigned)l.fblocks), block, 0, st, faces, n_faces, parent,
                       (const int *)id_of, n_vertices, n_components, face_label, face_count);
    if (int e = check_launch("mvsn_mesh_components_emit: face labels")) return e;
  }
  return 0;
}

extern "C" int mvsn_mesh_select(const int64_t *vertex_label, const int64_t *face_label, const uint8_t *keep,
                                long n_vertices, long n_faces, long n_components, int64_t *result, void *workspace,
                                size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(vertex_label && keep && result && (face_label || n_faces == 0), MVSN_E_BADARG,
               "mvsn_mesh_select: null pointer");
  MeshLayout l;
  if (int e = mesh_check("mvsn_mesh_select", n_vertices, n_faces, workspace, workspace_bytes, &l)) return e;
  MVSN_REQUIRE(n_components >= 1 && n_components <= n_vertices, MVSN_E_BADARG,
               "mvsn_mesh_select: %ld components of %ld vertices", n_components, n_vertices);
  char *ws = (char *)workspace;
  int *counts = (int *)(ws + l.counts), *map = (int *)(ws + l.map);
  int64_t *offsets = (int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(MS_THREADS);
  hipLaunchKernelGGL(mesh_select_count_kernel, dim3((unsigned)(l.vblocks + l.fblocks)), block, 0, st, vertex_label,
                     n_vertices, face_label, n_faces, keep, n_components, l.vblocks, counts);
  if (int e = check_launch("mvsn_mesh_select: count")) return e;
  // one scan over [vertex counts | face counts]: result[1] = M' + F', and M' = the prefix at the first face count
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)counts,
                     l.vblocks + l.fblocks, offsets, result + 1);
  if (int e = check_launch("mvsn_mesh_select: scan")) return e;
  hipLaunchKernelGGL(mesh_select_rank_kernel, dim3((unsigned)l.vblocks), block, 0, st, vertex_label, n_vertices, keep,
                     n_components, (const int64_t *)offsets, map);
  if (int e = check_launch("mvsn_mesh_select: rank")) return e;
  const hipError_t e = hipMemcpyAsync(result, offsets + l.vblocks, sizeof(int64_t), hipMemcpyDeviceToDevice, st);
  MVSN_REQUIRE(e == hipSuccess, (int)e, "mvsn_mesh_select: copy of the vertex total: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int mvsn_mesh_compact(const float *vertices, const float *normals, const uint8_t *colors, const int64_t *cell,
                                 const int64_t *faces, const int64_t *face_label, const uint8_t *keep, long n_vertices,
                                 long n_faces, long n_components, const void *workspace, size_t workspace_bytes,
                                 long n_vertices_out, long n_faces_out, float *out_vertices, float *out_normals,
                                 uint8_t *out_colors, int64_t *out_cell, int64_t *out_faces, int64_t *vertex_rows,
                                 int64_t *face_rows, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(vertices && normals && cell && keep && (n_faces == 0 || (faces && face_label)), MVSN_E_BADARG,
               "mvsn_mesh_compact: null pointer");
  MeshLayout l;
  if (int e = mesh_check("mvsn_mesh_compact", n_vertices, n_faces, workspace, workspace_bytes, &l)) return e;
  MVSN_REQUIRE(n_components >= 1 && n_components <= n_vertices, MVSN_E_BADARG,
               "mvsn_mesh_compact: %ld components of %ld vertices", n_components, n_vertices);
  MVSN_REQUIRE(n_vertices_out >= 0 && n_vertices_out <= n_vertices && n_faces_out >= 0 && n_faces_out <= n_faces,
               MVSN_E_BADARG, "mvsn_mesh_compact: %ld of %ld vertices and %ld of %ld faces", n_vertices_out, n_vertices,
               n_faces_out, n_faces);
  if (n_vertices_out == 0) return 0;                // nothing kept (a kept face keeps its vertices): nothing to launch
  MVSN_REQUIRE(out_vertices && out_normals && out_cell && vertex_rows && (n_faces_out == 0 || (out_faces && face_rows)),
               MVSN_E_BADARG, "mvsn_mesh_compact: null output");
  MVSN_REQUIRE(!colors == !out_colors, MVSN_E_BADARG, "mvsn_mesh_compact: colours in and out go together");
  const char *ws = (const char *)workspace;
  const int *map = (const int *)(ws + l.map);
  const int64_t *offsets = (const int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(MS_THREADS);
  hipLaunchKernelGGL(mesh_gather_vertices_kernel, dim3((unsigned)l.vblocks), block, 0, st, map, n_vertices,
                     n_vertices_out, (const uint32_t *)vertices, (const uint32_t *)normals, colors, cell,
                     (uint32_t *)out_vertices, (uint32_t *)out_normals, out_colors, out_cell, vertex_rows);
  if (int e = check_launch("mvsn_mesh_compact: vertices")) return e;
  if (n_faces_out > 0) {
    hipLaunchKernelGGL(mesh_gather_faces_kernel, dim3((unsigned)l.fblocks), block, 0, st, faces, face_label, n_faces,
                       keep, n_components, map, n_vertices, offsets, l.vblocks, n_faces_out, out_faces, face_rows);
    if (int e = check_launch("mvsn_mesh_compact: faces")) return e;
  }
  return 0;
}
