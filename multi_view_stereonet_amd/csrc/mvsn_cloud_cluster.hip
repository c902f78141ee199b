// Density-based clusters of a cloud (DBSCAN), and with min_points = 1 its Euclidean clusters (see include/mvsn_hip.h:
// mvsn_cloud_cluster_*; the semantics and the argument are DESIGN.md section 24).  The neighbours of a point are
// section 14's (mvsn_cloud.h: cloud_walk and cloud_visit on an index that mvsn_cloud_index_build made of the cloud
// itself); the components of the core points are section 18's lock-free union-find (mvsn_unionfind.h), with the core
// rows as nodes and the neighbour pairs as edges.  One thread per point everywhere.
//
//   Labelling, three launches and the scan, one host read (C, status) behind them:
//   cluster_core_kernel     within[i] = the points within the radius of point i, itself included (cloud_walk);
//                           core[i] = finite and within[i] >= min_points; parent[i] = i; the head (C, status) zeroed
//   cluster_hook_kernel     a core row i visits its neighbours (cloud_visit) and unites (i, j) for every core neighbour
//                           of a LOWER row j.  The relation is symmetric bit for bit (fl(a - b) = -fl(b - a), equal
//                           squares, the same order of the sum), so the higher row of every edge sees it: each edge is
//                           handled once.  The thread remembers the root it last reached: a neighbour whose find ends
//                           there is in i's component already and costs no compare-and-swap.  The order of the visit
//                           depends on the order in which the index's scatter arrived; the partition does not
//   cluster_flatten_kernel  a core row's parent becomes its root; the roots (core and parent == self) of the workgroup
//                           counted
//   geom_scan_kernel        mvsn_geom.h's scan over those counts: the total is C
//   Emission, two launches:
//   cluster_rank_kernel     the roots ranked inside the workgroup (block_rank): root -> dense id, first[id] = root, the
//                           two counters of the id zeroed
//   cluster_label_kernel    a core row gets the id of its root; any other row visits its neighbours and takes the id of
//                           the core neighbour with the least (d2 bits, row) key (cloud_walk's tie rule), -1 without one
//                           (a row that is not finite visits nothing); 1 added to count[id], and to core_count[id] for a
//                           core row
//
// `parent` is touched by agent-scope relaxed atomics and the compare-and-swap only while hooks or flattening run; `core`
// and `within` are written in one launch and read in later ones with plain loads.  Integer atomics only, no float
// arithmetic but cloud_visit's d2, no scratch, nothing waits on another thread, and every loop carries its bound: a walk
// that exhausts it can only mean a corrupted workspace; the thread stops and sets MVSN_CLUSTER_STATUS_WORKSPACE.
#include "mvsn_cloud.h"
#include "mvsn_unionfind.h"

namespace mvsn {

constexpr int CC_THREADS = 256;                         // one point per thread
constexpr long CC_MAX = 0x7fffffffL;                    // points: a row is an int32

// byte offsets of the workspace sections (each 256-byte aligned)
struct ClusterLayout {
  size_t head, parent, map, counts, offsets, bytes;
  long blocks;              // workgroups over the points
};

inline ClusterLayout cluster_layout(long n) {
  ClusterLayout l;
  l.blocks = (n + CC_THREADS - 1) / CC_THREADS;
  l.head = 0;
  l.parent = align256(l.head + 2 * sizeof(int64_t));
  l.map = align256(l.parent + sizeof(int) * (size_t)n);
  l.counts = align256(l.map + sizeof(int) * (size_t)n);
  l.offsets = align256(l.counts + sizeof(int) * (size_t)l.blocks);
  l.bytes = align256(l.offsets + sizeof(int64_t) * (size_t)l.blocks);
  return l;
}

__global__ __launch_bounds__(CC_THREADS) void cluster_core_kernel(
    const float *__restrict__ points, long n, float inv, float r2, long min_points,
    const unsigned long long *__restrict__ keys, const int *__restrict__ pop, const int *__restrict__ start,
    const floatx4 *__restrict__ records, size_t slots, int *__restrict__ within, uint8_t *__restrict__ core,
    int *__restrict__ parent, unsigned long long *__restrict__ head) {
  const long i = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i == 0) head[0] = 0, head[1] = 0;
  if (i >= n) return;
  const float qx = points[(size_t)i * 3], qy = points[(size_t)i * 3 + 1], qz = points[(size_t)i * 3 + 2];
  const CloudIndex ix = {keys, pop, start, slots};
  int count = 0;
  unsigned long long best = ~0ull;
  cloud_walk(qx, qy, qz, inv, r2, ix, records, n, best, count);
  const bool finite = isfinite(qx) && isfinite(qy) && isfinite(qz);
  within[i] = count;
  core[i] = finite && (long)count >= min_points ? 1 : 0;
  parent[i] = (int)i;
}

__global__ __launch_bounds__(CC_THREADS) void cluster_hook_kernel(
    const float *__restrict__ points, long n, float inv, float r2,
    const unsigned long long *__restrict__ keys, const int *__restrict__ pop, const int *__restrict__ start,
    const floatx4 *__restrict__ records, size_t slots, const uint8_t *__restrict__ core, int *parent,
    unsigned long long *head) {
  const long i = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i >= n || !core[i]) return;                                   // only core rows are nodes
  const float qx = points[(size_t)i * 3], qy = points[(size_t)i * 3 + 1], qz = points[(size_t)i * 3 + 2];
  const CloudIndex ix = {keys, pop, start, slots};
  int last = -1;                                                    // the root this thread last reached from i
  bool ok = true;
  cloud_visit(qx, qy, qz, inv, r2, ix, records, n,
              [&](float, float, float, float, const floatx4 &r) {
                const long j = (long)__float_as_uint(r[3]);
                if (!ok || j >= i || !core[j]) return;              // the edge belongs to its higher row; j < i <= n - 1
                const int rj = mesh_find(parent, (int)j, n);
                if (rj < 0) {
                  ok = false;
                  return;
                }
                if (rj == last) return;                             // a row of i's component already
                if (!mesh_unite(parent, (int)i, rj, n)) {
                  ok = false;
                  return;
                }
                last = mesh_find(parent, (int)i, n);
                ok = last >= 0;
              });
  if (!ok) atomicOr(head + 1, (unsigned long long)MVSN_CLUSTER_STATUS_WORKSPACE);
}

// No hook runs in this launch, so the roots stand still; the other entries of `parent` are being replaced by roots
// while they are read, and either value is an ancestor.
__global__ __launch_bounds__(CC_THREADS) void cluster_flatten_kernel(int *parent, const uint8_t *__restrict__ core,
                                                                     long n, int *__restrict__ counts,
                                                                     unsigned long long *head) {
  __shared__ int swave[CC_THREADS / 64];
  const long v = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  bool is_root = false;
  if (v < n && core[v]) {
    int r = (int)v;
    bool found = false;
    for (long step = 0; step <= n; ++step) {                        // strictly downwards: at most n steps
      const int p = mesh_load(parent + r);
      if ((unsigned)p > (unsigned)r) break;
      if (p == r) {
        found = true;
        break;
      }
      r = p;
    }
    if (!found) atomicOr(head + 1, (unsigned long long)MVSN_CLUSTER_STATUS_WORKSPACE);
    else if (r != (int)v) mesh_store(parent + v, r);
    is_root = found && r == (int)v;
  }
  const int roots = block_sum_256(is_root, swave);
  if (threadIdx.x == 0) counts[blockIdx.x] = roots;
}

__global__ __launch_bounds__(CC_THREADS) void cluster_rank_kernel(const int *__restrict__ parent,
                                                                  const uint8_t *__restrict__ core,
                                                                  const int64_t *__restrict__ offsets, long n, long c,
                                                                  int *__restrict__ id_of, int64_t *__restrict__ first,
                                                                  int64_t *__restrict__ count,
                                                                  int64_t *__restrict__ core_count) {
  __shared__ int swave[CC_THREADS / 64];
  const long v = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  const long at = min(v, n - 1);
  const bool is_root[1] = {v < n && core[at] != 0 && (long)parent[at] == v};
  const int64_t id = offsets[blockIdx.x] + block_rank(is_root, swave);
  if (!is_root[0]) return;
  id_of[v] = id < c ? (int)id : -1;                                 // (c = the scanned total: always inside)
  if (id < c) first[id] = v, count[id] = 0, core_count[id] = 0;
}

// the dense id of the cluster of core row v, -1 where the workspace holds none for it
__device__ __forceinline__ int cluster_id(const int *__restrict__ parent, const int *__restrict__ id_of, long v, long n,
                                          long c) {
  const int root = parent[v];
  if (root < 0 || root >= n) return -1;
  const int id = id_of[root];
  return id >= 0 && id < c ? id : -1;
}

__global__ __launch_bounds__(CC_THREADS) void cluster_label_kernel(
    const float *__restrict__ points, long n, float inv, float r2,
    const unsigned long long *__restrict__ keys, const int *__restrict__ pop, const int *__restrict__ start,
    const floatx4 *__restrict__ records, size_t slots, const uint8_t *__restrict__ core,
    const int *__restrict__ parent, const int *__restrict__ id_of, long c, int64_t *__restrict__ label,
    int64_t *__restrict__ count, int64_t *__restrict__ core_count) {
  const long i = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  int id = -1;
  bool is_core = false;
  if (i < n) {
    is_core = core[i] != 0;
    long from = is_core ? i : -1;                                   // the core row whose cluster this row joins
    if (!is_core) {
      const float qx = points[(size_t)i * 3], qy = points[(size_t)i * 3 + 1], qz = points[(size_t)i * 3 + 2];
      const CloudIndex ix = {keys, pop, start, slots};
      unsigned long long best = ~0ull;
      // (a row that is not finite visits nothing and stays noise)
      cloud_visit(qx, qy, qz, inv, r2, ix, records, n,
                  [&](float, float, float, float d2, const floatx4 &r) {
                    const unsigned row = __float_as_uint(r[3]);
                    if ((long)row >= n || !core[row]) return;
                    const unsigned long long k =
                        ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)row;
                    best = k < best ? k : best;
                  });
      if (best != ~0ull) from = (long)(best & 0xffffffffull);
    }
    if (from >= 0) id = cluster_id(parent, id_of, from, n, c);
    label[i] = id;
  }
  mesh_count(count, id);
  mesh_count(core_count, is_core ? id : -1);
}

}  // namespace mvsn

extern "C" size_t mvsn_cloud_cluster_workspace_bytes(long n) {
  if (n <= 0 || n > mvsn::CC_MAX) return 0;
  return mvsn::cluster_layout(n).bytes;
}

// the checks the two entries share (n_clusters: 0 where the entry takes none); `l` is filled when they pass
static int cluster_check(const char *who, long n, long n_clusters, float inv_cell, float r2, const void *index_workspace,
                         size_t index_workspace_bytes, const void *workspace, size_t workspace_bytes,
                         mvsn::ClusterLayout *l) {
  using namespace mvsn;
  MVSN_REQUIRE(n > 0, MVSN_E_BADARG, "%s: %ld points", who, n);
  MVSN_REQUIRE(n <= CC_MAX, MVSN_E_TOOLARGE, "%s: %ld points (at most 2^31 - 1)", who, n);
  // no cluster is empty: any other count is not this workspace's
  MVSN_REQUIRE(n_clusters >= 0 && n_clusters <= n, MVSN_E_BADARG, "%s: %ld clusters of %ld points", who, n_clusters, n);
  MVSN_REQUIRE(inv_cell > 0.0f && inv_cell <= 3.0e38f && r2 > 0.0f && r2 <= 3.0e38f, MVSN_E_BADARG,
               "%s: inverse cell size %g or squared radius %g is not a positive finite number", who, (double)inv_cell,
               (double)r2);
  const size_t index_bytes = cloud_layout(n).bytes;
  MVSN_REQUIRE(index_workspace && index_workspace_bytes >= index_bytes, MVSN_E_WORKSPACE,
               "%s: index workspace of %zu bytes, %zu needed", who, index_workspace_bytes, index_bytes);
  *l = cluster_layout(n);
  MVSN_REQUIRE(workspace && workspace_bytes >= l->bytes, MVSN_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who,
               workspace_bytes, l->bytes);
  MVSN_REQUIRE(((uintptr_t)index_workspace & 15) == 0 && ((uintptr_t)workspace & 15) == 0, MVSN_E_BADARG,
               "%s: workspace not 16-byte aligned", who);
  return 0;
}

extern "C" int mvsn_cloud_cluster_label(const float *points, long n, float inv_cell, float r2, long min_points,
                                        const void *index_workspace, size_t index_workspace_bytes, int *within,
                                        uint8_t *core, int64_t *result, void *workspace, size_t workspace_bytes,
                                        mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_cluster_label";
  MVSN_REQUIRE(points && within && core && result, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(min_points >= 1, MVSN_E_BADARG, "%s: min_points = %ld (at least 1)", who, min_points);
  ClusterLayout l;
  if (int e = cluster_check(who, n, 0, inv_cell, r2, index_workspace, index_workspace_bytes, workspace, workspace_bytes,
                            &l))
    return e;
  char *ws = (char *)workspace;
  unsigned long long *head = (unsigned long long *)(ws + l.head);
  int *parent = (int *)(ws + l.parent), *counts = (int *)(ws + l.counts);
  int64_t *offsets = (int64_t *)(ws + l.offsets);
  const floatx4 *records;
  const CloudIndex ix = cloud_index(index_workspace, cloud_layout(n), &records);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)l.blocks), block(CC_THREADS);
  hipLaunchKernelGGL(cluster_core_kernel, grid, block, 0, st, points, n, inv_cell, r2, min_points, ix.keys, ix.pop,
                     ix.start, records, ix.slots, within, core, parent, head);
  if (int e = check_launch("mvsn_cloud_cluster_label: core")) return e;
  hipLaunchKernelGGL(cluster_hook_kernel, grid, block, 0, st, points, n, inv_cell, r2, ix.keys, ix.pop, ix.start,
                     records, ix.slots, (const uint8_t *)core, parent, head);
  if (int e = check_launch("mvsn_cloud_cluster_label: hook")) return e;
  hipLaunchKernelGGL(cluster_flatten_kernel, grid, block, 0, st, parent, (const uint8_t *)core, n, counts, head);
  if (int e = check_launch("mvsn_cloud_cluster_label: flatten")) return e;
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)counts, l.blocks, offsets,
                     (int64_t *)head);
  if (int e = check_launch("mvsn_cloud_cluster_label: scan")) return e;
  const hipError_t e = hipMemcpyAsync(result, head, 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
  MVSN_REQUIRE(e == hipSuccess, (int)e, "%s: copy of the head: %s", who, hipGetErrorString(e));
  return 0;
}

extern "C" int mvsn_cloud_cluster_emit(const float *points, long n, float inv_cell, float r2,
                                       const void *index_workspace, size_t index_workspace_bytes, const uint8_t *core,
                                       void *workspace, size_t workspace_bytes, long n_clusters, int64_t *label,
                                       int64_t *count, int64_t *core_count, int64_t *first, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_cluster_emit";
  MVSN_REQUIRE(points && core && label && (n_clusters == 0 || (count && core_count && first)), MVSN_E_BADARG,
               "%s: null pointer", who);
  ClusterLayout l;
  if (int e = cluster_check(who, n, n_clusters, inv_cell, r2, index_workspace, index_workspace_bytes, workspace,
                            workspace_bytes, &l))
    return e;
  char *ws = (char *)workspace;
  const int *parent = (const int *)(ws + l.parent);
  int *id_of = (int *)(ws + l.map);
  const int64_t *offsets = (const int64_t *)(ws + l.offsets);
  const floatx4 *records;
  const CloudIndex ix = cloud_index(index_workspace, cloud_layout(n), &records);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)l.blocks), block(CC_THREADS);
  if (n_clusters > 0) {
    hipLaunchKernelGGL(cluster_rank_kernel, grid, block, 0, st, parent, core, offsets, n, n_clusters, id_of, first,
                       count, core_count);
    if (int e = check_launch("mvsn_cloud_cluster_emit: rank")) return e;
  }
  // (with no cluster there is no core row: nothing reads id_of, and every label is -1)
  hipLaunchKernelGGL(cluster_label_kernel, grid, block, 0, st, points, n, inv_cell, r2, ix.keys, ix.pop, ix.start,
                     records, ix.slots, core, parent, (const int *)id_of, n_clusters, label, count, core_count);
  return check_launch("mvsn_cloud_cluster_emit: labels");
}
