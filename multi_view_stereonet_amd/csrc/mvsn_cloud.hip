// Fixed-radius nearest neighbour between two unsorted clouds (see include/mvsn_hip.h: mvsn_cloud_*; the semantics and
// the proof that the cells visited are enough are DESIGN.md section 14): for every query point the nearest target point
// within max_dist (squared distance, row) and the number of target points within max_dist.
//
// mvsn_cloud_index_build: a counting sort of the target by grid cell through section 12's hash table, six launches:
//   cloud_init_kernel     every key empty, every population and cursor zero; the status word zeroed
//   cloud_assign_kernel   one thread per target point: cell, key and insert of mvsn_voxel.h (the voxel merge's own
//                         functions, cell size max_dist, origin 0: linear probing with a 64-bit compare-and-swap on
//                         empty keys only), a no-return atomicAdd of 1 to the slot's population; the point's slot goes
//                         to the workspace (-1 = never a neighbour)
//   cloud_count_kernel    1024 consecutive slots per workgroup: the sum of their populations
//   geom_scan_kernel      one workgroup: exclusive prefix of those sums in a fixed order (mvsn_geom.h; no total)
//   cloud_start_kernel    the count kernel's blocking again: the exclusive prefix inside the workgroup -> start[slot]
//   cloud_scatter_kernel  one thread per target point: a returning atomicAdd on its slot's cursor gives its place among
//                         the cell's records; one 16-byte record (x, y, z, row as bits) at start[slot] + place
// mvsn_cloud_nearest: one launch,
//   cloud_nearest_kernel  one thread per query point: for every cell of its range a bounded probe for the cell's key
//                         (stop at the key or at the first empty slot), then a walk over the cell's records with
//                         16-byte loads: d2 in fp32, the count of d2 <= r2, and the minimum of (d2 bits, row) as one
//                         64-bit key; one store of each output
//
// Where a point lands inside its cell's records depends on the order in which the scatter's atomics arrive; no output
// does: the nearest is a minimum over (d2, row) and `within` is a count.  Integer atomics only, no float atomics, no
// sort; every loop is bounded (a probe sequence visits every slot at most once, then sets a status bit and ends) and
// nothing waits on another thread.
#include "mvsn_cloud.h"

namespace mvsn {

// slots is a multiple of CL_BLOCK_SLOTS: every thread owns CL_SLOTS whole slots
__global__ __launch_bounds__(CL_THREADS) void cloud_init_kernel(unsigned long long *__restrict__ keys,
                                                                int *__restrict__ pop, int *__restrict__ cursor,
                                                                unsigned long long *__restrict__ status) {
  const size_t s = ((size_t)blockIdx.x * CL_THREADS + threadIdx.x) * CL_SLOTS;
  ulonglong2 *k = reinterpret_cast<ulonglong2 *>(keys + s);
  k[0] = make_ulonglong2(VX_EMPTY, VX_EMPTY);
  k[1] = make_ulonglong2(VX_EMPTY, VX_EMPTY);
  *reinterpret_cast<int4 *>(pop + s) = make_int4(0, 0, 0, 0);
  *reinterpret_cast<int4 *>(cursor + s) = make_int4(0, 0, 0, 0);
  if (s == 0) status[0] = 0;
}

__global__ __launch_bounds__(CL_THREADS) void cloud_assign_kernel(const float *__restrict__ target, long n, float inv,
                                                                  unsigned long long *__restrict__ keys,
                                                                  int *__restrict__ pop, size_t slots,
                                                                  int *__restrict__ slot,
                                                                  unsigned long long *__restrict__ status) {
  const long i = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= n) return;
  const float *p = target + (size_t)i * 3;
  const float o[3] = {0.0f, 0.0f, 0.0f};
  int c[3];
  unsigned q[3];
  const int state = voxel_cell(p, inv, o, c, q);
  int found = -1;
  if (state == VX_KEPT) {
    found = hash_insert(keys, slots, voxel_key(c));
    if (found >= 0)
      atomicAdd(pop + found, 1);
    else
      atomicOr(status, (unsigned long long)MVSN_CLOUD_STATUS_TABLE);
  } else if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
    // a finite point whose cell lies outside the grid, or whose t overflows: it could be somebody's neighbour and has
    // no cell to be found in, so the call must fail (a non-finite point is never a neighbour: nothing to do)
    atomicOr(status, (unsigned long long)MVSN_CLOUD_STATUS_RANGE);
  }
  slot[i] = found;
}

__global__ __launch_bounds__(CL_THREADS) void cloud_count_kernel(const int *__restrict__ pop,
                                                                 int *__restrict__ block_counts) {
  __shared__ int swave[CL_THREADS / 64];
  const size_t s = ((size_t)blockIdx.x * CL_THREADS + threadIdx.x) * CL_SLOTS;
  const int4 w = *reinterpret_cast<const int4 *>(pop + s);
  const int sum = block_sum_256((w.x + w.y) + (w.z + w.w), swave);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = sum;
}

__global__ __launch_bounds__(CL_THREADS) void cloud_start_kernel(const int *__restrict__ pop,
                                                                 const int64_t *__restrict__ offsets,
                                                                 int *__restrict__ start) {
  __shared__ int swave[CL_THREADS / 64];
  const size_t s = ((size_t)blockIdx.x * CL_THREADS + threadIdx.x) * CL_SLOTS;
  const int4 w = *reinterpret_cast<const int4 *>(pop + s);
  const int own = (w.x + w.y) + (w.z + w.w);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = own;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) swave[wave] = incl;
  __syncthreads();
  int base = (int)offsets[blockIdx.x] + incl - own;       // (a start is below n <= 2^31 - 1)
  for (int k = 0; k < wave; ++k) base += swave[k];
  *reinterpret_cast<int4 *>(start + s) = make_int4(base, base + w.x, base + w.x + w.y, base + w.x + w.y + w.z);
}

__global__ __launch_bounds__(CL_THREADS) void cloud_scatter_kernel(const float *__restrict__ target, long n,
                                                                   const int *__restrict__ slot,
                                                                   const int *__restrict__ start,
                                                                   int *__restrict__ cursor,
                                                                   floatx4 *__restrict__ records) {
  const long i = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  if (s < 0) return;
  const long at = (long)start[s] + (long)atomicAdd(cursor + s, 1);
  if (at < 0 || at >= n) return;                            // (the populations sum to at most n: always inside)
  const float *p = target + (size_t)i * 3;
  floatx4 r;
  r[0] = p[0], r[1] = p[1], r[2] = p[2], r[3] = __int_as_float((int)i);
  records[at] = r;
}

__global__ __launch_bounds__(CL_THREADS) void cloud_nearest_kernel(const float *__restrict__ query, long nq, float inv,
                                                                   float r2,
                                                                   const unsigned long long *__restrict__ keys,
                                                                   const int *__restrict__ pop,
                                                                   const int *__restrict__ start,
                                                                   const floatx4 *__restrict__ records, size_t slots,
                                                                   long n, float *__restrict__ dist2,
                                                                   int64_t *__restrict__ index,
                                                                   int *__restrict__ within) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= nq) return;
  const float qx = query[(size_t)i * 3], qy = query[(size_t)i * 3 + 1], qz = query[(size_t)i * 3 + 2];
  const CloudIndex ix = {keys, pop, start, slots};
  int count = 0;
  unsigned long long best = ~0ull;
  cloud_walk(qx, qy, qz, inv, r2, ix, records, n, best, count);
  const bool any = best != ~0ull;
  dist2[i] = any ? __uint_as_float((unsigned)(best >> 32)) : __builtin_inff();
  index[i] = any ? (int64_t)(unsigned)(best & 0xffffffffull) : (int64_t)-1;
  within[i] = count;
}

}  // namespace mvsn

extern "C" size_t mvsn_cloud_workspace_bytes(long n_target) {
  if (n_target <= 0 || n_target > 0x7fffffffL) return 0;
  return mvsn::cloud_layout(n_target).bytes;
}

extern "C" int mvsn_cloud_index_build(const float *target, long n, float cell, float inv_cell, int64_t *status,
                                      void *workspace, size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(target && status, MVSN_E_BADARG, "mvsn_cloud_index_build: null pointer");
  MVSN_REQUIRE(n > 0, MVSN_E_BADARG, "mvsn_cloud_index_build: %ld points", n);
  MVSN_REQUIRE(n <= 0x7fffffffL, MVSN_E_TOOLARGE, "mvsn_cloud_index_build: %ld points (at most 2^31 - 1)", n);
  MVSN_REQUIRE(cell > 0.0f && cell <= 3.0e38f && inv_cell > 0.0f && inv_cell <= 3.0e38f, MVSN_E_BADARG,
               "mvsn_cloud_index_build: cell size %g (inverse %g) is not a positive finite number", (double)cell,
               (double)inv_cell);
  CloudLayout l;
  if (int e = cloud_index_check("mvsn_cloud_index_build", "workspace", workspace, workspace_bytes, n, &l)) return e;
  char *ws = (char *)workspace;
  unsigned long long *keys = (unsigned long long *)(ws + l.keys), *st_word = (unsigned long long *)status;
  int *pop = (int *)(ws + l.pop), *start = (int *)(ws + l.start), *cursor = (int *)(ws + l.cursor);
  int *slot = (int *)(ws + l.slot), *counts = (int *)(ws + l.counts);
  floatx4 *records = (floatx4 *)(ws + l.records);
  int64_t *offsets = (int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  const unsigned point_blocks = (unsigned)((n + CL_THREADS - 1) / CL_THREADS);
  hipLaunchKernelGGL(cloud_init_kernel, dim3((unsigned)l.blocks), dim3(CL_THREADS), 0, st, keys, pop, cursor, st_word);
  if (int e = check_launch("mvsn_cloud_index_build: table init")) return e;
  hipLaunchKernelGGL(cloud_assign_kernel, dim3(point_blocks), dim3(CL_THREADS), 0, st, target, n, inv_cell, keys, pop,
                     l.slots, slot, st_word);
  if (int e = check_launch("mvsn_cloud_index_build: assign")) return e;
  hipLaunchKernelGGL(cloud_count_kernel, dim3((unsigned)l.blocks), dim3(CL_THREADS), 0, st, pop, counts);
  if (int e = check_launch("mvsn_cloud_index_build: count")) return e;
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)counts, l.blocks, offsets,
                     (int64_t *)nullptr);
  if (int e = check_launch("mvsn_cloud_index_build: scan")) return e;
  hipLaunchKernelGGL(cloud_start_kernel, dim3((unsigned)l.blocks), dim3(CL_THREADS), 0, st, pop, offsets, start);
  if (int e = check_launch("mvsn_cloud_index_build: start")) return e;
  hipLaunchKernelGGL(cloud_scatter_kernel, dim3(point_blocks), dim3(CL_THREADS), 0, st, target, n, slot, start, cursor,
                     records);
  return check_launch("mvsn_cloud_index_build: scatter");
}

extern "C" int mvsn_cloud_nearest(const float *query, long nq, float inv_cell, float r2, const void *workspace,
                                  size_t workspace_bytes, long n_target, float *dist2, int64_t *index, int *within,
                                  mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(query && dist2 && index && within, MVSN_E_BADARG, "mvsn_cloud_nearest: null pointer");
  MVSN_REQUIRE(nq > 0 && n_target > 0, MVSN_E_BADARG, "mvsn_cloud_nearest: %ld queries against %ld points", nq,
               n_target);
  MVSN_REQUIRE(nq <= 0x7fffffffL && n_target <= 0x7fffffffL, MVSN_E_TOOLARGE,
               "mvsn_cloud_nearest: %ld queries against %ld points (at most 2^31 - 1 each)", nq, n_target);
  MVSN_REQUIRE(inv_cell > 0.0f && inv_cell <= 3.0e38f && r2 > 0.0f && r2 <= 3.0e38f, MVSN_E_BADARG,
               "mvsn_cloud_nearest: inverse cell size %g or squared radius %g is not a positive finite number",
               (double)inv_cell, (double)r2);
  CloudLayout l;
  if (int e = cloud_index_check("mvsn_cloud_nearest", "workspace", workspace, workspace_bytes, n_target, &l)) return e;
  const floatx4 *records;
  const CloudIndex ix = cloud_index(workspace, l, &records);
  hipLaunchKernelGGL(cloud_nearest_kernel, dim3((unsigned)((nq + CL_THREADS - 1) / CL_THREADS)), dim3(CL_THREADS), 0,
                     (hipStream_t)stream, query, nq, inv_cell, r2, ix.keys, ix.pop, ix.start, records, ix.slots, n_target,
                     dist2, index, within);
  return check_launch("mvsn_cloud_nearest: nearest");
}
