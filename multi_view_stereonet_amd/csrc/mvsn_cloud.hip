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
#include "mvsn_common.h"
#include "mvsn_geom.h"
#include "mvsn_voxel.h"

namespace mvsn {

constexpr int CL_THREADS = 256;
constexpr int CL_SLOTS = 4;                             // table slots per thread of the init / count / start kernels
constexpr int CL_BLOCK_SLOTS = CL_THREADS * CL_SLOTS;   // slots per workgroup there
constexpr size_t CL_MIN_SLOTS = CL_BLOCK_SLOTS;

// byte offsets of the workspace sections (each 256-byte aligned)
struct CloudLayout {
  size_t keys, pop, start, cursor, slot, records, counts, offsets, bytes;
  size_t slots;   // power of two >= 2 n (>= n above 2^30 points)
  long blocks;    // workgroups of the count / start kernels
};

inline CloudLayout cloud_layout(long n) {
  CloudLayout l;
  l.slots = hash_table_slots(n, CL_MIN_SLOTS);
  l.blocks = (long)(l.slots / CL_BLOCK_SLOTS);
  l.keys = 0;
  l.pop = align256(l.keys + sizeof(unsigned long long) * l.slots);
  l.start = align256(l.pop + sizeof(int) * l.slots);
  l.cursor = align256(l.start + sizeof(int) * l.slots);
  l.slot = align256(l.cursor + sizeof(int) * l.slots);
  l.records = align256(l.slot + sizeof(int) * (size_t)n);
  l.counts = align256(l.records + 16 * (size_t)n);
  l.offsets = align256(l.counts + sizeof(int) * (size_t)l.blocks);
  l.bytes = align256(l.offsets + sizeof(int64_t) * (size_t)l.blocks);
  return l;
}

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

// The cells of axis t that can hold a target within reach of the query (DESIGN.md section 14 has the proof): from
// floor((t - reach) - e) to floor((t + reach) + e) with e = 2^-19 + |t| 2^-20, every step one fp32 operation, clipped
// to the grid.  reach is 1 cell, and 2 where r2 is so small that the square of a difference is a denormal.
__device__ __forceinline__ void cloud_cell_range(float t, float reach, int *lo, int *hi) {
#pragma clang fp contract(off)
  const float a = fabsf(t) * 0x1p-20f;
  const float e = 0x1p-19f + a;
  const float l = (t - reach) - e, u = (t + reach) + e;
  // (clamped on both sides before the conversion: a query far outside the grid gets an empty range, lo > hi)
  *lo = (int)fminf(fmaxf(floorf(l), -(float)VX_CELL_BIAS), (float)VX_CELL_BIAS);
  *hi = (int)fmaxf(fminf(floorf(u), (float)(VX_CELL_BIAS - 1)), -(float)VX_CELL_BIAS - 1.0f);
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
  const float tx = qx * inv, ty = qy * inv, tz = qz * inv;
  unsigned long long best = ~0ull;
  int count = 0;
  // a query whose t overflows is farther than max_dist from every point that has a cell: nothing to visit
  if (isfinite(qx) && isfinite(qy) && isfinite(qz) && isfinite(tx) && isfinite(ty) && isfinite(tz)) {
    const float reach = r2 < 0x1p-100f ? 2.0f : 1.0f;
    int lo[3], hi[3];
    cloud_cell_range(tx, reach, lo + 0, hi + 0);
    cloud_cell_range(ty, reach, lo + 1, hi + 1);
    cloud_cell_range(tz, reach, lo + 2, hi + 2);
    const size_t mask = slots - 1;
    int c[3];
    for (c[0] = lo[0]; c[0] <= hi[0]; ++c[0])
      for (c[1] = lo[1]; c[1] <= hi[1]; ++c[1])
        for (c[2] = lo[2]; c[2] <= hi[2]; ++c[2]) {
          const unsigned long long key = voxel_key(c);
          size_t h = (size_t)voxel_hash(key) & mask;
          long from = 0, to = 0;
          for (size_t probe = 0; probe < slots; ++probe) {  // bounded: every slot at most once
            const unsigned long long seen = keys[h];
            if (seen == key) {
              from = (long)start[h];
              to = from + (long)pop[h];
              break;
            }
            if (seen == VX_EMPTY) break;
            h = (h + 1) & mask;
          }
          from = max(from, 0L), to = min(to, n);           // (a built table's ranges are inside; any other stays inside too)
          for (long j = from; j < to; ++j) {
            const floatx4 r = records[j];
            const float dx = qx - r[0], dy = qy - r[1], dz = qz - r[2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= r2) {
              ++count;
              const unsigned long long k =
                  ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)__float_as_uint(r[3]);
              best = k < best ? k : best;
            }
          }
        }
  }
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
  const CloudLayout l = cloud_layout(n);
  MVSN_REQUIRE(workspace && workspace_bytes >= l.bytes, MVSN_E_WORKSPACE,
               "mvsn_cloud_index_build: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
  MVSN_REQUIRE(((uintptr_t)workspace & 15) == 0, MVSN_E_BADARG,
               "mvsn_cloud_index_build: workspace not 16-byte aligned");
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
  const CloudLayout l = cloud_layout(n_target);
  MVSN_REQUIRE(workspace && workspace_bytes >= l.bytes, MVSN_E_WORKSPACE,
               "mvsn_cloud_nearest: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
  MVSN_REQUIRE(((uintptr_t)workspace & 15) == 0, MVSN_E_BADARG, "mvsn_cloud_nearest: workspace not 16-byte aligned");
  const char *ws = (const char *)workspace;
  hipLaunchKernelGGL(cloud_nearest_kernel, dim3((unsigned)((nq + CL_THREADS - 1) / CL_THREADS)), dim3(CL_THREADS), 0,
                     (hipStream_t)stream, query, nq, inv_cell, r2, (const unsigned long long *)(ws + l.keys),
                     (const int *)(ws + l.pop), (const int *)(ws + l.start), (const floatx4 *)(ws + l.records), l.slots,
                     n_target, dist2, index, within);
  return check_launch("mvsn_cloud_nearest: nearest");
}
