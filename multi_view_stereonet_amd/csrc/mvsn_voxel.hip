// Voxel-grid merge of a point cloud (see include/mvsn_hip.h: mvsn_voxel_*; the semantics are DESIGN.md section 12): the
// points that fall into one cell of a regular grid become one point, the mean of their positions and colours, with the
// provenance (lowest input index, output row of every input point) kept.
//
// Seven launches, one host read between the fourth and the fifth:
//   voxel_init_kernel        the hash table: every key empty, every representative INT_MAX; the result words zeroed
//   voxel_assign_kernel      one thread per point: cell and 63-bit key in fp32, linear probing of the open-addressed
//                            table (64-bit compare-and-swap on the key), atomicMin of the slot's representative index
//                            with the point's; the point's slot goes to the workspace (-1 = dropped)
//   voxel_count_kernel       VX_PTS consecutive points per thread: a point is the first of its voxel when it is its
//                            slot's representative; one count per workgroup
//   geom_scan_kernel         one workgroup: exclusive prefix of those counts in a fixed order, and the total M (the scan
//                            of mvsn_geom.h, defined here; the fusion, the cloud index and the TSDF launch it too)
//   voxel_rank_kernel        the count kernel's blocking again: first points ranked inside the workgroup (block_rank of
//                            mvsn_geom.h); they write their slot's output row, first[row], and the
//                            row's accumulators (zeros and the voxel's key)
//   voxel_accumulate_kernel  one thread per point: inverse[i] = row of its slot, integer atomicAdd of the 16-bit
//                            in-cell fractions, the colours and 1 into the row's accumulators
//   voxel_finalise_kernel    one thread per row: the means
//
// Why atomics here when mvsn_fusion.hip has none: the fusion's outputs are per pixel, every one written by its own
// thread, while a voxel gathers points from anywhere in the input and the input is not sorted.  Every atomic here is an
// INTEGER one whose result does not depend on arrival order -- a compare-and-swap that only ever replaces the empty key,
// a minimum, sums of integers -- so every output is still a deterministic function of the inputs: which slot a key
// lands in depends on the race, but nothing that leaves this file does (rows are ordered by the voxel's lowest point
// index, sums are exact).  No float atomics, no sort.  Every loop is bounded: a probe sequence visits at most every slot
// once and then gives up with a status bit; nothing waits on another thread.
#include "mvsn_common.h"
#include "mvsn_geom.h"
#include "mvsn_voxel.h"

namespace mvsn {

constexpr int VX_THREADS = 256;
constexpr int VX_PTS = 4;                               // consecutive points per thread in the count / rank kernels
constexpr int VX_BLOCK_PTS = VX_THREADS * VX_PTS;       // points per workgroup there
constexpr int VX_INIT_SLOTS = 4;                        // table slots per thread of the init kernel
constexpr size_t VX_MIN_SLOTS = VX_THREADS * VX_INIT_SLOTS;
constexpr int VX_ROW_WORDS = 8;                         // accumulator row: sum qx qy qz, sum r g b, count, key

// byte offsets of the workspace sections (each 256-byte aligned)
struct VoxelLayout {
  size_t keys, rep, row, slot, counts, offsets, bytes;
  size_t slots;   // power of two >= 2 n (>= n above 2^30 points)
  long blocks;    // workgroups of the count / rank kernels
};

inline VoxelLayout voxel_layout(long n) {
  VoxelLayout l;
  l.slots = hash_table_slots(n, VX_MIN_SLOTS);
  l.blocks = (n + VX_BLOCK_PTS - 1) / VX_BLOCK_PTS;
  l.keys = 0;
  l.rep = align256(l.keys + sizeof(unsigned long long) * l.slots);
  l.row = align256(l.rep + sizeof(int) * l.slots);
  l.slot = align256(l.row + sizeof(int) * l.slots);
  l.counts = align256(l.slot + sizeof(int) * (size_t)n);
  l.offsets = align256(l.counts + sizeof(int) * (size_t)l.blocks);
  l.bytes = align256(l.offsets + sizeof(int64_t) * (size_t)l.blocks);
  return l;
}

// slots is a multiple of VX_THREADS * VX_INIT_SLOTS: every thread owns VX_INIT_SLOTS whole slots
__global__ __launch_bounds__(VX_THREADS) void voxel_init_kernel(unsigned long long *__restrict__ keys,
                                                                int *__restrict__ rep,
                                                                unsigned long long *__restrict__ result) {
  const size_t s = ((size_t)blockIdx.x * VX_THREADS + threadIdx.x) * VX_INIT_SLOTS;
  ulonglong2 *k = reinterpret_cast<ulonglong2 *>(keys + s);
  k[0] = make_ulonglong2(VX_EMPTY, VX_EMPTY);
  k[1] = make_ulonglong2(VX_EMPTY, VX_EMPTY);
  *reinterpret_cast<int4 *>(rep + s) = make_int4(0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff);
  if (s == 0) result[0] = 0, result[1] = 0;
}

__global__ __launch_bounds__(VX_THREADS) void voxel_assign_kernel(const float *__restrict__ points, long n, float inv,
                                                                  float ox, float oy, float oz,
                                                                  unsigned long long *__restrict__ keys,
                                                                  int *__restrict__ rep, size_t slots,
                                                                  int *__restrict__ slot,
                                                                  unsigned long long *__restrict__ result) {
  const long i = (long)blockIdx.x * VX_THREADS + threadIdx.x;
  if (i >= n) return;
  const float o[3] = {ox, oy, oz};
  int c[3];
  unsigned q[3];
  const int state = voxel_cell(points + (size_t)i * 3, inv, o, c, q);
  int found = -1;
  if (state == VX_KEPT) {
    found = hash_insert(keys, slots, voxel_key(c));
    if (found >= 0)
      atomicMin(rep + found, (int)i);
    else
      atomicOr(result + 1, (unsigned long long)MVSN_VOXEL_STATUS_TABLE);
  } else if (state == VX_OUT_OF_RANGE) {
    atomicOr(result + 1, (unsigned long long)MVSN_VOXEL_STATUS_RANGE);
  }
  slot[i] = found;
}

// whether each of the VX_PTS points at i0.. is the first (lowest index) of its voxel
__device__ __forceinline__ void voxel_firsts(const int *__restrict__ slot, const int *__restrict__ rep, long i0, long n,
                                             int *s, bool *first) {
  if (i0 + VX_PTS <= n) {                                  // (the slot section is 256-byte aligned, i0 a multiple of 4)
    const int4 w = *reinterpret_cast<const int4 *>(slot + i0);
    s[0] = w.x, s[1] = w.y, s[2] = w.z, s[3] = w.w;
  } else {
#pragma unroll
    for (int k = 0; k < VX_PTS; ++k) s[k] = i0 + k < n ? slot[i0 + k] : -1;
  }
#pragma unroll
  for (int k = 0; k < VX_PTS; ++k) first[k] = s[k] >= 0 && (long)rep[s[k]] == i0 + k;
}

__global__ __launch_bounds__(VX_THREADS) void voxel_count_kernel(const int *__restrict__ slot,
                                                                 const int *__restrict__ rep, long n,
                                                                 int *__restrict__ block_counts) {
  __shared__ int swave[VX_THREADS / 64];
  const long i0 = ((long)blockIdx.x * VX_THREADS + threadIdx.x) * VX_PTS;
  int s[VX_PTS];
  bool first[VX_PTS];
  voxel_firsts(slot, rep, i0, n, s, first);
  int mine = 0;
#pragma unroll
  for (int k = 0; k < VX_PTS; ++k) mine += first[k];
  mine = block_sum_256(mine, swave);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = mine;
}

// exclusive prefix of n per-workgroup counts, in index order, and their total (declared in mvsn_geom.h)
__global__ __launch_bounds__(GEOM_SCAN_THREADS) void geom_scan_kernel(const int *__restrict__ counts, long n,
                                                                      int64_t *__restrict__ offsets,
                                                                      int64_t *__restrict__ total) {
  __shared__ int64_t swave[GEOM_SCAN_THREADS / 64];
  const long per = (n + GEOM_SCAN_THREADS - 1) / GEOM_SCAN_THREADS;
  const long lo = min((long)threadIdx.x * per, n), hi = min(lo + per, n);
  int64_t own = 0;
  for (long i = lo; i < hi; ++i) own += counts[i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t incl = own;
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) swave[wave] = incl;
  __syncthreads();
  int64_t base = 0;
  for (int w = 0; w < wave; ++w) base += swave[w];
  int64_t run = base + incl - own;
  for (long i = lo; i < hi; ++i) {
    offsets[i] = run;
    run += counts[i];
  }
  if (threadIdx.x == GEOM_SCAN_THREADS - 1 && total) *total = run;
}

__global__ __launch_bounds__(VX_THREADS) void voxel_rank_kernel(const int *__restrict__ slot,
                                                                const int *__restrict__ rep,
                                                                const unsigned long long *__restrict__ keys,
                                                                const int64_t *__restrict__ offsets, long n,
                                                                long capacity, int *__restrict__ row,
                                                                int64_t *__restrict__ first_out,
                                                                unsigned long long *__restrict__ accum) {
  __shared__ int swave[VX_THREADS / 64];
  const long i0 = ((long)blockIdx.x * VX_THREADS + threadIdx.x) * VX_PTS;
  int s[VX_PTS];
  bool first[VX_PTS];
  voxel_firsts(slot, rep, i0, n, s, first);
  // rank among the workgroup's first points, then the points of this thread before each one
  int64_t idx = offsets[blockIdx.x] + block_rank(first, swave);
#pragma unroll
  for (int k = 0; k < VX_PTS; ++k) {
    if (!first[k]) continue;
    if (idx < capacity) {                           // (capacity = the scanned total: always true)
      row[s[k]] = (int)idx;
      first_out[idx] = i0 + k;
      ulonglong2 *a = reinterpret_cast<ulonglong2 *>(accum + (size_t)idx * VX_ROW_WORDS);
      a[0] = make_ulonglong2(0, 0);
      a[1] = make_ulonglong2(0, 0);
      a[2] = make_ulonglong2(0, 0);
      a[3] = make_ulonglong2(0, keys[s[k]]);
    }
    ++idx;
  }
}

__global__ __launch_bounds__(VX_THREADS) void voxel_accumulate_kernel(const float *__restrict__ points,
                                                                      const uint8_t *__restrict__ colors, long n,
                                                                      float inv, float ox, float oy, float oz,
                                                                      const int *__restrict__ slot,
                                                                      const int *__restrict__ row, long capacity,
                                                                      int64_t *__restrict__ inverse,
                                                                      unsigned long long *__restrict__ accum) {
  const long i = (long)blockIdx.x * VX_THREADS + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  const long r = s >= 0 ? (long)row[s] : -1;
  if (r < 0 || r >= capacity) {                     // dropped (a kept point's row is always inside)
    inverse[i] = -1;
    return;
  }
  inverse[i] = r;
  const float o[3] = {ox, oy, oz};
  int c[3];
  unsigned q[3];
  voxel_cell(points + (size_t)i * 3, inv, o, c, q);
  unsigned long long *a = accum + (size_t)r * VX_ROW_WORDS;
  atomicAdd(a + 0, (unsigned long long)q[0]);
  atomicAdd(a + 1, (unsigned long long)q[1]);
  atomicAdd(a + 2, (unsigned long long)q[2]);
  if (colors) {
    const uint8_t *col = colors + (size_t)i * 3;
    atomicAdd(a + 3, (unsigned long long)col[0]);
    atomicAdd(a + 4, (unsigned long long)col[1]);
    atomicAdd(a + 5, (unsigned long long)col[2]);
  }
  atomicAdd(a + 6, 1ull);
}

__global__ __launch_bounds__(VX_THREADS) void voxel_finalise_kernel(const unsigned long long *__restrict__ accum, long m,
                                                                    float voxel_size, float ox, float oy, float oz,
                                                                    float *__restrict__ points,
                                                                    uint8_t *__restrict__ colors,
                                                                    int *__restrict__ count) {
#pragma clang fp contract(off)
  const long r = (long)blockIdx.x * VX_THREADS + threadIdx.x;
  if (r >= m) return;
  const ulonglong2 *a = reinterpret_cast<const ulonglong2 *>(accum + (size_t)r * VX_ROW_WORDS);
  const ulonglong2 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
  const unsigned long long sq[3] = {a0.x, a0.y, a1.x}, sc[3] = {a1.y, a2.x, a2.y};
  const unsigned long long cnt = a3.x, key = a3.y;
  const float o[3] = {ox, oy, oz};
  const double nd = (double)cnt, v = (double)voxel_size;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int cell = (int)((key >> (21 * (2 - k))) & 0x1fffff) - VX_CELL_BIAS;
    // (float)(o + (c + (sum q / n + 0.5) / 65536) * v), every step one correctly rounded fp64 operation: plain
    // operators with contraction off (above), so no fused multiply-add forms (the __d*_rn intrinsics do not prevent one)
    const double frac = ((double)sq[k] / nd + 0.5) / 65536.0;
    const double pos = (double)o[k] + ((double)cell + frac) * v;
    points[(size_t)r * 3 + k] = (float)pos;
    if (colors) colors[(size_t)r * 3 + k] = (uint8_t)((2 * sc[k] + cnt) / (2 * cnt));
  }
  count[r] = (int)cnt;
}

}  // namespace mvsn

extern "C" size_t mvsn_voxel_workspace_bytes(long n) {
  if (n <= 0 || n > 0x7fffffffL) return 0;
  return mvsn::voxel_layout(n).bytes;
}

extern "C" int mvsn_voxel_assign(const float *points, long n, float voxel_size, float inv_voxel_size, float origin_x,
                                 float origin_y, float origin_z, int64_t *result, void *workspace,
                                 size_t workspace_bytes, mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(points && result, MVSN_E_BADARG, "mvsn_voxel_assign: null pointer");
  MVSN_REQUIRE(n > 0, MVSN_E_BADARG, "mvsn_voxel_assign: %ld points", n);
  MVSN_REQUIRE(n <= 0x7fffffffL, MVSN_E_TOOLARGE, "mvsn_voxel_assign: %ld points (at most 2^31 - 1)", n);
  MVSN_REQUIRE(voxel_size > 0.0f && voxel_size <= 3.0e38f && inv_voxel_size > 0.0f && inv_voxel_size <= 3.0e38f,
               MVSN_E_BADARG, "mvsn_voxel_assign: voxel size %g (inverse %g) is not a positive finite number",
               (double)voxel_size, (double)inv_voxel_size);
  MVSN_REQUIRE(fabsf(origin_x) <= 3.0e38f && fabsf(origin_y) <= 3.0e38f && fabsf(origin_z) <= 3.0e38f, MVSN_E_BADARG,
               "mvsn_voxel_assign: origin is not finite");
  const VoxelLayout l = voxel_layout(n);
  MVSN_REQUIRE(workspace && workspace_bytes >= l.bytes, MVSN_E_WORKSPACE,
               "mvsn_voxel_assign: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
  MVSN_REQUIRE(((uintptr_t)workspace & 15) == 0, MVSN_E_BADARG, "mvsn_voxel_assign: workspace not 16-byte aligned");
  char *ws = (char *)workspace;
  unsigned long long *keys = (unsigned long long *)(ws + l.keys), *res = (unsigned long long *)result;
  int *rep = (int *)(ws + l.rep), *slot = (int *)(ws + l.slot), *counts = (int *)(ws + l.counts);
  int64_t *offsets = (int64_t *)(ws + l.offsets);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(voxel_init_kernel, dim3((unsigned)(l.slots / (VX_THREADS * VX_INIT_SLOTS))), dim3(VX_THREADS), 0,
                     st, keys, rep, res);
  if (int e = check_launch("mvsn_voxel_assign: table init")) return e;
  const unsigned point_blocks = (unsigned)((n + VX_THREADS - 1) / VX_THREADS);
  hipLaunchKernelGGL(voxel_assign_kernel, dim3(point_blocks), dim3(VX_THREADS), 0, st, points, n, inv_voxel_size,
                     origin_x, origin_y, origin_z, keys, rep, l.slots, slot, res);
  if (int e = check_launch("mvsn_voxel_assign: assign")) return e;
  hipLaunchKernelGGL(voxel_count_kernel, dim3((unsigned)l.blocks), dim3(VX_THREADS), 0, st, slot, rep, n, counts);
  if (int e = check_launch("mvsn_voxel_assign: count")) return e;
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(GEOM_SCAN_THREADS), 0, st, (const int *)counts, l.blocks, offsets,
                     result);
  return check_launch("mvsn_voxel_assign: scan");
}

extern "C" int mvsn_voxel_merge(const float *points, const uint8_t *colors, long n, float voxel_size,
                                float inv_voxel_size, float origin_x, float origin_y, float origin_z, void *workspace,
                                size_t workspace_bytes, long capacity, void *accumulators, float *out_points,
                                uint8_t *out_colors, int *count, int64_t *first, int64_t *inverse,
                                mvsn_stream_t stream) {
  using namespace mvsn;
  MVSN_REQUIRE(points && workspace, MVSN_E_BADARG, "mvsn_voxel_merge: null pointer");
  MVSN_REQUIRE(n > 0 && capacity >= 0 && capacity <= n, MVSN_E_BADARG, "mvsn_voxel_merge: %ld voxels of %ld points",
               capacity, n);
  MVSN_REQUIRE(n <= 0x7fffffffL, MVSN_E_TOOLARGE, "mvsn_voxel_merge: %ld points (at most 2^31 - 1)", n);
  MVSN_REQUIRE(!colors == !out_colors, MVSN_E_BADARG, "mvsn_voxel_merge: colours in and out go together");
  MVSN_REQUIRE(voxel_size > 0.0f && voxel_size <= 3.0e38f && inv_voxel_size > 0.0f && inv_voxel_size <= 3.0e38f,
               MVSN_E_BADARG, "mvsn_voxel_merge: voxel size %g (inverse %g) is not a positive finite number",
               (double)voxel_size, (double)inv_voxel_size);
  const VoxelLayout l = voxel_layout(n);
  MVSN_REQUIRE(workspace_bytes >= l.bytes, MVSN_E_WORKSPACE, "mvsn_voxel_merge: workspace of %zu bytes, %zu needed",
               workspace_bytes, l.bytes);
  if (capacity == 0) return 0;                      // every point dropped: nothing to launch (inverse is all -1)
  MVSN_REQUIRE(accumulators && out_points && count && first && inverse, MVSN_E_BADARG, "mvsn_voxel_merge: null output");
  MVSN_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)accumulators & 15) == 0, MVSN_E_BADARG,
               "mvsn_voxel_merge: workspace or accumulators not 16-byte aligned");
  char *ws = (char *)workspace;
  const unsigned long long *keys = (const unsigned long long *)(ws + l.keys);
  const int *rep = (const int *)(ws + l.rep), *slot = (const int *)(ws + l.slot);
  int *row = (int *)(ws + l.row);
  const int64_t *offsets = (const int64_t *)(ws + l.offsets);
  unsigned long long *accum = (unsigned long long *)accumulators;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(voxel_rank_kernel, dim3((unsigned)l.blocks), dim3(VX_THREADS), 0, st, slot, rep, keys, offsets, n,
                     capacity, row, first, accum);
  if (int e = check_launch("mvsn_voxel_merge: rank")) return e;
  hipLaunchKernelGGL(voxel_accumulate_kernel, dim3((unsigned)((n + VX_THREADS - 1) / VX_THREADS)), dim3(VX_THREADS), 0,
                     st, points, colors, n, inv_voxel_size, origin_x, origin_y, origin_z, slot, row, capacity, inverse,
                     accum);
  if (int e = check_launch("mvsn_voxel_merge: accumulate")) return e;
  hipLaunchKernelGGL(voxel_finalise_kernel, dim3((unsigned)((capacity + VX_THREADS - 1) / VX_THREADS)),
                     dim3(VX_THREADS), 0, st, accum, capacity, voxel_size, origin_x, origin_y, origin_z, out_points,
                     out_colors, count);
  return check_launch("mvsn_voxel_merge: finalise");
}
