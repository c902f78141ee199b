// What the geometry kernels share (DESIGN.md sections 10 to 15: mvsn_fusion.hip, mvsn_voxel.hip, mvsn_normals.hip,
// mvsn_cloud.hip, mvsn_tsdf.hip): the workspace alignment, the one-workgroup scan, the sum and the rank inside a
// workgroup of 256 threads, the fp64 3x3 inverse and the gather of map values at (view, pixel).  The hash grid itself
// (cell, key, hash, insert) is mvsn_voxel.h.
// NOT here, on purpose: the 4-wide loads load_pix (zero beyond P), normals_load (clamped address, may start below 0) and
// tsdf_load (the caller decides `wide`) differ in what they do out of range, and in floatx4 against float4
// (mvsn_normals.hip has the note): they stay with their kernels.
#pragma once
#include "mvsn_common.h"

namespace mvsn {

// every section of a workspace starts on a 256-byte boundary
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The two requirements on a workspace of `needed` bytes, `what` its noun in the entry's message ("workspace", "index
// workspace"): MVSN_E_WORKSPACE for a null or short one, MVSN_E_BADARG for one that is not 16-byte aligned.
inline int workspace_check(const char *who, const char *what, const void *workspace, size_t bytes, size_t needed) {
  MVSN_REQUIRE(workspace && bytes >= needed, MVSN_E_WORKSPACE, "%s: %s of %zu bytes, %zu needed", who, what, bytes, needed);
  MVSN_REQUIRE(((uintptr_t)workspace & 15) == 0, MVSN_E_BADARG, "%s: workspace not 16-byte aligned", who);
  return 0;
}

constexpr int GEOM_SCAN_THREADS = 1024;                // the one workgroup of geom_scan_kernel

// Defined in mvsn_voxel.hip; launch with one workgroup of GEOM_SCAN_THREADS threads: the exclusive prefix of n
// per-workgroup counts in index order, and *total = their sum where total is not null.  Every thread owns a run of
// ceil(n / 1024) consecutive counts (the last threads none), the runs are combined by a __shfl_up prefix inside each wave
// and the waves in order: integer sums, so the order does not show.
__global__ __launch_bounds__(GEOM_SCAN_THREADS) void geom_scan_kernel(const int *__restrict__ counts, long n,
                                                                      int64_t *__restrict__ offsets,
                                                                      int64_t *__restrict__ total);

// the sum of `mine` over a workgroup of 256 threads, in every thread; swave: 4 ints of LDS.  Holds a barrier.
__device__ __forceinline__ int block_sum_256(int mine, int *swave) {
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if ((threadIdx.x & 63) == 0) swave[threadIdx.x >> 6] = mine;
  __syncthreads();
  return (swave[0] + swave[1]) + (swave[2] + swave[3]);
}

__device__ __forceinline__ int lanes_below(unsigned long long ballot) {   // set bits of the lanes below this one
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0));
}

// The number of set flags in the workgroup's threads below this one, which is the rank of this thread's first set flag
// when the items are ordered by thread, then by flag slot: the lanes below this one (one ballot per flag slot, mbcnt),
// then the waves below this one.  The wave totals stay in swave (one int per wave).  Holds a barrier, which also
// publishes what the caller wrote to LDS before the call.
template <int N>
__device__ __forceinline__ int block_rank(const bool (&flag)[N], int *swave) {
  int below = 0, wave_total = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const unsigned long long ballot = __ballot(flag[k]);
    below += lanes_below(ballot);
    wave_total += __popcll(ballot);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) swave[wave] = wave_total;
  __syncthreads();
  for (int w = 0; w < wave; ++w) below += swave[w];
  return below;
}

// The inverse of the top-left 3x3 of a row-major 4x4 in fp64, every step one correctly rounded operation: contraction
// is off inside, whatever the file that includes it is compiled with.
__device__ __forceinline__ void inv3_d(const float *K, double *o) {
#pragma clang fp contract(off)
  const double a = K[0], b = K[1], c = K[2], d = K[4], e = K[5], f = K[6], g = K[8], h = K[9], i = K[10];
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const double det = a * A + b * B + c * C, r = 1.0 / det;
  o[0] = A * r, o[1] = -(b * i - c * h) * r, o[2] = (b * f - c * e) * r;
  o[3] = B * r, o[4] = (a * i - c * g) * r, o[5] = -(a * f - c * d) * r;
  o[6] = C * r, o[7] = -(a * h - b * g) * r, o[8] = (a * e - b * d) * r;
}

// out[i, c] = maps[view[i], c, pixel[i]] for maps of C planes of HW values per view; an index outside the maps is never
// dereferenced (NaN).  mvsn_fusion_gather is C = 1, mvsn_normals_gather C = 3.
template <int C>
__global__ __launch_bounds__(256) void gather_kernel(const float *__restrict__ maps, const int *__restrict__ view,
                                                     const int *__restrict__ pixel, int V, long HW, long count,
                                                     float *__restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int v = view[i], q = pixel[i];
  float val[C];
#pragma unroll
  for (int c = 0; c < C; ++c) val[c] = NAN;
  if (v >= 0 && v < V && q >= 0 && q < HW) {
    const float *src = maps + (size_t)v * C * HW + q;
#pragma unroll
    for (int c = 0; c < C; ++c) val[c] = src[c * HW];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[i * C + c] = val[c];
}

}  // namespace mvsn
