// The hash grid's cell, key and hash, shared by the voxel merge (mvsn_voxel.hip) and the
// nearest-neighbour index between clouds (mvsn_cloud.hip): both put a point into the same cell of the same grid; and the
// declaration of the merge's scan kernel, which the TSDF extraction (mvsn_tsdf.hip) launches too.
#pragma once
#include "mvsn_common.h"

namespace mvsn {

constexpr unsigned long long VX_EMPTY = ~0ull;          // bit 63 set: no 63-bit key equals it
constexpr int VX_CELL_BIAS = 1 << 20;                   // cells in [-2^20, 2^20) per axis: 21 bits biased
enum { VX_KEPT = 0, VX_DROPPED = 1, VX_OUT_OF_RANGE = 2 };
constexpr int VX_SCAN_THREADS = 1024;                   // the one workgroup of voxel_scan_kernel

// Defined in mvsn_voxel.hip; launch with one workgroup of VX_SCAN_THREADS threads: the exclusive prefix of n
// per-workgroup counts in index order, and result[0] = their total.
__global__ __launch_bounds__(VX_SCAN_THREADS) void voxel_scan_kernel(const int *__restrict__ counts, long n,
                                                                     int64_t *__restrict__ offsets,
                                                                     unsigned long long *__restrict__ result);

// Cell and in-cell fraction of one point, every step a single fp32 operation:
// s = p - o, t = s * inv, c = floor(t), f = t - c, q = min(65535, (uint)(f * 65536)).  Contraction is off for the whole
// function, and the operations are plain operators under that pragma: the __f*_rn intrinsics are inline functions of a
// header compiled with contraction allowed, so with them t - c becomes fma(s, inv, -c), the fraction of the unrounded
// product, and q is off by one for some points.
__device__ __forceinline__ int voxel_cell(const float *__restrict__ p, float inv, const float *o, int *c, unsigned *q) {
#pragma clang fp contract(off)
  bool finite = true, inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float x = p[a];
    const float s = x - o[a];
    const float t = s * inv;
    const float fl = floorf(t);
    const float f = t - fl;
    finite = finite && isfinite(x) && isfinite(t);
    inside = inside && fl >= -(float)VX_CELL_BIAS && fl < (float)VX_CELL_BIAS;
    c[a] = finite && inside ? (int)fl : 0;
    const float g = f * 65536.0f;
    q[a] = finite && inside ? min(65535u, (unsigned)g) : 0u;     // f in [0, 1]: g in [0, 65536], exactly
  }
  return !finite ? VX_DROPPED : inside ? VX_KEPT : VX_OUT_OF_RANGE;
}

__device__ __forceinline__ unsigned long long voxel_key(const int *c) {
  return ((unsigned long long)(unsigned)(c[0] + VX_CELL_BIAS) << 42) |
         ((unsigned long long)(unsigned)(c[1] + VX_CELL_BIAS) << 21) | (unsigned long long)(unsigned)(c[2] + VX_CELL_BIAS);
}

__device__ __forceinline__ unsigned long long voxel_hash(unsigned long long k) {   // splitmix64's finaliser
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

}  // namespace mvsn
