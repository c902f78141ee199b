// The hash grid: its cell, key and hash, the sizing of its table and the insert of a key, shared by
// the voxel merge (mvsn_voxel.hip) and the nearest-neighbour index between clouds (mvsn_cloud.hip): both put a point into
// the same cell of the same grid, and into a table of the same kind.
#pragma once
#include "mvsn_common.h"

namespace mvsn {

constexpr unsigned long long VX_EMPTY = ~0ull;          // bit 63 set: no 63-bit key equals it
constexpr int VX_CELL_BIAS = 1 << 20;                   // cells in [-2^20, 2^20) per axis: 21 bits biased
enum { VX_KEPT = 0, VX_DROPPED = 1, VX_OUT_OF_RANGE = 2 };
constexpr size_t VX_MAX_SLOTS = (size_t)1 << 31;        // a slot index is an int32

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

// slots of the open-addressed table for n keys: min_slots doubled until >= 2 n (>= n above 2^30 keys)
inline size_t hash_table_slots(long n, size_t min_slots) {
  size_t slots = min_slots;
  while (slots < 2 * (size_t)n && slots < VX_MAX_SLOTS) slots <<= 1;
  return slots;
}

// The slot of `key` in the table of `slots` (a power of two) keys, claimed if no thread has yet: linear probing from the
// key's hash with a 64-bit compare-and-swap that only ever replaces the empty key.  Bounded: every slot at most once,
// then -1 (the table is full of other keys).  Which slot a key gets depends on the race; that it gets exactly one does not.
__device__ __forceinline__ int hash_insert(unsigned long long *__restrict__ keys, size_t slots, unsigned long long key) {
  const size_t mask = slots - 1;
  size_t h = (size_t)voxel_hash(key) & mask;
  int found = -1;
  for (size_t probe = 0; probe < slots; ++probe) {
    // a key never changes once it is set, so a plain look first saves the compare-and-swap on every occupied slot
    unsigned long long seen = __hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == VX_EMPTY) seen = atomicCAS(keys + h, VX_EMPTY, key);
    if (seen == VX_EMPTY || seen == key) {
      found = (int)h;
      break;
    }
    h = (h + 1) & mask;
  }
  return found;
}

}  // namespace mvsn
