// What the kernels that query a cloud's hash grid share (DESIGN.md section 14 has the semantics and the proof that the
// cells visited are enough; sections 20, 21, 22, 23, 24 and 26 all query through this file): the workspace layout of an
// index, the view of a built one that a kernel takes (CloudIndex) with the check of the workspace it lies in, and the
// query in three layers, each built on the one before:
//   cloud_cells   the cells a query visits: finite test, reach, the range per axis, the probe for every cell's key and
//                 the clamp of its record range; the caller's on_cell gets (cell, the range's lower corner, from, to)
//   cloud_visit   cloud_cells over 16-byte point records: the fp32 differences and d2 <= r2; the caller's visit gets
//                 every accepted record
//   cloud_walk    cloud_visit with the visitor that counts and keeps the minimum of (d2 bits, row)
// mvsn_cloud.hip builds the grid and answers the nearest-neighbour query; the mesh's point-to-face query
// (mvsn_mesh_nearest.hip) runs cloud_cells over its own 4-byte pair records.
#pragma once
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

// What a query needs of a built index.  The records are a separate, typed kernel argument: floatx4 points for a cloud,
// int face rows for the mesh's (cell, face) pairs.
struct CloudIndex {
  const unsigned long long *keys;
  const int *pop, *start;
  size_t slots;
};

// The view of the index in `workspace`, and its records.  Layout is CloudLayout, or any layout with the same sections
// (the mesh's NearestLayout).
template <class Layout, class Record>
inline CloudIndex cloud_index(const void *workspace, const Layout &l, const Record **records) {
  const char *ws = (const char *)workspace;
  *records = (const Record *)(ws + l.records);
  return {(const unsigned long long *)(ws + l.keys), (const int *)(ws + l.pop), (const int *)(ws + l.start), l.slots};
}

// workspace_check (mvsn_geom.h) on the workspace of an index of n points; 0 and the layout in `l`, or the error code.
inline int cloud_index_check(const char *who, const char *what, const void *workspace, size_t workspace_bytes, long n,
                             CloudLayout *l) {
  *l = cloud_layout(n);
  return workspace_check(who, what, workspace, workspace_bytes, l->bytes);
}

// defined in mvsn_cloud.hip, launched by the mesh's pair index too: the table init, the per-workgroup population sums
// and the starts of an index
__global__ __launch_bounds__(CL_THREADS) void cloud_init_kernel(unsigned long long *__restrict__ keys,
                                                                int *__restrict__ pop, int *__restrict__ cursor,
                                                                unsigned long long *__restrict__ status);
__global__ __launch_bounds__(CL_THREADS) void cloud_count_kernel(const int *__restrict__ pop,
                                                                 int *__restrict__ block_counts);
__global__ __launch_bounds__(CL_THREADS) void cloud_start_kernel(const int *__restrict__ pop,
                                                                 const int64_t *__restrict__ offsets,
                                                                 int *__restrict__ start);

// The cells of one query (qx, qy, qz) against a built index: for every cell c of its range a bounded probe for the
// cell's key (stop at the key or at the first empty slot), then on_cell(c, lo, from, to) with lo the range's lower
// corner and [from, to) the cell's records, clamped to [0, limit); a cell without a key gets the empty range.  False
// when the query has no cells at all: it is not finite, or its t overflows.
template <class OnCell>
__device__ __forceinline__ bool cloud_cells(float qx, float qy, float qz, float inv, float r2, const CloudIndex &ix,
                                            long limit, OnCell &&on_cell) {
#pragma clang fp contract(off)
  const float tx = qx * inv, ty = qy * inv, tz = qz * inv;
  // a query whose t overflows is farther than max_dist from everything that has a cell: nothing to visit
  if (!(isfinite(qx) && isfinite(qy) && isfinite(qz) && isfinite(tx) && isfinite(ty) && isfinite(tz))) return false;
  const float reach = r2 < 0x1p-100f ? 2.0f : 1.0f;
  int lo[3], hi[3];
  cloud_cell_range(tx, reach, lo + 0, hi + 0);
  cloud_cell_range(ty, reach, lo + 1, hi + 1);
  cloud_cell_range(tz, reach, lo + 2, hi + 2);
  const size_t mask = ix.slots - 1;
  int c[3];
  for (c[0] = lo[0]; c[0] <= hi[0]; ++c[0])
    for (c[1] = lo[1]; c[1] <= hi[1]; ++c[1])
      for (c[2] = lo[2]; c[2] <= hi[2]; ++c[2]) {
        const unsigned long long key = voxel_key(c);
        size_t h = (size_t)voxel_hash(key) & mask;
        long from = 0, to = 0;
        for (size_t probe = 0; probe < ix.slots; ++probe) {  // bounded: every slot at most once
          const unsigned long long seen = ix.keys[h];
          if (seen == key) {
            from = (long)ix.start[h];
            to = from + (long)ix.pop[h];
            break;
          }
          if (seen == VX_EMPTY) break;
          h = (h + 1) & mask;
        }
        from = max(from, 0L), to = min(to, limit);        // (a built table's ranges are inside; any other stays inside too)
        on_cell(c, lo, from, to);
      }
  return true;
}

// cloud_cells over the n point records of a cloud's index, with 16-byte loads: d2 in fp32, and every record with
// d2 <= r2 handed to visit(dx, dy, dz, d2, record) in walk order (which depends on the order in which the scatter's
// atomics arrived: a visitor must not let its result depend on it).
template <class Visit>
__device__ __forceinline__ void cloud_visit(float qx, float qy, float qz, float inv, float r2, const CloudIndex &ix,
                                            const floatx4 *__restrict__ records, long n, Visit &&visit) {
#pragma clang fp contract(off)
  cloud_cells(qx, qy, qz, inv, r2, ix, n, [&](const int *, const int *, long from, long to) {
    for (long j = from; j < to; ++j) {
      const floatx4 r = records[j];
      const float dx = qx - r[0], dy = qy - r[1], dz = qz - r[2];
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 <= r2) visit(dx, dy, dz, d2, r);
    }
  });
}

// cloud_visit with the count of the accepted records added to `count` and `best` lowered to the minimum of
// (d2 bits, row) as one 64-bit key.  The caller starts them at 0 and ~0 (~0 afterwards: nothing within).
__device__ __forceinline__ void cloud_walk(float qx, float qy, float qz, float inv, float r2, const CloudIndex &ix,
                                           const floatx4 *__restrict__ records, long n, unsigned long long &best,
                                           int &count) {
  cloud_visit(qx, qy, qz, inv, r2, ix, records, n, [&](float, float, float, float d2, const floatx4 &r) {
    ++count;
    const unsigned long long k =
        ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)__float_as_uint(r[3]);
    best = k < best ? k : best;
  });
}

}  // namespace mvsn
