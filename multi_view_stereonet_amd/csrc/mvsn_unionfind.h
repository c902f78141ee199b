// The lock-free union-find that the kernels labelling connected components share (mvsn_mesh.hip: the vertices of a
// triangle mesh joined by the sides of its faces; mvsn_cloud_cluster.hip: the core points of a cloud joined by the
// neighbour relation) and the per-component count behind their labels.  DESIGN.md section 18 has the termination and the
// visibility argument; a "vertex" below is a node of either graph, and m the number of rows of `parent`.
#pragma once
#include "mvsn_common.h"

namespace mvsn {

// `parent` while other workgroups write it: the L2s of the XCDs are not coherent with each other and a CU's L1 is never
// refreshed, so every access is an agent-scope atomic.  A read may still be stale; a former parent is an ancestor too.
__device__ __forceinline__ int mesh_load(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void mesh_store(int *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of v as this thread sees it, with path halving (v's parent becomes its grandparent: a vertex that has a parent
// is never a root again, so the store cannot undo a hook).  Every step moves to a strictly lower row: at most m steps.
// -1: the bound ran out or a parent lies above its vertex (a corrupted workspace); no row outside [0, v] is ever read.
__device__ __forceinline__ int mesh_find(int *parent, int v, long m) {
  for (long step = 0; step <= m; ++step) {
    const int p = mesh_load(parent + v);
    if ((unsigned)p > (unsigned)v) return -1;
    if (p == v) return v;
    const int g = mesh_load(parent + p);
    if ((unsigned)g > (unsigned)p) return -1;
    if (g == p) return p;
    mesh_store(parent + v, g);
    v = g;
  }
  return -1;
}

// a and b in one component: the higher of their roots hooked under the lower, if they differ.  A compare-and-swap that
// fails returns the parent another thread gave that root, below it: the walk goes on from there, so the higher of the
// two rows in hand falls with every retry, at most m of them; no thread waits for another.  false: see mesh_find.
__device__ __forceinline__ bool mesh_unite(int *parent, int a, int b, long m) {
  int ra = mesh_find(parent, a, m), rb = mesh_find(parent, b, m);
  for (long retry = 0; retry <= m; ++retry) {
    if (ra < 0 || rb < 0) return false;
    if (ra == rb) return true;
    const int hi = max(ra, rb), lo = min(ra, rb);
    const int seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi) return true;
    if ((unsigned)seen > (unsigned)hi) return false;
    ra = mesh_find(parent, seen, m);
    rb = lo;
  }
  return false;
}

// counts[id] += 1 for every lane with id >= 0; every lane of the wave calls.  One component usually holds nearly all of
// the mesh: a wave whose lanes all carry one id issues one add of their number, not 64 adds to one address.
__device__ __forceinline__ void mesh_count(int64_t *__restrict__ counts, int id) {
  const unsigned long long live = __ballot(id >= 0);
  if (live == 0) return;
  const int leader = __ffsll((long long)live) - 1;
  const int lead_id = __shfl(id, leader, 64);
  if (__ballot(id >= 0 && id != lead_id) == 0) {
    if ((int)(threadIdx.x & 63) == leader) atomicAdd((unsigned long long *)counts + lead_id, (unsigned long long)__popcll(live));
  } else if (id >= 0) {
    atomicAdd((unsigned long long *)counts + id, 1ull);
  }
}

}  // namespace mvsn
