// What the LDS-resident kernels share (internal): the F(2x2,3x3) layer of the chain forms (mvsn_chain_wino.hip,
// mvsn_chain_slab.hip, mvsn_chain_band.hip) and of the towers (mvsn_tower.hip), the half-wave sums of their GroupNorms,
// the LDS-only barrier, the poll loop of the band hand-offs, and the small names around them.  The chain forms are
// required to agree bit for bit (tests/test_hip_parity.py): they agree because they run THIS text.
#pragma once
#include "mvsn_common.h"

namespace mvsn {

constexpr float MVSN_GN_EPS = 1e-5f;   // GroupNorm's eps (torch's default)

#define MVSN_GPTR(p) ((const __attribute__((address_space(1))) void *)(p))
#define MVSN_LPTR(p) ((__attribute__((address_space(3))) void *)(p))
#define MVSN_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// hand-off granules {value, tag} and the vectors they travel in
typedef unsigned long long u64;
typedef __attribute__((address_space(1))) u64 gu64;
typedef __attribute__((address_space(1))) unsigned gu32;
typedef float float2v __attribute__((ext_vector_type(2)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

// Workgroup barrier that publishes LDS writes but leaves global loads / stores in flight (__syncthreads() also waits
// for vmcnt(0): the cost-slice stores and the left-feature loads would be drained at every barrier of the step).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Sums of N values at once over the 32 lanes of each half-wave (lanes 0..31 hold the channels of GroupNorm group
// 2ct, lanes 32..63 of group 2ct+1).  Four DPP steps leave every lane of a 16-lane row with its row's sum;
// row_bcast:15 then adds row 0 into row 1 and row 2 into row 3, so the half-wave sums sit in rows 1 and 3
// (lanes 16..31 / 48..63) -- no LDS crossbar round trip (ds_bpermute) in the chain of dependent steps.
template <int N>
__device__ __forceinline__ void half_wave_sums(float (&s)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] += dpp_mov<0xB1>(s[k]);    // quad_perm [1, 0, 3, 2]
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] += dpp_mov<0x4E>(s[k]);    // quad_perm [2, 3, 0, 1]
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] += dpp_mov<0x141>(s[k]);   // row_half_mirror
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] += dpp_mov<0x140>(s[k]);   // row_mirror
#pragma unroll
  for (int k = 0; k < N; ++k)                                  // row_bcast:15 into rows 1 and 3 (row_mask 0xA)
    s[k] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s[k]), 0x142, 0xA, 0xF, false));
}

// The bounded poll of a band hand-off.  `load(spins)` re-reads this lane's granules and reports whether all their tags
// match; the wave returns once they do in every lane.  After `spin_limit` sweeps it gives up: `dead` is set, `code`
// goes to *status, and every later poll of a dead workgroup returns after one sweep.
template <class Load>
__device__ __forceinline__ void poll_granules(Load load, bool &dead, gu32 *status, unsigned code, unsigned spin_limit) {
  for (unsigned spins = 0;; ++spins) {
    const bool ok = load(spins);
    if (__all(ok) || dead) return;
    if (spins >= spin_limit) {
      dead = true;
      __hip_atomic_store(status, code, MVSN_RLX_AGENT);
      return;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

// ---------------------------------------------------------------------------------------------
// one 3x3 layer: acc[ct][xi] (+)= U_xi * V_xi over NC k-steps of 4 input channels, then the output transform
// ---------------------------------------------------------------------------------------------
// A = U_xi (16 couts x 4 cins), B = V_xi (4 cins x 16 patches) on v_mfma_f32_16x16x4_f32.  Lane (k = lane>>4,
// p = lane&15) holds the 4x4 input window of patch p, channel 4*c4 + k, and computes B^T d B in registers; the 16
// coefficients it ends up with ARE its B-fragment values.  A form supplies where the window and U come from:
//   fetch_d(half, c4, d)   rows (half 0: 0,1,2; half 1: 1,2,3) of this lane's window of k-step c4 -> d[3][4]
//   fetch_u(half, c4, u)   U quads [ct][xq] of transform rows 2*half, 2*half + 1 of k-step c4 -> u[2 * NCT]
// NCT = cout tiles of this wave (y[ct][r][e]: cout ct*16 + (lane>>4)*4 + r, output e = a*2 + b of the patch).
// HSEL = -1: both transform-row halves (y = half 0's outputs + half 1's); 0 / 1: that half alone (y = its outputs; the
// caller adds the two waves' results in the same order, so the sum is bit for bit the one-wave form's).
//
// The 16 xi = (i, j) are walked in two halves by transform row i (i = 0,1 then i = 2,3): 64 accumulator registers
// at a time instead of 128, each half's output transform folded into y as soon as its multiplies are done.  The
// input transform costs the same (row i of B^T d B needs two rows of d), the window reads 3 rows per half.
// Software pipeline per k-step: transform the window that is already in registers, issue the LDS reads of the NEXT
// k-step (3 window rows + 4 quads of U), then the 16 multiplies -- no LDS round trip sits in front of an MFMA.
// Measured (tools/chain_phases.py, s_memtime stamps per wave), 9 k-steps x 2 halves of chain_wino_kernel's first layer:
//   * one wave per SIMD alone: 730 cycles per k-step = 16 MFMAs x 32 + 23 VALU / LDS instructions x ~9.5;
//   * two waves per SIMD (that kernel): 1405 per pair of k-steps -- the two waves leave their barrier together, run
//     their transform sections together and then alternate on the matrix pipe, so the sections ADD instead of
//     hiding under each other (73 % of the pipe); a raised priority for one wave of each pair starves the other
//     instead (same total);
//   * the next k-step's transform interleaved instruction by instruction with the multiplies (sched_group_barrier,
//     MFMA / VALU alternating): 834 cycles per k-step for a wave alone, 7 % slower for the pair -- a VALU
//     instruction between two fp32 MFMAs costs more than its slot.
// The in-register transform costs one VALU per MFMA at 32 output channels; that ratio, not the schedule, is the limit.
template <int NC, int NCT, int HSEL = -1, class FetchD, class FetchU>
__device__ __forceinline__ void f23_resident_layer(FetchD fetch_d, FetchU fetch_u, float (&y)[NCT][4][4]) {
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (HSEL >= 0 && half != HSEL) continue;
    floatx4 acc[NCT][8];
    float d[2][3][4];
    floatx4 u[2][2 * NCT];
    auto fetch = [&](int buf, int c4) {
      fetch_d(half, c4, d[buf]);
      fetch_u(half, c4, u[buf]);
    };
    fetch(0, 0);
#pragma unroll
    for (int c4 = 0; c4 < NC; ++c4) {
      const int cur = c4 & 1;
      // V = B^T d B,  B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]]; rows i = 2*half, 2*half + 1
      float t[2][4], v[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (half == 0) {
          t[0][j] = d[cur][0][j] - d[cur][2][j];   // d0 - d2
          t[1][j] = d[cur][1][j] + d[cur][2][j];   // d1 + d2
        } else {
          t[0][j] = d[cur][1][j] - d[cur][0][j];   // d2 - d1
          t[1][j] = d[cur][0][j] - d[cur][2][j];   // d1 - d3
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        v[i * 4 + 0] = t[i][0] - t[i][2];
        v[i * 4 + 1] = t[i][1] + t[i][2];
        v[i * 4 + 2] = t[i][2] - t[i][1];
        v[i * 4 + 3] = t[i][1] - t[i][3];
      }
      if (c4 + 1 < NC) fetch(cur ^ 1, c4 + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int xq = 0; xq < 2; ++xq)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const floatx4 c0 = c4 == 0 ? floatx4{0.f, 0.f, 0.f, 0.f} : acc[ct][xq * 4 + j];
            acc[ct][xq * 4 + j] = mfma16x16x4(u[cur][ct * 2 + xq][j], v[xq * 4 + j], c0);
          }
      __builtin_amdgcn_sched_barrier(0);
    }
    // Y = A^T m A,  A^T = [[1,1,1,0],[0,1,-1,-1]]: rows m0, m1 (half 0) / m2, m3 (half 1) of m enter
    // s0 = m0 + m1 + m2 and s1 = m1 - m2 - m3; element r of acc[ct][xi] is cout ct*16 + (lane>>4)*4 + r
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s0[4], s1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (half == 0) {
            s0[j] = acc[ct][j][r] + acc[ct][4 + j][r];
            s1[j] = acc[ct][4 + j][r];
          } else {
            s0[j] = acc[ct][j][r];
            s1[j] = -acc[ct][j][r] - acc[ct][4 + j][r];
          }
        }
        const float y0 = s0[0] + s0[1] + s0[2], y1 = s0[1] - s0[2] - s0[3];
        const float y2 = s1[0] + s1[1] + s1[2], y3 = s1[1] - s1[2] - s1[3];
        if (half == 0 || HSEL == 1) y[ct][r][0] = y0, y[ct][r][1] = y1, y[ct][r][2] = y2, y[ct][r][3] = y3;
        else y[ct][r][0] += y0, y[ct][r][1] += y1, y[ct][r][2] += y2, y[ct][r][3] += y3;
      }
    // keep the halves apart: interleaved by the scheduler they hold all 128 accumulators at once, and whatever is
    // live across the layer (moved features, left features) spills
    __builtin_amdgcn_sched_barrier(0);
  }
}

// fetch_d of the forms whose window is four float2 reads from row-major planes with a one-float left halo (data column
// x at index x + 1, so a window starts on an even index): rows wp, wp + RS, wp + 2 RS
__device__ __forceinline__ void window_rows(const float *wp, int RS, float (&d)[3][4]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float2 lo = *reinterpret_cast<const float2 *>(wp + i * RS);
    const float2 hi = *reinterpret_cast<const float2 *>(wp + i * RS + 2);
    d[i][0] = lo.x, d[i][1] = lo.y, d[i][2] = hi.x, d[i][3] = hi.y;
  }
}

}  // namespace mvsn
