// Neighbour joining on the device (cb_nj.hip): the join loop of phylogeny_estimation/_nj.py:neighbor_joining as three kernels
// per join.  One sequence of launches serves all families of a chunk (the family is blockIdx.y); launch t handles the family's
// m = n - t active slots, computed from the launch argument t and the family's size; a family with m <= 3 has finished and its
// workgroups return at once.  No workgroup waits for another and there are no atomics: the launch boundaries are the only
// ordering between the three kernels.  Every offset into a matrix is a size_t.
//
// The arithmetic is the host's, operation for operation (the translation unit is compiled with -ffp-contract=off); only the
// order of the row sums differs, and it is fixed: one wave per row, lane l adds the columns l, l + 64, ... upwards onto 0.0, then
// the xor butterfly over the offsets 32, 16, 8, 4, 2, 1 (tests/njd_reference.py restates it).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

#include "nj_layout.h"                // NjFamily, NjCand

#define NJ_BLOCK 256                  // threads of every workgroup: four waves
#define NJ_WAVES (NJ_BLOCK / 64)

// the total order (crit, lower rank, higher rank): ranks are distinct, so no two pairs compare equal
__device__ __forceinline__ bool nj_before(const NjCand &x, const NjCand &y) {
  if (x.crit != y.crit) return x.crit < y.crit;
  if (x.ra != y.ra) return x.ra < y.ra;
  return x.rb < y.rb;
}
// what loses against every pair; its slots are valid ones (m > 3)
__device__ __forceinline__ NjCand nj_no_cand() { return NjCand{__builtin_huge_val(), INT_MAX, INT_MAX, 0, 1}; }

__device__ __forceinline__ NjCand nj_wave_min(NjCand c) {
  for (int off = 32; off > 0; off >>= 1) {
    NjCand o;
    o.crit = __shfl_xor(c.crit, off, 64);
    o.ra = __shfl_xor(c.ra, off, 64);
    o.rb = __shfl_xor(c.rb, off, 64);
    o.sa = __shfl_xor(c.sa, off, 64);
    o.sb = __shfl_xor(c.sb, off, 64);
    if (nj_before(o, c)) c = o;
  }
  return c;
}
// the minimum of the workgroup's candidates, valid in thread 0 (lds: NJ_WAVES entries)
__device__ __forceinline__ NjCand nj_block_min(NjCand c, NjCand *lds) {
  c = nj_wave_min(c);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < NJ_WAVES; ++w)
      if (nj_before(lds[w], c)) c = lds[w];
  return c;
}

// candidate workgroups of a family with m active slots: a wave takes the rows w and m - 1 - w of the upper triangle (m - 1
// entries together), a workgroup NJ_WAVES such pairs of rows
__host__ __device__ inline int nj_num_cands(int m) { return ((m + 1) / 2 + NJ_WAVES - 1) / NJ_WAVES; }

// r[i] = sum_k D[i][k] over the m active slots.  grid (ceil(max m / NJ_WAVES), families)
__global__ __launch_bounds__(NJ_BLOCK) void nj_rowsum_kernel(int t, const NjFamily *__restrict__ fams, const double *__restrict__ D,
                                                             double *__restrict__ r) {
  const NjFamily F = fams[blockIdx.y];
  const int m = F.n - t;
  const int row = blockIdx.x * NJ_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m <= 3 || row >= m) return;
  const double *d = D + F.d0 + (size_t)row * (size_t)F.n;
  double s = 0.0;
#pragma unroll 4
  for (int k = lane; k < m; k += 64) s += d[k];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) r[F.v0 + row] = s;
}

// crit_ab = (m - 2) d_ab - (r_a + r_b) over the upper triangle by slot; one candidate per workgroup.
// grid (nj_num_cands(max m), families)
__global__ __launch_bounds__(NJ_BLOCK) void nj_argmin_kernel(int t, const NjFamily *__restrict__ fams, const double *__restrict__ D,
                                                             const double *__restrict__ r, const int *__restrict__ rank,
                                                             NjCand *__restrict__ cand) {
  __shared__ NjCand lds[NJ_WAVES];
  const NjFamily F = fams[blockIdx.y];
  const int m = F.n - t;
  if (m <= 3 || (int)blockIdx.x >= nj_num_cands(m)) return;
  const int w = blockIdx.x * NJ_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const double *rr = r + F.v0;
  const int *rk = rank + F.v0;
  const double scale = (double)(m - 2);
  NjCand best = nj_no_cand();
  if (w < (m + 1) / 2) {
    for (int half = 0; half < 2; ++half) {
      const int a = half == 0 ? w : m - 1 - w;
      if (half == 1 && a == w) break;                  // (m odd: the middle row once)
      const double *d = D + F.d0 + (size_t)a * (size_t)F.n;
      const double ra = rr[a];
      const int ka = rk[a];
      for (int b = a + 1 + lane; b < m; b += 64) {
        const double prod = scale * d[b];
        const double sum = ra + rr[b];
        const int kb = rk[b];
        NjCand c;
        c.crit = prod - sum;
        if (ka < kb) c.ra = ka, c.rb = kb, c.sa = a, c.sb = b;
        else c.ra = kb, c.rb = ka, c.sa = b, c.sb = a;
        if (nj_before(c, best)) best = c;
      }
    }
  }
  best = nj_block_min(best, lds);
  if (threadIdx.x == 0) cand[F.v0 + blockIdx.x] = best;
}

// One workgroup per family: the winner of the candidates, the join record, the new row and column in slot i (the lower rank),
// the last slot's node into slot j; after the family's last join its three remaining nodes and their distances.  grid (families)
__global__ __launch_bounds__(NJ_BLOCK) void nj_join_kernel(int t, const NjFamily *__restrict__ fams, double *__restrict__ D,
                                                           const double *__restrict__ r, double *__restrict__ tmp,
                                                           int *__restrict__ rank, int *__restrict__ node,
                                                           const NjCand *__restrict__ cand, int *__restrict__ join_nodes,
                                                           double *__restrict__ join_len, int *__restrict__ final_nodes,
                                                           double *__restrict__ final_D) {
  __shared__ NjCand lds[NJ_WAVES];
  __shared__ int win[2];
  const NjFamily F = fams[blockIdx.x];
  const int n = F.n, m = n - t, tid = threadIdx.x;
  if (m <= 3) return;
  NjCand best = nj_no_cand();
  for (int c = tid, nc = nj_num_cands(m); c < nc; c += NJ_BLOCK) {
    const NjCand o = cand[F.v0 + c];
    if (nj_before(o, best)) best = o;
  }
  best = nj_block_min(best, lds);
  if (tid == 0) win[0] = best.sa, win[1] = best.sb;
  __syncthreads();
  const int i = win[0], j = win[1];
  double *d = D + F.d0, *tv = tmp + F.v0;
  int *rk = rank + F.v0, *nd = node + F.v0;
  const size_t ld = (size_t)n;
  const double dij = d[(size_t)i * ld + j];
  if (tid == 0) {
    const double ri = r[F.v0 + i], rj = r[F.v0 + j];
    const double li = dij / 2.0 + (ri - rj) / (2.0 * (double)(m - 2));
    const size_t rec = ((size_t)F.join0 + (size_t)t) * 2;
    join_nodes[rec] = nd[i];
    join_nodes[rec + 1] = nd[j];
    join_len[rec] = li;
    join_len[rec + 1] = dij - li;
  }
  // d_uk = ((d_ik + d_jk) - d_ij) / 2, all of it before any of it is written
  for (int k = tid; k < m; k += NJ_BLOCK) tv[k] = ((d[(size_t)i * ld + k] + d[(size_t)j * ld + k]) - dij) / 2.0;
  __syncthreads();
  for (int k = tid; k < m; k += NJ_BLOCK) {
    const double v = k == i ? 0.0 : tv[k];
    d[(size_t)i * ld + k] = v;
    d[(size_t)k * ld + i] = v;
  }
  __syncthreads();
  if (tid == 0) nd[i] = n + t, rk[i] = n + t;
  if (j != m - 1) {                                      // (uniform) the last slot's node moves to slot j
    for (int k = tid; k < m; k += NJ_BLOCK) tv[k] = d[(size_t)(m - 1) * ld + k];
    __syncthreads();
    for (int k = tid; k < m; k += NJ_BLOCK) {
      const double v = k == j ? 0.0 : tv[k];
      d[(size_t)j * ld + k] = v;
      d[(size_t)k * ld + j] = v;
    }
    if (tid == 0) nd[j] = nd[m - 1], rk[j] = rk[m - 1];  // (thread 0 wrote slot i above: i == m - 1 moves the new node)
  }
  if (m != 4) return;
  __syncthreads();
  if (tid == 0) {                                        // the three nodes left, in the order of the active list
    int o[3] = {0, 1, 2};
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2 - a; ++b)
        if (rk[o[b]] > rk[o[b + 1]]) {
          const int x = o[b];
          o[b] = o[b + 1];
          o[b + 1] = x;
        }
    for (int a = 0; a < 3; ++a) {
      final_nodes[(size_t)blockIdx.x * 3 + a] = nd[o[a]];
      for (int b = 0; b < 3; ++b) final_D[(size_t)blockIdx.x * 9 + a * 3 + b] = d[(size_t)o[a] * ld + o[b]];
    }
  }
}
