// Co-evolution scan kernels (include/cherrybank.h, cb_coscan_*): for EVERY site pair i < j of a family, the log-likelihood of the
// family's counted sequence pairs under the pair model P2[q] = expm(grid[q] Q_2) and under the product of two single-site models
// P1[q] = expm(grid[q] Q_1), over exactly the terms cb_count_co_transitions adds for the contact list {(i, j)} (counting.hip.h,
// count_co_transitions_kernel): s = x_i S + x_j, e = y_i S + y_j, s', e' site-swapped; (s,e), (s',e') and, when symmetric,
// (e,s), (e',s'); a sequence pair with a negative code at any of the four residues contributes nothing to (i, j).
//   coscan_log_kernel  once per bank at creation, in place: an entry that is not positive has log -inf (as bl_log_kernel)
//   coscan_kernel      workgroup = one COSCAN_TILE x COSCAN_TILE tile of the upper triangle of one family's site pairs, thread =
//                      one site pair.  The family's kept sequence pairs are walked in the host's order (by bucket, ties by pair
//                      index) in chunks of CS_CHUNK whose residues for the tile's 2 x 16 sites are staged in LDS; a thread reads
//                      its four residues from there and gathers 4 entries of log P2 and 4 of log P1 per sequence pair (2 + 2
//                      when not symmetric).  Sums are kept in registers, in that one order; both mirror entries are written by
//                      the owning thread, the diagonal (0) by the diagonal tiles.  No atomics: a site pair's bits depend on its
//                      family's sequence pairs alone.  (Bucket order: workgroups meet a bucket's slice of log P2 together;
//                      measured on the 32 demo families, index order costs 5.7 % more kernel time -- EXPERIMENTS 26.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coscan_layout.h"

#define CS_CHUNK 64   // sequence pairs staged per step: 64 x 4 rows x 16 residues = 4 KB of LDS

__global__ __launch_bounds__(256) void coscan_log_kernel(size_t n, double *__restrict__ P) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double p = P[i];
  P[i] = p > 0.0 ? log(p) : -INFINITY;
}

struct CoscanArgs {
  int S;
  double w;                      // 0.25 (symmetric) or 0.5
  const double *logP1, *logP2;   // [B][S][S], [B][S^2][S^2]
  const int8_t *seqs;
  const CoscanFam *fam;
  const CoscanSeqPair *pairs;
  const CoscanTileItem *tiles;
  double *score, *pair_ll, *indep_ll;   // [sum L^2]
  int *n_used;
};

template <bool SYM>
__global__ __launch_bounds__(256) void coscan_kernel(const CoscanArgs a) {
  __shared__ int8_t code[CS_CHUNK][4][COSCAN_TILE];   // rows: x at the tile's i sites, x at its j sites, y at i, y at j
  __shared__ int qs[CS_CHUNK];
  const CoscanTileItem tile = a.tiles[blockIdx.x];
  const CoscanFam F = a.fam[tile.fam];
  const int L = F.L, S = a.S;
  const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
  const int i = tile.ti * COSCAN_TILE + r, j = tile.tj * COSCAN_TILE + c;
  const bool active = i < j && j < L;
  const size_t S2 = (size_t)S * S, SS1 = S2, SS2 = S2 * S2;
  const CoscanSeqPair *sp = a.pairs + (size_t)F.pair_off;
  // staging role of this thread: sequence pair k of the chunk, row `which`
  const int sk = threadIdx.x >> 2, which = threadIdx.x & 3;
  const int s0 = ((which & 1) ? tile.tj : tile.ti) * COSCAN_TILE;
  double acc2 = 0.0, acc1 = 0.0;
  int used = 0;
  for (int p0 = 0; p0 < F.n_kept; p0 += CS_CHUNK) {
    const int n = F.n_kept - p0 < CS_CHUNK ? F.n_kept - p0 : CS_CHUNK;
    __syncthreads();   // the previous chunk has been read
    if (sk < n) {
      const CoscanSeqPair P = sp[p0 + sk];
      const int8_t *row = a.seqs + (size_t)(which < 2 ? P.seq_a : P.seq_b);
      const int left = L - s0;   // sites of this row inside the family
#pragma unroll 4
      for (int u = 0; u < COSCAN_TILE; ++u) code[sk][which][u] = u < left ? row[s0 + u] : (int8_t)-1;
      if (which == 0) qs[sk] = P.q;
    }
    __syncthreads();
    if (!active) continue;
#pragma unroll 4
    for (int k = 0; k < n; ++k) {
      const int xi = code[k][0][r], xj = code[k][1][c], yi = code[k][2][r], yj = code[k][3][c];
      const bool ok = (xi | xj | yi | yj) >= 0;
      // a gapped pair loads entry 0 and adds nothing (a select: the entry may be -inf)
      const size_t ai = ok ? xi : 0, aj = ok ? xj : 0, bi = ok ? yi : 0, bj = ok ? yj : 0;
      const double *P2 = a.logP2 + (size_t)qs[k] * SS2, *P1 = a.logP1 + (size_t)qs[k] * SS1;
      const size_t s = ai * S + aj, sr = aj * S + ai, e = bi * S + bj, er = bj * S + bi;
      double t2 = P2[s * S2 + e] + P2[sr * S2 + er];
      double t1 = P1[ai * S + bi] + P1[aj * S + bj];   // the term (s,e); (s',e') is the same two entries
      if (SYM) {
        t2 += P2[e * S2 + s] + P2[er * S2 + sr];
        t1 += P1[bi * S + ai] + P1[bj * S + aj];
      }
      acc2 += ok ? t2 : 0.0;
      acc1 += ok ? 2.0 * t1 : 0.0;
      used += ok ? 1 : 0;
    }
  }
  const size_t o = (size_t)F.out_off;
  if (active) {
    const double p2 = a.w * acc2, p1 = a.w * acc1, sc = p2 - p1;
    const size_t up = o + (size_t)i * L + j, lo = o + (size_t)j * L + i;
    a.pair_ll[up] = p2;
    a.pair_ll[lo] = p2;
    a.indep_ll[up] = p1;
    a.indep_ll[lo] = p1;
    a.score[up] = sc;
    a.score[lo] = sc;
    a.n_used[up] = used;
    a.n_used[lo] = used;
  } else if (i == j && i < L) {   // (only the diagonal tiles have such threads)
    const size_t d = o + (size_t)i * L + i;
    a.pair_ll[d] = 0.0;
    a.indep_ll[d] = 0.0;
    a.score[d] = 0.0;
    a.n_used[d] = 0;
  }
}
