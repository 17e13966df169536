// Local branch supports on the branch-length handle (include/cherrybank.h, cb_bl_supports): aLRT, SH-like
// and RELL supports of the edge above every internal non-root node, by resampling the per-site log-likelihoods the NNI scan
// (nni.hip.h) leaves in its buffer.  With l_u the family's per-site log-likelihood, ll'_m[u] the scan's for move m and
// d_m[u] = ll'_m[u] - l_u (0 where either is not finite), replicate r draws L sites with replacement -- w_r[u] the number of
// times site u was drawn -- and
//
//     C[m][r] = sum_u d_m[u] w_r[u]
//
// is the resampled delta of move m.  The moves with the same v are the group of the edge above v.
//
//   sup_weights_kernel  one workgroup per replicate: draw j takes word j & 3 of philox4x32_10(counter = (j >> 2, r, 0, SUP_TAG),
//                       key = the family's seed) and lands on site (word * L) >> 32 of the caller's order.  The counts are an
//                       integer histogram in LDS over windows of SUP_WINDOW sites (a longer family repeats the draws per
//                       window); W[r][unit] takes them as doubles in DEVICE unit order (inv = the inverse of the family's perm).
//                       Integer LDS adds only: exact, and independent of the order of the draws.
//   sup_gemm_kernel     C = D W^T in 16 x 16 x 4 float64 MFMA tiles: a workgroup of four waves owns 16 moves x 64 replicates, a
//                       wave 16 x 16 of them.  Slabs of SUP_KT units go through LDS so that the global reads of out[m][u], l_u
//                       and W[r][u] run along the units; d is formed on the way in.  k runs from unit 0 up in steps of 4 whatever
//                       the launch holds, rows and columns past the ends are zero operands (never a read past a buffer), no
//                       atomics: C[m][r] does not depend on the other moves, replicates, chunks or families.
//   sup_edge_kernel     one workgroup per group, threads over replicates (C is read along r): the largest resampled delta of the
//                       group and the two largest of {0} and the centred values C[m][r] - delta[m], the two decisions, a ballot
//                       and a popcount per wave, an integer sum over the waves in LDS.  delta is nni_sum_kernel's, as it is.
#pragma once
#include "common.hip.h"
#include "philox.hip.h"   // sup_philox

constexpr int SUP_WINDOW = 16384;        // sites per histogram window (64 KiB of LDS)
constexpr int SUP_KT = 32;               // units per LDS slab of the product
constexpr uint32_t SUP_TAG = 0x53555050u;   // the fourth counter word: this stream is nobody else's

struct SupWeightArgs {
  int n_units;              // L
  uint32_t k0, k1;          // the family's seed, low and high word
  const int *inv;           // [L]: the device position of the caller's site
  double *W;                // [replicates][L], device unit order
};

// grid = replicates, 256 threads
__global__ __launch_bounds__(256) void sup_weights_kernel(SupWeightArgs a) {
  __shared__ int hist[SUP_WINDOW];
  const int L = a.n_units, r = blockIdx.x;
  const int n_quads = (L + 3) >> 2;
  double *row = a.W + (size_t)r * L;
  for (int s0 = 0; s0 < L; s0 += SUP_WINDOW) {
    const int ns = min(SUP_WINDOW, L - s0);
    for (int k = threadIdx.x; k < ns; k += 256) hist[k] = 0;
    __syncthreads();
    for (int q = threadIdx.x; q < n_quads; q += 256) {
      uint32_t x[4];
      sup_philox((uint32_t)q, (uint32_t)r, 0u, SUP_TAG, a.k0, a.k1, x);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int site = (int)(((unsigned long long)x[i] * (unsigned long long)L) >> 32) - s0;
        if (4 * q + i < L && site >= 0 && site < ns) atomicAdd(&hist[site], 1);
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < ns; k += 256) row[a.inv[s0 + k]] = (double)hist[k];
    __syncthreads();
  }
}

struct SupGemmArgs {
  int n_moves, n_rep, n_units;   // moves of the launch, replicates, units
  const double *out;             // the scan's ll'[move][unit]
  const double *ll;              // l_u [unit]
  const double *W;               // [replicate][unit]
  double *C;                     // [move][replicate]
};

// grid = (tiles of 64 replicates) x (tiles of 16 moves), flat; 256 threads
__global__ __launch_bounds__(256) void sup_gemm_kernel(SupGemmArgs a, int rep_tiles) {
  __shared__ double sA[16][SUP_KT + 1], sB[64][SUP_KT + 1];
  const int mt = blockIdx.x / rep_tiles, rt = blockIdx.x - mt * rep_tiles;
  const int m0 = mt * 16, r0 = rt * 64;
  const int U = a.n_units;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = threadIdx.x & (SUP_KT - 1), row8 = threadIdx.x / SUP_KT;   // 8 rows of a slab per pass
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < U; k0 += SUP_KT) {
    const int u = k0 + col;
    const bool in_u = u < U;
    const double l = in_u ? a.ll[u] : 0.0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int i = row8 + 8 * p, m = m0 + i;
      double d = 0.0;
      if (in_u && m < a.n_moves) {
        const double x = a.out[(size_t)m * U + u];
        d = (isfinite(x) && isfinite(l)) ? x - l : 0.0;
      }
      sA[i][col] = d;
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int j = row8 + 8 * p, r = r0 + j;
      sB[j][col] = (in_u && r < a.n_rep) ? a.W[(size_t)r * U + u] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SUP_KT / 4; ++s) {
      const int k = 4 * s + (lane >> 4);
      acc = mfma_f64(sA[lane & 15][k], sB[16 * wave + (lane & 15)][k], acc);
    }
    __syncthreads();
  }
  const int r = r0 + 16 * wave + (lane & 15);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int m = m0 + (lane >> 4) + 4 * q;
    if (m < a.n_moves && r < a.n_rep) a.C[(size_t)m * a.n_rep + r] = acc[q];
  }
}

struct SupEdgeArgs {
  int n_rep, move0;         // move0: the launch's first move within the family
  const int *group_ptr;     // [groups of the launch + 1]: the groups' first moves, within the family
  const double *delta;      // [moves of the launch]: nni_sum_kernel's
  const double *C;          // [moves of the launch][replicate]
  double *alrt;             // [groups of the launch]
  int *sh_count, *rell_count;
};

// grid = groups, 256 threads
__global__ __launch_bounds__(256) void sup_edge_kernel(SupEdgeArgs a) {
  __shared__ int part[2][4];
  const int g = blockIdx.x, mb = a.group_ptr[g] - a.move0, me = a.group_ptr[g + 1] - a.move0;
  const int R = a.n_rep;
  // the best neighbour at the data themselves (a move whose delta is not finite is left out)
  double best = -INFINITY;
  int used = 0;
  for (int m = mb; m < me; ++m) {
    const double dm = a.delta[m];
    if (isfinite(dm)) {
      best = fmax(best, dm);
      ++used;
    }
  }
  if (used == 0) {
    if (threadIdx.x == 0) {
      a.alrt[g] = NAN;
      a.sh_count[g] = -1;
      a.rell_count[g] = -1;
    }
    return;
  }
  int n_sh = 0, n_rell = 0;
  for (int rb = 0; rb < R; rb += 256) {
    const int r = rb + threadIdx.x;
    const bool act = r < R;
    double mx = -INFINITY, top = 0.0, second = -INFINITY;   // c_0 = 0 is in
    for (int m = mb; m < me; ++m) {
      const double dm = a.delta[m];
      if (!isfinite(dm)) continue;
      const double x = act ? a.C[(size_t)m * R + r] : 0.0;
      mx = fmax(mx, x);
      const double c = x - dm;
      if (c > top) {
        second = top;
        top = c;
      } else if (c > second) {
        second = c;
      }
    }
    const unsigned long long b_sh = __ballot(act && -best > top - second);
    const unsigned long long b_rell = __ballot(act && mx <= 0.0);
    n_sh += __popcll(b_sh);
    n_rell += __popcll(b_rell);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = n_sh;
    part[1][threadIdx.x >> 6] = n_rell;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.alrt[g] = -2.0 * best;
    a.sh_count[g] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    a.rell_count[g] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
  }
}
