// Bootstrap trees from the NNI search's own candidates on the branch-length handle (include/cherrybank.h, cb_bl_bootstrap_best;
// DESIGN.md section 24): every tree the search meets -- the handle's tree and all its NNI neighbours -- is scored under every site
// resample by RELL, and a replicate keeps the best score and the candidate that attains it.  One call, one family of L sites at
// the handle's current indices; l_u, ll'_m[u], d_m[u] = ll'_m[u] - l_u (0 where either is not finite) and the multiplicities
// w_r[u] are those of sup.hip.h (sup_weights_kernel as it is: the same Philox counters, tag and seed, so replicate r here is
// replicate r of cb_bl_supports).  With
//
//     B^r = sum_u w_r[u] l_u   (l_u taken as 0 where it is not finite),      Delta_m^r = sum_u w_r[u] d_m[u]
//
// the candidates of replicate r are, in this order,
//
//     code -2   the incoming best        score as passed in (-inf on the first call)
//     code -1   the tree itself          score B^r
//     code  m   move m of the list       score fl(B^r + Delta_m^r)      (a move whose Delta_m is not finite is left out)
//
// and the result is the largest score and the code of the FIRST candidate that attains it (strict >, in the order above); since
// the codes ascend in that order this is the lowest code among the maxima, which is how the kernels decide a tie -- a maximum
// has no order, so the result does not depend on how moves, replicates or families are tiled, sliced or chunked.
//
//   ufb_gemm_kernel<true>   B^r: the product below with the single row d = l; one workgroup per tile of replicates.
//   ufb_gemm_kernel<false>  the product Delta = D W^T of sup_gemm_kernel -- 16 x 16 x 4 float64 MFMA, k from unit 0 up in steps
//                           of 4 whatever the launch holds, zero operands past the ends (never a read past a buffer), so
//                           Delta_m^r is bitwise cb_bl_supports' delta_rep -- that never writes Delta: a workgroup of four
//                           waves owns UFB_RT = 128 replicates (a wave 32 of them, two accumulators) and a slice of the tiles
//                           of 16 moves (tile s, s + n_slices, ...); after a tile's k loop every thread folds its 2 x 4
//                           scores into the running maximum and lowest-code argmax of its two replicate columns, which stay
//                           in registers over the move tiles; at the end the four row-quads of a wave are folded by shuffles
//                           and lanes 0..15 write part[slice][r].  Slabs of UFB_KT units go through LDS (rows padded to
//                           UFB_LD doubles: the half-wave's ds_read_b64 of 16 rows x 2 k then falls on 32 distinct bank
//                           pairs), the global reads run along the units, d is formed on the way in.
//   ufb_merge_kernel        per replicate: the running best (the incoming one, code -2, on a family's first chunk), the tree's
//                           own B^r (first chunk) and the slices' partial results, by the same rule.
// No atomics; nothing here is shared with sup.hip.h but common.hip.h (sections 16 and 20 of DESIGN.md: shared device functions
// between such kernels have changed the register allocation of the older one before).
#pragma once
#include "common.hip.h"

constexpr int UFB_KT = 32;             // units per LDS slab of the product
constexpr int UFB_LD = UFB_KT + 2;     // doubles per LDS row: 68 dwords, so 16 rows x {k, k + 1} are 32 distinct 8-byte banks
constexpr int UFB_RT = 128;            // replicates per workgroup
constexpr int UFB_NONE = 0x7FFFFFFF;   // the code of "no candidate": above every move's

struct UfbGemmArgs {
  int n_moves, n_rep, n_units;   // moves of the launch, replicates, units
  int move0;                     // the launch's first move within the caller's list: the code of its move 0
  int n_tiles, n_slices;         // tiles of 16 moves of the launch; slices they are dealt to
  const double *out;             // the scan's ll'[move][unit]
  const double *ll;              // l_u [unit]
  const double *W;               // [replicate][unit]
  const double *delta;           // [moves of the launch]: nni_sum_kernel's (not finite: the move is left out)
  double *base;                  // [replicate] B^r: the <true> form writes it, the <false> form reads it
  double *part_score;            // [slice][replicate]
  int *part_code;
};

// the better of two candidates: the larger score, the lower code where the scores are equal
__device__ __forceinline__ void ufb_take(double &s, int &c, double s2, int c2) {
  if (s2 > s || (s2 == s && c2 < c)) {
    s = s2;
    c = c2;
  }
}

// BASE: grid = tiles of UFB_RT replicates; otherwise grid = n_slices x (tiles of UFB_RT replicates), flat; 256 threads
template <bool BASE>
__global__ __launch_bounds__(256) void ufb_gemm_kernel(UfbGemmArgs a, int rep_tiles) {
  __shared__ double sA[16][UFB_LD], sB[UFB_RT][UFB_LD];
  const int slice = BASE ? 0 : blockIdx.x / rep_tiles, rt = blockIdx.x - slice * rep_tiles;
  const int r0 = rt * UFB_RT;
  const int U = a.n_units;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = threadIdx.x & (UFB_KT - 1), row8 = threadIdx.x / UFB_KT;   // 8 rows of a slab per pass
  const int rc[2] = {r0 + 32 * wave + (lane & 15), r0 + 32 * wave + 16 + (lane & 15)};   // this thread's replicate columns
  double b[2] = {0.0, 0.0}, best[2] = {-INFINITY, -INFINITY};
  int code[2] = {UFB_NONE, UFB_NONE};
  if (!BASE) {
#pragma unroll
    for (int j = 0; j < 2; ++j) b[j] = rc[j] < a.n_rep ? a.base[rc[j]] : 0.0;
  }
  const int n_tiles = BASE ? 1 : a.n_tiles, step = BASE ? 1 : a.n_slices;
  for (int mt = slice; mt < n_tiles; mt += step) {
    const int m0 = mt * 16;
    d4 acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int k0 = 0; k0 < U; k0 += UFB_KT) {
      const int u = k0 + col;
      const bool in_u = u < U;
      const double l = in_u ? a.ll[u] : 0.0;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int i = row8 + 8 * p, m = m0 + i;
        double d = 0.0;
        if (BASE) {
          d = (i == 0 && isfinite(l)) ? l : 0.0;
        } else if (in_u && m < a.n_moves) {
          const double x = a.out[(size_t)m * U + u];
          d = (isfinite(x) && isfinite(l)) ? x - l : 0.0;
        }
        sA[i][col] = d;
      }
#pragma unroll
      for (int p = 0; p < UFB_RT / 8; ++p) {
        const int j = row8 + 8 * p, r = r0 + j;
        sB[j][col] = (in_u && r < a.n_rep) ? a.W[(size_t)r * U + u] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < UFB_KT / 4; ++s) {
        const int k = 4 * s + (lane >> 4);
        const double x = sA[lane & 15][k];
        acc[0] = mfma_f64(x, sB[32 * wave + (lane & 15)][k], acc[0]);
        acc[1] = mfma_f64(x, sB[32 * wave + 16 + (lane & 15)][k], acc[1]);
      }
      __syncthreads();
    }
    if (BASE) {   // row 0 of the tile: register 0 of lanes 0..15
      if (lane < 16) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (rc[j] < a.n_rep) a.base[rc[j]] = acc[j][0];
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = m0 + (lane >> 4) + 4 * q;
        if (m < a.n_moves && isfinite(a.delta[m])) {
#pragma unroll
          for (int j = 0; j < 2; ++j) ufb_take(best[j], code[j], b[j] + acc[j][q], a.move0 + m);
        }
      }
    }
  }
  if (!BASE) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const double s2 = __shfl_xor(best[j], off, 64);
        const int c2 = __shfl_xor(code[j], off, 64);
        ufb_take(best[j], code[j], s2, c2);
      }
      if (lane < 16 && rc[j] < a.n_rep) {
        a.part_score[(size_t)slice * a.n_rep + rc[j]] = best[j];
        a.part_code[(size_t)slice * a.n_rep + rc[j]] = code[j];
      }
    }
  }
}

struct UfbMergeArgs {
  int n_rep, n_slices;
  int first;                  // the family's first chunk: the running best is the incoming one (code -2), and the tree joins
  const double *base;         // [replicate] B^r
  const double *part_score;   // [slice][replicate]
  const int *part_code;
  double *best_score;         // [replicate] in-out
  int *best_code;
};

// grid = replicates / 256, 256 threads
__global__ __launch_bounds__(256) void ufb_merge_kernel(UfbMergeArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n_rep) return;
  double s = a.best_score[r];
  int c = a.first ? -2 : a.best_code[r];
  if (a.first) ufb_take(s, c, a.base[r], -1);
  for (int k = 0; k < a.n_slices; ++k) ufb_take(s, c, a.part_score[(size_t)k * a.n_rep + r], a.part_code[(size_t)k * a.n_rep + r]);
  a.best_score[r] = s;
  a.best_code[r] = c;
}
