// Transfer bootstrap on the device (include/cherrybank.h, cb_transfer_support): for every reference leaf set
// A_r and every replicate b the transfer distance to the replicate's closest split,
//
//     delta[r][b] = min( p_r - 1 ,  min_q min(h, n - h) ),   h = |A_r xor S_{b,q}|,
//
// S_{b,q} the leaf set of the node join q of replicate b makes.  All of it is integer work on bitsets: leaf k is bit
// 0x80 >> (k & 7) of byte k >> 3 (np.packbits, the layout of tree_splits), rows padded with zero bytes to whole 64-bit words, so
// a pad bit is 0 on both sides and never counts.
//
//   tb_sets_kernel       one workgroup per replicate builds the rows of its joined nodes in join order, in global memory: the
//                        threads run over the words of the row and OR the two members' rows; a member below n is a one-hot
//                        row that is formed, not stored.  A workgroup barrier separates the joins (join q may read the row of
//                        join q - 1).
//   tb_distance_kernel   a workgroup of four waves owns one replicate and TB_RT reference sets and takes the replicate's n - 3
//                        sets in tiles of TB_ST through LDS, TB_WC words of every row at a time.  Thread (tr, ts) = (tid & 15,
//                        tid >> 4) keeps the sixteen Hamming accumulators of the reference rows tr + 16 i and the sets
//                        ts + 16 j; they carry over the word chunks, and min(h, n - h) is taken after the last chunk only.
//                        The minimum over the sets runs in registers over j and the tiles, then over the four ts of a wave by
//                        shuffles, then over the waves through LDS; thread r of the first wave clamps with p_r - 1 and writes
//                        delta[r][b].  One workgroup writes an entry, there are no atomics, and a minimum of integers has no
//                        order: the result does not depend on the grid.
//
// LDS rows are TB_WC + 1 words long.  The operand read of a 32-lane half is ds_read_b64 of the rows tr = 0 .. 15 at one word
// (the two ts of the half read the same address of the set tile: a broadcast); with 64 four-byte banks a row stride of 16 words
// puts rows tr and tr + 2 on one bank (8-way), a stride of 17 words = 34 banks gives 34 tr mod 64: the even rows on the banks
// 0, 4, .. 28, the odd rows on 34, 38, .. 62 -- sixteen different bank pairs.
#pragma once
#include "common.hip.h"

#include <climits>

constexpr int TB_RT = 64;            // reference sets per workgroup
constexpr int TB_ST = 64;            // replicate sets per LDS tile
constexpr int TB_WC = 16;            // 64-bit words of a row per stage: 1024 leaves
constexpr int TB_LD = TB_WC + 1;     // words per LDS row (above)

// the word and the bit of leaf k in a packed row
__device__ __forceinline__ unsigned long long tb_leaf_bit(int k) { return 1ull << (8 * ((k >> 3) & 7) + 7 - (k & 7)); }

struct TbSetsArgs {
  int n, W;                          // leaves; 64-bit words per row
  const int *join_nodes;             // [replicates of the launch][n - 3][2]
  unsigned long long *sets;          // [replicates of the launch][n - 3][W] out
};

// grid = replicates of the launch, 256 threads
__global__ __launch_bounds__(256) void tb_sets_kernel(TbSetsArgs a) {
  const int n = a.n, W = a.W, joins = n - 3;
  const int *jn = a.join_nodes + (size_t)blockIdx.x * joins * 2;
  unsigned long long *rows = a.sets + (size_t)blockIdx.x * joins * W;
  for (int q = 0; q < joins; ++q) {
    const int u = jn[2 * q], v = jn[2 * q + 1];
    for (int w = threadIdx.x; w < W; w += 256) {
      const unsigned long long x = u < n ? ((u >> 6) == w ? tb_leaf_bit(u) : 0ull) : rows[(size_t)(u - n) * W + w];
      const unsigned long long y = v < n ? ((v >> 6) == w ? tb_leaf_bit(v) : 0ull) : rows[(size_t)(v - n) * W + w];
      rows[(size_t)q * W + w] = x | y;
    }
    __syncthreads();
  }
}

struct TbDistArgs {
  int n, W, n_ref, n_rep, rep0;      // leaves; words per row; reference sets; replicates of the CALL; the launch's first replicate
  const unsigned long long *refs;    // [n_ref][W]
  const int *clamp;                  // [n_ref]: p_r - 1
  const unsigned long long *sets;    // [replicates of the launch][n - 3][W]
  int *min_dist;                     // [n_ref][n_rep] out: column rep0 + blockIdx.y
};

// rows row0 .. of `src` (n_rows rows of W words), words w0 .., into a tile; a row or a word past the end is zero
__device__ __forceinline__ void tb_stage(unsigned long long (*tile)[TB_LD], const unsigned long long *src, int row0, int n_rows,
                                         int w0, int W, int tid) {
#pragma unroll
  for (int k = 0; k < TB_RT * TB_WC / 256; ++k) {
    const int idx = tid + 256 * k, row = idx / TB_WC, w = idx % TB_WC;
    tile[row][w] = (row0 + row < n_rows && w0 + w < W) ? src[(size_t)(row0 + row) * W + (w0 + w)] : 0ull;
  }
}

// grid = (tiles of TB_RT reference sets, replicates of the launch), 256 threads
__global__ __launch_bounds__(256) void tb_distance_kernel(TbDistArgs a) {
  static_assert(TB_RT == TB_ST && TB_RT == 64, "one staging loop and sixteen pairs per thread");
  __shared__ unsigned long long sRef[TB_RT][TB_LD], sSet[TB_ST][TB_LD];
  __shared__ int sMin[4][TB_RT];
  const int n = a.n, W = a.W, n_sets = n - 3;
  const int tid = threadIdx.x, tr = tid & 15, ts = tid >> 4, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * TB_RT;
  const unsigned long long *sets = a.sets + (size_t)blockIdx.y * n_sets * W;
  const bool one_chunk = W <= TB_WC;                                   // the reference tile is staged once
  int best[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
  for (int s0 = 0; s0 < n_sets; s0 += TB_ST) {                         // (uniform: every thread meets every barrier)
    int acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0;
    for (int w0 = 0; w0 < W; w0 += TB_WC) {
      if (!one_chunk || s0 == 0) tb_stage(sRef, a.refs, r0, a.n_ref, w0, W, tid);
      tb_stage(sSet, sets, s0, n_sets, w0, W, tid);
      __syncthreads();
      const int wc = min(TB_WC, W - w0);
      for (int w = 0; w < wc; ++w) {
        unsigned long long x[4], y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = sRef[tr + 16 * i][w], y[i] = sSet[ts + 16 * i][w];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] += __popcll(x[i] ^ y[j]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (s0 + ts + 16 * j < n_sets) {
#pragma unroll
        for (int i = 0; i < 4; ++i) best[i] = min(best[i], min(acc[i][j], n - acc[i][j]));
      }
  }
  // lane = 16 (ts & 3) + tr: the four ts of a wave, then the four waves
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    best[i] = min(best[i], __shfl_xor(best[i], 16));
    best[i] = min(best[i], __shfl_xor(best[i], 32));
    if (lane < 16) sMin[wave][tr + 16 * i] = best[i];
  }
  __syncthreads();
  const int r = r0 + tid;
  if (tid < TB_RT && r < a.n_ref) {
    const int m = min(min(sMin[0][tid], sMin[1][tid]), min(sMin[2][tid], sMin[3][tid]));
    a.min_dist[(size_t)r * a.n_rep + (size_t)(a.rep0 + (int)blockIdx.y)] = min(m, a.clamp[r]);
  }
}
