// Nearest-neighbour interchange on the branch-length handle (include/cherrybank.h, cb_bl_nni_scan): the
// likelihood of every rearranged tree from the messages the passes of cb_bl.hip leave resident.  A move (v, c, s) of one family --
// v internal and not the root, p = parent[v], c a child of v, s a child of p other than v -- exchanges the subtrees of c and s;
// every node keeps the edge above it.  With msg[w] the inside message at the parent end of the edge above w and U[p] the outside
// message at p (log pi_root at the root), for unit u of category k:
//
//     A[b]  = sum_{c' in ch(v), c' != c} msg[c'][u][b] + msg[s][u][b]
//     w[a]  = log sum_b P[qb[v][k]][a][b] exp(A[b])
//     B[a]  = out_p[u][a] + sum_{s' in ch(p), s' not in {v, s}} msg[s'][u][a] + msg[c][u][a] + w[a]
//     ll'   = log sum_a exp(B[a])
//
// which is the per-site log-likelihood of the rearranged tree at the same indices: nothing outside the two nodes changes.
//
//   nni_scan_kernel  one launch for all moves of a family (of a chunk of them): no levels, a workgroup (one wave) owns one
//                    (move, site tile) and writes ll'[move][unit], nothing else.  tl_group_body's arrangement: thread (g, r) =
//                    site g of the tile, state r; the row of P comes from the bank through qb per unit, so a tile may straddle
//                    categories.  Log space with the maximum per site, log(max(arg, 0)); a term at -inf contributes 0 even where
//                    the maximum is -inf, so an impossible site ends at -inf and not NaN.
//   nni_sum_kernel   one wave per move: delta = sum_u (ll'[u] - l_u) in a fixed order (lane l takes units l, l + 64, ...; then
//                    the xor tree); a unit whose l_u is -inf contributes 0.
// No atomics: the results of a move do not depend on what else the launch holds.
#pragma once
#include "common.hip.h"

struct NniArgs {
  int S, n_units, n_cats, root, n_blocks;   // n_blocks: site tiles
  const int *moves;                  // [moves of the launch][3]: v, c, s
  const int *parent, *child_ptr, *child_idx;
  const int *qb, *unit_cat;
  const double *P;                   // the bank of all families [entry][S][S]
  const double *pi_root;             // [S]
  const double *msg, *U;             // the family's [node][unit][S]
  const double *ll;                  // the family's l_u [unit]
  double *out;                       // [moves of the launch][unit]
  double *delta;                     // [moves of the launch]
};

// the maximum of the S values of the thread's site (sw holds one value per thread)
__device__ __forceinline__ double nni_site_max(const double *sw, int gb, int S) {
  double m = sw[gb];
  for (int k = 1; k < S; ++k) m = fmax(m, sw[gb + k]);
  return m;
}

// grid = moves x site tiles, 64 threads
__global__ __launch_bounds__(64) void nni_scan_kernel(NniArgs a) {
  __shared__ double sw[64];
  const int S = a.S, upw = 64 / S;
  const int g = threadIdx.x / S, r = threadIdx.x - g * S;
  const int mi = blockIdx.x / a.n_blocks, blk = blockIdx.x - mi * a.n_blocks;
  const int u = blk * upw + g;
  const bool act = g < upw && u < a.n_units;
  const int uu = act ? u : 0, gb = act ? g * S : 0, rr = act ? r : 0;
  const int v = a.moves[3 * (size_t)mi], c = a.moves[3 * (size_t)mi + 1], s = a.moves[3 * (size_t)mi + 2];
  const int p = a.parent[v];
  const size_t us = (size_t)uu * S + rr, ns = (size_t)a.n_units * S;
  // the rearranged v: its children but c, and s
  double d = a.msg[(size_t)s * ns + us];
  for (int k = a.child_ptr[v]; k < a.child_ptr[v + 1]; ++k) {
    const int w = a.child_idx[k];
    if (w != c) d += a.msg[(size_t)w * ns + us];
  }
  sw[threadIdx.x] = d;
  __syncthreads();
  double m = nni_site_max(sw, gb, S);
  __syncthreads();
  sw[threadIdx.x] = d > -INFINITY ? exp(d - m) : 0.0;
  __syncthreads();
  const double *Pr = a.P + ((size_t)a.qb[(size_t)v * a.n_cats + a.unit_cat[uu]] * S + rr) * S;
  double arg = 0.0;
  for (int k = 0; k < S; ++k) arg = fma(Pr[k], sw[gb + k], arg);
  // the rearranged p: what is outside it, its children but v and s, c, and the new message of v
  double x = log(arg < 0.0 ? 0.0 : arg) + m;
  x += p == a.root ? log(a.pi_root[rr]) : a.U[(size_t)p * ns + us];
  x += a.msg[(size_t)c * ns + us];
  for (int k = a.child_ptr[p]; k < a.child_ptr[p + 1]; ++k) {
    const int w = a.child_idx[k];
    if (w != v && w != s) x += a.msg[(size_t)w * ns + us];
  }
  __syncthreads();
  sw[threadIdx.x] = x;
  __syncthreads();
  m = nni_site_max(sw, gb, S);
  __syncthreads();
  sw[threadIdx.x] = x > -INFINITY ? exp(x - m) : 0.0;
  __syncthreads();
  arg = 0.0;
  for (int k = 0; k < S; ++k) arg += sw[gb + k];
  if (act && r == 0) a.out[(size_t)mi * a.n_units + u] = log(arg < 0.0 ? 0.0 : arg) + m;
}

// grid = moves, 64 threads
__global__ __launch_bounds__(64) void nni_sum_kernel(NniArgs a) {
  const double *row = a.out + (size_t)blockIdx.x * a.n_units;
  double t = 0.0;
  for (int u = threadIdx.x; u < a.n_units; u += 64) {
    const double l = a.ll[u];
    if (l > -INFINITY) t += row[u] - l;
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) t += __shfl_xor(t, off, 64);
  if (threadIdx.x == 0) a.delta[blockIdx.x] = t;
}
