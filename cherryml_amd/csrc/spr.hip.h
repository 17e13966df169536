// Subtree prune-and-regraft on the branch-length handle (include/cherrybank.h, cb_bl_spr_scan): the
// likelihood of every rearranged tree from the messages the passes of cb_bl.hip leave resident.  A move (x, y, ts, tp, ty) of one
// family -- p = parent[x] binary and not the root, s the other child of p, g = parent[p] -- dissolves p (s hangs from g at index
// ts) and puts it back on the edge above y (p under parent[y] at index tp, y under p at index ty; x stays under p).  With msg[w]
// the inside message at the parent end of the edge above w, U[w] the outside message at internal w (log pi_root at the root),
// up(t, d)[a] = log sum_b P[t][k][a][b] exp(d[b]) and down(t, o)[b] = log sum_a exp(o[a]) P[t][k][a][b] for unit u of category k,
//
//     ll' = log sum_a exp( O'[a] + up(tp, msg[x] + up(ty, I'))[a] )
//
// where I' is what is inside y and O' what is outside y at parent[y], both in the tree without x and p.  They differ from the
// resident messages only along the way from the prune point to y, which cb_bl.hip walks on the host while it validates the move
// and writes down as a record of at most CB_SPR_MAX_RADIUS + 1 steps and a last one:
//
//     step:  cur = { nothing | up(tau, cur) | down(tau, cur) } + spr_term(node, ex1, ex2, flags)
//     last:  the other of (I', O') = spr_term(node, ex1, -1, flags); cur is I' (cur_inside) or O'
//     spr_term = the indicator of the leaf's code                                   (SPR_LEAF)
//              | sum of msg[c] over the children c of node but ex1 and ex2  [+ U[node], log pi_root at the root]   (SPR_ADD_U)
//
// A message that has to be left out is never subtracted (-inf is a legal value): the record names the children to skip.
//
//   spr_scan_kernel  one launch for all moves of a family (of a chunk of them): a workgroup (one wave) owns one (move, site tile)
//                    and writes ll'[move][unit], nothing else.  nni_scan_kernel's arrangement: thread (g, r) = site g of the
//                    tile, state r; up reads row r of P, down column r (at fixed a the lanes of a site read consecutive
//                    addresses); the matrix is the bank's entry bank_base + tau n_cats + k.  The record is wave-uniform and
//                    read from global memory.  Log space with the maximum per site, log(max(arg, 0)); a term at -inf
//                    contributes 0 even where the maximum is -inf.
// delta = sum_u (ll' - l_u) is nni_sum_kernel's (nni.hip.h), on the same out / ll / delta fields.
// No atomics: the results of a move do not depend on what else the launch holds.
#pragma once
#include "common.hip.h"
#include "nni.hip.h"

constexpr int SPR_HEAD = 4;                                             // n_steps, x, tau_p, tau_y
constexpr int SPR_STEP = 6;                                             // op, tau, node, ex1, ex2, flags
constexpr int SPR_REC = SPR_HEAD + SPR_STEP * (CB_SPR_MAX_RADIUS + 2);  // ints per move
enum { SPR_NONE = 0, SPR_UP = 1, SPR_DOWN = 2 };                        // op (the last step: cur_inside)
enum { SPR_ADD_U = 1, SPR_LEAF = 2 };                                   // flags

struct SprArgs {
  int S, n_units, n_cats, root, n_blocks, bank_base;
  const int *rec;                    // [moves of the launch][SPR_REC]
  const int *child_ptr, *child_idx, *unit_cat;
  const signed char *codes;          // [node][unit]
  const double *P;                   // the bank of all families [entry][S][S]
  const double *pi_root;             // [S]
  const double *msg, *U;             // the family's [node][unit][S]
  double *out;                       // [moves of the launch][unit]
};

__device__ __forceinline__ double spr_term(const SprArgs &a, int node, int ex1, int ex2, int flags, int uu, int rr, size_t us,
                                           size_t ns) {
  if (flags & SPR_LEAF) {
    const int code = a.codes[(size_t)node * a.n_units + uu];
    return code < 0 || code == rr ? 0.0 : -INFINITY;
  }
  double d = 0.0;
  if (flags & SPR_ADD_U) d = node == a.root ? log(a.pi_root[rr]) : a.U[(size_t)node * ns + us];
  for (int k = a.child_ptr[node]; k < a.child_ptr[node + 1]; ++k) {
    const int w = a.child_idx[k];
    if (w != ex1 && w != ex2) d += a.msg[(size_t)w * ns + us];
  }
  return d;
}

// log sum_k M[k * stride] exp(d_k) over the S values d_k of the thread's site; every thread of the workgroup calls it
__device__ __forceinline__ double spr_product(double *sw, double d, const double *M, int stride, int gb, int S) {
  sw[threadIdx.x] = d;
  __syncthreads();
  const double m = nni_site_max(sw, gb, S);
  __syncthreads();
  sw[threadIdx.x] = d > -INFINITY ? exp(d - m) : 0.0;
  __syncthreads();
  double arg = 0.0;
  for (int k = 0; k < S; ++k) arg = fma(M[(size_t)k * stride], sw[gb + k], arg);
  __syncthreads();
  return log(arg < 0.0 ? 0.0 : arg) + m;
}

// grid = moves x site tiles, 64 threads
__global__ __launch_bounds__(64) void spr_scan_kernel(SprArgs a) {
  __shared__ double sw[64];
  const int S = a.S, upw = 64 / S;
  const int g = threadIdx.x / S, r = threadIdx.x - g * S;
  const int mi = blockIdx.x / a.n_blocks, blk = blockIdx.x - mi * a.n_blocks;
  const int u = blk * upw + g;
  const bool act = g < upw && u < a.n_units;
  const int uu = act ? u : 0, gb = act ? g * S : 0, rr = act ? r : 0;
  const size_t us = (size_t)uu * S + rr, ns = (size_t)a.n_units * S;
  const int *rec = a.rec + (size_t)mi * SPR_REC;
  const int n_steps = rec[0], x = rec[1];
  // the unit's matrices: entry bank_base + tau n_cats + k
  const double *Pk = a.P + (size_t)(a.bank_base + a.unit_cat[uu]) * S * S;
  const size_t tstride = (size_t)a.n_cats * S * S;
  double cur = 0.0;
  for (int i = 0; i < n_steps; ++i) {
    const int *st = rec + SPR_HEAD + SPR_STEP * i;
    const int op = st[0];
    if (op == SPR_UP) cur = spr_product(sw, cur, Pk + (size_t)st[1] * tstride + (size_t)rr * S, 1, gb, S);
    else if (op == SPR_DOWN) cur = spr_product(sw, cur, Pk + (size_t)st[1] * tstride + rr, S, gb, S);
    cur += spr_term(a, st[2], st[3], st[4], st[5], uu, rr, us, ns);
  }
  const int *st = rec + SPR_HEAD + SPR_STEP * n_steps;
  const double other = spr_term(a, st[2], st[3], -1, st[5], uu, rr, us, ns);
  const double in = st[0] ? cur : other, outside = st[0] ? other : cur;
  // y under p at tau_y, x beside it, p under parent[y] at tau_p
  double w = spr_product(sw, in, Pk + (size_t)rec[3] * tstride + (size_t)rr * S, 1, gb, S);
  w += a.msg[(size_t)x * ns + us];
  w = spr_product(sw, w, Pk + (size_t)rec[2] * tstride + (size_t)rr * S, 1, gb, S);
  w += outside;
  sw[threadIdx.x] = w;
  __syncthreads();
  const double m = nni_site_max(sw, gb, S);
  __syncthreads();
  sw[threadIdx.x] = w > -INFINITY ? exp(w - m) : 0.0;
  __syncthreads();
  double arg = 0.0;
  for (int k = 0; k < S; ++k) arg += sw[gb + k];
  if (act && r == 0) a.out[(size_t)mi * a.n_units + u] = log(arg < 0.0 ? 0.0 : arg) + m;
}
