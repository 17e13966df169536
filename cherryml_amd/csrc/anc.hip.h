// Marginal ancestral reconstruction on the branch-length handle (include/cherrybank.h, cb_bl_ancestral): the
// posterior of the state at EVERY node of a family from the messages the passes of cb_bl.hip leave resident.  With msg[c] the
// inside message at the parent end of the edge above c and U[w] the outside message at an internal node w, for unit u of category
// k the node w has an inside part L_w and an outside part U_w (log space):
//
//     root                   L_w[a] = sum_{c in ch(w)} msg[c][u][a]            U_w[a] = log pi_root[a]
//     internal, not the root L_w[a] = sum_{c in ch(w)} msg[c][u][a]            U_w[a] = U[w][u][a]
//     leaf                   L_w[a] = 0 if the code is a gap or a, else -inf   U_w[a] = log sum_a' exp(x[a']) P[qb[w][k]][a'][a]
//
// with x = U_p (log pi_root if p = parent[w] is the root) + sum_{siblings s != w} msg[s][u]: the outside pass stops at the internal
// nodes, so a leaf's outside message -- em_down_kernel's formula applied to a leaf -- is this kernel's own S x S product.  Then
//
//     z = L_w + U_w,  m = max z,  post[a] = exp(z[a] - m) / sum_b exp(z[b] - m),  state = argmax_a post[a],  conf = post[state]
//
// the posterior normalised by its own sum (not by l_u), the argmax the lowest index among exactly equal maxima.  A site whose z is
// -inf (or, from an inside pass that met -inf - -inf, NaN) at every state is impossible: state -1, conf 0, post 0, never NaN.
//
//   anc_post_kernel  one launch for all nodes of a family (of a chunk of them): no levels, a workgroup (one wave) owns one
//                    (node, site tile) and writes state, conf and post of its tile, nothing else.  tl_group_body's arrangement:
//                    thread (g, r) = site g of the tile, state r; the leaf's column of P comes from the bank through qb per unit,
//                    so a tile may straddle categories.  Log space with the maximum per site, log(max(arg, 0)).
// No atomics: the results of a node do not depend on what else the launch holds.
#pragma once
#include "common.hip.h"

struct AncArgs {
  int S, n_units, n_cats, root, n_blocks;   // n_blocks: site tiles
  int node0;                         // the first node of the launch
  const int *parent, *child_ptr, *child_idx;
  const int *qb, *unit_cat;
  const signed char *codes;          // the family's [node][unit]; leaf rows are read
  const double *P;                   // the bank of all families [entry][S][S]
  const double *pi_root;             // [S]
  const double *msg, *U;             // the family's [node][unit][S]
  signed char *state;                // [nodes of the launch][unit]
  double *conf;                      // [nodes of the launch][unit]
  double *post;                      // [nodes of the launch][unit][S], or null
};

// the maximum of the S values of the thread's site (sw holds one value per thread); a NaN is passed over
__device__ __forceinline__ double anc_site_max(const double *sw, int gb, int S) {
  double m = sw[gb];
  for (int k = 1; k < S; ++k) m = fmax(m, sw[gb + k]);
  return m;
}

// grid = nodes of the launch x site tiles, 64 threads
__global__ __launch_bounds__(64) void anc_post_kernel(AncArgs a) {
  __shared__ double sw[64];
  const int S = a.S, upw = 64 / S;
  const int g = threadIdx.x / S, r = threadIdx.x - g * S;
  const int ni = blockIdx.x / a.n_blocks, blk = blockIdx.x - ni * a.n_blocks;
  const int u = blk * upw + g;
  const bool act = g < upw && u < a.n_units;
  const int uu = act ? u : 0, gb = act ? g * S : 0, rr = act ? r : 0;
  const int w = a.node0 + ni;        // (the same for the whole workgroup: the branches below are uniform)
  const size_t us = (size_t)uu * S + rr, ns = (size_t)a.n_units * S;
  const int c0 = a.child_ptr[w], c1 = a.child_ptr[w + 1];
  double z;
  if (w == a.root) {
    z = log(a.pi_root[rr]);
  } else if (c0 < c1) {
    z = a.U[(size_t)w * ns + us];
  } else {
    // the outside message of a leaf: what is outside its parent and its siblings, through the edge above it
    const int p = a.parent[w];
    double x = p == a.root ? log(a.pi_root[rr]) : a.U[(size_t)p * ns + us];
    for (int k = a.child_ptr[p]; k < a.child_ptr[p + 1]; ++k) {
      const int s = a.child_idx[k];
      if (s != w) x += a.msg[(size_t)s * ns + us];
    }
    sw[threadIdx.x] = x;
    __syncthreads();
    double mx = anc_site_max(sw, gb, S);
    if (!(mx > -INFINITY)) mx = 0.0;
    __syncthreads();
    sw[threadIdx.x] = x > -INFINITY ? exp(x - mx) : 0.0;
    __syncthreads();
    const double *Pc = a.P + (size_t)a.qb[(size_t)w * a.n_cats + a.unit_cat[uu]] * S * S + rr;   // column r of P_w
    double arg = 0.0;
    for (int k = 0; k < S; ++k) arg = fma(sw[gb + k], Pc[(size_t)k * S], arg);
    z = log(arg < 0.0 ? 0.0 : arg) + mx;
    __syncthreads();
  }
  if (c0 < c1) {
    for (int k = c0; k < c1; ++k) z += a.msg[(size_t)a.child_idx[k] * ns + us];
  } else {
    const int code = a.codes[(size_t)w * a.n_units + uu];
    if (!(code < 0 || code == rr)) z = -INFINITY;
  }
  sw[threadIdx.x] = z;
  __syncthreads();
  const double m = anc_site_max(sw, gb, S);
  const bool ok = m > -INFINITY;     // false for an impossible site, all -inf or NaN
  __syncthreads();
  const double e = z > -INFINITY ? exp(z - m) : 0.0;
  sw[threadIdx.x] = e;
  __syncthreads();
  double sum = 0.0;
  for (int k = 0; k < S; ++k) sum += sw[gb + k];
  const double post = ok ? e / sum : 0.0;
  __syncthreads();
  sw[threadIdx.x] = post;
  __syncthreads();
  if (!act) return;
  const size_t o = (size_t)ni * a.n_units + u;
  if (a.post) a.post[o * S + r] = post;
  if (r == 0) {
    int best = 0;
    for (int k = 1; k < S; ++k)
      if (sw[gb + k] > sw[gb + best]) best = k;
    a.state[o] = (signed char)(ok ? best : -1);
    a.conf[o] = ok ? sw[gb + best] : 0.0;
  }
}
