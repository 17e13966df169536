// The pruning state shared by the held-out likelihood (likelihood.hip.h) and the EM inside pass (em.hip.h): the argument
// block and the S <= 64 pruning step as a device function (kernels are defined by the headers that include this one).
#pragma once
#include "common.hip.h"

struct TlArgs {
  int S, S1;                   // states; S1 > 0: pair model over an S1-letter alphabet
  int n_nodes, n_units, NU;    // NU: units padded to the message layout's unit stride
  int root, n_level, n_blocks;  // this launch: nodes of one height x unit blocks (1-D grid)
  int RS;                      // tl_mfma_kernel: row splits per (node, unit block)
  const int *level_nodes;      // nodes of the height processed by this launch
  const int *child_ptr, *child_idx;   // CSR children, in the reference's child order
  const double *P;             // [cat][node][S][S] transition matrices of the edge above `node`
  const int *unit_cat;         // [n_units] rate category of each unit
  const signed char *code_a, *code_b;  // [node][unit] observed state (-1: unobserved); leaves only
  const double *pi_root;       // [S]
  double *msg;                 // upward messages (layout per kernel)
  double *ll;                  // [n_units]
  // S > 64 with a reversible model (round 6): the bank holds INTERNAL nodes only -- slot[v] (-1: none) -- and the leaves take their
  // messages from the model's eigendecomposition (tl_leaf_mfma_kernel)
  const int *slot;             // [n_nodes] or null (P indexed by node)
  const double *tnode;         // [n_nodes] rate x branch length above the node
  const double *U, *lam, *dsq, *sigma;   // U [LD][LD] row-major, lam [LD], dsq = sqrt(pi) [LD], sigma = max |A_ii|
  const double *TU, *TA;       // [nJ][LD]: sum_{j in J} U[j][k] d_j  and  sum_{j in J} A[i][j] d_j  (tl_tables_kernel)
  int LD;
};

__device__ __forceinline__ bool tl_observed(int S1, int k, int ca, int cb) {
  if (S1 > 0) return (ca < 0 || k / S1 == ca) && (cb < 0 || k % S1 == cb);
  return ca < 0 || ca == k;
}

// ------------------------------------------------------------------ S <= 64
// grid = nodes of the level x unit blocks, 64 threads.  msg layout [node][unit][S].
// The body takes the edge's transition matrix from `prow(unit, node, row)` (a pointer to row `row` of P above `node` for
// the unit's rate category): tl_group_kernel reads the per-(category, node) bank, the EM inside pass (em.hip.h) a bank of
// grid points indexed by the edge's bucket.
template <class PRow>
__device__ __forceinline__ void tl_group_body(const TlArgs &a, PRow prow) {
  __shared__ double sw[64];
  const int S = a.S, upw = 64 / S;
  const int g = threadIdx.x / S, r = threadIdx.x - g * S;
  const int node_i = blockIdx.x / a.n_blocks, blk = blockIdx.x - node_i * a.n_blocks;
  const int u = blk * upw + g;
  const bool act = g < upw && u < a.n_units;
  const int uu = act ? u : 0, gb = act ? g * S : 0;
  const int v = a.level_nodes[node_i];
  const int c0 = a.child_ptr[v], c1 = a.child_ptr[v + 1];
  double d = 0.0;
  for (int c = c0; c < c1; ++c) d += a.msg[((size_t)a.child_idx[c] * a.n_units + uu) * S + r];
  sw[threadIdx.x] = d;
  __syncthreads();
  double m = sw[gb];
  for (int k = 1; k < S; ++k) m = fmax(m, sw[gb + k]);
  __syncthreads();
  bool obs = true;
  if (c0 == c1) {  // leaf
    const size_t ci = (size_t)v * a.n_units + uu;
    obs = tl_observed(a.S1, r, a.code_a[ci], a.S1 > 0 ? a.code_b[ci] : -1);
  }
  sw[threadIdx.x] = obs ? exp(d - m) : 0.0;
  __syncthreads();
  double arg = 0.0;
  if (v == a.root) {
    for (int k = 0; k < S; ++k) arg = fma(a.pi_root[k], sw[gb + k], arg);
    if (act && r == 0) a.ll[u] = log(arg < 0.0 ? 0.0 : arg) + m;
  } else {
    const double *Pr = prow(uu, v, r);
    for (int k = 0; k < S; ++k) arg = fma(Pr[k], sw[gb + k], arg);
    if (act) a.msg[((size_t)v * a.n_units + uu) * S + r] = log(arg < 0.0 ? 0.0 : arg) + m;
  }
}
