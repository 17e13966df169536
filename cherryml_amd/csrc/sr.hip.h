// Site rates on fixed full trees: the rate-category scan (include/cherrybank.h, cb_tree_site_rates).
// Every site is evaluated at every candidate rate, so for a fixed (node v, candidate c) ALL sites share the one transition matrix
// P[v][c] = expm(length_v cands[c] Q) -- what the per-unit passes (tl_group.hip.h), whose units carry different categories,
// cannot use.
//
//   sr_scan_kernel  level-synchronous from the leaves up, one launch per height.  One workgroup (one wave) owns one
//                   (node, candidate, site tile): blockIdx.x = node of the height x tile, blockIdx.y = candidate.  It stages
//                   the S x S matrix in LDS once (coalesced) and every site of the tile reads its rows from there.  Leaf codes
//                   stay [node][site] and are read in place for every candidate.  Messages are [node][cand][site][S]: a tile's
//                   loads and stores are one contiguous run.  The arithmetic is tl_group_body's: log space with the maximum per
//                   (site, candidate), log(max(arg, 0)), a gap = all states; the root applies pi_root and writes ll[cand][site].
//   sr_pick_kernel  one thread per site: the candidate of highest log-likelihood; among exact maxima `current` wins if it is one
//                   of them, else the lowest index.  A site with fewer than two observed leaves is decided from the codes, not
//                   from the likelihoods: it keeps `current` (candidate 0 where there is none).
// No atomics: a workgroup writes only its own tile, so the results do not depend on what else the launch or the call holds.
#pragma once
#include "common.hip.h"

#define SR_LDS_PAD 1   // row stride S + 1 doubles: the S lanes of a site (rows r, the same column) fall into different banks

struct SrScanArgs {
  int S, n_units, n_cands;     // n_cands: the family's candidates (the bank's and ll's stride)
  int c0;                      // the first candidate of this launch (blockIdx.y counts from it; msg holds this chunk only)
  int n_chunk;                 // candidates of this chunk (msg's stride)
  int root, n_blocks;          // n_blocks: site tiles
  const int *level_nodes;      // nodes of the height processed by this launch
  const int *child_ptr, *child_idx;
  const double *P;             // [node][cand][S][S], the edge above `node`
  const signed char *codes;    // [node][site] (-1: a gap); leaves only
  const double *pi_root;       // [S]
  double *msg;                 // [node][chunk cand][site][S]
  double *ll;                  // [cand][site]
};

// grid = (nodes of the level x site tiles, candidates of the chunk), 64 threads: thread (g, r) = site g of the tile, state r
__global__ __launch_bounds__(64) void sr_scan_kernel(SrScanArgs a) {
  __shared__ double sP[32 * (32 + SR_LDS_PAD)];
  __shared__ double sw[64];
  const int S = a.S, upw = 64 / S, ld = S + SR_LDS_PAD;
  const int g = threadIdx.x / S, r = threadIdx.x - g * S;
  const int node_i = blockIdx.x / a.n_blocks, blk = blockIdx.x - node_i * a.n_blocks;
  const int cl = blockIdx.y, c = a.c0 + cl;
  const int u = blk * upw + g;
  const bool act = g < upw && u < a.n_units;
  const int uu = act ? u : 0, gb = act ? g * S : 0;
  const int v = a.level_nodes[node_i];
  const int c0 = a.child_ptr[v], c1 = a.child_ptr[v + 1];
  if (v != a.root) {   // the one matrix of (v, c), once for all sites of the tile
    const double *Pv = a.P + ((size_t)v * a.n_cands + c) * S * S;
    for (int e = threadIdx.x; e < S * S; e += 64) {
      const int i = e / S;
      sP[i * ld + (e - i * S)] = Pv[e];
    }
  }
  double d = 0.0;
  for (int k = c0; k < c1; ++k) d += a.msg[(((size_t)a.child_idx[k] * a.n_chunk + cl) * a.n_units + uu) * S + r];
  sw[threadIdx.x] = d;
  __syncthreads();
  double m = sw[gb];
  for (int k = 1; k < S; ++k) m = fmax(m, sw[gb + k]);
  __syncthreads();
  bool obs = true;
  if (c0 == c1) {  // leaf
    const int code = a.codes[(size_t)v * a.n_units + uu];
    obs = code < 0 || code == r;
  }
  sw[threadIdx.x] = obs && d > -INFINITY ? exp(d - m) : 0.0;   // (m = -inf: an impossible site stays at -inf, not NaN)
  __syncthreads();
  double arg = 0.0;
  if (v == a.root) {
    for (int k = 0; k < S; ++k) arg = fma(a.pi_root[k], sw[gb + k], arg);
    if (act && r == 0) a.ll[(size_t)c * a.n_units + u] = log(arg < 0.0 ? 0.0 : arg) + m;
  } else {
    const double *Pr = sP + (act ? r : 0) * ld;
    for (int k = 0; k < S; ++k) arg = fma(Pr[k], sw[gb + k], arg);
    if (act) a.msg[(((size_t)v * a.n_chunk + cl) * a.n_units + u) * S + r] = log(arg < 0.0 ? 0.0 : arg) + m;
  }
}

struct SrPickArgs {
  int n_units, n_cands, n_leaves;
  const int *leaves;           // [n_leaves] the family's leaf nodes
  const signed char *codes;    // [node][site]
  const int *current;          // [n_units] or null
  const double *ll;            // [cand][site]
  int *best;                   // [n_units]
  double *best_ll;             // [n_units]
};

// grid = ceil(n_units / 256), 256 threads: one thread per site
__global__ __launch_bounds__(256) void sr_pick_kernel(SrPickArgs a) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= a.n_units) return;
  const int cur = a.current ? a.current[u] : -1;
  int seen = 0;
  for (int k = 0; k < a.n_leaves && seen < 2; ++k) seen += a.codes[(size_t)a.leaves[k] * a.n_units + u] >= 0;
  int b = cur >= 0 ? cur : 0;
  if (seen >= 2) {
    b = 0;
    double top = a.ll[u];
    for (int c = 1; c < a.n_cands; ++c) {
      const double x = a.ll[(size_t)c * a.n_units + u];
      if (x > top) {
        top = x;
        b = c;
      }
    }
    if (cur >= 0 && a.ll[(size_t)cur * a.n_units + u] == top) b = cur;
  }
  a.best[u] = b;
  a.best_ll[u] = a.ll[(size_t)b * a.n_units + u];
}
