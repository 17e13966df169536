// MSA simulation (cherryml/simulation/_simulate_msas.py:94-252, strategy "all_transitions"): one thread per (family, unit)
// walks its family's nodes in preorder and runs the exact jump chain down every edge.
//
// Unit: an independent site (S1 states, rate = its site rate) or a contacting pair (S2 = S1 * S1 states, the caller passes
// rate 1).  Node v's state of a unit is read back from the output rows the same thread wrote for node parent[v] < v, so a
// thread keeps no per-node state: the output [node][site] (int8 codes; a pair writes s / S1 and s % S1 into its two
// columns) is the only memory of the walk.
//
// Random stream (include/cherrybank.h): Philox4x32-10, key = family seed (low, high word), counter
// (u, v, j, 0) for draw j of unit u at node v (preorder index); one block -> two uniforms a, b in (0, 1].  Root: alias draw
// on pi with a (counter (u, 0, 0, 0)).  Edge step j: w = -log(a) / q_s; stop unless t + w < elapsed; else t += w and the next
// state is the alias draw on row s with b.
//
// What bounds the kernel: the jump loop.  A lane makes about elapsed * q_s jumps per edge, so lanes of one wave run loops of
// different lengths and the wave runs the longest; the loop body is one Philox block, one log, one division and two table
// loads, with no branch on which model the lane runs (the lane's table pointers are chosen once, before the walk).
// cb_sim_model_run refuses runs whose expected jumps on one edge exceed CB_SIM_MAX_JUMPS, so no launch can run for minutes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SIM_BLOCK 256            // 4 waves of 64; every block belongs to ONE family (its per-node loads are wave-uniform)
#define SIM_MAX_S1 64            // the S1 tables in LDS: S1^2 (8 + 4) + S1 (8 + 8 + 4) bytes, 50 KB at 64
#define CB_SIM_MAX_JUMPS 1.0e7   // expected jumps of one unit on one edge, at most (elapsed * largest exit rate)

struct SimArgs {
  int S1, S2;                                     // S2 = 0: no pair model
  const double *prob1, *exit1, *piprob1;          // [S1][S1], [S1], [S1] (copied to LDS)
  const int *alias1, *pialias1;                   // [S1][S1], [S1]
  const double *prob2, *exit2, *piprob2;          // [S2][S2], [S2], [S2] (global / L2)
  const int *alias2, *pialias2;
  int n_fam;
  const int *blk_off;                             // [n_fam + 1] first block of each family
  const int *n_nodes, *n_sites, *n_units;         // [n_fam]
  const long long *node_off, *unit_off, *out_off; // [n_fam]
  const unsigned long long *seed;                 // [n_fam]
  const int *parent;                              // [sum n_nodes], family-local preorder indices, -1 at the root
  const double *length;                           // [sum n_nodes]
  const int *site_a, *site_b;                     // [sum n_units], site_b = -1: independent site
  const double *rate;                             // [sum n_units]
  int8_t *out;                                    // [sum n_nodes * n_sites]
};

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t x[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// 53 random bits -> (k + 1/2) 2^-53, in (0, 1]
__device__ __forceinline__ double sim_uniform(uint32_t hi, uint32_t lo) {
  const unsigned long long k = ((unsigned long long)hi << 32 | lo) >> 11;
  return (double)k * 0x1.0p-53 + 0x1.0p-54;
}

// Vose alias draw from one uniform: column k = floor(u n) (clamped), coin = the fraction
__device__ __forceinline__ int sim_alias(const double *prob, const int *alias, int n, double u) {
  const double x = u * (double)n;
  int k = (int)x;
  k = k < n - 1 ? k : n - 1;
  return (x - (double)k) < prob[k] ? k : alias[k];
}

__global__ void __launch_bounds__(SIM_BLOCK) sim_walk(SimArgs a) {
  extern __shared__ double sim_lds[];
  const int S1 = a.S1, S1S1 = S1 * S1;
  double *l_prob = sim_lds, *l_exit = sim_lds + S1S1, *l_piprob = l_exit + S1;
  int *l_alias = reinterpret_cast<int *>(l_piprob + S1), *l_pialias = l_alias + S1S1;
  for (int i = threadIdx.x; i < S1S1; i += SIM_BLOCK) {
    l_prob[i] = a.prob1[i];
    l_alias[i] = a.alias1[i];
  }
  for (int i = threadIdx.x; i < S1; i += SIM_BLOCK) {
    l_exit[i] = a.exit1[i];
    l_piprob[i] = a.piprob1[i];
    l_pialias[i] = a.pialias1[i];
  }
  __syncthreads();

  // the block's family: the last f with blk_off[f] <= blockIdx.x (wave-uniform binary search)
  int lo = 0, hi = a.n_fam - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.blk_off[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int f = lo;
  const int u = ((int)blockIdx.x - a.blk_off[f]) * SIM_BLOCK + (int)threadIdx.x;
  if (u >= a.n_units[f]) return;

  const long long ug = a.unit_off[f] + u;
  const int sa = a.site_a[ug], sb = a.site_b[ug];
  const bool pair = sb >= 0;
  const double rate = a.rate[ug];
  // the lane's model, chosen once: S1 tables in LDS or S2 tables in global memory (flat pointers either way)
  const int n = pair ? a.S2 : S1;
  const double *prob = pair ? a.prob2 : l_prob;
  const int *alias = pair ? a.alias2 : l_alias;
  const double *exitr = pair ? a.exit2 : l_exit;
  const double *piprob = pair ? a.piprob2 : l_piprob;
  const int *pialias = pair ? a.pialias2 : l_pialias;

  const unsigned long long seed = a.seed[f];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int L = a.n_sites[f], nn = a.n_nodes[f];
  const int *parent = a.parent + a.node_off[f];
  const double *length = a.length + a.node_off[f];
  int8_t *out = a.out + a.out_off[f];

  uint32_t x[4];
  philox4x32_10((uint32_t)u, 0u, 0u, 0u, k0, k1, x);
  int s = sim_alias(piprob, pialias, n, sim_uniform(x[1], x[0]));
  out[sa] = (int8_t)(pair ? s / S1 : s);
  if (pair) out[sb] = (int8_t)(s % S1);

  for (int v = 1; v < nn; ++v) {
    const int8_t *prow = out + (long long)parent[v] * L;
    s = pair ? (int)prow[sa] * S1 + (int)prow[sb] : (int)prow[sa];
    const double elapsed = length[v] * rate;
    double t = 0.0;
    for (uint32_t j = 0;; ++j) {
      philox4x32_10((uint32_t)u, (uint32_t)v, j, 0u, k0, k1, x);
      const double w = -log(sim_uniform(x[1], x[0])) / exitr[s];
      if (!(t + w < elapsed)) break;   // (also stops on a NaN: 0 / 0 when a = 1 on an absorbing state)
      t += w;
      s = sim_alias(prob + (long long)s * n, alias + (long long)s * n, n, sim_uniform(x[3], x[2]));
    }
    int8_t *row = out + (long long)v * L;
    row[sa] = (int8_t)(pair ? s / S1 : s);
    if (pair) row[sb] = (int8_t)(s % S1);
  }
}
