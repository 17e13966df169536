// Maximum-likelihood branch lengths on fixed trees by EM over the internal states: the lengths are the
// parameters and live on the quantisation grid, tau_v = the index of the edge above node v; Q, the root distribution and the site
// rates are fixed.  The edge above v carries P[tau_v][c] = expm(grid[tau_v] rate_c Q) at a site of category c -- the exact product of
// length and rate, one bank of T x R matrices per family, built once.
//
//   E-step   em_up_kernel / em_down_kernel (em.hip.h, launched through em_shared.hip.h) unchanged: qb[v][c] points at bank
//            entry (tau_v, c).
//   M-step   bl_mstep_kernel, one wave per (family, edge): per category segment (a family's categories are its distinct
//            rates: none is empty) the wave forms
//              Z_vc = sum_{u in c} X_u diag(s_u) Y_u^T   (bl_operands + v_mfma_f64_16x16x4, as em_acc_kernel)
//              E_vc = P[tau_v][c] o Z_vc                  (into LDS)
//            and adds <E_vc, log P[tau][c]> to the score of EVERY grid point tau (lanes run over tau); then
//              tau_v' = argmax_tau score, the lowest index among exact maxima,
//            and rewrites its own row of qb.  The E-step used the very P[tau][c] the M-step ranks and tau_v is a candidate, so a
//            round is an exact EM step for all edges at once: no family's likelihood goes down.
//   bl_log_kernel  once per family at creation: log of the bank, transposed to [c][a][b][tau] so that the M-step's lanes
//            (consecutive tau) read consecutive addresses.
// No atomics; an edge reads and writes only its own rows, so the update is in place.
#pragma once
#include "common.hip.h"
#include "em_shared.hip.h"

// grid = ceil(T R S S / 256), 256 threads.  P: the family's bank [tau][c][a][b]; logP: [c][a][b][tau].  An entry that is not
// positive (an exact or rounded zero of expm) has log -inf: such a candidate loses wherever the edge has expected counts.
__global__ __launch_bounds__(256) void bl_log_kernel(int T, int R, int SS, const double *__restrict__ P, double *__restrict__ logP) {
  const size_t n = (size_t)T * R * SS, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t ce = i / T;                 // c * SS + e
  const int tau = int(i - ce * T);
  const size_t c = ce / SS, e = ce - c * SS;
  const double p = P[((size_t)tau * R + c) * SS + e];
  logP[i] = p > 0.0 ? log(p) : -INFINITY;
}

// max over the 16 lanes of one lane row (same hi)
__device__ __forceinline__ double bl_max16(double x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x = fmax(x, __shfl_xor(x, off, 64));
  return x;
}

constexpr int BL_NT = 2;   // S <= 32: the 32 x 32 padded Z as 2 x 2 tiles

// The MFMA operands of one accumulation step -- em_acc_kernel's step (em.hip.h), restated here: as a function shared by both
// kernels it cost em_acc_kernel SGPR spills, so that kernel keeps its own text.  For unit u of
// one family (valid: the step's lane row has a unit), edge above v with parent p, the lane's states lo + 16 i:
// A[i] = X = exp(x - max x), Bv[i] = s Y = exp(max x + max y - l_u) exp(y - max y).  cidx / codes / msg / U: the family's views;
// l_u at ll[u].
__device__ __forceinline__ void bl_operands(int S, int lo, bool valid, int u, int n_units, int v, int p, int root, int pc0, int pc1,
                                            int vc0, int vc1, const int *cidx, const signed char *codes, const double *pi_root,
                                            const double *msg, const double *U, const double *ll, double (&A)[BL_NT],
                                            double (&Bv)[BL_NT]) {
  const int code = vc0 == vc1 ? codes[(size_t)v * n_units + u] : -1;
  // x = U_p (log pi_root at the root) + the siblings' messages, y = the children's messages (a leaf: log of its 0/1 vector);
  // the state loop innermost, so that the child loops are shared by the BL_NT rows
  const double *urow = p == root ? nullptr : U + ((size_t)p * n_units + u) * S;
  double x[BL_NT], y[BL_NT];
#pragma unroll
  for (int i = 0; i < BL_NT; ++i) {
    const int s = lo + 16 * i;
    x[i] = s < S ? (urow ? urow[s] : log(pi_root[s])) : -INFINITY;
    y[i] = s < S && (code < 0 || code == s) ? 0.0 : -INFINITY;
  }
  for (int c = pc0; c < pc1; ++c) {
    const int w = cidx[c];
    if (w == v) continue;
    const double *mr = msg + ((size_t)w * n_units + u) * S;
#pragma unroll
    for (int i = 0; i < BL_NT; ++i)
      if (lo + 16 * i < S) x[i] += mr[lo + 16 * i];
  }
  for (int c = vc0; c < vc1; ++c) {
    const double *mr = msg + ((size_t)cidx[c] * n_units + u) * S;
#pragma unroll
    for (int i = 0; i < BL_NT; ++i)
      if (lo + 16 * i < S) y[i] += mr[lo + 16 * i];
  }
  double mx = x[0], my = y[0];
#pragma unroll
  for (int i = 1; i < BL_NT; ++i) {
    mx = fmax(mx, x[i]);
    my = fmax(my, y[i]);
  }
  mx = bl_max16(mx);
  my = bl_max16(my);
  const bool ok = valid && mx > -INFINITY && my > -INFINITY;
  const double sc = ok ? exp(mx + my - ll[u]) : 0.0;
#pragma unroll
  for (int i = 0; i < BL_NT; ++i) {
    A[i] = ok ? exp(x[i] - mx) : 0.0;
    Bv[i] = ok ? sc * exp(y[i] - my) : 0.0;
  }
}

struct BlArgs {
  int S, T, n_cats, n_units, root;
  int bank_base;                     // the family's first entry of the bank: entry (tau, c) is bank_base + tau n_cats + c
  const int *parent, *child_ptr, *child_idx, *cat_ptr;   // the family's views; cat_ptr [n_cats + 1]: units of each category
  const signed char *codes;          // [node][unit]
  const double *pi_root;
  const double *msg, *U, *ll;        // the family's messages and l_u
  const double *P;                   // the bank of all families [entry][S][S]
  const double *logP;                // the family's [c][a][b][tau]
  int *qb;                           // the family's [node][n_cats]: bank entries, rewritten for the wave's own edge
  int *tau, *changed;                // the family's [node]
};

constexpr int BL_CH = 4;   // candidates per lane and sweep: one sweep ranks 256 grid points

// grid = the family's nodes, one wave each (the root's returns).  Lane layout of the accumulation as in em_acc_kernel; in the
// scoring lane l holds the candidates t0 + l + 64 j (j < BL_CH) of sweep t0.  A grid of more than 64 BL_CH points takes several
// sweeps, each forming Z again (the statistics of one edge are cheaper than a score buffer of unbounded size).
__global__ __launch_bounds__(64) void bl_mstep_kernel(BlArgs a) {
  __shared__ double Es[32 * 32];
  const int v = blockIdx.x;
  if (v == a.root) return;
  const int S = a.S, T = a.T, SS = S * S, lane = threadIdx.x, lo = lane & 15, hi = lane >> 4;
  const int p = a.parent[v];
  const int pc0 = a.child_ptr[p], pc1 = a.child_ptr[p + 1], vc0 = a.child_ptr[v], vc1 = a.child_ptr[v + 1];
  const int *qrow = a.qb + (size_t)v * a.n_cats;
  const int old = a.tau[v];
  double best = -INFINITY;
  int best_i = T;                    // (no candidate yet)
  for (int t0 = 0; t0 < T; t0 += 64 * BL_CH) {
    double score[BL_CH];
#pragma unroll
    for (int j = 0; j < BL_CH; ++j) score[j] = 0.0;
    for (int c = 0; c < a.n_cats; ++c) {
      const int u0 = a.cat_ptr[c], n = a.cat_ptr[c + 1] - u0;
      d4 acc[BL_NT][BL_NT];
#pragma unroll
      for (int i = 0; i < BL_NT; ++i)
#pragma unroll
        for (int j = 0; j < BL_NT; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
      for (int k = 0; k < n; k += 4) {
        const bool valid = k + hi < n;
        const int u = u0 + (valid ? k + hi : 0);
        double A[BL_NT], Bv[BL_NT];
        bl_operands(S, lo, valid, u, a.n_units, v, p, a.root, pc0, pc1, vc0, vc1, a.child_idx, a.codes, a.pi_root, a.msg, a.U, a.ll,
                    A, Bv);
#pragma unroll
        for (int i = 0; i < BL_NT; ++i)
#pragma unroll
          for (int j = 0; j < BL_NT; ++j) acc[i][j] = mfma_f64(A[i], Bv[j], acc[i][j]);
      }
      const double *Pc = a.P + (size_t)qrow[c] * SS;
      __syncthreads();               // the previous category's scoring is done with Es
#pragma unroll
      for (int i = 0; i < BL_NT; ++i)
#pragma unroll
        for (int j = 0; j < BL_NT; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * i + hi + 4 * r, col = 16 * j + lo;
            if (row < S && col < S) Es[row * S + col] = Pc[(size_t)row * S + col] * acc[i][j][r];
          }
      __syncthreads();
      const double *lp = a.logP + (size_t)c * SS * T;
      size_t at[BL_CH];
#pragma unroll
      for (int j = 0; j < BL_CH; ++j) at[j] = (size_t)min(t0 + lane + 64 * j, T - 1);
      for (int e = 0; e < SS; ++e) {
        const double w = Es[e];
        if (!(w > 0.0)) continue;    // (the same for all lanes) E = 0 contributes 0, even where log P = -inf
        const double *row = lp + (size_t)e * T;
#pragma unroll
        for (int j = 0; j < BL_CH; ++j)
          if (t0 + 64 * j < T) score[j] += w * row[at[j]];
      }
    }
#pragma unroll
    for (int j = 0; j < BL_CH; ++j) {
      const int t = t0 + lane + 64 * j;
      if (t < T && (best_i == T || score[j] > best)) {
        best = score[j];
        best_i = t;
      }
    }
  }
  // the wave's argmax, the lowest index among equal scores (every lane ends with the same pair)
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double ob = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(best_i, off, 64);
    if (oi < T && (best_i == T || ob > best || (ob == best && oi < best_i))) {
      best = ob;
      best_i = oi;
    }
  }
  if (lane == 0) {
    a.tau[v] = best_i;
    a.changed[v] = best_i != old;
  }
  for (int c = lane; c < a.n_cats; c += 64) a.qb[(size_t)v * a.n_cats + c] = a.bank_base + best_i * a.n_cats + c;
}
