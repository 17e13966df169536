// Full-tree EM for the 20-state model (reference: cherryml/estimation/_em_lg.py:251, which runs Historian / XRATE): the
// E-step on the GPU.  The states at the internal nodes are the missing data; every edge length x site rate is put on the
// quantisation grid, so the transition matrix of (node v, rate category c) is P_beta = expm(grid[beta] Q), beta = q(t_v r_c).
// Per unit u (one site), with msg the upward messages of likelihood.hip.h (log space, [node][unit][S]):
//
//   inside   em_up_kernel      tl_group_body (tl_group.hip.h) with P read from the bank of grid points by bucket;
//                              leaves: 0/1 observation vectors (a gap: all states); the root writes l_u.
//   outside  em_down_kernel    level-synchronous, root first, INTERNAL non-root nodes only (leaves are nobody's parent):
//                                U_v[b] = log sum_a exp(x_v[a]) P_v[a][b],  x_v = U_p + sum_{siblings c != v} msg_c
//                              with U_root = log pi_root; log space with the per-unit maximum, as the inside pass.
//   expected counts            the posterior of (x_p = a, x_v = b) at unit u is exp(x_v[a]) P_v[a][b] exp(y_v[b]) / exp(l_u),
//                              y_v = d_v + log obs_v (d_v = sum_{children} msg), so per bucket
//                                Z_beta = sum_{(v, u) in beta} X_u diag(s_u) Y_u^T,  X = exp(x_v - m), Y = exp(y_v - m'),
//                                s_u = exp(m + m' - l_u),    E_beta = P_beta o Z_beta.
//            em_acc_kernel     one wave per TASK -- a fixed run of (edge, unit range) segments of ONE bucket -- forms its
//                              partial Z as v_mfma_f64_16x16x4 tiles (rows a, columns b, 4 units per step; S <= 32 padded to 32)
//                              and stores it; no atomics.
//            em_reduce_kernel  one workgroup per bucket sums its tasks' partials in task order and multiplies by P_beta.
// The task lists are fixed at handle creation, so two E-steps on the same input give bitwise-equal counts.
#pragma once
#include "common.hip.h"
#include "em_shared.hip.h"

// inside pass: tl_group_body with P_v of unit u = bank[qb[v * n_cats + unit_cat[u]]]
__global__ __launch_bounds__(64) void em_up_kernel(TlArgs a, const int *__restrict__ qb, int n_cats) {
  tl_group_body(a, [&](int uu, int v, int r) {
    return a.P + ((size_t)qb[(size_t)v * n_cats + a.unit_cat[uu]] * a.S + r) * a.S;
  });
}

// grid = nodes of the depth x unit blocks, 64 threads; lane = (unit in wave, state): state a while x is formed, b for U_v[b]
__global__ __launch_bounds__(64) void em_down_kernel(EmDownArgs a) {
  __shared__ double sw[64];
  const int S = a.S, upw = 64 / S;
  const int g = threadIdx.x / S, r = threadIdx.x - g * S;
  const int node_i = blockIdx.x / a.n_blocks, blk = blockIdx.x - node_i * a.n_blocks;
  const int u = blk * upw + g;
  const bool act = g < upw && u < a.n_units;
  const int uu = act ? u : 0, gb = act ? g * S : 0;
  const int v = a.level_nodes[node_i], p = a.parent[v];
  double x = p == a.root ? log(a.pi_root[r]) : a.U[((size_t)p * a.n_units + uu) * S + r];
  for (int c = a.child_ptr[p]; c < a.child_ptr[p + 1]; ++c) {
    const int w = a.child_idx[c];
    if (w != v) x += a.msg[((size_t)w * a.n_units + uu) * S + r];
  }
  sw[threadIdx.x] = x;
  __syncthreads();
  double m = sw[gb];
  for (int k = 1; k < S; ++k) m = fmax(m, sw[gb + k]);
  if (!(m > -INFINITY)) m = 0.0;
  __syncthreads();
  sw[threadIdx.x] = exp(x - m);
  __syncthreads();
  const double *Pc = a.P + (size_t)a.qb[(size_t)v * a.n_cats + a.unit_cat[uu]] * S * S + r;   // column r of P_v
  double arg = 0.0;
  for (int k = 0; k < S; ++k) arg = fma(sw[gb + k], Pc[(size_t)k * S], arg);
  if (act) a.U[((size_t)v * a.n_units + uu) * S + r] = log(arg < 0.0 ? 0.0 : arg) + m;
}

// One family's view for the accumulation (all families of a handle share the buffers)
struct EmFam {
  long long nu_base;   // sum over the earlier families of n_nodes x n_units: codes at nu_base, messages at nu_base S
  int node_base;       // parent / child_ptr (+ family index) / child_idx offset
  int unit_base;       // l_u offset
  int n_units, root;
};
struct EmSeg {
  int fam, v, u0, n;   // edge above node v of family fam, units u0 .. u0 + n - 1 (one rate category: units sorted by it)
};
struct EmAccArgs {
  int S;
  const int *task_seg;               // [n_tasks + 1] segments of each task
  const EmSeg *seg;
  const EmFam *fam;
  const int *parent, *child_ptr, *child_idx;
  const signed char *codes;          // [node][unit] per family
  const double *pi_root;
  const double *msg, *U, *ll;
  double *part;                      // [n_tasks][S][S]
};

// max over the 16 lanes of one lane row (same hi)
__device__ __forceinline__ double em_max16(double x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x = fmax(x, __shfl_xor(x, off, 64));
  return x;
}

// grid = tasks, one wave.  Lane (lo, hi): unit u0 + k + hi of the segment in step k, states lo + 16 i (i < 2) -- the A / B
// operand layout of v_mfma_f64_16x16x4 (A[row lo][k hi], B[k hi][col lo]), so X and s Y go into the MFMA from the lane that
// formed them.  Z tile (i, j) register r: row 16 i + hi + 4 r, column 16 j + lo.
constexpr int NT = 2;   // S <= 32: the 32 x 32 padded Z as 2 x 2 tiles
__global__ __launch_bounds__(64) void em_acc_kernel(EmAccArgs a) {
  const int S = a.S, lane = threadIdx.x, lo = lane & 15, hi = lane >> 4;
  d4 acc[NT][NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
  for (int sg = a.task_seg[blockIdx.x]; sg < a.task_seg[blockIdx.x + 1]; ++sg) {
    const EmSeg sgm = a.seg[sg];
    const EmFam F = a.fam[sgm.fam];
    const int *cptr = a.child_ptr + F.node_base + sgm.fam, *cidx = a.child_idx + F.node_base;
    const int v = sgm.v, p = a.parent[F.node_base + v];
    const int pc0 = cptr[p], pc1 = cptr[p + 1], vc0 = cptr[v], vc1 = cptr[v + 1];
    const double *msg = a.msg + (size_t)F.nu_base * S, *U = a.U + (size_t)F.nu_base * S;
    const signed char *codes = a.codes + F.nu_base;
    for (int k = 0; k < sgm.n; k += 4) {
      const bool valid = k + hi < sgm.n;
      const int u = sgm.u0 + (valid ? k + hi : 0);
      const int code = vc0 == vc1 ? codes[(size_t)v * F.n_units + u] : -1;
      // x = U_p (log pi_root at the root) + the siblings' messages, y = the children's messages (a leaf: log of its 0/1 vector);
      // the state loop innermost, so that the child loops are shared by the NT rows
      const double *urow = p == F.root ? nullptr : U + ((size_t)p * F.n_units + u) * S;
      double x[NT], y[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int s = lo + 16 * i;
        x[i] = s < S ? (urow ? urow[s] : log(a.pi_root[s])) : -INFINITY;
        y[i] = s < S && (code < 0 || code == s) ? 0.0 : -INFINITY;
      }
      for (int c = pc0; c < pc1; ++c) {
        const int w = cidx[c];
        if (w == v) continue;
        const double *mr = msg + ((size_t)w * F.n_units + u) * S;
#pragma unroll
        for (int i = 0; i < NT; ++i)
          if (lo + 16 * i < S) x[i] += mr[lo + 16 * i];
      }
      for (int c = vc0; c < vc1; ++c) {
        const double *mr = msg + ((size_t)cidx[c] * F.n_units + u) * S;
#pragma unroll
        for (int i = 0; i < NT; ++i)
          if (lo + 16 * i < S) y[i] += mr[lo + 16 * i];
      }
      double mx = x[0], my = y[0];
#pragma unroll
      for (int i = 1; i < NT; ++i) {
        mx = fmax(mx, x[i]);
        my = fmax(my, y[i]);
      }
      mx = em_max16(mx);
      my = em_max16(my);
      const bool ok = valid && mx > -INFINITY && my > -INFINITY;
      const double sc = ok ? exp(mx + my - a.ll[F.unit_base + u]) : 0.0;
      double A[NT], Bv[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        A[i] = ok ? exp(x[i] - mx) : 0.0;
        Bv[i] = ok ? sc * exp(y[i] - my) : 0.0;
      }
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = mfma_f64(A[i], Bv[j], acc[i][j]);
    }
  }
  double *out = a.part + (size_t)blockIdx.x * S * S;
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * i + hi + 4 * r, col = 16 * j + lo;
        if (row < S && col < S) out[(size_t)row * S + col] = acc[i][j][r];
      }
}

// grid = buckets, 256 threads: E_beta = P_beta o sum_{tasks of beta, in order} part
__global__ __launch_bounds__(256) void em_reduce_kernel(int S, const int *__restrict__ bucket_task, const double *__restrict__ part,
                                                        const double *__restrict__ P, double *__restrict__ E) {
  const int b = blockIdx.x, SS = S * S;
  const int t0 = bucket_task[b], t1 = bucket_task[b + 1];
  for (int e = threadIdx.x; e < SS; e += 256) {
    double z = 0.0;
    for (int t = t0; t < t1; ++t) z += part[(size_t)t * SS + e];
    E[(size_t)b * SS + e] = P[(size_t)b * SS + e] * z;
  }
}
