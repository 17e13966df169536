// Felsenstein's bootstrap on the device (include/cherrybank.h, cb_boot_nj): the all-pairs maximum-likelihood
// distances of n_rep site resamples of one alignment, written straight into the resident matrices the join kernels (nj.hip.h)
// read.  For a pair (i, j) the per-site term v[t][s] = sym[t][rate(s)][x_s][y_s] does not depend on the replicate, only the site
// multiplicities w_b[s] do: the whole likelihood curve of the pair for all replicates is one product
//
//     F[b][t] = sum_s w_b[s] v[t][s]                      (replicates x sites times sites x grid points, float64)
//
// and the reference's bisection (ble_pairwise_kernel's rule) replays on F[b][.]: one gather of v per pair, not one per pair and
// replicate.
//
//   boot_weights_kernel   one workgroup per replicate: draw j takes word j & 3 of philox4x32_10(counter = (j >> 2, b, 0, BOOT_TAG),
//                         key = the family's seed) and lands on site (word * L) >> 32 -- sup_weights_kernel's rule on a stream of
//                         its own, b the replicate's number in the CALL (a chunk starts at rep0).  An integer histogram in LDS over
//                         windows of BOOT_WINDOW sites; W[b][s] takes it as doubles in the caller's site order.
//   boot_pairwise_kernel  a workgroup of four waves owns BOOT_PT consecutive pairs x BOOT_RB replicates and takes the pairs in
//                         turn.  The grid points go in chunks of BOOT_TC; per chunk the sites go in slabs of BOOT_KT through LDS:
//                         sV[t][s] gathered from the symmetrised bank (a site not observed in both sequences, a site past L and a
//                         grid point past T are zero operands), sW[b][s] read along the sites (a replicate past the launch's
//                         last is a zero operand).  Wave w forms the 16 replicates 16 w .. of the four 16 x 16 tiles of the chunk
//                         with v_mfma_f64_16x16x4: k runs from site 0 up in steps of 4 whatever the launch holds, and there are
//                         no atomics, so F[b][t] of a pair does not depend on the other replicates, pairs or chunks.  The chunk's
//                         F goes to LDS (over the slabs), where one thread per replicate turns it into the bits
//                         F[t] > F[t + 1] -- all the bisection ever asks of the curve -- with the last value carried into the
//                         next chunk; after the last chunk the same thread replays the bisection on its bits and writes
//                         D[b][i][j] = D[b][j][i] = grid[index] (and the index).  The diagonal is the host's memset.
//
// LDS rows are BOOT_KT + 2 doubles long: the operand read of a 32-lane half takes rows i = 0 .. 15 at the columns k and k + 1;
// with 8-byte words on 32 banks, row stride 32 puts all sixteen rows on one bank (16-way), stride 33 puts (i, k + 1) on
// (i + 1, k) (2-way), stride 34 gives 2 i + k: thirty-two different banks.
#pragma once
#include "common.hip.h"
#include "philox.hip.h"

constexpr int BOOT_WINDOW = 16384;          // sites per histogram window (64 KiB of LDS)
constexpr uint32_t BOOT_TAG = 0x424F4F54u;  // the fourth counter word: this stream is nobody else's
constexpr int BOOT_KT = 32;                 // sites per LDS slab
constexpr int BOOT_LD = BOOT_KT + 2;        // doubles per slab row (above)
constexpr int BOOT_TC = 64;                 // grid points per chunk of the curve: four 16 x 16 tiles per wave
constexpr int BOOT_RB = 64;                 // replicates per workgroup: sixteen per wave
constexpr int BOOT_PT = 8;                  // pairs per workgroup
constexpr int BOOT_T_MAX = 1024;            // grid points at most (the bits of a curve live in LDS)

struct BootWeightArgs {
  int L, rep0;              // sites; the number of the launch's first replicate in the call
  uint32_t k0, k1;          // the family's seed, low and high word
  double *W;                // [replicates of the launch][L]
};

// grid = replicates of the launch, 256 threads
__global__ __launch_bounds__(256) void boot_weights_kernel(BootWeightArgs a) {
  __shared__ int hist[BOOT_WINDOW];
  const int L = a.L;
  const uint32_t b = (uint32_t)(a.rep0 + (int)blockIdx.x);
  const int n_quads = (L + 3) >> 2;
  double *row = a.W + (size_t)blockIdx.x * L;
  for (int s0 = 0; s0 < L; s0 += BOOT_WINDOW) {
    const int ns = min(BOOT_WINDOW, L - s0);
    for (int k = threadIdx.x; k < ns; k += 256) hist[k] = 0;
    __syncthreads();
    for (int q = threadIdx.x; q < n_quads; q += 256) {
      uint32_t x[4];
      sup_philox((uint32_t)q, b, 0u, BOOT_TAG, a.k0, a.k1, x);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int site = (int)(((unsigned long long)x[i] * (unsigned long long)L) >> 32) - s0;
        if (4 * q + i < L && site >= 0 && site < ns) atomicAdd(&hist[site], 1);
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < ns; k += 256) row[s0 + k] = (double)hist[k];
    __syncthreads();
  }
}

struct BootPairArgs {
  int S, T, R, n, L, n_rep;      // n_rep: the replicates of the launch
  long long n_pairs;             // n (n - 1) / 2
  const double *sym;             // [T][R][S][S]: logP[x][y] + logP[y][x]
  const double *grid;            // [T]
  const int8_t *seqs;            // [n][L]
  const int *site_to_rate;       // [L]
  const double *W;               // [n_rep][L]
  double *D;                     // [n_rep][n][n]
  int *index;                    // [n_rep][n][n] or null
};

// the first pair of row i of the upper triangle, rows in turn: pair p = row_start(i) + (j - i - 1)
__device__ __forceinline__ long long boot_row_start(long long i, long long n) { return i * (2 * n - i - 1) / 2; }

// grid = (tiles of BOOT_PT pairs, tiles of BOOT_RB replicates), 256 threads
__global__ __launch_bounds__(256) void boot_pairwise_kernel(BootPairArgs a) {
  __shared__ double slab[2 * 64 * BOOT_LD];                          // sV and sW; the chunk's F afterwards
  __shared__ unsigned long long bits[BOOT_T_MAX / 64][BOOT_RB];      // bit t of a replicate: F[t] > F[t + 1]
  static_assert(BOOT_RB * (BOOT_TC + 1) <= 2 * 64 * BOOT_LD, "the chunk's F fits over the slabs");
  double(*sV)[BOOT_LD] = reinterpret_cast<double(*)[BOOT_LD]>(slab);
  double(*sW)[BOOT_LD] = reinterpret_cast<double(*)[BOOT_LD]>(slab + 64 * BOOT_LD);
  double(*sF)[BOOT_TC + 1] = reinterpret_cast<double(*)[BOOT_TC + 1]>(slab);
  const int S = a.S, T = a.T, L = a.L, n = a.n;
  const size_t SS = (size_t)S * S, RSS = (size_t)a.R * SS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & (BOOT_KT - 1), row8 = tid / BOOT_KT;          // 8 rows of a slab per pass
  const int r0 = blockIdx.y * BOOT_RB;
  const long long p0 = (long long)blockIdx.x * BOOT_PT, p1 = min(p0 + BOOT_PT, a.n_pairs);
  // the first pair: the row by the root of row_start(i) = p, set right in integers
  int i = (int)((2.0 * n - 1.0 - sqrt((2.0 * n - 1.0) * (2.0 * n - 1.0) - 8.0 * (double)p0)) / 2.0);
  i = max(0, min(i, n - 2));
  while (i > 0 && boot_row_start(i, n) > p0) --i;
  while (i < n - 2 && boot_row_start(i + 1, n) <= p0) ++i;
  int j = i + 1 + (int)(p0 - boot_row_start(i, n));
  for (long long p = p0; p < p1; ++p) {                              // (uniform: every thread meets every barrier)
    const int8_t *x = a.seqs + (size_t)i * L, *y = a.seqs + (size_t)j * L;
    double last = 0.0;                                               // F[t0 - 1] of the thread's replicate
    for (int t0 = 0, c = 0; t0 < T; t0 += BOOT_TC, ++c) {
      d4 acc[BOOT_TC / 16];
#pragma unroll
      for (int tt = 0; tt < BOOT_TC / 16; ++tt) acc[tt] = d4{0.0, 0.0, 0.0, 0.0};
      for (int k0 = 0; k0 < L; k0 += BOOT_KT) {
        const int s = k0 + col;
        long long o = -1;                                            // the site's entry in a grid point's block of the bank
        if (s < L) {
          const int xi = x[s], yi = y[s];
          if (xi >= 0 && yi >= 0) o = (long long)a.site_to_rate[s] * (long long)SS + xi * S + yi;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int row = row8 + 8 * q, t = t0 + row, r = r0 + row;
          sV[row][col] = (o >= 0 && t < T) ? a.sym[(size_t)t * RSS + (size_t)o] : 0.0;
          sW[row][col] = (s < L && r < a.n_rep) ? a.W[(size_t)r * L + s] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < BOOT_KT / 4; ++ks) {
          const int k = 4 * ks + (lane >> 4);
          const double w = sW[16 * wave + (lane & 15)][k];
#pragma unroll
          for (int tt = 0; tt < BOOT_TC / 16; ++tt)
            acc[tt] = mfma_f64(sV[16 * tt + (lane & 15)][k], w, acc[tt]);
        }
        __syncthreads();
      }
      // acc[tt] register q of lane l: grid point 16 tt + (l >> 4) + 4 q, replicate 16 wave + (l & 15)
#pragma unroll
      for (int tt = 0; tt < BOOT_TC / 16; ++tt)
#pragma unroll
        for (int q = 0; q < 4; ++q) sF[16 * wave + (lane & 15)][16 * tt + (lane >> 4) + 4 * q] = acc[tt][q];
      __syncthreads();
      if (tid < BOOT_RB) {                                           // one thread per replicate: the chunk's bits
        double prev = sF[tid][0];
        if (c > 0 && last > prev) bits[c - 1][tid] |= 1ull << 63;
        unsigned long long word = 0;
#pragma unroll 8
        for (int b = 0; b < BOOT_TC - 1; ++b) {
          const double next = sF[tid][b + 1];
          word |= (unsigned long long)(prev > next) << b;
          prev = next;
        }
        bits[c][tid] = word;
        last = prev;
      }
      __syncthreads();                                               // (the next slab overwrites F)
    }
    if (tid < BOOT_RB && r0 + tid < a.n_rep) {                       // the reference's bisection on the finished curve
      int low = 0, high = T - 1;
      while (low < high) {
        const int mid = low + (high - low) / 2;
        if ((bits[mid >> 6][tid] >> (mid & 63)) & 1ull) high = mid;  // a > b keeps the lower half
        else low = mid + 1;
      }
      const size_t base = (size_t)(r0 + tid) * n * n, ij = base + (size_t)i * n + j, ji = base + (size_t)j * n + i;
      const double d = a.grid[low];
      a.D[ij] = d;
      a.D[ji] = d;
      if (a.index) {
        a.index[ij] = low;
        a.index[ji] = low;
      }
    }
    if (++j == n) {
      ++i;
      j = i + 1;
    }
  }
}
