// libcherrybank: Felsenstein's bootstrap on the device (kernels: boot.hip.h; the joins: nj.hip.h through nj_host.hip.h).
// Stateless, like cb_ble_pairwise and cb_nj_batch: every argument is validated on the host before any device work; the
// replicates go to the device in chunks of whole replicates, and per chunk the weights are drawn (or uploaded), the distances of
// all pairs and replicates are written into the resident matrices, and the joins run on them where they are.
#include "cb_internal.hip.h"
#include "boot.hip.h"
#include "nj_host.hip.h"

namespace {
constexpr size_t BOOT_BYTES = (size_t)512 << 20;   // resident matrices of one chunk (test hook: CB_BOOT_BYTES)

int boot_validate(int S, int T, int R, const double *logP, const double *grid, const int8_t *seqs, int n, int L,
                  const int *site_to_rate, int n_rep, const double *weights) {
  if (n < 2) return fail(CB_EINVAL, "cb_boot_nj: n = %d sequences (at least 2)", n);
  if (L < 1) return fail(CB_EINVAL, "cb_boot_nj: L = %d sites (at least 1)", L);
  if (S < 2 || S > 127) return fail(CB_EINVAL, "cb_boot_nj: S = %d states (2 to 127)", S);
  if (T < 1 || R < 1) return fail(CB_EINVAL, "cb_boot_nj: T = %d grid points, R = %d rate categories (at least 1)", T, R);
  if (T > BOOT_T_MAX) return fail(CB_EINVAL, "cb_boot_nj: T = %d grid points (at most %d)", T, BOOT_T_MAX);
  if ((size_t)R * S * S > (size_t)INT32_MAX) return fail(CB_EINVAL, "cb_boot_nj: R = %d rate categories: the bank offsets pass 2^31", R);
  if (n_rep < 1) return fail(CB_EINVAL, "cb_boot_nj: n_rep = %d replicates (at least 1)", n_rep);
  if ((size_t)n * (size_t)n > (size_t)INT32_MAX)
    return fail(CB_EINVAL, "cb_boot_nj: n = %d sequences: the matrix passes 2^31 - 1 entries", n);
  for (int t = 0; t < T; ++t)
    if (!std::isfinite(grid[t]) || !(grid[t] > 0.0) || (t > 0 && !(grid[t] > grid[t - 1])))
      return fail(CB_EINVAL, "cb_boot_nj: grid[%d] = %g: the grid must be finite, positive and increasing", t, grid[t]);
  for (int i = 0; i < n; ++i)
    for (int s = 0; s < L; ++s) {
      const int v = seqs[(size_t)i * L + s];
      if (v >= S || v < -1) return fail(CB_EINVAL, "cb_boot_nj: state code %d out of range (sequence %d, site %d)", v, i, s);
    }
  for (int s = 0; s < L; ++s)
    if (site_to_rate[s] < 0 || site_to_rate[s] >= R)
      return fail(CB_EINVAL, "cb_boot_nj: rate index %d out of range (site %d)", site_to_rate[s], s);
  const size_t n_bank = (size_t)T * R * S * S;
  for (size_t e = 0; e < n_bank; ++e)
    if (!std::isfinite(logP[e])) return fail(CB_EINVAL, "cb_boot_nj: logP entry %zu = %g is not finite", e, logP[e]);
  if (weights)
    for (int b = 0; b < n_rep; ++b)
      for (int s = 0; s < L; ++s) {
        const double w = weights[(size_t)b * L + s];
        if (!std::isfinite(w) || w < 0.0 || w != std::floor(w))
          return fail(CB_EINVAL, "cb_boot_nj: weights[%d][%d] = %g is negative, not finite or not an integer value", b, s, w);
      }
  return CB_OK;
}
}  // namespace

extern "C" int cb_boot_nj(int device, int S, int T, int R, const double *logP, const double *grid, const int8_t *seqs, int n,
                          int L, const int *site_to_rate, int n_rep, uint64_t seed, const double *weights, int *join_nodes,
                          double *join_len, int *final_nodes, double *final_D, int *index, double *weights_out,
                          double *kernel_ms) {
  if (!logP || !grid || !seqs || !site_to_rate || !join_nodes || !join_len || !final_nodes || !final_D)
    return fail(CB_EINVAL, "cb_boot_nj: NULL argument");
  int rc = boot_validate(S, T, R, logP, grid, seqs, n, L, site_to_rate, n_rep, weights);
  if (rc != CB_OK) return rc;
  const int ndev = cb_device_count();
  if (ndev <= 0) return fail(CB_EHIP, "cb_boot_nj: no HIP device visible");
  if (device < 0 || device >= ndev) return fail(CB_EINVAL, "cb_boot_nj: device %d out of range", device);
  HIP_TRY(hipSetDevice(device));

  // the symmetrised bank, sym[t][r][x][y] = logP[t][r][x][y] + logP[t][r][y][x]: ble_symmetrise_kernel's sum, bit for bit
  const size_t SS = (size_t)S * S, n_mats = (size_t)T * R;
  std::vector<double> sym(n_mats * SS);
  for (size_t m = 0; m < n_mats; ++m)
    for (int x = 0; x < S; ++x)
      for (int y = 0; y < S; ++y) sym[m * SS + (size_t)x * S + y] = logP[m * SS + (size_t)x * S + y] + logP[m * SS + (size_t)y * S + x];

  // chunks of whole replicates under the byte bound; a replicate alone above it runs alone
  const size_t nn = (size_t)n, mat = nn * nn, joins = nn > 3 ? nn - 3 : 0;
  const size_t bound = cb_hook_bytes("CB_BOOT_BYTES", BOOT_BYTES);
  const int per = (int)std::min<size_t>(std::max<size_t>(bound / (mat * sizeof(double)), 1), (size_t)NJ_MAX_FAMILIES);
  const int cap = std::min(per, n_rep);
  std::vector<NjFamily> fams((size_t)cap);         // (host buffers the uploads read: before the device buffers)
  std::vector<int> iota((size_t)cap * nn);
  for (int f = 0; f < cap; ++f) {
    fams[(size_t)f] = NjFamily{n, (int)((size_t)f * joins), (size_t)f * mat, (size_t)f * nn};
    for (size_t s = 0; s < nn; ++s) iota[(size_t)f * nn + s] = (int)s;
  }
  std::vector<double> small_D(n <= 3 ? (size_t)cap * mat : 0);
  NjBufs b;
  if ((rc = b.alloc((size_t)cap, (size_t)cap * mat, (size_t)cap * nn, std::max<size_t>((size_t)cap * joins, 1))) != CB_OK) return rc;
  const double *d_sym = b.d.up(sym.data(), sym.size(), rc), *d_grid = b.d.up(grid, (size_t)T, rc);
  const int8_t *d_seqs = b.d.up(seqs, nn * (size_t)L, rc);
  const int *d_s2r = b.d.up(site_to_rate, (size_t)L, rc);
  double *d_W = b.d.up<double>(nullptr, (size_t)cap * L, rc);
  int *d_index = index ? b.d.up<int>(nullptr, (size_t)cap * mat, rc) : nullptr;
  if (rc != CB_OK) return rc;
  HIP_TRY(hipMemcpyAsync(b.fams, fams.data(), fams.size() * sizeof(NjFamily), hipMemcpyHostToDevice, 0));

  const long long n_pairs = (long long)n * (n - 1) / 2;
  const bool timed = kernel_ms != nullptr;
  double ms_w = 0.0, ms_d = 0.0, ms_j = 0.0;
  for (int f0 = 0; f0 < n_rep; f0 += per) {
    const int nf = std::min(per, n_rep - f0);
    const size_t n_w = (size_t)nf * L, n_mat = (size_t)nf * mat;
    double ms = 0.0;
    if (weights) {
      HIP_TRY(hipMemcpyAsync(d_W, weights + (size_t)f0 * L, n_w * sizeof(double), hipMemcpyHostToDevice, 0));
    } else {
      CbKernelTimer timer(timed);
      if ((rc = timer.begin(false)) != CB_OK) return rc;
      hipLaunchKernelGGL(boot_weights_kernel, dim3((unsigned)nf), dim3(256), 0, 0,
                         BootWeightArgs{L, f0, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), d_W});
      if ((rc = timer.end(&ms)) != CB_OK) return rc;
      ms_w += ms;
    }
    HIP_TRY(hipMemsetAsync(b.D, 0, n_mat * sizeof(double), 0));                       // the diagonals
    if (d_index) HIP_TRY(hipMemsetAsync(d_index, 0xFF, n_mat * sizeof(int), 0));      // -1 there
    HIP_TRY(hipMemcpyAsync(b.rank, iota.data(), (size_t)nf * nn * sizeof(int), hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(b.node, iota.data(), (size_t)nf * nn * sizeof(int), hipMemcpyHostToDevice, 0));
    {
      CbKernelTimer timer(timed);
      if ((rc = timer.begin(false)) != CB_OK) return rc;
      const dim3 tiles((unsigned)((n_pairs + BOOT_PT - 1) / BOOT_PT), (unsigned)((nf + BOOT_RB - 1) / BOOT_RB));
      hipLaunchKernelGGL(boot_pairwise_kernel, tiles, dim3(256), 0, 0,
                         BootPairArgs{S, T, R, n, L, nf, n_pairs, d_sym, d_grid, d_seqs, d_s2r, (const double *)d_W, b.D, d_index});
      if ((rc = timer.end(&ms)) != CB_OK) return rc;
      ms_d += timed ? ms : 0.0;
    }
    HIP_TRY(hipGetLastError());
    if (weights_out) HIP_TRY(hipMemcpyAsync(weights_out + (size_t)f0 * L, d_W, n_w * sizeof(double), hipMemcpyDeviceToHost, 0));
    if (index) HIP_TRY(hipMemcpyAsync(index + (size_t)f0 * mat, d_index, n_mat * sizeof(int), hipMemcpyDeviceToHost, 0));
    if (n > 3) {
      if ((rc = cb_nj_join_chunk(b, nf, n, (size_t)nf * joins, timed, &ms_j, join_nodes + (size_t)f0 * joins * 2,
                                 join_len + (size_t)f0 * joins * 2, final_nodes + (size_t)f0 * 3, final_D + (size_t)f0 * 9)) != CB_OK)
        return rc;
    } else {   // three or two leaves are not joined: the leaves themselves with their distances, unused slots -1 / 0
      HIP_TRY(hipMemcpy(small_D.data(), b.D, n_mat * sizeof(double), hipMemcpyDeviceToHost));
      for (int f = 0; f < nf; ++f)
        for (int a = 0; a < 3; ++a) {
          final_nodes[(size_t)(f0 + f) * 3 + a] = a < n ? a : -1;
          for (int k = 0; k < 3; ++k)
            final_D[(size_t)(f0 + f) * 9 + a * 3 + k] = (a < n && k < n) ? small_D[(size_t)f * mat + (size_t)a * n + k] : 0.0;
        }
    }
    HIP_TRY(hipStreamSynchronize(0));   // (the copies into the caller's arrays are done; the next chunk rewrites the buffers)
  }
  if (kernel_ms) kernel_ms[0] = ms_w, kernel_ms[1] = ms_d, kernel_ms[2] = ms_j;
  return CB_OK;
}
