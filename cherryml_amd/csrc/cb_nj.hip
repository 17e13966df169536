// libcherrybank: neighbour joining on the device (kernels: nj.hip.h).  Stateless, like cb_ble_pairwise: every argument is
// validated on the host before any device work; the families go to the device in chunks of whole families, and per chunk the
// host enqueues three launches per join of its largest family without waiting in between.
#include "cb_internal.hip.h"
#include "nj.hip.h"
#include "nj_host.hip.h"

namespace {
constexpr size_t NJ_BYTES = (size_t)512 << 20;   // resident matrices of one chunk (test hook: CB_NJ_BYTES)

int nj_validate(int n_fam, const int *n, const double *D) {
  if (n_fam < 1) return fail(CB_EINVAL, "cb_nj_batch: n_fam = %d families (at least 1)", n_fam);
  for (int f = 0; f < n_fam; ++f) {
    if (n[f] < 2) return fail(CB_EINVAL, "cb_nj_batch: family %d: n = %d leaves (at least 2)", f, n[f]);
    if ((size_t)n[f] * (size_t)n[f] > (size_t)INT32_MAX)
      return fail(CB_EINVAL, "cb_nj_batch: family %d: n = %d leaves: the matrix passes 2^31 - 1 entries", f, n[f]);
  }
  const double *d = D;
  constexpr size_t TILE = 64;   // of the symmetry check: both a tile and its mirror image stay in cache
  for (int f = 0; f < n_fam; ++f) {
    const size_t nf = (size_t)n[f];
    for (size_t i = 0; i < nf; ++i)
      for (size_t j = 0; j < nf; ++j) {
        const double v = d[i * nf + j];
        if (!(v >= 0.0) || !std::isfinite(v))
          return fail(CB_EINVAL, "cb_nj_batch: family %d: D[%zu][%zu] = %g is negative or not finite", f, i, j, v);
        if (i == j && v != 0.0) return fail(CB_EINVAL, "cb_nj_batch: family %d: the diagonal entry D[%zu][%zu] = %g is not 0", f, i, j, v);
      }
    for (size_t i0 = 0; i0 < nf; i0 += TILE)
      for (size_t j0 = 0; j0 <= i0; j0 += TILE)
        for (size_t i = i0; i < std::min(i0 + TILE, nf); ++i)
          for (size_t j = j0; j < std::min(j0 + TILE, i); ++j)
            if (d[i * nf + j] != d[j * nf + i])
              return fail(CB_EINVAL, "cb_nj_batch: family %d: D[%zu][%zu] = %.17g but D[%zu][%zu] = %.17g (not symmetric)", f, i, j,
                          d[i * nf + j], j, i, d[j * nf + i]);
    d += nf * nf;
  }
  return CB_OK;
}

}  // namespace

int cb_nj_join_chunk(const NjBufs &b, int nf_c, int n_max, size_t joins, bool timed, double *ms_total, int *join_nodes,
                     double *join_len, int *final_nodes, double *final_D) {
  int rc;
  CbKernelTimer timer(timed);
  if ((rc = timer.begin(false)) != CB_OK) return rc;
  for (int t = 0; t < n_max - 3; ++t) {         // all iterations enqueued, no wait in between
    const int m = n_max - t;
    hipLaunchKernelGGL(nj_rowsum_kernel, dim3((unsigned)((m + NJ_WAVES - 1) / NJ_WAVES), (unsigned)nf_c), dim3(NJ_BLOCK), 0, 0, t,
                       (const NjFamily *)b.fams, (const double *)b.D, b.r);
    hipLaunchKernelGGL(nj_argmin_kernel, dim3((unsigned)nj_num_cands(m), (unsigned)nf_c), dim3(NJ_BLOCK), 0, 0, t,
                       (const NjFamily *)b.fams, (const double *)b.D, (const double *)b.r, (const int *)b.rank, b.cand);
    hipLaunchKernelGGL(nj_join_kernel, dim3((unsigned)nf_c), dim3(NJ_BLOCK), 0, 0, t, (const NjFamily *)b.fams, b.D,
                       (const double *)b.r, b.tmp, b.rank, b.node, (const NjCand *)b.cand, b.join_nodes, b.join_len,
                       b.final_nodes, b.final_D);
  }
  double ms = 0.0;
  if ((rc = timer.end(&ms)) != CB_OK) return rc;
  *ms_total += ms;
  HIP_TRY(hipGetLastError());
  if (joins) {
    HIP_TRY(hipMemcpy(join_nodes, b.join_nodes, joins * 2 * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(join_len, b.join_len, joins * 2 * sizeof(double), hipMemcpyDeviceToHost));
  }
  HIP_TRY(hipMemcpy(final_nodes, b.final_nodes, (size_t)nf_c * 3 * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(final_D, b.final_D, (size_t)nf_c * 9 * sizeof(double), hipMemcpyDeviceToHost));
  return CB_OK;
}

extern "C" int cb_nj_batch(int device, int n_fam, const int *n, const double *D, int *join_nodes, double *join_len,
                           int *final_nodes, double *final_D, double *kernel_ms) {
  if (!n || !D || !join_nodes || !join_len || !final_nodes || !final_D) return fail(CB_EINVAL, "cb_nj_batch: NULL argument");
  int rc = nj_validate(n_fam, n, D);
  if (rc != CB_OK) return rc;
  const int ndev = cb_device_count();
  if (ndev <= 0) return fail(CB_EHIP, "cb_nj_batch: no HIP device visible");
  if (device < 0 || device >= ndev) return fail(CB_EINVAL, "cb_nj_batch: device %d out of range", device);
  HIP_TRY(hipSetDevice(device));

  // chunks of whole families under the byte bound; a family alone above it runs alone
  const size_t bound = cb_hook_bytes("CB_NJ_BYTES", NJ_BYTES);
  std::vector<NjChunk> chunks;
  for (int f = 0; f < n_fam; ++f) {
    const size_t nf = (size_t)n[f], mat = nf * nf, joins = nf > 3 ? nf - 3 : 0;
    if (chunks.empty() || (chunks.back().mat + mat) * sizeof(double) > bound || chunks.back().f1 - chunks.back().f0 >= NJ_MAX_FAMILIES)
      chunks.push_back(NjChunk{f, f, 0, 0, 0});
    NjChunk &c = chunks.back();
    c.f1 = f + 1, c.mat += mat, c.vec += nf, c.joins += joins;
  }
  NjChunk cap{0, 0, 0, 0, 0};
  for (const NjChunk &c : chunks) {
    cap.f1 = std::max(cap.f1, c.f1 - c.f0);
    cap.mat = std::max(cap.mat, c.mat), cap.vec = std::max(cap.vec, c.vec), cap.joins = std::max(cap.joins, c.joins);
  }
  std::vector<NjFamily> fams((size_t)cap.f1);   // (host buffers the uploads read: before the device buffers)
  std::vector<int> iota(cap.vec);
  NjBufs b;
  if ((rc = b.alloc((size_t)cap.f1, cap.mat, cap.vec, std::max<size_t>(cap.joins, 1))) != CB_OK) return rc;

  double ms_total = 0.0;
  size_t mat0 = 0, join0 = 0;                   // where the chunk starts in D and in the join records
  for (const NjChunk &c : chunks) {
    const int nf_c = c.f1 - c.f0;
    int n_max = 0;
    size_t d0 = 0, v0 = 0, j0 = 0;
    for (int f = c.f0; f < c.f1; ++f) {
      const size_t nf = (size_t)n[f];
      fams[(size_t)(f - c.f0)] = NjFamily{n[f], (int)j0, d0, v0};
      for (size_t s = 0; s < nf; ++s) iota[v0 + s] = (int)s;
      d0 += nf * nf, v0 += nf, j0 += nf > 3 ? nf - 3 : 0;
      n_max = std::max(n_max, n[f]);
    }
    HIP_TRY(hipMemcpyAsync(b.fams, fams.data(), (size_t)nf_c * sizeof(NjFamily), hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(b.D, D + mat0, c.mat * sizeof(double), hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(b.rank, iota.data(), c.vec * sizeof(int), hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(b.node, iota.data(), c.vec * sizeof(int), hipMemcpyHostToDevice, 0));
    HIP_TRY(hipStreamSynchronize(0));           // (fams and iota are rewritten by the next chunk)
    if (n_max > 3 && (rc = cb_nj_join_chunk(b, nf_c, n_max, c.joins, kernel_ms != nullptr, &ms_total, join_nodes + join0 * 2,
                                            join_len + join0 * 2, final_nodes + (size_t)c.f0 * 3, final_D + (size_t)c.f0 * 9)) != CB_OK)
      return rc;
    // three or two leaves are not joined: the leaves themselves with their distances, unused slots -1 / 0
    size_t at = mat0;
    for (int f = c.f0; f < c.f1; ++f) {
      const int nf = n[f];
      if (nf <= 3)
        for (int a = 0; a < 3; ++a) {
          final_nodes[(size_t)f * 3 + a] = a < nf ? a : -1;
          for (int k = 0; k < 3; ++k) final_D[(size_t)f * 9 + a * 3 + k] = (a < nf && k < nf) ? D[at + (size_t)a * nf + k] : 0.0;
        }
      at += (size_t)nf * nf;
    }
    mat0 += c.mat, join0 += c.joins;
  }
  if (kernel_ms) *kernel_ms = ms_total;
  return CB_OK;
}
