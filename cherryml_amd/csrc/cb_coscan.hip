// libcherrybank: the co-evolution scan on a resident handle (coscan.hip.h; include/cherrybank.h, cb_coscan_*).
// The host layout (checks, buckets, pair order, tiles, offsets) is coscan_layout.h; here: the device.
#include "cb_internal.hip.h"
#include "common.hip.h"
#include "coscan.hip.h"

struct cb_coscan_s {
  int device = 0, S = 0, B = 0;
  std::vector<double> grid;
  double *dlogP1 = nullptr, *dlogP2 = nullptr;   // [B][S][S], [B][S^2][S^2]
  CbKernelTimer events{true};                   // owns the two events a call's timer borrows
};

extern "C" int cb_coscan_destroy(cb_coscan_s *h) {
  if (!h) return CB_OK;
  (void)hipSetDevice(h->device);
  if (h->dlogP1) (void)hipFree(h->dlogP1);
  if (h->dlogP2) (void)hipFree(h->dlogP2);
  delete h;
  return CB_OK;
}

// log expm(grid[b] Q) for every grid point into dlog [B][n][n], by the library's own expm on a counts-free handle (pi != NULL:
// the spectral path of a reversible Q, NULL: scaling and squaring), the log taken in place
static int coscan_log_bank(int device, int n, int B, const double *grid, const double *Q, const double *pi, double *dlog) {
  const size_t nn = (size_t)n * n;
  cb_handle hx = nullptr;
  const std::vector<double> t0(B, 0.0);
  int rc = cb_create(device, n, 1, B, CB_F64, t0.data(), nullptr, CB_EXPM_ONLY, &hx);
  if (rc == CB_OK) rc = cb_set_stream(hx, nullptr, 0);
  if (rc == CB_OK) rc = cb_internal_set_times(hx, grid, B, nullptr);
  if (rc == CB_OK) {
    CbDevBufs bufs;
    double *dQ = bufs.up(Q, nn, rc);
    double *dpi = pi ? bufs.up(pi, (size_t)n, rc) : nullptr;
    if (rc == CB_OK) rc = cb_internal_expm_bank(hx, dQ, dpi, CB_PTR_DEVICE | CB_NO_SYNC, dlog);
    if (rc == CB_OK) {
      const size_t tot = (size_t)B * nn;
      hipLaunchKernelGGL(coscan_log_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0, tot, dlog);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess)
        rc = fail(CB_EHIP, "cb_coscan_create: the log of the bank failed");
    }
  }
  if (hx) cb_destroy(hx);
  return rc;
}

extern "C" int cb_coscan_create(int device, int S, int B, const double *grid, const double *Q1, const double *pi1,
                                const double *Q2, const double *pi2, cb_coscan_s **out) {
  if (!grid || !Q1 || !Q2 || !out) return fail(CB_EINVAL, "cb_coscan_create: NULL argument");
  *out = nullptr;
  int rc = coscan_check_model(S, B, grid);
  if (rc != CB_OK) return rc;
  const int ndev = cb_device_count();
  if (ndev <= 0) return fail(CB_EHIP, "cb_coscan_create: no HIP device visible");
  if (device < 0 || device >= ndev) return fail(CB_EINVAL, "cb_coscan_create: device %d out of range", device);
  HIP_TRY(hipSetDevice(device));
  cb_coscan_s *h = new cb_coscan_s;
  h->device = device; h->S = S; h->B = B;
  h->grid.assign(grid, grid + B);
  const size_t S2 = (size_t)S * S;
  if (hipMalloc((void **)&h->dlogP1, (size_t)B * S2 * sizeof(double)) != hipSuccess ||
      hipMalloc((void **)&h->dlogP2, (size_t)B * S2 * S2 * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    cb_coscan_destroy(h);
    return fail(CB_ENOMEM, "cb_coscan_create: %zu bytes for the two log banks", (size_t)B * (S2 + S2 * S2) * sizeof(double));
  }
  rc = coscan_log_bank(device, S, B, grid, Q1, pi1, h->dlogP1);
  if (rc == CB_OK) rc = coscan_log_bank(device, (int)S2, B, grid, Q2, pi2, h->dlogP2);
  if (rc == CB_OK) rc = h->events.create();
  if (rc != CB_OK) {
    cb_coscan_destroy(h);
    return rc;
  }
  *out = h;
  return CB_OK;
}

extern "C" int cb_coscan_run(cb_coscan_s *h, int n_fam, const int *L, const int8_t *seqs, int64_t seqs_bytes,
                             const cb_count_pair *pairs, const int64_t *n_pairs, int symmetric, double *score, double *pair_ll,
                             double *indep_ll, int *n_used, double *kernel_ms) {
  if (!h) return fail(CB_EINVAL, "cb_coscan_run: NULL handle");
  if (!L || !n_pairs || !score || !pair_ll || !indep_ll || !n_used) return fail(CB_EINVAL, "cb_coscan_run: NULL argument");
  int64_t tot_pairs = 0;
  for (int f = 0; f < n_fam; ++f) tot_pairs += n_pairs[f] > 0 ? n_pairs[f] : 0;
  if ((tot_pairs > 0 && !pairs) || (seqs_bytes > 0 && !seqs)) return fail(CB_EINVAL, "cb_coscan_run: NULL argument");
  CoscanLayout lay;
  int rc = coscan_layout(h->S, h->B, h->grid.data(), n_fam, L, seqs, seqs_bytes, pairs, n_pairs, lay);
  if (rc != CB_OK) return rc;
  if (cb_test_hook("CB_COSCAN_INDEX_ORDER"))   // (profiles/tools/time_coscan.py: what the bucket order is worth)
    for (const CoscanFam &F : lay.fam)
      std::sort(lay.pairs.begin() + F.pair_off, lay.pairs.begin() + F.pair_off + F.n_kept,
                [](const CoscanSeqPair &x, const CoscanSeqPair &y) { return x.index < y.index; });
  HIP_TRY(hipSetDevice(h->device));
  CbDevBufs bufs;
  CoscanArgs a{};
  a.S = h->S;
  a.w = symmetric ? 0.25 : 0.5;
  a.logP1 = h->dlogP1;
  a.logP2 = h->dlogP2;
  a.seqs = bufs.up(seqs, (size_t)seqs_bytes, rc);
  a.fam = bufs.up(lay.fam.data(), lay.fam.size(), rc);
  a.pairs = bufs.up(lay.pairs.data(), lay.pairs.size(), rc);
  a.tiles = bufs.up(lay.tiles.data(), lay.tiles.size(), rc);
  double *dout = bufs.up<double>(nullptr, 3 * lay.n_out, rc);
  int *dused = bufs.up<int>(nullptr, lay.n_out, rc);
  if (rc != CB_OK) return rc;
  a.score = dout;
  a.pair_ll = dout + lay.n_out;
  a.indep_ll = dout + 2 * lay.n_out;
  a.n_used = dused;
  CbKernelTimer timer(kernel_ms != nullptr, h->events.ev0, h->events.ev1);
  if ((rc = timer.begin(true)) != CB_OK) return rc;
  const dim3 grid((unsigned)lay.tiles.size());
  if (symmetric) hipLaunchKernelGGL(coscan_kernel<true>, grid, dim3(256), 0, 0, a);
  else hipLaunchKernelGGL(coscan_kernel<false>, grid, dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  if ((rc = timer.end(kernel_ms)) != CB_OK) return rc;
  HIP_TRY(hipMemcpy(score, a.score, lay.n_out * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(pair_ll, a.pair_ll, lay.n_out * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(indep_ll, a.indep_ll, lay.n_out * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_used, a.n_used, lay.n_out * sizeof(int), hipMemcpyDeviceToHost));
  return CB_OK;
}
