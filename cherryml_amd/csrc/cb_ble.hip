// libcherrybank: FastCherries branch lengths / site rates.
// The host arithmetic (priors, initial bins, transposes, size checks, batch offsets) is ble_layout.h; here: the device.
#include "cb_internal.hip.h"
#include "common.hip.h"
#include "ble.hip.h"
#include "ble_layout.h"

// ----------------------------------------------------------------- FastCherries BLE (8f #3)
extern "C" int cb_ble_log_bank(int device, int S, int T, int R, const double *Q, const double *pi,
                               const double *grid, const double *rates, double *logP) {
  if (!Q || !grid || !rates || !logP) return fail(CB_EINVAL, "cb_ble_log_bank: NULL argument");
  if (S < 2 || T < 1 || R < 1) return fail(CB_EINVAL, "cb_ble_log_bank: bad sizes");
  const size_t nb = (size_t)T * R, SS = (size_t)S * S;
  std::vector<double> tt(nb);
  for (int t = 0; t < T; ++t)
    for (int r = 0; r < R; ++r) tt[(size_t)t * R + r] = grid[t] * rates[r];   // as io_helpers.cpp:161
  cb_handle h = nullptr;
  // a counts-free handle: the bank alone (with dummy counts the handle staged 8 MB and ran the count preparation -- 1.2 ms of
  // kernels for nothing, more than the thirteen bisection passes of a family)
  int rc = cb_create(device, S, 1, (int)nb, CB_F64, tt.data(), nullptr, CB_EXPM_ONLY, &h);
  if (rc != CB_OK) return rc;
  rc = cb_expm_bank(h, Q, pi, 0, logP);
  cb_destroy(h);
  if (rc != CB_OK) return rc;
  for (size_t i = 0; i < nb * SS; ++i) logP[i] = std::log(logP[i]);
  return CB_OK;
}

namespace {
std::vector<int8_t> ble_transposed(const int8_t *c, int n, int L) {
  std::vector<int8_t> t((size_t)n * L);
  ble_transpose(c, n, L, t.data());
  return t;
}
// the one device check of every entry; `who` heads the refusal
int ble_device(const char *who, int device) {
  const int ndev = cb_device_count();
  if (ndev <= 0) return fail(CB_EHIP, "%s: no HIP device visible", who);
  if (device < 0 || device >= ndev) return fail(CB_EINVAL, "%s: device %d out of range", who, device);
  return CB_OK;
}
// sizes, then the device, then the codes
int ble_check(int device, int S, int T, int R, int n, int L, const int8_t *cx, const int8_t *cy) {
  int rc = ble_check_sizes(S, T, R, n, L);
  if (rc == CB_OK) rc = ble_device("ble", device);
  return rc == CB_OK ? ble_check_codes(S, n, L, cx, cy) : rc;
}

// ---- the coordinate ascent (branch_length_estimation.cpp:146-241), for every entry that runs one -----------------------------
struct BleBankView {
  int S, T, R;
  const double *logP, *priors;
};
// one family on the device; l0 holds its lengths when the ascent returns (l1: the other buffer)
struct BleFamilyView {
  int n, L;
  const int8_t *x, *y, *xT, *yT;
  int *s2r, *l0, *l1;
};
void ble_launch_branch_lengths(const BleBankView &b, const BleFamilyView &f, const int *previous, int *out, int *flag) {
  hipLaunchKernelGGL(ble_branch_lengths_kernel, dim3((f.n + 3) / 4), dim3(256), 0, 0, b.S, b.T, b.R, f.n, f.L, b.logP, f.x, f.y,
                     (const int *)f.s2r, previous, out, flag);
}
// The families in lockstep: the first branch-length pass, then per round a memset of the flag words, two launches per
// still-moving family and ONE blocking read-back of all the flags.  dflag [n_fam] on the device (a family's word is set when its
// lengths moved), moving [n_fam] on the host (scratch), iters [n_fam] out.  A converged family is a fixed point and is left alone.
int ble_ascent(const BleBankView &b, BleFamilyView *fam, int n_fam, int max_iters, int *dflag, int *moving, int *iters) {
  for (int f = 0; f < n_fam; ++f) {
    ble_launch_branch_lengths(b, fam[f], nullptr, fam[f].l0, nullptr);
    moving[f] = 1;
    iters[f] = 0;
  }
  bool any = true;
  for (int round = 0; round < max_iters && any; ++round) {
    HIP_TRY(hipMemsetAsync(dflag, 0, n_fam * sizeof(int), 0));
    for (int f = 0; f < n_fam; ++f) {
      if (!moving[f]) continue;
      BleFamilyView &F = fam[f];
      ble_launch_site_rates(b.S, b.T, b.R, F.n, F.L, b.logP, F.xT, F.yT, (const int *)F.l0, b.priors, F.s2r);
      ble_launch_branch_lengths(b, F, F.l0, F.l1, dflag + f);
      std::swap(F.l0, F.l1);
      ++iters[f];
    }
    HIP_TRY(hipMemcpy(moving, dflag, n_fam * sizeof(int), hipMemcpyDeviceToHost));   // (a family left alone reads 0 again)
    any = std::any_of(moving, moving + n_fam, [](int m) { return m != 0; });
  }
  return CB_OK;
}
}  // namespace

extern "C" int cb_ble_branch_lengths(int device, int S, int T, int R, const double *logP, const int8_t *cx,
                                     const int8_t *cy, int n, int L, const int *site_to_rate, int *lengths_index) {
  if (!logP || !cx || !cy || !site_to_rate || !lengths_index) return fail(CB_EINVAL, "cb_ble_branch_lengths: NULL argument");
  int rc = ble_check(device, S, T, R, n, L, cx, cy);
  if (rc != CB_OK) return rc;
  for (int i = 0; i < L; ++i)
    if (site_to_rate[i] < 0 || site_to_rate[i] >= R) return fail(CB_EINVAL, "cb_ble_branch_lengths: rate index out of range");
  HIP_TRY(hipSetDevice(device));
  CbDevBufs d;
  const double *dP = d.up(logP, (size_t)T * R * S * S, rc);
  const int8_t *dx = d.up(cx, (size_t)n * L, rc), *dy = d.up(cy, (size_t)n * L, rc);
  const int *ds = d.up(site_to_rate, L, rc);
  int *dout = d.up<int>(nullptr, n, rc);
  if (rc != CB_OK) return rc;
  hipLaunchKernelGGL(ble_branch_lengths_kernel, dim3((n + 3) / 4), dim3(256), 0, 0, S, T, R, n, L, dP, dx, dy, ds,
                     (const int *)nullptr, dout, (int *)nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(lengths_index, dout, n * sizeof(int), hipMemcpyDeviceToHost));
  return CB_OK;
}

// get_branch_lengths (:60-103) for all pairs of one family's sequences: the distance pass of neighbour joining.  Everything is
// validated on the host before any device work; the device holds the bank and its symmetrised copy, seqs [n][L], the rate
// indices and index [n][n].
extern "C" int cb_ble_pairwise(int device, int S, int T, int R, const double *logP, const int8_t *seqs, int n, int L,
                               const int *site_to_rate, int *index, double *kernel_ms) {
  if (!logP || !seqs || !site_to_rate || !index) return fail(CB_EINVAL, "cb_ble_pairwise: NULL argument");
  if (n < 2) return fail(CB_EINVAL, "cb_ble_pairwise: n = %d sequences (at least 2)", n);
  if (L < 1) return fail(CB_EINVAL, "cb_ble_pairwise: L = %d sites (at least 1)", L);
  if (S < 2 || S > 127) return fail(CB_EINVAL, "cb_ble_pairwise: S = %d states (2 to 127)", S);
  if (T < 1 || R < 1) return fail(CB_EINVAL, "cb_ble_pairwise: T = %d grid points, R = %d rate categories (at least 1)", T, R);
  if ((size_t)R * S * S > (size_t)INT32_MAX) return fail(CB_EINVAL, "cb_ble_pairwise: R = %d rate categories: the bank offsets pass 2^31", R);
  const int nb = (n + BLE_PW_TILE - 1) / BLE_PW_TILE;
  if ((nb + 1) / 2 > 65535) return fail(CB_EINVAL, "cb_ble_pairwise: n = %d sequences are more than one launch takes", n);
  for (int i = 0; i < n; ++i)
    for (int s = 0; s < L; ++s) {
      const int v = seqs[(size_t)i * L + s];
      if (v >= S || v < -1) return fail(CB_EINVAL, "cb_ble_pairwise: state code %d out of range (sequence %d, site %d)", v, i, s);
    }
  for (int s = 0; s < L; ++s)
    if (site_to_rate[s] < 0 || site_to_rate[s] >= R)
      return fail(CB_EINVAL, "cb_ble_pairwise: rate index %d out of range (site %d)", site_to_rate[s], s);
  int rc = ble_device("cb_ble_pairwise", device);
  if (rc != CB_OK) return rc;
  HIP_TRY(hipSetDevice(device));
  CbDevBufs d;
  const double *dP = d.up(logP, (size_t)T * R * S * S, rc);
  const int8_t *dq = d.up(seqs, (size_t)n * L, rc);
  const int *ds = d.up(site_to_rate, L, rc);
  int *dout = d.up<int>(nullptr, (size_t)n * n, rc);
  const size_t n_bank = (size_t)T * R * S * S;
  double *dsym = d.up<double>(nullptr, n_bank, rc);
  if (rc != CB_OK) return rc;
  CbKernelTimer timer(kernel_ms != nullptr);
  if ((rc = timer.begin(true)) != CB_OK) return rc;
  hipLaunchKernelGGL(ble_symmetrise_kernel, dim3((unsigned)((n_bank + 255) / 256)), dim3(256), 0, 0, S, (size_t)T * R, dP, dsym);
  hipLaunchKernelGGL(ble_pairwise_kernel, dim3(nb + 1, (nb + 1) / 2), dim3(256), 0, 0, S, T, R, n, L, nb, (const double *)dsym, dq, ds,
                     dout);
  if ((rc = timer.end(kernel_ms)) != CB_OK) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(index, dout, (size_t)n * n * sizeof(int), hipMemcpyDeviceToHost));
  return CB_OK;
}

extern "C" int cb_ble_site_rates(int device, int S, int T, int R, const double *logP, const int8_t *cx,
                                 const int8_t *cy, int n, int L, const int *lengths_index, const double *priors,
                                 int *rate_index) {
  if (!logP || !cx || !cy || !lengths_index || !priors || !rate_index) return fail(CB_EINVAL, "cb_ble_site_rates: NULL argument");
  int rc = ble_check(device, S, T, R, n, L, cx, cy);
  if (rc != CB_OK) return rc;
  for (int i = 0; i < n; ++i)
    if (lengths_index[i] < 0 || lengths_index[i] >= T) return fail(CB_EINVAL, "cb_ble_site_rates: length index out of range");
  HIP_TRY(hipSetDevice(device));
  const std::vector<int8_t> xT = ble_transposed(cx, n, L), yT = ble_transposed(cy, n, L);
  CbDevBufs d;
  const double *dP = d.up(logP, (size_t)T * R * S * S, rc), *dpr = d.up(priors, R, rc);
  const int8_t *dxT = d.up(xT.data(), (size_t)n * L, rc), *dyT = d.up(yT.data(), (size_t)n * L, rc);
  const int *dl = d.up(lengths_index, n, rc);
  int *dout = d.up<int>(nullptr, L, rc);
  if (rc != CB_OK) return rc;
  HIP_TRY(hipStreamSynchronize(0));  // xT / yT are locals
  ble_launch_site_rates(S, T, R, n, L, dP, dxT, dyT, dl, dpr, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(rate_index, dout, L * sizeof(int), hipMemcpyDeviceToHost));
  return CB_OK;
}

extern "C" int cb_ble(int device, int S, int T, int R, const double *logP, const int8_t *cx, const int8_t *cy, int n,
                      int L, const int8_t *all_seqs, int n_seqs, const double *rates, const double *weights,
                      int max_iters, int *lengths_index, int *rate_index, int *iterations, double *kernel_ms) {
  if (!logP || !cx || !cy || !all_seqs || !rates || !weights || !lengths_index || !rate_index)
    return fail(CB_EINVAL, "cb_ble: NULL argument");
  int rc = ble_check(device, S, T, R, n, L, cx, cy);
  if (rc != CB_OK) return rc;
  if (n_seqs < 1 || max_iters < 0) return fail(CB_EINVAL, "cb_ble: bad sizes");
  std::vector<int> s2r(L, 0);
  if ((rc = ble_initial_bins(all_seqs, n_seqs, L, S, R, weights, s2r.data())) != CB_OK) return rc;
  const std::vector<double> priors = ble_priors(rates, R);
  const std::vector<int8_t> xT = ble_transposed(cx, n, L), yT = ble_transposed(cy, n, L);
  HIP_TRY(hipSetDevice(device));
  CbDevBufs d;   // (after every vector it uploads)
  const size_t nc = (size_t)n * L;   // (braces: the uploads in the order written)
  const BleBankView bank{S, T, R, d.up(logP, (size_t)T * R * S * S, rc), d.up(priors.data(), R, rc)};
  BleFamilyView fam{n, L, d.up(cx, nc, rc), d.up(cy, nc, rc), d.up(xT.data(), nc, rc), d.up(yT.data(), nc, rc),
                    d.up(s2r.data(), L, rc), d.up<int>(nullptr, n, rc), d.up<int>(nullptr, n, rc)};
  int *dflag = d.up<int>(nullptr, 1, rc);
  if (rc != CB_OK) return rc;
  CbKernelTimer timer(kernel_ms != nullptr);
  int moving = 0, iters = 0;
  if ((rc = timer.begin(true)) != CB_OK || (rc = ble_ascent(bank, &fam, 1, max_iters, dflag, &moving, &iters)) != CB_OK ||
      (rc = timer.end(kernel_ms)) != CB_OK)
    return rc;
  if (iterations) *iterations = iters;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(lengths_index, fam.l0, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rate_index, fam.s2r, L * sizeof(int), hipMemcpyDeviceToHost));
  return CB_OK;
}

// Many families in one call (the reference maps families over a process pool, utils.py:59-67): the
// log-transition bank is uploaded ONCE, all sequences in one transfer, and the coordinate ascents run
// in lockstep -- per round two launches per still-moving family and ONE read-back of all the
// convergence flags (cb_ble: a synchronising read-back per family per iteration, and 8 MB of bank per
// family).  A converged family is a fixed point of the ascent, so results are those of cb_ble.
extern "C" int cb_ble_batch(int device, int S, int T, int R, const double *logP, int n_fam, const int *n,
                            const int *L, const int8_t *cx, const int8_t *cy, const int8_t *all_seqs,
                            const int *n_seqs, const double *rates, const double *weights, int max_iters,
                            int *lengths_index, int *rate_index, int *iterations, double *kernel_ms) {
  if (!logP || !n || !L || !cx || !cy || !all_seqs || !n_seqs || !rates || !weights || !lengths_index || !rate_index)
    return fail(CB_EINVAL, "cb_ble_batch: NULL argument");
  if (n_fam < 1 || max_iters < 0) return fail(CB_EINVAL, "cb_ble_batch: bad sizes");
  BleBatchOffsets o;
  int rc = ble_batch_offsets(n_fam, n, L, n_seqs, o);
  // (every n[f], L[f] is at least 1: the rest of ble_check's sizes and the device are the same for all the families)
  if (rc == CB_OK) rc = ble_check_sizes(S, T, R, 1, 1);
  if (rc == CB_OK) rc = ble_device("ble", device);
  if (rc != CB_OK) return rc;
  const size_t nc = o.off_c[n_fam], nn = o.off_n[n_fam], nL = o.off_L[n_fam];
  std::vector<int> s2r(nL, 0);
  std::vector<int8_t> xT(nc), yT(nc);
  for (int f = 0; f < n_fam; ++f) {
    const size_t oc = o.off_c[f];
    if ((rc = ble_check_codes(S, n[f], L[f], cx + oc, cy + oc)) != CB_OK) return rc;
    if ((rc = ble_initial_bins(all_seqs + o.off_s[f], n_seqs[f], L[f], S, R, weights, s2r.data() + o.off_L[f])) != CB_OK) return rc;
    ble_transpose(cx + oc, n[f], L[f], xT.data() + oc);
    ble_transpose(cy + oc, n[f], L[f], yT.data() + oc);
  }
  const std::vector<double> priors = ble_priors(rates, R);
  HIP_TRY(hipSetDevice(device));
  CbDevBufs d;   // (after every vector it uploads)
  const BleBankView bank{S, T, R, d.up(logP, (size_t)T * R * S * S, rc), d.up(priors.data(), R, rc)};
  const int8_t *dx = d.up(cx, nc, rc), *dy = d.up(cy, nc, rc);
  const int8_t *dxT = d.up(xT.data(), nc, rc), *dyT = d.up(yT.data(), nc, rc);
  int *ds = d.up(s2r.data(), nL, rc);
  int *dl0 = d.up<int>(nullptr, nn, rc), *dl1 = d.up<int>(nullptr, nn, rc);
  int *dflag = d.up<int>(nullptr, n_fam, rc);
  if (rc != CB_OK) return rc;
  std::vector<BleFamilyView> fam(n_fam);
  for (int f = 0; f < n_fam; ++f) {
    const size_t oc = o.off_c[f];
    fam[f] = {n[f], L[f], dx + oc, dy + oc, dxT + oc, dyT + oc, ds + o.off_L[f], dl0 + o.off_n[f], dl1 + o.off_n[f]};
  }
  std::vector<int> moving(n_fam), iters(n_fam);
  CbKernelTimer timer(kernel_ms != nullptr);
  if ((rc = timer.begin(true)) != CB_OK ||
      (rc = ble_ascent(bank, fam.data(), n_fam, max_iters, dflag, moving.data(), iters.data())) != CB_OK ||
      (rc = timer.end(kernel_ms)) != CB_OK)
    return rc;
  HIP_TRY(hipGetLastError());
  for (int f = 0; f < n_fam; ++f) {
    HIP_TRY(hipMemcpyAsync(lengths_index + o.off_n[f], fam[f].l0, n[f] * sizeof(int), hipMemcpyDeviceToHost, 0));
    if (iterations) iterations[f] = iters[f];
  }
  HIP_TRY(hipMemcpyAsync(rate_index, ds, nL * sizeof(int), hipMemcpyDeviceToHost, 0));
  HIP_TRY(hipStreamSynchronize(0));
  return CB_OK;
}

// ---- the device-resident entry (round 6; VERDICT r5 "missing 3") ------------------------------------------------------------
// cb_ble pays, per family, for 8 MB of bank upload, ten device allocations and three passes over every sequence byte on the
// host (range check, two transposes, the site statistics): 15 ms per call around 1 ms of kernels.  The reference computes the
// bank once per rate matrix and then calls ble() per family (FastCherries main.cpp: read_rate_compute_log_transition_matrices, then
// the loop over families) -- so does this handle: the bank lives on the device, the workspace is kept between calls, and the
// per-call host work is one sort of L integers.
struct cb_ble_bank_s {
  int device = 0, S = 0, T = 0, R = 0;
  double *logP = nullptr, *priors = nullptr;
  // workspace, grown on demand
  size_t cap_c = 0, cap_s = 0, cap_n = 0, cap_L = 0;
  int8_t *x = nullptr, *y = nullptr, *xT = nullptr, *yT = nullptr, *seqs = nullptr;
  int *s2r = nullptr, *l0 = nullptr, *l1 = nullptr, *flags = nullptr;
  long long *totals = nullptr;
  CbKernelTimer events{true};   // owns the two events a call's timer borrows
  // host ends of a call's asynchronous copies: here, not locals of the call, so that they outlive the copies on every return path
  std::vector<long long> h_totals;   // [cap_L], like h_s2r
  std::vector<int> h_s2r;
  int h_bad = 0;
};

static void ble_bank_free_ws(cb_ble_bank_s *b) {
  for (void *p : {(void *)b->x, (void *)b->y, (void *)b->xT, (void *)b->yT, (void *)b->seqs, (void *)b->s2r, (void *)b->l0, (void *)b->l1,
                  (void *)b->totals})
    if (p) (void)hipFree(p);
  b->x = b->y = b->xT = b->yT = b->seqs = nullptr;
  b->s2r = b->l0 = b->l1 = nullptr;
  b->totals = nullptr;
  b->cap_c = b->cap_s = b->cap_n = b->cap_L = 0;
}

extern "C" int cb_ble_bank_destroy(cb_ble_bank_s *b) {
  if (!b) return CB_OK;
  (void)hipSetDevice(b->device);
  ble_bank_free_ws(b);
  if (b->logP) (void)hipFree(b->logP);
  if (b->priors) (void)hipFree(b->priors);
  if (b->flags) (void)hipFree(b->flags);
  delete b;   // (and its events)
  return CB_OK;
}

extern "C" int cb_ble_bank_create(int device, int S, int T, int R, const double *logP, const double *rates, cb_ble_bank_s **out) {
  if (!logP || !rates || !out) return fail(CB_EINVAL, "cb_ble_bank_create: NULL argument");
  if (S < 2 || S > 127 || T < 1 || R < 1) return fail(CB_EINVAL, "cb_ble_bank_create: bad sizes");
  const int rc = ble_device("cb_ble_bank_create", device);
  if (rc != CB_OK) return rc;
  HIP_TRY(hipSetDevice(device));
  cb_ble_bank_s *b = new cb_ble_bank_s;
  b->device = device; b->S = S; b->T = T; b->R = R;
  const std::vector<double> priors = ble_priors(rates, R);
  const size_t nb = (size_t)T * R * S * S;
  bool ok = hipMalloc((void **)&b->logP, nb * sizeof(double)) == hipSuccess && hipMalloc((void **)&b->priors, R * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&b->flags, 4 * sizeof(int)) == hipSuccess && b->events.create() == CB_OK;
  ok = ok && hipMemcpy(b->logP, logP, nb * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(b->priors, priors.data(), R * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    cb_ble_bank_destroy(b);
    return fail(CB_ENOMEM, "cb_ble_bank_create: device allocation or upload failed");
  }
  *out = b;
  return CB_OK;
}

// a call on the handle's device, its arguments checked (the entry below waits for the stream when this fails)
static int ble_bank_run(cb_ble_bank_s *b, const int8_t *cx, const int8_t *cy, int n, int L, const int8_t *all_seqs, int n_seqs,
                        const double *weights, int max_iters, int *lengths_index, int *rate_index, int *iterations,
                        double *kernel_ms) {
  const int S = b->S, T = b->T, R = b->R;
  const size_t nc = (size_t)n * L, ns = (size_t)n_seqs * L;
  if (nc > b->cap_c || ns > b->cap_s || (size_t)n > b->cap_n || (size_t)L > b->cap_L) {   // (grow: everything anew, sizes kept as maxima)
    const size_t cc = std::max(nc, b->cap_c), cs = std::max(ns, b->cap_s), cn = std::max((size_t)n, b->cap_n), cl = std::max((size_t)L, b->cap_L);
    ble_bank_free_ws(b);
    bool ok = hipMalloc((void **)&b->x, cc) == hipSuccess && hipMalloc((void **)&b->y, cc) == hipSuccess &&
              hipMalloc((void **)&b->xT, cc) == hipSuccess && hipMalloc((void **)&b->yT, cc) == hipSuccess &&
              hipMalloc((void **)&b->seqs, cs) == hipSuccess && hipMalloc((void **)&b->s2r, cl * sizeof(int)) == hipSuccess &&
              hipMalloc((void **)&b->l0, cn * sizeof(int)) == hipSuccess && hipMalloc((void **)&b->l1, cn * sizeof(int)) == hipSuccess &&
              hipMalloc((void **)&b->totals, cl * sizeof(long long)) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      ble_bank_free_ws(b);
      return fail(CB_ENOMEM, "cb_ble_bank_run: device allocation failed");
    }
    b->cap_c = cc; b->cap_s = cs; b->cap_n = cn; b->cap_L = cl;
    b->h_totals = std::vector<long long>(cl);
    b->h_s2r = std::vector<int>(cl);
  }
  HIP_TRY(hipMemsetAsync(b->flags, 0, 4 * sizeof(int), 0));
  HIP_TRY(hipMemcpyAsync(b->seqs, all_seqs, ns, hipMemcpyHostToDevice, 0));
  HIP_TRY(hipMemcpyAsync(b->x, cx, nc, hipMemcpyHostToDevice, 0));
  HIP_TRY(hipMemcpyAsync(b->y, cy, nc, hipMemcpyHostToDevice, 0));
  // site statistics, range checks and the transposed copies on the device
  hipLaunchKernelGGL(ble_site_totals_kernel, dim3((L + 31) / 32), dim3(256), 32 * S * sizeof(int), 0, n_seqs, L, S, b->seqs, b->totals, b->flags + 1);
  const dim3 tg((L + 63) / 64, (n + 63) / 64);
  hipLaunchKernelGGL(ble_transpose_check_kernel, tg, dim3(256), 0, 0, n, L, S, b->x, b->xT, b->flags + 1);
  hipLaunchKernelGGL(ble_transpose_check_kernel, tg, dim3(256), 0, 0, n, L, S, b->y, b->yT, b->flags + 1);
  HIP_TRY(hipMemcpyAsync(b->h_totals.data(), b->totals, L * sizeof(long long), hipMemcpyDeviceToHost, 0));
  HIP_TRY(hipMemcpyAsync(&b->h_bad, b->flags + 1, sizeof(int), hipMemcpyDeviceToHost, 0));
  HIP_TRY(hipStreamSynchronize(0));
  if (b->h_bad) return fail(CB_EINVAL, "cb_ble_bank_run: state code out of range");
  ble_bins_from_totals(b->h_totals.data(), L, R, weights, b->h_s2r.data());
  HIP_TRY(hipMemcpyAsync(b->s2r, b->h_s2r.data(), L * sizeof(int), hipMemcpyHostToDevice, 0));
  const BleBankView bank{S, T, R, b->logP, b->priors};
  BleFamilyView fam{n, L, b->x, b->y, b->xT, b->yT, b->s2r, b->l0, b->l1};
  CbKernelTimer timer(kernel_ms != nullptr, b->events.ev0, b->events.ev1);
  int rc, moving = 0, iters = 0;   // (flag word 0: the ascent's; word 1: the bad-code flag read above)
  if ((rc = timer.begin(false)) != CB_OK || (rc = ble_ascent(bank, &fam, 1, max_iters, b->flags, &moving, &iters)) != CB_OK ||
      (rc = timer.end(kernel_ms)) != CB_OK)
    return rc;
  if (iterations) *iterations = iters;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(lengths_index, fam.l0, n * sizeof(int), hipMemcpyDeviceToHost, 0));
  HIP_TRY(hipMemcpyAsync(rate_index, b->s2r, L * sizeof(int), hipMemcpyDeviceToHost, 0));
  HIP_TRY(hipStreamSynchronize(0));
  return CB_OK;
}

extern "C" int cb_ble_bank_run(cb_ble_bank_s *b, const int8_t *cx, const int8_t *cy, int n, int L, const int8_t *all_seqs, int n_seqs,
                               const double *weights, int max_iters, int *lengths_index, int *rate_index, int *iterations,
                               double *kernel_ms) {
  if (!b || !cx || !cy || !all_seqs || !weights || !lengths_index || !rate_index) return fail(CB_EINVAL, "cb_ble_bank_run: NULL argument");
  if (n < 1 || L < 1 || n_seqs < 1 || max_iters < 0) return fail(CB_EINVAL, "cb_ble_bank_run: bad sizes");
  HIP_TRY(hipSetDevice(b->device));
  const int rc = ble_bank_run(b, cx, cy, n, L, all_seqs, n_seqs, weights, max_iters, lengths_index, rate_index, iterations, kernel_ms);
  // the caller's arrays are the other ends of asynchronous copies: none is in flight when a failed call returns
  if (rc != CB_OK) (void)hipStreamSynchronize(0);
  return rc;
}

extern "C" int cb_site_rate_gather(int device, int S, int R, int n, int L, const double *tens, const int8_t *cx,
                                   const int8_t *cy, const double *log_prior, int *best) {
  if (!tens || !cx || !cy || !log_prior || !best) return fail(CB_EINVAL, "cb_site_rate_gather: NULL argument");
  int rc = ble_check(device, S, 1, R, n, L, cx, cy);
  if (rc != CB_OK) return rc;
  for (size_t i = 0; i < (size_t)n * L; ++i)
    if (cx[i] < 0 || cy[i] < 0) return fail(CB_EINVAL, "cb_site_rate_gather: negative state code (map gaps to a state)");
  HIP_TRY(hipSetDevice(device));
  CbDevBufs d;
  const double *dt = d.up(tens, (size_t)R * n * S * S, rc), *dpr = d.up(log_prior, R, rc);
  const int8_t *dx = d.up(cx, (size_t)n * L, rc), *dy = d.up(cy, (size_t)n * L, rc);
  int *dout = d.up<int>(nullptr, L, rc);
  if (rc != CB_OK) return rc;
  hipLaunchKernelGGL(site_rate_gather_kernel, dim3((L + 3) / 4), dim3(256), 0, 0, S, R, n, L, dt, dx, dy, dpr, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(best, dout, L * sizeof(int), hipMemcpyDeviceToHost));
  return CB_OK;
}
