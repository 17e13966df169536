// libcherrybank: the maximum-likelihood rate category of every site on fixed full trees (sr.hip.h; include/cherrybank.h,
// cb_tree_site_rates).  One family at a time, its candidates in chunks under a byte bound; everything is freed on return.
#include "cb_internal.hip.h"
#include "common.hip.h"
#include "sr.hip.h"
#include "em_layout.h"

constexpr size_t SR_MSG_BYTES = (size_t)1 << 30;   // the messages of one chunk of candidates, at most (one candidate always goes);
                                                   // the test hook CB_SR_MSG_BYTES: the results do not depend on the chunking

extern "C" int cb_tree_site_rates(int device, int S, const double *Q, const double *pi_root, int n_fam, const int *n_nodes,
                                  const int *parent, const double *length, const int *n_units, const int8_t *codes,
                                  const int *n_cands, const double *cands, const int *current, int *best, double *best_ll,
                                  double *ll_all, double *kernel_ms) {
  static const char *who = "cb_tree_site_rates";
  if (!Q || !pi_root || !n_nodes || !parent || !length || !n_units || !codes || !n_cands || !cands || !best || !best_ll)
    return fail(CB_EINVAL, "%s: NULL argument", who);
  if (S < 2 || S > 32) return fail(CB_EINVAL, "%s: S = %d (2 <= S <= 32)", who, S);
  if (n_fam < 1) return fail(CB_EINVAL, "%s: families = %d", who, n_fam);
  int rc = em_check_model(who, S, Q, pi_root);
  if (rc != CB_OK) return rc;
  // validation and the host-side structures of every family, before any device work
  std::vector<EmFamHost> fam(n_fam);
  std::vector<size_t> off_n(n_fam + 1, 0), off_u(n_fam + 1, 0), off_c(n_fam + 1, 0), off_k(n_fam + 1, 0), off_ll(n_fam + 1, 0);
  const double one = 1.0;   // em_prepare's quantisation (one point, one rate) is not used here
  size_t max_bank = 0;
  for (int f = 0; f < n_fam; ++f) {
    const int n = n_nodes[f], U = n_units[f], C = n_cands[f];
    if (n < 1 || U < 1) return fail(CB_EINVAL, "%s: family %d has bad sizes (nodes = %d, units = %d)", who, f, n, U);
    if (C < 1 || C > CB_SR_MAX_CANDS)
      return fail(CB_EINVAL, "%s: family %d has %d candidates (1 <= n_cands <= %d)", who, f, C, CB_SR_MAX_CANDS);
    const double *cd = cands + off_k[f];
    for (int c = 0; c < C; ++c)
      if (!(cd[c] > 0.0) || !std::isfinite(cd[c]) || (c > 0 && !(cd[c] > cd[c - 1])))
        return fail(CB_EINVAL, "%s: family %d: the candidates must be positive, finite and strictly increasing (candidate %d = %g)",
                    who, f, c, cd[c]);
    if (current)
      for (int u = 0; u < U; ++u)
        if (current[off_u[f] + u] < -1 || current[off_u[f] + u] >= C)
          return fail(CB_EINVAL, "%s: family %d: current[%d] = %d (-1 or an index below %d)", who, f, u, current[off_u[f] + u], C);
    const std::vector<double> ones(U, 1.0);
    rc = em_prepare(who, S, 1, &one, n, parent + off_n[f], length + off_n[f], U, ones.data(), codes + off_c[f], f, fam[f]);
    if (rc != CB_OK) return rc;
    const size_t n_blocks = ((size_t)U + 64 / S - 1) / (64 / S);
    if ((size_t)n * n_blocks > (size_t)INT32_MAX || (size_t)n * C > (size_t)INT32_MAX)
      return fail(CB_EINVAL, "%s: family %d: %d nodes x %zu site tiles or x %d candidates pass 2^31", who, f, n, n_blocks, C);
    max_bank = std::max(max_bank, (size_t)n * C);
    off_n[f + 1] = off_n[f] + n;
    off_u[f + 1] = off_u[f] + U;
    off_c[f + 1] = off_c[f] + (size_t)n * U;
    off_k[f + 1] = off_k[f] + C;
    off_ll[f + 1] = off_ll[f] + (size_t)C * U;
  }
  // device work from here on
  const int ndev = cb_device_count();
  if (ndev <= 0) return fail(CB_EHIP, "%s: no HIP device (this path has no CPU fallback)", who);
  if (device < 0 || device >= ndev) return fail(CB_EINVAL, "%s: device %d of %d", who, device, ndev);
  HIP_TRY(hipSetDevice(device));
  const size_t SS = (size_t)S * S, msg_bound = cb_hook_bytes("CB_SR_MSG_BYTES", SR_MSG_BYTES);
  const int upw = 64 / S;
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
  // the library's own GENERAL expm, counts-free, as cb_bl_create builds its banks: one handle for the call.  (The expm of the
  // symmetric eigendecomposition is far faster on n_nodes x n_cands matrices but misses the scan's accuracy at very long edges:
  // DESIGN.md section 17.)
  cb_handle hexp = nullptr;
  {
    const std::vector<double> t0(max_bank, 0.0);
    rc = cb_create(device, S, 1, (int)max_bank, CB_F64, t0.data(), nullptr, CB_EXPM_ONLY, &hexp);
  }
  if (rc == CB_OK) rc = cb_set_stream(hexp, nullptr, 0);
  std::vector<double> times;
  std::vector<int> leaves;
  for (int f = 0; f < n_fam && rc == CB_OK; ++f) {
    const EmFamHost &F = fam[f];
    const int n = F.n_nodes, U = F.n_units, C = n_cands[f];
    const double *cd = cands + off_k[f], *len = length + off_n[f];
    times.assign((size_t)n * C, 0.0);   // (the root's stay 0: its matrices are not read)
    leaves.clear();
    for (int v = 0; v < n; ++v) {
      if (F.child_ptr[v] == F.child_ptr[v + 1]) leaves.push_back(v);
      if (v != F.root)
        for (int c = 0; c < C; ++c) times[(size_t)v * C + c] = len[v] * cd[c];
    }
    const size_t per_cand = (size_t)n * U * S * sizeof(double);
    const int chunk = (int)std::min<size_t>(C, std::max<size_t>(msg_bound / per_cand, 1));
    const int n_blocks = (U + upw - 1) / upw;
    CbDevBufs bufs;
    double *dQ = bufs.up(Q, SS, rc), *dpi = bufs.up(pi_root, S, rc);
    double *dP = bufs.up<double>(nullptr, (size_t)n * C * SS, rc);
    double *dmsg = bufs.up<double>(nullptr, (size_t)n * chunk * U * S, rc);
    double *dll = bufs.up<double>(nullptr, (size_t)C * U, rc), *dbest_ll = bufs.up<double>(nullptr, U, rc);
    int *dcp = bufs.up(F.child_ptr.data(), F.child_ptr.size(), rc), *dci = bufs.up(F.child_idx.data(), F.child_idx.size(), rc);
    int *dlev = bufs.up(F.level_nodes.data(), F.level_nodes.size(), rc), *dleaves = bufs.up(leaves.data(), leaves.size(), rc);
    int *dcur = current ? bufs.up(current + off_u[f], U, rc) : nullptr, *dbest = bufs.up<int>(nullptr, U, rc);
    const int8_t *dcodes = bufs.up(codes + off_c[f], (size_t)n * U, rc);
    if (rc != CB_OK) break;
    CbKernelTimer timer(kernel_ms != nullptr);   // (bank, scan + pick) of this family
    double ms[2] = {0.0, 0.0};
    rc = timer.begin(false);
    if (rc == CB_OK) rc = cb_internal_set_times(hexp, times.data(), n * C, nullptr);
    if (rc == CB_OK) rc = cb_internal_expm_bank(hexp, dQ, nullptr, CB_PTR_DEVICE | CB_NO_SYNC, dP);
    if (rc == CB_OK) rc = timer.lap();
    if (rc != CB_OK) break;
    SrScanArgs a{};
    a.S = S; a.n_units = U; a.n_cands = C; a.root = F.root; a.n_blocks = n_blocks;
    a.child_ptr = dcp; a.child_idx = dci; a.P = dP; a.codes = reinterpret_cast<const signed char *>(dcodes); a.pi_root = dpi;
    a.msg = dmsg; a.ll = dll;
    for (int c0 = 0; c0 < C; c0 += chunk) {
      a.c0 = c0;
      a.n_chunk = std::min(chunk, C - c0);
      for (size_t l = 0; l + 1 < F.level_ptr.size(); ++l) {
        const int n_level = F.level_ptr[l + 1] - F.level_ptr[l];
        a.level_nodes = dlev + F.level_ptr[l];
        hipLaunchKernelGGL(sr_scan_kernel, dim3((unsigned)n_level * (unsigned)n_blocks, (unsigned)a.n_chunk), dim3(64), 0, 0, a);
      }
    }
    SrPickArgs p{};
    p.n_units = U; p.n_cands = C; p.n_leaves = (int)leaves.size(); p.leaves = dleaves; p.codes = a.codes; p.current = dcur;
    p.ll = dll; p.best = dbest; p.best_ll = dbest_ll;
    hipLaunchKernelGGL(sr_pick_kernel, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, 0, p);
    if (rc == CB_OK && hipGetLastError() != hipSuccess) rc = fail(CB_EHIP, "%s: family %d: a kernel launch failed", who, f);
    if (rc == CB_OK) rc = timer.end(ms);
    if (rc != CB_OK) break;
    if (kernel_ms) {
      kernel_ms[0] += ms[0];
      kernel_ms[1] += ms[1];
    }
    hipError_t e = hipMemcpy(best + off_u[f], dbest, (size_t)U * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(best_ll + off_u[f], dbest_ll, (size_t)U * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && ll_all) e = hipMemcpy(ll_all + off_ll[f], dll, (size_t)C * U * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(CB_EHIP, "%s: family %d: %s", who, f, hipGetErrorString(e));
  }
  if (hipDeviceSynchronize() != hipSuccess && rc == CB_OK) rc = fail(CB_EHIP, "%s: %s", who, hipGetErrorString(hipGetLastError()));
  if (hexp) cb_destroy(hexp);
  return rc;
}
