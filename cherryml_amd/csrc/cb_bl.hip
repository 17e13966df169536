// libcherrybank: maximum-likelihood branch lengths on fixed trees by EM, on a resident handle (bl.hip.h; include/cherrybank.h,
// cb_bl_*), the nearest-neighbour-interchange scan on the handle's resident messages (nni.hip.h; cb_bl_nni_scan) and the marginal
// ancestral reconstruction from the same messages (anc.hip.h; cb_bl_ancestral).
#include "cb_internal.hip.h"
#include "common.hip.h"
#include "bl.hip.h"
#include "nni.hip.h"
#include "anc.hip.h"
#include "em_host.hip.h"

struct cb_bl_s {
  int device = 0, S = 0, T = 0, n_fam = 0;
  size_t n_units_all = 0, n_nodes_all = 0;
  std::vector<EmFamHost> fam;
  std::vector<size_t> off_n, off_q, off_u, off_c, off_lev, off_cat, off_log;   // per family: nodes, qb, units, codes, depth list,
                                                                               // cat_ptr, log bank
  std::vector<int> bank_base;             // per family: its first bank entry
  std::vector<int> tau;                   // [sum n_nodes] the current indices (root: -1), the device's mirror
  std::vector<int> parent;                // [sum n_nodes] the families' parent arrays (the host's copy: cb_bl_nni_scan validates on it)
  std::vector<char> fixed, ll_fresh;      // per family: at a fixed point; dll holds l_u at the current indices
  std::vector<double> fam_ll;             // per family: the log-likelihood at the current indices when ll_fresh
  std::vector<void *> bufs;               // every device buffer below
  double *dQ = nullptr, *dpi = nullptr, *dP = nullptr, *dlogP = nullptr, *dmsg = nullptr, *dU = nullptr, *dll = nullptr;
  int *dparent = nullptr, *dcp = nullptr, *dci = nullptr, *dlev = nullptr, *ddep = nullptr, *dqb = nullptr, *duc = nullptr;
  int *dcat = nullptr, *dtau = nullptr, *dchanged = nullptr;
  signed char *dcodes = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

template <typename T>
static T *bl_alloc(cb_bl_s *h, const T *host, size_t count, int &rc) {
  if (rc != CB_OK) return nullptr;
  void *p = nullptr;
  if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    rc = fail(CB_ENOMEM, "cb_bl_create: %zu bytes of device memory", count * sizeof(T));
    return nullptr;
  }
  h->bufs.push_back(p);
  if (host && count && hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(CB_EHIP, "cb_bl_create: upload failed");
  return static_cast<T *>(p);
}

extern "C" int cb_bl_destroy(cb_bl_s *h) {
  if (!h) return CB_OK;
  if (!h->bufs.empty() || h->ev[0]) (void)hipSetDevice(h->device);
  for (hipEvent_t e : h->ev)
    if (e) (void)hipEventDestroy(e);
  for (void *p : h->bufs)
    if (p) (void)hipFree(p);
  delete h;
  return CB_OK;
}

extern "C" int cb_bl_create(int device, int S, int T, const double *grid, const double *Q, const double *pi_root, int n_fam,
                            const int *n_nodes, const int *parent, const double *length, const int *n_units,
                            const double *unit_rate, const int8_t *codes, cb_bl_s **out) {
  if (!grid || !Q || !pi_root || !n_nodes || !parent || !length || !n_units || !unit_rate || !codes || !out)
    return fail(CB_EINVAL, "cb_bl_create: NULL argument");
  *out = nullptr;
  if (S < 2 || S > 32) return fail(CB_EINVAL, "cb_bl_create: S = %d (2 <= S <= 32: one 32 x 32 MFMA tile per edge)", S);
  if (T < 2) return fail(CB_EINVAL, "cb_bl_create: T = %d (a grid of at least 2 points)", T);
  if (n_fam < 1) return fail(CB_EINVAL, "cb_bl_create: families = %d", n_fam);
  for (int b = 0; b < T; ++b)
    if (!(grid[b] > 0.0) || !std::isfinite(grid[b]) || (b > 0 && !(grid[b] > grid[b - 1])))
      return fail(CB_EINVAL, "cb_bl_create: the grid must be positive and strictly increasing (grid[%d] = %g)", b, grid[b]);
  int rc = em_check_model("cb_bl_create", S, Q, pi_root);
  if (rc != CB_OK) return rc;
  cb_bl_s *h = new cb_bl_s;
  h->device = device; h->S = S; h->T = T; h->n_fam = n_fam;
  h->fam.resize(n_fam);
  for (auto *o : {&h->off_n, &h->off_q, &h->off_u, &h->off_c, &h->off_lev, &h->off_cat, &h->off_log}) o->assign(n_fam + 1, 0);
  h->bank_base.assign(n_fam + 1, 0);
  const size_t SS = (size_t)S * S;
  size_t entries = 0, max_bank = 0;
  for (int f = 0; f < n_fam; ++f) {
    const double *rate = unit_rate + h->off_u[f];
    // rate 0 is a rate of cb_em_create, not of this handle: log expm(0) is no bank entry
    for (int u = 0; u < n_units[f]; ++u)
      if (!(rate[u] > 0.0) || !std::isfinite(rate[u])) {
        rc = fail(CB_EINVAL, "cb_bl_create: family %d: site rate %d = %g (finite and > 0)", f, u, rate[u]);
        break;
      }
    EmFamHost &F = h->fam[f];
    if (rc == CB_OK)
      rc = em_prepare("cb_bl_create", S, T, grid, n_nodes[f], parent + h->off_n[f], length + h->off_n[f], n_units[f], rate,
                      codes + h->off_c[f], f, F);
    if (rc == CB_OK && F.n_cats > CB_BL_MAX_CATS)
      rc = fail(CB_EINVAL, "cb_bl_create: family %d has %d distinct site rates (at most %d)", f, F.n_cats, CB_BL_MAX_CATS);
    if (rc == CB_OK && entries + (size_t)T * F.n_cats > (size_t)1 << 30)
      rc = fail(CB_EINVAL, "cb_bl_create: %zu bank entries up to family %d (at most 2^30 per handle)", entries + (size_t)T * F.n_cats, f);
    if (rc != CB_OK) {
      cb_bl_destroy(h);
      return rc;
    }
    h->bank_base[f] = (int)entries;
    entries += (size_t)T * F.n_cats;
    max_bank = std::max(max_bank, (size_t)T * F.n_cats);
    h->off_n[f + 1] = h->off_n[f] + n_nodes[f];
    h->off_u[f + 1] = h->off_u[f] + n_units[f];
    h->off_c[f + 1] = h->off_c[f] + (size_t)n_nodes[f] * n_units[f];
    h->off_q[f + 1] = h->off_q[f] + (size_t)n_nodes[f] * F.n_cats;
    h->off_cat[f + 1] = h->off_cat[f] + F.n_cats + 1;
    h->off_log[f + 1] = h->off_log[f] + (size_t)T * F.n_cats * SS;
  }
  h->bank_base[n_fam] = (int)entries;
  h->n_nodes_all = h->off_n[n_fam];
  h->n_units_all = h->off_u[n_fam];
  h->parent.assign(parent, parent + h->n_nodes_all);
  // the input lengths snapped to the grid (the nearest point in ratio, clamped to its ends); the edge's bank entries
  h->tau.assign(h->n_nodes_all, -1);
  for (int f = 0; f < n_fam; ++f) {
    EmFamHost &F = h->fam[f];
    for (int v = 0; v < F.n_nodes; ++v) {
      const int t = v == F.root ? 0 : em_quantize(length[h->off_n[f] + v], grid, T);
      if (v != F.root) h->tau[h->off_n[f] + v] = t;
      for (int c = 0; c < F.n_cats; ++c) F.qb[(size_t)v * F.n_cats + c] = h->bank_base[f] + t * F.n_cats + c;
    }
  }
  h->fixed.assign(n_fam, 0);
  h->ll_fresh.assign(n_fam, 0);
  h->fam_ll.assign(n_fam, 0.0);
  // device work from here on
  const int ndev = cb_device_count();
  if (ndev <= 0) {
    cb_bl_destroy(h);
    return fail(CB_EHIP, "cb_bl_create: no HIP device (this path has no CPU fallback)");
  }
  if (device < 0 || device >= ndev) {
    cb_bl_destroy(h);
    return fail(CB_EINVAL, "cb_bl_create: device %d of %d", device, ndev);
  }
  if (hipSetDevice(device) != hipSuccess) {
    cb_bl_destroy(h);
    return fail(CB_EHIP, "cb_bl_create: hipSetDevice(%d) failed", device);
  }
  // per-family arrays, concatenated; units permuted into category order
  const size_t NN = h->n_nodes_all;
  std::vector<int> par_all(NN), cp_all(NN + n_fam), ci_all(NN), lev_all(NN), dep_all, qb_all(h->off_q[n_fam]), uc_all(h->n_units_all);
  std::vector<int> cat_all(h->off_cat[n_fam]);
  std::vector<int8_t> code_all(h->off_c[n_fam]);
  for (int f = 0; f < n_fam; ++f) {
    const EmFamHost &F = h->fam[f];
    std::copy(parent + h->off_n[f], parent + h->off_n[f + 1], par_all.begin() + h->off_n[f]);
    std::copy(F.child_ptr.begin(), F.child_ptr.end(), cp_all.begin() + h->off_n[f] + f);
    std::copy(F.child_idx.begin(), F.child_idx.begin() + (F.n_nodes - 1), ci_all.begin() + h->off_n[f]);
    std::copy(F.level_nodes.begin(), F.level_nodes.end(), lev_all.begin() + h->off_n[f]);
    h->off_lev[f] = dep_all.size();
    dep_all.insert(dep_all.end(), F.depth_nodes.begin(), F.depth_nodes.end());
    std::copy(F.qb.begin(), F.qb.end(), qb_all.begin() + h->off_q[f]);
    std::copy(F.unit_cat.begin(), F.unit_cat.end(), uc_all.begin() + h->off_u[f]);
    std::copy(F.cat_ptr.begin(), F.cat_ptr.end(), cat_all.begin() + h->off_cat[f]);
    for (int v = 0; v < F.n_nodes; ++v)
      for (int k = 0; k < F.n_units; ++k)
        code_all[h->off_c[f] + (size_t)v * F.n_units + k] = codes[h->off_c[f] + (size_t)v * F.n_units + F.perm[k]];
  }
  h->off_lev[n_fam] = dep_all.size();
  h->dQ = bl_alloc(h, Q, SS, rc);
  h->dpi = bl_alloc(h, pi_root, S, rc);
  h->dP = bl_alloc<double>(h, nullptr, entries * SS, rc);
  h->dlogP = bl_alloc<double>(h, nullptr, entries * SS, rc);
  h->dmsg = bl_alloc<double>(h, nullptr, h->off_c[n_fam] * S, rc);
  h->dU = bl_alloc<double>(h, nullptr, h->off_c[n_fam] * S, rc);
  h->dll = bl_alloc<double>(h, nullptr, h->n_units_all, rc);
  h->dparent = bl_alloc(h, par_all.data(), par_all.size(), rc);
  h->dcp = bl_alloc(h, cp_all.data(), cp_all.size(), rc);
  h->dci = bl_alloc(h, ci_all.data(), ci_all.size(), rc);
  h->dlev = bl_alloc(h, lev_all.data(), lev_all.size(), rc);
  h->ddep = bl_alloc(h, dep_all.data(), dep_all.size(), rc);
  h->dqb = bl_alloc(h, qb_all.data(), qb_all.size(), rc);
  h->duc = bl_alloc(h, uc_all.data(), uc_all.size(), rc);
  h->dcat = bl_alloc(h, cat_all.data(), cat_all.size(), rc);
  h->dtau = bl_alloc(h, h->tau.data(), h->tau.size(), rc);
  h->dchanged = bl_alloc<int>(h, nullptr, NN, rc);
  h->dcodes = reinterpret_cast<signed char *>(bl_alloc(h, code_all.data(), code_all.size(), rc));
  for (hipEvent_t &e : h->ev)
    if (rc == CB_OK && hipEventCreate(&e) != hipSuccess) rc = fail(CB_EHIP, "cb_bl_create: hipEventCreate failed");
  // the banks, once (Q is fixed): the library's own expm at the T R times grid[tau] rate_c of each family, then their logs
  cb_handle hexp = nullptr;
  if (rc == CB_OK) {
    const std::vector<double> t0(max_bank, 0.0);
    rc = cb_create(device, S, 1, (int)max_bank, CB_F64, t0.data(), nullptr, CB_EXPM_ONLY, &hexp);
  }
  if (rc == CB_OK) rc = cb_set_stream(hexp, nullptr, 0);
  std::vector<double> times;
  for (int f = 0; f < n_fam && rc == CB_OK; ++f) {
    const EmFamHost &F = h->fam[f];
    const int R = F.n_cats;
    times.resize((size_t)T * R);
    for (int t = 0; t < T; ++t)
      for (int c = 0; c < R; ++c) times[(size_t)t * R + c] = grid[t] * F.cats[c];
    rc = cb_internal_set_times(hexp, times.data(), T * R, nullptr);
    double *Pf = h->dP + (size_t)h->bank_base[f] * SS;
    if (rc == CB_OK) rc = cb_internal_expm_bank(hexp, h->dQ, nullptr, CB_PTR_DEVICE | CB_NO_SYNC, Pf);
    if (rc == CB_OK) {
      const size_t n = (size_t)T * R * SS;
      hipLaunchKernelGGL(bl_log_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, T, R, (int)SS, Pf, h->dlogP + h->off_log[f]);
    }
  }
  if (rc == CB_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(CB_EHIP, "cb_bl_create: %s", hipGetErrorString(hipGetLastError()));
  if (hexp) cb_destroy(hexp);
  if (rc != CB_OK) {
    cb_bl_destroy(h);
    return rc;
  }
  *out = h;
  return CB_OK;
}

// the inside pass of family f (and its outside pass) at the current indices, stream 0
static void bl_launch_passes(cb_bl_s *h, int f, bool outside) {
  const int S = h->S, upw = 64 / S;
  const EmFamHost &F = h->fam[f];
  const size_t nb = h->off_c[f];
  const int n_blocks = (F.n_units + upw - 1) / upw;
  TlArgs a{};
  a.S = S; a.S1 = 0; a.n_nodes = F.n_nodes; a.n_units = F.n_units; a.NU = F.n_units; a.root = F.root; a.n_blocks = n_blocks;
  a.child_ptr = h->dcp + h->off_n[f] + f; a.child_idx = h->dci + h->off_n[f]; a.P = h->dP;
  a.unit_cat = h->duc + h->off_u[f]; a.code_a = h->dcodes + nb; a.code_b = nullptr; a.pi_root = h->dpi;
  a.msg = h->dmsg + nb * S; a.ll = h->dll + h->off_u[f];
  const int *qb = h->dqb + h->off_q[f];
  for (size_t l = 0; l + 1 < F.level_ptr.size(); ++l) {
    TlArgs b = a;
    b.level_nodes = h->dlev + h->off_n[f] + F.level_ptr[l];
    b.n_level = F.level_ptr[l + 1] - F.level_ptr[l];
    em_launch_up(b, qb, F.n_cats, (unsigned)(b.n_level * n_blocks));
  }
  if (!outside) return;
  EmDownArgs d{};
  d.S = S; d.n_units = F.n_units; d.root = F.root; d.n_blocks = n_blocks; d.n_cats = F.n_cats;
  d.parent = h->dparent + h->off_n[f]; d.child_ptr = a.child_ptr; d.child_idx = a.child_idx; d.qb = qb;
  d.unit_cat = a.unit_cat; d.P = h->dP; d.pi_root = h->dpi; d.msg = a.msg; d.U = h->dU + nb * S;
  for (size_t l = 0; l + 1 < F.depth_ptr.size(); ++l) {
    const int nl = F.depth_ptr[l + 1] - F.depth_ptr[l];
    if (nl == 0) continue;
    EmDownArgs e = d;
    e.level_nodes = h->ddep + h->off_lev[f] + F.depth_ptr[l];
    em_launch_down(e, (unsigned)(nl * n_blocks));
  }
}

static void bl_launch_mstep(cb_bl_s *h, int f) {
  const EmFamHost &F = h->fam[f];
  if (F.n_nodes < 2) return;
  const size_t nb = h->off_c[f];
  BlArgs a{};
  a.S = h->S; a.T = h->T; a.n_cats = F.n_cats; a.n_units = F.n_units; a.root = F.root; a.bank_base = h->bank_base[f];
  a.parent = h->dparent + h->off_n[f]; a.child_ptr = h->dcp + h->off_n[f] + f; a.child_idx = h->dci + h->off_n[f];
  a.cat_ptr = h->dcat + h->off_cat[f]; a.codes = h->dcodes + nb; a.pi_root = h->dpi;
  a.msg = h->dmsg + nb * h->S; a.U = h->dU + nb * h->S; a.ll = h->dll + h->off_u[f];
  a.P = h->dP; a.logP = h->dlogP + h->off_log[f];
  a.qb = h->dqb + h->off_q[f]; a.tau = h->dtau + h->off_n[f]; a.changed = h->dchanged + h->off_n[f];
  hipLaunchKernelGGL(bl_mstep_kernel, dim3((unsigned)F.n_nodes), dim3(64), 0, 0, a);
}

// l_u of the device (category order) -> the caller's unit order; the families in `which` get their sums (in the caller's order)
static int bl_read_ll(cb_bl_s *h, const std::vector<char> &which, std::vector<double> *orig_out) {
  std::vector<double> llp(h->n_units_all), orig(h->n_units_all);
  HIP_TRY(hipMemcpy(llp.data(), h->dll, h->n_units_all * sizeof(double), hipMemcpyDeviceToHost));
  for (int f = 0; f < h->n_fam; ++f) {
    const EmFamHost &F = h->fam[f];
    const size_t ub = h->off_u[f];
    for (int k = 0; k < F.n_units; ++k) orig[ub + F.perm[k]] = llp[ub + k];
    if (!which[f]) continue;
    double s = 0.0;
    for (int u = 0; u < F.n_units; ++u) s += orig[ub + u];
    h->fam_ll[f] = s;
  }
  if (orig_out) orig_out->swap(orig);
  return CB_OK;
}

extern "C" int cb_bl_round(cb_bl_s *h, int *n_changed, double *fam_ll, double *kernel_ms) {
  if (!h) return fail(CB_EINVAL, "cb_bl_round: NULL handle");
  if (!n_changed || !fam_ll) return fail(CB_EINVAL, "cb_bl_round: NULL argument");
  HIP_TRY(hipSetDevice(h->device));
  std::vector<char> live(h->n_fam);
  for (int f = 0; f < h->n_fam; ++f) live[f] = !h->fixed[f];
  if (kernel_ms) HIP_TRY(hipEventRecord(h->ev[0], 0));
  for (int f = 0; f < h->n_fam; ++f)
    if (live[f]) bl_launch_passes(h, f, true);
  if (kernel_ms) HIP_TRY(hipEventRecord(h->ev[1], 0));
  for (int f = 0; f < h->n_fam; ++f)
    if (live[f]) bl_launch_mstep(h, f);
  if (kernel_ms) {
    float ms0 = 0.f, ms1 = 0.f;
    HIP_TRY(hipEventRecord(h->ev[2], 0));
    HIP_TRY(hipEventSynchronize(h->ev[2]));
    HIP_TRY(hipEventElapsedTime(&ms0, h->ev[0], h->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms1, h->ev[1], h->ev[2]));
    kernel_ms[0] = ms0;
    kernel_ms[1] = ms1;
  }
  HIP_TRY(hipGetLastError());
  // a fixed family keeps the sum of the round that found its fixed point: the same lengths, the same bits
  const int rc = bl_read_ll(h, live, nullptr);
  if (rc != CB_OK) return rc;
  std::vector<int> flags(h->n_nodes_all);
  HIP_TRY(hipMemcpy(flags.data(), h->dchanged, flags.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->tau.data(), h->dtau, h->tau.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int f = 0; f < h->n_fam; ++f) {
    fam_ll[f] = h->fam_ll[f];
    n_changed[f] = 0;
    if (!live[f]) continue;
    const EmFamHost &F = h->fam[f];
    for (int v = 0; v < F.n_nodes; ++v)
      if (v != F.root) n_changed[f] += flags[h->off_n[f] + v] != 0;
    h->fixed[f] = n_changed[f] == 0;
    h->ll_fresh[f] = n_changed[f] == 0;
  }
  return CB_OK;
}

extern "C" int cb_bl_get(cb_bl_s *h, int *index, double *ll, double *fam_ll) {
  if (!h) return fail(CB_EINVAL, "cb_bl_get: NULL handle");
  if (!index) return fail(CB_EINVAL, "cb_bl_get: NULL argument");
  std::copy(h->tau.begin(), h->tau.end(), index);
  if (!ll && !fam_ll) return CB_OK;
  HIP_TRY(hipSetDevice(h->device));
  std::vector<char> stale(h->n_fam);
  for (int f = 0; f < h->n_fam; ++f) {
    stale[f] = !h->ll_fresh[f];
    if (stale[f]) bl_launch_passes(h, f, false);
  }
  HIP_TRY(hipGetLastError());
  std::vector<double> orig;
  const int rc = bl_read_ll(h, stale, &orig);
  if (rc != CB_OK) return rc;
  std::fill(h->ll_fresh.begin(), h->ll_fresh.end(), 1);
  if (ll) std::copy(orig.begin(), orig.end(), ll);
  if (fam_ll) std::copy(h->fam_ll.begin(), h->fam_ll.end(), fam_ll);
  return CB_OK;
}

namespace {
constexpr size_t NNI_LL_BYTES = (size_t)256 << 20;   // ll'[move][unit] of one chunk of moves, at most (one move always goes)

// the bound above, or the test hook CB_NNI_LL_BYTES (cb_internal.hip.h): the results do not depend on the chunking
size_t nni_ll_bound() {
  const char *s = cb_test_hook("CB_NNI_LL_BYTES");
  const long long x = s ? atoll(s) : 0;
  return x > 0 ? (size_t)x : NNI_LL_BYTES;
}
}  // namespace

extern "C" int cb_bl_nni_scan(cb_bl_s *h, const int *n_moves, const int *moves, double *delta, double *ll_moves, double *fam_ll,
                              double *kernel_ms) {
  static const char *who = "cb_bl_nni_scan";
  if (!h) return fail(CB_EINVAL, "%s: NULL handle", who);
  if (!n_moves || !delta) return fail(CB_EINVAL, "%s: NULL argument", who);
  // every triple, on the host, before any device work
  const int n_fam = h->n_fam;
  std::vector<size_t> off_m(n_fam + 1, 0), off_o(n_fam + 1, 0);
  for (int f = 0; f < n_fam; ++f) {
    if (n_moves[f] < 0) return fail(CB_EINVAL, "%s: family %d: n_moves = %d", who, f, n_moves[f]);
    off_m[f + 1] = off_m[f] + n_moves[f];
    off_o[f + 1] = off_o[f] + (size_t)n_moves[f] * h->fam[f].n_units;
  }
  if (off_m[n_fam] > 0 && !moves) return fail(CB_EINVAL, "%s: NULL argument", who);
  size_t max_moves = 0, max_out = 0;
  std::vector<int> chunk(n_fam, 0);
  const size_t bound = nni_ll_bound();
  for (int f = 0; f < n_fam; ++f) {
    const EmFamHost &F = h->fam[f];
    const int n = F.n_nodes, *par = h->parent.data() + h->off_n[f];
    for (int m = 0; m < n_moves[f]; ++m) {
      const int *t = moves + 3 * (off_m[f] + m);
      const int v = t[0], c = t[1], s = t[2];
      if (v < 0 || v >= n) return fail(CB_EINVAL, "%s: family %d move %d: v = %d (0 <= index < %d)", who, f, m, v, n);
      if (c < 0 || c >= n) return fail(CB_EINVAL, "%s: family %d move %d: c = %d (0 <= index < %d)", who, f, m, c, n);
      if (s < 0 || s >= n) return fail(CB_EINVAL, "%s: family %d move %d: s = %d (0 <= index < %d)", who, f, m, s, n);
      if (v == F.root) return fail(CB_EINVAL, "%s: family %d move %d: v = %d is the root", who, f, m, v);
      if (F.child_ptr[v] == F.child_ptr[v + 1]) return fail(CB_EINVAL, "%s: family %d move %d: v = %d is a leaf", who, f, m, v);
      if (par[c] != v) return fail(CB_EINVAL, "%s: family %d move %d: c = %d is not a child of v = %d", who, f, m, c, v);
      if (s == v) return fail(CB_EINVAL, "%s: family %d move %d: s = %d equals v", who, f, m, s);
      if (par[s] != par[v])
        return fail(CB_EINVAL, "%s: family %d move %d: s = %d is not a child of parent[v] = %d", who, f, m, s, par[v]);
    }
    if (n_moves[f] == 0) continue;
    const size_t n_blocks = ((size_t)F.n_units + 64 / h->S - 1) / (64 / h->S);
    const size_t fit = std::min(bound / ((size_t)F.n_units * sizeof(double)), (size_t)INT32_MAX / n_blocks);
    chunk[f] = (int)std::min<size_t>(n_moves[f], std::max<size_t>(fit, 1));
    max_moves = std::max(max_moves, (size_t)n_moves[f]);
    max_out = std::max(max_out, (size_t)chunk[f] * F.n_units);
  }
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
  if (max_moves > 0) {
    HIP_TRY(hipSetDevice(h->device));
    // the messages of the families that are scanned, at the current indices: after a round the resident ones are its start's
    if (kernel_ms) HIP_TRY(hipEventRecord(h->ev[0], 0));
    for (int f = 0; f < n_fam; ++f)
      if (n_moves[f] > 0) bl_launch_passes(h, f, true);
    HIP_TRY(hipGetLastError());
    if (kernel_ms) {
      float ms = 0.f;
      HIP_TRY(hipEventRecord(h->ev[1], 0));
      HIP_TRY(hipEventSynchronize(h->ev[1]));
      HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
      kernel_ms[0] = ms;
    }
    int rc = CB_OK;
    std::vector<double> host_out(ll_moves ? max_out : 0);
    CbDevBufs bufs;   // this call's: freed on every return path
    int *dmoves = bufs.up<int>(nullptr, 3 * max_moves, rc);
    double *dout = bufs.up<double>(nullptr, max_out, rc), *ddelta = bufs.up<double>(nullptr, max_moves, rc);
    if (rc != CB_OK) return rc;
    for (int f = 0; f < n_fam; ++f) {
      if (n_moves[f] == 0) continue;
      const EmFamHost &F = h->fam[f];
      const size_t nb = h->off_c[f];
      const int U = F.n_units, upw = 64 / h->S;
      HIP_TRY(hipMemcpy(dmoves, moves + 3 * off_m[f], 3 * (size_t)n_moves[f] * sizeof(int), hipMemcpyHostToDevice));
      NniArgs a{};
      a.S = h->S; a.n_units = U; a.n_cats = F.n_cats; a.root = F.root; a.n_blocks = (U + upw - 1) / upw;
      a.parent = h->dparent + h->off_n[f]; a.child_ptr = h->dcp + h->off_n[f] + f; a.child_idx = h->dci + h->off_n[f];
      a.qb = h->dqb + h->off_q[f]; a.unit_cat = h->duc + h->off_u[f]; a.P = h->dP; a.pi_root = h->dpi;
      a.msg = h->dmsg + nb * h->S; a.U = h->dU + nb * h->S; a.ll = h->dll + h->off_u[f]; a.out = dout;
      for (int m0 = 0; m0 < n_moves[f]; m0 += chunk[f]) {
        const int nm = std::min(chunk[f], n_moves[f] - m0);
        a.moves = dmoves + 3 * (size_t)m0;
        a.delta = ddelta + m0;
        if (kernel_ms) HIP_TRY(hipEventRecord(h->ev[1], 0));
        hipLaunchKernelGGL(nni_scan_kernel, dim3((unsigned)nm * (unsigned)a.n_blocks), dim3(64), 0, 0, a);
        hipLaunchKernelGGL(nni_sum_kernel, dim3((unsigned)nm), dim3(64), 0, 0, a);
        HIP_TRY(hipGetLastError());
        if (kernel_ms) {
          float ms = 0.f;
          HIP_TRY(hipEventRecord(h->ev[2], 0));
          HIP_TRY(hipEventSynchronize(h->ev[2]));
          HIP_TRY(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
          kernel_ms[1] += ms;
        }
        // (the next chunk writes the same buffer: stream order puts it behind this chunk's sum)
        if (ll_moves) {   // device (category) order -> the caller's unit order
          HIP_TRY(hipMemcpy(host_out.data(), dout, (size_t)nm * U * sizeof(double), hipMemcpyDeviceToHost));
          for (int m = 0; m < nm; ++m) {
            double *dst = ll_moves + off_o[f] + (size_t)(m0 + m) * U;
            for (int k = 0; k < U; ++k) dst[F.perm[k]] = host_out[(size_t)m * U + k];
          }
        }
      }
      HIP_TRY(hipMemcpy(delta + off_m[f], ddelta, (size_t)n_moves[f] * sizeof(double), hipMemcpyDeviceToHost));
    }
    // dll of the scanned families now holds l_u at the current indices -- the bits cb_bl_get's inside pass would write
    std::vector<char> stale(n_fam);
    for (int f = 0; f < n_fam; ++f) stale[f] = n_moves[f] > 0 && !h->ll_fresh[f];
    rc = bl_read_ll(h, stale, nullptr);
    if (rc != CB_OK) return rc;
    for (int f = 0; f < n_fam; ++f)
      if (stale[f]) h->ll_fresh[f] = 1;
  }
  if (fam_ll)
    for (int f = 0; f < n_fam; ++f) fam_ll[f] = h->ll_fresh[f] ? h->fam_ll[f] : std::nan("");
  return CB_OK;
}

namespace {
constexpr size_t ANC_POST_BYTES = (size_t)256 << 20;   // post[node][unit][S] of one chunk of nodes, at most (one node always goes)

// the bound above, or the test hook CB_ANC_POST_BYTES (cb_internal.hip.h): the results do not depend on the chunking
size_t anc_post_bound() {
  const char *s = cb_test_hook("CB_ANC_POST_BYTES");
  const long long x = s ? atoll(s) : 0;
  return x > 0 ? (size_t)x : ANC_POST_BYTES;
}
}  // namespace

extern "C" int cb_bl_ancestral(cb_bl_s *h, int8_t *state, double *conf, double *post, double *fam_ll, double *kernel_ms) {
  static const char *who = "cb_bl_ancestral";
  if (!h) return fail(CB_EINVAL, "%s: NULL handle", who);
  if (!state) return fail(CB_EINVAL, "%s: NULL argument (state)", who);
  const int n_fam = h->n_fam, S = h->S, upw = 64 / S;
  // nodes per launch: all of a family's, fewer under the bound on post and where nodes x site tiles would pass 2^31
  std::vector<int> chunk(n_fam, 0);
  size_t max_out = 0;
  const size_t bound = anc_post_bound();
  for (int f = 0; f < n_fam; ++f) {
    const EmFamHost &F = h->fam[f];
    const size_t n_blocks = ((size_t)F.n_units + upw - 1) / upw;
    size_t fit = (size_t)INT32_MAX / n_blocks;
    if (post) fit = std::min(fit, bound / ((size_t)F.n_units * S * sizeof(double)));
    chunk[f] = (int)std::min<size_t>(F.n_nodes, std::max<size_t>(fit, 1));
    if ((size_t)chunk[f] * n_blocks > (size_t)INT32_MAX)
      return fail(CB_EINVAL, "%s: family %d: %zu site tiles (at most 2^31 - 1 per launch)", who, f, n_blocks);
    max_out = std::max(max_out, (size_t)chunk[f] * F.n_units);
  }
  HIP_TRY(hipSetDevice(h->device));
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
  // the messages at the current indices: after a round the resident ones are its start's
  if (kernel_ms) HIP_TRY(hipEventRecord(h->ev[0], 0));
  for (int f = 0; f < n_fam; ++f) bl_launch_passes(h, f, true);
  HIP_TRY(hipGetLastError());
  if (kernel_ms) {
    float ms = 0.f;
    HIP_TRY(hipEventRecord(h->ev[1], 0));
    HIP_TRY(hipEventSynchronize(h->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    kernel_ms[0] = ms;
  }
  int rc = CB_OK;
  std::vector<int8_t> host_state(max_out);
  std::vector<double> host_conf(conf ? max_out : 0), host_post(post ? max_out * S : 0);
  CbDevBufs bufs;   // this call's: freed on every return path
  signed char *dstate = bufs.up<signed char>(nullptr, max_out, rc);
  double *dconf = bufs.up<double>(nullptr, max_out, rc), *dpost = post ? bufs.up<double>(nullptr, max_out * S, rc) : nullptr;
  if (rc != CB_OK) return rc;
  for (int f = 0; f < n_fam; ++f) {
    const EmFamHost &F = h->fam[f];
    const size_t nb = h->off_c[f];
    const int U = F.n_units;
    AncArgs a{};
    a.S = S; a.n_units = U; a.n_cats = F.n_cats; a.root = F.root; a.n_blocks = (U + upw - 1) / upw;
    a.parent = h->dparent + h->off_n[f]; a.child_ptr = h->dcp + h->off_n[f] + f; a.child_idx = h->dci + h->off_n[f];
    a.qb = h->dqb + h->off_q[f]; a.unit_cat = h->duc + h->off_u[f]; a.codes = h->dcodes + nb; a.P = h->dP; a.pi_root = h->dpi;
    a.msg = h->dmsg + nb * S; a.U = h->dU + nb * S; a.state = dstate; a.conf = dconf; a.post = dpost;
    for (int v0 = 0; v0 < F.n_nodes; v0 += chunk[f]) {
      const int nv = std::min(chunk[f], F.n_nodes - v0);
      a.node0 = v0;
      if (kernel_ms) HIP_TRY(hipEventRecord(h->ev[1], 0));
      hipLaunchKernelGGL(anc_post_kernel, dim3((unsigned)nv * (unsigned)a.n_blocks), dim3(64), 0, 0, a);
      HIP_TRY(hipGetLastError());
      if (kernel_ms) {
        float ms = 0.f;
        HIP_TRY(hipEventRecord(h->ev[2], 0));
        HIP_TRY(hipEventSynchronize(h->ev[2]));
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
        kernel_ms[1] += ms;
      }
      // device (category) order -> the caller's unit order (the next chunk writes the same buffers: these copies wait for this one)
      const size_t cnt = (size_t)nv * U, base = nb + (size_t)v0 * U;
      HIP_TRY(hipMemcpy(host_state.data(), dstate, cnt * sizeof(int8_t), hipMemcpyDeviceToHost));
      if (conf) HIP_TRY(hipMemcpy(host_conf.data(), dconf, cnt * sizeof(double), hipMemcpyDeviceToHost));
      if (post) HIP_TRY(hipMemcpy(host_post.data(), dpost, cnt * S * sizeof(double), hipMemcpyDeviceToHost));
      for (int v = 0; v < nv; ++v)
        for (int k = 0; k < U; ++k) {
          const size_t src = (size_t)v * U + k, dst = base + (size_t)v * U + F.perm[k];
          state[dst] = host_state[src];
          if (conf) conf[dst] = host_conf[src];
          if (post) std::copy(host_post.begin() + src * S, host_post.begin() + (src + 1) * S, post + dst * S);
        }
    }
  }
  // dll now holds l_u at the current indices -- the bits cb_bl_get's inside pass would write
  std::vector<char> stale(n_fam);
  for (int f = 0; f < n_fam; ++f) stale[f] = !h->ll_fresh[f];
  rc = bl_read_ll(h, stale, nullptr);
  if (rc != CB_OK) return rc;
  std::fill(h->ll_fresh.begin(), h->ll_fresh.end(), 1);
  if (fam_ll) std::copy(h->fam_ll.begin(), h->fam_ll.end(), fam_ll);
  return CB_OK;
}
