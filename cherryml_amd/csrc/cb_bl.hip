// libcherrybank: maximum-likelihood branch lengths on fixed trees by EM, on a resident handle (bl.hip.h; include/cherrybank.h,
// cb_bl_*), the nearest-neighbour-interchange scan on the handle's resident messages (nni.hip.h; cb_bl_nni_scan) and the marginal
// ancestral reconstruction from the same messages (anc.hip.h; cb_bl_ancestral) and the local branch supports by resampling the
// scan's per-site log-likelihoods (sup.hip.h; cb_bl_supports) and the best resampled candidate per bootstrap replicate among a
// tree and its NNI neighbours (ufb.hip.h; cb_bl_bootstrap_best) and the subtree prune-and-regraft scan on the same messages
// (spr.hip.h; cb_bl_spr_scan).
// The five calls on the resident messages are built from the same steps, each in one place: the move lists (bl_move_lists, and
// bl_check_moves / bl_spr_record per move), the passes at the current indices (bl_refresh), a timed group of launches (bl_timed),
// the arguments of the scan and of the resampling weights (bl_nni_args, bl_weight_args) and the l_u the passes leave
// (bl_finish).  The two scans share their driver, bl_scan; the supports, the bootstrap and the reconstruction keep their own
// chunking rules and their own middle.
#include "cb_internal.hip.h"
#include "common.hip.h"
#include "bl.hip.h"
#include "nni.hip.h"
#include "spr.hip.h"
#include "anc.hip.h"
#include "sup.hip.h"
#include "ufb.hip.h"
#include "em_host.hip.h"

struct cb_bl_s {
  int T = 0;
  EmForest forest;
  std::vector<size_t> off_cat, off_log;   // per family: cat_ptr, log bank
  std::vector<int> bank_base;             // per family: its first bank entry
  std::vector<int> tau;                   // [sum n_nodes] the current indices (root: -1), the device's mirror
  std::vector<char> fixed, ll_fresh;      // per family: at a fixed point; dll holds l_u at the current indices
  std::vector<double> fam_ll;             // per family: the log-likelihood at the current indices when ll_fresh
  double *dQ = nullptr, *dpi = nullptr, *dP = nullptr, *dlogP = nullptr;
  int *dcat = nullptr, *dtau = nullptr, *dchanged = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

extern "C" int cb_bl_destroy(cb_bl_s *h) {
  if (!h) return CB_OK;
  if (!h->forest.bufs.empty() || h->ev[0]) (void)hipSetDevice(h->forest.device);
  for (hipEvent_t e : h->ev)
    if (e) (void)hipEventDestroy(e);
  h->forest.free_all();
  delete h;
  return CB_OK;
}

extern "C" int cb_bl_create(int device, int S, int T, const double *grid, const double *Q, const double *pi_root, int n_fam,
                            const int *n_nodes, const int *parent, const double *length, const int *n_units,
                            const double *unit_rate, const int8_t *codes, cb_bl_s **out) {
  static const char *who = "cb_bl_create";
  if (!grid || !Q || !pi_root || !n_nodes || !parent || !length || !n_units || !unit_rate || !codes || !out)
    return fail(CB_EINVAL, "cb_bl_create: NULL argument");
  *out = nullptr;
  if (S < 2 || S > 32) return fail(CB_EINVAL, "cb_bl_create: S = %d (2 <= S <= 32: one 32 x 32 MFMA tile per edge)", S);
  if (T < 2) return fail(CB_EINVAL, "cb_bl_create: T = %d (a grid of at least 2 points)", T);
  if (n_fam < 1) return fail(CB_EINVAL, "cb_bl_create: families = %d", n_fam);
  for (int b = 0; b < T; ++b)
    if (!(grid[b] > 0.0) || !std::isfinite(grid[b]) || (b > 0 && !(grid[b] > grid[b - 1])))
      return fail(CB_EINVAL, "cb_bl_create: the grid must be positive and strictly increasing (grid[%d] = %g)", b, grid[b]);
  int rc = em_check_model(who, S, Q, pi_root);
  if (rc != CB_OK) return rc;
  cb_bl_s *h = new cb_bl_s;
  EmForestHost &H = h->forest.host;
  h->forest.device = device; h->forest.S = S; h->T = T;
  h->off_cat.assign(1, 0);
  h->off_log.assign(1, 0);
  const size_t SS = (size_t)S * S;
  size_t entries = 0, max_bank = 0;
  std::vector<int> cat_all;
  for (int f = 0; f < n_fam; ++f) {
    const double *rate = unit_rate + H.off_u[f];
    // rate 0 is a rate of cb_em_create, not of this handle: log expm(0) is no bank entry
    for (int u = 0; u < n_units[f]; ++u)
      if (!(rate[u] > 0.0) || !std::isfinite(rate[u])) {
        rc = fail(CB_EINVAL, "cb_bl_create: family %d: site rate %d = %g (finite and > 0)", f, u, rate[u]);
        break;
      }
    if (rc == CB_OK) rc = em_forest_add(H, who, S, T, grid, n_nodes[f], parent, length, n_units[f], unit_rate, codes);
    const int R = rc == CB_OK ? H.fam[f].n_cats : 0;
    if (rc == CB_OK && R > CB_BL_MAX_CATS)
      rc = fail(CB_EINVAL, "cb_bl_create: family %d has %d distinct site rates (at most %d)", f, R, CB_BL_MAX_CATS);
    if (rc == CB_OK && entries + (size_t)T * R > (size_t)1 << 30)
      rc = fail(CB_EINVAL, "cb_bl_create: %zu bank entries up to family %d (at most 2^30 per handle)", entries + (size_t)T * R, f);
    if (rc != CB_OK) {
      cb_bl_destroy(h);
      return rc;
    }
    const EmFamHost &F = H.fam[f];
    h->bank_base.push_back((int)entries);
    // the input lengths snapped to the grid (the nearest point in ratio, clamped to its ends); the edge's bank entries
    for (int v = 0; v < F.n_nodes; ++v) {
      const int t = v == F.root ? 0 : em_quantize(length[H.off_n[f] + v], grid, T);
      h->tau.push_back(v == F.root ? -1 : t);
      for (int c = 0; c < R; ++c) H.qb[H.off_q[f] + (size_t)v * R + c] = (int)entries + t * R + c;
    }
    cat_all.insert(cat_all.end(), F.cat_ptr.begin(), F.cat_ptr.end());
    entries += (size_t)T * R;
    max_bank = std::max(max_bank, (size_t)T * R);
    h->off_cat.push_back(cat_all.size());
    h->off_log.push_back(h->off_log[f] + (size_t)T * R * SS);
  }
  h->bank_base.push_back((int)entries);
  h->fixed.assign(n_fam, 0);
  h->ll_fresh.assign(n_fam, 0);
  h->fam_ll.assign(n_fam, 0.0);
  // device work from here on
  EmForest &D = h->forest;
  rc = em_open_device(who, device);
  h->dQ = D.alloc(who, Q, SS, rc);
  h->dpi = D.alloc(who, pi_root, S, rc);
  h->dP = D.alloc<double>(who, nullptr, entries * SS, rc);
  h->dlogP = D.alloc<double>(who, nullptr, entries * SS, rc);
  D.upload(who, rc);
  h->dcat = D.alloc(who, cat_all.data(), cat_all.size(), rc);
  h->dtau = D.alloc(who, h->tau.data(), h->tau.size(), rc);
  h->dchanged = D.alloc<int>(who, nullptr, h->tau.size(), rc);
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
    const EmFamHost &F = H.fam[f];
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

static void bl_launch_passes(cb_bl_s *h, int f, bool outside) { em_launch_passes(h->forest, f, h->dP, h->dpi, outside); }

static void bl_launch_mstep(cb_bl_s *h, int f) {
  const EmFamView w = h->forest.view(f);
  if (w.F.n_nodes < 2) return;
  const size_t on = h->forest.host.off_n[f];
  BlArgs a{};
  a.S = h->forest.S; a.T = h->T; a.n_cats = w.F.n_cats; a.n_units = w.F.n_units; a.root = w.F.root; a.bank_base = h->bank_base[f];
  a.parent = w.parent; a.child_ptr = w.child_ptr; a.child_idx = w.child_idx; a.cat_ptr = h->dcat + h->off_cat[f];
  a.codes = w.codes; a.pi_root = h->dpi; a.msg = w.msg; a.U = w.U; a.ll = w.ll; a.P = h->dP; a.logP = h->dlogP + h->off_log[f];
  a.qb = w.qb; a.tau = h->dtau + on; a.changed = h->dchanged + on;
  hipLaunchKernelGGL(bl_mstep_kernel, dim3((unsigned)w.F.n_nodes), dim3(64), 0, 0, a);
}

// l_u of the device -> the caller's unit order; the families in `which` get their sums (a fixed family keeps the one it has)
static int bl_read_ll(cb_bl_s *h, const std::vector<char> &which, std::vector<double> *orig_out) {
  std::vector<double> orig;
  const int rc = em_read_ll(h->forest, which.data(), orig, h->fam_ll.data());
  if (rc == CB_OK && orig_out) orig_out->swap(orig);
  return rc;
}

extern "C" int cb_bl_round(cb_bl_s *h, int *n_changed, double *fam_ll, double *kernel_ms) {
  if (!h) return fail(CB_EINVAL, "cb_bl_round: NULL handle");
  if (!n_changed || !fam_ll) return fail(CB_EINVAL, "cb_bl_round: NULL argument");
  const EmForestHost &H = h->forest.host;
  const int n_fam = H.n_fam();
  HIP_TRY(hipSetDevice(h->forest.device));
  std::vector<char> live(n_fam);
  for (int f = 0; f < n_fam; ++f) live[f] = !h->fixed[f];
  CbKernelTimer timer(kernel_ms != nullptr, h->ev[0], h->ev[2], h->ev[1]);
  int rc = timer.begin(false);
  if (rc != CB_OK) return rc;
  for (int f = 0; f < n_fam; ++f)
    if (live[f]) bl_launch_passes(h, f, true);
  if ((rc = timer.lap()) != CB_OK) return rc;
  for (int f = 0; f < n_fam; ++f)
    if (live[f]) bl_launch_mstep(h, f);
  if ((rc = timer.end(kernel_ms)) != CB_OK) return rc;
  HIP_TRY(hipGetLastError());
  // a fixed family keeps the sum of the round that found its fixed point: the same lengths, the same bits
  if ((rc = bl_read_ll(h, live, nullptr)) != CB_OK) return rc;
  std::vector<int> flags(h->tau.size());
  HIP_TRY(hipMemcpy(flags.data(), h->dchanged, flags.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->tau.data(), h->dtau, h->tau.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int f = 0; f < n_fam; ++f) {
    fam_ll[f] = h->fam_ll[f];
    n_changed[f] = 0;
    if (!live[f]) continue;
    const EmFamHost &F = H.fam[f];
    for (int v = 0; v < F.n_nodes; ++v)
      if (v != F.root) n_changed[f] += flags[H.off_n[f] + v] != 0;
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
  HIP_TRY(hipSetDevice(h->forest.device));
  const int n_fam = h->forest.host.n_fam();
  std::vector<char> stale(n_fam);
  for (int f = 0; f < n_fam; ++f) {
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

// the triples of family f, on the host: what cb_bl_nni_scan and cb_bl_supports refuse, in these words
static int bl_check_moves(const char *who, const EmForestHost &H, int f, int n_moves, const int *moves) {
  const EmFamHost &F = H.fam[f];
  const int n = F.n_nodes, *par = H.parent.data() + H.off_n[f];
  for (int m = 0; m < n_moves; ++m) {
    const int *t = moves + 3 * (size_t)m;
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
  return CB_OK;
}

// ---- the steps that the calls on the resident messages share (the scans, the supports, the bootstrap, the reconstruction) ----

// The move lists of a call: refuses a negative count and, where there is a move, NULL `moves`.  off_m: per family its first
// move (and the total); has: per family whether it has a move.
static int bl_move_lists(const char *who, const EmForestHost &H, const int *n_moves, const int *moves, std::vector<size_t> &off_m,
                         std::vector<char> &has) {
  const int n_fam = H.n_fam();
  off_m.assign(n_fam + 1, 0);
  has.assign(n_fam, 0);
  for (int f = 0; f < n_fam; ++f) {
    if (n_moves[f] < 0) return fail(CB_EINVAL, "%s: family %d: n_moves = %d", who, f, n_moves[f]);
    off_m[f + 1] = off_m[f] + n_moves[f];
    has[f] = n_moves[f] > 0;
  }
  if (off_m[n_fam] > 0 && !moves) return fail(CB_EINVAL, "%s: NULL argument", who);
  return CB_OK;
}

// The kernels `launch(timer)` enqueues, under the handle's events: their time is added to kernel_ms[slot] and, where launch
// calls timer.lap(), the time of what follows the lap to kernel_ms[slot + 1].  kernel_ms NULL: no event and no wait.
template <typename Launch>
static int bl_timed(cb_bl_s *h, double *kernel_ms, int slot, Launch &&launch) {
  CbKernelTimer timer(kernel_ms != nullptr, h->ev[0], h->ev[2], h->ev[1]);
  double ms[2] = {0.0, 0.0};
  int rc = timer.begin(false);
  if (rc != CB_OK) return rc;
  if ((rc = launch(timer)) != CB_OK) return rc;
  HIP_TRY(hipGetLastError());
  if ((rc = timer.end(ms)) != CB_OK) return rc;
  if (kernel_ms) kernel_ms[slot] += ms[0];
  if (timer.lapped) kernel_ms[slot + 1] += ms[1];   // (lapped: only with kernel_ms)
  return CB_OK;
}

// The messages and l_u of the families in `which` at the current indices, their time in kernel_ms[0] (zeroed by the caller):
// after a round the resident ones are its start's.
static int bl_refresh(cb_bl_s *h, const std::vector<char> &which, double *kernel_ms) {
  HIP_TRY(hipSetDevice(h->forest.device));
  return bl_timed(h, kernel_ms, 0, [&](CbKernelTimer &) -> int {
    for (size_t f = 0; f < which.size(); ++f)
      if (which[f]) bl_launch_passes(h, (int)f, true);
    return CB_OK;
  });
}

// After bl_refresh(which) and the call's own kernels: dll of those families holds l_u at the current indices -- the bits
// cb_bl_get's inside pass would write -- so the stale ones among them get their sums and are fresh.  fam_ll (or NULL) takes
// every family's sum, NaN for one that is still not fresh.
static int bl_finish(cb_bl_s *h, const std::vector<char> &which, double *fam_ll) {
  const int n_fam = h->forest.host.n_fam();
  std::vector<char> stale(n_fam);
  bool any = false;
  for (int f = 0; f < n_fam; ++f) {
    stale[f] = which[f] && !h->ll_fresh[f];
    any = any || which[f];
  }
  if (any) {
    const int rc = bl_read_ll(h, stale, nullptr);
    if (rc != CB_OK) return rc;
    for (int f = 0; f < n_fam; ++f)
      if (stale[f]) h->ll_fresh[f] = 1;
  }
  if (fam_ll)
    for (int f = 0; f < n_fam; ++f) fam_ll[f] = h->ll_fresh[f] ? h->fam_ll[f] : std::nan("");
  return CB_OK;
}

// nni_scan_kernel's and nni_sum_kernel's arguments for a family, but the chunk's moves and delta
static NniArgs bl_nni_args(const cb_bl_s *h, const EmFamView &w, double *out) {
  NniArgs a{};
  a.S = h->forest.S; a.n_units = w.F.n_units; a.n_cats = w.F.n_cats; a.root = w.F.root; a.n_blocks = w.n_blocks;
  a.parent = w.parent; a.child_ptr = w.child_ptr; a.child_idx = w.child_idx; a.qb = w.qb; a.unit_cat = w.unit_cat; a.P = h->dP;
  a.pi_root = h->dpi; a.msg = w.msg; a.U = w.U; a.ll = w.ll; a.out = out;
  return a;
}

// sup_weights_kernel's arguments for a family: its inverse permutation, uploaded to dinv (inv: host room for it), and its seed
static int bl_weight_args(const EmFamHost &F, uint64_t seed, std::vector<int> &inv, int *dinv, double *dW, SupWeightArgs &wa) {
  for (int k = 0; k < F.n_units; ++k) inv[F.perm[k]] = k;
  HIP_TRY(hipMemcpy(dinv, inv.data(), (size_t)F.n_units * sizeof(int), hipMemcpyHostToDevice));
  wa = SupWeightArgs{};
  wa.n_units = F.n_units; wa.k0 = (uint32_t)(seed & 0xFFFFFFFFu); wa.k1 = (uint32_t)(seed >> 32); wa.inv = dinv; wa.W = dW;
  return CB_OK;
}

constexpr size_t SCAN_LL_BYTES = (size_t)256 << 20;   // ll'[move][unit] of one chunk of moves, at most (one move always goes); the
                                                      // test hooks CB_NNI_LL_BYTES and CB_SPR_LL_BYTES: the results do not
                                                      // depend on the chunking

// The driver of cb_bl_nni_scan and cb_bl_spr_scan, after their checks.  hook: the name of the byte bound's test hook; rows:
// per move (off_m) `width` ints, what the scan kernel reads of it; launch(f, w, drows, dout, ddelta, nm): enqueues the scan
// kernel and nni_sum_kernel for nm moves of family f with view w, whose rows, ll' and deltas start at the three device pointers.
template <typename Launch>
static int bl_scan(cb_bl_s *h, const char *hook, const int *n_moves, const std::vector<size_t> &off_m, const std::vector<char> &has,
                   const int *rows, size_t width, Launch &&launch, double *delta, double *ll_moves, double *fam_ll,
                   double *kernel_ms) {
  const EmForestHost &H = h->forest.host;
  const int n_fam = H.n_fam(), S = h->forest.S;
  // moves per launch: all of a family's, fewer under the byte bound and where moves x site tiles would pass 2^31
  size_t max_moves = 0, max_out = 0;
  std::vector<int> chunk(n_fam, 0);
  const size_t bound = cb_hook_bytes(hook, SCAN_LL_BYTES);
  for (int f = 0; f < n_fam; ++f) {
    if (!has[f]) continue;
    const EmFamHost &F = H.fam[f];
    const size_t n_blocks = ((size_t)F.n_units + 64 / S - 1) / (64 / S);
    const size_t fit = std::min(bound / ((size_t)F.n_units * sizeof(double)), (size_t)INT32_MAX / n_blocks);
    chunk[f] = (int)std::min<size_t>(n_moves[f], std::max<size_t>(fit, 1));
    max_moves = std::max(max_moves, (size_t)n_moves[f]);
    max_out = std::max(max_out, (size_t)chunk[f] * F.n_units);
  }
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
  if (max_moves > 0) {
    int rc = bl_refresh(h, has, kernel_ms);
    if (rc != CB_OK) return rc;
    std::vector<double> host_out(ll_moves ? max_out : 0);
    CbDevBufs bufs;   // this call's: freed on every return path
    int *drows = bufs.up<int>(nullptr, width * max_moves, rc);
    double *dout = bufs.up<double>(nullptr, max_out, rc), *ddelta = bufs.up<double>(nullptr, max_moves, rc);
    if (rc != CB_OK) return rc;
    size_t off_o = 0;   // the family's first ll' in ll_moves
    for (int f = 0; f < n_fam; ++f) {
      if (!has[f]) continue;
      const EmFamView w = h->forest.view(f);
      const int U = w.F.n_units;
      HIP_TRY(hipMemcpy(drows, rows + width * off_m[f], width * n_moves[f] * sizeof(int), hipMemcpyHostToDevice));
      for (int m0 = 0; m0 < n_moves[f]; m0 += chunk[f]) {
        const int nm = std::min(chunk[f], n_moves[f] - m0);
        rc = bl_timed(h, kernel_ms, 1, [&](CbKernelTimer &) -> int {
          launch(f, w, drows + width * m0, dout, ddelta + m0, nm);
          return CB_OK;
        });
        if (rc != CB_OK) return rc;
        // (the next chunk writes the same buffer: stream order puts it behind this chunk's sum)
        if (ll_moves) {   // device (category) order -> the caller's unit order
          HIP_TRY(hipMemcpy(host_out.data(), dout, (size_t)nm * U * sizeof(double), hipMemcpyDeviceToHost));
          double *dst = ll_moves + off_o + (size_t)m0 * U;
          for (int m = 0; m < nm; ++m) em_unpermute(w.F.perm, host_out.data() + (size_t)m * U, dst + (size_t)m * U);
        }
      }
      HIP_TRY(hipMemcpy(delta + off_m[f], ddelta, (size_t)n_moves[f] * sizeof(double), hipMemcpyDeviceToHost));
      off_o += (size_t)n_moves[f] * U;
    }
  }
  return bl_finish(h, has, fam_ll);
}

extern "C" int cb_bl_nni_scan(cb_bl_s *h, const int *n_moves, const int *moves, double *delta, double *ll_moves, double *fam_ll,
                              double *kernel_ms) {
  static const char *who = "cb_bl_nni_scan";
  if (!h) return fail(CB_EINVAL, "%s: NULL handle", who);
  if (!n_moves || !delta) return fail(CB_EINVAL, "%s: NULL argument", who);
  // every triple, on the host, before any device work
  const EmForestHost &H = h->forest.host;
  std::vector<size_t> off_m;
  std::vector<char> has;
  int rc = bl_move_lists(who, H, n_moves, moves, off_m, has);
  for (int f = 0; f < H.n_fam() && rc == CB_OK; ++f) rc = bl_check_moves(who, H, f, n_moves[f], moves + 3 * off_m[f]);
  if (rc != CB_OK) return rc;
  auto launch = [h](int, const EmFamView &w, const int *dmoves, double *dout, double *ddelta, int nm) {
    NniArgs a = bl_nni_args(h, w, dout);
    a.moves = dmoves; a.delta = ddelta;
    hipLaunchKernelGGL(nni_scan_kernel, dim3((unsigned)nm * (unsigned)a.n_blocks), dim3(64), 0, 0, a);
    hipLaunchKernelGGL(nni_sum_kernel, dim3((unsigned)nm), dim3(64), 0, 0, a);
  };
  return bl_scan(h, "CB_NNI_LL_BYTES", n_moves, off_m, has, moves, 3, launch, delta, ll_moves, fam_ll, kernel_ms);
}

// Move m of family f, (x, y, tau_s, tau_p, tau_y), on the host: what cb_bl_spr_scan refuses, and the move's step record for
// spr_scan_kernel (spr.hip.h).  tau: the family's current indices; pos: n_nodes entries of -1, left so.
static int bl_spr_record(const char *who, const EmForestHost &H, int f, int m, const int *mv, const int *tau, int T,
                         std::vector<int> &pos, int *rec) {
  const EmFamHost &F = H.fam[f];
  const int n = F.n_nodes, *par = H.parent.data() + H.off_n[f];
  const int x = mv[0], y = mv[1];
  if (x < 0 || x >= n) return fail(CB_EINVAL, "%s: family %d move %d: x = %d (0 <= index < %d)", who, f, m, x, n);
  if (y < 0 || y >= n) return fail(CB_EINVAL, "%s: family %d move %d: y = %d (0 <= index < %d)", who, f, m, y, n);
  if (x == F.root) return fail(CB_EINVAL, "%s: family %d move %d: x = %d is the root", who, f, m, x);
  const int p = par[x];
  if (p == F.root) return fail(CB_EINVAL, "%s: family %d move %d: p = parent[x] = %d is the root", who, f, m, p);
  const int np = F.child_ptr[p + 1] - F.child_ptr[p];
  if (np != 2) return fail(CB_EINVAL, "%s: family %d move %d: p = parent[x] = %d has %d children (exactly 2)", who, f, m, p, np);
  const int c0 = F.child_idx[F.child_ptr[p]], s = c0 != x ? c0 : F.child_idx[F.child_ptr[p] + 1], g = par[p];
  if (y == F.root) return fail(CB_EINVAL, "%s: family %d move %d: y = %d is the root", who, f, m, y);
  if (y == x) return fail(CB_EINVAL, "%s: family %d move %d: y = %d equals x", who, f, m, y);
  if (y == p) return fail(CB_EINVAL, "%s: family %d move %d: y = %d equals p = parent[x]", who, f, m, y);
  if (y == s) return fail(CB_EINVAL, "%s: family %d move %d: y = %d equals s, the other child of parent[x]", who, f, m, y);
  static const char *names[3] = {"tau_s", "tau_p", "tau_y"};
  for (int k = 0; k < 3; ++k)
    if (mv[2 + k] < 0 || mv[2 + k] >= T)
      return fail(CB_EINVAL, "%s: family %d move %d: %s = %d (0 <= index < %d)", who, f, m, names[k], mv[2 + k], T);
  // y and its ancestors up to s, x or the root
  std::vector<int> chain;
  for (int w = y; w >= 0 && w != x; w = w == s ? -1 : par[w]) chain.push_back(w);
  const int top = chain.back();
  if (top != s && top != F.root) return fail(CB_EINVAL, "%s: family %d move %d: y = %d lies in the subtree of x = %d", who, f, m, y, x);
  auto is_leaf = [&](int w) { return F.child_ptr[w] == F.child_ptr[w + 1]; };
  auto step = [&](int i, int op, int t, int node, int ex1, int ex2, int flags) {
    int *st = rec + SPR_HEAD + SPR_STEP * i;
    st[0] = op, st[1] = t, st[2] = node, st[3] = ex1, st[4] = ex2, st[5] = flags;
  };
  std::fill(rec, rec + SPR_REC, 0);
  int d = 0;
  if (top == s) {   // below s: s = z0, ..., zd = y
    d = (int)chain.size() - 1;
    if (d > CB_SPR_MAX_RADIUS)
      return fail(CB_EINVAL, "%s: family %d move %d: y = %d is at distance %d of x = %d (at most %d)", who, f, m, y, d, x, CB_SPR_MAX_RADIUS);
    step(0, SPR_NONE, 0, g, p, -1, SPR_ADD_U);
    for (int i = 1; i <= d; ++i) {
      const int z = chain[d - i + 1];
      step(i, SPR_DOWN, i == 1 ? mv[2] : tau[z], z, chain[d - i], -1, 0);
    }
    step(d + 1, 0, 0, y, -1, -1, is_leaf(y) ? SPR_LEAF : 0);
  } else {          // through g: up k ancestors of g to the first that is y or above it, then down j nodes to y
    for (size_t i = 0; i < chain.size(); ++i) pos[chain[i]] = (int)i;
    std::vector<int> anc(1, g);
    while (pos[anc.back()] < 0) anc.push_back(par[anc.back()]);
    const int k = (int)anc.size() - 1, j = pos[anc.back()];
    for (int w : chain) pos[w] = -1;
    d = k + 1 + std::max(j - 1, 0);
    if (d > CB_SPR_MAX_RADIUS)
      return fail(CB_EINVAL, "%s: family %d move %d: y = %d is at distance %d of x = %d (at most %d)", who, f, m, y, d, x, CB_SPR_MAX_RADIUS);
    const int z1 = j > 0 ? chain[j - 1] : -1;
    step(0, SPR_NONE, 0, s, -1, -1, is_leaf(s) ? SPR_LEAF : 0);
    for (int i = 1; i <= k + 1; ++i) {
      const bool turn = i == k + 1 && j > 0;   // the outside of z1: U of the top and all it holds but z1
      step(i, SPR_UP, i == 1 ? mv[2] : tau[anc[i - 2]], anc[i - 1], i == 1 ? p : anc[i - 2], turn ? z1 : -1, turn ? SPR_ADD_U : 0);
    }
    for (int i = 1; i < j; ++i) step(k + 1 + i, SPR_DOWN, tau[chain[j - i]], chain[j - i], chain[j - i - 1], -1, 0);
    if (j == 0) step(d + 1, 1, 0, par[y], y, -1, SPR_ADD_U);
    else step(d + 1, 0, 0, y, -1, -1, is_leaf(y) ? SPR_LEAF : 0);
  }
  rec[0] = d + 1, rec[1] = x, rec[2] = mv[3], rec[3] = mv[4];
  return CB_OK;
}

extern "C" int cb_bl_spr_scan(cb_bl_s *h, const int *n_moves, const int *moves, double *delta, double *ll_moves, double *fam_ll,
                              double *kernel_ms) {
  static const char *who = "cb_bl_spr_scan";
  if (!h) return fail(CB_EINVAL, "%s: NULL handle", who);
  if (!n_moves || !delta) return fail(CB_EINVAL, "%s: NULL argument", who);
  // every move, on the host, before any device work: its checks and its step record
  const EmForestHost &H = h->forest.host;
  std::vector<size_t> off_m;
  std::vector<char> has;
  int rc = bl_move_lists(who, H, n_moves, moves, off_m, has);
  if (rc != CB_OK) return rc;
  std::vector<int> pos, recs(off_m.back() * SPR_REC);
  for (int f = 0; f < H.n_fam(); ++f) {
    pos.assign(H.fam[f].n_nodes, -1);
    for (int m = 0; m < n_moves[f]; ++m) {
      rc = bl_spr_record(who, H, f, m, moves + 5 * (off_m[f] + m), h->tau.data() + H.off_n[f], h->T, pos,
                         recs.data() + (off_m[f] + m) * SPR_REC);
      if (rc != CB_OK) return rc;
    }
  }
  auto launch = [h](int f, const EmFamView &w, const int *drec, double *dout, double *ddelta, int nm) {
    const EmFamHost &F = w.F;
    SprArgs a{};
    a.S = h->forest.S; a.n_units = F.n_units; a.n_cats = F.n_cats; a.root = F.root; a.n_blocks = w.n_blocks; a.bank_base = h->bank_base[f];
    a.child_ptr = w.child_ptr; a.child_idx = w.child_idx; a.unit_cat = w.unit_cat; a.codes = w.codes; a.P = h->dP;
    a.pi_root = h->dpi; a.msg = w.msg; a.U = w.U; a.out = dout; a.rec = drec;
    NniArgs b{};      // nni_sum_kernel's fields
    b.n_units = F.n_units; b.ll = w.ll; b.out = dout; b.delta = ddelta;
    hipLaunchKernelGGL(spr_scan_kernel, dim3((unsigned)nm * (unsigned)a.n_blocks), dim3(64), 0, 0, a);
    hipLaunchKernelGGL(nni_sum_kernel, dim3((unsigned)nm), dim3(64), 0, 0, b);
  };
  return bl_scan(h, "CB_SPR_LL_BYTES", n_moves, off_m, has, recs.data(), SPR_REC, launch, delta, ll_moves, fam_ll, kernel_ms);
}

constexpr size_t SUP_BYTES = (size_t)256 << 20;   // ll'[move][unit] and C[move][replicate] of one chunk of whole groups, at most (one
                                                  // group always goes); the test hook CB_SUP_BYTES: the results do not depend on it
constexpr int SUP_MAX_REP = 65536;

extern "C" int cb_bl_supports(cb_bl_s *h, int n_rep, const uint64_t *seeds, const int *n_moves, const int *moves, double *alrt,
                              int *sh_count, int *rell_count, double *delta_rep, double *fam_ll, double *kernel_ms) {
  static const char *who = "cb_bl_supports";
  if (!h) return fail(CB_EINVAL, "%s: NULL handle", who);
  if (!n_moves || !seeds) return fail(CB_EINVAL, "%s: NULL argument", who);
  if (n_rep < 1 || n_rep > SUP_MAX_REP) return fail(CB_EINVAL, "%s: n_rep = %d (1 <= replicates <= %d)", who, n_rep, SUP_MAX_REP);
  // every triple and the grouping, on the host, before any device work
  const EmForestHost &H = h->forest.host;
  const int n_fam = H.n_fam(), S = h->forest.S;
  std::vector<size_t> off_m, off_g(n_fam + 1, 0);
  std::vector<char> has;
  int rc = bl_move_lists(who, H, n_moves, moves, off_m, has);
  if (rc != CB_OK) return rc;
  std::vector<int> group_ptr;                    // per family its groups' first moves and the end, within the family
  std::vector<size_t> off_gp(n_fam + 1, 0);      // ... where they start in group_ptr
  std::vector<std::vector<int>> cuts(n_fam);     // per family the groups at which its chunks start, and the end
  const size_t bound = cb_hook_bytes("CB_SUP_BYTES", SUP_BYTES);
  const size_t rep_tiles = ((size_t)n_rep + 63) / 64;
  size_t max_moves = 0, max_chunk = 0, max_out = 0, max_groups = 0, max_units = 0;
  for (int f = 0; f < n_fam; ++f) {
    const EmFamHost &F = H.fam[f];
    const int *mv = moves + 3 * off_m[f];
    if ((rc = bl_check_moves(who, H, f, n_moves[f], mv)) != CB_OK) return rc;
    std::vector<char> seen(F.n_nodes, 0);
    for (int m = 0; m < n_moves[f]; ++m) {
      const int v = mv[3 * (size_t)m];
      if (m > 0 && v == mv[3 * (size_t)(m - 1)]) continue;
      if (seen[v])
        return fail(CB_EINVAL, "%s: family %d move %d: v = %d comes back after another edge's moves (the moves of an edge must be "
                    "consecutive)", who, f, m, v);
      seen[v] = 1;
      group_ptr.push_back(m);
    }
    group_ptr.push_back(n_moves[f]);
    off_gp[f + 1] = group_ptr.size();
    const size_t n_groups = off_gp[f + 1] - off_gp[f] - 1;
    off_g[f + 1] = off_g[f] + n_groups;
    if (!has[f]) continue;
    // chunks of whole groups: the byte bound, and the tiles of the scan's and the product's launches below 2^31
    const int *gp = group_ptr.data() + off_gp[f];
    const size_t n_blocks = ((size_t)F.n_units + 64 / S - 1) / (64 / S);
    const size_t fit = std::min({bound / (((size_t)F.n_units + n_rep) * sizeof(double)), (size_t)INT32_MAX / n_blocks,
                                 16 * ((size_t)INT32_MAX / rep_tiles - 1)});
    for (size_t g = 0; g < n_groups;) {
      cuts[f].push_back((int)g);
      size_t e = g + 1;
      while (e < n_groups && (size_t)(gp[e + 1] - gp[g]) <= fit) ++e;
      const size_t nm = gp[e] - gp[g];
      if (nm * n_blocks > (size_t)INT32_MAX || (nm + 15) / 16 * rep_tiles > (size_t)INT32_MAX)
        return fail(CB_EINVAL, "%s: family %d: the %zu moves of the edge above v = %d need more than 2^31 - 1 tiles in one launch",
                    who, f, nm, mv[3 * (size_t)gp[g]]);
      max_chunk = std::max(max_chunk, nm);
      max_out = std::max(max_out, nm * F.n_units);
      g = e;
    }
    cuts[f].push_back((int)n_groups);
    max_moves = std::max(max_moves, (size_t)n_moves[f]);
    max_groups = std::max(max_groups, n_groups);
    max_units = std::max(max_units, (size_t)F.n_units);
  }
  if (off_g[n_fam] > 0 && (!alrt || !sh_count || !rell_count)) return fail(CB_EINVAL, "%s: NULL argument", who);
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.0;
  if (max_moves > 0) {
    if ((rc = bl_refresh(h, has, kernel_ms)) != CB_OK) return rc;
    std::vector<int> inv(max_units);
    CbDevBufs bufs;   // this call's: freed on every return path
    int *dmoves = bufs.up<int>(nullptr, 3 * max_moves, rc), *dgp = bufs.up<int>(nullptr, max_groups + 1, rc);
    int *dinv = bufs.up<int>(nullptr, max_units, rc);
    double *dout = bufs.up<double>(nullptr, max_out, rc), *ddelta = bufs.up<double>(nullptr, max_moves, rc);
    double *dW = bufs.up<double>(nullptr, (size_t)n_rep * max_units, rc), *dC = bufs.up<double>(nullptr, max_chunk * n_rep, rc);
    double *dalrt = bufs.up<double>(nullptr, max_groups, rc);
    int *dsh = bufs.up<int>(nullptr, max_groups, rc), *drell = bufs.up<int>(nullptr, max_groups, rc);
    if (rc != CB_OK) return rc;
    for (int f = 0; f < n_fam; ++f) {
      if (!has[f]) continue;
      const EmFamView w = h->forest.view(f);
      const int U = w.F.n_units, *gp = group_ptr.data() + off_gp[f];
      const size_t n_groups = off_g[f + 1] - off_g[f];
      HIP_TRY(hipMemcpy(dmoves, moves + 3 * off_m[f], 3 * (size_t)n_moves[f] * sizeof(int), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(dgp, gp, (n_groups + 1) * sizeof(int), hipMemcpyHostToDevice));
      // the multiplicities of every replicate, once per family: every edge resamples the same sites
      SupWeightArgs wa;
      if ((rc = bl_weight_args(w.F, seeds[f], inv, dinv, dW, wa)) != CB_OK) return rc;
      rc = bl_timed(h, kernel_ms, 2, [&](CbKernelTimer &) -> int {
        hipLaunchKernelGGL(sup_weights_kernel, dim3((unsigned)n_rep), dim3(256), 0, 0, wa);
        return CB_OK;
      });
      if (rc != CB_OK) return rc;
      NniArgs a = bl_nni_args(h, w, dout);
      for (size_t ci = 0; ci + 1 < cuts[f].size(); ++ci) {
        const int g0 = cuts[f][ci], g1 = cuts[f][ci + 1], m0 = gp[g0], nm = gp[g1] - m0;
        a.moves = dmoves + 3 * (size_t)m0;
        a.delta = ddelta + m0;
        SupGemmArgs ga{};
        ga.n_moves = nm; ga.n_rep = n_rep; ga.n_units = U; ga.out = dout; ga.ll = w.ll; ga.W = dW; ga.C = dC;
        SupEdgeArgs ea{};
        ea.n_rep = n_rep; ea.move0 = m0; ea.group_ptr = dgp + g0; ea.delta = a.delta; ea.C = dC;
        ea.alrt = dalrt + g0; ea.sh_count = dsh + g0; ea.rell_count = drell + g0;
        rc = bl_timed(h, kernel_ms, 1, [&](CbKernelTimer &timer) -> int {
          hipLaunchKernelGGL(nni_scan_kernel, dim3((unsigned)nm * (unsigned)a.n_blocks), dim3(64), 0, 0, a);
          hipLaunchKernelGGL(nni_sum_kernel, dim3((unsigned)nm), dim3(64), 0, 0, a);
          const int rc_lap = timer.lap();
          if (rc_lap != CB_OK) return rc_lap;
          hipLaunchKernelGGL(sup_gemm_kernel, dim3((unsigned)(((size_t)nm + 15) / 16 * rep_tiles)), dim3(256), 0, 0, ga, (int)rep_tiles);
          hipLaunchKernelGGL(sup_edge_kernel, dim3((unsigned)(g1 - g0)), dim3(256), 0, 0, ea);
          return CB_OK;
        });
        if (rc != CB_OK) return rc;
        // (the next chunk writes the same buffers: stream order puts it behind this chunk's kernels and this copy)
        if (delta_rep)
          HIP_TRY(hipMemcpy(delta_rep + (off_m[f] + m0) * n_rep, dC, (size_t)nm * n_rep * sizeof(double), hipMemcpyDeviceToHost));
      }
      HIP_TRY(hipMemcpy(alrt + off_g[f], dalrt, n_groups * sizeof(double), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(sh_count + off_g[f], dsh, n_groups * sizeof(int), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(rell_count + off_g[f], drell, n_groups * sizeof(int), hipMemcpyDeviceToHost));
    }
  }
  return bl_finish(h, has, fam_ll);
}

constexpr size_t UFB_BYTES = (size_t)256 << 20;   // ll'[move][unit] of one chunk of moves, at most (one tile of 16 moves always
                                                  // goes); the test hook CB_UFB_BYTES: the results do not depend on the chunking
constexpr int UFB_WORKGROUPS = 1024;              // the product's launch aims at this many workgroups: four per CU

extern "C" int cb_bl_bootstrap_best(cb_bl_s *h, int n_rep, const uint64_t *seeds, const int *n_moves, const int *moves,
                                    double *best_score, int *best_code, double *base, double *fam_ll, double *kernel_ms) {
  static const char *who = "cb_bl_bootstrap_best";
  if (!h) return fail(CB_EINVAL, "%s: NULL handle", who);
  if (!n_moves || !seeds || !best_score || !best_code) return fail(CB_EINVAL, "%s: NULL argument", who);
  if (n_rep < 1 || n_rep > SUP_MAX_REP) return fail(CB_EINVAL, "%s: n_rep = %d (1 <= replicates <= %d)", who, n_rep, SUP_MAX_REP);
  // every triple and every incoming score, on the host, before any device work
  const EmForestHost &H = h->forest.host;
  const int n_fam = H.n_fam(), S = h->forest.S;
  std::vector<size_t> off_m;
  std::vector<char> has;
  int rc = bl_move_lists(who, H, n_moves, moves, off_m, has);
  if (rc != CB_OK) return rc;
  const size_t bound = cb_hook_bytes("CB_UFB_BYTES", UFB_BYTES);
  const int rep_tiles = (n_rep + UFB_RT - 1) / UFB_RT;
  std::vector<int> chunk(n_fam, 0);
  size_t max_moves = 0, max_out = 0, max_units = 0, max_slices = 1;
  for (int f = 0; f < n_fam; ++f) {
    const EmFamHost &F = H.fam[f];
    if ((rc = bl_check_moves(who, H, f, n_moves[f], moves + 3 * off_m[f])) != CB_OK) return rc;
    for (int r = 0; r < n_rep; ++r)
      if (std::isnan(best_score[(size_t)f * n_rep + r]))
        return fail(CB_EINVAL, "%s: family %d replicate %d: the incoming best score is NaN", who, f, r);
    max_units = std::max(max_units, (size_t)F.n_units);
    if (!has[f]) continue;
    // chunks of whole move tiles: the byte bound, and the scan's launch below 2^31 blocks
    const size_t n_blocks = ((size_t)F.n_units + 64 / S - 1) / (64 / S);
    const size_t fit = std::max<size_t>(bound / ((size_t)F.n_units * sizeof(double)) / 16 * 16, 16);
    const size_t launch = (size_t)INT32_MAX / n_blocks;
    if (launch < 1) return fail(CB_EINVAL, "%s: family %d: %zu site tiles (at most 2^31 - 1 per launch)", who, f, n_blocks);
    chunk[f] = (int)std::min<size_t>(n_moves[f], std::min(fit, launch));
    max_moves = std::max(max_moves, (size_t)n_moves[f]);
    max_out = std::max(max_out, (size_t)chunk[f] * F.n_units);
    max_slices = std::max(max_slices, std::min<size_t>(((size_t)chunk[f] + 15) / 16, std::max(1, UFB_WORKGROUPS / rep_tiles)));
  }
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.0;
  const std::vector<char> all(n_fam, 1);   // a family with no move still scores its tree
  if ((rc = bl_refresh(h, all, kernel_ms)) != CB_OK) return rc;
  std::vector<int> inv(max_units);
  CbDevBufs bufs;   // this call's: freed on every return path
  int *dmoves = bufs.up<int>(nullptr, 3 * max_moves, rc), *dinv = bufs.up<int>(nullptr, max_units, rc);
  double *dout = bufs.up<double>(nullptr, max_out, rc), *ddelta = bufs.up<double>(nullptr, max_moves, rc);
  double *dW = bufs.up<double>(nullptr, (size_t)n_rep * max_units, rc), *dbase = bufs.up<double>(nullptr, n_rep, rc);
  double *dpart = bufs.up<double>(nullptr, max_slices * n_rep, rc), *dbest = bufs.up<double>(nullptr, n_rep, rc);
  int *dpcode = bufs.up<int>(nullptr, max_slices * n_rep, rc), *dcode = bufs.up<int>(nullptr, n_rep, rc);
  if (rc != CB_OK) return rc;
  for (int f = 0; f < n_fam; ++f) {
    const EmFamView w = h->forest.view(f);
    const int U = w.F.n_units;
    if (has[f]) HIP_TRY(hipMemcpy(dmoves, moves + 3 * off_m[f], 3 * (size_t)n_moves[f] * sizeof(int), hipMemcpyHostToDevice));
    // the multiplicities of every replicate, once per family, and the tree's own resampled log-likelihood
    SupWeightArgs wa;
    if ((rc = bl_weight_args(w.F, seeds[f], inv, dinv, dW, wa)) != CB_OK) return rc;
    HIP_TRY(hipMemcpy(dbest, best_score + (size_t)f * n_rep, (size_t)n_rep * sizeof(double), hipMemcpyHostToDevice));
    UfbGemmArgs ga{};
    ga.n_rep = n_rep; ga.n_units = U; ga.out = dout; ga.ll = w.ll; ga.W = dW; ga.base = dbase; ga.part_score = dpart;
    ga.part_code = dpcode;
    UfbMergeArgs ma{};
    ma.n_rep = n_rep; ma.first = 1; ma.base = dbase; ma.part_score = dpart; ma.part_code = dpcode; ma.best_score = dbest;
    ma.best_code = dcode;
    const unsigned merge_grid = (unsigned)((n_rep + 255) / 256);
    rc = bl_timed(h, kernel_ms, 2, [&](CbKernelTimer &) -> int {
      hipLaunchKernelGGL(sup_weights_kernel, dim3((unsigned)n_rep), dim3(256), 0, 0, wa);
      hipLaunchKernelGGL(ufb_gemm_kernel<true>, dim3((unsigned)rep_tiles), dim3(256), 0, 0, ga, rep_tiles);
      if (!has[f]) hipLaunchKernelGGL(ufb_merge_kernel, dim3(merge_grid), dim3(256), 0, 0, ma);   // the tree against the incoming best
      return CB_OK;
    });
    if (rc != CB_OK) return rc;
    NniArgs a = bl_nni_args(h, w, dout);
    for (int m0 = 0; m0 < n_moves[f]; m0 += chunk[f]) {
      const int nm = std::min(chunk[f], n_moves[f] - m0);
      a.moves = dmoves + 3 * (size_t)m0;
      a.delta = ddelta + m0;
      ga.n_moves = nm; ga.move0 = m0; ga.delta = a.delta; ga.n_tiles = (nm + 15) / 16;
      ga.n_slices = std::min(ga.n_tiles, std::max(1, UFB_WORKGROUPS / rep_tiles));
      ma.n_slices = ga.n_slices; ma.first = m0 == 0;
      rc = bl_timed(h, kernel_ms, 1, [&](CbKernelTimer &timer) -> int {
        hipLaunchKernelGGL(nni_scan_kernel, dim3((unsigned)nm * (unsigned)a.n_blocks), dim3(64), 0, 0, a);
        hipLaunchKernelGGL(nni_sum_kernel, dim3((unsigned)nm), dim3(64), 0, 0, a);
        const int rc_lap = timer.lap();
        if (rc_lap != CB_OK) return rc_lap;
        hipLaunchKernelGGL(ufb_gemm_kernel<false>, dim3((unsigned)(ga.n_slices * rep_tiles)), dim3(256), 0, 0, ga, rep_tiles);
        hipLaunchKernelGGL(ufb_merge_kernel, dim3(merge_grid), dim3(256), 0, 0, ma);
        return CB_OK;
      });
      if (rc != CB_OK) return rc;
      // (the next chunk writes the same buffers: stream order puts it behind this chunk's kernels)
    }
    HIP_TRY(hipMemcpy(best_score + (size_t)f * n_rep, dbest, (size_t)n_rep * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(best_code + (size_t)f * n_rep, dcode, (size_t)n_rep * sizeof(int), hipMemcpyDeviceToHost));
    if (base) HIP_TRY(hipMemcpy(base + (size_t)f * n_rep, dbase, (size_t)n_rep * sizeof(double), hipMemcpyDeviceToHost));
  }
  return bl_finish(h, all, fam_ll);
}

constexpr size_t ANC_POST_BYTES =(size_t)256 << 20;   // post[node][unit][S] of one chunk of nodes, at most (one node always goes);
                                                       // the test hook CB_ANC_POST_BYTES: the results do not depend on the chunking

extern "C" int cb_bl_ancestral(cb_bl_s *h, int8_t *state, double *conf, double *post, double *fam_ll, double *kernel_ms) {
  static const char *who = "cb_bl_ancestral";
  if (!h) return fail(CB_EINVAL, "%s: NULL handle", who);
  if (!state) return fail(CB_EINVAL, "%s: NULL argument (state)", who);
  const EmForestHost &H = h->forest.host;
  const int n_fam = H.n_fam(), S = h->forest.S, upw = 64 / S;
  // nodes per launch: all of a family's, fewer under the bound on post and where nodes x site tiles would pass 2^31
  std::vector<int> chunk(n_fam, 0);
  size_t max_out = 0;
  const size_t bound = cb_hook_bytes("CB_ANC_POST_BYTES", ANC_POST_BYTES);
  for (int f = 0; f < n_fam; ++f) {
    const EmFamHost &F = H.fam[f];
    const size_t n_blocks = ((size_t)F.n_units + upw - 1) / upw;
    size_t fit = (size_t)INT32_MAX / n_blocks;
    if (post) fit = std::min(fit, bound / ((size_t)F.n_units * S * sizeof(double)));
    chunk[f] = (int)std::min<size_t>(F.n_nodes, std::max<size_t>(fit, 1));
    if ((size_t)chunk[f] * n_blocks > (size_t)INT32_MAX)
      return fail(CB_EINVAL, "%s: family %d: %zu site tiles (at most 2^31 - 1 per launch)", who, f, n_blocks);
    max_out = std::max(max_out, (size_t)chunk[f] * F.n_units);
  }
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
  const std::vector<char> all(n_fam, 1);
  int rc = bl_refresh(h, all, kernel_ms);
  if (rc != CB_OK) return rc;
  std::vector<int8_t> host_state(max_out);
  std::vector<double> host_conf(conf ? max_out : 0), host_post(post ? max_out * S : 0);
  CbDevBufs bufs;   // this call's: freed on every return path
  signed char *dstate = bufs.up<signed char>(nullptr, max_out, rc);
  double *dconf = bufs.up<double>(nullptr, max_out, rc), *dpost = post ? bufs.up<double>(nullptr, max_out * S, rc) : nullptr;
  if (rc != CB_OK) return rc;
  for (int f = 0; f < n_fam; ++f) {
    const EmFamView w = h->forest.view(f);
    const EmFamHost &F = w.F;
    const int U = F.n_units;
    AncArgs a{};
    a.S = S; a.n_units = U; a.n_cats = F.n_cats; a.root = F.root; a.n_blocks = w.n_blocks;
    a.parent = w.parent; a.child_ptr = w.child_ptr; a.child_idx = w.child_idx; a.qb = w.qb; a.unit_cat = w.unit_cat;
    a.codes = w.codes; a.P = h->dP; a.pi_root = h->dpi; a.msg = w.msg; a.U = w.U; a.state = dstate; a.conf = dconf; a.post = dpost;
    for (int v0 = 0; v0 < F.n_nodes; v0 += chunk[f]) {
      const int nv = std::min(chunk[f], F.n_nodes - v0);
      a.node0 = v0;
      rc = bl_timed(h, kernel_ms, 1, [&](CbKernelTimer &) -> int {
        hipLaunchKernelGGL(anc_post_kernel, dim3((unsigned)nv * (unsigned)a.n_blocks), dim3(64), 0, 0, a);
        return CB_OK;
      });
      if (rc != CB_OK) return rc;
      // device (category) order -> the caller's unit order (the next chunk writes the same buffers: these copies wait for this one)
      const size_t cnt = (size_t)nv * U, base = H.off_c[f] + (size_t)v0 * U;
      HIP_TRY(hipMemcpy(host_state.data(), dstate, cnt * sizeof(int8_t), hipMemcpyDeviceToHost));
      if (conf) HIP_TRY(hipMemcpy(host_conf.data(), dconf, cnt * sizeof(double), hipMemcpyDeviceToHost));
      if (post) HIP_TRY(hipMemcpy(host_post.data(), dpost, cnt * S * sizeof(double), hipMemcpyDeviceToHost));
      // (one fused pass over the three arrays, not em_unpermute per array and node: that took 2 to 3 ms more of a 42 ms call on
      // the 32 demo families)
      for (int v = 0; v < nv; ++v)
        for (int k = 0; k < U; ++k) {
          const size_t src = (size_t)v * U + k, dst = base + (size_t)v * U + F.perm[k];
          state[dst] = host_state[src];
          if (conf) conf[dst] = host_conf[src];
          if (post) std::copy(host_post.begin() + src * S, host_post.begin() + (src + 1) * S, post + dst * S);
        }
    }
  }
  return bl_finish(h, all, fam_ll);
}
