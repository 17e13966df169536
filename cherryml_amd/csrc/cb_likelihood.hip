// libcherrybank: held-out log-likelihood by level-synchronous pruning.
#include "cb_internal.hip.h"
#include "common.hip.h"
#include "likelihood.hip.h"
#include "tl_layout.h"

// ---- the model resident on the device ------------------------------------------------------------------------------------
// cb_tree_likelihood[_batch] takes the model with every call, like the reference's per-family processes
// (evaluation/_likelihood.py:474-600): Q uploaded, a counts-free expm handle created, 2.6 GB of transition bank and the message
// buffer allocated and freed, the model's eigendecomposition recomputed -- 21 ms per 1024-leaf family of the 400-state pair model
// around 10.7 ms of kernels.  A cb_tl_model keeps all of that between calls.
struct cb_tl_model_s {
  int device = 0, S = 0, S1 = 0;
  bool reversible = false;                  // made with pi_rev: the bank comes from the symmetric eigendecomposition
  double *dQ = nullptr, *dpi = nullptr, *dproot = nullptr;
  double *dP = nullptr, *dmsg = nullptr;    // transition bank [slot][S][S] and messages, grown on demand
  size_t cap_P = 0, cap_msg = 0, cap_bank = 0;
  cb_handle hl = nullptr;                   // the counts-free expm handle, cap_bank slots
  bool eigh_done = false;
  // S > 64, reversible: the leaves' tables (tl_tables_kernel), built behind the model's first eigensolve
  double *dTU = nullptr, *dTA = nullptr;
  bool tables_done = false;
};

namespace {
// the device side of one call's arrays (TlLayout's offsets apply), or of one family of it (tl_family_view)
struct TlDev {
  double *dll = nullptr;
  const int *duc = nullptr;
  const int8_t *dca = nullptr, *dcb = nullptr;
  const int *dlev = nullptr, *dcp = nullptr, *dci = nullptr;
  const double *dt_all = nullptr, *dt_node = nullptr;
  const int *dslot = nullptr;
};

TlDev tl_family_view(const TlDev &d, const TlLayout &L, int f) {
  const size_t on = L.off_n[f], ou = L.off_u[f], oc = L.off_c[f];
  TlDev v;
  v.dll = d.dll + ou; v.duc = d.duc + ou; v.dca = d.dca + oc; v.dcb = d.dcb ? d.dcb + oc : nullptr;
  v.dlev = d.dlev + on; v.dcp = d.dcp + on + f; v.dci = d.dci + on;
  v.dt_all = d.dt_all + L.off_t[f];
  if (L.factored) { v.dt_node = d.dt_node + on; v.dslot = d.dslot + on; }
  return v;
}

// The timing events of one call: the whole timed region (ev0 .. ev1) and a marker pair around each family's pruning.
// Whatever was created is destroyed on every way out of the call.
struct TlTimer {
  const bool on;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> marks;   // (begin, end) per timed family
  explicit TlTimer(bool on_) : on(on_) {}
  TlTimer(const TlTimer &) = delete;
  ~TlTimer() {
    for (hipEvent_t ev : marks) (void)hipEventDestroy(ev);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
  int start() {
    if (!on) return CB_OK;
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    HIP_TRY(hipStreamSynchronize(0));   // the timed region starts with resident inputs
    HIP_TRY(hipEventRecord(ev0, 0));
    return CB_OK;
  }
  // both markers of a family or neither
  bool family_begin() {
    hipEvent_t b = nullptr, e = nullptr;
    if (!on || hipEventCreate(&b) != hipSuccess) return false;
    if (hipEventCreate(&e) != hipSuccess) {
      (void)hipEventDestroy(b);
      return false;
    }
    marks.push_back(b);
    marks.push_back(e);
    (void)hipEventRecord(b, 0);
    return true;
  }
  void family_end() { (void)hipEventRecord(marks.back(), 0); }
  // waits for the stream; kernel_ms[0] = the region, kernel_ms[1] = the sum over the families' marker pairs
  int finish(double *kernel_ms, int rc) {
    if (!on) return rc;
    float ms = 0.f;
    hipError_t e = hipEventRecord(ev1, 0);
    if (e == hipSuccess) e = hipEventSynchronize(ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    double ms_prune = 0.0;
    for (size_t i = 0; i + 1 < marks.size(); i += 2) {
      float mp = 0.f;
      if (hipEventElapsedTime(&mp, marks[i], marks[i + 1]) == hipSuccess) ms_prune += mp;
    }
    kernel_ms[0] = ms;
    kernel_ms[1] = ms_prune;
    if (e != hipSuccess && rc == CB_OK) rc = fail(CB_EHIP, "cb_tree_likelihood: %s", hipGetErrorString(e));
    return rc;
  }
};

int tl_grow(double *&p, size_t &cap, size_t need, const char *what) {
  if (need <= cap) return CB_OK;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  if (hipMalloc((void **)&p, need * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CB_ENOMEM, "cb_tree_likelihood: %zu bytes for the %s", need * sizeof(double), what);
  }
  cap = need;
  return CB_OK;
}

// What all families AND all calls on a model share, sized for the largest family met so far: the transition bank's and the
// messages' buffers (2.6 GB for a 1024-leaf family of the 400-state pair model) ...
int tl_model_reserve(cb_tl_model_s &m, const TlLayout &L) {
  const int rc = tl_grow(m.dP, m.cap_P, L.max_bank * m.S * m.S, "transition bank");
  return rc != CB_OK ? rc : tl_grow(m.dmsg, m.cap_msg, L.max_msg, "messages");
}

// ... and one counts-free handle: a single "site" whose buckets are a family's bank slots.  A new handle has no decomposition
// yet, so the eigensolve and the leaves' tables that hang on it are due again.
int tl_model_handle(cb_tl_model_s &m, const TlLayout &L) {
  if (m.hl && L.max_bank <= m.cap_bank) return CB_OK;
  if (m.hl) cb_destroy(m.hl);
  m.hl = nullptr;
  m.eigh_done = false;
  m.tables_done = false;   // (the same solver on the same matrix would give the same tables: not a promise kept here)
  const std::vector<double> t0(L.max_bank, 0.0);
  int rc = cb_create(m.device, m.S, 1, (int)L.max_bank, CB_F64, t0.data(), nullptr, CB_EXPM_ONLY, &m.hl);
  if (rc == CB_OK) rc = cb_set_stream(m.hl, nullptr, 0);
  if (rc == CB_OK) m.cap_bank = L.max_bank;
  return rc;
}

// the caller's codes and categories and the trees, before the timed region starts
int tl_upload_inputs(CbDevBufs &bufs, const TlCall &c, const TlLayout &L, bool pairs, TlDev &d) {
  int rc = CB_OK;
  const size_t n_units = L.off_u[c.n_fam], n_codes = L.off_c[c.n_fam];
  d.dll = bufs.up<double>(nullptr, n_units, rc);
  d.duc = bufs.up(c.unit_cat, n_units, rc);
  d.dca = bufs.up(c.code_a, n_codes, rc);
  d.dcb = pairs ? bufs.up(c.code_b, n_codes, rc) : nullptr;
  d.dlev = bufs.up(L.level_nodes.data(), L.level_nodes.size(), rc);
  d.dcp = bufs.up(L.child_ptr.data(), L.child_ptr.size(), rc);
  d.dci = bufs.up(L.child_idx.data(), L.child_idx.size(), rc);
  return rc;
}

// rate x length of ALL families, inside the timed region: a family's bank then starts behind the previous family's pruning on
// the stream without the host waiting for it
int tl_upload_times(CbDevBufs &bufs, const TlLayout &L, TlDev &d) {
  int rc = CB_OK;
  d.dt_all = bufs.up(L.t_all.data(), L.t_all.size(), rc);
  d.dt_node = L.factored ? bufs.up(L.t_node.data(), L.t_node.size(), rc) : nullptr;
  d.dslot = L.factored ? bufs.up(L.slot_all.data(), L.slot_all.size(), rc) : nullptr;
  return rc;
}

// family f's transition bank expm(t Q), one [S][S] matrix per bank slot, by the bank's own expm kernels (d: the family's view); the reversible
// bank of S > 32 keeps the model's eigendecomposition from the first family on
int tl_family_bank(cb_tl_model_s &m, const TlLayout &L, int f, const TlDev &d) {
  int rc = cb_internal_set_times(m.hl, L.t_all.data() + L.off_t[f], (int)L.fam[f].n_bank, d.dt_all);
  if (rc != CB_OK) return rc;
  const int reuse = m.S > 32 && m.eigh_done && m.dpi ? CB_REUSE_EIGH : 0;
  rc = cb_internal_expm_bank(m.hl, m.dQ, m.dpi, CB_PTR_DEVICE | CB_NO_SYNC | reuse, m.dP);
  if (rc == CB_OK) m.eigh_done = true;
  return rc;
}

// the leaves' tables of a factored model: once per decomposition, behind its eigensolve on the stream
int tl_leaf_tables(cb_tl_model_s &m, const CbSpectral &sp) {
  if (m.tables_done) return CB_OK;
  const int nJ = m.S + (m.S1 > 0 ? 2 * m.S1 : 0) + 1;
  if (!m.dTU && (hipMalloc((void **)&m.dTU, (size_t)nJ * sp.LD * sizeof(double)) != hipSuccess ||
                 hipMalloc((void **)&m.dTA, (size_t)nJ * sp.LD * sizeof(double)) != hipSuccess)) {
    (void)hipGetLastError();
    return fail(CB_ENOMEM, "cb_tree_likelihood: device allocation failed");
  }
  hipLaunchKernelGGL(tl_tables_kernel, dim3(nJ), dim3(256), 0, 0, m.S, m.S1, sp.LD, nJ, sp.U, sp.A, sp.dsq, m.dTU, m.dTA);
  m.tables_done = true;
  return CB_OK;
}

// the levels of one family with NB blocks of 16 units per workgroup: one launch per height over (nodes of that height) x
// (blocks of units), stream 0.  a.slot != nullptr: the leaves come from the eigendecomposition (tl_leaf_mfma_kernel).
template <int NB>
int tl_prune_levels(const TlFamily &F, TlArgs a, const int *dlev) {
  const int S = a.S, Sp = (S + 15) / 16 * 16;
  const size_t lds = ((size_t)(Sp * NB + Sp / 4 + NB) * 16 + (size_t)TL_NW * NB * 16) * sizeof(double);
  const size_t lds_leaf = ((size_t)TL_LR * (S + 1) + TL_LR + (size_t)TL_LR * 2 * a.S1) * sizeof(double) + 2 * (size_t)F.n_units;
  if (S > 64 && lds_leaf > 160 * 1024)
    return fail(CB_EUNSUPPORTED, "cb_tree_likelihood: %d units per family at S > 64 (at most 50 000)", F.n_units);
  const auto set_lds = [](auto *kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  };
  if (S > 64 && (set_lds(tl_mfma_kernel<NB>, lds) != hipSuccess || set_lds(tl_leaf_mfma_kernel<NB>, lds) != hipSuccess ||
                 set_lds(tl_leaf_kernel, lds_leaf) != hipSuccess))
    return fail(CB_EHIP, "cb_tree_likelihood: cannot reserve %zu bytes of LDS", lds);
  for (int l = 0; l < F.n_levels; ++l) {
    const int nl = F.level_ptr[l + 1] - F.level_ptr[l];
    // height 0 = the leaves (never the root when the tree has an edge): gathered or factored, not multiplied
    const bool leaves = S > 64 && l == 0 && F.n_levels > 1;
    const bool leaves_fx = leaves && a.slot != nullptr;
    a.n_blocks = (leaves && !leaves_fx) ? 1 : S > 64 ? (F.n_units + 16 * NB - 1) / (16 * NB) : (F.n_units + 64 / S - 1) / (64 / S);
    a.RS = 1;
    if (S > 64 && !leaves) {   // small levels: split the rows of a node over 2 or 4 workgroups (one per CU)
      const long wgs = (long)nl * a.n_blocks;
      a.RS = wgs * 4 <= 256 ? 4 : wgs * 2 <= 256 ? 2 : 1;
    }
    const int per_node = a.n_blocks * a.RS;
    const int per_launch = std::max(1, (1 << 30) / per_node);   // keep the 1-D grid below 2^30 workgroups
    for (int y0 = 0; y0 < nl; y0 += per_launch) {
      TlArgs b = a;
      b.level_nodes = dlev + F.level_ptr[l] + y0;
      b.n_level = std::min(per_launch, nl - y0);
      const dim3 grid((unsigned)b.n_level * (unsigned)per_node);
      if (leaves_fx)
        hipLaunchKernelGGL(tl_leaf_mfma_kernel<NB>, grid, dim3(TL_NW * 64), lds, 0, b);
      else if (leaves)
        hipLaunchKernelGGL(tl_leaf_kernel, grid, dim3(TL_LT), lds_leaf, 0, b);
      else if (S > 64)
        hipLaunchKernelGGL(tl_mfma_kernel<NB>, grid, dim3(TL_NW * 64), lds, 0, b);
      else
        hipLaunchKernelGGL(tl_group_kernel, grid, dim3(64), 0, 0, b);
    }
  }
  return CB_OK;
}

// the pruning of one family; d: the family's view of the call's device arrays; sp: the decomposition the factored leaves take
// their operands from (empty otherwise: the leaves gather from the bank, tl_leaf_kernel)
int tl_prune(const cb_tl_model_s &m, const TlFamily &F, const TlDev &d, const CbSpectral &sp) {
  TlArgs a{};
  a.slot = d.dslot; a.tnode = d.dt_node;
  a.U = sp.U; a.lam = sp.lam; a.dsq = sp.dsq; a.sigma = sp.sigma; a.TU = m.dTU; a.TA = m.dTA; a.LD = sp.LD;
  a.S = m.S; a.S1 = m.S1; a.n_nodes = F.n_nodes; a.n_units = F.n_units; a.NU = F.NU; a.root = F.root;
  a.child_ptr = d.dcp; a.child_idx = d.dci; a.P = m.dP; a.unit_cat = d.duc;
  a.code_a = reinterpret_cast<const signed char *>(d.dca);
  a.code_b = reinterpret_cast<const signed char *>(d.dcb);
  a.pi_root = m.dproot; a.msg = m.dmsg; a.ll = d.dll;
  return F.n_units > 16 ? tl_prune_levels<2>(F, a, d.dlev) : tl_prune_levels<1>(F, a, d.dlev);
}

// One run of the pruning over the families of a call that tl_check_call has passed, on a resident model (the reference maps
// families over a process pool, evaluation/_likelihood.py:474-600 / utils.py:59-67).  The families share the model's
// buffers and its one counts-free bank handle: new branch lengths per family, and for a reversible Q of S > 32 one
// eigensolve per handle.  All branch lengths are uploaded once, so a reversible family's bank is enqueued behind the previous
// family's pruning without a host wait; the general (non-reversible) bank reads one norm back per family.  A refused call
// (tl_layout) has touched neither the device nor the model.  Results equal cb_tree_likelihood's.
int tl_run(cb_tl_model_s &m, const TlCall &c, double *kernel_ms) {
  TlLayout L;
  int rc = tl_layout(m.S, m.S1, m.reversible, c, L);
  if (rc != CB_OK) return rc;
  HIP_TRY(hipSetDevice(m.device));
  if ((rc = tl_model_reserve(m, L)) != CB_OK) return rc;
  CbDevBufs bufs;
  TlDev d;
  if ((rc = tl_upload_inputs(bufs, c, L, m.S1 > 0, d)) != CB_OK) return rc;
  if ((rc = tl_model_handle(m, L)) != CB_OK) return rc;   // (behind the uploads: its creation enqueues copies of its own)
  TlTimer timer(kernel_ms != nullptr);
  if ((rc = timer.start()) != CB_OK) return rc;
  if ((rc = tl_upload_times(bufs, L, d)) != CB_OK) return rc;
  for (int f = 0; f < c.n_fam && rc == CB_OK; ++f) {
    const TlDev df = tl_family_view(d, L, f);
    if ((rc = tl_family_bank(m, L, f, df)) != CB_OK) break;
    const bool timed = timer.family_begin();   // the pruning time of this family
    CbSpectral sp;   // factored: what the family's bank left on the handle, and the model's tables of it
    if (L.factored && ((rc = cb_internal_spectral(m.hl, &sp)) != CB_OK || (rc = tl_leaf_tables(m, sp)) != CB_OK)) break;
    rc = tl_prune(m, L.fam[f], df, sp);
    if (timed) timer.family_end();
  }
  if ((rc = timer.finish(kernel_ms, rc)) != CB_OK) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(c.ll, d.dll, L.off_u[c.n_fam] * sizeof(double), hipMemcpyDeviceToHost));
  return CB_OK;
}
}  // namespace

extern "C" int cb_tl_model_destroy(cb_tl_model_s *m) {
  if (!m) return CB_OK;
  (void)hipSetDevice(m->device);
  if (m->hl) cb_destroy(m->hl);
  for (double *p : {m->dQ, m->dpi, m->dproot, m->dP, m->dmsg, m->dTU, m->dTA})
    if (p) (void)hipFree(p);
  delete m;
  return CB_OK;
}

extern "C" int cb_tl_model_create(int device, int S, int S1, const double *Q, const double *pi_rev, const double *pi_root,
                                  cb_tl_model_s **out) {
  if (!Q || !pi_root || !out) return fail(CB_EINVAL, "cb_tl_model_create: NULL argument");
  if (S < 2 || S > 16 * TL_NW * TL_MAXT) return fail(CB_EINVAL, "cb_tree_likelihood: bad sizes (S = %d)", S);
  if (S1 < 0 || (S1 > 0 && S1 * S1 != S)) return fail(CB_EINVAL, "cb_tree_likelihood: pair model needs S = S1 * S1 and code_b");
  const int ndev = cb_device_count();
  if (ndev <= 0) return fail(CB_EHIP, "cb_tree_likelihood: no HIP device (this path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(CB_EINVAL, "cb_tree_likelihood: device %d of %d", device, ndev);
  HIP_TRY(hipSetDevice(device));
  cb_tl_model_s *m = new cb_tl_model_s;
  m->device = device; m->S = S; m->S1 = S1; m->reversible = pi_rev != nullptr;
  const size_t SS = (size_t)S * S;
  bool ok = hipMalloc((void **)&m->dproot, S * sizeof(double)) == hipSuccess &&
            hipMemcpy(m->dproot, pi_root, S * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (ok)
    ok = hipMalloc((void **)&m->dQ, SS * sizeof(double)) == hipSuccess && hipMemcpy(m->dQ, Q, SS * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (ok && pi_rev)
    ok = hipMalloc((void **)&m->dpi, S * sizeof(double)) == hipSuccess && hipMemcpy(m->dpi, pi_rev, S * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    cb_tl_model_destroy(m);
    return fail(CB_ENOMEM, "cb_tl_model_create: device allocation or upload failed");
  }
  *out = m;
  return CB_OK;
}

extern "C" int cb_tl_model_run(cb_tl_model_s *m, int n_fam, const int *n_nodes, const int *postorder, const int *parent,
                               const double *length, const int *n_cats, const double *cat_rate, const int *n_units,
                               const int *unit_cat, const int8_t *code_a, const int8_t *code_b, double *ll, double *kernel_ms) {
  if (!m) return fail(CB_EINVAL, "cb_tl_model_run: NULL model");
  const TlCall c{n_fam, n_nodes, postorder, parent, length, n_cats, cat_rate, n_units, unit_cat, code_a, code_b, ll};
  const int rc = tl_check_call(m->S, m->S1, true, c);
  return rc != CB_OK ? rc : tl_run(*m, c, kernel_ms);
}

// MANY families under ONE model made for the call (cb_tl_model_create / tl_run / cb_tl_model_destroy); what needs no device
// to refuse is refused before the model is made
extern "C" int cb_tree_likelihood_batch(int device, int S, int S1, const double *Q, const double *pi_rev,
                                        const double *pi_root, int n_fam, const int *n_nodes, const int *postorder,
                                        const int *parent, const double *length, const int *n_cats,
                                        const double *cat_rate, const int *n_units, const int *unit_cat,
                                        const int8_t *code_a, const int8_t *code_b, double *ll, double *kernel_ms) {
  const TlCall c{n_fam, n_nodes, postorder, parent, length, n_cats, cat_rate, n_units, unit_cat, code_a, code_b, ll};
  int rc = tl_check_call(S, S1, Q && pi_root, c);
  if (rc != CB_OK) return rc;
  cb_tl_model_s *m = nullptr;
  if ((rc = cb_tl_model_create(device, S, S1, Q, pi_rev, pi_root, &m)) != CB_OK) return rc;
  rc = tl_run(*m, c, kernel_ms);
  cb_tl_model_destroy(m);
  return rc;
}

extern "C" int cb_tree_likelihood(int device, int S, int S1, const double *Q, const double *pi_rev,
                                  const double *pi_root, int n_nodes, const int *postorder, const int *parent,
                                  const double *length, int n_cats, const double *cat_rate, int n_units,
                                  const int *unit_cat, const int8_t *code_a, const int8_t *code_b, double *ll,
                                  double *kernel_ms) {
  return cb_tree_likelihood_batch(device, S, S1, Q, pi_rev, pi_root, 1, &n_nodes, postorder, parent, length, &n_cats,
                                  cat_rate, &n_units, unit_cat, code_a, code_b, ll, kernel_ms);
}
