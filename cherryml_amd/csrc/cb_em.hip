// libcherrybank: the E-step of full-tree EM on a resident handle (em.hip.h; include/cherrybank.h, cb_em_*).
#include "cb_internal.hip.h"
#include "common.hip.h"
#include "em.hip.h"
#include "em_host.hip.h"

namespace {
constexpr int EM_TASK_UNITS = 512;   // (edge, unit) pairs per accumulation task, at most

}  // namespace

struct cb_em_s {
  int device = 0, S = 0, B = 0, n_fam = 0, n_tasks = 0;
  size_t n_units_all = 0, nu_all = 0;
  std::vector<double> grid;
  std::vector<EmFamHost> fam;
  std::vector<EmFam> famd;
  cb_handle hexp = nullptr;               // counts-free expm handle over the grid points
  std::vector<void *> bufs;               // every device buffer below
  double *dQ = nullptr, *dpi = nullptr, *dP = nullptr, *dmsg = nullptr, *dU = nullptr, *dll = nullptr, *dpart = nullptr, *dE = nullptr;
  int *dparent = nullptr, *dcp = nullptr, *dci = nullptr, *dlev = nullptr, *ddep = nullptr, *dqb = nullptr, *duc = nullptr;
  int *dtask_seg = nullptr, *dbucket_task = nullptr;
  signed char *dcodes = nullptr;
  EmFam *dfam = nullptr;
  EmSeg *dseg = nullptr;
  std::vector<size_t> off_n, off_q, off_lev;   // per family: node offset, qb offset
};

template <typename T>
static T *em_alloc(cb_em_s *h, const T *host, size_t count, int &rc) {
  if (rc != CB_OK) return nullptr;
  void *p = nullptr;
  if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    rc = fail(CB_ENOMEM, "cb_em_create: %zu bytes of device memory", count * sizeof(T));
    return nullptr;
  }
  h->bufs.push_back(p);
  if (host && count && hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(CB_EHIP, "cb_em_create: upload failed");
  return static_cast<T *>(p);
}

extern "C" int cb_em_destroy(cb_em_s *h) {
  if (!h) return CB_OK;
  (void)hipSetDevice(h->device);
  if (h->hexp) cb_destroy(h->hexp);
  for (void *p : h->bufs)
    if (p) (void)hipFree(p);
  delete h;
  return CB_OK;
}

extern "C" int cb_em_create(int device, int S, int B, const double *grid, int n_fam, const int *n_nodes, const int *parent,
                            const double *length, const int *n_units, const double *unit_rate, const int8_t *codes,
                            cb_em_s **out) {
  if (!grid || !n_nodes || !parent || !length || !n_units || !unit_rate || !codes || !out)
    return fail(CB_EINVAL, "cb_em_create: NULL argument");
  *out = nullptr;
  if (S < 2 || S > 32) return fail(CB_EINVAL, "cb_em_create: S = %d (2 <= S <= 32: one 32 x 32 MFMA tile per task)", S);
  if (B < 1 || n_fam < 1) return fail(CB_EINVAL, "cb_em_create: bad sizes (B = %d, families = %d)", B, n_fam);
  for (int b = 0; b < B; ++b)
    if (!(grid[b] > 0.0) || !std::isfinite(grid[b]) || (b > 0 && !(grid[b] > grid[b - 1])))
      return fail(CB_EINVAL, "cb_em_create: the grid must be positive and strictly increasing (grid[%d] = %g)", b, grid[b]);
  cb_em_s *h = new cb_em_s;
  h->device = device; h->S = S; h->B = B; h->n_fam = n_fam;
  h->grid.assign(grid, grid + B);
  h->fam.resize(n_fam);
  h->off_n.assign(n_fam + 1, 0);
  h->off_q.assign(n_fam + 1, 0);
  std::vector<size_t> off_u(n_fam + 1, 0), off_c(n_fam + 1, 0);
  for (int f = 0; f < n_fam; ++f) {
    const int rc = em_prepare("cb_em_create", S, B, grid, n_nodes[f], parent + h->off_n[f], length + h->off_n[f], n_units[f],
                              unit_rate + off_u[f], codes + off_c[f], f, h->fam[f]);
    if (rc != CB_OK) {
      cb_em_destroy(h);
      return rc;
    }
    h->off_n[f + 1] = h->off_n[f] + n_nodes[f];
    off_u[f + 1] = off_u[f] + n_units[f];
    off_c[f + 1] = off_c[f] + (size_t)n_nodes[f] * n_units[f];
    h->off_q[f + 1] = h->off_q[f] + (size_t)n_nodes[f] * h->fam[f].n_cats;
  }
  h->n_units_all = off_u[n_fam];
  h->nu_all = off_c[n_fam];
  // the accumulation's work: per bucket, the (edge, category) segments in (family, node, category) order, packed into tasks
  std::vector<std::vector<EmSeg>> per_bucket(B);
  for (int f = 0; f < n_fam; ++f) {
    const EmFamHost &F = h->fam[f];
    for (int v = 0; v < F.n_nodes; ++v) {
      if (v == F.root) continue;
      for (int c = 0; c < F.n_cats; ++c) {
        const int n = F.cat_ptr[c + 1] - F.cat_ptr[c];
        if (n > 0) per_bucket[F.qb[(size_t)v * F.n_cats + c]].push_back(EmSeg{f, v, F.cat_ptr[c], n});
      }
    }
  }
  std::vector<EmSeg> segs;
  std::vector<int> task_seg{0}, bucket_task{0};
  for (int b = 0; b < B; ++b) {
    int fill = 0;
    for (const EmSeg &s0 : per_bucket[b])
      for (int u = 0; u < s0.n;) {
        if (fill == EM_TASK_UNITS) {
          task_seg.push_back((int)segs.size());
          fill = 0;
        }
        const int take = std::min(s0.n - u, EM_TASK_UNITS - fill);
        segs.push_back(EmSeg{s0.fam, s0.v, s0.u0 + u, take});
        u += take;
        fill += take;
      }
    if (fill > 0) task_seg.push_back((int)segs.size());
    bucket_task.push_back((int)task_seg.size() - 1);
  }
  h->n_tasks = (int)task_seg.size() - 1;
  // device work from here on
  const int ndev = cb_device_count();
  if (ndev <= 0) {
    cb_em_destroy(h);
    return fail(CB_EHIP, "cb_em_create: no HIP device (this path has no CPU fallback)");
  }
  if (device < 0 || device >= ndev) {
    cb_em_destroy(h);
    return fail(CB_EINVAL, "cb_em_create: device %d of %d", device, ndev);
  }
  if (hipSetDevice(device) != hipSuccess) {
    cb_em_destroy(h);
    return fail(CB_EHIP, "cb_em_create: hipSetDevice(%d) failed", device);
  }
  // per-family arrays, concatenated; units permuted into category order
  std::vector<int> par_all(h->off_n[n_fam]), cp_all(h->off_n[n_fam] + n_fam), ci_all(h->off_n[n_fam]), lev_all(h->off_n[n_fam]);
  std::vector<int> dep_all, qb_all(h->off_q[n_fam]), uc_all(h->n_units_all);
  std::vector<int8_t> code_all(h->nu_all);
  h->off_lev.assign(n_fam + 1, 0);
  for (int f = 0; f < n_fam; ++f) {
    const EmFamHost &F = h->fam[f];
    std::copy(parent + h->off_n[f], parent + h->off_n[f + 1], par_all.begin() + h->off_n[f]);
    std::copy(F.child_ptr.begin(), F.child_ptr.end(), cp_all.begin() + h->off_n[f] + f);
    std::copy(F.child_idx.begin(), F.child_idx.begin() + (F.n_nodes - 1), ci_all.begin() + h->off_n[f]);
    std::copy(F.level_nodes.begin(), F.level_nodes.end(), lev_all.begin() + h->off_n[f]);
    h->off_lev[f] = dep_all.size();
    dep_all.insert(dep_all.end(), F.depth_nodes.begin(), F.depth_nodes.end());
    std::copy(F.qb.begin(), F.qb.end(), qb_all.begin() + h->off_q[f]);
    std::copy(F.unit_cat.begin(), F.unit_cat.end(), uc_all.begin() + off_u[f]);
    for (int v = 0; v < F.n_nodes; ++v)
      for (int k = 0; k < F.n_units; ++k)
        code_all[off_c[f] + (size_t)v * F.n_units + k] = codes[off_c[f] + (size_t)v * F.n_units + F.perm[k]];
    h->famd.push_back(EmFam{(long long)off_c[f], (int)h->off_n[f], (int)off_u[f], F.n_units, F.root});
  }
  h->off_lev[n_fam] = dep_all.size();
  int rc = CB_OK;
  const size_t SS = (size_t)S * S;
  h->dQ = em_alloc<double>(h, nullptr, SS, rc);
  h->dpi = em_alloc<double>(h, nullptr, S, rc);
  h->dP = em_alloc<double>(h, nullptr, (size_t)B * SS, rc);
  h->dE = em_alloc<double>(h, nullptr, (size_t)B * SS, rc);
  h->dmsg = em_alloc<double>(h, nullptr, h->nu_all * S, rc);
  h->dU = em_alloc<double>(h, nullptr, h->nu_all * S, rc);
  h->dll = em_alloc<double>(h, nullptr, h->n_units_all, rc);
  h->dpart = em_alloc<double>(h, nullptr, (size_t)h->n_tasks * SS, rc);
  h->dparent = em_alloc(h, par_all.data(), par_all.size(), rc);
  h->dcp = em_alloc(h, cp_all.data(), cp_all.size(), rc);
  h->dci = em_alloc(h, ci_all.data(), ci_all.size(), rc);
  h->dlev = em_alloc(h, lev_all.data(), lev_all.size(), rc);
  h->ddep = em_alloc(h, dep_all.data(), dep_all.size(), rc);
  h->dqb = em_alloc(h, qb_all.data(), qb_all.size(), rc);
  h->duc = em_alloc(h, uc_all.data(), uc_all.size(), rc);
  h->dcodes = reinterpret_cast<signed char *>(em_alloc(h, code_all.data(), code_all.size(), rc));
  h->dfam = em_alloc(h, h->famd.data(), h->famd.size(), rc);
  h->dseg = em_alloc(h, segs.data(), segs.size(), rc);
  h->dtask_seg = em_alloc(h, task_seg.data(), task_seg.size(), rc);
  h->dbucket_task = em_alloc(h, bucket_task.data(), bucket_task.size(), rc);
  if (rc == CB_OK) rc = cb_create(device, S, 1, B, CB_F64, grid, nullptr, CB_EXPM_ONLY, &h->hexp);
  if (rc == CB_OK) rc = cb_set_stream(h->hexp, nullptr, 0);
  if (rc != CB_OK) {
    cb_em_destroy(h);
    return rc;
  }
  *out = h;
  return CB_OK;
}

void em_launch_up(const TlArgs &a, const int *qb, int n_cats, unsigned grid) {
  hipLaunchKernelGGL(em_up_kernel, dim3(grid), dim3(64), 0, 0, a, qb, n_cats);
}
void em_launch_down(const EmDownArgs &a, unsigned grid) { hipLaunchKernelGGL(em_down_kernel, dim3(grid), dim3(64), 0, 0, a); }

static void em_launch_passes(cb_em_s *h) {
  const int S = h->S, upw = 64 / S;
  for (int f = 0; f < h->n_fam; ++f) {
    const EmFamHost &F = h->fam[f];
    const size_t nb = (size_t)h->famd[f].nu_base;
    const int n_blocks = (F.n_units + upw - 1) / upw;
    TlArgs a{};
    a.S = S; a.S1 = 0; a.n_nodes = F.n_nodes; a.n_units = F.n_units; a.NU = F.n_units; a.root = F.root; a.n_blocks = n_blocks;
    a.child_ptr = h->dcp + h->off_n[f] + f; a.child_idx = h->dci + h->off_n[f]; a.P = h->dP;
    a.unit_cat = h->duc + h->famd[f].unit_base; a.code_a = h->dcodes + nb; a.code_b = nullptr; a.pi_root = h->dpi;
    a.msg = h->dmsg + nb * S; a.ll = h->dll + h->famd[f].unit_base;
    const int *qb = h->dqb + h->off_q[f];
    for (size_t l = 0; l + 1 < F.level_ptr.size(); ++l) {
      TlArgs b = a;
      b.level_nodes = h->dlev + h->off_n[f] + F.level_ptr[l];
      b.n_level = F.level_ptr[l + 1] - F.level_ptr[l];
      em_launch_up(b, qb, F.n_cats, (unsigned)(b.n_level * n_blocks));
    }
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
  if (h->n_tasks > 0) {
    EmAccArgs c{};
    c.S = S; c.task_seg = h->dtask_seg; c.seg = h->dseg; c.fam = h->dfam; c.parent = h->dparent; c.child_ptr = h->dcp;
    c.child_idx = h->dci; c.codes = h->dcodes; c.pi_root = h->dpi; c.msg = h->dmsg; c.U = h->dU; c.ll = h->dll; c.part = h->dpart;
    hipLaunchKernelGGL(em_acc_kernel, dim3((unsigned)h->n_tasks), dim3(64), 0, 0, c);
  }
  hipLaunchKernelGGL(em_reduce_kernel, dim3((unsigned)h->B), dim3(256), 0, 0, S, h->dbucket_task, h->dpart, h->dP, h->dE);
}

extern "C" int cb_em_estep(cb_em_s *h, const double *Q, const double *pi_root, double *counts, double *ll, double *fam_ll,
                           double *kernel_ms) {
  if (!h) return fail(CB_EINVAL, "cb_em_estep: NULL handle");
  if (!Q || !pi_root || !counts) return fail(CB_EINVAL, "cb_em_estep: NULL argument");
  const int S = h->S;
  const size_t SS = (size_t)S * S;
  const int mrc = em_check_model("cb_em_estep", S, Q, pi_root);
  if (mrc != CB_OK) return mrc;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpy(h->dQ, Q, SS * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->dpi, pi_root, S * sizeof(double), hipMemcpyHostToDevice));
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (kernel_ms) {
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    HIP_TRY(hipEventRecord(ev0, 0));
  }
  // the transition bank P_beta = expm(grid[beta] Q) by the bank's own expm (scaling and squaring: any rate matrix)
  int rc = cb_internal_expm_bank(h->hexp, h->dQ, nullptr, CB_PTR_DEVICE | CB_NO_SYNC, h->dP);
  if (rc == CB_OK) em_launch_passes(h);
  if (kernel_ms) {
    float ms = 0.f;
    hipError_t e = hipEventRecord(ev1, 0);
    if (e == hipSuccess) e = hipEventSynchronize(ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    *kernel_ms = ms;
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    if (e != hipSuccess && rc == CB_OK) rc = fail(CB_EHIP, "cb_em_estep: %s", hipGetErrorString(e));
  }
  if (rc != CB_OK) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(counts, h->dE, (size_t)h->B * SS * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> llp(h->n_units_all);
  HIP_TRY(hipMemcpy(llp.data(), h->dll, h->n_units_all * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> orig(h->n_units_all);   // the sites' log-likelihoods in the caller's unit order
  for (int f = 0; f < h->n_fam; ++f) {
    const EmFamHost &F = h->fam[f];
    const size_t ub = (size_t)h->famd[f].unit_base;
    for (int k = 0; k < F.n_units; ++k) orig[ub + F.perm[k]] = llp[ub + k];
    double s = 0.0;
    for (int u = 0; u < F.n_units; ++u) s += orig[ub + u];
    if (fam_ll) fam_ll[f] = s;
  }
  if (ll) std::copy(orig.begin(), orig.end(), ll);
  return CB_OK;
}
