// libcherrybank: the E-step of full-tree EM on a resident handle (em.hip.h; include/cherrybank.h, cb_em_*).
#include "cb_internal.hip.h"
#include "common.hip.h"
#include "em.hip.h"
#include "em_host.hip.h"

namespace {
constexpr int EM_TASK_UNITS = 512;   // (edge, unit) pairs per accumulation task, at most

}  // namespace

struct cb_em_s {
  int B = 0, n_tasks = 0;
  EmForest forest;
  std::vector<EmFam> famd;
  cb_handle hexp = nullptr;               // counts-free expm handle over the grid points
  CbKernelTimer events{true};             // owns the two events a call's timer borrows
  double *dQ = nullptr, *dpi = nullptr, *dP = nullptr, *dpart = nullptr, *dE = nullptr;
  int *dtask_seg = nullptr, *dbucket_task = nullptr;
  EmFam *dfam = nullptr;
  EmSeg *dseg = nullptr;
};

extern "C" int cb_em_destroy(cb_em_s *h) {
  if (!h) return CB_OK;
  (void)hipSetDevice(h->forest.device);
  if (h->hexp) cb_destroy(h->hexp);
  h->forest.free_all();
  delete h;
  return CB_OK;
}

extern "C" int cb_em_create(int device, int S, int B, const double *grid, int n_fam, const int *n_nodes, const int *parent,
                            const double *length, const int *n_units, const double *unit_rate, const int8_t *codes,
                            cb_em_s **out) {
  static const char *who = "cb_em_create";
  if (!grid || !n_nodes || !parent || !length || !n_units || !unit_rate || !codes || !out)
    return fail(CB_EINVAL, "cb_em_create: NULL argument");
  *out = nullptr;
  if (S < 2 || S > 32) return fail(CB_EINVAL, "cb_em_create: S = %d (2 <= S <= 32: one 32 x 32 MFMA tile per task)", S);
  if (B < 1 || n_fam < 1) return fail(CB_EINVAL, "cb_em_create: bad sizes (B = %d, families = %d)", B, n_fam);
  for (int b = 0; b < B; ++b)
    if (!(grid[b] > 0.0) || !std::isfinite(grid[b]) || (b > 0 && !(grid[b] > grid[b - 1])))
      return fail(CB_EINVAL, "cb_em_create: the grid must be positive and strictly increasing (grid[%d] = %g)", b, grid[b]);
  cb_em_s *h = new cb_em_s;
  EmForest &T = h->forest;
  T.device = device; T.S = S; h->B = B;
  int rc = CB_OK;
  for (int f = 0; f < n_fam && rc == CB_OK; ++f)
    rc = em_forest_add(T.host, who, S, B, grid, n_nodes[f], parent, length, n_units[f], unit_rate, codes);
  if (rc != CB_OK) {
    cb_em_destroy(h);
    return rc;
  }
  // the accumulation's work: per bucket, the (edge, category) segments in (family, node, category) order, packed into tasks
  std::vector<std::vector<EmSeg>> per_bucket(B);
  for (int f = 0; f < n_fam; ++f) {
    const EmFamHost &F = T.host.fam[f];
    h->famd.push_back(EmFam{(long long)T.host.off_c[f], (int)T.host.off_n[f], (int)T.host.off_u[f], F.n_units, F.root});
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
  rc = em_open_device(who, device);
  const size_t SS = (size_t)S * S;
  h->dQ = T.alloc<double>(who, nullptr, SS, rc);
  h->dpi = T.alloc<double>(who, nullptr, S, rc);
  h->dP = T.alloc<double>(who, nullptr, (size_t)B * SS, rc);
  h->dE = T.alloc<double>(who, nullptr, (size_t)B * SS, rc);
  h->dpart = T.alloc<double>(who, nullptr, (size_t)h->n_tasks * SS, rc);
  T.upload(who, rc);
  h->dfam = T.alloc(who, h->famd.data(), h->famd.size(), rc);
  h->dseg = T.alloc(who, segs.data(), segs.size(), rc);
  h->dtask_seg = T.alloc(who, task_seg.data(), task_seg.size(), rc);
  h->dbucket_task = T.alloc(who, bucket_task.data(), bucket_task.size(), rc);
  if (rc == CB_OK) rc = h->events.create();
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

static void em_launch_estep(cb_em_s *h) {
  const EmForest &T = h->forest;
  const int S = T.S;
  for (int f = 0; f < T.host.n_fam(); ++f) em_launch_passes(T, f, h->dP, h->dpi, true);
  if (h->n_tasks > 0) {
    EmAccArgs c{};
    c.S = S; c.task_seg = h->dtask_seg; c.seg = h->dseg; c.fam = h->dfam; c.parent = T.dparent; c.child_ptr = T.dcp;
    c.child_idx = T.dci; c.codes = T.dcodes; c.pi_root = h->dpi; c.msg = T.dmsg; c.U = T.dU; c.ll = T.dll; c.part = h->dpart;
    hipLaunchKernelGGL(em_acc_kernel, dim3((unsigned)h->n_tasks), dim3(64), 0, 0, c);
  }
  hipLaunchKernelGGL(em_reduce_kernel, dim3((unsigned)h->B), dim3(256), 0, 0, S, h->dbucket_task, h->dpart, h->dP, h->dE);
}

extern "C" int cb_em_estep(cb_em_s *h, const double *Q, const double *pi_root, double *counts, double *ll, double *fam_ll,
                           double *kernel_ms) {
  if (!h) return fail(CB_EINVAL, "cb_em_estep: NULL handle");
  if (!Q || !pi_root || !counts) return fail(CB_EINVAL, "cb_em_estep: NULL argument");
  const int S = h->forest.S;
  const size_t SS = (size_t)S * S;
  int rc = em_check_model("cb_em_estep", S, Q, pi_root);
  if (rc != CB_OK) return rc;
  HIP_TRY(hipSetDevice(h->forest.device));
  HIP_TRY(hipMemcpy(h->dQ, Q, SS * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->dpi, pi_root, S * sizeof(double), hipMemcpyHostToDevice));
  CbKernelTimer timer(kernel_ms != nullptr, h->events.ev0, h->events.ev1);
  if ((rc = timer.begin(false)) != CB_OK) return rc;
  // the transition bank P_beta = expm(grid[beta] Q) by the bank's own expm (scaling and squaring: any rate matrix)
  if ((rc = cb_internal_expm_bank(h->hexp, h->dQ, nullptr, CB_PTR_DEVICE | CB_NO_SYNC, h->dP)) != CB_OK) return rc;
  em_launch_estep(h);
  if ((rc = timer.end(kernel_ms)) != CB_OK) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(counts, h->dE, (size_t)h->B * SS * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> orig;   // the sites' log-likelihoods in the caller's unit order
  if ((rc = em_read_ll(h->forest, nullptr, orig, fam_ll)) != CB_OK) return rc;
  if (ll) std::copy(orig.begin(), orig.end(), ll);
  return CB_OK;
}
