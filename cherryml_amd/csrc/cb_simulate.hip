// libcherrybank: MSA simulation on a resident model (cherryml/simulation/_simulate_msas.py, simulation/simulate.cpp).
#include "cb_internal.hip.h"
#include "simulate.hip.h"

// ---------------------------------------------------------------- alias tables (host, double)
// Vose's method with the stable update p_g <- (p_g + p_l) - 1.  Zero-weight columns are paired first, so each is a "small"
// column with prob 0 and an alias of positive weight while the "large" list is certainly not empty; leftovers (rounding)
// keep prob 1 -- except a zero-weight column, which keeps prob 0 and points at the heaviest column.
extern "C" int cb_sim_alias_table(int n, const double *w, double *prob, int *alias) {
  if (n < 1 || !w || !prob || !alias) return fail(CB_EINVAL, "cb_sim_alias_table: bad arguments (n = %d)", n);
  double sum = 0.0;
  int heaviest = 0;
  for (int i = 0; i < n; ++i) {
    if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return fail(CB_EINVAL, "cb_sim_alias_table: w[%d] = %g", i, w[i]);
    sum += w[i];
    if (w[i] > w[heaviest]) heaviest = i;
  }
  if (!(sum > 0.0) || !std::isfinite(sum)) return fail(CB_EINVAL, "cb_sim_alias_table: the weights sum to %g", sum);
  std::vector<double> p(n);
  std::vector<int> small, large;
  for (int i = n - 1; i >= 0; --i) {   // (zero weights pushed last = popped first)
    p[i] = w[i] * (double)n / sum;
    if (w[i] > 0.0) (p[i] < 1.0 ? small : large).push_back(i);
  }
  for (int i = n - 1; i >= 0; --i)
    if (w[i] == 0.0) small.push_back(i);
  while (!small.empty() && !large.empty()) {
    const int l = small.back(), g = large.back();
    small.pop_back();
    large.pop_back();
    prob[l] = p[l];
    alias[l] = g;
    p[g] = (p[g] + p[l]) - 1.0;
    (p[g] < 1.0 ? small : large).push_back(g);
  }
  for (int g : large) { prob[g] = 1.0; alias[g] = g; }
  for (int l : small) {
    if (w[l] == 0.0) { prob[l] = 0.0; alias[l] = heaviest; }
    else { prob[l] = 1.0; alias[l] = l; }
  }
  return CB_OK;
}

// ---------------------------------------------------------------- the resident model
struct cb_sim_model_s {
  int device = 0, S1 = 0, S2 = 0;
  double max_exit1 = 0.0, max_exit2 = 0.0;
  // [prob S^2][exit S][piprob S] doubles and [alias S^2][pialias S] ints per model (1: singles, 2: pairs)
  double *d1 = nullptr, *d2 = nullptr;
  int *i1 = nullptr, *i2 = nullptr;
};

namespace {
// the tables of one model: row s = alias table of the off-diagonal rates of Q (an absorbing row: prob 0, alias s -- never
// drawn, the waiting time is infinite), exit rate -Q[s,s], root table of pi
int sim_tables(int S, const double *Q, const double *pi, std::vector<double> &dbl, std::vector<int> &ints, double &max_exit,
               const char *what) {
  const size_t SS = (size_t)S * S;
  dbl.assign(SS + 2 * (size_t)S, 0.0);
  ints.assign(SS + S, 0);
  max_exit = 0.0;
  std::vector<double> w(S);
  for (int s = 0; s < S; ++s) {
    double off = 0.0;
    for (int k = 0; k < S; ++k) {
      const double q = Q[(size_t)s * S + k];
      if (!std::isfinite(q) || (k != s && q < 0.0))
        return fail(CB_EINVAL, "cb_sim_model_create: %s[%d][%d] = %g", what, s, k, q);
      w[k] = k == s ? 0.0 : q;
      off += w[k];
    }
    const double exit_rate = -Q[(size_t)s * S + s];
    if (!(exit_rate >= 0.0)) return fail(CB_EINVAL, "cb_sim_model_create: %s[%d][%d] = %g (an exit rate < 0)", what, s, s, -exit_rate);
    if (exit_rate > 0.0 && !(off > 0.0))
      return fail(CB_EINVAL, "cb_sim_model_create: row %d of %s leaves at rate %g but has no off-diagonal rate", s, what, exit_rate);
    dbl[SS + s] = exit_rate;
    max_exit = std::max(max_exit, exit_rate);
    if (off > 0.0) {
      const int rc = cb_sim_alias_table(S, w.data(), dbl.data() + (size_t)s * S, ints.data() + (size_t)s * S);
      if (rc != CB_OK) return rc;
    } else {
      for (int k = 0; k < S; ++k) { dbl[(size_t)s * S + k] = 0.0; ints[(size_t)s * S + k] = s; }
    }
  }
  const int rc = cb_sim_alias_table(S, pi, dbl.data() + SS + S, ints.data() + SS);
  if (rc != CB_OK) {
    const std::string why = cb_last_error();
    return fail(rc, "cb_sim_model_create: the root distribution of %s: %s", what, why.c_str());
  }
  return CB_OK;
}

int sim_upload(const std::vector<double> &dbl, const std::vector<int> &ints, double **d, int **i) {
  HIP_TRY(hipMalloc((void **)d, dbl.size() * sizeof(double)));
  HIP_TRY(hipMalloc((void **)i, ints.size() * sizeof(int)));
  HIP_TRY(hipMemcpy(*d, dbl.data(), dbl.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(*i, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice));
  return CB_OK;
}
}  // namespace

extern "C" int cb_sim_model_destroy(cb_sim_model_s *m) {
  if (!m) return CB_OK;
  (void)hipSetDevice(m->device);
  for (void *p : {(void *)m->d1, (void *)m->d2, (void *)m->i1, (void *)m->i2})
    if (p) (void)hipFree(p);
  delete m;
  return CB_OK;
}

extern "C" int cb_sim_model_create(int device, int S1, const double *Q1, const double *pi1, const double *Q2, const double *pi2,
                                   cb_sim_model_s **out) {
  if (!Q1 || !pi1 || !out) return fail(CB_EINVAL, "cb_sim_model_create: NULL argument");
  if (S1 < 2 || S1 > SIM_MAX_S1) return fail(CB_EINVAL, "cb_sim_model_create: S1 = %d (2 .. %d states)", S1, SIM_MAX_S1);
  if ((Q2 == nullptr) != (pi2 == nullptr)) return fail(CB_EINVAL, "cb_sim_model_create: Q2 and pi2 go together");
  std::vector<double> dbl1, dbl2;
  std::vector<int> int1, int2;
  double mx1 = 0.0, mx2 = 0.0;
  int rc = sim_tables(S1, Q1, pi1, dbl1, int1, mx1, "Q1");
  if (rc == CB_OK && Q2) rc = sim_tables(S1 * S1, Q2, pi2, dbl2, int2, mx2, "Q2");
  if (rc != CB_OK) return rc;
  const int ndev = cb_device_count();
  if (ndev <= 0) return fail(CB_EHIP, "cb_sim_model_create: no HIP device (this path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(CB_EINVAL, "cb_sim_model_create: device %d of %d", device, ndev);
  HIP_TRY(hipSetDevice(device));
  cb_sim_model_s *m = new cb_sim_model_s;
  m->device = device; m->S1 = S1; m->S2 = Q2 ? S1 * S1 : 0;
  m->max_exit1 = mx1; m->max_exit2 = mx2;
  rc = sim_upload(dbl1, int1, &m->d1, &m->i1);
  if (rc == CB_OK && Q2) rc = sim_upload(dbl2, int2, &m->d2, &m->i2);
  if (rc != CB_OK) {
    (void)hipDeviceSynchronize();
    cb_sim_model_destroy(m);
    return rc;
  }
  *out = m;
  return CB_OK;
}

namespace {
// every family's tree, units and rates, checked on the host before anything is uploaded
int sim_validate(const cb_sim_model_s &m, int n_fam, const int *n_nodes, const int *parent, const double *length,
                 const int *n_sites, const int *n_units, const int *ua, const int *ub, const double *rate,
                 std::vector<long long> &node_off, std::vector<long long> &unit_off, std::vector<long long> &out_off,
                 std::vector<int> &blk_off) {
  node_off.assign(n_fam, 0); unit_off.assign(n_fam, 0); out_off.assign(n_fam, 0); blk_off.assign(n_fam + 1, 0);
  long long no = 0, uo = 0, oo = 0, blocks = 0;
  std::vector<char> covered;
  for (int f = 0; f < n_fam; ++f) {
    const int nn = n_nodes[f], L = n_sites[f], U = n_units[f];
    if (nn < 1 || L < 0 || U < 0 || U > L)
      return fail(CB_EINVAL, "cb_sim_model_run: family %d has bad sizes (nodes = %d, sites = %d, units = %d)", f, nn, L, U);
    node_off[f] = no; unit_off[f] = uo; out_off[f] = oo; blk_off[f] = (int)blocks;
    const int *par = parent + no;
    const double *len = length + no;
    if (par[0] != -1) return fail(CB_EINVAL, "cb_sim_model_run: family %d: node 0 must be the root (parent -1)", f);
    double max_len = 0.0;
    for (int v = 1; v < nn; ++v) {
      if (par[v] < 0 || par[v] >= v) return fail(CB_EINVAL, "cb_sim_model_run: family %d: parent[%d] = %d is not an earlier node "
                                                "(the nodes must be in preorder)", f, v, par[v]);
      if (!(len[v] >= 0.0) || !std::isfinite(len[v])) return fail(CB_EINVAL, "cb_sim_model_run: family %d: length[%d] = %g", f, v, len[v]);
      max_len = std::max(max_len, len[v]);
    }
    covered.assign(L, 0);
    for (int u = 0; u < U; ++u) {
      const int a = ua[uo + u], b = ub[uo + u];
      const double r = rate[uo + u];
      if (a < 0 || a >= L || b < -1 || b >= L || a == b)
        return fail(CB_EINVAL, "cb_sim_model_run: family %d: unit %d has sites (%d, %d) of %d", f, u, a, b, L);
      if (b >= 0 && !m.S2) return fail(CB_EINVAL, "cb_sim_model_run: family %d: a pair unit, but the model has no Q2", f);
      if (covered[a] || (b >= 0 && covered[b]))
        return fail(CB_EINVAL, "cb_sim_model_run: family %d: site %d is in two units", f, covered[a] ? a : b);
      covered[a] = 1;
      if (b >= 0) covered[b] = 1;
      if (!(r >= 0.0) || !std::isfinite(r)) return fail(CB_EINVAL, "cb_sim_model_run: family %d: unit_rate[%d] = %g", f, u, r);
      const double jumps = max_len * r * (b >= 0 ? m.max_exit2 : m.max_exit1);
      if (jumps > CB_SIM_MAX_JUMPS)
        return fail(CB_EINVAL, "cb_sim_model_run: family %d: unit %d expects %.3g jumps on its longest edge (at most %.0g)", f, u,
                    jumps, CB_SIM_MAX_JUMPS);
    }
    for (int s = 0; s < L; ++s)
      if (!covered[s]) return fail(CB_EINVAL, "cb_sim_model_run: family %d: site %d is in no unit", f, s);
    no += nn; uo += U; oo += (long long)nn * L;
    blocks += (U + SIM_BLOCK - 1) / SIM_BLOCK;
    if (blocks > INT32_MAX / 2) return fail(CB_EINVAL, "cb_sim_model_run: too many units in one call");
  }
  blk_off[n_fam] = (int)blocks;
  return CB_OK;
}
}  // namespace

extern "C" int cb_sim_model_run(cb_sim_model_s *m, int n_fam, const uint64_t *fam_seed, const int *n_nodes, const int *parent,
                                const double *length, const int *n_sites, const int *n_units, const int *unit_site_a,
                                const int *unit_site_b, const double *unit_rate, int8_t *out, double *kernel_ms) {
  if (!m) return fail(CB_EINVAL, "cb_sim_model_run: NULL model");
  if (n_fam < 1 || !fam_seed || !n_nodes || !parent || !length || !n_sites || !n_units || !out)
    return fail(CB_EINVAL, "cb_sim_model_run: NULL argument or no family (n_fam = %d)", n_fam);
  long long total_units = 0;
  for (int f = 0; f < n_fam; ++f) total_units += std::max(n_units[f], 0);
  if (total_units > 0 && (!unit_site_a || !unit_site_b || !unit_rate)) return fail(CB_EINVAL, "cb_sim_model_run: NULL unit arrays");
  std::vector<long long> node_off, unit_off, out_off;
  std::vector<int> blk_off;
  int rc = sim_validate(*m, n_fam, n_nodes, parent, length, n_sites, n_units, unit_site_a, unit_site_b, unit_rate, node_off,
                        unit_off, out_off, blk_off);
  if (rc != CB_OK) return rc;
  const long long total_nodes = node_off[n_fam - 1] + n_nodes[n_fam - 1];
  const long long total_out = out_off[n_fam - 1] + (long long)n_nodes[n_fam - 1] * n_sites[n_fam - 1];
  if (kernel_ms) *kernel_ms = 0.0;
  if (blk_off[n_fam] == 0) {   // no unit anywhere: nothing to draw
    if (total_out) std::memset(out, 0, (size_t)total_out);
    return CB_OK;
  }
  HIP_TRY(hipSetDevice(m->device));
  hipEvent_t ev[2] = {nullptr, nullptr};
  {
    CbDevBufs bufs;
    SimArgs a{};
    a.S1 = m->S1; a.S2 = m->S2;
    const size_t SS1 = (size_t)m->S1 * m->S1, SS2 = (size_t)m->S2 * m->S2;
    a.prob1 = m->d1; a.exit1 = m->d1 + SS1; a.piprob1 = m->d1 + SS1 + m->S1;
    a.alias1 = m->i1; a.pialias1 = m->i1 + SS1;
    if (m->S2) {
      a.prob2 = m->d2; a.exit2 = m->d2 + SS2; a.piprob2 = m->d2 + SS2 + m->S2;
      a.alias2 = m->i2; a.pialias2 = m->i2 + SS2;
    }
    a.n_fam = n_fam;
    a.blk_off = bufs.up(blk_off.data(), blk_off.size(), rc);
    a.n_nodes = bufs.up(n_nodes, n_fam, rc);
    a.n_sites = bufs.up(n_sites, n_fam, rc);
    a.n_units = bufs.up(n_units, n_fam, rc);
    a.node_off = bufs.up(node_off.data(), n_fam, rc);
    a.unit_off = bufs.up(unit_off.data(), n_fam, rc);
    a.out_off = bufs.up(out_off.data(), n_fam, rc);
    a.seed = bufs.up(reinterpret_cast<const unsigned long long *>(fam_seed), n_fam, rc);
    a.parent = bufs.up(parent, total_nodes, rc);
    a.length = bufs.up(length, total_nodes, rc);
    a.site_a = bufs.up(unit_site_a, total_units, rc);
    a.site_b = bufs.up(unit_site_b, total_units, rc);
    a.rate = bufs.up(unit_rate, total_units, rc);
    a.out = bufs.up<int8_t>(nullptr, total_out, rc);
    // sites no unit covers cannot exist (validated), so every output byte is written by the kernel
    const size_t lds = SS1 * (sizeof(double) + sizeof(int)) + m->S1 * (2 * sizeof(double) + sizeof(int));
    if (rc == CB_OK && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess))
      rc = fail(CB_EHIP, "cb_sim_model_run: hipEventCreate failed");
    if (rc == CB_OK) {
      (void)hipEventRecord(ev[0], 0);
      hipLaunchKernelGGL(sim_walk, dim3(blk_off[n_fam]), dim3(SIM_BLOCK), lds, 0, a);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) rc = fail(CB_EHIP, "cb_sim_model_run: sim_walk launch failed: %s", hipGetErrorString(e));
      (void)hipEventRecord(ev[1], 0);
    }
    if (rc == CB_OK && hipMemcpyAsync(out, a.out, (size_t)total_out, hipMemcpyDeviceToHost, 0) != hipSuccess)
      rc = fail(CB_EHIP, "cb_sim_model_run: download failed");
    const hipError_t se = hipStreamSynchronize(0);   // every path, errors included: nothing is left in flight
    if (rc == CB_OK && se != hipSuccess) rc = fail(CB_EHIP, "cb_sim_model_run: sim_walk failed: %s", hipGetErrorString(se));
    if (rc == CB_OK && kernel_ms) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) *kernel_ms = ms;
    }
  }
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}
