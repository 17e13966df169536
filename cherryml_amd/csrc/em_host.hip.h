// Device side of the tree EM handles (cb_em.hip, cb_bl.hip): the forest's resident buffers, a family's view of them, the inside
// and outside passes and the way back of l_u.  The host side (validation, layout, unit order) is em_layout.h.
#pragma once
#include "cb_internal.hip.h"
#include "em_layout.h"
#include "em_shared.hip.h"

// what a create does before its first allocation: a device, `device` among them, the current one
static int em_open_device(const char *who, int device) {
  const int ndev = cb_device_count();
  if (ndev <= 0) return fail(CB_EHIP, "%s: no HIP device (this path has no CPU fallback)", who);
  if (device < 0 || device >= ndev) return fail(CB_EINVAL, "%s: device %d of %d", who, device, ndev);
  if (hipSetDevice(device) != hipSuccess) return fail(CB_EHIP, "%s: hipSetDevice(%d) failed", who, device);
  return CB_OK;
}

// family f of a forest on the device: where each of its arrays starts
struct EmFamView {
  const EmFamHost &F;
  int n_blocks;   // site tiles of a launch: 64 / S units per wave
  int *parent, *child_ptr, *child_idx, *level_nodes, *depth_nodes, *qb, *unit_cat;
  signed char *codes;   // [node][unit]
  double *msg, *U;      // [node][unit][S]
  double *ll;           // [unit]
};

struct EmForest {
  int device = 0, S = 0;
  EmForestHost host;
  std::vector<void *> bufs;   // every device buffer of the handle, the owner's own included
  int *dparent = nullptr, *dcp = nullptr, *dci = nullptr, *dlev = nullptr, *ddep = nullptr, *dqb = nullptr, *duc = nullptr;
  signed char *dcodes = nullptr;
  double *dmsg = nullptr, *dU = nullptr, *dll = nullptr;

  // `count` elements (at least one), from `src` when not null; after a failure (rc) it does nothing
  template <typename T>
  T *alloc(const char *who, const T *src, size_t count, int &rc) {
    if (rc != CB_OK) return nullptr;
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      rc = fail(CB_ENOMEM, "%s: %zu bytes of device memory", who, count * sizeof(T));
      return nullptr;
    }
    bufs.push_back(p);
    if (src && count && hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(CB_EHIP, "%s: upload failed", who);
    return static_cast<T *>(p);
  }
  // the host's arrays, and the messages and l_u of all families
  void upload(const char *who, int &rc) {
    const size_t NU = host.off_c.back();
    dmsg = alloc<double>(who, nullptr, NU * S, rc);
    dU = alloc<double>(who, nullptr, NU * S, rc);
    dll = alloc<double>(who, nullptr, host.off_u.back(), rc);
    dparent = alloc(who, host.parent.data(), host.parent.size(), rc);
    dcp = alloc(who, host.child_ptr.data(), host.child_ptr.size(), rc);
    dci = alloc(who, host.child_idx.data(), host.child_idx.size(), rc);
    dlev = alloc(who, host.level_nodes.data(), host.level_nodes.size(), rc);
    ddep = alloc(who, host.depth_nodes.data(), host.depth_nodes.size(), rc);
    dqb = alloc(who, host.qb.data(), host.qb.size(), rc);
    duc = alloc(who, host.unit_cat.data(), host.unit_cat.size(), rc);
    dcodes = reinterpret_cast<signed char *>(alloc(who, host.codes.data(), NU, rc));
  }
  void free_all() {
    for (void *p : bufs)
      if (p) (void)hipFree(p);
    bufs.clear();
  }
  EmFamView view(int f) const {
    const EmFamHost &F = host.fam[f];
    const size_t on = host.off_n[f], oc = host.off_c[f];
    const int upw = 64 / S;
    return EmFamView{F, (F.n_units + upw - 1) / upw, dparent + on, dcp + on + f, dci + on, dlev + on, ddep + host.off_dep[f],
                     dqb + host.off_q[f], duc + host.off_u[f], dcodes + oc, dmsg + oc * S, dU + oc * S, dll + host.off_u[f]};
  }
};

// the inside pass of family f (and its outside pass) with the bank P and the root distribution, stream 0
static void em_launch_passes(const EmForest &T, int f, const double *P, const double *pi_root, bool outside) {
  const EmFamView w = T.view(f);
  const EmFamHost &F = w.F;
  TlArgs a{};
  a.S = T.S; a.S1 = 0; a.n_nodes = F.n_nodes; a.n_units = F.n_units; a.NU = F.n_units; a.root = F.root; a.n_blocks = w.n_blocks;
  a.child_ptr = w.child_ptr; a.child_idx = w.child_idx; a.P = P; a.unit_cat = w.unit_cat; a.code_a = w.codes; a.code_b = nullptr;
  a.pi_root = pi_root; a.msg = w.msg; a.ll = w.ll;
  for (size_t l = 0; l + 1 < F.level_ptr.size(); ++l) {
    TlArgs b = a;
    b.level_nodes = w.level_nodes + F.level_ptr[l];
    b.n_level = F.level_ptr[l + 1] - F.level_ptr[l];
    em_launch_up(b, w.qb, F.n_cats, (unsigned)(b.n_level * w.n_blocks));
  }
  if (!outside) return;
  EmDownArgs d{};
  d.S = T.S; d.n_units = F.n_units; d.root = F.root; d.n_blocks = w.n_blocks; d.n_cats = F.n_cats;
  d.parent = w.parent; d.child_ptr = w.child_ptr; d.child_idx = w.child_idx; d.qb = w.qb; d.unit_cat = w.unit_cat; d.P = P;
  d.pi_root = pi_root; d.msg = w.msg; d.U = w.U;
  for (size_t l = 0; l + 1 < F.depth_ptr.size(); ++l) {
    const int nl = F.depth_ptr[l + 1] - F.depth_ptr[l];
    if (nl == 0) continue;
    EmDownArgs e = d;
    e.level_nodes = w.depth_nodes + F.depth_ptr[l];
    em_launch_down(e, (unsigned)(nl * w.n_blocks));
  }
}

// l_u of the device (category order) -> orig, the caller's unit order; fam_ll (or null) takes the sums of the families in `which`
// (null: of all), in the caller's order
static int em_read_ll(const EmForest &T, const char *which, std::vector<double> &orig, double *fam_ll) {
  const size_t n = T.host.off_u.back();
  std::vector<double> llp(n);
  orig.resize(n);
  HIP_TRY(hipMemcpy(llp.data(), T.dll, n * sizeof(double), hipMemcpyDeviceToHost));
  for (int f = 0; f < T.host.n_fam(); ++f) {
    const EmFamHost &F = T.host.fam[f];
    const size_t ub = T.host.off_u[f];
    em_unpermute(F.perm, llp.data() + ub, orig.data() + ub);
    if (fam_ll && (!which || which[f])) fam_ll[f] = em_family_ll(orig.data() + ub, F.n_units);
  }
  return CB_OK;
}
