// Host side of the tree EM handles (cb_em.hip, cb_bl.hip) and of the site-rate scan (cb_sr.hip): the quantisation rule, one
// family's validation and host-side structures, the model check, the forest (the families of a handle, concatenated as the device
// takes them) and the way back from the device's unit order to the caller's.  `who` names the entry point in the messages.
// No HIP header: tests/em_layout_driver.cpp builds it with the host compiler.  (static: nothing of this header is a symbol of the
// library)
#pragma once
#include <stddef.h>

#include "../../include/cherrybank.h"

#include <algorithm>
#include <cmath>
#include <vector>

int cb_fail(int code, const char *fmt, ...);   // cherrybank.hip: sets cb_last_error(), returns `code`

namespace {
// the reference's quantisation rule (cherryml/utils.py:35-56, counting.hip.h cnt_quantize), clamped to the grid's ends:
// every edge of the tree needs a transition matrix
int em_quantize(double t, const double *grid, int B) {
  if (!(t > grid[0])) return 0;
  if (t >= grid[B - 1]) return B - 1;
  const int lo = int(std::lower_bound(grid, grid + B, t) - grid);
  const double rel_left = t / grid[lo - 1] - 1.0, rel_right = grid[lo] / t - 1.0;
  return rel_left < rel_right ? lo - 1 : lo;
}

struct EmFamHost {
  int n_nodes = 0, n_units = 0, n_cats = 0, root = -1;
  std::vector<int> child_ptr, child_idx, level_ptr, level_nodes, depth_ptr, depth_nodes, perm, unit_cat, cat_ptr, qb;
  std::vector<double> cats;   // the distinct site rates, ascending
};
}  // namespace

// validation and the host-side structures of one family (no device work)
static int em_prepare(const char *who, int S, int B, const double *grid, int n, const int *parent, const double *length, int U,
                      const double *rate, const int8_t *codes, int f, EmFamHost &F) {
  if (n < 1 || U < 1) return cb_fail(CB_EINVAL, "%s: family %d has bad sizes (nodes = %d, units = %d)", who, f, n, U);
  F.n_nodes = n;
  F.n_units = U;
  std::vector<int> nchild(n, 0);
  for (int v = 0; v < n; ++v) {
    const int p = parent[v];
    if (p == -1) {
      if (F.root >= 0) return cb_fail(CB_EINVAL, "%s: family %d has two roots (%d and %d)", who, f, F.root, v);
      F.root = v;
    } else if (p < 0 || p >= n || p == v) {
      return cb_fail(CB_EINVAL, "%s: family %d: parent[%d] = %d", who, f, v, p);
    } else {
      nchild[p]++;
      if (!(length[v] >= 0.0) || !std::isfinite(length[v]))
        return cb_fail(CB_EINVAL, "%s: family %d: length[%d] = %g", who, f, v, length[v]);
    }
  }
  if (F.root < 0) return cb_fail(CB_EINVAL, "%s: family %d has no root (parent -1)", who, f);
  F.child_ptr.assign(n + 1, 0);
  for (int v = 0; v < n; ++v) F.child_ptr[v + 1] = F.child_ptr[v] + nchild[v];
  F.child_idx.assign(std::max(n - 1, 1), 0);
  std::vector<int> fill(n, 0);
  for (int v = 0; v < n; ++v)
    if (parent[v] >= 0) F.child_idx[F.child_ptr[parent[v]] + fill[parent[v]]++] = v;
  // depths from the root (breadth first): every node reached exactly once <=> the parent array is a tree
  std::vector<int> depth(n, -1), order;
  order.reserve(n);
  order.push_back(F.root);
  depth[F.root] = 0;
  for (size_t i = 0; i < order.size(); ++i) {
    const int v = order[i];
    for (int c = F.child_ptr[v]; c < F.child_ptr[v + 1]; ++c) {
      depth[F.child_idx[c]] = depth[v] + 1;
      order.push_back(F.child_idx[c]);
    }
  }
  if ((int)order.size() != n) return cb_fail(CB_EINVAL, "%s: family %d: the parent array is not a tree (a cycle)", who, f);
  std::vector<int> height(n, 0);
  for (int i = n - 1; i > 0; --i) height[parent[order[i]]] = std::max(height[parent[order[i]]], height[order[i]] + 1);
  const int nh = height[F.root] + 1;
  F.level_ptr.assign(nh + 1, 0);
  for (int v = 0; v < n; ++v) F.level_ptr[height[v] + 1]++;
  for (int l = 0; l < nh; ++l) F.level_ptr[l + 1] += F.level_ptr[l];
  F.level_nodes.assign(n, 0);
  {
    std::vector<int> at(F.level_ptr.begin(), F.level_ptr.end() - 1);
    for (int v = 0; v < n; ++v) F.level_nodes[at[height[v]]++] = v;
  }
  // internal non-root nodes by depth (the outside pass)
  int nd = 0;
  for (int v = 0; v < n; ++v) nd = std::max(nd, depth[v] + 1);
  F.depth_ptr.assign(nd + 1, 0);
  for (int v = 0; v < n; ++v)
    if (v != F.root && nchild[v] > 0) F.depth_ptr[depth[v] + 1]++;
  for (int l = 0; l < nd; ++l) F.depth_ptr[l + 1] += F.depth_ptr[l];
  F.depth_nodes.assign(std::max(F.depth_ptr[nd], 1), 0);
  {
    std::vector<int> at(F.depth_ptr.begin(), F.depth_ptr.end() - 1);
    for (int v : order)
      if (v != F.root && nchild[v] > 0) F.depth_nodes[at[depth[v]]++] = v;
  }
  // rate categories (distinct rates, ascending) and the units sorted by category (stable)
  std::vector<double> cats(rate, rate + U);
  for (int u = 0; u < U; ++u)
    if (!(rate[u] >= 0.0) || !std::isfinite(rate[u]))
      return cb_fail(CB_EINVAL, "%s: family %d: site rate %d = %g", who, f, u, rate[u]);
  std::sort(cats.begin(), cats.end());
  cats.erase(std::unique(cats.begin(), cats.end()), cats.end());
  F.n_cats = (int)cats.size();
  F.cats = cats;
  std::vector<int> ucat(U);
  for (int u = 0; u < U; ++u) ucat[u] = int(std::lower_bound(cats.begin(), cats.end(), rate[u]) - cats.begin());
  F.perm.resize(U);
  for (int u = 0; u < U; ++u) F.perm[u] = u;
  std::stable_sort(F.perm.begin(), F.perm.end(), [&](int x, int y) { return ucat[x] < ucat[y]; });
  F.unit_cat.resize(U);
  F.cat_ptr.assign(F.n_cats + 1, 0);
  for (int k = 0; k < U; ++k) {
    F.unit_cat[k] = ucat[F.perm[k]];
    F.cat_ptr[F.unit_cat[k] + 1]++;
  }
  for (int c = 0; c < F.n_cats; ++c) F.cat_ptr[c + 1] += F.cat_ptr[c];
  F.qb.assign((size_t)n * F.n_cats, 0);
  for (int v = 0; v < n; ++v)
    if (v != F.root)
      for (int c = 0; c < F.n_cats; ++c) F.qb[(size_t)v * F.n_cats + c] = em_quantize(length[v] * cats[c], grid, B);
  for (int v = 0; v < n; ++v)
    if (!nchild[v])
      for (int u = 0; u < U; ++u)
        if (codes[(size_t)v * U + u] >= S || codes[(size_t)v * U + u] < -1)
          return cb_fail(CB_EINVAL, "%s: family %d: state code %d out of range [-1, S) at node %d unit %d", who, f,
                         (int)codes[(size_t)v * U + u], v, u);
  return CB_OK;
}

// a rate matrix (finite, off-diagonal >= 0) and a root distribution (finite, >= 0, positive sum)
static int em_check_model(const char *who, int S, const double *Q, const double *pi_root) {
  double psum = 0.0;
  for (int i = 0; i < S; ++i) {
    if (!(pi_root[i] >= 0.0) || !std::isfinite(pi_root[i])) return cb_fail(CB_EINVAL, "%s: pi_root[%d] = %g", who, i, pi_root[i]);
    psum += pi_root[i];
    for (int j = 0; j < S; ++j)
      if (!std::isfinite(Q[i * S + j]) || (i != j && Q[i * S + j] < 0.0))
        return cb_fail(CB_EINVAL, "%s: Q[%d][%d] = %g", who, i, j, Q[i * S + j]);
  }
  if (!(psum > 0.0)) return cb_fail(CB_EINVAL, "%s: pi_root sums to %g", who, psum);
  return CB_OK;
}

// the families of a resident handle: per-family offsets [n_fam + 1] and the arrays the device takes, concatenated in family
// order -- child_ptr keeps every family's n + 1 entries (family f at off_n[f] + f), child_idx its n - 1, depth_nodes its padded
// list (off_dep), qb [node][n_cats] at off_q, unit_cat and the codes' units in category order (EmFamHost::perm)
struct EmForestHost {
  std::vector<EmFamHost> fam;
  std::vector<size_t> off_n{0}, off_u{0}, off_c{0}, off_q{0}, off_dep{0};   // nodes, units, codes (nodes x units), qb, depth list
  std::vector<int> parent, child_ptr, child_idx, level_nodes, depth_nodes, qb, unit_cat;
  std::vector<int8_t> codes;
  int n_fam() const { return (int)fam.size(); }
};

// the builder, a family at a time (a caller's own refusals stay between em_prepare's): validates the next family of the caller's
// concatenated inputs -- the forest's own offsets say where it starts -- and appends it.  A refused family leaves T as it was.
// qb holds em_prepare's grid indices; a caller with entries of its own (cb_bl_create) rewrites T.qb from off_q[f] on.
static inline int em_forest_add(EmForestHost &T, const char *who, int S, int B, const double *grid, int n, const int *parent,
                                const double *length, int U, const double *rate, const int8_t *codes) {
  const int f = T.n_fam();
  const size_t on = T.off_n[f], oc = T.off_c[f];
  EmFamHost F;
  const int rc = em_prepare(who, S, B, grid, n, parent + on, length + on, U, rate + T.off_u[f], codes + oc, f, F);
  if (rc != CB_OK) return rc;
  T.parent.insert(T.parent.end(), parent + on, parent + on + n);
  T.child_ptr.insert(T.child_ptr.end(), F.child_ptr.begin(), F.child_ptr.end());
  T.child_idx.insert(T.child_idx.end(), F.child_idx.begin(), F.child_idx.begin() + (n - 1));
  T.child_idx.push_back(0);   // (the concatenation has one slot per node)
  T.level_nodes.insert(T.level_nodes.end(), F.level_nodes.begin(), F.level_nodes.end());
  T.depth_nodes.insert(T.depth_nodes.end(), F.depth_nodes.begin(), F.depth_nodes.end());
  T.qb.insert(T.qb.end(), F.qb.begin(), F.qb.end());
  T.unit_cat.insert(T.unit_cat.end(), F.unit_cat.begin(), F.unit_cat.end());
  T.codes.resize(oc + (size_t)n * U);
  for (int v = 0; v < n; ++v)
    for (int k = 0; k < U; ++k) T.codes[oc + (size_t)v * U + k] = codes[oc + (size_t)v * U + F.perm[k]];
  T.off_n.push_back(on + n);
  T.off_u.push_back(T.off_u[f] + U);
  T.off_c.push_back(oc + (size_t)n * U);
  T.off_q.push_back(T.qb.size());
  T.off_dep.push_back(T.depth_nodes.size());
  T.fam.push_back(std::move(F));
  return CB_OK;
}

// rows of `width` elements from the device's unit order (category order) to the caller's: dst row perm[k] = src row k
template <typename T>
static inline void em_unpermute(const std::vector<int> &perm, const T *src, T *dst, size_t width = 1) {
  if (width == 1) {   // (an assignment per element, not a copy call)
    for (size_t k = 0; k < perm.size(); ++k) dst[perm[k]] = src[k];
    return;
  }
  for (size_t k = 0; k < perm.size(); ++k) std::copy(src + k * width, src + (k + 1) * width, dst + (size_t)perm[k] * width);
}

// a family's log-likelihood: l_u in the caller's unit order, summed from unit 0 up (the bits depend on the order)
static inline double em_family_ll(const double *ll, int U) {
  double s = 0.0;
  for (int u = 0; u < U; ++u) s += ll[u];
  return s;
}
