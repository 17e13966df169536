// Host-only layout of one held-out likelihood call (cb_likelihood.hip): the caller's concatenated per-family arrays, checked,
// and every table the device takes derived from them.  No HIP header: tests/tl_layout_driver.cpp builds it with the host compiler.
#pragma once
#include <stddef.h>

#include "../../include/cherrybank.h"

#include <algorithm>
#include <cmath>
#include <vector>

int cb_fail(int code, const char *fmt, ...);   // cherrybank.hip: sets cb_last_error(), returns `code`

// the caller's arrays (include/cherrybank.h, cb_tl_model_run): the families' arrays concatenated in order
struct TlCall {
  int n_fam;
  const int *n_nodes, *postorder, *parent;
  const double *length;
  const int *n_cats;
  const double *cat_rate;
  const int *n_units, *unit_cat;
  const int8_t *code_a, *code_b;
  double *ll;
};

// what needs no device to refuse; `model_given`: the entry point's model arguments (Q, pi_root) are there
inline int tl_check_call(int S, int S1, bool model_given, const TlCall &c) {
  if (!model_given || !c.n_nodes || !c.postorder || !c.parent || !c.length || !c.n_cats || !c.cat_rate || !c.n_units ||
      !c.unit_cat || !c.code_a || !c.ll)
    return cb_fail(CB_EINVAL, "cb_tree_likelihood: NULL argument");
  if (c.n_fam < 1) return cb_fail(CB_EINVAL, "cb_tree_likelihood: bad sizes (S = %d, families = %d)", S, c.n_fam);
  if (S1 > 0 && !c.code_b) return cb_fail(CB_EINVAL, "cb_tree_likelihood: pair model needs S = S1 * S1 and code_b");
  return CB_OK;
}

struct TlFamily {
  int n_nodes = 0, n_units = 0, n_cats = 0, root = 0, n_levels = 0;
  int NU = 0;                   // unit columns of a message: n_units, padded to the 32 of tl_mfma_kernel's widest block at S > 64
  size_t n_bank = 0;            // transition matrices in the family's bank
  std::vector<int> level_ptr;   // [n_levels + 1] into the family's level_nodes: the nodes of equal height
};

struct TlLayout {
  // S > 64 with a reversible model: the leaves take their messages from the eigendecomposition (tl_leaf_mfma_kernel) and the
  // bank holds the INTERNAL non-root nodes only -- at least one slot, so that a family of leaves still triggers the eigensolve
  bool factored = false;
  std::vector<TlFamily> fam;
  std::vector<size_t> off_n, off_u, off_c, off_k, off_t;   // [n_fam + 1]: nodes, units, codes, categories, bank slots
  size_t max_msg = 0, max_bank = 0;                        // doubles of messages / bank slots the largest family takes
  // family f's tree at off_n[f] (child_ptr, one entry longer per family, at off_n[f] + f); node indices local to the family
  std::vector<int> level_nodes, child_ptr, child_idx;
  // rate x length of the bank's slots at off_t[f]: [category][node] with the root at 0, or one per internal non-root node
  std::vector<double> t_all;
  std::vector<double> t_node;   // factored, at off_n[f]: rate x length of every node (root 0)
  std::vector<int> slot_all;    // factored, at off_n[f]: a node's bank slot, ascending by node index (-1: none)
};

// validates one tree; children in post-order (the reference's child order, _tree.py traversal), levels by height in post-order
inline int tl_tree(int n, const int *postorder, const int *parent, const double *length, TlFamily &F, int *level_nodes,
                   int *child_ptr, int *child_idx) {
  std::vector<int> height(n, 0), seen(n, 0);
  std::fill(child_ptr, child_ptr + n + 1, 0);
  for (int i = 0; i < n; ++i) {
    const int v = postorder[i];
    if (v < 0 || v >= n || seen[v]) return cb_fail(CB_EINVAL, "cb_tree_likelihood: postorder is not a permutation");
    seen[v] = 1;
    const int p = parent[v];
    if (i == n - 1) {
      if (p != -1) return cb_fail(CB_EINVAL, "cb_tree_likelihood: the last node of postorder must be the root (parent -1)");
      break;
    }
    if (p < 0 || p >= n || seen[p]) return cb_fail(CB_EINVAL, "cb_tree_likelihood: node %d precedes its child %d", p, v);
    if (!(length[v] >= 0.0) || !std::isfinite(length[v]))
      return cb_fail(CB_EINVAL, "cb_tree_likelihood: length[%d] = %g", v, length[v]);
    height[p] = std::max(height[p], height[v] + 1);
    child_ptr[p + 1]++;
  }
  F.root = postorder[n - 1];
  for (int v = 0; v < n; ++v) child_ptr[v + 1] += child_ptr[v];
  std::vector<int> at(child_ptr, child_ptr + n);
  for (int i = 0; i + 1 < n; ++i) child_idx[at[parent[postorder[i]]]++] = postorder[i];
  F.n_levels = height[F.root] + 1;
  F.level_ptr.assign(F.n_levels + 1, 0);
  for (int v = 0; v < n; ++v) F.level_ptr[height[v] + 1]++;
  for (int l = 0; l < F.n_levels; ++l) F.level_ptr[l + 1] += F.level_ptr[l];
  at.assign(F.level_ptr.begin(), F.level_ptr.end() - 1);
  for (int i = 0; i < n; ++i) level_nodes[at[height[postorder[i]]]++] = postorder[i];
  return CB_OK;
}

// a family's categories, rates and leaf codes (alphabet: S1 for pairs, else S); child_ptr: the family's, from tl_tree
inline int tl_check_units(int S, int S1, const TlFamily &F, const int *child_ptr, const double *cat_rate, const int *unit_cat,
                          const int8_t *code_a, const int8_t *code_b) {
  for (int u = 0; u < F.n_units; ++u)
    if (unit_cat[u] < 0 || unit_cat[u] >= F.n_cats)
      return cb_fail(CB_EINVAL, "cb_tree_likelihood: unit_cat[%d] = %d", u, unit_cat[u]);
  for (int c = 0; c < F.n_cats; ++c)
    if (!(cat_rate[c] >= 0.0) || !std::isfinite(cat_rate[c]))
      return cb_fail(CB_EINVAL, "cb_tree_likelihood: cat_rate[%d] = %g", c, cat_rate[c]);
  const int alpha = S1 > 0 ? S1 : S;
  for (int v = 0; v < F.n_nodes; ++v) {
    if (child_ptr[v + 1] > child_ptr[v]) continue;
    for (int u = 0; u < F.n_units; ++u) {
      const size_t i = (size_t)v * F.n_units + u;
      if (code_a[i] >= alpha || (S1 > 0 && code_b[i] >= alpha))
        return cb_fail(CB_EINVAL, "cb_tree_likelihood: state code out of range at node %d unit %d", v, u);
    }
  }
  return CB_OK;
}

// family f's bank slots and time tables, appended behind those of the families before it; sets n_bank and off_t[f + 1]
inline void tl_times(TlLayout &L, int f, const double *length, const double *cat_rate) {
  TlFamily &F = L.fam[f];
  const size_t on = L.off_n[f], ot = L.off_t[f];
  if (L.factored) {   // (one category at S > 64)
    L.t_node.resize(on + F.n_nodes);
    L.slot_all.resize(on + F.n_nodes);
    const int *cp = L.child_ptr.data() + on + f;
    int n_int = 0;
    for (int v = 0; v < F.n_nodes; ++v) {
      L.t_node[on + v] = v == F.root ? 0.0 : cat_rate[0] * length[v];
      L.slot_all[on + v] = (cp[v + 1] > cp[v] && v != F.root) ? n_int++ : -1;
    }
    F.n_bank = (size_t)std::max(n_int, 1);
    L.t_all.resize(ot + F.n_bank, 0.0);
    for (int v = 0; v < F.n_nodes; ++v)
      if (L.slot_all[on + v] >= 0) L.t_all[ot + L.slot_all[on + v]] = L.t_node[on + v];
  } else {
    F.n_bank = (size_t)F.n_cats * F.n_nodes;
    L.t_all.resize(ot + F.n_bank);
    for (int c = 0; c < F.n_cats; ++c)
      for (int v = 0; v < F.n_nodes; ++v)
        L.t_all[ot + (size_t)c * F.n_nodes + v] = v == F.root ? 0.0 : cat_rate[c] * length[v];
  }
  L.off_t[f + 1] = ot + F.n_bank;
}

// The layout of a call tl_check_call has passed, family by family: a refusal names the first family at fault.
inline int tl_layout(int S, int S1, bool reversible, const TlCall &c, TlLayout &L) {
  L = TlLayout{};
  L.factored = S > 64 && reversible;
  L.fam.resize(c.n_fam);
  for (std::vector<size_t> *o : {&L.off_n, &L.off_u, &L.off_c, &L.off_k, &L.off_t}) o->assign(c.n_fam + 1, 0);
  for (int f = 0; f < c.n_fam; ++f) {
    TlFamily &F = L.fam[f];
    const int n = c.n_nodes[f];
    const size_t on = L.off_n[f], ou = L.off_u[f], oc = L.off_c[f], ok = L.off_k[f];
    if (n < 1 || c.n_units[f] < 1 || c.n_cats[f] < 1) return cb_fail(CB_EINVAL, "cb_tree_likelihood: family %d has bad sizes", f);
    if (S > 64 && c.n_cats[f] != 1)
      return cb_fail(CB_EUNSUPPORTED, "cb_tree_likelihood: S > 64 takes one rate category (the reference evaluates pairs "
                     "of sites at rate 1, _likelihood.py:214-230)");
    F.n_nodes = n; F.n_units = c.n_units[f]; F.n_cats = c.n_cats[f];
    F.NU = S > 64 ? (F.n_units + 31) / 32 * 32 : F.n_units;
    L.level_nodes.resize(on + n);
    L.child_ptr.resize(on + f + n + 1);
    L.child_idx.resize(on + n);
    int rc = tl_tree(n, c.postorder + on, c.parent + on, c.length + on, F, L.level_nodes.data() + on,
                     L.child_ptr.data() + on + f, L.child_idx.data() + on);
    if (rc == CB_OK)
      rc = tl_check_units(S, S1, F, L.child_ptr.data() + on + f, c.cat_rate + ok, c.unit_cat + ou, c.code_a + oc,
                          c.code_b ? c.code_b + oc : nullptr);
    if (rc != CB_OK) return rc;
    L.off_n[f + 1] = on + n;
    L.off_u[f + 1] = ou + F.n_units;
    L.off_c[f + 1] = oc + (size_t)n * F.n_units;
    L.off_k[f + 1] = ok + F.n_cats;
    tl_times(L, f, c.length + on, c.cat_rate + ok);
    L.max_msg = std::max(L.max_msg, (size_t)n * S * F.NU);
    L.max_bank = std::max(L.max_bank, F.n_bank);
  }
  return CB_OK;
}
