// Host-only arithmetic of FastCherries (cb_ble.hip): the rate priors, the initial site-rate bins, the transposes, the size checks
// that need no device and the offsets of a batch.  No HIP header: tests/ble_layout_driver.cpp builds it with the host compiler.
// (static, hidden: nothing of this header is a symbol of the library)
#pragma once
#include <stddef.h>

#include "../../include/cherrybank.h"

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

int cb_fail(int code, const char *fmt, ...);   // cherrybank.hip: sets cb_last_error(), returns `code`

// log density of Gamma(3, 3) up to a constant (branch_length_estimation.cpp:199-203)
static inline std::vector<double> ble_priors(const double *rates, int R) {
  std::vector<double> priors(R);
  for (int r = 0; r < R; ++r) priors[r] = 2 * std::log(rates[r]) - 3 * rates[r];
  return priors;
}

// :10-34: per site the number of ordered sequence pairs whose states differ, total [L]; a negative code is a gap
static inline int ble_site_totals(const int8_t *all_seqs, int n_seqs, int L, int S, long long *total) {
  std::vector<long long> cnt((size_t)L * S, 0);
  for (int i = 0; i < n_seqs; ++i)
    for (int j = 0; j < L; ++j) {
      const int v = all_seqs[(size_t)i * L + j];
      if (v >= S) return cb_fail(CB_EINVAL, "cb_ble: state code out of range");
      if (v >= 0) cnt[(size_t)j * S + v] += 1;
    }
  for (int j = 0; j < L; ++j) {
    long long non_missing = 0;
    total[j] = 0;
    for (int k = 0; k < S; ++k) non_missing += cnt[(size_t)j * S + k];
    for (int k = 0; k < S; ++k) total[j] += (non_missing - cnt[(size_t)j * S + k]) * cnt[(size_t)j * S + k];
  }
  return CB_OK;
}

// :36-58: sites ordered by their totals (ties: site index); the i-th site of that order gets category `cat`, which advances by
// one when i >= round(weights[cat] * L) (halves away from zero) and stops at R - 1
static inline void ble_bins_from_totals(const long long *total, int L, int R, const double *weights, int *s2r) {
  std::vector<std::pair<long long, int>> order(L);
  for (int j = 0; j < L; ++j) order[j] = {total[j], j};
  std::sort(order.begin(), order.end());
  int cat = 0;
  for (int i = 0; i < L; ++i) {
    if (cat < R && i >= std::llround(weights[cat] * L)) ++cat;
    s2r[order[i].second] = cat < R ? cat : R - 1;
  }
}

// initial site-rate bins (:10-58) of the sequences all_seqs [n_seqs][L]
static inline int ble_initial_bins(const int8_t *all_seqs, int n_seqs, int L, int S, int R, const double *weights, int *s2r) {
  std::vector<long long> total(L);
  const int rc = ble_site_totals(all_seqs, n_seqs, L, S, total.data());
  if (rc == CB_OK) ble_bins_from_totals(total.data(), L, R, weights, s2r);
  return rc;
}

// c [n][L] -> t [L][n]
static inline void ble_transpose(const int8_t *c, int n, int L, int8_t *t) {
  for (int i = 0; i < n; ++i)
    for (int s = 0; s < L; ++s) t[(size_t)s * n + i] = c[(size_t)i * L + s];
}

static inline int ble_check_sizes(int S, int T, int R, int n, int L) {
  if (S < 2 || S > 127 || T < 1 || R < 1 || n < 1 || L < 1) return cb_fail(CB_EINVAL, "ble: bad sizes");
  return CB_OK;
}

// (any negative code is a gap)
static inline int ble_check_codes(int S, int n, int L, const int8_t *cx, const int8_t *cy) {
  for (size_t i = 0; i < (size_t)n * L; ++i)
    if (cx[i] >= S || cy[i] >= S) return cb_fail(CB_EINVAL, "ble: state code out of range");
  return CB_OK;
}

// where family f's arrays start in the concatenated arrays of cb_ble_batch, each [n_fam + 1]
struct __attribute__((visibility("hidden"))) BleBatchOffsets {
  std::vector<size_t> off_c, off_n, off_L, off_s;   // cherry codes n L, cherries n, sites L, sequence codes n_seqs L
};
static inline int ble_batch_offsets(int n_fam, const int *n, const int *L, const int *n_seqs, BleBatchOffsets &o) {
  for (std::vector<size_t> *v : {&o.off_c, &o.off_n, &o.off_L, &o.off_s}) v->assign(n_fam + 1, 0);
  for (int f = 0; f < n_fam; ++f) {
    if (n[f] < 1 || L[f] < 1 || n_seqs[f] < 1) return cb_fail(CB_EINVAL, "cb_ble_batch: family %d has bad sizes", f);
    o.off_c[f + 1] = o.off_c[f] + (size_t)n[f] * L[f];
    o.off_n[f + 1] = o.off_n[f] + n[f];
    o.off_L[f + 1] = o.off_L[f] + L[f];
    o.off_s[f + 1] = o.off_s[f] + (size_t)n_seqs[f] * L[f];
  }
  return CB_OK;
}
