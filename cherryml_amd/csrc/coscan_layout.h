// Host-only layout of the co-evolution scan (cb_coscan.hip): the checks of a call's families, the bucket of every sequence pair,
// the order the kernel walks them in (by bucket, ties by pair index), the tile list over the upper triangle of site pairs and
// the families' offsets.  No HIP header: tests/coscan_layout_driver.cpp builds it with the host compiler.
// (static, hidden: nothing of this header is a symbol of the library)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cherrybank.h"

#include <algorithm>
#include <unordered_set>
#include <vector>

int cb_fail(int code, const char *fmt, ...);   // cherrybank.hip: sets cb_last_error(), returns `code`

#define COSCAN_TILE 16     // a workgroup owns COSCAN_TILE x COSCAN_TILE site pairs: one per thread
#define COSCAN_MIN_S 2
#define COSCAN_MAX_S 20

// one kept sequence pair, in the order the kernel walks them
struct CoscanSeqPair {
  long long seq_a, seq_b;   // byte offsets of the two sequences in `seqs`
  int q;                    // bucket on the grid
  int index;                // the pair's index inside its family (before any was dropped)
};
// one family of a call
struct CoscanFam {
  unsigned long long out_off;    // first entry of its [L][L] outputs (size_t on the device)
  unsigned long long pair_off;   // first of its kept pairs in the sorted pair list
  int L, n_kept;
};
struct CoscanTileItem {
  int fam, ti, tj, pad;   // tile (ti <= tj) of family fam: sites ti * COSCAN_TILE .. x tj * COSCAN_TILE ..
};
struct CoscanLayout {
  std::vector<CoscanFam> fam;
  std::vector<CoscanSeqPair> pairs;
  std::vector<CoscanTileItem> tiles;
  size_t n_out = 0;   // sum of L^2
};

// cherryml/utils.py:35-56 in IEEE double arithmetic: counting.hip.h's cnt_quantize on the host (same comparisons, same divisions)
static inline int coscan_quantize(double bl, const double *grid, int B) {
  if (!(bl >= grid[0]) || bl > grid[B - 1]) return -1;
  int lo = 0, hi = B;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (grid[mid] < bl) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return 0;
  const double left = grid[lo - 1], right = grid[lo];
  const double rel_left = bl / left - 1.0, rel_right = right / bl - 1.0;
  return (rel_left < rel_right) ? lo - 1 : lo;
}

static inline int coscan_check_model(int S, int B, const double *grid) {
  if (S < COSCAN_MIN_S || S > COSCAN_MAX_S)
    return cb_fail(CB_EINVAL, "cb_coscan_create: S = %d (%d <= S <= %d: the pair model has S^2 <= 400 states)", S, COSCAN_MIN_S,
                   COSCAN_MAX_S);
  if (B < 2) return cb_fail(CB_EINVAL, "cb_coscan_create: B = %d (at least 2 grid points)", B);
  for (int b = 0; b < B; ++b)
    if (!(grid[b] > 0.0) || !(grid[b] < 1e300) || (b > 0 && !(grid[b] > grid[b - 1])))
      return cb_fail(CB_EINVAL, "cb_coscan_create: the grid must be positive and strictly increasing (grid[%d] = %g)", b, grid[b]);
  return CB_OK;
}

// The layout of one call.  Every family's pairs are checked (offsets, then the codes of the sequences they name) whether they
// are kept or not; a pair whose length is off the grid is dropped as the counter drops it.
static inline int coscan_layout(int S, int B, const double *grid, int n_fam, const int *L, const int8_t *seqs, int64_t seqs_bytes,
                                const cb_count_pair *pairs, const int64_t *n_pairs, CoscanLayout &out) {
  out = CoscanLayout();
  if (n_fam < 1) return cb_fail(CB_EINVAL, "cb_coscan_run: n_fam = %d", n_fam);
  if (seqs_bytes < 0) return cb_fail(CB_EINVAL, "cb_coscan_run: seqs_bytes = %lld", (long long)seqs_bytes);
  int64_t p0 = 0;
  for (int f = 0; f < n_fam; ++f) {
    if (L[f] < 1) return cb_fail(CB_EINVAL, "cb_coscan_run: family %d has L = %d", f, L[f]);
    if (n_pairs[f] < 0) return cb_fail(CB_EINVAL, "cb_coscan_run: family %d has n_pairs = %lld", f, (long long)n_pairs[f]);
    if (n_pairs[f] > INT32_MAX) return cb_fail(CB_EINVAL, "cb_coscan_run: family %d has n_pairs = %lld", f, (long long)n_pairs[f]);
    CoscanFam F;
    F.out_off = out.n_out;
    F.pair_off = out.pairs.size();
    F.L = L[f];
    std::vector<CoscanSeqPair> kept;
    std::unordered_set<int64_t> checked;   // a sequence many pairs share (every inner node in `edge` mode) is read once
    for (int64_t k = 0; k < n_pairs[f]; ++k) {
      const cb_count_pair &pr = pairs[p0 + k];
      for (const int64_t off : {pr.seq_a, pr.seq_b}) {
        if (off < 0 || off > seqs_bytes - L[f])
          return cb_fail(CB_EINVAL, "cb_coscan_run: family %d pair %lld: sequence offset %lld + L = %d lies beyond seqs_bytes = %lld",
                         f, (long long)k, (long long)off, L[f], (long long)seqs_bytes);
        if (!checked.insert(off).second) continue;
        for (int s = 0; s < L[f]; ++s) {
          const int c = seqs[off + s];
          if (c < -1 || c >= S)
            return cb_fail(CB_EINVAL, "cb_coscan_run: family %d pair %lld: state code %d out of range [-1, %d) at site %d", f,
                           (long long)k, c, S, s);
        }
      }
      const int q = coscan_quantize(pr.len_a + pr.len_b, grid, B);
      if (q >= 0) kept.push_back(CoscanSeqPair{pr.seq_a, pr.seq_b, q, (int)k});
    }
    // by bucket, ties by pair index (kept is in index order: a stable sort)
    std::stable_sort(kept.begin(), kept.end(), [](const CoscanSeqPair &a, const CoscanSeqPair &b) { return a.q < b.q; });
    F.n_kept = (int)kept.size();
    out.pairs.insert(out.pairs.end(), kept.begin(), kept.end());
    out.fam.push_back(F);
    const int nt = (L[f] + COSCAN_TILE - 1) / COSCAN_TILE;
    for (int ti = 0; ti < nt; ++ti)
      for (int tj = ti; tj < nt; ++tj) out.tiles.push_back(CoscanTileItem{f, ti, tj, 0});
    out.n_out += (size_t)L[f] * (size_t)L[f];
    p0 += n_pairs[f];
  }
  if (out.tiles.size() > (size_t)INT32_MAX) return cb_fail(CB_EINVAL, "cb_coscan_run: %zu tiles in one call", out.tiles.size());
  return CB_OK;
}
