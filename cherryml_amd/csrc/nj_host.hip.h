// Neighbour joining on the device, the host side that cb_nj_batch (cb_nj.hip) and cb_boot_nj (cb_boot.hip) share: the buffers of
// a resident chunk of families and the one function that joins it.  The kernels (nj.hip.h) are compiled in cb_nj.hip alone.
#pragma once
#include "cb_internal.hip.h"
#include "nj_layout.h"

constexpr int NJ_MAX_FAMILIES = 65535;           // of one chunk: the family is a grid dimension

// the device buffers of the largest chunk, reused by every chunk
struct NjBufs {
  CbDevBufs d;
  NjFamily *fams = nullptr;
  double *D = nullptr, *r = nullptr, *tmp = nullptr, *join_len = nullptr, *final_D = nullptr;
  int *rank = nullptr, *node = nullptr, *join_nodes = nullptr, *final_nodes = nullptr;
  NjCand *cand = nullptr;
  int alloc(size_t fam_cap, size_t mat_cap, size_t vec_cap, size_t join_cap) {
    int rc = CB_OK;
    fams = d.up<NjFamily>(nullptr, fam_cap, rc);
    D = d.up<double>(nullptr, mat_cap, rc);
    r = d.up<double>(nullptr, vec_cap, rc);
    tmp = d.up<double>(nullptr, vec_cap, rc);
    rank = d.up<int>(nullptr, vec_cap, rc);
    node = d.up<int>(nullptr, vec_cap, rc);
    cand = d.up<NjCand>(nullptr, vec_cap, rc);
    join_nodes = d.up<int>(nullptr, join_cap * 2, rc);
    join_len = d.up<double>(nullptr, join_cap * 2, rc);
    final_nodes = d.up<int>(nullptr, fam_cap * 3, rc);
    final_D = d.up<double>(nullptr, fam_cap * 9, rc);
    return rc;
  }
};

struct NjChunk {
  int f0, f1;                      // families [f0, f1)
  size_t mat, vec, joins;          // entries of its matrices, slots, join records
};

// The joins of one resident chunk of nf_c families, the largest of n_max > 3 leaves: b.fams, b.D, b.rank and b.node hold the
// chunk (the default stream is past their writes).  Enqueues three launches per join of the largest family without waiting in
// between, adds their GPU time to *ms_total when `timed`, and copies the chunk's `joins` join records and its families' last
// three nodes to the host arrays, which point at the chunk's first record and first family.  (cb_nj.hip)
int cb_nj_join_chunk(const NjBufs &b, int nf_c, int n_max, size_t joins, bool timed, double *ms_total, int *join_nodes,
                     double *join_len, int *final_nodes, double *final_D);
