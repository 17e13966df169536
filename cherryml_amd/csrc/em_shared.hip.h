// What the EM E-step (em.hip.h, cb_em.hip) shares with the branch-length EM (bl.hip.h, cb_bl.hip): the outside pass's argument
// block and the launchers of the two passes' kernels (the kernels themselves are defined once, in cb_em.hip's translation unit).
#pragma once
#include "common.hip.h"
#include "tl_group.hip.h"

struct EmDownArgs {
  int S, n_units, root, n_blocks, n_cats;
  const int *level_nodes;            // internal non-root nodes of one depth
  const int *parent, *child_ptr, *child_idx;
  const int *qb, *unit_cat;
  const double *P;                   // [B][S][S]
  const double *pi_root;             // [S]
  const double *msg;                 // upward messages [node][unit][S]
  double *U;                         // outside messages [node][unit][S] (internal non-root nodes)
};

// em_up_kernel / em_down_kernel on stream 0 (cb_em.hip)
void em_launch_up(const TlArgs &a, const int *qb, int n_cats, unsigned grid);
void em_launch_down(const EmDownArgs &a, unsigned grid);
