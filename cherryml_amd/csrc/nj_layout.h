// Neighbour joining on the device: what the host and the kernels (nj.hip.h) share about a chunk of resident families.  HIP-free.
#pragma once
#include <cstddef>

// one family of a chunk: where its arrays start in the chunk's buffers
struct NjFamily {
  int n;            // leaves = slots = the row stride of D
  int join0;        // its first join record in the chunk's join_nodes / join_len
  size_t d0;        // its matrix in the chunk's D
  size_t v0;        // its slot vectors (r, tmp, rank, node) and its candidates
};

// a candidate of the argmin: the criterion, the ranks (lower, higher) and the slots (of the lower rank, of the higher rank)
struct NjCand {
  double crit;
  int ra, rb, sa, sb;
};
