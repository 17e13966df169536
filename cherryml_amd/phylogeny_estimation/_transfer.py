"""Transfer bootstrap supports of neighbour-joining trees on the GPU (csrc/transfer.hip.h, `cb_transfer_support`; DESIGN.md
section 23): Lemoine et al., "Renewing Felsenstein's phylogenetic bootstrap in the era of big data", Nature 2018.

Felsenstein's support (`_bootstrap.py`) asks whether a replicate's tree has an edge's split exactly; on a tree of a thousand
leaves one wandering leaf loses a deep split, so deep edges get supports near zero whatever their quality.  The transfer
bootstrap compares the split with the CLOSEST split of the replicate's tree instead, counted in leaves that would have to move:
with A the leaves on one side of the edge, p = min(|A|, n - |A|) and S_q the leaf sets of the replicate's joined nodes,

    delta_b  = min(p - 1, min_q min(h, n - h)),  h = |A xor S_q|        (p - 1: the nearest leaf edge of the replicate's tree)
    transfer = 1 - sum_b delta_b / (B (p - 1)),   bootstrap = #{b: delta_b = 0} / B

so 0 <= bootstrap <= transfer <= 1, and `bootstrap` is `supports_of_records`' number.  Every reference split against every split
of every replicate is n x B x n Hamming distances of n-bit sets: xor and popcount on the device, where the replicates' leaf sets
are built from the join records and never leave.

* `transfer_distances`: the ctypes face -- per reference set the sum of delta over the replicates and the exact matches.
* `transfer_supports_of_records`: (nodes, bootstrap, transfer) of a tree from the replicates' join records.
* `transfer_bootstrap_supports`: the same from the alignment (`bootstrap_nj_records`, then the above).
* `nj_transfer_supports`: the stage on tree / MSA / site-rate directories, `nj_bootstrap_supports`' sibling.

Out of scope: the per-leaf transfer indices of `booster`, consensus trees."""
import ctypes
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .. import _lib
from ..caching import cached_computation
from ..io._tree import Tree
from ._bootstrap import _node_splits, _stage_families, bootstrap_nj_records

HEADER = "node bootstrap transfer\n"


def transfer_distances(ref_sets, n: int, join_nodes, device: int = 0, profile: Optional[dict] = None,
                       per_replicate: bool = False):
    """`cb_transfer_support` on the reference leaf sets `ref_sets` [n_ref, ceil(n / 8)] (uint8, `np.packbits` rows as
    `tree_splits` packs them, either side of every split, p >= 2) and the join records `join_nodes` [n_rep, n - 3, 2] of n_rep
    replicates on n leaves: (sum_dist int64 [n_ref], present int32 [n_ref]) -- the sum over the replicates of the transfer
    distance delta[r][b] and the number of replicates with delta = 0 -- and with `per_replicate` also min_dist int32
    [n_ref, n_rep] = delta.  What the library refuses raises ValueError with its message, no device CherryBankError.
    `profile` (a dict) receives sets_kernel_ms and distance_kernel_ms (HIP events)."""
    n = int(n)
    refs = np.ascontiguousarray(ref_sets, dtype=np.uint8)
    joins = np.ascontiguousarray(join_nodes, dtype=np.int32)
    if refs.ndim != 2 or refs.shape[1] != (max(n, 0) + 7) // 8:
        raise ValueError(f"ref_sets must be [n_ref, ceil(n / 8)] = [n_ref, {(max(n, 0) + 7) // 8}], got {refs.shape}")
    if joins.ndim != 3 or joins.shape[1:] != (max(n - 3, 0), 2):
        raise ValueError(f"join_nodes must be [n_rep, n - 3, 2] = [n_rep, {max(n - 3, 0)}, 2], got {joins.shape}")
    n_ref, n_rep = refs.shape[0], joins.shape[0]
    sum_dist = np.zeros(max(n_ref, 1), dtype=np.int64)
    present = np.zeros(max(n_ref, 1), dtype=np.int32)
    min_dist = np.zeros((max(n_ref, 1), max(n_rep, 1)), dtype=np.int32) if per_replicate else None
    ms = (ctypes.c_double * 2)()
    rc = _lib.load().cb_transfer_support(device, n, n_ref, refs.ctypes.data, n_rep, joins.ctypes.data,
                                         None if min_dist is None else min_dist.ctypes.data, sum_dist.ctypes.data,
                                         present.ctypes.data, ctypes.addressof(ms) if profile is not None else None)
    _lib.check(rc, "cb_transfer_support")
    if profile is not None:
        profile["sets_kernel_ms"], profile["distance_kernel_ms"] = ms[0], ms[1]
    return (sum_dist, present, min_dist) if per_replicate else (sum_dist, present)


def transfer_supports_of_records(tree: Tree, names: Sequence[str], records, device: int = 0,
                                 profile: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(nodes, bootstrap, transfer) for the edges above the internal non-root nodes of `tree` from the replicates' join records
    (join_nodes, join_len, final_nodes, final_D), leaf k of the records being names[k].  `nodes` and `bootstrap` are
    `supports_of_records`' (the share of the replicates whose tree has the split); `transfer` is the transfer bootstrap
    expectation 1 - sum_b delta_b / (B (p - 1)).  An edge that cuts off a single leaf gets 1.0 in both columns (host); the two
    edges at a bifurcating root are one split and get the same numbers; only the non-trivial splits, each once, go to the
    device (`transfer_distances`), and a tree of fewer than four leaves needs no device at all."""
    names = [str(v) for v in names]
    nodes, packed, real = _node_splits(tree, names)
    n, B = len(names), len(records)
    if B < 1:
        raise ValueError("at least one replicate")
    for _, _, final_nodes, _ in records:
        if np.count_nonzero(np.asarray(final_nodes) >= 0) != min(n, 3):
            raise ValueError("final_nodes must hold the last three (or two) active nodes")
    bootstrap, transfer = np.ones(len(nodes)), np.ones(len(nodes))
    if n < 4 or not real.any():
        return nodes, bootstrap, transfer
    rows, inverse = np.unique(packed[real], axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    joins = np.stack([np.asarray(r[0], dtype=np.int32).reshape(-1, 2) for r in records])
    sum_dist, present = transfer_distances(rows, n, joins, device=device, profile=profile)
    size = np.unpackbits(rows, axis=1).sum(axis=1, dtype=np.int64)
    p = np.minimum(size, n - size)
    bootstrap[real] = (present / B)[inverse]
    transfer[real] = (1.0 - sum_dist / (B * (p - 1)))[inverse]     # (integers below 2^53: one rounding, the division's)
    return nodes, bootstrap, transfer


def transfer_bootstrap_supports(tree: Tree, names: Sequence[str], seqs, logP, site_to_rate, grid, num_replicates: int, seed: int,
                                weights=None, device: int = 0,
                                profile: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`transfer_supports_of_records` of the `num_replicates` neighbour-joining trees of resampled sites that
    `bootstrap_supports` judges the tree by (`bootstrap_nj_records`, same arguments, same replicates at the same seed):
    (nodes, bootstrap, transfer).  `profile` receives the kernel times of both calls: weights_kernel_ms, distance_kernel_ms and
    join_kernel_ms of the replicates, transfer_sets_kernel_ms and transfer_distance_kernel_ms of the distances."""
    names = [str(v) for v in names]
    _node_splits(tree, names)                                   # (refuses names that are not the leaves, before the device)
    records = bootstrap_nj_records(seqs, logP, site_to_rate, grid, num_replicates, seed, weights=weights, device=device,
                                   profile=profile)
    prof: Optional[Dict[str, float]] = {} if profile is not None else None
    out = transfer_supports_of_records(tree, names, records, device=device, profile=prof)
    if profile is not None:
        profile["transfer_sets_kernel_ms"] = prof.get("sets_kernel_ms", 0.0)
        profile["transfer_distance_kernel_ms"] = prof.get("distance_kernel_ms", 0.0)
    return out


# ------------------------------------------------------------------------------------------------ files and the stage
def write_transfer_supports(path: str, names: Sequence[str], nodes, bootstrap, transfer) -> None:
    """the header `node bootstrap transfer`, then per internal non-root node `name share tbe`; `names` = `tree.nodes()`"""
    with open(path, "w") as fh:
        fh.write(HEADER + "".join(f"{names[int(v)]} {float(s)!r} {float(t)!r}\n" for v, s, t in zip(nodes, bootstrap, transfer)))


def read_transfer_supports(path: str) -> Dict[str, Tuple[float, float]]:
    """{node: (share, tbe)} of a file `write_transfer_supports` wrote"""
    lines = open(path).read().split("\n")
    if lines[0] + "\n" != HEADER:
        raise ValueError(f"{path}: not a transfer-support file (header {lines[0]!r})")
    return {x[0]: (float(x[1]), float(x[2])) for x in (ln.split() for ln in lines[1:] if ln)}


@cached_computation(output_dirs=["output_support_dir"])
def nj_transfer_supports(tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str,
                         num_replicates: int = 100, random_seed: int = 0, quantization_grid_center: float = 0.03,
                         quantization_grid_step: float = 1.1, quantization_grid_num_steps: int = 64,
                         output_support_dir: Optional[str] = None, _version="1") -> None:
    """Felsenstein's and the transfer bootstrap support of every internal edge of `<tree_dir>/<family>.txt` from
    `num_replicates` neighbour-joining trees of resampled sites, on the GPU (`transfer_bootstrap_supports`).  Arguments,
    distances, replicates and seeding are `nj_bootstrap_supports`': the resampling seed of a family is
    `support_seeds(families, random_seed)`'s, so the bootstrap column is that stage's number and a family's result depends on
    its name and the seed alone.  Per family:
    `<output_support_dir>/<family>.txt`: the header `node bootstrap transfer`, then one line `name share tbe` per internal
    non-root node in `tree.nodes()` order (the share of the replicates whose tree has the split of the edge above the node; one
    minus the mean normalised transfer distance of the split to the replicates' trees);
    `<output_support_dir>/<family>.profiling`."""
    if output_support_dir is None:
        raise ValueError("output_support_dir is required")
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError("nj_transfer_supports: no HIP device visible; the bootstrap runs on the MI355X only "
                                   "(no CPU fallback)")
    os.makedirs(output_support_dir, exist_ok=True)
    for family, seed, st, t_bank, dev, tree, names, seqs, logP, s2r, grid in _stage_families(
            tree_dir, msa_dir, site_rates_dir, families, rate_matrix_path, random_seed, quantization_grid_center,
            quantization_grid_step, quantization_grid_num_steps):
        prof: Dict[str, float] = {}
        nodes, bootstrap, transfer = transfer_bootstrap_supports(tree, names, seqs, logP, s2r, grid, int(num_replicates), seed,
                                                                 device=dev, profile=prof)
        write_transfer_supports(os.path.join(output_support_dir, family + ".txt"), tree.nodes(), nodes, bootstrap, transfer)
        with open(os.path.join(output_support_dir, family + ".profiling"), "w") as fh:
            fh.write(f"bank_time: {t_bank}\n" + "".join(f"{k}: {v}\n" for k, v in prof.items()) + f"total_time: {time.time() - st}")
