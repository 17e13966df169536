"""Felsenstein's bootstrap of neighbour-joining trees on the GPU (csrc/boot.hip.h, `cb_boot_nj`).

A replicate draws L sites of the alignment with replacement; its tree is the neighbour-joining tree of the maximum-likelihood
distances of all pairs of sequences on the resampled alignment; the support of an edge is the share of the replicates whose tree
has the edge's split of the leaves.  It is the one support here that judges a split against all other trees and not only against
its two nearest-neighbour interchanges (`_supports.py`).

On the device nothing is resampled: for a pair of sequences the per-site log-likelihood terms at every grid point do not depend
on the replicate, only the site multiplicities do, so the likelihood curves of a pair for all replicates are one float64 matrix
product (replicates x sites times sites x grid points) on the matrix cores; the reference's bisection runs on the finished
curves, the distance matrices are written where `cb_nj_batch`'s join kernels read them, and only join records come back.

* `bootstrap_nj_records`: the ctypes face -- per replicate the join records of `nj_join_records`.
* `tree_splits`, `splits_of_join_records`: the non-trivial bipartitions of a tree / of join records as packed bitsets (host).
* `bootstrap_supports`: (nodes, support) for the edges above the internal non-root nodes of a given tree.
* `nj_bootstrap_supports`: the stage on tree / MSA / site-rate directories.

The transfer bootstrap of the same replicates, which judges a split by the closest split of a replicate's tree and not by an
exact match, is `_transfer.py` (`nj_transfer_supports`).

Out of scope: re-estimating the site rates per replicate (a site keeps its rate category when it is drawn), consensus trees,
re-optimising lengths or topology by maximum likelihood per replicate."""
import ctypes
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .. import _lib
from ..caching import cached_computation
from ..io._tree import Tree, read_tree
from ._ble import compute_log_transition_matrices
from ._fast_cherries import quantization_points_ble
from ._supports import support_seeds

HEADER = "node bootstrap\n"


def bootstrap_nj_records(seqs, logP, site_to_rate, grid, num_replicates: int, seed: int, weights=None, device: int = 0,
                         profile: Optional[dict] = None, return_index: bool = False, return_weights: bool = False):
    """`cb_boot_nj` on the encoded sequences `seqs` [n, L] (int8, -1 = gap), the bank `logP` [T, R, S, S] of the grid `grid` [T]
    and the sites' rate categories `site_to_rate` [L]: per replicate (join_nodes [n - 3, 2] int32, join_len [n - 3, 2],
    final_nodes [3] int32, final_D [3, 3]), as `nj_join_records` returns them for the replicate's distance matrix
    grid[index_b] (zero diagonal).  `weights` [num_replicates, L]: the site multiplicities (non-negative integer values); None:
    drawn on the device from `seed` (include/cherrybank.h has the rule).  With `return_index` the grid indices
    [num_replicates, n, n] (int32, -1 on the diagonal) follow the records, with `return_weights` the weights used
    [num_replicates, L].  What the library refuses raises ValueError with its message, no device CherryBankError.  `profile` (a
    dict) receives weights_kernel_ms, distance_kernel_ms and join_kernel_ms (HIP events)."""
    seqs = np.ascontiguousarray(seqs, dtype=np.int8)
    logP = np.ascontiguousarray(logP, dtype=np.float64)
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    if seqs.ndim != 2 or logP.ndim != 4 or logP.shape[2] != logP.shape[3]:
        raise ValueError("the sequences must be one [n, L] array and the bank [T, R, S, S]")
    T, R, S, _ = logP.shape
    n, L = seqs.shape
    s2r = np.ascontiguousarray(site_to_rate, dtype=np.int32)
    if s2r.shape != (L,):
        raise ValueError("site_to_rate must hold one rate index per site")
    if grid.shape != (T,):
        raise ValueError("grid must hold one branch length per grid point of the bank")
    B = int(num_replicates)
    W = None
    if weights is not None:
        W = np.ascontiguousarray(weights, dtype=np.float64)
        if W.shape != (B, L):
            raise ValueError(f"weights must be [num_replicates, L] = [{B}, {L}], got {W.shape}")
    nb, nj = max(B, 1), max(n - 3, 0)
    join_nodes = np.full((max(nb * nj, 1), 2), -1, dtype=np.int32)
    join_len = np.zeros((max(nb * nj, 1), 2))
    final_nodes = np.full((nb, 3), -1, dtype=np.int32)
    final_D = np.zeros((nb, 9))
    index = np.zeros((nb, n, n), dtype=np.int32) if return_index else None
    w_out = np.zeros((nb, L)) if return_weights else None
    ms = (ctypes.c_double * 3)()
    rc = _lib.load().cb_boot_nj(device, S, T, R, logP.ctypes.data, grid.ctypes.data, seqs.ctypes.data, n, L, s2r.ctypes.data, B,
                                int(seed) & 0xFFFFFFFFFFFFFFFF, None if W is None else W.ctypes.data, join_nodes.ctypes.data,
                                join_len.ctypes.data, final_nodes.ctypes.data, final_D.ctypes.data,
                                None if index is None else index.ctypes.data, None if w_out is None else w_out.ctypes.data,
                                ctypes.addressof(ms) if profile is not None else None)
    _lib.check(rc, "cb_boot_nj")
    if profile is not None:
        profile["weights_kernel_ms"], profile["distance_kernel_ms"], profile["join_kernel_ms"] = ms[0], ms[1], ms[2]
    records = [(join_nodes[b * nj:(b + 1) * nj], join_len[b * nj:(b + 1) * nj], final_nodes[b], final_D[b].reshape(3, 3))
               for b in range(B)]
    out = (records,) + ((index,) if return_index else ()) + ((w_out,) if return_weights else ())
    return out[0] if len(out) == 1 else out


# ------------------------------------------------------------------------------------------------ splits (host, NumPy)
def _canonical_packed(member: np.ndarray) -> np.ndarray:
    """bool [k, n] leaf sets -> uint8 [k, ceil(n / 8)]: the side without leaf 0, packed (the pad bits are 0)"""
    member = np.where(member[:, :1], ~member, member)
    return np.packbits(member, axis=1)


def _unique_rows(packed: np.ndarray) -> np.ndarray:
    return np.unique(packed, axis=0) if len(packed) else packed


def _node_splits(tree: Tree, names: Optional[Sequence[str]]):
    """per internal non-root node of `tree`, in `tree.nodes()` order: (its index in `tree.nodes()`, the canonical packed split
    of the edge above it, whether the split is non-trivial); leaf k of the bitsets is names[k] (default `tree.leaves()`)"""
    names = list(tree.leaves()) if names is None else [str(v) for v in names]
    if sorted(names) != sorted(tree.leaves()):
        raise ValueError("names must be the leaves of the tree")
    n = len(names)
    leaf_index = {v: k for k, v in enumerate(names)}
    nodes = tree.nodes()
    row = {v: k for k, v in enumerate(nodes)}
    below = np.zeros((len(nodes), n), dtype=bool)
    for v in tree.postorder_traversal():
        if tree.is_leaf(v):
            below[row[v], leaf_index[v]] = True
        else:
            for c, _ in tree.children(v):
                below[row[v]] |= below[row[c]]
    keep = [k for k, v in enumerate(nodes) if not tree.is_leaf(v) and not tree.is_root(v)]
    member = below[keep]
    size = member.sum(axis=1)
    return np.array(keep, dtype=np.int64), _canonical_packed(member), (size > 1) & (size < n - 1)


def tree_splits(tree: Tree, names: Optional[Sequence[str]] = None) -> np.ndarray:
    """The non-trivial bipartitions of the leaves by the edges of `tree` as canonical packed bitsets: uint8 [k, ceil(n / 8)],
    one row per split (`np.packbits` of the side WITHOUT leaf 0), rows unique and sorted.  Leaf k is names[k] (default
    `tree.leaves()`).  The two edges at a bifurcating root are one split."""
    _, packed, real = _node_splits(tree, names)
    return _unique_rows(packed[real])


SPLIT_BLOCK = 64   # replicates whose leaf sets are held at once (64 x 2 n x n / 8 bytes: 16 MB at a thousand leaves)


def _packed_join_sets(n: int, join_nodes: np.ndarray) -> np.ndarray:
    """join_nodes [b, k, 2] of b replicates on n leaves -> uint8 [b, k, ceil(n / 8)]: per replicate and join the canonical packed
    leaf set of the joined node -- the union of its two members', built in join order (one step for all b replicates)"""
    b, k = join_nodes.shape[:2]
    if k != max(n - 3, 0):
        raise ValueError(f"{n} leaves take {max(n - 3, 0)} joins, got {k}")
    nbytes = (n + 7) // 8
    sets = np.zeros((b, n + k, nbytes), dtype=np.uint8)
    sets[:, :n] = np.packbits(np.eye(n, dtype=bool), axis=1)[None]
    low = np.arange(n, n + k)[None, :, None]
    if k and not (np.all(join_nodes >= 0) and np.all(join_nodes < low)):
        raise ValueError("a join names a node that does not exist yet")
    rows = np.arange(b)
    for q in range(k):
        np.bitwise_or(sets[rows, join_nodes[:, q, 0]], sets[rows, join_nodes[:, q, 1]], out=sets[:, n + q])
    joined = sets[:, n:]
    full = np.packbits(np.ones(n, dtype=bool))                  # (the pad bits stay 0 under the complement)
    return np.where((joined[:, :, :1] & 0x80) != 0, joined ^ full, joined)


def splits_of_join_records(n: int, join_nodes, final_nodes) -> np.ndarray:
    """`tree_splits` of the tree of join records (`nj_join_records`, `bootstrap_nj_records`) on n leaves, without building the
    tree: the leaf set of the node join k makes (node n + k) is the union of its two members', built in join order, and the edge
    above every joined node is a non-trivial split.  uint8 [n - 3, ceil(n / 8)] (n <= 3: no rows)."""
    join_nodes = np.asarray(join_nodes, dtype=np.int64).reshape(-1, 2)
    if np.count_nonzero(np.asarray(final_nodes) >= 0) != min(n, 3):
        raise ValueError("final_nodes must hold the last three (or two) active nodes")
    return _unique_rows(_packed_join_sets(n, join_nodes[None])[0])


def _row_keys(packed: np.ndarray):
    """the rows of uint8 [k, w] as bytes objects"""
    packed = np.ascontiguousarray(packed)
    if packed.shape[0] == 0 or packed.shape[1] == 0:
        return [b""] * packed.shape[0]
    return packed.view(np.dtype((np.void, packed.shape[1]))).ravel().tolist()


def bootstrap_supports(tree: Tree, names: Sequence[str], seqs, logP, site_to_rate, grid, num_replicates: int, seed: int,
                       weights=None, device: int = 0, profile: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Felsenstein's bootstrap support of the edges of `tree` from `num_replicates` neighbour-joining trees of resampled
    sites (`bootstrap_nj_records`; `names` [n]: the leaf of every row of `seqs`).  Returns (nodes, support): the internal
    non-root nodes as indices into `tree.nodes()`, in that order, and per node the share of the replicates whose tree has the
    split of the edge above it -- k / num_replicates for an integer k.  The two edges at a bifurcating root are one split and
    get the same number; an edge that cuts off a single leaf is in every tree (1.0).  The replicates' splits are formed
    `SPLIT_BLOCK` replicates at a time, never all at once."""
    names = [str(v) for v in names]
    _node_splits(tree, names)                                   # (refuses names that are not the leaves, before the device)
    records = bootstrap_nj_records(seqs, logP, site_to_rate, grid, num_replicates, seed, weights=weights, device=device,
                                   profile=profile)
    return supports_of_records(tree, names, records)


def supports_of_records(tree: Tree, names: Sequence[str], records) -> Tuple[np.ndarray, np.ndarray]:
    """`bootstrap_supports`' (nodes, support) from the replicates' join records (join_nodes, join_len, final_nodes, final_D),
    leaf k of the records being names[k]: host only."""
    names = [str(v) for v in names]
    nodes, packed, real = _node_splits(tree, names)
    keys = _row_keys(packed)
    count: Dict[bytes, int] = {k: 0 for k in keys}
    n = len(names)
    for r0 in range(0, len(records), SPLIT_BLOCK):             # SPLIT_BLOCK replicates at a time
        block = records[r0:r0 + SPLIT_BLOCK]
        for _, _, final_nodes, _ in block:
            if np.count_nonzero(np.asarray(final_nodes) >= 0) != min(n, 3):
                raise ValueError("final_nodes must hold the last three (or two) active nodes")
        joins = np.stack([np.asarray(r[0], dtype=np.int64).reshape(-1, 2) for r in block])
        for rows in _packed_join_sets(n, joins):
            have = set(_row_keys(rows))
            for k in count:
                if k in have:
                    count[k] += 1
    B = len(records)
    if B < 1:
        raise ValueError("at least one replicate")
    support = np.array([count[k] / B if r else 1.0 for k, r in zip(keys, real)], dtype=np.float64)
    return nodes, support


# ------------------------------------------------------------------------------------------------ files and the stage
def write_bootstrap_supports(path: str, names: Sequence[str], nodes, support) -> None:
    """the header `node bootstrap`, then per internal non-root node `name share`; `names` = `tree.nodes()`"""
    with open(path, "w") as fh:
        fh.write(HEADER + "".join(f"{names[int(v)]} {float(s)!r}\n" for v, s in zip(nodes, support)))


def read_bootstrap_supports(path: str) -> Dict[str, float]:
    """{node: share} of a file `write_bootstrap_supports` wrote"""
    lines = open(path).read().split("\n")
    if lines[0] + "\n" != HEADER:
        raise ValueError(f"{path}: not a bootstrap-support file (header {lines[0]!r})")
    return {x[0]: float(x[1]) for x in (ln.split() for ln in lines[1:] if ln)}


def _stage_families(tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str, random_seed: int,
                    quantization_grid_center: float, quantization_grid_step: float, quantization_grid_num_steps: int):
    """what the bootstrap stages (`nj_bootstrap_supports`, `nj_transfer_supports`) read per family, in the families' order:
    (family, seed, start time, seconds for the bank, device, tree, leaf names, seqs [n, L], logP, site_to_rate, grid)"""
    from ..counting._host import read_msa, read_site_rates
    from ..counting._stage import _device_index
    from ..io import read_rate_matrix
    rm = read_rate_matrix(rate_matrix_path)
    alphabet = [str(c) for c in rm.columns]
    Q = np.ascontiguousarray(rm.to_numpy(), dtype=np.float64)
    grid = np.array(quantization_points_ble(quantization_grid_center, quantization_grid_step, quantization_grid_num_steps))
    lut = np.full(256, -1, dtype=np.int8)
    for i, aa in enumerate(alphabet):
        if len(aa) == 1 and ord(aa) < 256:
            lut[ord(aa)] = i
    dev = _device_index()
    for family, seed in zip(families, support_seeds(families, random_seed)):
        st = time.time()
        tree = read_tree(os.path.join(tree_dir, family + ".txt"))
        msa = read_msa(os.path.join(msa_dir, family + ".txt"))
        rates = np.asarray(read_site_rates(os.path.join(site_rates_dir, family + ".txt")), dtype=np.float64)
        names = tree.leaves()
        missing = [v for v in names if v not in msa]
        if missing:
            raise ValueError(f"{family}: the alignment has no sequence for the leaves {missing[:5]}")
        text = "".join(msa[v] for v in names).encode("latin-1")
        if len(text) != len(names) * len(rates):
            raise ValueError(f"{family}: every sequence of the alignment must have one character per site rate")
        seqs = lut[np.frombuffer(text, dtype=np.uint8)].reshape(len(names), len(rates))
        unique_rates, s2r = np.unique(rates, return_inverse=True)
        logP = compute_log_transition_matrices(Q, grid, unique_rates, device=dev)
        yield family, seed, st, time.time() - st, dev, tree, names, seqs, logP, s2r.astype(np.int32), grid


@cached_computation(output_dirs=["output_support_dir"])
def nj_bootstrap_supports(tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str,
                          num_replicates: int = 100, random_seed: int = 0, quantization_grid_center: float = 0.03,
                          quantization_grid_step: float = 1.1, quantization_grid_num_steps: int = 64,
                          output_support_dir: Optional[str] = None, _version="1") -> None:
    """Felsenstein's bootstrap support of every internal edge of `<tree_dir>/<family>.txt` from `num_replicates`
    neighbour-joining trees of resampled sites, on the GPU (`bootstrap_supports`).  The distances are the maximum-likelihood
    grid points (center, step, num_steps) under the rate matrix at the family's site rates `<site_rates_dir>/<family>.txt`:
    the rate categories are the unique values of that file, and D = grid[index] with no mean-rate factor, because the file's
    rates are already normalised.  The resampling seed of a family is `support_seeds(families, random_seed)`'s, so its result
    depends on its name and the seed alone.  Per family:
    `<output_support_dir>/<family>.txt`: the header `node bootstrap`, then one line `name share` per internal non-root node in
    `tree.nodes()` order (the share of the replicates whose tree has the split of the edge above the node);
    `<output_support_dir>/<family>.profiling`.
    Site rates are not re-estimated per replicate: a site keeps its rate when it is drawn."""
    if output_support_dir is None:
        raise ValueError("output_support_dir is required")
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError("nj_bootstrap_supports: no HIP device visible; the bootstrap runs on the MI355X only "
                                   "(no CPU fallback)")
    os.makedirs(output_support_dir, exist_ok=True)
    for family, seed, st, t_bank, dev, tree, names, seqs, logP, s2r, grid in _stage_families(
            tree_dir, msa_dir, site_rates_dir, families, rate_matrix_path, random_seed, quantization_grid_center,
            quantization_grid_step, quantization_grid_num_steps):
        prof: Dict[str, float] = {}
        nodes, support = bootstrap_supports(tree, names, seqs, logP, s2r, grid, int(num_replicates), seed,
                                            device=dev, profile=prof)
        write_bootstrap_supports(os.path.join(output_support_dir, family + ".txt"), tree.nodes(), nodes, support)
        with open(os.path.join(output_support_dir, family + ".profiling"), "w") as fh:
            fh.write(f"bank_time: {t_bank}\n" + "".join(f"{k}: {v}\n" for k, v in prof.items()) + f"total_time: {time.time() - st}")
