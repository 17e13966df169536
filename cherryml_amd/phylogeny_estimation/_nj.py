"""Full trees from an alignment: all-pairs maximum-likelihood distances on the GPU, neighbour joining on the host or the GPU.

* distances: FastCherries' coordinate ascent (`cb_ble`) gives every site its rate category; then ONE launch of
  `ble_pairwise_kernel` (`cb_ble_pairwise`, csrc/ble.hip.h) runs the reference's branch-length bisection
  (branch_length_estimation.cpp:60-103) for all n (n - 1) / 2 pairs of sequences at those rates.  d_ij = grid[index_ij] times
  the mean site rate (FastCherries' normalisation, fast_cherries.cpp:262-304, without its text round trip).
* topology and lengths: canonical neighbour joining (Saitou & Nei 1987 with the Studier & Keppler 1988 criterion) in NumPy,
  O(n^3) simple flops next to the n^2 L 16 bank gathers of the distance pass; deterministic, testable without a GPU.
* the same join loop on the GPU (`cb_nj_batch`, csrc/nj.hip.h; `neighbor_joining_device`, `joiner="device"`): three launches per
  join for all families at once, the host's arithmetic operation for operation with one fixed order of the row sums.
  Both build their `Tree` from join records with one function.

Out of scope: ML refinement of the joined lengths, topology search (the stages behind this one)."""
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..caching import cached_computation
from ..io._tree import Tree, write_tree
from ._ble import compute_log_transition_matrices, estimate_branch_lengths_and_site_rates, pairwise_branch_lengths
from ._fast_cherries import (_encode_and_pair, _read_msa_file, get_weights_for_initial_site_rates, quantization_points_ble,
                             rate_categories_ble)


def neighbor_joining(D, names: Sequence[str], min_length: float = 0.0) -> Tree:
    """Canonical neighbour joining on the symmetric distance matrix `D` [n, n] of the leaves `names`.

    While m > 3 nodes are active: r_i = sum_k d_ik; the pair minimising (m - 2) d_ij - r_i - r_j is joined -- on ties the first
    pair in (i, j) lexicographic order of the current active list, to whose END the new node goes --, with
    l_i = d_ij / 2 + (r_i - r_j) / (2 (m - 2)), l_j = d_ij - l_i and d_uk = (d_ik + d_jk - d_ij) / 2.  The last three nodes
    hang off the root at (d_ab + d_ac - d_bc) / 2 and so on; two leaves hang off the root at d / 2 each.  The root is `root`,
    the joined nodes `internal-<k>` in join order (FastCherries' names).  Every length below `min_length` is raised to it (a
    non-additive matrix can give negative lengths).  On an additive matrix the tree's path lengths are the matrix."""
    D, names = _checked_input(D, names)
    D = np.array(D)
    np.fill_diagonal(D, 0.0)
    n = len(names)
    # The active nodes live in the slots 0 .. m-1 of D, in no particular order (the joined node takes slot i, the last slot's
    # node moves into slot j: two rows and columns rewritten per join, nothing compacted); rank[slot] is the node's place in
    # the active list -- leaves in the given order, joined nodes behind them in join order.  Leaves are the nodes 0 .. n-1,
    # the node join k makes is n + k.
    node = list(range(n))
    rank = np.arange(n)
    join_nodes: List[Tuple[int, int]] = []
    join_len: List[Tuple[float, float]] = []
    m = n
    work, diag = np.empty((2, n * n)), np.arange(n)
    while m > 3:
        V = D[:m, :m]
        r = V.sum(axis=1)
        crit, rr = work[0, :m * m].reshape(m, m), work[1, :m * m].reshape(m, m)   # (contiguous, and no allocation per join)
        np.multiply(V, float(m - 2), out=crit)
        crit -= np.add.outer(r, r, out=rr)                      # (symmetric bit for bit, as D is)
        crit[diag[:m], diag[:m]] = np.inf
        i, j = divmod(int(np.argmin(crit)), m)
        if np.count_nonzero(crit == crit[i, j]) > 2:            # more minima than this pair and its mirror image:
            a, b = np.nonzero(crit == crit[i, j])               # the first pair of the active list among them
            ra, rb = rank[a], rank[b]
            k = np.lexsort((np.maximum(ra, rb), np.minimum(ra, rb)))[0]
            i, j = int(a[k]), int(b[k])
        if rank[i] > rank[j]:
            i, j = j, i
        dij = V[i, j]
        li = dij / 2.0 + (r[i] - r[j]) / (2.0 * (m - 2))
        lj = dij - li
        join_nodes.append((node[i], node[j]))
        join_len.append((li, lj))
        du = (V[i] + V[j] - dij) / 2.0
        V[i, :] = du
        V[:, i] = du
        V[i, i] = 0.0
        node[i], rank[i] = n + len(join_nodes) - 1, n + len(join_nodes)
        if j != m - 1:
            V[j, :] = V[m - 1, :]
            V[:, j] = V[:, m - 1]
            V[j, j] = 0.0
            node[j], rank[j] = node[m - 1], rank[m - 1]
        m -= 1
    order = [int(k) for k in np.argsort(rank[:m])]
    return _tree_from_joins(names, join_nodes, join_len, [node[k] for k in order], D[np.ix_(order, order)], min_length)


def _checked_input(D, names: Sequence[str]):
    """`neighbor_joining`'s input checks, for the host and the device: (D as float64 -- the caller's own array where it is one
    already, so copy before writing --, the names).  The join loops run on a copy with a zero diagonal."""
    D = np.asarray(D, dtype=np.float64)
    names = [str(v) for v in names]
    n = len(names)
    if n < 2:
        raise ValueError(f"neighbor_joining needs at least two leaves, got {n}")
    if D.ndim != 2 or D.shape[0] != D.shape[1] or D.shape[0] != n:
        raise ValueError(f"D must be a square [{n}, {n}] matrix, got shape {D.shape}")
    if not np.array_equal(D, D.T):
        raise ValueError("D must be symmetric")
    if len(set(names)) != n:
        raise ValueError("leaf names must be distinct")
    reserved = {"root"} | {f"internal-{k}" for k in range(max(n - 3, 0))}
    if reserved & set(names):
        raise ValueError(f"leaf names must not be the tree's own node names: {sorted(reserved & set(names))}")
    return D, names


def _tree_from_joins(names: Sequence[str], join_nodes, join_len, final_nodes, final_D, min_length: float) -> Tree:
    """The tree of join records, for the host and the device: `join_nodes` [n - 3][2] (leaves 0 .. n-1, the node of join k is
    n + k) with the raw lengths `join_len`, and the last three (or two) active nodes `final_nodes` in active-list order with
    their distances `final_D`, on which the root step is taken here; nodes < 0 are unused slots.  Every length below
    `min_length` is raised to it."""
    n = len(names)

    def name(v):
        return names[v] if v < n else f"internal-{v - n}"

    joins: Dict[str, List[Tuple[str, float]]] = {}
    for k, ((a, b), (la, lb)) in enumerate(zip(join_nodes, join_len)):
        joins[f"internal-{k}"] = [(name(int(a)), la), (name(int(b)), lb)]
    active = [name(int(v)) for v in final_nodes if int(v) >= 0]
    D = np.asarray(final_D, dtype=np.float64)
    if len(active) == 3:
        joins["root"] = [(active[0], (D[0, 1] + D[0, 2] - D[1, 2]) / 2.0), (active[1], (D[0, 1] + D[1, 2] - D[0, 2]) / 2.0),
                         (active[2], (D[0, 2] + D[1, 2] - D[0, 1]) / 2.0)]
    else:
        joins["root"] = [(active[0], D[0, 1] / 2.0), (active[1], D[0, 1] / 2.0)]
    tree = Tree()
    tree.add_node("root")
    stack = ["root"]
    while stack:                                                # parents before children, children in join order
        u = stack.pop()
        for v, length in joins.get(u, []):
            tree.add_node(v)
            tree.add_edge(u, v, max(float(length), float(min_length)))
        stack.extend(v for v, _ in reversed(joins.get(u, [])))
    return tree


def nj_join_records(Ds: Sequence[np.ndarray], device: int = 0, profile: Optional[dict] = None, zero_diagonal: bool = False):
    """The join loop of `neighbor_joining` on the GPU (`cb_nj_batch`, csrc/nj.hip.h) for the symmetric float64 matrices `Ds`,
    all families in one call: per family (join_nodes [n - 3, 2] int32, join_len [n - 3, 2], final_nodes [3] int32,
    final_D [3, 3]) as include/cherrybank.h describes them.  The matrices are copied once, into the one buffer the library
    reads (`zero_diagonal`: with their diagonals set to 0 there, as `neighbor_joining` does on its copy).  The library validates
    them on the host before any device work; what it refuses raises `CherryBankError` with its message, which names family and
    value.  `profile` (a dict) receives `kernel_ms` (GPU time of the join launches, HIP events)."""
    import ctypes

    from .. import _lib
    Ds = [np.asarray(D, dtype=np.float64) for D in Ds]
    for D in Ds:
        if D.ndim != 2 or D.shape[0] != D.shape[1]:
            raise ValueError(f"every D must be a square matrix, got shape {D.shape}")
    n = np.array([D.shape[0] for D in Ds], dtype=np.int32)
    n_joins = np.maximum(n.astype(np.int64) - 3, 0)
    starts = np.concatenate([[0], np.cumsum(n.astype(np.int64) ** 2)])
    flat = np.empty(int(starts[-1]))
    for D, at in zip(Ds, starts):
        V = flat[at:at + D.size].reshape(D.shape)
        V[...] = D
        if zero_diagonal:
            np.fill_diagonal(V, 0.0)
    join_nodes = np.full((max(int(n_joins.sum()), 1), 2), -1, dtype=np.int32)
    join_len = np.zeros((max(int(n_joins.sum()), 1), 2))
    final_nodes = np.full((max(len(Ds), 1), 3), -1, dtype=np.int32)
    final_D = np.zeros((max(len(Ds), 1), 9))
    ms = ctypes.c_double(0.0)
    rc = _lib.load().cb_nj_batch(device, len(Ds), n.ctypes.data, flat.ctypes.data, join_nodes.ctypes.data, join_len.ctypes.data,
                                 final_nodes.ctypes.data, final_D.ctypes.data, ctypes.addressof(ms) if profile is not None else None)
    if rc == _lib.CB_EINVAL:   # a refused call: the library's message names the family and the value
        raise _lib.CherryBankError(f"cb_nj_batch failed ({rc}): {_lib.load().cb_last_error().decode('utf-8', 'replace')}")
    _lib.check(rc, "cb_nj_batch")
    if profile is not None:
        profile["kernel_ms"] = ms.value
    cuts = np.concatenate([[0], np.cumsum(n_joins)])
    return [(join_nodes[cuts[f]:cuts[f + 1]], join_len[cuts[f]:cuts[f + 1]], final_nodes[f], final_D[f].reshape(3, 3))
            for f in range(len(Ds))]


def neighbor_joining_device_batch(Ds: Sequence, names_list: Sequence[Sequence[str]], min_length: float = 0.0, device: int = 0,
                                  profile: Optional[dict] = None) -> List[Tree]:
    """`neighbor_joining` for many families with the join loop on the GPU, all families in ONE `cb_nj_batch` call: the same
    input checks and `ValueError`s, the same node names, child order and clamp; the root step on the last three or two nodes is
    taken here with the host's formulae.  Only the order of the row sums differs from the host: on matrices whose
    sums are exact the trees are equal bit for bit, otherwise a criterion closer to the next than that rounding may join
    another pair (at m = 4, where a pair ties with its complement in exact arithmetic, to the same unrooted tree)."""
    if len(Ds) != len(names_list):
        raise ValueError("one list of names per matrix")
    checked = [_checked_input(D, names) for D, names in zip(Ds, names_list)]
    if not checked:
        return []
    records = nj_join_records([D for D, _ in checked], device=device, profile=profile, zero_diagonal=True)
    return [_tree_from_joins(names, *rec, min_length) for (_, names), rec in zip(checked, records)]


def neighbor_joining_device(D, names: Sequence[str], min_length: float = 0.0, device: int = 0) -> Tree:
    """`neighbor_joining_device_batch` for one family."""
    return neighbor_joining_device_batch([D], [names], min_length=min_length, device=device)[0]


JOINERS = ("host", "device")


def _check_joiner(joiner: str) -> None:
    if joiner not in JOINERS:
        raise ValueError(f"joiner must be one of {JOINERS}, got {joiner!r}")


def nj_distance_indices(seqs: np.ndarray, pairs: Sequence[Tuple[int, int]], rate_matrix: np.ndarray, num_rate_categories: int = 20,
                        max_iters: int = 50, quantization_grid_center: float = 0.03, quantization_grid_step: float = 1.1,
                        quantization_grid_num_steps: int = 64, device: int = 0, profile: Optional[dict] = None,
                        log_transition_matrices: Optional[np.ndarray] = None):
    """The two device passes of `nj_tree_family` on encoded sequences `seqs` [n, L] and FastCherries' cherries `pairs`:
    returns (index [n, n] of `pairwise_branch_lengths`, cherry_index [len(pairs)], rate_index [L], grid, rates) -- the grid
    indices of all pairs, those of the cherries the coordinate ascent ended on, and every site's rate category.  The ascent's
    last step is the pairwise bisection at the returned rates, so index[a, b] == cherry_index[k] for every cherry k = (a, b).
    `log_transition_matrices`: the bank of this rate matrix, grid and categories if the caller has it already."""
    Q = np.ascontiguousarray(rate_matrix, dtype=np.float64)
    grid = np.array(quantization_points_ble(quantization_grid_center, quantization_grid_step, quantization_grid_num_steps))
    rates = np.array(rate_categories_ble(num_rate_categories))
    weights = get_weights_for_initial_site_rates(rates)
    logP = log_transition_matrices
    if logP is None:
        logP = compute_log_transition_matrices(Q, grid, rates, device=device)
    st = time.time()
    prof: dict = {}
    lengths, site_rates = estimate_branch_lengths_and_site_rates(
        seqs[[a for a, _ in pairs]], seqs[[b for _, b in pairs]], seqs, logP, grid, rates, weights, max_iters, device=device,
        profile=prof)
    t_ble = time.time() - st
    # the ascent returns exact elements of the grid and of the category list: their indices
    cherry_index = np.searchsorted(grid, lengths).astype(np.int32)
    rate_index = np.searchsorted(rates, site_rates).astype(np.int32)
    if not (np.array_equal(grid[cherry_index], lengths) and np.array_equal(rates[rate_index], site_rates)):
        raise RuntimeError("branch lengths / site rates are not elements of the grid / the rate categories")
    st = time.time()
    pw: dict = {}
    index = pairwise_branch_lengths(seqs, logP, rate_index, device=device, profile=pw)
    if profile is not None:
        profile["ble_time"], profile["distance_time"] = t_ble, time.time() - st
        profile["iterations"], profile["ble_kernel_ms"], profile["kernel_ms"] = prof["iterations"], prof["kernel_ms"], pw["kernel_ms"]
    return index, cherry_index, rate_index, grid, rates


def _family_distances(names: Sequence[str], sequences: Sequence[str], rate_matrix: np.ndarray, alphabet: Sequence[str],
                      num_rate_categories: int, max_iters: int, seed: int, quantization_grid_center: float,
                      quantization_grid_step: float, quantization_grid_num_steps: int, device: int, profile: Optional[dict],
                      log_transition_matrices: Optional[np.ndarray]):
    """`nj_tree_family` up to the distance matrix: (D [n, n], site_rates [L] normalised, the grid's first point)."""
    if len(names) != len(sequences):
        raise ValueError("one name per sequence")
    st = time.time()
    seqs, pairs = _encode_and_pair(sequences, alphabet, seed, "lemire")
    t_pair = time.time() - st
    index, _, rate_index, grid, rates = nj_distance_indices(
        seqs, pairs, rate_matrix, num_rate_categories=num_rate_categories, max_iters=max_iters,
        quantization_grid_center=quantization_grid_center, quantization_grid_step=quantization_grid_step,
        quantization_grid_num_steps=quantization_grid_num_steps, device=device, profile=profile,
        log_transition_matrices=log_transition_matrices)
    site_rates = rates[rate_index]
    mean_rate = 0.0
    for r in site_rates:                                        # FastCherries' left-to-right sum
        mean_rate += float(r)
    mean_rate /= len(site_rates)
    D = grid[np.maximum(index, 0)] * mean_rate
    np.fill_diagonal(D, 0.0)
    if profile is not None:
        profile["pairing_time"] = t_pair
    return D, site_rates / mean_rate, float(grid[0])


def nj_tree_family(names: Sequence[str], sequences: Sequence[str], rate_matrix: np.ndarray, alphabet: Sequence[str],
                   num_rate_categories: int = 20, max_iters: int = 50, seed: int = 1234,
                   quantization_grid_center: float = 0.03, quantization_grid_step: float = 1.1,
                   quantization_grid_num_steps: int = 64, device: int = 0, profile: Optional[dict] = None,
                   log_transition_matrices: Optional[np.ndarray] = None, joiner: str = "host") -> Tuple[Tree, np.ndarray]:
    """One MSA to a full tree: FastCherries' pairing and coordinate ascent for the site rates (`fast_cherries_family`'s grid,
    rate categories, weights and bank), the ML distance of every pair of sequences at those rates on the GPU
    (`pairwise_branch_lengths`), neighbour joining on the host (`joiner="host"`, `neighbor_joining`) or on the GPU
    (`joiner="device"`, `neighbor_joining_device`).  Returns (tree, site_rates [L]); distances are multiplied and
    site rates divided by the mean rate, as FastCherries normalises them.  No edge is shorter than the grid's first point: a
    zero-length edge between two different states has likelihood 0 for every consumer of the tree.
    `profile` (a dict) receives pairing_time, ble_time, distance_time, nj_time (seconds) and kernel_ms (the pairwise kernel)."""
    _check_joiner(joiner)
    D, site_rates, grid0 = _family_distances(names, sequences, rate_matrix, alphabet, num_rate_categories, max_iters, seed,
                                             quantization_grid_center, quantization_grid_step, quantization_grid_num_steps, device,
                                             profile, log_transition_matrices)
    st = time.time()
    if joiner == "host":
        tree = neighbor_joining(D, names, min_length=grid0)
    else:
        tree = neighbor_joining_device(D, names, min_length=grid0, device=device)
    if profile is not None:
        profile["nj_time"] = time.time() - st
    return tree, site_rates


@cached_computation(output_dirs=["output_tree_dir", "output_site_rates_dir", "output_likelihood_dir"],
                    exclude_args=["num_processes", "verbose", "remake"])
def nj_trees(msa_dir: str, families: List[str], rate_matrix_path: str, num_rate_categories: int, max_iters: int = 50,
             num_processes: int = 1, _version="1", output_tree_dir: Optional[str] = None,
             output_site_rates_dir: Optional[str] = None, output_likelihood_dir: Optional[str] = None, remake=False,
             quantization_grid_center=0.03, quantization_grid_step=1.1, quantization_grid_num_steps=64, verbose=True,
             seed=1234, joiner="host") -> None:
    """The tree-estimation stage with `fast_cherries`' interface and files, full trees instead of a star of cherries: per
    family `<tree_dir>/<family>.txt` (the neighbour-joining tree of `nj_tree_family`), `<site_rates_dir>/<family>.txt`,
    `<likelihood_dir>/<family>.txt` -- the log-likelihood of the family's alignment on that tree under the rate matrix at the
    written site rates, total and per site (`dp_likelihood_computation_batch`, root distribution = the matrix's stationary
    distribution; `fast_cherries` writes 0.0 there) -- and `<tree_dir>/<family>.profiling`.  `num_processes` / `remake` are
    accepted and ignored.  Wrapped in `functools.partial` it is a `tree_estimator` of the end-to-end pipelines.
    `joiner`: "host" joins every family with `neighbor_joining` as it goes; "device" computes the distances of all families
    first and joins them in ONE `neighbor_joining_device_batch` call (csrc/nj.hip.h), then writes the same files -- `nj_time` in
    `.profiling` is then the family's share of that call, as `likelihood_time` is of the likelihood batch."""
    from .. import _lib
    from ..evaluation._likelihood import _stationary_distribution, dp_likelihood_computation_batch, write_log_likelihood
    from ..io import read_rate_matrix
    _check_joiner(joiner)
    if joiner == "device" and _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError("nj_trees: no HIP device visible; joiner=\"device\" runs on the MI355X only (no CPU fallback)")
    if output_tree_dir is None or output_site_rates_dir is None or output_likelihood_dir is None:
        raise ValueError("output_tree_dir, output_site_rates_dir and output_likelihood_dir are required")
    for d in (output_tree_dir, output_site_rates_dir, output_likelihood_dir):
        os.makedirs(d, exist_ok=True)
    rm = read_rate_matrix(rate_matrix_path)
    alphabet = [str(c) for c in rm.columns]
    Q = np.ascontiguousarray(rm.to_numpy(), dtype=np.float64)
    import torch
    dev = torch.cuda.current_device()
    grid = quantization_points_ble(quantization_grid_center, quantization_grid_step, quantization_grid_num_steps)
    logP = compute_log_transition_matrices(Q, grid, rate_categories_ble(num_rate_categories), device=dev)   # one bank for all families
    msas, trees, rates, profs = [], [], [], []
    all_names, Ds = [], []
    grid_args = dict(num_rate_categories=num_rate_categories, max_iters=max_iters, seed=seed,
                     quantization_grid_center=quantization_grid_center, quantization_grid_step=quantization_grid_step,
                     quantization_grid_num_steps=quantization_grid_num_steps)
    for family in families:
        st = time.time()
        names, sequences = _read_msa_file(os.path.join(msa_dir, family + ".txt"))
        prof: Dict[str, float] = {}
        if joiner == "host":
            tree, site_rates = nj_tree_family(names, sequences, Q, alphabet, device=dev, profile=prof, log_transition_matrices=logP,
                                              **grid_args)
            write_tree(tree, os.path.join(output_tree_dir, family + ".txt"))
            trees.append(tree)
        else:                                                   # the distances now, the joins of all families below
            D, site_rates, _ = _family_distances(names, sequences, Q, alphabet, device=dev, profile=prof,
                                                 log_transition_matrices=logP, **grid_args)
            all_names.append(names)
            Ds.append(D)
        with open(os.path.join(output_site_rates_dir, family + ".txt"), "w") as f:
            f.write(f"{len(site_rates)} sites\n" + " ".join(repr(float(r)) for r in site_rates))
        prof["total_time"] = time.time() - st
        msas.append(dict(zip(names, sequences)))
        rates.append([float(r) for r in site_rates])
        profs.append(prof)
    if joiner == "device":
        st = time.time()
        trees = neighbor_joining_device_batch(Ds, all_names, min_length=float(grid[0]), device=dev)
        for family, tree in zip(families, trees):
            write_tree(tree, os.path.join(output_tree_dir, family + ".txt"))
        t_nj = (time.time() - st) / max(len(families), 1)       # (all families in ONE batch: shares)
        for prof in profs:
            prof["nj_time"] = t_nj
            prof["total_time"] += t_nj
    st = time.time()
    lls = dp_likelihood_computation_batch(trees, msas, [None] * len(families), rates, alphabet, _stationary_distribution(Q), Q,
                                          device=dev)
    t_ll = (time.time() - st) / max(len(families), 1)           # (all families in ONE batch: shares)
    for family, ll, prof in zip(families, lls, profs):
        write_log_likelihood(ll, os.path.join(output_likelihood_dir, family + ".txt"))
        with open(os.path.join(output_tree_dir, family + ".profiling"), "w") as f:
            f.write("".join(f"{k}: {prof.get(k, 0.0)}\n" for k in ("pairing_time", "ble_time", "distance_time", "nj_time"))
                    + f"likelihood_time: {t_ll}\ntotal_time: {prof['total_time'] + t_ll}")
