"""Maximum-likelihood branch lengths on fixed trees: EM over the internal states on the GPU (csrc/bl.hip.h, the resident `cb_bl_*`
handle).

The lengths are the parameters and live on the quantisation grid of `fast_cherries` / `nj_trees`; the topology, the rate matrix,
the root distribution and the site rates are fixed.  One round is the inside and outside passes at the current lengths and, for
every edge independently, the grid point that maximises the expected complete-data log-likelihood -- an exact EM step, so no
round lowers a family's likelihood.  `BranchLengthFitter` is the handle, `ml_branch_lengths` the stage on tree / MSA / site-rate
directories, `nj_ml_trees` the tree estimator `nj_trees` + `ml_branch_lengths`.

The handle also scores the nearest-neighbour interchanges of its trees from the messages its passes leave resident (`nni_moves`,
`nni_scan`; the search on top of them is `_nni.py`) and reconstructs the marginal posterior of the state at
every node from the same messages (`ancestral_states`; the stage is `_ancestral.py`), and resamples the
scan's per-site log-likelihoods into local branch supports (`branch_supports`; the stage is `_supports.py`)
and into the best candidate of every bootstrap replicate (`bootstrap_best`; `_ufboot.py`).

Out of scope: changing a handle's topology in place, a continuous (off-grid) optimiser, S > 32."""
import ctypes
import os
import time
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .. import _lib
from ..caching import cached_computation
from ..io._tree import Tree, read_tree, write_tree
from ._fast_cherries import quantization_points_ble

DEFAULT_MAX_BANK_BYTES = 4 << 30   # banks (P and log P) of the families of one handle, at most


class BranchLengthFitter(_lib.ResidentHandle):
    """Branch-length EM resident on one GPU: trees, leaf codes, site-rate categories and each family's bank of
    expm(grid[tau] rate_c Q) and its logarithm are built once (`cb_bl_create`); `round()` is one EM step for all families.

    trees: `io.Tree`s (their lengths are snapped to the grid: the start); leaf_codes: per family an int8 array
    [n_nodes, n_sites] with rows in `tree.nodes()` order (-1 = gap; only leaf rows are read); site_rates: per family [n_sites],
    finite and > 0; grid: the T >= 2 grid points (increasing); Q [S, S], pi_root [S], 2 <= S <= 32.  A context manager;
    `close()` frees the handle."""
    _destroy = "cb_bl_destroy"

    def __init__(self, trees: Sequence, leaf_codes: Sequence[np.ndarray], site_rates: Sequence, grid: Sequence[float], Q, pi_root,
                 device: Optional[int] = None):
        from ..counting._stage import _device_index
        from ..evaluation._likelihood import _pack_forest
        self.grid = np.ascontiguousarray(np.asarray(grid, dtype=np.float64).reshape(-1))
        self.Q = np.ascontiguousarray(Q, dtype=np.float64)
        self.pi_root = np.ascontiguousarray(pi_root, dtype=np.float64).reshape(-1)
        S = self.Q.shape[0]
        if self.Q.shape != (S, S) or self.pi_root.shape != (S,):
            raise ValueError(f"BranchLengthFitter: Q must be square and pi_root of its size: {self.Q.shape}, {self.pi_root.shape}")
        if len(trees) == 0 or len(trees) != len(leaf_codes) or len(trees) != len(site_rates):
            raise ValueError("BranchLengthFitter: need one tree, one code array and one site-rate vector per family "
                             "(at least one family)")
        self.n_nodes, self.n_units, *self._args = _pack_forest("BranchLengthFitter", trees, leaf_codes, site_rates)
        self._nodes: List[List[str]] = [list(tree.nodes()) for tree in trees]
        self.S = S
        self.device = _device_index() if device is None else int(device)
        self.last_kernel_ms = (0.0, 0.0)   # (passes, M-step) of the last round
        self._parent = np.split(self._args[0], np.cumsum(self.n_nodes)[:-1])
        self.last_nni_kernel_ms = (0.0, 0.0)   # (passes, scan) of the last nni_scan
        self.last_spr_kernel_ms = (0.0, 0.0)   # (passes, scan) of the last spr_scan
        self.last_ancestral_kernel_ms = (0.0, 0.0)   # (passes, reconstruction) of the last ancestral_states
        self.last_support_kernel_ms = (0.0, 0.0, 0.0)   # (passes, scan, resampling) of the last branch_supports
        self.last_ufboot_kernel_ms = (0.0, 0.0, 0.0)   # (passes, scan, resampling and reduction) of the last bootstrap_best
        self._create()

    def _create(self) -> None:
        par, ln, rt, cd = self._args
        h = ctypes.c_void_p()
        rc = _lib.load().cb_bl_create(self.device, self.S, self.grid.size, self.grid.ctypes.data, self.Q.ctypes.data,
                                      self.pi_root.ctypes.data, self.n_nodes.size, self.n_nodes.ctypes.data, par.ctypes.data,
                                      ln.ctypes.data, self.n_units.ctypes.data, rt.ctypes.data, cd.ctypes.data, ctypes.byref(h))
        _lib.check(rc, "cb_bl_create")
        self._h = h

    def round(self) -> Tuple[np.ndarray, np.ndarray]:
        """One EM step -> (n_changed [n_fam], fam_ll [n_fam]): the indices the round changed and every family's log-likelihood
        at the lengths the round STARTED from.  A family whose round changes nothing is at a fixed point and is skipped from
        then on (0 and the same log-likelihood)."""
        n_changed = np.zeros(self.n_nodes.size, dtype=np.int32)
        fam_ll = np.empty(self.n_nodes.size)
        ms = (ctypes.c_double * 2)(0.0, 0.0)
        _lib.check(_lib.load().cb_bl_round(self._handle(), n_changed.ctypes.data, fam_ll.ctypes.data, ctypes.addressof(ms)), "cb_bl_round")
        self.last_kernel_ms = (ms[0], ms[1])
        return n_changed, fam_ll

    def _get(self, with_ll: bool):
        index = np.empty(int(self.n_nodes.sum()), dtype=np.int32)
        ll = np.empty(int(self.n_units.sum())) if with_ll else None
        fam = np.empty(self.n_nodes.size) if with_ll else None
        rc = _lib.load().cb_bl_get(self._handle(), index.ctypes.data, ll.ctypes.data if with_ll else None,
                                   fam.ctypes.data if with_ll else None)
        _lib.check(rc, "cb_bl_get")
        return index, ll, fam

    def indices(self) -> List[np.ndarray]:
        """per family the grid index of the edge above every node, rows in `tree.nodes()` order (the root: -1)"""
        return np.split(self._get(False)[0], np.cumsum(self.n_nodes)[:-1])

    def lengths(self) -> List[Dict[str, float]]:
        """per family {node: grid[tau]} for every node but the root"""
        return [{v: float(self.grid[t]) for v, t in zip(nodes, idx) if t >= 0} for nodes, idx in zip(self._nodes, self.indices())]

    def log_likelihoods(self) -> Tuple[List[np.ndarray], np.ndarray]:
        """(per family the log-likelihood of every site, their sums per family) at the current lengths"""
        _, ll, fam = self._get(True)
        return np.split(ll, np.cumsum(self.n_units)[:-1]), fam

    def _call(self, name: str, *args) -> None:
        """the library call `name` on the handle; a refused argument (CB_EINVAL) is a `CherryBankError` with the library's
        message, which names family, move and value"""
        rc = getattr(_lib.load(), name)(self._handle(), *args)
        if rc == _lib.CB_EINVAL:
            raise _lib.CherryBankError(f"{name} failed ({rc}): {_lib.load().cb_last_error().decode('utf-8', 'replace')}")
        _lib.check(rc, name)

    def _move_lists(self, who: str, moves: Optional[Sequence], width: int, default):
        """one list per family as int32 [n, width] (`default()` when None) -> (moves, n_moves [n_fam], all of them flat)"""
        moves = default() if moves is None else [np.ascontiguousarray(m, dtype=np.int32).reshape(-1, width) for m in moves]
        if len(moves) != self.n_nodes.size:
            raise ValueError(f"{who}: {len(moves)} move lists for {self.n_nodes.size} families")
        n_moves = np.array([len(m) for m in moves], dtype=np.int32)
        return moves, n_moves, np.ascontiguousarray(np.concatenate(moves).reshape(-1), dtype=np.int32)

    def _seed_array(self, who: str, seeds: Optional[Sequence[int]]) -> np.ndarray:
        """one 64-bit seed per family (default 0) as uint64"""
        seeds = [0] * self.n_nodes.size if seeds is None else [int(s) for s in seeds]
        if len(seeds) != self.n_nodes.size:
            raise ValueError(f"{who}: {len(seeds)} seeds for {self.n_nodes.size} families")
        return np.array([s & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64)

    def _scan(self, who: str, moves: Optional[Sequence], width: int, default, per_site: bool):
        """`nni_scan` and `spr_scan`: the library's `cb_bl_<who>` on lists of `width` ints per move -> (its kernel_ms, the
        method's result)"""
        moves, n_moves, flat = self._move_lists(who, moves, width, default)
        delta = np.empty(int(n_moves.sum()))
        sizes = n_moves.astype(np.int64) * self.n_units
        ll = np.empty(int(sizes.sum())) if per_site else None
        ms = (ctypes.c_double * 2)(0.0, 0.0)
        self._call("cb_bl_" + who, n_moves.ctypes.data, flat.ctypes.data, delta.ctypes.data,
                   ll.ctypes.data if per_site else None, None, ctypes.addressof(ms))
        deltas = np.split(delta, np.cumsum(n_moves)[:-1])
        if not per_site:
            return (ms[0], ms[1]), (moves, deltas)
        lls = [x.reshape(int(k), int(u)) for x, k, u in zip(np.split(ll, np.cumsum(sizes)[:-1]), n_moves, self.n_units)]
        return (ms[0], ms[1]), (moves, deltas, lls)

    def nni_moves(self) -> List[np.ndarray]:
        """per family the int32 [n, 3] array of ALL nearest-neighbour interchanges (v, c, s) of its tree, node indices in
        `tree.nodes()` order: v (internal, not the root) ascending, then c over the children of v, then s over the other children
        of parent[v], children in node order (`_nni.enumerate_nni_moves`)"""
        from ._nni import enumerate_nni_moves
        return [enumerate_nni_moves(p) for p in self._parent]

    def nni_scan(self, moves: Optional[Sequence] = None, per_site: bool = False):
        """Score moves by likelihood at the current indices (`cb_bl_nni_scan`: one launch per family from the resident messages)
        -> (moves, delta) and with `per_site` also ll_moves: per family the [n, 3] moves (`nni_moves()` when None; a family with
        none is skipped), delta [n] = the log-likelihood of the rearranged tree minus the present one, and ll_moves [n, n_sites]
        the rearranged tree's log-likelihood per site.  Changes nothing `round()`, `indices()` or `log_likelihoods()` return.
        Sets `last_nni_kernel_ms` = (passes, scan)."""
        self.last_nni_kernel_ms, out = self._scan("nni_scan", moves, 3, self.nni_moves, per_site)
        return out

    def spr_moves(self, radius: int = 3) -> List[np.ndarray]:
        """per family the int32 [n, 5] array of ALL subtree prune-and-regraft moves (x, y, tau_s, tau_p, tau_y) of its tree within
        `radius`, at the handle's current indices: (x, y) from `_spr.enumerate_spr_moves` (x ascending, then y), the three
        indices from `_spr.spr_indices`"""
        from ._spr import _moves_at
        return [_moves_at(p, tau, self.grid, radius) for p, tau in zip(self._parent, self.indices())]

    def spr_scan(self, moves: Optional[Sequence] = None, radius: int = 3, per_site: bool = False):
        """Score subtree prune-and-regraft moves by likelihood at the current indices (`cb_bl_spr_scan`: one launch per family
        from the resident messages) -> (moves, delta) and with `per_site` also ll_moves: per family the [n, 5] moves
        (`spr_moves(radius)` when None; a family with none is skipped), delta [n] = the log-likelihood of the rearranged tree
        at the move's three indices minus the present one, and ll_moves [n, n_sites] the rearranged tree's log-likelihood per
        site.  Changes nothing any other method returns.  Sets `last_spr_kernel_ms` = (passes, scan)."""
        self.last_spr_kernel_ms, out = self._scan("spr_scan", moves, 5, lambda: self.spr_moves(radius), per_site)
        return out

    def branch_supports(self, num_replicates: int = 1000, seeds: Optional[Sequence[int]] = None, per_replicate: bool = False,
                        moves: Optional[Sequence] = None):
        """Local supports of the edge above every internal non-root node at the current indices (`cb_bl_supports`: the NNI scan,
        then a resampling of its per-site log-likelihoods on the GPU) -> per family
        (nodes, alrt, sh, rell) and with `per_replicate` also delta_rep: nodes int32 [g] the v of each group of `nni_moves()` in
        its order, alrt float64 [g] = -2 max of the group's `nni_scan` deltas (negative where a neighbour beats the tree), sh and
        rell float64 [g] the SH-like and RELL supports, counts over `num_replicates` (1 .. 65536) site resamples divided by it,
        and delta_rep float64 [n_moves, num_replicates] the resampled deltas.  `seeds`: one 64-bit seed per family (default 0);
        replicate r of a family depends on its seed and r alone.  A family with no move gets empty arrays; an edge none of whose
        neighbours has a finite likelihood gets NaN three times.  `moves`: per family its own [n, 3] list in place of
        `nni_moves()`, equal v consecutive (a subset of the edges, or of an edge's neighbours).  Changes nothing
        `round()`, `indices()`, `log_likelihoods()`, `nni_scan()` or `ancestral_states()` return.  Sets
        `last_support_kernel_ms` = (passes, scan, resampling)."""
        num_replicates = int(num_replicates)
        seed_arr = self._seed_array("branch_supports", seeds)
        moves, n_moves, flat = self._move_lists("branch_supports", moves, 3, self.nni_moves)
        # the groups: runs of equal v (the library refuses a v that comes back)
        nodes = [m[np.r_[True, m[1:, 0] != m[:-1, 0]], 0].astype(np.int32) if len(m) else np.zeros(0, dtype=np.int32) for m in moves]
        n_groups = np.array([len(v) for v in nodes], dtype=np.int64)
        total = int(n_groups.sum())
        alrt = np.empty(total)
        sh, rell = np.empty(total, dtype=np.int32), np.empty(total, dtype=np.int32)
        rep = np.empty(int(n_moves.sum()) * max(num_replicates, 0)) if per_replicate else None
        ms = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
        self._call("cb_bl_supports", num_replicates, seed_arr.ctypes.data, n_moves.ctypes.data, flat.ctypes.data, alrt.ctypes.data,
                   sh.ctypes.data, rell.ctypes.data, rep.ctypes.data if per_replicate else None, None, ctypes.addressof(ms))
        self.last_support_kernel_ms = (ms[0], ms[1], ms[2])
        cuts = np.cumsum(n_groups)[:-1]
        share = [[np.where(x >= 0, x / num_replicates, np.nan) for x in np.split(c, cuts)] for c in (sh, rell)]
        out = [nodes, np.split(alrt, cuts), share[0], share[1]]
        if per_replicate:
            out.append([x.reshape(int(k), num_replicates)
                        for x, k in zip(np.split(rep, np.cumsum(n_moves.astype(np.int64))[:-1] * num_replicates), n_moves)])
        return [tuple(x[k] for x in out) for k in range(len(moves))]

    def bootstrap_best(self, num_replicates: int = 1000, seeds: Optional[Sequence[int]] = None, best: Optional[Sequence] = None,
                       moves: Optional[Sequence] = None, base: bool = False):
        """Per bootstrap replicate the best resampled log-likelihood among a running best, this handle's tree and its
        nearest-neighbour interchanges at the current indices, and which of them attains it (`cb_bl_bootstrap_best`; DESIGN.md
        section 24) -> per family (score [R], code [R]) and with `base` also the tree's own resampled log-likelihood B [R].
        Replicate r of a family is replicate r of `branch_supports` with the same seed.  The candidates of a replicate, in
        order: the incoming `best[k][r]` (code -2; `best=None` means -inf, a first call), the tree (code -1, score B^r), move m
        of the family's list (code m, score B^r + delta_rep[m][r] of `branch_supports`; a move whose delta is not finite is left
        out); the result is the largest score and the FIRST candidate that attains it.  `moves`: per family its own [n, 3] list
        in place of `nni_moves()`, in any order.  Feeding a call's scores to the next handle's call as `best` carries the
        running best through a search (`_ufboot.py`).  Changes nothing `round()`, `indices()`, `log_likelihoods()`,
        `nni_scan()`, `branch_supports()` or `ancestral_states()` return.  Sets `last_ufboot_kernel_ms` = (passes, scan,
        resampling and reduction)."""
        n_fam = self.n_nodes.size
        num_replicates = int(num_replicates)
        R = max(num_replicates, 0)
        seed_arr = self._seed_array("bootstrap_best", seeds)
        moves, n_moves, flat = self._move_lists("bootstrap_best", moves, 3, self.nni_moves)
        if best is None:
            score = np.full((n_fam, R), -np.inf)
        else:
            if len(best) != n_fam:
                raise ValueError(f"bootstrap_best: {len(best)} incoming arrays for {n_fam} families")
            score = np.ascontiguousarray(np.stack([np.asarray(b, dtype=np.float64).reshape(-1) for b in best]) if R else
                                         np.zeros((n_fam, 0)))
            if score.shape != (n_fam, R):
                raise ValueError(f"bootstrap_best: the incoming best has shape {score.shape}, not {(n_fam, R)}")
        code = np.empty((n_fam, R), dtype=np.int32)
        own = np.empty((n_fam, R)) if base else None
        ms = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
        self._call("cb_bl_bootstrap_best", num_replicates, seed_arr.ctypes.data, n_moves.ctypes.data, flat.ctypes.data,
                   score.ctypes.data, code.ctypes.data, own.ctypes.data if base else None, None, ctypes.addressof(ms))
        self.last_ufboot_kernel_ms = (ms[0], ms[1], ms[2])
        return [(score[k], code[k], own[k]) if base else (score[k], code[k]) for k in range(n_fam)]

    def ancestral_states(self, posteriors: bool = False):
        """The marginal posterior of the state at EVERY node (root, internal nodes, leaves) at the current indices
        (`cb_bl_ancestral`: one launch per family from the resident messages) -> (states, confidence) and with `posteriors` also
        the whole distributions: per family int8 [n_nodes, n_sites] the most probable state (the lowest index among exactly equal
        maxima), float64 [n_nodes, n_sites] its posterior and float64 [n_nodes, n_sites, S]; rows in `tree.nodes()` order.  An
        observed leaf character gets its own state with posterior 1, a gapped one is imputed; a site that is impossible under the
        model gets state -1, confidence 0 and a zero posterior.  Changes nothing `round()`, `indices()`, `log_likelihoods()` or
        `nni_scan()` return.  Sets `last_ancestral_kernel_ms` = (passes, reconstruction)."""
        sizes = self.n_nodes.astype(np.int64) * self.n_units
        total = int(sizes.sum())
        state = np.empty(total, dtype=np.int8)
        conf = np.empty(total)
        post = np.empty(total * self.S) if posteriors else None
        ms = (ctypes.c_double * 2)(0.0, 0.0)
        rc = _lib.load().cb_bl_ancestral(self._handle(), state.ctypes.data, conf.ctypes.data, post.ctypes.data if posteriors else None,
                                         None, ctypes.addressof(ms))
        _lib.check(rc, "cb_bl_ancestral")
        self.last_ancestral_kernel_ms = (ms[0], ms[1])
        cuts = np.cumsum(sizes)[:-1]
        shapes = list(zip(self.n_nodes.tolist(), self.n_units.tolist()))
        states = [x.reshape(sh) for x, sh in zip(np.split(state, cuts), shapes)]
        confs = [x.reshape(sh) for x, sh in zip(np.split(conf, cuts), shapes)]
        if not posteriors:
            return states, confs
        return states, confs, [x.reshape(sh + (self.S,)) for x, sh in zip(np.split(post, cuts * self.S), shapes)]


def _batches(bank_bytes: Sequence[int], bound: int) -> List[List[int]]:
    """the families in order, cut where the next family's banks would pass `bound` (a family larger than it goes alone)"""
    out: List[List[int]] = []
    fill = 0
    for f, b in enumerate(bank_bytes):
        if not out or fill + b > bound:
            out.append([])
            fill = 0
        out[-1].append(f)
        fill += b
    return out


class _StageInputs(NamedTuple):
    """what `ml_branch_lengths` and the searches (`_search.py`) read before their first handle"""
    families: List[str]
    output_tree_dir: str
    output_likelihood_dir: str
    start: float           # time.time() at the stage's start
    alphabet: List[str]
    Q: np.ndarray
    pi_root: np.ndarray
    grid: np.ndarray
    device: int
    trees: List[Tree]
    msas: list
    rates: List[np.ndarray]
    codes: List[np.ndarray]     # rows in tree.nodes() order, which no move changes
    bank_bytes: List[int]

    def fitter(self, fams: Sequence[int], trees: Sequence[Tree]) -> BranchLengthFitter:
        """a handle on `trees`, the trees of the families `fams`"""
        return BranchLengthFitter(trees, [self.codes[f] for f in fams], [self.rates[f] for f in fams], self.grid, self.Q,
                                  self.pi_root, device=self.device)


def _read_stage_inputs(stage: str, runs: str, tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str],
                       rate_matrix_path: str, grid_args: Sequence, output_tree_dir: Optional[str],
                       output_likelihood_dir: Optional[str]) -> _StageInputs:
    """the checks of a stage on tree / MSA / site-rate directories (`runs`: what it does, for the no-device message), its output
    directories, the model, the grid `quantization_points_ble(*grid_args)` and the families' trees, MSAs, site rates and codes"""
    from ..counting._host import read_msa, read_site_rates
    from ..counting._stage import _device_index
    from ..evaluation._likelihood import _family_units, _stationary_distribution
    from ..io import read_rate_matrix
    if output_tree_dir is None or output_likelihood_dir is None:
        raise ValueError("output_tree_dir and output_likelihood_dir are required")
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError(f"{stage}: no HIP device visible; the {runs} runs on the MI355X only (no CPU fallback)")
    st_all = time.time()
    for d in (output_tree_dir, output_likelihood_dir):
        os.makedirs(d, exist_ok=True)
    rm = read_rate_matrix(rate_matrix_path)
    alphabet = [str(c) for c in rm.columns]
    Q = np.ascontiguousarray(rm.to_numpy(), dtype=np.float64)
    pi_root = _stationary_distribution(Q)
    grid = np.array(quantization_points_ble(*grid_args))
    device = _device_index()
    trees, msas, rates, codes = [], [], [], []
    for family in families:
        tree = read_tree(os.path.join(tree_dir, family + ".txt"))
        msa = read_msa(os.path.join(msa_dir, family + ".txt"))
        r = np.asarray(read_site_rates(os.path.join(site_rates_dir, family + ".txt")), dtype=np.float64)
        trees.append(tree), msas.append(msa), rates.append(r)
        codes.append(_family_units(tree, msa, None, len(r), alphabet, False)[2])
    bank_bytes = [2 * grid.size * np.unique(r).size * Q.size * 8 for r in rates]
    return _StageInputs(families, output_tree_dir, output_likelihood_dir, st_all, alphabet, Q, pi_root, grid, device, trees, msas,
                        rates, codes, bank_bytes)


def _tree_at(tree: Tree, lengths: Dict[str, float]) -> Tree:
    """`tree` with the lengths of a fitter's `lengths()`: the same nodes and edges in the same order"""
    t = Tree()
    t.add_nodes(tree.nodes())
    t.add_edges([(u, v, lengths[v]) for u, v, _ in tree.edges()])
    return t


def _write_stage_outputs(inp: _StageInputs, trees: Sequence[Tree], logs: Sequence[List[str]], log_ext: str,
                         profs: Sequence[Dict[str, float]]) -> None:
    """the likelihoods of the final trees and, per family, the tree, its log `<family><log_ext>`, its likelihoods and
    `<family>.profiling` (`profs` and the shares of the likelihood and the total time)"""
    from ..evaluation._likelihood import dp_likelihood_computation_batch, write_log_likelihood
    F = len(inp.families)
    st = time.time()
    lls = dp_likelihood_computation_batch(trees, inp.msas, [None] * F, [[float(x) for x in r] for r in inp.rates], inp.alphabet,
                                          inp.pi_root, inp.Q, device=inp.device)
    t_ll = (time.time() - st) / max(F, 1)
    t_total = (time.time() - inp.start) / max(F, 1)
    for f, family in enumerate(inp.families):
        write_tree(trees[f], os.path.join(inp.output_tree_dir, family + ".txt"))
        with open(os.path.join(inp.output_tree_dir, family + log_ext), "w") as fh:
            fh.write("".join(logs[f]))
        write_log_likelihood(lls[f], os.path.join(inp.output_likelihood_dir, family + ".txt"))
        with open(os.path.join(inp.output_tree_dir, family + ".profiling"), "w") as fh:
            fh.write("".join(f"{k}: {v}\n" for k, v in profs[f].items()) + f"likelihood_time: {t_ll}\ntotal_time: {t_total}")


@cached_computation(output_dirs=["output_tree_dir", "output_likelihood_dir"], exclude_args=["max_bank_bytes"])
def ml_branch_lengths(tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str,
                      num_rounds: int = 10, quantization_grid_center: float = 0.03, quantization_grid_step: float = 1.1,
                      quantization_grid_num_steps: int = 64, output_tree_dir: Optional[str] = None,
                      output_likelihood_dir: Optional[str] = None, max_bank_bytes: int = DEFAULT_MAX_BANK_BYTES, _version="1") -> None:
    """Refit the branch lengths of `<tree_dir>/<family>.txt` by at most `num_rounds` EM rounds under the rate matrix at the
    family's site rates, on the grid (center, step, num_steps) of `fast_cherries` / `nj_trees`.  Per family:
    `<output_tree_dir>/<family>.txt` (the input tree, topology, node names and their order untouched, every length a grid point),
    `<family>.rounds` (per round `<round> <log-likelihood at its start> <indices changed>`, then `final <log-likelihood of the
    written lengths>`; a family stops at its fixed point), `<family>.profiling`, and `<output_likelihood_dir>/<family>.txt` as
    `nj_trees` writes it (`dp_likelihood_computation_batch` on the written trees, root distribution = the matrix's stationary
    distribution).  All families go in one handle unless their banks would exceed `max_bank_bytes`; then they go in batches in
    family order -- families are independent, so the results do not depend on the batching."""
    inp = _read_stage_inputs("ml_branch_lengths", "fit", tree_dir, msa_dir, site_rates_dir, families, rate_matrix_path,
                             (quantization_grid_center, quantization_grid_step, quantization_grid_num_steps), output_tree_dir,
                             output_likelihood_dir)
    out_trees: List[Optional[Tree]] = [None] * len(families)
    logs: List[List[str]] = [[] for _ in families]
    profs: List[Dict[str, float]] = [{} for _ in families]
    for batch in _batches(inp.bank_bytes, int(max_bank_bytes)):
        st = time.time()
        with inp.fitter(batch, [inp.trees[f] for f in batch]) as fit:
            t_create = time.time() - st
            live = np.ones(len(batch), dtype=bool)
            ms_pass = ms_mstep = 0.0
            rounds = 0
            for rnd in range(int(num_rounds)):
                if not live.any():
                    break
                n_changed, fam_ll = fit.round()
                rounds += 1
                ms_pass, ms_mstep = ms_pass + fit.last_kernel_ms[0], ms_mstep + fit.last_kernel_ms[1]
                for k, f in enumerate(batch):
                    if live[k]:
                        logs[f].append(f"{rnd} {float(fam_ll[k])!r} {int(n_changed[k])}\n")
                live &= n_changed > 0
            lengths = fit.lengths()
            _, fam_final = fit.log_likelihoods()
        for k, f in enumerate(batch):
            logs[f].append(f"final {float(fam_final[k])!r}\n")
            out_trees[f] = _tree_at(inp.trees[f], lengths[k])
            profs[f] = dict(create_time=t_create / len(batch), rounds=rounds, passes_kernel_ms=ms_pass / len(batch),
                            mstep_kernel_ms=ms_mstep / len(batch), fit_time=(time.time() - st) / len(batch))   # (shares of the batch)
    _write_stage_outputs(inp, out_trees, logs, ".rounds", profs)


def _nj_stage(output_tree_dir: Optional[str], output_site_rates_dir: Optional[str], output_likelihood_dir: Optional[str],
              **nj_args) -> Dict[str, str]:
    """`nj_trees(**nj_args)` as the first stage of `nj_ml_trees`, `nj_nni_trees` and `nj_spr_trees` -> its output directories.
    With a cache directory its trees and likelihoods go to the cache; without one the three output directories are required
    and they go to the `nj_trees` subdirectories of the estimator's."""
    from ..caching import get_cache_dir
    from ._nj import nj_trees
    nj_out = dict(output_tree_dir=None, output_site_rates_dir=output_site_rates_dir, output_likelihood_dir=None)
    if get_cache_dir() is None:
        if output_tree_dir is None or output_site_rates_dir is None or output_likelihood_dir is None:
            raise ValueError("output_tree_dir, output_site_rates_dir and output_likelihood_dir are required without a cache directory")
        nj_out.update(output_tree_dir=os.path.join(output_tree_dir, "nj_trees"),
                      output_likelihood_dir=os.path.join(output_likelihood_dir, "nj_trees"))
    nj = nj_trees(**nj_args, **nj_out)
    return nj if nj is not None else nj_out


def nj_ml_trees(*, msa_dir: str, families: List[str], rate_matrix_path: str, num_rate_categories: int, max_iters: int = 50,
                num_processes: int = 1, num_rounds: int = 10, output_tree_dir: Optional[str] = None,
                output_site_rates_dir: Optional[str] = None, output_likelihood_dir: Optional[str] = None, remake=False,
                quantization_grid_center=0.03, quantization_grid_step=1.1, quantization_grid_num_steps=64, verbose=True,
                seed=1234, joiner="host") -> Dict[str, str]:
    """`nj_trees` (with its `joiner`), then `ml_branch_lengths` on its trees at its site rates and the same grid: `nj_trees`' interface plus
    `num_rounds`, and under `functools.partial` a `tree_estimator` of the end-to-end pipelines.  Returns the output directories:
    `output_tree_dir` / `output_likelihood_dir` hold the refitted trees and their likelihoods, `output_site_rates_dir` is
    `nj_trees`' own.  Both stages are cached on their own; `nj_trees`, its files and its cache keys are what they are without
    this function.  With no cache directory the three output directories are required and the neighbour-joining trees and
    likelihoods go to their `nj_trees` subdirectories."""
    grid_args = dict(quantization_grid_center=quantization_grid_center, quantization_grid_step=quantization_grid_step,
                     quantization_grid_num_steps=quantization_grid_num_steps)
    nj = _nj_stage(output_tree_dir, output_site_rates_dir, output_likelihood_dir, msa_dir=msa_dir, families=families,
                   rate_matrix_path=rate_matrix_path, num_rate_categories=num_rate_categories, max_iters=max_iters,
                   num_processes=num_processes, remake=remake, verbose=verbose, seed=seed, joiner=joiner, **grid_args)
    ml_out = dict(output_tree_dir=output_tree_dir, output_likelihood_dir=output_likelihood_dir)
    ml = ml_branch_lengths(tree_dir=nj["output_tree_dir"], msa_dir=msa_dir, site_rates_dir=nj["output_site_rates_dir"],
                           families=families, rate_matrix_path=rate_matrix_path, num_rounds=num_rounds, **grid_args, **ml_out)
    ml = ml if ml is not None else ml_out
    return dict(output_tree_dir=ml["output_tree_dir"], output_site_rates_dir=nj["output_site_rates_dir"],
                output_likelihood_dir=ml["output_likelihood_dir"])
