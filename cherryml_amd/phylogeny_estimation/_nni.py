"""Topology search by nearest-neighbour interchange (NNI) on the branch-length handle (csrc/nni.hip.h, `cb_bl_nni_scan`;
DESIGN.md section 18).

A move on a rooted, possibly multifurcating tree is a triple of node indices (v, c, s) in `tree.nodes()` order: v internal and
not the root, p = parent[v], c a child of v, s a child of p other than v.  It exchanges the subtrees of c and s; every node
keeps the edge above it and that edge's length.  `BranchLengthFitter.nni_scan` scores all moves of a tree from the messages its
passes leave resident; `select_nni` picks a set of moves at disjoint places, `apply_nni` makes the rearranged tree, and
`ml_nni_trees` alternates the branch-length EM with scan / select / apply, keeping a candidate tree only if its likelihood at
the same lengths is strictly higher.  `nj_nni_trees` is the tree estimator `nj_trees` + `ml_nni_trees`.

Out of scope: SPR / TBR moves (SPR is `_spr.py`), changing a handle's topology in place (a rearranged tree gets a new handle), refitting site
rates inside the search, S > 32."""
import os
import time
from typing import Dict, List, Optional

import numpy as np

from .. import _lib
from ..caching import cached_computation
from ..io._tree import Tree
from ._ml_lengths import DEFAULT_MAX_BANK_BYTES, _nj_stage
from ._search import HandleHooks, MoveKind, search_trees


def enumerate_nni_moves(parent) -> np.ndarray:
    """int32 [n, 3]: all moves (v, c, s) of the tree with this parent array (the root: -1) -- v ascending, then c over the
    children of v, then s over the children of parent[v] other than v, children in node order"""
    parent = np.asarray(parent)
    ch: List[List[int]] = [[] for _ in parent]
    for v, p in enumerate(parent):
        if p >= 0:
            ch[int(p)].append(v)
    out = [(v, c, s) for v, p in enumerate(parent) if p >= 0 and ch[v] for c in ch[v] for s in ch[int(p)] if s != v]
    return np.array(out, dtype=np.int32).reshape(-1, 3)


def _parent_array(tree: Tree) -> np.ndarray:
    index = {v: i for i, v in enumerate(tree.nodes())}
    parent = np.full(len(index), -1, dtype=np.int32)
    for u, v, _ in tree.edges():
        parent[index[v]] = index[u]
    return parent


def apply_nni(tree: Tree, moves) -> Tree:
    """A new `Tree` with the nodes of `tree` in the same order and, for every move (v, c, s) (node indices in `tree.nodes()`
    order), the subtrees of c and s exchanged: parent[c] = parent[v], parent[s] = v.  Every node keeps the length of the edge
    above it, and the edges keep their order.  ValueError for a triple that is no move of the tree and for a set of moves that
    share a node (of the four of a move: parent[v], v, c, s): such moves do not commute."""
    moves = np.asarray(moves, dtype=np.int64).reshape(-1, 3)
    nodes = tree.nodes()
    parent = _parent_array(tree)
    n = len(nodes)
    new = parent.copy()
    used: Dict[int, int] = {}
    for k, (v, c, s) in enumerate(moves.tolist()):
        if not (0 <= v < n and 0 <= c < n and 0 <= s < n):
            raise ValueError(f"apply_nni: move {k} = ({v}, {c}, {s}): an index outside [0, {n})")
        p = int(parent[v])
        if p < 0 or parent[c] != v or s == v or parent[s] != p:
            raise ValueError(f"apply_nni: move {k} = ({v}, {c}, {s}) is no move of the tree (v internal and not the root, c a "
                             f"child of v, s another child of parent[v] = {p})")
        for w in (p, v, c, s):
            if w in used:
                raise ValueError(f"apply_nni: moves {used[w]} and {k} share node {w} ({nodes[w]})")
        for w in (p, v, c, s):
            used[w] = k
        new[c], new[s] = p, v
    index = {v: i for i, v in enumerate(nodes)}
    out = Tree()
    out.add_nodes(nodes)
    out.add_edges([(nodes[int(new[index[v]])], v, t) for _, v, t in tree.edges()])
    return out


def select_nni(moves, delta, parent, min_gain: float = 0.0) -> np.ndarray:
    """The indices (into `moves`) of a set of moves at disjoint places, greedily by descending `delta` (ties: the lower move
    index): only moves with delta > min_gain are considered, and a move is taken only if none of its four nodes {parent[v], v,
    c, s} belongs to a move already taken.  In the order taken."""
    moves = np.asarray(moves, dtype=np.int64).reshape(-1, 3)
    delta = np.asarray(delta, dtype=np.float64).reshape(-1)
    parent = np.asarray(parent)
    if delta.size != len(moves):
        raise ValueError(f"select_nni: {len(moves)} moves and {delta.size} deltas")
    order = [int(m) for m in np.argsort(-delta, kind="stable") if delta[m] > min_gain]
    used, taken = set(), []
    for m in order:
        v, c, s = (int(x) for x in moves[m])
        four = {int(parent[v]), v, c, s}
        if used & four:
            continue
        used |= four
        taken.append(m)
    return np.array(taken, dtype=np.int64)


def _scan_nni(fit, trees, want):
    moves, delta = fit.nni_scan([m if w else m[:0] for m, w in zip(fit.nni_moves(), want)])
    return moves, delta, fit.last_nni_kernel_ms[1]


NNI = MoveKind(stage="ml_nni_trees", log_ext=".nni", rounds_key="nni_rounds", scan=_scan_nni, select=select_nni,
               apply=lambda tree, moves, grid: apply_nni(tree, moves))


class _SupportsAndBootstrap(HandleHooks):
    """`ml_nni_trees`' `output_support_dir` and `output_bootstrap_dir`, either or none, on the search's own handles"""

    def __init__(self, families: List[str], output_support_dir: Optional[str], num_support_replicates: int,
                 output_bootstrap_dir: Optional[str], num_bootstrap_replicates: int, bootstrap_seed: int, max_bank_bytes: int):
        self.families, self.max_bank_bytes = families, max_bank_bytes
        self.support_dir, self.n_support = output_support_dir, num_support_replicates
        self.bootstrap_dir, self.n_boot, self.bootstrap_seed = output_bootstrap_dir, int(num_bootstrap_replicates), bootstrap_seed
        F, n_boot = len(families), max(self.n_boot, 0)
        self.supports: List[Optional[tuple]] = [None] * F   # the final trees' supports
        # per family: the running best score of every replicate, the (t, code) it chose, the contributing trees and per
        # contribution its NNI round and its number of candidates
        self.best: List[Optional[np.ndarray]] = [None] * F
        self.choice = [(np.full(n_boot, -1, dtype=np.int64), np.full(n_boot, -2, dtype=np.int64)) for _ in families]
        self.contributions: List[List[Tree]] = [[] for _ in families]
        self.rounds: List[List[int]] = [[] for _ in families]
        self.cands: List[List[int]] = [[] for _ in families]
        self.ufb = self.all_moves = None                    # of the current handle

    def on_handle(self, fit, fams, go, ends, prof) -> None:
        from ._supports import support_seeds
        names = [self.families[f] for f in fams]
        if self.support_dir is not None and any(ends):
            sup = fit.branch_supports(self.n_support, seeds=support_seeds(names, 0),
                                      moves=[m if e else m[:0] for m, e in zip(fit.nni_moves(), ends)])
            for k, f in enumerate(fams):
                if ends[k]:
                    self.supports[f] = sup[k]
        self.ufb = None
        if self.bootstrap_dir is not None and go.any():
            # every family whose tree on this handle is accepted contributes it and all its neighbours; a refused
            # candidate meets an incoming best of +inf, which nothing beats, and its result is dropped
            n_boot = self.n_boot
            self.all_moves = fit.nni_moves()
            st_ufb = time.time()
            self.ufb = fit.bootstrap_best(n_boot, seeds=support_seeds(names, self.bootstrap_seed),
                                          best=[(np.full(n_boot, -np.inf) if self.best[f] is None else self.best[f]) if go[k]
                                                else np.full(n_boot, np.inf) for k, f in enumerate(fams)],
                                          moves=[m if g else m[:0] for m, g in zip(self.all_moves, go)])
            for f in fams:                             # (shares of the batch; these keys exist only with the bootstrap)
                prof[f]["bootstrap_time"] = prof[f].get("bootstrap_time", 0.0) + (time.time() - st_ufb) / len(fams)
                prof[f]["bootstrap_kernel_ms"] = (prof[f].get("bootstrap_kernel_ms", 0.0)
                                                  + fit.last_ufboot_kernel_ms[2] / len(fams))
                prof[f]["bootstrap_scan_kernel_ms"] = (prof[f].get("bootstrap_scan_kernel_ms", 0.0)   # its own passes and scan
                                                       + sum(fit.last_ufboot_kernel_ms[:2]) / len(fams))

    def on_accepted(self, k, f, tree, rnd) -> None:
        from ._ufboot import update_choice
        if self.ufb is not None:
            self.best[f] = self.ufb[k][0]
            update_choice(self.choice[f], len(self.contributions[f]), self.ufb[k][1])
            self.contributions[f].append(tree)
            self.rounds[f].append(rnd)
            self.cands[f].append(1 + len(self.all_moves[k]))

    def finish(self, inp, trees) -> None:
        from ._supports import support_seeds, supports_of_trees, write_supports
        from ._ufboot import choices_lines, ufboot_supports, write_ufboot_supports
        if self.support_dir is not None:
            os.makedirs(self.support_dir, exist_ok=True)
            # a family whose last candidate was refused ends on the tree of an earlier handle: one more handle for those
            rest = [f for f in range(len(trees)) if self.supports[f] is None]
            if rest:
                got, _ = supports_of_trees([trees[f] for f in rest], [inp.codes[f] for f in rest], [inp.rates[f] for f in rest],
                                           inp.grid, inp.Q, inp.pi_root, support_seeds([self.families[f] for f in rest], 0),
                                           int(self.n_support), inp.device, self.max_bank_bytes)
                for f, res in zip(rest, got):
                    self.supports[f] = res
            for f, family in enumerate(self.families):
                write_supports(os.path.join(self.support_dir, family + ".txt"), list(trees[f].nodes()), self.supports[f])
        if self.bootstrap_dir is not None:
            os.makedirs(self.bootstrap_dir, exist_ok=True)
            for f, family in enumerate(self.families):
                nodes, share = ufboot_supports(trees[f], self.contributions[f], self.choice[f])
                write_ufboot_supports(os.path.join(self.bootstrap_dir, family + ".txt"), list(trees[f].nodes()), nodes, share)
                with open(os.path.join(self.bootstrap_dir, family + ".choices"), "w") as fh:
                    fh.write("".join(choices_lines(self.rounds[f], self.cands[f], self.choice[f])))


@cached_computation(output_dirs=["output_tree_dir", "output_likelihood_dir"], exclude_args=["max_bank_bytes"])
def ml_nni_trees(tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str,
                 num_nni_rounds: int = 10, num_rounds: int = 10, quantization_grid_center: float = 0.03,
                 quantization_grid_step: float = 1.1, quantization_grid_num_steps: int = 64, output_tree_dir: Optional[str] = None,
                 output_likelihood_dir: Optional[str] = None, max_bank_bytes: int = DEFAULT_MAX_BANK_BYTES,
                 output_support_dir: Optional[str] = None, num_support_replicates: int = 1000,
                 output_bootstrap_dir: Optional[str] = None, num_bootstrap_replicates: int = 1000, bootstrap_seed: int = 0,
                 _version="1") -> None:
    """Improve the topologies of `<tree_dir>/<family>.txt` by likelihood: at most `num_nni_rounds` times, per family, fit the
    lengths of the current tree (`BranchLengthFitter`, at most `num_rounds` EM rounds), score ALL its nearest-neighbour
    interchanges (`nni_scan`), select those of positive gain at disjoint places (`select_nni`) and apply them (`apply_nni`).
    The gains of simultaneous moves are not additive, so the candidate tree is kept only if its log-likelihood at the same
    lengths -- `log_likelihoods()` of the next round's fitter on it, before any EM round -- is strictly above the one before
    the moves (so a round costs one handle); otherwise the family retries with the first half of its selected moves, down to
    one move (whose gain is exact).  A family with no accepted move is finished; a family that still moved in the last NNI
    round gets EM rounds on its final topology.
    Per family: `<output_tree_dir>/<family>.txt` (the input's node names and their order, every length a grid point),
    `<family>.nni` (per NNI round `<round> <log-likelihood before> <moves scanned> <selected> <applied> <log-likelihood after,
    same lengths>`, then `final <log-likelihood of the written tree>`: no number is below the one before it),
    `<family>.profiling`, and `<output_likelihood_dir>/<family>.txt` as `ml_branch_lengths` writes it.  With
    `output_support_dir`, also `<output_support_dir>/<family>.txt` as `ml_branch_supports` writes it: the aLRT, SH-like and RELL
    supports of the FINAL tree's internal edges from `num_support_replicates` site resamples (seed
    `simulation.family_seed(family, 0)`), computed on the last handle that holds the final tree at its final lengths; without
    it (the default) nothing else is written or computed.  With `output_bootstrap_dir`, also the bootstrap supports of the
    FINAL tree's internal edges from the search's own trees (`_ufboot.py`; UFBoot's idea, not IQ-TREE's
    arithmetic): on every handle on which the family's tree is accepted, after its EM rounds, `bootstrap_best` scores that tree
    and all its NNI neighbours under `num_bootstrap_replicates` site resamples (seed `simulation.family_seed(family,
    bootstrap_seed)`) against the running best of every replicate; `<output_bootstrap_dir>/<family>.txt` holds the header
    `node ufboot` and per internal non-root node of the final tree, in `tree.nodes()` order, the share of the replicates whose
    best tree has the split of the edge above it, `<family>.choices` per contributing handle
    `<t> <nni_round> <candidates> <replicates won by the tree> <replicates won by its neighbours>`.  A family's file does not
    depend on its batch; without the directory (the default) every other file is byte for byte what it is with it."""
    hooks = _SupportsAndBootstrap(families, output_support_dir, num_support_replicates, output_bootstrap_dir,
                                  num_bootstrap_replicates, bootstrap_seed, max_bank_bytes)
    search_trees(NNI, num_nni_rounds, num_rounds, max_bank_bytes, hooks, tree_dir, msa_dir, site_rates_dir, families,
                 rate_matrix_path, (quantization_grid_center, quantization_grid_step, quantization_grid_num_steps), output_tree_dir,
                 output_likelihood_dir)


def nj_nni_trees(*, msa_dir: str, families: List[str], rate_matrix_path: str, num_rate_categories: int, max_iters: int = 50,
                 num_processes: int = 1, num_rounds: int = 10, num_nni_rounds: int = 10, output_tree_dir: Optional[str] = None,
                 output_site_rates_dir: Optional[str] = None, output_likelihood_dir: Optional[str] = None, remake=False,
                 quantization_grid_center=0.03, quantization_grid_step=1.1, quantization_grid_num_steps=64, verbose=True,
                 seed=1234, output_support_dir: Optional[str] = None, num_support_replicates: int = 1000,
                 joiner="host", output_bootstrap_dir: Optional[str] = None, num_bootstrap_replicates: int = 1000,
                 bootstrap_seed: int = 0) -> Dict[str, str]:
    """`nj_trees` (with its `joiner`), then `ml_nni_trees` on its trees at its site rates and the same grid: `nj_ml_trees`'
    interface plus `num_nni_rounds`, and under `functools.partial` a `tree_estimator` of the end-to-end pipelines.  Returns the output
    directories: `output_tree_dir` / `output_likelihood_dir` hold the searched trees and their likelihoods,
    `output_site_rates_dir` is `nj_trees`' own.  Both stages are cached on their own.  With no cache directory the three output
    directories are required and the neighbour-joining trees and likelihoods go to their `nj_trees` subdirectories.  With
    `output_support_dir` the supports of the final trees are written there (`ml_nni_trees`); the returned dict is the same.
    With `output_bootstrap_dir` the bootstrap supports from the search's own trees are written there (`ml_nni_trees`,
    `num_bootstrap_replicates`, `bootstrap_seed`); the returned dict is the same."""
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError("nj_nni_trees: no HIP device visible; the search runs on the MI355X only (no CPU fallback)")
    grid_args = dict(quantization_grid_center=quantization_grid_center, quantization_grid_step=quantization_grid_step,
                     quantization_grid_num_steps=quantization_grid_num_steps)
    nj = _nj_stage(output_tree_dir, output_site_rates_dir, output_likelihood_dir, msa_dir=msa_dir, families=families,
                   rate_matrix_path=rate_matrix_path, num_rate_categories=num_rate_categories, max_iters=max_iters,
                   num_processes=num_processes, remake=remake, verbose=verbose, seed=seed, joiner=joiner, **grid_args)
    out = dict(output_tree_dir=output_tree_dir, output_likelihood_dir=output_likelihood_dir)
    sup = dict(output_support_dir=output_support_dir, num_support_replicates=num_support_replicates,
               output_bootstrap_dir=output_bootstrap_dir, num_bootstrap_replicates=num_bootstrap_replicates,
               bootstrap_seed=bootstrap_seed)
    ml = ml_nni_trees(tree_dir=nj["output_tree_dir"], msa_dir=msa_dir, site_rates_dir=nj["output_site_rates_dir"],
                      families=families, rate_matrix_path=rate_matrix_path, num_nni_rounds=num_nni_rounds, num_rounds=num_rounds,
                      **grid_args, **out, **sup)
    ml = ml if ml is not None else out
    return dict(output_tree_dir=ml["output_tree_dir"], output_site_rates_dir=nj["output_site_rates_dir"],
                output_likelihood_dir=ml["output_likelihood_dir"])
