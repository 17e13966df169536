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
from ..io._tree import Tree, read_tree, write_tree
from ._fast_cherries import quantization_points_ble
from ._ml_lengths import DEFAULT_MAX_BANK_BYTES, BranchLengthFitter, _batches


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
    from ..counting._host import read_msa, read_site_rates
    from ..counting._stage import _device_index
    from ..evaluation._likelihood import (_family_units, _stationary_distribution, dp_likelihood_computation_batch,
                                          write_log_likelihood)
    from ..io import read_rate_matrix
    from ._supports import support_seeds, supports_of_trees, write_supports
    from ._ufboot import choices_lines, ufboot_supports, update_choice, write_ufboot_supports
    if output_tree_dir is None or output_likelihood_dir is None:
        raise ValueError("output_tree_dir and output_likelihood_dir are required")
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError("ml_nni_trees: no HIP device visible; the search runs on the MI355X only (no CPU fallback)")
    st_all = time.time()
    for d in (output_tree_dir, output_likelihood_dir):
        os.makedirs(d, exist_ok=True)
    rm = read_rate_matrix(rate_matrix_path)
    alphabet = [str(c) for c in rm.columns]
    Q = np.ascontiguousarray(rm.to_numpy(), dtype=np.float64)
    pi_root = _stationary_distribution(Q)
    grid = np.array(quantization_points_ble(quantization_grid_center, quantization_grid_step, quantization_grid_num_steps))
    device = _device_index()
    trees, msas, rates, codes = [], [], [], []
    for family in families:
        tree = read_tree(os.path.join(tree_dir, family + ".txt"))
        msa = read_msa(os.path.join(msa_dir, family + ".txt"))
        r = np.asarray(read_site_rates(os.path.join(site_rates_dir, family + ".txt")), dtype=np.float64)
        trees.append(tree), msas.append(msa), rates.append(r)
        # (the codes' rows follow tree.nodes(), which no move changes)
        codes.append(_family_units(tree, msa, None, len(r), alphabet, False)[2])
    F = len(families)
    logs: List[List[str]] = [[] for _ in families]
    prof = [dict(create_time=0.0, scan_time=0.0, scan_kernel_ms=0.0, fit_time=0.0, handles=0, nni_rounds=0, moves_applied=0)
            for _ in families]
    final_ll: List[Optional[float]] = [None] * F
    supports: List[Optional[tuple]] = [None] * F   # (with output_support_dir) the final trees' supports
    # (with output_bootstrap_dir) per family: the running best score of every replicate, the (t, code) it chose, the contributing
    # trees and per contribution its NNI round and its number of candidates
    n_boot = int(num_bootstrap_replicates)
    ufb_best: List[Optional[np.ndarray]] = [None] * F
    ufb_choice = [(np.full(max(n_boot, 0), -1, dtype=np.int64), np.full(max(n_boot, 0), -2, dtype=np.int64)) for _ in families]
    contributions: List[List[Tree]] = [[] for _ in families]
    ufb_rounds: List[List[int]] = [[] for _ in families]
    ufb_cands: List[List[int]] = [[] for _ in families]
    bank_bytes = [2 * grid.size * np.unique(r).size * Q.size * 8 for r in rates]
    # Per family: rnd = its NNI round; trees[f] = the tree the next handle takes -- the input, or a candidate (fitted[f] with the
    # moves sel[f] applied) that has to beat before[f].  ONE handle per pass over the work list: on a candidate its
    # log_likelihoods() before any EM round decides (the lengths are the fitted ones: grid points snap to themselves), and the
    # accepted families go on in the same handle with the EM rounds and the scan of their next round.
    rnd = [0] * F
    before: List[Optional[float]] = [None] * F
    fitted: List[Optional[Tree]] = [None] * F
    sel: List[Optional[np.ndarray]] = [None] * F
    scanned, selected = [0] * F, [0] * F
    work = list(range(F))
    while work:
        nxt: List[int] = []
        for batch in _batches([bank_bytes[f] for f in work], int(max_bank_bytes)):
            fams = [work[k] for k in batch]
            st = time.time()
            with BranchLengthFitter([trees[f] for f in fams], [codes[f] for f in fams], [rates[f] for f in fams], grid, Q, pi_root,
                                    device=device) as fit:
                t_create = time.time() - st
                go = np.ones(len(fams), dtype=bool)            # the input tree, or an accepted candidate
                if any(before[f] is not None for f in fams):
                    _, ll0 = fit.log_likelihoods()
                    for k, f in enumerate(fams):
                        if before[f] is None:
                            continue
                        if ll0[k] > before[f]:
                            logs[f].append(f"{rnd[f]} {before[f]!r} {scanned[f]} {selected[f]} {len(sel[f])} {float(ll0[k])!r}\n")
                            prof[f]["moves_applied"] += len(sel[f])
                            rnd[f] += 1
                        else:
                            go[k] = False
                live = go.copy()                               # (a refused candidate's rounds are nobody's)
                for _ in range(int(num_rounds)):
                    if not live.any():
                        break
                    n_changed, _ = fit.round()
                    live &= n_changed > 0
                lengths = fit.lengths()
                _, fam_ll = fit.log_likelihoods()
                want = [bool(go[k]) and rnd[f] < int(num_nni_rounds) for k, f in enumerate(fams)]
                st_scan = time.time()
                if any(want):
                    moves, delta = fit.nni_scan([m if w else m[:0] for m, w in zip(fit.nni_moves(), want)])
                t_scan, ms_scan = time.time() - st_scan, fit.last_nni_kernel_ms[1]
                picked = [moves[k][select_nni(moves[k], delta[k], _parent_array(trees[f]))] if want[k] else None
                          for k, f in enumerate(fams)]
                if output_support_dir is not None:
                    # the families that end on this handle's tree at these lengths: no further round, or no move that gains
                    ends = [bool(go[k]) and (not want[k] or len(picked[k]) == 0) for k in range(len(fams))]
                    if any(ends):
                        sup = fit.branch_supports(num_support_replicates, seeds=support_seeds([families[f] for f in fams], 0),
                                                  moves=[m if e else m[:0] for m, e in zip(fit.nni_moves(), ends)])
                        for k, f in enumerate(fams):
                            if ends[k]:
                                supports[f] = sup[k]
                ufb = None
                if output_bootstrap_dir is not None and go.any():
                    # every family whose tree on this handle is accepted contributes it and all its neighbours; a refused
                    # candidate meets an incoming best of +inf, which nothing beats, and its result is dropped
                    all_moves = fit.nni_moves()
                    st_ufb = time.time()
                    ufb = fit.bootstrap_best(n_boot, seeds=support_seeds([families[f] for f in fams], bootstrap_seed),
                                             best=[(np.full(n_boot, -np.inf) if ufb_best[f] is None else ufb_best[f]) if go[k]
                                                   else np.full(n_boot, np.inf) for k, f in enumerate(fams)],
                                             moves=[m if g else m[:0] for m, g in zip(all_moves, go)])
                    for f in fams:                             # (shares of the batch; these keys exist only with the bootstrap)
                        prof[f]["bootstrap_time"] = prof[f].get("bootstrap_time", 0.0) + (time.time() - st_ufb) / len(fams)
                        prof[f]["bootstrap_kernel_ms"] = (prof[f].get("bootstrap_kernel_ms", 0.0)
                                                          + fit.last_ufboot_kernel_ms[2] / len(fams))
                        prof[f]["bootstrap_scan_kernel_ms"] = (prof[f].get("bootstrap_scan_kernel_ms", 0.0)   # its own passes and scan
                                                               + sum(fit.last_ufboot_kernel_ms[:2]) / len(fams))
            for k, f in enumerate(fams):
                for key, x in (("create_time", t_create), ("scan_time", t_scan), ("scan_kernel_ms", ms_scan),
                               ("fit_time", time.time() - st)):
                    prof[f][key] += x / len(fams)              # (shares of the batch)
                prof[f]["handles"] += 1
                if not go[k]:                                  # refused: half of the moves, down to one, whose gain is exact
                    if len(sel[f]) > 1:
                        sel[f] = sel[f][:len(sel[f]) // 2]
                        trees[f] = apply_nni(fitted[f], sel[f])
                        nxt.append(f)
                    else:                                      # (rounding only)
                        logs[f].append(f"{rnd[f]} {before[f]!r} {scanned[f]} {selected[f]} 0 {before[f]!r}\n")
                        trees[f], final_ll[f] = fitted[f], before[f]
                    continue
                t = Tree()
                t.add_nodes(trees[f].nodes())
                t.add_edges([(u, v, lengths[k][v]) for u, v, _ in trees[f].edges()])
                trees[f], ll = t, float(fam_ll[k])
                if ufb is not None:
                    ufb_best[f] = ufb[k][0]
                    update_choice(ufb_choice[f], len(contributions[f]), ufb[k][1])
                    contributions[f].append(t)
                    ufb_rounds[f].append(rnd[f])
                    ufb_cands[f].append(1 + len(all_moves[k]))
                if not want[k]:                                # the topology of the last round's moves after its own EM rounds
                    final_ll[f] = ll
                    continue
                prof[f]["nni_rounds"] += 1
                s = picked[k]
                scanned[f], selected[f] = len(moves[k]), len(s)
                if len(s) == 0:                                # no move gains: finished
                    logs[f].append(f"{rnd[f]} {ll!r} {scanned[f]} 0 0 {ll!r}\n")
                    final_ll[f] = ll
                    continue
                fitted[f], before[f], sel[f] = t, ll, s
                trees[f] = apply_nni(t, s)
                nxt.append(f)
        work = nxt
    if output_support_dir is not None:
        os.makedirs(output_support_dir, exist_ok=True)
        # a family whose last candidate was refused ends on the tree of an earlier handle: one more handle for those
        rest = [f for f in range(F) if supports[f] is None]
        if rest:
            got, _ = supports_of_trees([trees[f] for f in rest], [codes[f] for f in rest], [rates[f] for f in rest], grid, Q, pi_root,
                                       support_seeds([families[f] for f in rest], 0), int(num_support_replicates), device,
                                       max_bank_bytes)
            for f, res in zip(rest, got):
                supports[f] = res
        for f, family in enumerate(families):
            write_supports(os.path.join(output_support_dir, family + ".txt"), list(trees[f].nodes()), supports[f])
    if output_bootstrap_dir is not None:
        os.makedirs(output_bootstrap_dir, exist_ok=True)
        for f, family in enumerate(families):
            nodes, share = ufboot_supports(trees[f], contributions[f], ufb_choice[f])
            write_ufboot_supports(os.path.join(output_bootstrap_dir, family + ".txt"), list(trees[f].nodes()), nodes, share)
            with open(os.path.join(output_bootstrap_dir, family + ".choices"), "w") as fh:
                fh.write("".join(choices_lines(ufb_rounds[f], ufb_cands[f], ufb_choice[f])))
    st = time.time()
    lls = dp_likelihood_computation_batch(trees, msas, [None] * F, [[float(x) for x in r] for r in rates], alphabet, pi_root, Q,
                                          device=device)
    t_ll = (time.time() - st) / max(F, 1)
    t_total = (time.time() - st_all) / max(F, 1)
    for f, family in enumerate(families):
        write_tree(trees[f], os.path.join(output_tree_dir, family + ".txt"))
        with open(os.path.join(output_tree_dir, family + ".nni"), "w") as fh:
            fh.write("".join(logs[f]) + f"final {final_ll[f]!r}\n")
        write_log_likelihood(lls[f], os.path.join(output_likelihood_dir, family + ".txt"))
        with open(os.path.join(output_tree_dir, family + ".profiling"), "w") as fh:
            fh.write("".join(f"{k}: {v}\n" for k, v in prof[f].items()) + f"likelihood_time: {t_ll}\ntotal_time: {t_total}")


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
    from ..caching import get_cache_dir
    from ._nj import nj_trees
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError("nj_nni_trees: no HIP device visible; the search runs on the MI355X only (no CPU fallback)")
    nj_out = dict(output_tree_dir=None, output_site_rates_dir=output_site_rates_dir, output_likelihood_dir=None)
    if get_cache_dir() is None:
        if output_tree_dir is None or output_site_rates_dir is None or output_likelihood_dir is None:
            raise ValueError("output_tree_dir, output_site_rates_dir and output_likelihood_dir are required without a cache directory")
        nj_out.update(output_tree_dir=os.path.join(output_tree_dir, "nj_trees"),
                      output_likelihood_dir=os.path.join(output_likelihood_dir, "nj_trees"))
    grid_args = dict(quantization_grid_center=quantization_grid_center, quantization_grid_step=quantization_grid_step,
                     quantization_grid_num_steps=quantization_grid_num_steps)
    nj = nj_trees(msa_dir=msa_dir, families=families, rate_matrix_path=rate_matrix_path, num_rate_categories=num_rate_categories,
                  max_iters=max_iters, num_processes=num_processes, remake=remake, verbose=verbose, seed=seed, joiner=joiner, **grid_args,
                  **nj_out)
    nj = nj if nj is not None else nj_out
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
