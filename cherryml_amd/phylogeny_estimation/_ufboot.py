"""Bootstrap supports from the NNI search's own trees (csrc/ufb.hip.h, `cb_bl_bootstrap_best`).

While `ml_nni_trees` searches, every tree it meets is scored under every site resample by RELL: the resampled log-likelihood of
a tree is the sum of its per-site log-likelihoods weighted by how often the resample drew each site.  The bootstrap tree of a
replicate is the met tree with the highest resampled log-likelihood, and the support (`ufboot`) of an edge of the FINAL tree is
the share of the replicates whose bootstrap tree has the edge's leaf split.  This is the idea of IQ-TREE's ultrafast bootstrap
(Minh et al. 2013), not its arithmetic: there is no likelihood-threshold filter and no convergence criterion, the neighbours are
not re-optimised, and the candidate set is exactly the search's accepted trees and their single-NNI neighbours at the accepted
tree's (unrefitted) lengths.

A handle of the search "contributes" when the family's tree on it is accepted -- the input tree or an accepted candidate; the
handle on which the family ends contributes too, a handle whose candidate was refused does not.  After the family's EM rounds
on contributing handle t, `BranchLengthFitter.bootstrap_best` takes the running best of every replicate, the handle's tree
(code -1) and all of `nni_moves()` (code m) and returns the new best and its code on the GPU; the host records (t, code) where
the code is not -2 ("the incoming best stays").  `ufboot_supports` then builds every DISTINCT chosen tree once
(`contributions[t]`, with move `code` of `enumerate_nni_moves` applied where code >= 0) and counts splits on packed bitsets.

Out of scope: IQ-TREE's threshold, convergence and refinement steps, re-optimising neighbours, transfer distances of the
bootstrap trees, consensus trees, the 400-state model or S > 32, writing supports into the tree file format."""
from typing import Dict, List, Sequence, Tuple

import numpy as np

from ..io._tree import Tree
from ._bootstrap import _node_splits, tree_splits
from ._nni import _parent_array, apply_nni, enumerate_nni_moves

HEADER = "node ufboot\n"


def bootstrap_tree(contributions: Sequence[Tree], t: int, code: int) -> Tree:
    """the tree a replicate chose: contribution t, with move `code` of its `enumerate_nni_moves` applied where code >= 0"""
    t, code = int(t), int(code)
    if not 0 <= t < len(contributions):
        raise ValueError(f"bootstrap_tree: contribution {t} of {len(contributions)}")
    tree = contributions[t]
    if code == -1:
        return tree
    moves = enumerate_nni_moves(_parent_array(tree))
    if not 0 <= code < len(moves):
        raise ValueError(f"bootstrap_tree: code {code} on contribution {t}, which has {len(moves)} moves (-1: the tree itself)")
    return apply_nni(tree, moves[code])


def update_choice(choice: Tuple[np.ndarray, np.ndarray], t: int, code) -> None:
    """record one contribution's codes in the running choice (t [R], code [R]), in place: a replicate whose code is not -2
    now chooses (t, code)"""
    won = np.asarray(code) != -2
    choice[0][won] = t
    choice[1][won] = np.asarray(code)[won]


def ufboot_supports(final_tree: Tree, contributions: Sequence[Tree], choice) -> Tuple[np.ndarray, np.ndarray]:
    """-> (nodes, share): per internal non-root node of `final_tree`, in `tree.nodes()` order, its index in `tree.nodes()` and
    the share of the replicates whose bootstrap tree has the leaf split of the edge above it (unrooted splits, as `tree_splits`
    forms them; a trivial split -- one leaf against the rest -- is in every tree: 1).  `contributions`: the contributing trees
    of the search, all on the leaves of `final_tree`; `choice` = (t [R], code [R]): replicate r chose contribution t[r], itself
    (code -1) or with move code[r] of `enumerate_nni_moves` applied.  Every distinct (t, code) tree is built once."""
    t_arr = np.asarray(choice[0], dtype=np.int64).reshape(-1)
    c_arr = np.asarray(choice[1], dtype=np.int64).reshape(-1)
    if t_arr.shape != c_arr.shape or t_arr.size == 0:
        raise ValueError("ufboot_supports: choice must be (t [R], code [R]) with R >= 1")
    names = list(final_tree.leaves())
    nodes, packed, real = _node_splits(final_tree, names)
    keys = [row.tobytes() for row in packed]
    count = np.zeros(len(keys), dtype=np.int64)
    pairs, n_won = np.unique(np.stack([t_arr, c_arr], axis=1), axis=0, return_counts=True)
    for (t, code), k in zip(pairs.tolist(), n_won.tolist()):
        have = {row.tobytes() for row in tree_splits(bootstrap_tree(contributions, t, code), names)}
        count += k * np.array([key in have for key in keys], dtype=np.int64)
    share = np.where(real, count / t_arr.size, 1.0)
    return nodes, share


def write_ufboot_supports(path: str, names: Sequence[str], nodes, share) -> None:
    """the header `node ufboot`, then per internal non-root node `name share`; `names` = `tree.nodes()`"""
    with open(path, "w") as fh:
        fh.write(HEADER + "".join(f"{names[int(v)]} {float(s)!r}\n" for v, s in zip(nodes, share)))


def read_ufboot_supports(path: str) -> Dict[str, float]:
    """{node: share} of a file `write_ufboot_supports` wrote"""
    lines = open(path).read().split("\n")
    if lines[0] + "\n" != HEADER:
        raise ValueError(f"{path}: not a ufboot support file (header {lines[0]!r})")
    return {x[0]: float(x[1]) for x in (ln.split() for ln in lines[1:] if ln)}


def choices_lines(rounds: Sequence[int], candidates: Sequence[int], choice) -> List[str]:
    """the lines of `<family>.choices`: per contribution `t nni_round candidates replicates_won_by_tree
    replicates_won_by_moves`"""
    t_arr, c_arr = np.asarray(choice[0]), np.asarray(choice[1])
    return [f"{t} {int(rounds[t])} {int(candidates[t])} {int(np.sum((t_arr == t) & (c_arr == -1)))} "
            f"{int(np.sum((t_arr == t) & (c_arr >= 0)))}\n" for t in range(len(rounds))]
