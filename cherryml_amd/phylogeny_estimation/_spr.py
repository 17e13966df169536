"""Topology search by subtree prune-and-regraft (SPR) on the branch-length handle (csrc/spr.hip.h, `cb_bl_spr_scan`; DESIGN.md
section 25).

A move on a rooted, possibly multifurcating tree is (x, y, tau_s, tau_p, tau_y), node indices in `tree.nodes()` order: x is the
pruned node, p = parent[x] must be binary and not the root, s is the other child of p and g = parent[p]; y is the node whose
edge receives the subtree -- not the root, not x, p or s, not in the subtree of x.  The rearranged tree has parent[s] = g,
parent[p] = the old parent[y], parent[y] = p, and x stays under p; the edges above s, p and y take the grid indices tau_s,
tau_p, tau_y and every other node keeps its edge.  With T' the tree without x and p, the distance of y is the number of nodes
of T' on the path between the merged edge g-s and the edge above y: distance 1 gives the NNI topologies, and a search radius
of 3 has about nine times as many moves as NNI.

`enumerate_spr_moves` lists the (x, y) within a radius, `spr_indices` is the one place that decides which three indices a move
is offered at, `BranchLengthFitter.spr_scan` scores moves from the messages the handle's passes leave resident, `select_spr`
picks moves whose touched sets are disjoint, `apply_spr` makes the rearranged tree, and `ml_spr_trees` alternates the
branch-length EM with scan / select / apply, keeping a candidate tree only if its likelihood at the carried lengths is strictly
higher.  `nj_spr_trees` is the tree estimator `nj_trees` + `ml_spr_trees` (+ `ml_nni_trees`).

Out of scope: TBR, optimising the three lengths per candidate beyond the one offered triple, changing a handle's topology in
place, S > 32, SPR candidates in `bootstrap_best` and `branch_supports`."""
import os
from typing import Dict, List, Optional, Set, Tuple

import numpy as np

from .. import _lib
from ..caching import cached_computation
from ..io._tree import Tree
from ._ml_lengths import DEFAULT_MAX_BANK_BYTES, _nj_stage
from ._nni import _parent_array
from ._search import MoveKind, search_trees

SPR_MAX_RADIUS = 8   # CB_SPR_MAX_RADIUS of include/cherrybank.h


def _children(parent) -> List[List[int]]:
    ch: List[List[int]] = [[] for _ in parent]
    for v, p in enumerate(parent):
        if p >= 0:
            ch[int(p)].append(v)
    return ch


def _route(parent, ch, x: int, y: int) -> Optional[Tuple[List[int], List[int]]]:
    """(up, down) for a move (x, y), None for what is none: `up` = [g, a1, ..., ak], the ancestors the way climbs (empty for a
    target below s), `down` = the nodes it descends through, ending on y ([s, z1, ..., y] below s; [z1, ..., y], or empty
    where y is the last of `up`, otherwise)"""
    n = len(parent)
    if not (0 <= x < n and 0 <= y < n):
        return None
    p = int(parent[x])
    if p < 0 or parent[p] < 0 or len(ch[p]) != 2 or parent[y] < 0:
        return None
    s = ch[p][0] if ch[p][0] != x else ch[p][1]
    if y in (x, p, s):
        return None
    chain = [y]                                    # y and its ancestors, up to s or the root
    while chain[-1] != s and parent[chain[-1]] >= 0:
        chain.append(int(parent[chain[-1]]))
        if chain[-1] == x:
            return None
    if chain[-1] == s:
        return [], chain[::-1]
    where = {w: i for i, w in enumerate(chain)}
    up = [int(parent[p])]
    while up[-1] not in where:
        up.append(int(parent[up[-1]]))
    return up, chain[:where[up[-1]]][::-1]


def enumerate_spr_moves(parent, radius: int = 3) -> np.ndarray:
    """int32 [n, 2]: all (x, y) of distance <= radius of the tree with this parent array (the root: -1) -- x ascending, then y
    ascending.  Per x a walk of at most `radius` nodes outwards from the two ends of the merged edge: a node reached at
    distance d gives that distance to the edges it has not come through."""
    parent = np.asarray(parent)
    if not 1 <= int(radius) <= SPR_MAX_RADIUS:
        raise ValueError(f"enumerate_spr_moves: radius = {radius} (1 <= radius <= {SPR_MAX_RADIUS})")
    ch = _children(parent)
    par = [int(q) for q in parent]
    out = []
    for x, p in enumerate(par):
        if p < 0 or par[p] < 0 or len(ch[p]) != 2:
            continue
        s = ch[p][0] if ch[p][0] != x else ch[p][1]
        g = par[p]
        ys = []
        front = [(s, g), (g, p)]                   # (node, the neighbour the walk came from); s counts as coming from g
        for _ in range(int(radius)):
            nxt = []
            for w, back in front:
                if w != s and par[w] >= 0 and par[w] != back:
                    ys.append(w)                   # the edge above w
                    nxt.append((par[w], w))
                for c in ch[w]:
                    if c != back:
                        ys.append(c)
                        nxt.append((c, w))
            front = nxt
        out += [(x, y) for y in sorted(ys)]
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def spr_indices(grid, tau, parent, xy) -> np.ndarray:
    """int32 [n, 3] (tau_s, tau_p, tau_y), the indices the moves (x, y) are offered at: the merged edge keeps the prune point's
    path length -- tau_s is the grid index nearest to grid[tau[p]] + grid[tau[s]] -- and the regraft edge is halved -- tau_p =
    tau_y is the index nearest to grid[tau[y]] / 2.  Nearest: the smallest |log grid[k] - log t| in float64, the lowest index
    on ties; the grid's ends clamp."""
    grid = np.asarray(grid, dtype=np.float64).reshape(-1)
    log_grid = np.log(grid)
    parent, tau = np.asarray(parent), np.asarray(tau)
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    if len(xy) == 0:
        return np.zeros((0, 3), dtype=np.int32)
    ch = _children(parent)
    p = parent[xy[:, 0]]
    s = np.array([ch[q][0] if ch[q][0] != x else ch[q][1] for x, q in zip(xy[:, 0].tolist(), p.tolist())])

    def nearest(t):
        return np.argmin(np.abs(log_grid[None, :] - np.log(t)[:, None]), axis=1)

    half = nearest(grid[tau[xy[:, 1]]] / 2)
    return np.stack([nearest(grid[tau[p]] + grid[tau[s]]), half, half], axis=1).astype(np.int32)


def _moves_at(parent, tau, grid, radius: int) -> np.ndarray:
    """int32 [n, 5]: the moves within `radius` at `spr_indices`' indices"""
    xy = enumerate_spr_moves(parent, radius)
    return np.ascontiguousarray(np.concatenate([xy, spr_indices(grid, tau, parent, xy)], axis=1), dtype=np.int32)


def _touched(parent, ch, x: int, y: int, what: str, k: int) -> Set[int]:
    r = _route(parent, ch, x, y)
    if r is None:
        raise ValueError(f"{what}: move {k} = ({x}, {y}) is no move of the tree (parent[x] binary and not the root; y not the "
                         f"root, not x, parent[x] or the other child of parent[x], not in the subtree of x)")
    p = int(parent[x])
    s = ch[p][0] if ch[p][0] != x else ch[p][1]
    return {x, p, s, int(parent[p]), y, int(parent[y])} | set(r[0]) | set(r[1])


def select_spr(moves, delta, parent, min_gain: float = 0.0) -> np.ndarray:
    """The indices (into `moves`, [n, >= 2] with columns x, y first) of a set of moves at disjoint places, greedily by
    descending `delta` (ties: the lower move index): only moves with delta > min_gain are considered, and a move is taken only
    if its touched set -- {x, p, s, g, y, parent[y]} and every node on the way from the prune point to y -- meets that of no
    move already taken.  With the way in the set no taken move can carry another's y into its x's subtree.  In the order
    taken."""
    moves = np.asarray(moves, dtype=np.int64)
    moves = moves.reshape(-1, moves.shape[-1] if moves.ndim == 2 else 5)
    delta = np.asarray(delta, dtype=np.float64).reshape(-1)
    parent = np.asarray(parent)
    if delta.size != len(moves):
        raise ValueError(f"select_spr: {len(moves)} moves and {delta.size} deltas")
    ch = _children(parent)
    order = [int(m) for m in np.argsort(-delta, kind="stable") if delta[m] > min_gain]
    used: Set[int] = set()
    taken = []
    for m in order:
        t = _touched(parent, ch, int(moves[m][0]), int(moves[m][1]), "select_spr", m)
        if used & t:
            continue
        used |= t
        taken.append(m)
    return np.array(taken, dtype=np.int64)


def apply_spr(tree: Tree, moves, grid) -> Tree:
    """A new `Tree` with the nodes of `tree` in the same order and the moves (x, y, tau_s, tau_p, tau_y) (node indices in
    `tree.nodes()` order) applied in order: parent[s] = g, parent[p] = the old parent[y], parent[y] = p; the edges above s, p
    and y get the lengths grid[tau_s], grid[tau_p], grid[tau_y], every other node keeps the length of the edge above it, and
    the edges keep their order.  ValueError for what is no move of the tree, an index outside the grid, and moves whose touched
    sets (`select_spr`) meet: such moves do not commute."""
    moves = np.asarray(moves, dtype=np.int64).reshape(-1, 5)
    grid = np.asarray(grid, dtype=np.float64).reshape(-1)
    nodes = tree.nodes()
    parent = _parent_array(tree)
    ch = _children(parent)
    new = parent.copy()
    length: Dict[int, float] = {}
    used: Dict[int, int] = {}
    for k, (x, y, ts, tp, ty) in enumerate(moves.tolist()):
        t = _touched(parent, ch, x, y, "apply_spr", k)
        for tau in (ts, tp, ty):
            if not 0 <= tau < grid.size:
                raise ValueError(f"apply_spr: move {k} = ({x}, {y}, {ts}, {tp}, {ty}): an index outside [0, {grid.size})")
        for w in sorted(t):
            if w in used:
                raise ValueError(f"apply_spr: moves {used[w]} and {k} share node {w} ({nodes[w]})")
        for w in t:
            used[w] = k
        p = int(parent[x])
        s = ch[p][0] if ch[p][0] != x else ch[p][1]
        new[s], new[p], new[y] = parent[p], parent[y], p
        length[s], length[p], length[y] = float(grid[ts]), float(grid[tp]), float(grid[ty])
    index = {v: i for i, v in enumerate(nodes)}
    out = Tree()
    out.add_nodes(nodes)
    out.add_edges([(nodes[int(new[index[v]])], v, length.get(index[v], t)) for _, v, t in tree.edges()])
    return out


@cached_computation(output_dirs=["output_tree_dir", "output_likelihood_dir"], exclude_args=["max_bank_bytes"])
def ml_spr_trees(tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str,
                 num_spr_rounds: int = 10, spr_radius: int = 3, num_rounds: int = 10, quantization_grid_center: float = 0.03,
                 quantization_grid_step: float = 1.1, quantization_grid_num_steps: int = 64, output_tree_dir: Optional[str] = None,
                 output_likelihood_dir: Optional[str] = None, max_bank_bytes: int = DEFAULT_MAX_BANK_BYTES, _version="1") -> None:
    """Improve the topologies of `<tree_dir>/<family>.txt` by likelihood with subtree prune-and-regraft moves: `ml_nni_trees`'
    loop with the SPR pieces.  At most `num_spr_rounds` times, per family, fit the lengths of the current tree
    (`BranchLengthFitter`, at most `num_rounds` EM rounds), score ALL its moves within `spr_radius` at `spr_indices`' lengths
    (`spr_scan`), select those of positive gain at disjoint places (`select_spr`) and apply them (`apply_spr`).  The candidate
    is kept only if its log-likelihood at the carried lengths -- `log_likelihoods()` of the next round's fitter on it, before
    any EM round -- is strictly above the one before the moves; otherwise the family retries with the first half of its
    selected moves, down to one (whose gain is exact).  A family with no accepted move is finished; a family that still moved
    in the last round gets EM rounds on its final topology.
    Per family: `<output_tree_dir>/<family>.txt` (the input's node names and their order, every length a grid point),
    `<family>.spr` (per round `<round> <log-likelihood before> <moves scanned> <selected> <applied> <log-likelihood after,
    carried lengths>`, then `final <log-likelihood of the written tree>`: no number is below the one before it),
    `<family>.profiling`, and `<output_likelihood_dir>/<family>.txt` as `ml_branch_lengths` writes it."""
    def scan(fit, trees, want):
        none = np.zeros((0, 5), dtype=np.int32)
        moves, delta = fit.spr_scan([_moves_at(_parent_array(tree), tau, fit.grid, spr_radius) if w else none
                                     for tree, tau, w in zip(trees, fit.indices(), want)])
        return moves, delta, fit.last_spr_kernel_ms[1]

    kind = MoveKind(stage="ml_spr_trees", log_ext=".spr", rounds_key="spr_rounds", scan=scan, select=select_spr, apply=apply_spr)
    search_trees(kind, num_spr_rounds, num_rounds, max_bank_bytes, None, tree_dir, msa_dir, site_rates_dir, families,
                 rate_matrix_path, (quantization_grid_center, quantization_grid_step, quantization_grid_num_steps), output_tree_dir,
                 output_likelihood_dir)


def nj_spr_trees(*, msa_dir: str, families: List[str], rate_matrix_path: str, num_rate_categories: int, max_iters: int = 50,
                 num_processes: int = 1, num_rounds: int = 10, num_spr_rounds: int = 10, spr_radius: int = 3,
                 num_nni_rounds: int = 0, output_tree_dir: Optional[str] = None, output_site_rates_dir: Optional[str] = None,
                 output_likelihood_dir: Optional[str] = None, remake=False, quantization_grid_center=0.03,
                 quantization_grid_step=1.1, quantization_grid_num_steps=64, verbose=True, seed=1234,
                 output_support_dir: Optional[str] = None, num_support_replicates: int = 1000, joiner="host",
                 output_bootstrap_dir: Optional[str] = None, num_bootstrap_replicates: int = 1000,
                 bootstrap_seed: int = 0) -> Dict[str, str]:
    """`nj_trees` (with its `joiner`), then `ml_spr_trees` on its trees at its site rates and the same grid, then -- with
    `num_nni_rounds` > 0 (default 0) -- `ml_nni_trees` on the result: `nj_nni_trees`' interface plus `num_spr_rounds` and
    `spr_radius`, and under `functools.partial` a `tree_estimator` of the end-to-end pipelines.  Returns the output
    directories: `output_tree_dir` / `output_likelihood_dir` hold the searched trees and their likelihoods,
    `output_site_rates_dir` is `nj_trees`' own.  Every stage is cached on its own.  With no cache directory the three output
    directories are required; the neighbour-joining trees and likelihoods go to their `nj_trees` subdirectories and, where
    `ml_nni_trees` follows, the SPR search's to their `spr_trees` subdirectories.  The supports and the search bootstrap are
    `ml_nni_trees`' (the SPR search has none): `output_support_dir` and `output_bootstrap_dir` need `num_nni_rounds` > 0."""
    from ..caching import get_cache_dir
    from ._nni import ml_nni_trees
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError("nj_spr_trees: no HIP device visible; the search runs on the MI355X only (no CPU fallback)")
    nni = int(num_nni_rounds) > 0
    if not nni and (output_support_dir is not None or output_bootstrap_dir is not None):
        raise ValueError("nj_spr_trees: output_support_dir and output_bootstrap_dir are ml_nni_trees' (num_nni_rounds > 0)")
    out = dict(output_tree_dir=output_tree_dir, output_likelihood_dir=output_likelihood_dir)
    spr_out = dict(out) if not nni else dict(output_tree_dir=None, output_likelihood_dir=None)
    grid_args = dict(quantization_grid_center=quantization_grid_center, quantization_grid_step=quantization_grid_step,
                     quantization_grid_num_steps=quantization_grid_num_steps)
    nj = _nj_stage(output_tree_dir, output_site_rates_dir, output_likelihood_dir, msa_dir=msa_dir, families=families,
                   rate_matrix_path=rate_matrix_path, num_rate_categories=num_rate_categories, max_iters=max_iters,
                   num_processes=num_processes, remake=remake, verbose=verbose, seed=seed, joiner=joiner, **grid_args)
    if nni and get_cache_dir() is None:   # (_nj_stage has required the output directories)
        spr_out.update(output_tree_dir=os.path.join(output_tree_dir, "spr_trees"),
                       output_likelihood_dir=os.path.join(output_likelihood_dir, "spr_trees"))
    ml = ml_spr_trees(tree_dir=nj["output_tree_dir"], msa_dir=msa_dir, site_rates_dir=nj["output_site_rates_dir"],
                      families=families, rate_matrix_path=rate_matrix_path, num_spr_rounds=num_spr_rounds, spr_radius=spr_radius,
                      num_rounds=num_rounds, **grid_args, **spr_out)
    ml = ml if ml is not None else spr_out
    if nni:
        sup = dict(output_support_dir=output_support_dir, num_support_replicates=num_support_replicates,
                   output_bootstrap_dir=output_bootstrap_dir, num_bootstrap_replicates=num_bootstrap_replicates,
                   bootstrap_seed=bootstrap_seed)
        res = ml_nni_trees(tree_dir=ml["output_tree_dir"], msa_dir=msa_dir, site_rates_dir=nj["output_site_rates_dir"],
                           families=families, rate_matrix_path=rate_matrix_path, num_nni_rounds=num_nni_rounds,
                           num_rounds=num_rounds, **grid_args, **out, **sup)
        ml = res if res is not None else out
    return dict(output_tree_dir=ml["output_tree_dir"], output_site_rates_dir=nj["output_site_rates_dir"],
                output_likelihood_dir=ml["output_likelihood_dir"])
