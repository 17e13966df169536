"""The small families the branch-length EM is checked on (tests/test_bl_cpu.py, tests/test_gpu_bl.py): trees, leaves simulated
down the tree under the model, site-rate categories, and the restatement's round on each case -- computed once and shared."""
import functools

import numpy as np

import bl_reference
from test_em_cpu import GRID, TREES, _random_Q

GRID5 = [0.01, 0.05, 0.2, 0.8, 3.0]
RATES20 = [round(0.1 * 1.22 ** k, 6) for k in range(20)]   # 0.1 .. 4.4


def star3():
    return np.array([-1, 0, 0, 0])


def caterpillar(n_leaves):
    """internal nodes 0 .. n-2 in a chain (0 the root), leaf k hangs off internal min(k, n-2)"""
    ni = n_leaves - 1
    return np.array([-1] + list(range(ni - 1)) + [min(k, ni - 1) for k in range(n_leaves)])


def random_tree(n_leaves, rng):
    """random joins down to a trifurcating root (the root is the last node)"""
    nodes, parent, nxt = list(range(n_leaves)), {}, n_leaves
    while len(nodes) > 3:
        i, j = rng.choice(len(nodes), 2, replace=False)
        a, b = nodes[i], nodes[j]
        parent[a] = parent[b] = nxt
        nodes = [x for x in nodes if x not in (a, b)] + [nxt]
        nxt += 1
    for a in nodes:
        parent[a] = nxt
    return np.array([parent.get(v, -1) for v in range(nxt + 1)])


def simulate(parent, tau, rates, grid, Q, pi, rng, gap_fraction=0.25):
    """leaf codes [n_nodes, L] drawn down the tree with P[tau_v][c] on the edge above v; `gap_fraction` of the leaf entries
    become gaps and the first leaf is all gaps"""
    parent = np.asarray(parent)
    cats = np.unique(rates)
    P = bl_reference.bank(grid, cats, Q)
    cat = np.searchsorted(cats, rates)
    root, ch, order = bl_reference._preorder(parent)
    S, L = Q.shape[0], len(rates)
    x = np.zeros((len(parent), L), dtype=np.int64)
    x[root] = rng.choice(S, L, p=pi)
    for v in order[1:]:
        rows = np.clip(P[tau[v], cat, x[parent[v]]], 0.0, None)            # [L, S]
        cdf = np.cumsum(rows / rows.sum(axis=1, keepdims=True), axis=1)
        x[v] = np.minimum((rng.random(L)[:, None] > cdf).sum(axis=1), S - 1)
    codes = x.astype(np.int8)
    leaves = [v for v in range(len(parent)) if not ch[v]]
    codes[rng.random(codes.shape) < gap_fraction] = -1
    codes[leaves[0]] = -1
    return codes


def family(parent, S, segments, rate_list, grid, seed, spread=(40, 85)):
    """(parent, length, codes, rates): `segments[k]` sites at rate `rate_list[k]` (shuffled over the alignment); lengths are
    grid points in `spread`, except one exactly 0, one off the grid and one beyond its last point"""
    rng = np.random.default_rng(seed)
    n, T = len(parent), len(grid)
    Q, pi = model(S)
    true = rng.integers(min(spread[0], T - 1), min(spread[1], T), n)
    rates = rng.permutation(np.repeat(np.asarray(rate_list, dtype=np.float64)[:len(segments)], segments))
    codes = simulate(parent, true, rates, grid, Q, pi, rng)
    length = np.asarray(grid)[true].astype(np.float64)
    edges = [v for v in range(n) if parent[v] >= 0]
    length[edges[0]] = 0.0
    length[edges[1]] *= 1.03
    length[edges[2]] = 1e4
    length[parent < 0] = 0.0
    return np.asarray(parent), length, codes, rates


@functools.lru_cache(maxsize=None)
def model(S):
    return _random_Q(S, 7)


# name -> (S, grid, [families]); the families of one case share a handle
@functools.lru_cache(maxsize=None)
def case(name):
    if name == "s4":        # the smallest tree with one site; a multifurcating internal node, segments of 3, 4, 5 and > 64 sites
        return 4, GRID, [family(star3(), 4, [1], [1.0], GRID, 10), family(TREES[4][0], 4, [3, 4, 5, 70], [0.3, 0.8, 1.5, 3.0], GRID, 2)]
    if name == "s20":       # height-bound tree with 20 categories; a trifurcating root with 4 of the 20 rates (the others empty)
        seg = [1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5]
        return 20, GRID, [family(caterpillar(9), 20, seg, RATES20, GRID, 3),
                          family(random_tree(17, np.random.default_rng(5)), 20, [1, 3, 5, 65], RATES20[3::5], GRID, 4)]
    if name == "s32":       # exact fit of the tiles; fewer candidates than lanes
        return 32, GRID5, [family(TREES[4][0], 32, [4, 5], [0.5, 2.0], GRID5, 6, spread=(0, 5)),
                           family(star3(), 32, [3], [1.0], GRID5, 7, spread=(0, 5))]
    if name == "s20one":    # one category of more than 64 sites on the 17-leaf tree
        return 20, GRID, [family(random_tree(17, np.random.default_rng(8)), 20, [66], [1.0], GRID, 9)]
    raise KeyError(name)


CASES = ["s4", "s20", "s32", "s20one"]


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement's round on every family of the case, from the snapped input lengths"""
    S, grid, fams = case(name)
    Q, pi = model(S)
    out = []
    for parent, length, codes, rates in fams:
        tau = bl_reference.snap(length, parent, grid)
        out.append((tau, bl_reference.em_round(parent, tau, codes, rates, grid, Q, pi)))
    return out
