"""The families the NNI scan and search are checked on (tests/test_nni_cpu.py, tests/test_gpu_nni.py): the four cases of
bl_cases.py -- S = 4, 20 and 32; the 3-leaf star (no move; it shares a handle with a family that has moves), the 9-leaf
caterpillar, the 17-leaf trees with a trifurcating root, the multifurcating internal node; category segments of 1 to 70 sites;
1, 4 and 20 categories; 25 % gaps and an all-gap leaf; lengths 0, off the grid and beyond it; T = 129 and T = 5 -- plus one case
of two small trees: the rooted binary 4-leaf tree, the smallest with a move (every move's p is the root), and a 4-leaf ladder
whose deepest move has a p that is not the root.  The restatement's scan of every family is computed once and shared; so is the
simulated family of the search test."""
import functools

import numpy as np

import bl_cases
import bl_reference
import nni_reference
from bl_cases import GRID

BIN4 = np.array([-1, 0, 0, 1, 1, 2, 2])       # ((a, b), (c, d))
LADDER4 = np.array([-1, 0, 0, 1, 1, 3, 3])    # (((a, b), c), d): v = 3 has p = 1
CASES = bl_cases.CASES + ["s4small"]
# moves per family: v (internal, not the root) contributes |ch(v)| (|ch(p)| - 1).  The 4-internal-node tree: 2 2 + 2 2 + 3 2;
# the caterpillar: 7 binary nodes under binary parents; the 17-leaf trees: 14 binary nodes, three of them under the
# trifurcating root (2 2 each, the others 2 1); the two small trees: 2 + 2 each
MOVE_COUNTS = {"s4": [0, 14], "s20": [14, 34], "s32": [14, 0], "s20one": [34], "s4small": [4, 4]}


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "s4small":
        return 4, GRID, [bl_cases.family(BIN4, 4, [2, 5], [0.5, 2.0], GRID, 21), bl_cases.family(LADDER4, 4, [7], [1.0], GRID, 22)]
    return bl_cases.case(name)


@functools.lru_cache(maxsize=None)
def restated(name):
    """per family (tau, moves, ll_moves [m, L], ll [L]) of the restatement at the snapped input lengths"""
    S, grid, fams = case(name)
    Q, pi = bl_cases.model(S)
    out = []
    for parent, length, codes, rates in fams:
        tau = bl_reference.snap(length, parent, grid)
        mvs = nni_reference.moves(parent)
        ll_moves, ll = nni_reference.scan(parent, tau, codes, rates, grid, Q, pi, mvs)
        out.append((tau, mvs, ll_moves, ll))
    return out


# ------------------------------------------------------------------------------------------------ the search test's family
SEARCH_SEED = 17   # chosen on the CPU: every decision of the restated search is decided (test_nni_cpu.py asserts it).  Most seeds
#                    are not: at the trifurcating root two conflicting moves give the same unrooted tree, and under a reversible
#                    model with a stationary root their gains tie up to rounding
SEARCH_NNI_ROUNDS, SEARCH_EM_ROUNDS = 4, 3
SEARCH_RATES = [0.3, 0.8, 1.5, 3.0]


@functools.lru_cache(maxsize=None)
def search_family(seed=SEARCH_SEED):
    """A 12-leaf family of 400 sites in 4 rate categories simulated (no gaps) under the 20-state model of bl_cases on a random
    tree whose lengths are grid points; the start is the true tree with three moves at disjoint places applied.
    -> dict(true_parent, start_parent, tau (the true indices), codes, rates)"""
    rng = np.random.default_rng(seed)
    parent = bl_cases.random_tree(12, rng)
    n = len(parent)
    tau = rng.integers(48, 72, n)          # lengths 0.007 .. 0.06 x rates: edges that leave a signal
    tau[parent < 0] = -1
    rates = rng.permutation(np.repeat(SEARCH_RATES, 100))
    Q, pi = bl_cases.model(20)
    # drawn down the tree with P[tau_v][c] on the edge above v (bl_cases.simulate without its gaps and its all-gap leaf)
    P = bl_reference.bank(GRID, np.unique(rates), Q)
    cat = np.searchsorted(np.unique(rates), rates)
    x = np.zeros((n, len(rates)), dtype=np.int64)
    root, _, order = bl_reference._preorder(parent)
    x[root] = rng.choice(20, len(rates), p=pi)
    for v in order[1:]:
        rows = np.clip(P[tau[v], cat, x[parent[v]]], 0.0, None)
        cdf = np.cumsum(rows / rows.sum(axis=1, keepdims=True), axis=1)
        x[v] = np.minimum((rng.random(len(rates))[:, None] > cdf).sum(axis=1), 19)
    codes = x.astype(np.int8)
    mvs = nni_reference.moves(parent)
    taken = []
    while len(taken) < 3:                  # (a random order may block itself: draw again)
        taken, used = [], set()
        for m in rng.permutation(len(mvs)):
            v, c, s = (int(x) for x in mvs[m])
            four = {int(parent[v]), v, c, s}
            if len(taken) < 3 and not used & four:
                used |= four
                taken.append(mvs[m])
    return dict(true_parent=parent, start_parent=nni_reference.apply(parent, taken), tau=tau, codes=codes, rates=rates)


@functools.lru_cache(maxsize=None)
def restated_search(seed=SEARCH_SEED):
    f = search_family(seed)
    Q, pi = bl_cases.model(20)
    return nni_reference.search(f["start_parent"], f["tau"], f["codes"], f["rates"], GRID, Q, pi, SEARCH_NNI_ROUNDS, SEARCH_EM_ROUNDS)
