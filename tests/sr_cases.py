"""The small families the site-rate scan is checked on (tests/test_sr_cpu.py, tests/test_gpu_sr.py): bl_cases' trees and
simulation with the true rates drawn from the candidate list, the edge cases of the codes, the `current` arrays, and the
restatement's scan of each case -- computed once and shared.

case        S   (a workgroup's tile)  families: tree, sites, candidates                                        current
s4          4   (16 sites)            3-leaf star, 1, 1;  multifurcating internal node (TREES[4]), 70, 5       NULL
s20         20  (3 sites)             9-leaf caterpillar, 7, 40;  17 leaves with a trifurcating root, 70, 5    a mix
s32         32  (2 sites)             TREES[4], 2, 40;  3-leaf star, 7, 1                                      all -1
s20small    20                        17 leaves with a trifurcating root, 1, 5;  9-leaf caterpillar, 2, 1      a mix
s4general   4                         TREES[4], 7, 5;  3-leaf star, 2, 1 -- under a NON-reversible Q and a root          a mix
                                      distribution that is not its stationary one
Every family has 25 % gaps, an all-gap leaf, one length 0, one off the grid, one beyond its last point and (four or more edges)
one below its first; a family of 7 or more sites has an all-gap site (site 0) and a site with exactly one observed leaf (site 1)."""
import functools

import numpy as np

import bl_cases
import sr_reference
from bl_cases import GRID5, caterpillar, model, random_tree, star3
from test_em_cpu import GRID, TREES

CANDS1 = [1.0]
CANDS5 = [0.25, 0.5, 1.0, 2.0, 4.0]
CANDS40 = [round(0.05 * 1.14 ** k, 6) for k in range(40)]   # 0.05 .. 8.3


def family(parent, S, n_sites, cands, grid, seed, spread=(40, 85)):
    """(parent, length, codes, cands): the sites' true rates are drawn from at most four of the candidates"""
    rng = np.random.default_rng(1000 + seed)
    some = np.asarray(cands)[np.unique(np.linspace(0, len(cands) - 1, 4).astype(int))]
    seg = np.bincount(rng.integers(0, len(some), n_sites), minlength=len(some))
    parent, length, codes, _ = bl_cases.family(parent, S, [int(x) for x in seg], list(some), grid, seed, spread=spread)
    edges = [v for v in range(len(parent)) if parent[v] >= 0]
    if len(edges) >= 4:
        length[edges[3]] = 1e-7
    if n_sites >= 7:
        ch = sr_reference._children(parent)
        leaves = [v for v in range(len(parent)) if not ch[v]]
        codes[:, 0] = -1
        codes[:, 1] = -1
        codes[leaves[-1], 1] = S - 1
    return parent, length, codes, np.asarray(cands, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (S, [families], current: None or one index array per family)"""
    if name == "s4":
        S, fams, mode = 4, [family(star3(), 4, 1, CANDS1, GRID, 1), family(TREES[4][0], 4, 70, CANDS5, GRID, 26)], "null"
    elif name == "s20":
        S, fams, mode = 20, [family(caterpillar(9), 20, 7, CANDS40, GRID, 3),
                             family(random_tree(17, np.random.default_rng(5)), 20, 70, CANDS5, GRID, 4)], "mix"
    elif name == "s32":
        S, fams, mode = 32, [family(TREES[4][0], 32, 2, CANDS40, GRID5, 5, spread=(0, 5)),
                             family(star3(), 32, 7, CANDS1, GRID5, 6, spread=(0, 5))], "none"
    elif name == "s4general":
        S, fams, mode = 4, [family(TREES[4][0], 4, 7, CANDS5, GRID, 9), family(star3(), 4, 2, CANDS1, GRID, 10)], "mix"
    elif name == "s20small":
        S, fams, mode = 20, [family(random_tree(17, np.random.default_rng(8)), 20, 1, CANDS5, GRID, 7),
                             family(caterpillar(9), 20, 2, CANDS1, GRID, 8)], "mix"
    else:
        raise KeyError(name)
    if mode == "null":
        return S, fams, None
    rng = np.random.default_rng(len(name))
    current = []
    for _, _, codes, cands in fams:
        k = rng.integers(-1, len(cands), codes.shape[1]).astype(np.int32) if mode == "mix" else np.full(codes.shape[1], -1, np.int32)
        if mode == "mix" and codes.shape[1] >= 7:
            k[0], k[1] = -1, len(cands) - 1        # the all-gap site has none, the one-leaf site keeps the last candidate
        current.append(k)
    return S, fams, current


CASES = ["s4", "s20", "s32", "s20small", "s4general"]


@functools.lru_cache(maxsize=None)
def model_of(name):
    """(Q, pi_root) of the case: bl_cases' reversible model, or for s4general that model with a cyclic flow added"""
    S = case(name)[0]
    Q, pi = model(S)
    if name != "s4general":
        return Q, pi
    Q = Q.copy()
    for i in range(S):
        Q[i, (i + 1) % S] += 0.3
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q, np.random.default_rng(12).dirichlet(np.ones(S))


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement's scan of every family of the case"""
    S, fams, current = case(name)
    Q, pi = model_of(name)
    return [sr_reference.scan(parent, length, codes, cands, Q, pi, None if current is None else current[k])
            for k, (parent, length, codes, cands) in enumerate(fams)]
