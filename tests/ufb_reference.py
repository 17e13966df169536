"""A NumPy restatement of the bootstrap supports from the NNI search's own trees (include/cherrybank.h, cb_bl_bootstrap_best;
csrc/ufb.hip.h; phylogeny_estimation/_ufboot.py), with the margin of every replicate's decision, so that a
test knows which of them rounding could turn.  It builds on the restated scan (nni_reference.scan), the restated weights
(sup_reference.weights) and the pieces of the restated search (nni_reference) and shares nothing with the package.

One call, one family of L sites: l_u its per-site log-likelihood, ll'_m[u] the scan's for move m, d_m[u] = ll'_m[u] - l_u (0
where either is not finite), w_r[u] the multiplicities of sup_reference.weights (replicate r here is replicate r of the branch
supports).  B^r = sum_u w_r[u] l_u (l_u taken as 0 where it is not finite), Delta_m^r = sum_u w_r[u] d_m[u]; a move whose
Delta_m = sum_u d_m[u] is not finite is left out.  The candidates of replicate r, in order:
    code -2   the incoming best (-inf on the first call)        code -1   the tree itself, B^r
    code  m   move m, in the order of the list, B^r + Delta_m^r
The result is the largest score and the code of the FIRST candidate that attains it.

The search: a handle contributes when the family's tree on it is accepted -- in nni_reference.search's loop that is every
iteration (the tree `parent` after its EM rounds: the start tree, or a candidate that was kept) and the closing EM rounds after a
move in the last round.  The running best is carried from one contribution to the next; replicate r records (t, code).  Its
bootstrap tree is contribution t's tree with the one move applied when code >= 0, and the ufboot of an internal non-root node of
the final tree is the share of the replicates whose bootstrap tree has the node's leaf split (nni_reference.splits; one leaf
against the rest is in every tree: 1)."""
import functools

import numpy as np

import bl_cases
import bl_reference
import nni_cases
import nni_reference
import sup_reference
from em_reference import _children

REPLICATES = 256


def scores(ll_moves, ll, W):
    """-> (base [R], score [m, R] = base + Delta (a move left out: -inf everywhere), delta_rep [m, R], used [m])"""
    ll = np.asarray(ll, dtype=np.float64)
    ll_moves = np.asarray(ll_moves, dtype=np.float64).reshape(-1, len(ll))
    Wf = W.T.astype(np.float64)
    base = np.where(np.isfinite(ll), ll, 0.0) @ Wf
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(ll)[None, :], ll_moves - ll[None, :], 0.0)
        used = np.isfinite(d.sum(axis=1))
    delta_rep = np.where(np.isfinite(d), d, 0.0) @ Wf
    score = np.where(used[:, None], base[None, :] + delta_rep, -np.inf)
    return base, score, delta_rep, used


def best(ll_moves, ll, R, seed, incoming=None, W=None):
    """one call on one family -> dict(score [R], code [R], base [R], cand [2 + m, R] the candidates' scores in their order
    (row 0 the incoming best, row 1 the tree), margin [R] = the best minus the second best candidate (inf with one candidate))"""
    ll = np.asarray(ll)
    W = sup_reference.weights(len(ll), R, seed) if W is None else W
    base, score, _, _ = scores(ll_moves, ll, W)
    incoming = np.full(R, -np.inf) if incoming is None else np.asarray(incoming, dtype=np.float64)
    cand = np.vstack([incoming[None, :], base[None, :], score])
    arg = np.argmax(cand, axis=0)                     # the first of equal maxima
    top = np.sort(cand, axis=0)[-2:]
    with np.errstate(invalid="ignore"):
        margin = np.where(np.isfinite(top[0]), top[1] - top[0], np.inf)
    return dict(score=cand[arg, np.arange(R)], code=arg - 2, base=base, cand=cand, margin=margin, fam_ll=float(ll.sum()))


@functools.lru_cache(maxsize=None)
def restated(name, R=REPLICATES):
    """per family of the case a first call at the snapped input lengths, seeds sup_reference.family_seed(k)"""
    return [best(ll_moves, ll, R, sup_reference.family_seed(k)) for k, (_, _, ll_moves, ll) in enumerate(nni_cases.restated(name))]


# ------------------------------------------------------------------------------------------------------------ the search
def contributions(parent, tau, codes, rates, grid, Q, pi, num_nni_rounds, num_rounds):
    """nni_reference.search's loop, recording every accepted tree after its EM rounds -> (the final parent array,
    [dict(parent, tau, moves, ll_moves, ll, nni_round)])"""
    parent, tau = np.asarray(parent).copy(), np.asarray(tau).copy()
    P = bl_reference.bank(grid, np.unique(rates), Q)
    with np.errstate(divide="ignore"):
        logP = np.log(np.where(P > 0, P, 0.0))
    out = []

    def contribute(rnd):
        nonlocal tau
        tau, _ = nni_reference._em(parent, tau, codes, rates, grid, Q, pi, P, num_rounds)
        mvs = nni_reference.moves(parent)
        ll_moves, ll = nni_reference.scan(parent, tau, codes, rates, grid, Q, pi, mvs, logP)
        out.append(dict(parent=parent.copy(), tau=tau.copy(), moves=mvs, ll_moves=ll_moves, ll=ll, nni_round=rnd))
        return mvs, ll_moves, ll

    moved = True
    for rnd in range(num_nni_rounds):
        mvs, ll_moves, ll = contribute(rnd)
        before = float(ll.sum())
        delta = (ll_moves - ll[None, :]).sum(axis=1)
        sel = mvs[nni_reference.select(mvs, delta, parent)]
        moved = False
        while len(sel):
            cand = nni_reference.apply(parent, sel)
            if float(nni_reference.site_ll(cand, tau, codes, rates, grid, Q, pi, logP).sum()) > before:
                parent, moved = cand, True
                break
            sel = sel[:len(sel) // 2]
        if not moved:
            break
    if moved:
        contribute(num_nni_rounds)
    return parent, out


def carry(contribs, R, seed):
    """the running best over the contributions -> dict(t [R], code [R], score [R], margin [R] = the best minus the second best
    of ALL candidates of all contributions, pairs = {(t, code): replicates})"""
    W = sup_reference.weights(len(contribs[0]["ll"]), R, seed)
    score = np.full(R, -np.inf)
    t_arr, code = np.full(R, -1, dtype=np.int64), np.full(R, -2, dtype=np.int64)
    rows = []
    for t, c in enumerate(contribs):
        res = best(c["ll_moves"], c["ll"], R, seed, incoming=score, W=W)
        won = res["code"] != -2
        t_arr[won], code[won], score = t, res["code"][won], res["score"]
        rows.append(res["cand"][1:])
    union = np.vstack(rows)
    top = np.sort(union, axis=0)[-2:]
    pairs = {}
    for key in zip(t_arr.tolist(), code.tolist()):
        pairs[key] = pairs.get(key, 0) + 1
    return dict(t=t_arr, code=code, score=score, margin=top[1] - top[0], union=union, pairs=pairs)


def chosen_parent(contribs, t, code):
    c = contribs[t]
    return c["parent"] if code < 0 else nni_reference.apply(c["parent"], [c["moves"][code]])


def supports(final_parent, contribs, t_arr, code):
    """-> (nodes: the internal non-root nodes of the final tree ascending, share [len(nodes)])"""
    final_parent = np.asarray(final_parent)
    ch = _children(final_parent)
    leaves = frozenset(v for v in range(len(final_parent)) if not ch[v])

    def below(v):
        return frozenset([v]) if not ch[v] else frozenset().union(*(below(w) for w in ch[v]))

    nodes = [v for v in range(len(final_parent)) if final_parent[v] >= 0 and ch[v]]
    have = {}
    share = np.zeros(len(nodes))
    for t, c in zip(np.asarray(t_arr).tolist(), np.asarray(code).tolist()):
        if (t, c) not in have:
            have[(t, c)] = nni_reference.splits(chosen_parent(contribs, t, c))
        for g, v in enumerate(nodes):
            a = below(v)
            trivial = not 1 < len(a) < len(leaves) - 1
            share[g] += trivial or frozenset([a, leaves - a]) in have[(t, c)]
    return np.array(nodes, dtype=np.int64), share / len(np.asarray(t_arr))


@functools.lru_cache(maxsize=None)
def restated_search(R=REPLICATES, seed=1):
    """nni_cases.search_family() searched with SEARCH_NNI_ROUNDS / SEARCH_EM_ROUNDS ->
    (final parent, contributions, carry(...), (nodes, share))"""
    f = nni_cases.search_family()
    Q, pi = bl_cases.model(20)
    final, contribs = contributions(f["start_parent"], f["tau"], f["codes"], f["rates"], nni_cases.GRID, Q, pi,
                                    nni_cases.SEARCH_NNI_ROUNDS, nni_cases.SEARCH_EM_ROUNDS)
    c = carry(contribs, R, seed)
    return final, contribs, c, supports(final, contribs, c["t"], c["code"])
