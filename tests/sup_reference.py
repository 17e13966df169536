"""A NumPy restatement of the local branch supports (include/cherrybank.h, cb_bl_supports): the site
resampling, the resampled deltas of every move and, per edge, aLRT, the SH-like count and the RELL count -- with the margin of
every decision, so that a test knows which of them rounding could turn.  It builds on the restated scan (nni_cases.restated) and
on sim_stream.philox4x32_10 and shares nothing else with the package.

For one family of L sites: l_u its per-site log-likelihood, ll'_m[u] the scan's for move m, d_m[u] = ll'_m[u] - l_u (0 where l_u
is not finite), delta_m = sum_u d_m[u].  Replicate r draws L sites with replacement: draw j takes word j & 3 of
philox4x32_10(counter = (j >> 2, r, 0, 0x53555050), key = (seed low word, seed high word)) and lands on site (word * L) >> 32;
w_r[u] counts the draws of u; delta_m^r = sum_u w_r[u] d_m[u].  The moves with one v are the group G of the edge above v (a move
whose delta is not finite is left out; an empty group gets NaN, -1, -1):
    alrt = -2 max_G delta_m;   rell = #{r: max_G delta_m^r <= 0};
    sh   = #{r: -max_G delta_m > t^r},  t^r = the largest minus the second largest of {0} and {delta_m^r - delta_m : m in G}."""
import functools

import numpy as np

import bl_cases
import nni_cases
import nni_reference
from sim_stream import philox4x32_10

TAG = 0x53555050
REPLICATES = 256


def family_seed(k):
    """the seed of family k of its case"""
    return 1 + 1000 * k


def weights(L, R, seed):
    """int64 [R, L]: how often each site (the caller's order) is drawn in each replicate"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (L + 3) // 4
    q = np.broadcast_to(np.arange(nq, dtype=np.uint64)[None, :], (R, nq))
    r = np.broadcast_to(np.arange(R, dtype=np.uint64)[:, None], (R, nq))
    zero = np.zeros((R, nq), dtype=np.uint64)
    x = philox4x32_10(q, r, zero, zero + np.uint64(TAG), seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(x, axis=2).reshape(R, 4 * nq)[:, :L]          # draw j = 4 q + word index
    site = ((words * np.uint64(L)) >> np.uint64(32)).astype(np.int64)
    W = np.zeros((R, L), dtype=np.int64)
    for k in range(R):
        W[k] = np.bincount(site[k], minlength=L)
    return W


def groups(moves):
    """[(v, indices of its moves)] in the order of the groups' first moves; equal v must be consecutive"""
    moves = np.asarray(moves).reshape(-1, 3)
    out = []
    for m, v in enumerate(moves[:, 0].tolist()):
        if out and out[-1][0] == v:
            out[-1][1].append(m)
        else:
            assert all(v != g[0] for g in out), "the moves are not grouped"
            out.append((v, [m]))
    return [(v, np.array(idx)) for v, idx in out]


def supports(moves, ll_moves, ll, R, seed, W=None):
    """(W: the weights, when the caller has them) -> dict(nodes [g], delta [m], delta_rep [m, R], alrt [g], sh_count [g], rell_count [g], sh_margin [g, R] =
    |-max delta - t^r|, rell_margin [g, R] = |max_G delta^r|, sh_win / rell_win [g, R] the decisions, fam_ll)"""
    ll = np.asarray(ll, dtype=np.float64)
    ll_moves = np.asarray(ll_moves, dtype=np.float64).reshape(-1, len(ll))
    L = len(ll)
    W = weights(L, R, seed) if W is None else W
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(ll)[None, :], ll_moves - ll[None, :], 0.0)
    delta = d.sum(axis=1)
    with np.errstate(invalid="ignore"):
        delta_rep = np.where(np.isfinite(d), d, 0.0) @ W.T.astype(np.float64)
    gs = groups(moves)
    G = len(gs)
    nodes = np.array([v for v, _ in gs], dtype=np.int64)
    alrt = np.full(G, np.nan)
    sh, rell = np.full(G, -1, dtype=np.int64), np.full(G, -1, dtype=np.int64)
    sh_margin, rell_margin = np.full((G, R), np.inf), np.full((G, R), np.inf)
    sh_win, rell_win = np.zeros((G, R), dtype=bool), np.zeros((G, R), dtype=bool)
    for g, (_, idx) in enumerate(gs):
        idx = idx[np.isfinite(delta[idx])]
        if len(idx) == 0:
            continue
        best = delta[idx].max()
        alrt[g] = -2.0 * best
        rep = delta_rep[idx]                                            # [|G|, R]
        centred = np.vstack([np.zeros((1, R)), rep - delta[idx][:, None]])
        top2 = np.sort(centred, axis=0)[-2:]
        t = top2[1] - top2[0]
        sh_win[g], rell_win[g] = -best > t, rep.max(axis=0) <= 0.0
        sh[g], rell[g] = int(sh_win[g].sum()), int(rell_win[g].sum())
        sh_margin[g] = np.abs(-best - t)
        rell_margin[g] = np.abs(rep.max(axis=0))
    return dict(nodes=nodes, delta=delta, delta_rep=delta_rep, alrt=alrt, sh_count=sh, rell_count=rell, sh_margin=sh_margin,
                rell_margin=rell_margin, sh_win=sh_win, rell_win=rell_win, fam_ll=float(ll.sum()))


def bounds(s, bar):
    """per edge the counts every computation within `bar` of the restatement's values must give: (sh_lo, sh_hi, rell_lo, rell_hi)
    -- the decided wins, and those plus the decisions whose margin is not above `bar` (an empty group: -1 four times)"""
    out = []
    for g in range(len(s["nodes"])):
        if s["sh_count"][g] < 0:
            out.append((-1, -1, -1, -1))
            continue
        und_sh, und_rell = s["sh_margin"][g] <= bar, s["rell_margin"][g] <= bar
        lo_sh, lo_rell = int(np.sum(s["sh_win"][g] & ~und_sh)), int(np.sum(s["rell_win"][g] & ~und_rell))
        out.append((lo_sh, lo_sh + int(und_sh.sum()), lo_rell, lo_rell + int(und_rell.sum())))
    return out


@functools.lru_cache(maxsize=None)
def restated(name, R=REPLICATES):
    """per family of the case the supports of the restated scan at the snapped input lengths, seeds family_seed(k)"""
    out = []
    for k, (_, mvs, ll_moves, ll) in enumerate(nni_cases.restated(name)):
        out.append(supports(mvs, ll_moves, ll, R, family_seed(k)))
    return out


def edge_in_tree(parent, true_parent):
    """per internal non-root node v of `parent` (ascending): is the leaf bipartition of the edge above v one of true_parent's"""
    parent = np.asarray(parent)
    ch = [[] for _ in parent]
    for v, p in enumerate(parent):
        if p >= 0:
            ch[int(p)].append(v)
    leaves = frozenset(v for v in range(len(parent)) if not ch[v])

    def below(v):
        return frozenset([v]) if not ch[v] else frozenset().union(*(below(w) for w in ch[v]))

    true = nni_reference.splits(true_parent)
    return {v: frozenset([below(v), leaves - below(v)]) in true for v in range(len(parent)) if parent[v] >= 0 and ch[v]}


@functools.lru_cache(maxsize=None)
def restated_search_family(R=REPLICATES, seed=1):
    """the simulated family of nni_cases on its START tree at its true indices -> (moves, supports, {v: the edge is a true one})"""
    f = nni_cases.search_family()
    Q, pi = bl_cases.model(20)
    mvs = nni_reference.moves(f["start_parent"])
    ll_moves, ll = nni_reference.scan(f["start_parent"], f["tau"], f["codes"], f["rates"], nni_cases.GRID, Q, pi, mvs)
    return mvs, supports(mvs, ll_moves, ll, R, seed), edge_in_tree(f["start_parent"], f["true_parent"])
