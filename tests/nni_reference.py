"""A NumPy restatement of the nearest-neighbour-interchange search (csrc/nni.hip.h, phylogeny_estimation/_nni.py; DESIGN.md
section 18): the enumeration of the moves, their application to a parent array, the scan formula from restated inside and
outside messages, the per-site log-likelihood of a tree by pruning (for the rearranged trees), the greedy selection, and the
search loop with its halving rule.  Every decision of the search records its margin.  It shares nothing with the package but the
branch-length restatement (bl_reference.py) it alternates with."""
import numpy as np
from scipy.special import logsumexp

import bl_reference
from em_reference import _children, _preorder


def moves(parent):
    """[n, 3] (v, c, s): v ascending over the internal non-root nodes, c over ch(v), s over ch(parent[v]) without v"""
    ch = _children(parent)
    out = []
    for v, p in enumerate(parent):
        if p < 0 or not ch[v]:
            continue
        for c in ch[v]:
            out += [(v, c, s) for s in ch[p] if s != v]
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def apply(parent, mvs):
    """the parent array after the moves (they must not share a node): parent[c] = parent[v], parent[s] = v"""
    parent = np.asarray(parent)
    new = parent.copy()
    seen = set()
    for v, c, s in np.asarray(mvs).reshape(-1, 3).tolist():
        p = int(parent[v])
        assert p >= 0 and parent[c] == v and s != v and parent[s] == p, (v, c, s)
        assert not seen & {p, v, c, s}, (v, c, s)
        seen |= {p, v, c, s}
        new[c], new[s] = p, v
    return new


def _log_bank(grid, rates, Q):
    P = bl_reference.bank(grid, np.unique(rates), Q)
    with np.errstate(divide="ignore"):
        return np.log(np.where(P > 0, P, 0.0))


def messages(parent, tau, codes, rates, grid, Q, pi, logP=None):
    """-> (msg [n, L, S] at the parent end of the edge above every node (the root's row unused), out [n, L, S] at every internal
    node: what is outside it (log pi at the root), ll [L]) at the indices tau"""
    parent, tau, codes, rates = np.asarray(parent), np.asarray(tau), np.asarray(codes), np.asarray(rates, dtype=np.float64)
    cats = np.unique(rates)
    S, n, L = Q.shape[0], len(parent), codes.shape[1]
    logP = _log_bank(grid, rates, Q) if logP is None else logP
    root, ch, order = _preorder(parent)
    msg, out, ll = np.zeros((n, L, S)), np.zeros((n, L, S)), np.zeros(L)
    with np.errstate(divide="ignore"):
        logpi = np.log(pi)
    for c, r in enumerate(cats):
        units = np.flatnonzero(rates == r)
        for v in order[::-1]:
            if ch[v]:
                d = sum(msg[w][units] for w in ch[v])
            else:
                k = codes[v, units]
                d = np.where((k[:, None] < 0) | (k[:, None] == np.arange(S)[None, :]), 0.0, -np.inf)
            if v == root:
                ll[units] = logsumexp(logpi[None, :] + d, axis=1)
            else:
                msg[v][units] = logsumexp(logP[tau[v], c][None, :, :] + d[:, None, :], axis=2)
        out[root][units] = logpi[None, :]
        for v in order[1:]:
            if not ch[v]:
                continue
            p = parent[v]
            x = out[p][units] + sum(msg[w][units] for w in ch[p] if w != v)
            out[v][units] = logsumexp(x[:, :, None] + logP[tau[v], c][None, :, :], axis=1)
    return msg, out, ll


def site_ll(parent, tau, codes, rates, grid, Q, pi, logP=None):
    """the per-site log-likelihood of the tree by pruning"""
    return messages(parent, tau, codes, rates, grid, Q, pi, logP)[2]


def scan(parent, tau, codes, rates, grid, Q, pi, mvs, logP=None):
    """-> (ll_moves [m, L] by the scan formula, ll [L] of the tree itself)"""
    parent, tau, rates = np.asarray(parent), np.asarray(tau), np.asarray(rates, dtype=np.float64)
    logP = _log_bank(grid, rates, Q) if logP is None else logP
    msg, out, ll = messages(parent, tau, codes, rates, grid, Q, pi, logP)
    ch = _children(parent)
    cat = np.searchsorted(np.unique(rates), rates)
    mvs = np.asarray(mvs).reshape(-1, 3)
    res = np.zeros((len(mvs), len(rates)))
    for m, (v, c, s) in enumerate(mvs.tolist()):
        p = parent[v]
        A = msg[s] + sum(msg[w] for w in ch[v] if w != c)                                     # [L, b]
        w = logsumexp(logP[tau[v], cat] + A[:, None, :], axis=2)                               # [L, a]
        B = out[p] + msg[c] + w + sum(msg[x] for x in ch[p] if x not in (v, s))
        res[m] = logsumexp(B, axis=1)
    return res, ll


def select(mvs, delta, parent, min_gain=0.0):
    """indices into mvs: by descending delta (ties: the lower index), delta > min_gain, no node {p, v, c, s} used twice"""
    mvs, delta = np.asarray(mvs).reshape(-1, 3), np.asarray(delta)
    order = sorted((m for m in range(len(mvs)) if delta[m] > min_gain), key=lambda m: (-delta[m], m))
    used, taken = set(), []
    for m in order:
        v, c, s = (int(x) for x in mvs[m])
        four = {int(parent[v]), v, c, s}
        if not used & four:
            used |= four
            taken.append(m)
    return np.array(taken, dtype=np.int64)


def _em(parent, tau, codes, rates, grid, Q, pi, P, num_rounds):
    """at most num_rounds rounds of the branch-length restatement -> (tau, the smallest relative argmax margin met)"""
    margin = np.inf
    for _ in range(num_rounds):
        r = bl_reference.em_round(parent, tau, codes, rates, grid, Q, pi, P=P)
        margin = min(margin, float(r["margin"][np.asarray(parent) >= 0].min()))
        if np.array_equal(r["tau"], tau):
            break
        tau = r["tau"]
    return tau, margin


def search(parent, tau, codes, rates, grid, Q, pi, num_nni_rounds, num_rounds):
    """The loop of ml_nni_trees on one family -> dict(parent, tau, final, rounds = [dict(before, scanned, selected = [moves],
    applied = [moves], after)], margin = the smallest margin of a decision relative to |log-likelihood| -- delta > 0, the order
    of two positive deltas, accept or reject --, em_margin = the smallest relative argmax margin of an EM round)."""
    parent, tau = np.asarray(parent).copy(), np.asarray(tau).copy()
    P = bl_reference.bank(grid, np.unique(rates), Q)
    with np.errstate(divide="ignore"):
        logP = np.log(np.where(P > 0, P, 0.0))
    rounds, margin, em_margin = [], np.inf, np.inf
    final, moved = None, True
    for _ in range(num_nni_rounds):
        tau, em = _em(parent, tau, codes, rates, grid, Q, pi, P, num_rounds)
        em_margin = min(em_margin, em)
        mvs = moves(parent)
        ll_moves, ll = scan(parent, tau, codes, rates, grid, Q, pi, mvs, logP)
        before = float(ll.sum())
        delta = (ll_moves - ll[None, :]).sum(axis=1)
        if len(delta):
            margin = min(margin, float(np.abs(delta).min()) / abs(before))
            pos = [m for m in range(len(mvs)) if delta[m] > 0]
            four = {m: {int(parent[mvs[m][0]])} | {int(x) for x in mvs[m]} for m in pos}
            for i, a in enumerate(pos):      # the order of two moves matters where they cannot both be taken
                for b in pos[i + 1:]:
                    if four[a] & four[b]:
                        margin = min(margin, abs(float(delta[a] - delta[b])) / abs(before))
        sel = mvs[select(mvs, delta, parent)]
        rec = dict(before=before, scanned=len(mvs), selected=sel.tolist(), applied=[], after=before)
        rounds.append(rec)
        moved = False
        while len(sel):
            cand = apply(parent, sel)
            after = float(site_ll(cand, tau, codes, rates, grid, Q, pi, logP).sum())
            margin = min(margin, abs(after - before) / abs(before))
            if after > before:
                parent, moved = cand, True
                rec.update(applied=sel.tolist(), after=after)
                break
            sel = sel[:len(sel) // 2]
        if not moved:
            final = before
            break
    if moved:
        tau, em = _em(parent, tau, codes, rates, grid, Q, pi, P, num_rounds)
        em_margin = min(em_margin, em)
        final = float(site_ll(parent, tau, codes, rates, grid, Q, pi, logP).sum())
    return dict(parent=parent, tau=tau, final=final, rounds=rounds, margin=margin, em_margin=em_margin)


def splits(parent):
    """the set of the tree's non-trivial leaf bipartitions (as frozensets of frozensets of leaf indices): the unrooted topology"""
    ch = _children(parent)
    leaves = frozenset(v for v in range(len(parent)) if not ch[v])
    below = {}
    root, _, order = _preorder(parent)
    for v in order[::-1]:
        below[v] = frozenset([v]) if not ch[v] else frozenset().union(*(below[w] for w in ch[v]))
    out = set()
    for v in range(len(parent)):
        a = below[v]
        if 1 < len(a) < len(leaves) - 1:
            out.add(frozenset([a, leaves - a]))
    return out
