"""A NumPy restatement of the site-rate scan (csrc/sr.hip.h): log-space pruning of every site at every
candidate rate with expm(length_v cands[c] Q) on the edge above v, the pick rule (the highest log-likelihood; among exact maxima
`current` if it is one of them, else the lowest index), the fewer-than-two-observed-leaves rule (decided from the codes: keep
`current`, or candidate 0), a per-site margin (best - second) / |best|, brute-force enumeration of the internal states for
small trees, and the alternating stage restated with bl_reference's round.  It shares nothing with the library."""
import itertools

import numpy as np
from scipy.linalg import expm
from scipy.special import logsumexp

import bl_reference
from em_reference import _children, _preorder


def site_ll(parent, length, codes, rate, Q, pi):
    """the log-likelihood [L] of every site at ONE rate (pruning in log space)"""
    parent, codes = np.asarray(parent), np.asarray(codes)
    S = Q.shape[0]
    root, ch, order = _preorder(parent)
    with np.errstate(divide="ignore"):
        logpi = np.log(pi)
        L, msg = {}, {}
        for v in order[::-1]:
            if ch[v]:
                L[v] = sum(msg[w] for w in ch[v])
            else:
                k = codes[v]
                L[v] = np.where((k[:, None] < 0) | (k[:, None] == np.arange(S)[None, :]), 0.0, -np.inf)
            if v != root:
                P = expm(float(length[v]) * float(rate) * Q)
                logP = np.log(np.where(P > 0, P, 0.0))
                msg[v] = logsumexp(logP[None, :, :] + L[v][:, None, :], axis=2)
        return logsumexp(logpi[None, :] + L[root], axis=1)


def observed_leaves(parent, codes):
    """[L] the number of leaves with an observed state at every site"""
    ch = _children(np.asarray(parent))
    leaves = [v for v in range(len(parent)) if not ch[v]]
    return (np.asarray(codes)[leaves] >= 0).sum(axis=0)


def pick(ll, n_obs, current=None):
    """ll [C, L] -> (best [L], margin [L]): margin = inf for a single candidate and for the sites the codes decide"""
    C, L = ll.shape
    cur = np.full(L, -1, dtype=np.int64) if current is None else np.asarray(current, dtype=np.int64)
    best, margin = np.zeros(L, dtype=np.int64), np.full(L, np.inf)
    for u in range(L):
        if n_obs[u] < 2:
            best[u] = cur[u] if cur[u] >= 0 else 0
            continue
        top = ll[:, u].max()
        best[u] = cur[u] if cur[u] >= 0 and ll[cur[u], u] == top else int(np.argmax(ll[:, u]))   # argmax: the first maximum
        if C > 1 and np.isfinite(top):
            two = np.sort(ll[:, u])[-2:]
            margin[u] = (two[1] - two[0]) / abs(two[1])
        elif C > 1:
            margin[u] = 0.0      # every candidate at -inf: a tie
    return best, margin


def scan(parent, length, codes, cands, Q, pi, current=None):
    """-> dict(ll [C, L], best [L], best_ll [L], margin [L], n_obs [L])"""
    ll = np.array([site_ll(parent, length, codes, r, Q, pi) for r in cands])
    n_obs = observed_leaves(parent, codes)
    best, margin = pick(ll, n_obs, current)
    return dict(ll=ll, best=best, best_ll=ll[best, np.arange(ll.shape[1])], margin=margin, n_obs=n_obs)


def brute_force(parent, length, codes, rate, Q, pi):
    """the same log-likelihood [L] by enumerating every assignment of states to the INTERNAL nodes (small trees only)"""
    parent, codes = np.asarray(parent), np.asarray(codes)
    S, n = Q.shape[0], len(parent)
    ch = _children(parent)
    root = int(np.flatnonzero(parent == -1)[0])
    internal = [v for v in range(n) if ch[v]]
    col = {v: k for k, v in enumerate(internal)}
    X = np.array(list(itertools.product(range(S), repeat=len(internal))), dtype=int)
    P = {v: expm(float(length[v]) * float(rate) * Q) for v in range(n) if v != root}
    ll = np.zeros(codes.shape[1])
    for u in range(codes.shape[1]):
        w = pi[X[:, col[root]]].copy()
        for v in range(n):
            if v == root:
                continue
            xp = X[:, col[parent[v]]]
            if ch[v]:
                w *= P[v][xp, X[:, col[v]]]
            else:
                obs = np.ones(S) if codes[v, u] < 0 else np.eye(S)[int(codes[v, u])]
                w *= (P[v] @ obs)[xp]
        ll[u] = np.log(w.sum())
    return ll


def alternate(parent, tau, codes, index, cands, grid, Q, pi, n_outer, n_rounds):
    """the alternating stage restated: per outer iteration at most `n_rounds` rounds of bl_reference.em_round at the rates
    cands[index], then the pick at the lengths grid[tau] with `index` as current; stops when an outer iteration changes nothing.
    -> (tau, index, trace): trace holds, in order, the family log-likelihoods the stage meets (per outer iteration: at the start
    of the length fit, before the pick and after it); n_rounds >= 1"""
    parent, tau, index, cands, grid = np.asarray(parent), np.array(tau), np.array(index), np.asarray(cands), np.asarray(grid)
    trace = []
    for _ in range(n_outer):
        moved = 0
        rates = cands[index]
        for k in range(n_rounds):
            r = bl_reference.em_round(parent, tau, codes, rates, grid, Q, pi)
            if k == 0:
                trace.append(r["ll"].sum())
            changed = int((r["tau"] != tau).sum())
            moved += changed
            tau = r["tau"]
            if changed == 0:
                break
        length = np.where(tau >= 0, grid[np.maximum(tau, 0)], 0.0)
        s = scan(parent, length, codes, cands, Q, pi, current=index)
        trace += [s["ll"][index, np.arange(len(index))].sum(), s["best_ll"].sum()]   # (before the pick = the end of the length fit)
        moved += int((s["best"] != index).sum())
        index = s["best"]
        if moved == 0:
            break
    return tau, index, trace
