"""A NumPy restatement of one round of the branch-length EM (csrc/bl.hip.h): the inside and outside
passes in log space with P[tau_v][c] = expm(grid[tau_v] rate_c Q) on the edge above v, the per-(edge, category) expected counts
E_vc, the score of EVERY grid point and its argmax (the lowest index among exact maxima), plus brute-force enumeration of the
internal states for small trees.  Per edge it records the relative margin (best - second) / |best| of the scores.  It shares
nothing with the library but the snapping rule."""
import itertools

import numpy as np
from scipy.linalg import expm
from scipy.special import logsumexp

from em_reference import _children, _preorder, quantize


def snap(length, parent, grid):
    """the grid index of every input length (the reference's nearest-point rule, clamped to the grid's ends); the root: -1"""
    return np.array([-1 if p < 0 else quantize(t, grid) for t, p in zip(length, parent)], dtype=np.int64)


def bank(grid, cats, Q):
    """P [T, R, S, S] = expm(grid[tau] * cats[c] * Q)"""
    return np.array([[expm(t * r * Q) for r in cats] for t in grid])


def em_round(parent, tau, codes, rates, grid, Q, pi, P=None):
    """One round from the indices `tau` -> dict(tau = the new indices, ll = per-site log-likelihood at the OLD indices,
    E = {(v, c): [S, S]}, scores [n_nodes, T], margin [n_nodes] (inf at the root)).  codes [n_nodes, L] (-1 = gap; leaf rows only
    are read), rates [L] > 0; category c = the c-th distinct rate."""
    parent, tau, codes, rates = np.asarray(parent), np.asarray(tau), np.asarray(codes), np.asarray(rates, dtype=np.float64)
    cats = np.unique(rates)
    S, T, n = Q.shape[0], len(grid), len(parent)
    if P is None:
        P = bank(grid, cats, Q)
    root, ch, order = _preorder(parent)
    ll = np.zeros(codes.shape[1])
    E, scores = {}, np.zeros((n, T))
    with np.errstate(divide="ignore", invalid="ignore"):
        logP, logpi = np.log(np.where(P > 0, P, 0.0)), np.log(pi)
        for c, r in enumerate(cats):
            units = np.flatnonzero(rates == r)
            L, msg = {}, {}
            for v in order[::-1]:   # inside
                if ch[v]:
                    L[v] = sum(msg[w] for w in ch[v])
                else:
                    k = codes[v, units]
                    L[v] = np.where((k[:, None] < 0) | (k[:, None] == np.arange(S)[None, :]), 0.0, -np.inf)
                if v != root:
                    msg[v] = logsumexp(logP[tau[v], c][None, :, :] + L[v][:, None, :], axis=2)
            lu = logsumexp(logpi[None, :] + L[root], axis=1)
            ll[units] = lu
            Uo = {root: np.broadcast_to(logpi, (len(units), S))}
            for v in order[1:]:     # outside
                p = parent[v]
                X = Uo[p] + sum(msg[w] for w in ch[p] if w != v)
                if ch[v]:
                    Uo[v] = logsumexp(X[:, :, None] + logP[tau[v], c][None, :, :], axis=1)
                e = np.exp(X[:, :, None] + logP[tau[v], c][None, :, :] + L[v][:, None, :] - lu[:, None, None]).sum(axis=0)
                E[(v, c)] = e
                # a term with E = 0 contributes 0, even where log P = -inf
                scores[v] += np.where(e[None] > 0, e[None] * np.where(e[None] > 0, logP[:, c], 0.0), 0.0).sum(axis=(1, 2))
    new = np.array(tau).copy()
    margin = np.full(n, np.inf)
    for v in range(n):
        if v == root:
            continue
        new[v] = int(np.argmax(scores[v]))   # the first of equal maxima
        top = np.sort(scores[v])[-2:]
        margin[v] = (top[1] - top[0]) / abs(top[1])
    return dict(tau=new, ll=ll, E=E, scores=scores, margin=margin)


def brute_force(parent, tau, codes, rates, grid, Q, pi):
    """(E = {(v, c): [S, S]}, per-site log-likelihood) by enumerating every assignment of states to the INTERNAL nodes (small
    trees only); a leaf contributes sum_{b observed} P[x_parent, b], and its edge's pair posterior is split over b in proportion
    to P[x_parent, b]"""
    parent, tau, codes, rates = np.asarray(parent), np.asarray(tau), np.asarray(codes), np.asarray(rates, dtype=np.float64)
    cats = np.unique(rates)
    S, n = Q.shape[0], len(parent)
    P = bank(grid, cats, Q)
    ch = _children(parent)
    root = int(np.flatnonzero(parent == -1)[0])
    internal = [v for v in range(n) if ch[v]]
    col = {v: k for k, v in enumerate(internal)}
    X = np.array(list(itertools.product(range(S), repeat=len(internal))), dtype=int)
    E = {(v, c): np.zeros((S, S)) for v in range(n) if v != root for c in range(len(cats))}
    ll = np.zeros(codes.shape[1])
    for u in range(codes.shape[1]):
        c = int(np.searchsorted(cats, rates[u]))
        Pv = {v: P[tau[v], c] for v in range(n) if v != root}
        obs = {v: (np.ones(S) if codes[v, u] < 0 else np.eye(S)[int(codes[v, u])]) for v in range(n) if not ch[v]}
        f = {v: Pv[v] @ obs[v] for v in obs}
        w = pi[X[:, col[root]]].copy()
        for v in range(n):
            if v == root:
                continue
            xp = X[:, col[parent[v]]]
            w *= Pv[v][xp, X[:, col[v]]] if ch[v] else f[v][xp]
        Z = w.sum()
        ll[u] = np.log(Z)
        for v in range(n):
            if v == root:
                continue
            xp = X[:, col[parent[v]]]
            if ch[v]:
                np.add.at(E[(v, c)], (xp, X[:, col[v]]), w / Z)
            else:
                g = np.bincount(xp, weights=w / Z, minlength=S) / f[v]
                E[(v, c)] += g[:, None] * Pv[v] * obs[v][None, :]
    return E, ll
