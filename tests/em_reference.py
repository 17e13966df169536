"""A NumPy restatement of the EM E-step (csrc/em.hip.h): forward-backward on the quantised tree, in
log space, vectorised over the sites of one rate category, plus brute-force enumeration of the internal states for small
trees.  It shares nothing with the library but the quantisation rule."""
import itertools

import numpy as np
from scipy.linalg import expm
from scipy.special import logsumexp


def quantize(t, grid):
    """the reference's nearest-point rule (cherryml/utils.py:35-56), clamped to the grid's ends"""
    grid = np.asarray(grid, dtype=np.float64)
    if not t > grid[0]:
        return 0
    if t >= grid[-1]:
        return len(grid) - 1
    lo = int(np.searchsorted(grid, t, side="left"))
    return lo - 1 if t / grid[lo - 1] - 1.0 < grid[lo] / t - 1.0 else lo


def _children(parent):
    ch = [[] for _ in parent]
    for v, p in enumerate(parent):
        if p >= 0:
            ch[p].append(v)
    return ch


def _preorder(parent):
    ch = _children(parent)
    root = int(np.flatnonzero(np.asarray(parent) == -1)[0])
    order, stack = [], [root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(ch[v][::-1])
    return root, ch, order


def estep(parent, length, codes, rates, grid, Q, pi):
    """-> (E [B, S, S], per-site log-likelihood).  parent[v] (-1 at the root), length[v] (edge into v), codes [n_nodes, L]
    (-1 = gap; leaf rows only are read), rates [L]."""
    parent, codes, rates = np.asarray(parent), np.asarray(codes), np.asarray(rates, dtype=np.float64)
    S, B = Q.shape[0], len(grid)
    P = np.array([expm(t * Q) for t in grid])
    E = np.zeros((B, S, S))
    ll = np.zeros(codes.shape[1])
    root, ch, order = _preorder(parent)
    with np.errstate(divide="ignore"):
        logP, logpi = np.log(P), np.log(pi)
        for r in np.unique(rates):
            units = np.flatnonzero(rates == r)
            q = {v: quantize(length[v] * r, grid) for v in range(len(parent)) if v != root}
            L, msg = {}, {}
            for v in order[::-1]:   # inside
                if ch[v]:
                    L[v] = sum(msg[c] for c in ch[v])
                else:
                    c = codes[v, units]
                    L[v] = np.where((c[:, None] < 0) | (c[:, None] == np.arange(S)[None, :]), 0.0, -np.inf)
                if v != root:
                    msg[v] = logsumexp(logP[q[v]][None, :, :] + L[v][:, None, :], axis=2)
            lu = logsumexp(logpi[None, :] + L[root], axis=1)
            ll[units] = lu
            Uo = {root: np.broadcast_to(logpi, (len(units), S))}
            for v in order[1:]:     # outside
                p = parent[v]
                X = Uo[p] + sum(msg[c] for c in ch[p] if c != v)
                if ch[v]:
                    Uo[v] = logsumexp(X[:, :, None] + logP[q[v]][None, :, :], axis=1)
                post = np.exp(X[:, :, None] + logP[q[v]][None, :, :] + L[v][:, None, :] - lu[:, None, None])
                E[q[v]] += post.sum(axis=0)
    return E, ll


def estep_brute_force(parent, length, codes, rates, grid, Q, pi):
    """the same by enumerating every assignment of states to the INTERNAL nodes (small trees only); a leaf contributes
    sum_{b observed} P[x_parent, b], and its edge's pair posterior is split over b in proportion to P[x_parent, b]"""
    parent, codes = np.asarray(parent), np.asarray(codes)
    S, B = Q.shape[0], len(grid)
    P = np.array([expm(t * Q) for t in grid])
    n = len(parent)
    ch = _children(parent)
    root = int(np.flatnonzero(parent == -1)[0])
    internal = [v for v in range(n) if ch[v]]
    col = {v: k for k, v in enumerate(internal)}
    X = np.array(list(itertools.product(range(S), repeat=len(internal))), dtype=int)   # [K, n_internal]
    E = np.zeros((B, S, S))
    ll = np.zeros(codes.shape[1])
    for u in range(codes.shape[1]):
        q = {v: quantize(length[v] * rates[u], grid) for v in range(n) if v != root}
        obs = {v: (np.ones(S) if codes[v, u] < 0 else np.eye(S)[int(codes[v, u])]) for v in range(n) if not ch[v]}
        f = {v: P[q[v]] @ obs[v] for v in obs}
        w = pi[X[:, col[root]]].copy()
        for v in range(n):
            if v == root:
                continue
            xp = X[:, col[parent[v]]]
            w *= P[q[v]][xp, X[:, col[v]]] if ch[v] else f[v][xp]
        Z = w.sum()
        ll[u] = np.log(Z)
        for v in range(n):
            if v == root:
                continue
            xp = X[:, col[parent[v]]]
            if ch[v]:
                np.add.at(E[q[v]], (xp, X[:, col[v]]), w / Z)
            else:
                g = np.bincount(xp, weights=w / Z, minlength=S) / f[v]
                E[q[v]] += g[:, None] * P[q[v]] * obs[v][None, :]
    return E, ll
