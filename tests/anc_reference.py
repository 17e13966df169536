"""A NumPy restatement of the marginal ancestral reconstruction (csrc/anc.hip.h): the log-space inside and
outside passes of bl_reference.py with P[tau_v][c] = expm(grid[tau_v] rate_c Q) on the edge above v, the outside message of a
LEAF (which those passes never form), and the posterior of the state at every node normalised by its own sum -- plus brute-force
enumeration of the states of ALL nodes for small trees.  It shares nothing with the library but the snapping rule."""
import itertools

import numpy as np
from scipy.special import logsumexp

from bl_reference import _children, _preorder, bank


def inside_outside(parent, tau, codes, rates, grid, Q, pi, P=None):
    """(L, U [n, sites, S] in log space, ll [sites]): L_w the inside part of node w (the sum of its children's messages; at a
    leaf 0 where the code is a gap or the state, else -inf), U_w the outside part (log pi at the root; below it
    log sum_a exp(x[a]) P_w[a][.], x = U_p + the siblings' messages, at internal nodes AND leaves)"""
    parent, tau, codes, rates = np.asarray(parent), np.asarray(tau), np.asarray(codes), np.asarray(rates, dtype=np.float64)
    cats = np.unique(rates)
    S, n, sites = Q.shape[0], len(parent), codes.shape[1]
    if P is None:
        P = bank(grid, cats, Q)
    root, ch, order = _preorder(parent)
    Lo, Uo, ll = np.zeros((n, sites, S)), np.zeros((n, sites, S)), np.zeros(sites)
    with np.errstate(divide="ignore", invalid="ignore"):
        logP, logpi = np.log(np.where(P > 0, P, 0.0)), np.log(pi)
        for c, r in enumerate(cats):
            units = np.flatnonzero(rates == r)
            L, msg, U = {}, {}, {}
            for v in order[::-1]:
                if ch[v]:
                    L[v] = sum(msg[w] for w in ch[v])
                else:
                    k = codes[v, units]
                    L[v] = np.where((k[:, None] < 0) | (k[:, None] == np.arange(S)[None, :]), 0.0, -np.inf)
                if v != root:
                    msg[v] = logsumexp(logP[tau[v], c][None, :, :] + L[v][:, None, :], axis=2)
            ll[units] = logsumexp(logpi[None, :] + L[root], axis=1)
            U[root] = np.broadcast_to(logpi, (len(units), S))
            for v in order[1:]:
                p = parent[v]
                X = U[p] + sum(msg[w] for w in ch[p] if w != v)
                U[v] = logsumexp(X[:, :, None] + logP[tau[v], c][None, :, :], axis=1)
            for v in range(n):
                Lo[v, units], Uo[v, units] = L[v], U[v]
    return Lo, Uo, ll


def posteriors(parent, tau, codes, rates, grid, Q, pi, P=None):
    """(post [n_nodes, sites, S], ll [sites]): post[w, u] = exp(z - logsumexp z), z = L_w + U_w; a site whose z is -inf at every
    state (ll = -inf) has post 0"""
    L, U, ll = inside_outside(parent, tau, codes, rates, grid, Q, pi, P)
    with np.errstate(invalid="ignore"):
        z = L + U
        norm = logsumexp(z, axis=2, keepdims=True)
        post = np.where(np.isfinite(norm), np.exp(z - np.where(np.isfinite(norm), norm, 0.0)), 0.0)
    return post, ll


def normaliser(parent, tau, codes, rates, grid, Q, pi):
    """logsumexp_a (L_w + U_w)[a] [n_nodes, sites]: the per-site log-likelihood, at every node"""
    L, U, _ = inside_outside(parent, tau, codes, rates, grid, Q, pi)
    return logsumexp(L + U, axis=2)


def states(post):
    """(state int [n, sites] = the first of equal maxima, -1 where post is 0 everywhere; confidence; margin = top - second)"""
    state = np.argmax(post, axis=2)
    top = np.sort(post, axis=2)
    conf = top[:, :, -1]
    return np.where(conf > 0, state, -1), conf, top[:, :, -1] - top[:, :, -2]


def brute_force(parent, tau, codes, rates, grid, Q, pi):
    """(post [n_nodes, sites, S], ll [sites]) by enumerating every assignment of states to ALL nodes, leaves included (small trees
    only): the weight of an assignment is pi[x_root] prod_v P_v[x_parent(v), x_v], and 0 where an observed leaf disagrees"""
    parent, tau, codes, rates = np.asarray(parent), np.asarray(tau), np.asarray(codes), np.asarray(rates, dtype=np.float64)
    cats = np.unique(rates)
    S, n, sites = Q.shape[0], len(parent), codes.shape[1]
    P = bank(grid, cats, Q)
    ch = _children(parent)
    root = int(np.flatnonzero(parent == -1)[0])
    X = np.array(list(itertools.product(range(S), repeat=n)), dtype=int)
    post, ll = np.zeros((n, sites, S)), np.zeros(sites)
    for u in range(sites):
        c = int(np.searchsorted(cats, rates[u]))
        w = pi[X[:, root]].copy()
        for v in range(n):
            if v != root:
                w *= P[tau[v], c][X[:, parent[v]], X[:, v]]
            if not ch[v] and codes[v, u] >= 0:
                w *= X[:, v] == int(codes[v, u])
        Z = w.sum()
        ll[u] = np.log(Z)
        for v in range(n):
            post[v, u] = np.bincount(X[:, v], weights=w, minlength=S) / Z
    return post, ll
