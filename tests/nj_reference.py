"""What the neighbour-joining tests share (no GPU, NumPy only): random unrooted trees and their path-length matrices, the splits
of a tree, sequences evolved down a tree, a log-transition bank by eigendecomposition, and the NumPy restatement of the
branch-length bisection (branch_length_estimation.cpp:60-103; oracle/ble_oracle.py:get_branch_lengths) for all pairs of
sequences, which also records how close every pair came to a tie."""
import numpy as np


def random_tree(n, rng, length=lambda rng: rng.uniform(0.05, 1.0)):
    """A random unrooted binary tree on the leaves 0 .. n-1 (internal nodes n ..) as {node: {neighbour: length}}: every new
    leaf splits a uniformly chosen edge.  n = 2: one edge."""
    adj = {}

    def add(u, v, t):
        adj.setdefault(u, {})[v] = t
        adj.setdefault(v, {})[u] = t

    if n == 2:
        add(0, 1, length(rng))
        return adj
    nxt = n
    for leaf in range(3):
        add(leaf, nxt, length(rng))
    for leaf in range(3, n):
        nxt += 1
        edges = sorted((u, v) for u in adj for v in adj[u] if u < v)
        u, v = edges[int(rng.integers(len(edges)))]
        del adj[u][v], adj[v][u]
        add(u, nxt, length(rng))
        add(nxt, v, length(rng))
        add(nxt, leaf, length(rng))
    return adj


def adjacency(tree):
    """{node: {neighbour: length}} of a cherryml_amd.io.Tree"""
    adj = {}
    for u, v, t in tree.edges():
        adj.setdefault(u, {})[v] = t
        adj.setdefault(v, {})[u] = t
    return adj


def path_lengths(adj, leaves):
    """[len(leaves)]^2 leaf-to-leaf path lengths"""
    D = np.zeros((len(leaves), len(leaves)))
    for i, s in enumerate(leaves):
        dist, stack = {s: 0.0}, [s]
        while stack:
            u = stack.pop()
            for v, t in adj[u].items():
                if v not in dist:
                    dist[v] = dist[u] + t
                    stack.append(v)
        D[i] = [dist[v] for v in leaves]
    return D


def splits(adj, leaves):
    """the non-trivial bipartitions of `leaves` by the edges of the tree, each as the frozenset of the side without leaves[0]"""
    leaves, out = list(leaves), set()
    for u in adj:
        for v in adj[u]:
            side, stack = {v}, [v]                    # what lies behind the edge u -> v
            while stack:
                a = stack.pop()
                for b in adj[a]:
                    if b != u and b not in side:
                        side.add(b)
                        stack.append(b)
            part = frozenset(x for x in leaves if x in side)
            if leaves[0] in part:
                part = frozenset(leaves) - part
            if 1 < len(part) < len(leaves) - 1:
                out.add(part)
    return out


def stationary(Q):
    w, v = np.linalg.eig(Q.T)
    pi = np.real(v[:, np.argmin(np.abs(w))])
    return pi / pi.sum()


def transition_matrices(Q, times):
    """expm(t Q) for a reversible Q by the symmetric eigendecomposition: [len(times), S, S]"""
    pi = stationary(Q)
    d = np.sqrt(pi)
    lam, U = np.linalg.eigh(d[:, None] * Q / d[None, :])
    P = np.einsum("ik,tk,jk->tij", U, np.exp(np.multiply.outer(np.asarray(times, dtype=np.float64), lam)), U)
    return np.maximum(P / d[None, :, None] * d[None, None, :], 1e-300)


def log_bank(Q, grid, rates):
    """log expm(grid[t] rates[r] Q): [T, R, S, S]"""
    S = Q.shape[0]
    tt = np.multiply.outer(np.asarray(grid, dtype=np.float64), np.asarray(rates, dtype=np.float64))
    return np.log(transition_matrices(Q, tt.reshape(-1))).reshape(len(grid), len(rates), S, S)


def evolve(adj, n_leaves, Q, site_rates, rng):
    """sequences [n_leaves, L] evolved from the stationary distribution down the tree `adj` (leaves 0 .. n_leaves-1), site s at
    rate site_rates[s]"""
    site_rates = np.asarray(site_rates, dtype=np.float64)
    S, L = Q.shape[0], len(site_rates)
    pi = stationary(Q)
    root = max(adj)
    state = {root: rng.choice(S, size=L, p=pi / pi.sum())}
    stack = [root]
    while stack:
        u = stack.pop()
        for v, t in adj[u].items():
            if v in state:
                continue
            cats, inv = np.unique(site_rates, return_inverse=True)
            P = transition_matrices(Q, t * cats)
            cdf = np.cumsum(P[inv, state[u], :], axis=1)
            state[v] = np.minimum((rng.random(L)[:, None] * cdf[:, -1:] > cdf).sum(axis=1), S - 1)
            stack.append(v)
    return np.stack([state[i] for i in range(n_leaves)]).astype(np.int8)


def pairwise_bisection(seqs, logP, site_to_rate):
    """The reference's bisection for all pairs i < j of seqs [n, L] (-1 = gap): compare mid against mid + 1 over the sites where
    both sequences are observed with sum logP[t][rate(site)][x][y] + logP[t][rate(site)][y][x]; `a > b` keeps the lower half.
    Returns (index [n, n] int32, symmetric, -1 on the diagonal; margin [n, n]: the smallest |a - b| / max(|a|, |b|) a pair met on
    its way, inf where both sums were 0 at every step -- `0 > 0` is false, nothing to decide)."""
    seqs = np.asarray(seqs).astype(np.int64)
    n, L = seqs.shape
    T = logP.shape[0]
    sym = logP + logP.transpose(0, 1, 3, 2)
    I, J = np.triu_indices(n, 1)
    X, Y = seqs[I], seqs[J]
    ok = (X >= 0) & (Y >= 0)
    X, Y = np.where(ok, X, 0), np.where(ok, Y, 0)
    rate = np.broadcast_to(np.asarray(site_to_rate, dtype=np.int64)[None, :], X.shape)
    low, high = np.zeros(len(I), dtype=np.int64), np.full(len(I), T - 1, dtype=np.int64)
    margin = np.full(len(I), np.inf)
    while np.any(low < high):
        live = low < high
        mid = np.where(live, low + (high - low) // 2, 0)
        a = np.where(ok, sym[mid[:, None], rate, X, Y], 0.0).sum(axis=1)
        b = np.where(ok, sym[np.minimum(mid + 1, T - 1)[:, None], rate, X, Y], 0.0).sum(axis=1)
        scale = np.maximum(np.abs(a), np.abs(b))
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(scale > 0, np.abs(a - b) / scale, np.inf)
        margin = np.where(live, np.minimum(margin, rel), margin)
        lower = a > b
        high = np.where(live & lower, mid, high)
        low = np.where(live & ~lower, mid + 1, low)
    index = np.full((n, n), -1, dtype=np.int32)
    index[I, J] = index[J, I] = low
    m = np.full((n, n), np.inf)
    m[I, J] = m[J, I] = margin
    return index, m
