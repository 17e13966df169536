"""A NumPy restatement of the transfer distances on the device (include/cherrybank.h, cb_transfer_support),
no GPU and nothing of `_bootstrap.py`'s packed sets: leaf sets are boolean rows built from the join records, a Hamming distance
is a count of unequal entries, and everything is integers.

    leaf_sets(n, join_nodes)                      bool [n - 3, n]: the leaf set of the node every join makes
    distances(ref, n, join_nodes)                 dict: raw [n_ref, B] = min_q min(h, n - h), min_dist = min(raw, p - 1), sum_dist,
                                                  present, p
    supports(sum_dist, present, p, B)             (bootstrap, transfer) as the issue's formulas state them

and the trees the tests feed both sides: unrooted binary trees as adjacency dicts (leaves 0 .. n - 1, internal nodes from n),
random ones, ones with a few leaves re-attached elsewhere, and their join records (a rooted postorder: every internal node but
the root joins its two children; the root's three children are the final nodes)."""
import numpy as np

# every case of tests/test_gpu_transfer.py, (n, n_ref, n_rep): `make_case` builds it.  Each holds exact matches, clamped values
# and, from eight leaves on, minima below the clamp (p = 2 for every split of four or five leaves: delta is 0 or 1 there)
CASES = [(4, 1, 3), (5, 2, 3), (8, 5, 6), (31, 28, 4), (32, 29, 3), (33, 30, 70), (63, 60, 3), (64, 61, 1), (65, 62, 17),
         (257, 65, 3), (1030, 7, 3), (2100, 5, 2)]


# bootstrap = k / B and transfer = 1 - s / (B (p - 1)) are each within 2^-54 per rounding of numbers that satisfy
# bootstrap <= transfer exactly: 3 x 2^-54 < 2^-52 (with p = 2 they are k / B and 1 - (B - k) / B: equal, one ulp apart as floats)
CHAIN_SLACK = 2.0 ** -52


def leaf_sets(n, join_nodes):
    join_nodes = np.asarray(join_nodes).reshape(-1, 2)
    assert len(join_nodes) == n - 3
    sets = np.zeros((n + len(join_nodes), n), dtype=bool)
    sets[np.arange(n), np.arange(n)] = True
    for q, (u, v) in enumerate(join_nodes):
        assert 0 <= u < n + q and 0 <= v < n + q and u != v
        sets[n + q] = sets[u] | sets[v]
    return sets[n:]


def distances(ref, n, join_nodes, block=8):
    """ref: bool [n_ref, n], one side of every reference split; join_nodes [B, n - 3, 2]"""
    ref = np.asarray(ref, dtype=bool)
    join_nodes = np.asarray(join_nodes)
    n_ref, B = len(ref), len(join_nodes)
    size = ref.sum(axis=1).astype(np.int64)
    p = np.minimum(size, n - size)
    assert np.all(p >= 2)
    raw = np.zeros((n_ref, B), dtype=np.int64)
    for b in range(B):
        S = leaf_sets(n, join_nodes[b])
        for r0 in range(0, n_ref, block):                      # (a block of reference rows at a time: memory)
            h = (ref[r0:r0 + block, None, :] != S[None, :, :]).sum(axis=2).astype(np.int64)
            raw[r0:r0 + block, b] = np.minimum(h, n - h).min(axis=1)
    min_dist = np.minimum(raw, (p - 1)[:, None])
    return dict(raw=raw, min_dist=min_dist.astype(np.int32), sum_dist=min_dist.sum(axis=1).astype(np.int64),
                present=(min_dist == 0).sum(axis=1).astype(np.int32), p=p)


def supports(sum_dist, present, p, B):
    bootstrap = np.array([int(k) / B for k in present], dtype=np.float64)
    transfer = np.array([1.0 - int(s) / (B * (int(q) - 1)) for s, q in zip(sum_dist, p)], dtype=np.float64)
    return bootstrap, transfer


# ------------------------------------------------------------------------------------------------ trees
def random_topology(n, rng):
    """a uniformly grown unrooted binary tree on the leaves 0 .. n - 1 (n >= 3): {node: set of neighbours}"""
    adj = {0: {n}, 1: {n}, 2: {n}, n: {0, 1, 2}}
    edges = [(0, n), (1, n), (2, n)]
    for k in range(3, n):
        e, mid = rng.integers(len(edges)), n + k - 2
        u, v = edges[e]
        _attach(adj, k, u, v, mid)
        edges[e] = (u, mid)
        edges += [(mid, v), (mid, k)]
    return adj


def _attach(adj, leaf, u, v, mid):
    adj[u].remove(v)
    adj[v].remove(u)
    adj[mid] = {u, v, leaf}
    adj[u].add(mid)
    adj[v].add(mid)
    adj[leaf] = {mid}


def move_leaves(adj, leaves, rng):
    """a copy of the tree with every leaf of `leaves` cut off and attached to a random edge of what is left"""
    adj = {u: set(vs) for u, vs in adj.items()}
    for leaf in leaves:
        (mid,) = adj[leaf]
        x, y = sorted(adj[mid] - {leaf})
        del adj[mid], adj[leaf]
        adj[x].remove(mid)
        adj[y].remove(mid)
        adj[x].add(y)
        adj[y].add(x)
        edges = [(u, v) for u in sorted(adj) for v in sorted(adj[u]) if u < v]
        u, v = edges[rng.integers(len(edges))]
        _attach(adj, leaf, u, v, mid)
    return adj


def final_nodes(n, join_nodes):
    """the three nodes no join takes: what is left active after the last join"""
    left = np.setdiff1d(np.arange(2 * n - 3), np.asarray(join_nodes).ravel())
    assert len(left) == 3
    return left.astype(np.int32)


KINDS = ("moved", "random", "copy")


def make_case(n, n_ref, n_rep, seed=0):
    """(ref bool [n_ref, n], join_nodes int32 [n_rep, n - 3, 2]) of a random reference tree: its n_ref reference sets are the
    deepest and the shallowest of its n - 3 non-trivial splits, half and half, each given on a random side; replicate b is of
    kind KINDS[b % 3] -- the reference with one leaf (n > 16: three leaves) re-attached elsewhere, an independent random tree, a
    copy of the reference -- with its own root and member order, so no two records of one tree look alike"""
    rng = np.random.default_rng(1000003 * seed + 1009 * n + 17 * n_ref + n_rep)
    tree = random_topology(n, rng)
    sets = leaf_sets(n, join_records(tree, n, rng))
    size = sets.sum(axis=1)
    order = np.argsort(-np.minimum(size, n - size), kind="stable")
    deep = (n_ref + 1) // 2
    ref = sets[np.concatenate([order[:deep], order[len(order) - (n_ref - deep):]])]
    assert len(ref) == n_ref <= n - 3
    ref = np.where(rng.integers(0, 2, n_ref).astype(bool)[:, None], ~ref, ref)
    reps = []
    for b in range(n_rep):
        kind = KINDS[b % 3]
        if kind == "moved":
            other = move_leaves(tree, rng.choice(n, 3 if n > 16 else 1, replace=False).tolist(), rng)
        else:
            other = random_topology(n, rng) if kind == "random" else tree
        reps.append(join_records(other, n, rng))
    return ref, np.stack(reps)


def join_records(adj, n, rng):
    """join_nodes int32 [n - 3, 2] of the tree, rooted at a random internal node: the children before their parent"""
    inner = sorted(u for u in adj if u >= n)
    root = inner[rng.integers(len(inner))]
    order, stack, parent = [], [root], {root: None}
    while stack:
        u = stack.pop()
        order.append(u)
        for v in sorted(adj[u]):
            if v != parent[u]:
                parent[v] = u
                stack.append(v)
    ident = {u: u for u in adj if u < n}
    joins = []
    for u in reversed(order):
        if u >= n and u != root:
            a, b = [ident[v] for v in sorted(adj[u]) if v != parent[u]]
            if rng.integers(2):
                a, b = b, a
            ident[u] = n + len(joins)
            joins.append((a, b))
    assert len(joins) == n - 3
    return np.array(joins, dtype=np.int32).reshape(n - 3, 2)
