"""A NumPy restatement of Felsenstein's bootstrap on the device (include/cherrybank.h, cb_boot_nj), no GPU:

* `weights`: the site multiplicities -- draw j of replicate b takes word j & 3 of philox4x32_10(counter = (j >> 2, b, 0, TAG),
  key = (seed low word, seed high word)) and lands on site (word * L) >> 32; W[b][s] counts the draws of site s;
* `weighted_bisection`: nj_reference.pairwise_bisection with every site's term multiplied by its weight, per replicate, with the
  same per-entry margin (the smallest |a - b| / max(|a|, |b|) met on the way, inf where both sums were 0 at every step);
* `supports`: the four steps chained -- weights, weighted bisection, njd_reference.join (the device's order of the row sums) on
  D = grid[index] with a zero diagonal, and the splits of every replicate's tree by nj_reference.splits on its edges -- against the
  splits of the edges above the internal non-root nodes of a given tree.

It shares sim_stream.philox4x32_10, nj_reference and njd_reference with the other tests and nothing with the package."""
import numpy as np

import nj_reference as ref
import njd_reference as njd
from sim_stream import philox4x32_10

TAG = 0x424F4F54

# Philox4x32-10 known answers (Random123, kat_vectors): (counter, key, output)
PHILOX_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def draws(L, B, seed, tag=TAG, rep0=0):
    """int64 [B, L]: the site every draw lands on, replicates rep0 .. rep0 + B - 1"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (L + 3) // 4
    q = np.broadcast_to(np.arange(nq, dtype=np.uint64)[None, :], (B, nq))
    r = np.broadcast_to(np.arange(rep0, rep0 + B, dtype=np.uint64)[:, None], (B, nq))
    zero = np.zeros((B, nq), dtype=np.uint64)
    x = philox4x32_10(q, r, zero, zero + np.uint64(tag), seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(x, axis=2).reshape(B, 4 * nq)[:, :L]              # draw j = 4 q + word index
    return ((words * np.uint64(L)) >> np.uint64(32)).astype(np.int64)


def weights(L, B, seed, tag=TAG, rep0=0):
    """int64 [B, L]: how often each site (the caller's order) is drawn in each replicate"""
    site = draws(L, B, seed, tag, rep0)
    W = np.zeros((B, L), dtype=np.int64)
    for k in range(B):
        W[k] = np.bincount(site[k], minlength=L)
    return W


def weighted_bisection(seqs, logP, site_to_rate, W):
    """nj_reference.pairwise_bisection with the weights W [B, L]: (index [B, n, n] int32, symmetric, -1 on the diagonal;
    margin [B, n, n]).  W = 1 gives pairwise_bisection's sums in its order (a product with 1.0 is exact)."""
    seqs = np.asarray(seqs).astype(np.int64)
    W = np.asarray(W, dtype=np.float64)
    n, L = seqs.shape
    B, T = W.shape[0], logP.shape[0]
    sym = logP + logP.transpose(0, 1, 3, 2)
    I, J = np.triu_indices(n, 1)
    X, Y = seqs[I], seqs[J]
    ok = (X >= 0) & (Y >= 0)
    X, Y = np.where(ok, X, 0), np.where(ok, Y, 0)
    rate = np.broadcast_to(np.asarray(site_to_rate, dtype=np.int64)[None, :], X.shape)
    index = np.full((B, n, n), -1, dtype=np.int32)
    margins = np.full((B, n, n), np.inf)
    for k in range(B):
        w = W[k][None, :]
        low, high = np.zeros(len(I), dtype=np.int64), np.full(len(I), T - 1, dtype=np.int64)
        margin = np.full(len(I), np.inf)
        while np.any(low < high):
            live = low < high
            mid = np.where(live, low + (high - low) // 2, 0)
            a = (w * np.where(ok, sym[mid[:, None], rate, X, Y], 0.0)).sum(axis=1)
            b = (w * np.where(ok, sym[np.minimum(mid + 1, T - 1)[:, None], rate, X, Y], 0.0)).sum(axis=1)
            scale = np.maximum(np.abs(a), np.abs(b))
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.where(scale > 0, np.abs(a - b) / scale, np.inf)
            margin = np.where(live, np.minimum(margin, rel), margin)
            lower = a > b
            high = np.where(live & lower, mid, high)
            low = np.where(live & ~lower, mid + 1, low)
        index[k][I, J] = index[k][J, I] = low
        margins[k][I, J] = margins[k][J, I] = margin
    return index, margins


def distance_matrix(grid, index):
    """grid[index] with a zero diagonal"""
    D = np.asarray(grid, dtype=np.float64)[np.maximum(index, 0)]
    np.fill_diagonal(D, 0.0)
    return D


def record_splits(names, rec):
    """the splits of the tree of join records, through its edges: a set of frozensets of names (the side without names[0])"""
    return ref.splits(njd.edge_adjacency(njd.edges(names, rec)), names)


def node_splits(tree, names):
    """[(node, frozenset of the leaves on the side without names[0], is the split non-trivial)] for the internal non-root nodes
    of a cherryml_amd.io.Tree in `tree.nodes()` order: the split of the edge above the node"""
    def below(v):
        kids = tree.children(v)
        return frozenset([v]) if not kids else frozenset().union(*(below(c) for c, _ in kids))

    out = []
    for v in tree.nodes():
        if tree.is_leaf(v) or tree.is_root(v):
            continue
        part = below(v)
        if names[0] in part:
            part = frozenset(names) - part
        out.append((v, part, 1 < len(part) < len(names) - 1))
    return out


def supports(tree, names, seqs, logP, site_to_rate, grid, B, seed, W=None):
    """the end-to-end restatement -> dict(nodes [names], support [k / B; 1.0 for a trivial split], margin [B, n, n], W)"""
    names = [str(v) for v in names]
    W = weights(seqs.shape[1], B, seed) if W is None else np.asarray(W)
    index, margin = weighted_bisection(seqs, logP, site_to_rate, W)
    rep_splits = [record_splits(names, njd.join(distance_matrix(grid, index[k]), with_margins=False)) for k in range(len(W))]
    per_node = node_splits(tree, names)
    support = np.array([sum(part in s for s in rep_splits) / len(W) if real else 1.0 for _, part, real in per_node])
    return dict(nodes=[v for v, _, _ in per_node], support=support, margin=margin, W=W, index=index, splits=rep_splits)
