"""The NumPy restatement of neighbour joining on the device (csrc/nj.hip.h, `cb_nj_batch`), no GPU: the join loop of
`neighbor_joining` with the device's order of the row sums -- one wave per row, lane l adds the columns l, l + 64, ... upwards
onto 0.0, then the xor butterfly over the offsets 32, 16, 8, 4, 2, 1 -- and everything else as the device and the host do it:
crit = (m - 2) d_ij - (r_i + r_j) as a rounded product minus a rounded sum, the winner under the total order (crit, lower rank,
higher rank), l_i = d_ij / 2 + (r_i - r_j) / (2 (m - 2)), l_j = d_ij - l_i, d_uk = ((d_ik + d_jk) - d_ij) / 2, the joined node
in slot i, the last slot's node in slot j.  Per join it records the relative margin between the best and the next distinct
criterion value and whether the best value occurred more than once.  Random trees, splits and path lengths: nj_reference."""
import numpy as np

from nj_reference import adjacency, path_lengths, random_tree, splits  # noqa: F401  (shared with the tests)

LANES = 64


def row_sums(V):
    """the sums of the rows of V [rows, m] in the device's order"""
    rows, m = V.shape
    chunks = (m + LANES - 1) // LANES
    P = np.zeros((rows, chunks * LANES))
    P[:, :m] = V
    acc = np.zeros((rows, LANES))
    for c in range(chunks):                                 # lane l: columns l, l + 64, ... upwards from 0.0
        acc = acc + P[:, c * LANES:(c + 1) * LANES]
    lane = np.arange(LANES)
    for off in (32, 16, 8, 4, 2, 1):                        # the xor butterfly: every lane ends with the same sum
        acc = acc + acc[:, lane ^ off]
    return np.ascontiguousarray(acc[:, 0])


def join(D, with_margins=True):
    """`cb_nj_batch`'s outputs for one symmetric matrix D [n, n] with a zero diagonal, restated: a dict of join_nodes [n - 3, 2]
    int32 (leaves 0 .. n-1, the node of join k is n + k; column 0 = the lower place in the active list), join_len [n - 3, 2] raw,
    final_nodes [3] int32 and final_D [3, 3] (the last three active nodes in active-list order; n = 3 or 2: the leaves, unused
    slots -1 / 0), and per join m [n - 3], margin [n - 3] ((next distinct criterion - best) / max(|next|, |best|), inf when there
    is no other value; empty with `with_margins=False`, which saves a pass per join on a large family) and tie [n - 3] (the best
    value occurred at more than one pair)."""
    D = np.array(D, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n) and n >= 2 and np.array_equal(D, D.T) and not np.diag(D).any()
    node, rank = np.arange(n), np.arange(n)
    jn, jl, ms, margins, ties = [], [], [], [], []
    m = n
    work, diag = np.empty((2, n * n)), np.arange(n)
    while m > 3:
        V = D[:m, :m]
        r = row_sums(V)
        crit, rr = work[0, :m * m].reshape(m, m), work[1, :m * m].reshape(m, m)
        np.multiply(V, float(m - 2), out=crit)                  # a rounded product,
        crit -= np.add.outer(r, r, out=rr)                      # then a rounded difference of the rounded sum
        crit[diag[:m], diag[:m]] = np.inf
        best = crit.min()
        a, b = np.nonzero(crit == best)                         # (every pair and its mirror image)
        ra, rb = rank[a], rank[b]
        k = np.lexsort((np.maximum(ra, rb), np.minimum(ra, rb)))[0]
        i, j = int(a[k]), int(b[k])
        if rank[i] > rank[j]:
            i, j = j, i
        if with_margins:
            nxt = np.where(crit > best, crit, np.inf).min()
            margins.append((nxt - best) / max(abs(nxt), abs(best)) if np.isfinite(nxt) else np.inf)
        ties.append(len(a) > 2)
        ms.append(m)
        dij = V[i, j]
        li = dij / 2.0 + (r[i] - r[j]) / (2.0 * (m - 2))
        jn.append((node[i], node[j]))
        jl.append((li, dij - li))
        du = ((V[i] + V[j]) - dij) / 2.0
        V[i, :] = du
        V[:, i] = du
        V[i, i] = 0.0
        node[i] = rank[i] = n + len(jn) - 1
        if j != m - 1:
            V[j, :] = V[m - 1, :]
            V[:, j] = V[:, m - 1]
            V[j, j] = 0.0
            node[j], rank[j] = node[m - 1], rank[m - 1]
        m -= 1
    order = np.argsort(rank[:m])
    final_nodes, final_D = np.full(3, -1, dtype=np.int32), np.zeros((3, 3))
    final_nodes[:m] = node[order]
    final_D[:m, :m] = D[np.ix_(order, order)]
    return dict(join_nodes=np.array(jn, dtype=np.int32).reshape(-1, 2), join_len=np.array(jl, dtype=np.float64).reshape(-1, 2),
                final_nodes=final_nodes, final_D=final_D, m=np.array(ms, dtype=np.int64), margin=np.array(margins, dtype=np.float64),
                tie=np.array(ties, dtype=bool))


def edges(names, rec, min_length=0.0):
    """the edges (parent, child, length) of the tree of join records, in `Tree.edges()`' order as `neighbor_joining` builds it:
    the root step with the host's formulae, `root` and `internal-<k>`, parents before children, children in join order, every
    length below `min_length` raised to it"""
    names = [str(v) for v in names]
    n = len(names)
    label = lambda v: names[v] if v < n else f"internal-{v - n}"   # noqa: E731
    kids = {f"internal-{k}": [(label(int(a)), la), (label(int(b)), lb)]
            for k, ((a, b), (la, lb)) in enumerate(zip(rec["join_nodes"], rec["join_len"]))}
    act = [label(int(v)) for v in rec["final_nodes"] if v >= 0]
    F = rec["final_D"]
    if len(act) == 3:
        kids["root"] = [(act[0], (F[0, 1] + F[0, 2] - F[1, 2]) / 2.0), (act[1], (F[0, 1] + F[1, 2] - F[0, 2]) / 2.0),
                        (act[2], (F[0, 2] + F[1, 2] - F[0, 1]) / 2.0)]
    else:
        kids["root"] = [(act[0], F[0, 1] / 2.0), (act[1], F[0, 1] / 2.0)]
    out, stack = [], ["root"]
    while stack:
        u = stack.pop()
        out += [(u, v, max(float(t), float(min_length))) for v, t in kids.get(u, [])]
        stack.extend(v for v, _ in reversed(kids.get(u, [])))
    return out


def edge_adjacency(edge_list):
    """{node: {neighbour: length}} of `edges`"""
    adj = {}
    for u, v, t in edge_list:
        adj.setdefault(u, {})[v] = t
        adj.setdefault(v, {})[u] = t
    return adj


# ------------------------------------------------------------------------------------------------ the tests' matrices
def integer_matrix(n, seed):
    """symmetric, entries 1 .. 8, zero diagonal: every sum is exact in float64"""
    rng = np.random.default_rng(seed)
    A = np.triu(rng.integers(1, 9, (n, n)).astype(np.float64), 1)
    return A + A.T


def ones_matrix(n):
    return np.ones((n, n)) - np.eye(n)


def random_matrix(n, seed):
    """Euclidean distances of n random points in five dimensions"""
    rng = np.random.default_rng(seed)
    X = rng.random((n, 5))
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    D = np.maximum(D, D.T)
    np.fill_diagonal(D, 0.0)
    return D


def grid_matrix(n, seed, c=0.9731):
    """grid[idx] * c with the stage's grid 0.03 * 1.1^k and few distinct indices: many duplicate entries"""
    rng = np.random.default_rng(seed)
    grid = np.array([0.03 * 1.1 ** k for k in range(-64, 65)])
    idx = np.triu(rng.integers(40, 90, (n, n)), 1)
    D = np.triu(grid[idx] * c, 1)
    return D + D.T
