"""A NumPy restatement of the co-evolution scan (include/cherrybank.h, cb_coscan_*): plain loops over
(i, j, sequence pair, term) with a float64 expm of its own.  The tests compare the GPU with it, and it with a brute-force form
that builds the one-pair count tensor with the counting oracle."""
import numpy as np


def quantize(bl, grid):
    """cherryml/utils.py:35-56: nearest grid point in relative error, ties to the right, None outside the grid"""
    if bl < grid[0] or bl > grid[-1]:
        return None
    k = int(np.searchsorted(grid, bl))
    if k == 0:
        return 0
    left, right = grid[k - 1], grid[k]
    return k - 1 if (bl / left - 1) < (right / bl - 1) else k


def expm(A):
    """scaling and squaring around a Taylor series (norm below 1/4 after scaling: 18 terms reach 1e-17)"""
    A = np.asarray(A, dtype=np.float64)
    norm = np.abs(A).sum(axis=1).max()
    s = max(0, int(np.ceil(np.log2(max(norm, 1e-300) / 0.25))))
    X = A / 2.0 ** s
    E, term = np.eye(A.shape[0]) + X, X
    for k in range(2, 19):
        term = term @ X / k
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


def bank(Q, grid, pi=None):
    """P[q] = expm(grid[q] Q).  pi (the stationary distribution of a reversible Q): through the symmetric eigendecomposition of
    D^1/2 Q D^-1/2 -- one decomposition for the whole grid, what makes the 400-state bank affordable on the CPU"""
    Q, grid = np.asarray(Q, dtype=np.float64), np.asarray(grid, dtype=np.float64)
    if pi is None:
        return np.stack([expm(t * Q) for t in grid])
    d = np.sqrt(np.asarray(pi, dtype=np.float64))
    A = d[:, None] * Q / d[None, :]
    lam, U = np.linalg.eigh((A + A.T) / 2)
    return np.stack([(U * np.exp(t * lam)) @ U.T * d[None, :] / d[:, None] for t in grid])


def log_bank(P):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(P > 0, np.log(np.where(P > 0, P, 1.0)), -np.inf)


def terms(xi, xj, yi, yj, S, symmetric):
    """the (from, to) states the counter adds for one sequence pair and the contact (i, j)"""
    s, sr, e, er = xi * S + xj, xj * S + xi, yi * S + yj, yj * S + yi
    return [(s, e), (sr, er)] + ([(e, s), (er, sr)] if symmetric else [])


def scan(codes, pairs, grid, logP1, logP2, symmetric):
    """codes [n_sequences][L] (negative = a gap), pairs [(row a, row b, len_a, len_b)] -> score, pair_ll, indep_ll, n_used [L][L].
    The sequence pairs are walked by bucket, ties by pair index; off-grid pairs are dropped."""
    codes = np.asarray(codes)
    L = codes.shape[1]
    S = logP1.shape[1]
    w = 0.25 if symmetric else 0.5
    kept = [(quantize(la + lb, grid), k, a, b) for k, (a, b, la, lb) in enumerate(pairs)]
    kept = sorted((q, k, a, b) for q, k, a, b in kept if q is not None)
    pair_ll, indep_ll = np.zeros((L, L)), np.zeros((L, L))
    n_used = np.zeros((L, L), dtype=np.int32)
    for i in range(L):
        for j in range(i + 1, L):
            s2 = s1 = 0.0
            for q, _, a, b in kept:
                xi, xj, yi, yj = int(codes[a, i]), int(codes[a, j]), int(codes[b, i]), int(codes[b, j])
                if xi < 0 or xj < 0 or yi < 0 or yj < 0:
                    continue
                n_used[i, j] += 1
                for frm, to in terms(xi, xj, yi, yj, S, symmetric):
                    s2 += logP2[q, frm, to]
                    s1 += logP1[q, frm // S, to // S] + logP1[q, frm % S, to % S]
            pair_ll[i, j] = pair_ll[j, i] = w * s2
            indep_ll[i, j] = indep_ll[j, i] = w * s1
            n_used[j, i] = n_used[i, j]
    return dict(score=pair_ll - indep_ll, pair_ll=pair_ll, indep_ll=indep_ll, n_used=n_used)


def brute_force(codes, pairs, grid, logP1, logP2, symmetric, co_count_pair):
    """the same quantities from count tensors: per (i, j) and sequence pair the counting oracle's one-pair tensor for the
    contact list [(i, j)] (it carries the weight), contracted with the log banks"""
    codes = np.asarray(codes)
    L = codes.shape[1]
    S = logP1.shape[1]
    S2 = S * S
    # log P1 (x) log P1 as a [S^2][S^2] table: entry ((a,c), (b,d)) = log P1[a][b] + log P1[c][d]
    prod = [(lp[:, None, :, None] + lp[None, :, None, :]).reshape(S2, S2) for lp in logP1]
    out = dict(pair_ll=np.zeros((L, L)), indep_ll=np.zeros((L, L)), n_used=np.zeros((L, L), dtype=np.int32))
    for i in range(L):
        for j in range(i + 1, L):
            C = np.zeros((len(grid), S2, S2))
            for a, b, la, lb in pairs:
                q = quantize(la + lb, grid)
                if q is None:
                    continue
                before = C[q].sum()
                co_count_pair(C[q], [int(v) for v in codes[a]], [int(v) for v in codes[b]], [(i, j)], S, symmetric)
                out["n_used"][i, j] += int(C[q].sum() - before > 0)
            nz = np.nonzero(C)
            out["pair_ll"][i, j] = sum(C[b, s, e] * logP2[b, s, e] for b, s, e in zip(*nz))
            out["indep_ll"][i, j] = sum(C[b, s, e] * prod[b][s, e] for b, s, e in zip(*nz))
            for key in out:
                out[key][j, i] = out[key][i, j]
    out["score"] = out["pair_ll"] - out["indep_ll"]
    return out


def apc(score):
    """the average product correction, from the formula: m_i the mean of score[i, k] over k != i, m the mean over i != j"""
    L = score.shape[0]
    if L < 2:
        return score.copy()
    m_i = np.array([np.mean([score[i, k] for k in range(L) if k != i]) for i in range(L)])
    m = np.mean([score[i, j] for i in range(L) for j in range(L) if i != j])
    if m == 0:
        return score.copy()
    out = np.array([[score[i, j] - m_i[i] * m_i[j] / m if i != j else 0.0 for j in range(L)] for i in range(L)])
    return out


# ---------------------------------------------------------------- models and families for the tests
def random_reversible(n, seed, low=0.2):
    """a dense reversible rate matrix (every off-diagonal entry positive) and its stationary distribution"""
    rng = np.random.default_rng(seed)
    pi = rng.uniform(0.5, 1.5, n)
    pi /= pi.sum()
    X = rng.uniform(low, 1.0, (n, n))
    X = (X + X.T) / 2
    Q = X * pi[None, :]
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q / -(pi * np.diag(Q)).sum(), pi


def random_general(n, seed):
    rng = np.random.default_rng(seed)
    Q = rng.uniform(0.2, 1.0, (n, n))
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q / n


def product_model(Q1):
    """Q_2 = Q_1 (x) I + I (x) Q_1: two sites evolving independently"""
    Id = np.eye(Q1.shape[0])
    return np.kron(Q1, Id) + np.kron(Id, Q1)


def tilted_pair_model(Q1, pi1, favoured, tilt):
    """A reversible Q_2 with single-site changes only whose stationary law is pi1 (x) pi1 tilted by exp(tilt) towards the state
    pairs in `favoured`: q(x -> y) = s(x, y) pi2(y) with s the exchangeability of the one site that changes.  -> Q_2, pi_2"""
    S = len(pi1)
    pi2 = np.outer(pi1, pi1)
    for a, b in favoured:
        pi2[a, b] *= np.exp(tilt)
    pi2 = (pi2 / pi2.sum()).reshape(-1)
    s1 = Q1 / pi1[None, :]
    Q2 = np.zeros((S * S, S * S))
    for a in range(S):
        for b in range(S):
            for c in range(S):
                if c != a:
                    Q2[a * S + b, c * S + b] = s1[a, c] * pi2[c * S + b]
                if c != b:
                    Q2[a * S + b, a * S + c] = s1[b, c] * pi2[a * S + c]
    np.fill_diagonal(Q2, -Q2.sum(axis=1))
    return Q2 / -(pi2 * np.diag(Q2)).sum() * 2.0, pi2      # two sites: two expected changes per unit time


def random_tree_text(n_leaves, seed):
    """a random binary tree in the tree file format: leaves l0.., internal nodes n0.., lengths uniform in [0.05, 0.5]"""
    rng = np.random.default_rng(seed)
    live = [f"l{k}" for k in range(n_leaves)]
    nodes, edges = list(live), []
    k = 0
    while len(live) > 1:
        i, j = sorted(rng.choice(len(live), 2, replace=False).tolist())
        a, b = live[i], live[j]
        live = [v for v in live if v not in (a, b)] + [f"n{k}"]
        nodes.append(f"n{k}")
        edges += [(f"n{k}", a, float(rng.uniform(0.05, 0.5))), (f"n{k}", b, float(rng.uniform(0.05, 0.5)))]
        k += 1
    return f"{len(nodes)} nodes\n" + "\n".join(nodes) + f"\n{len(edges)} edges\n" + "\n".join(f"{u} {v} {t!r}" for u, v, t in edges) + "\n"


def top_pairs(apc_matrix, n_used, min_dist, k):
    """the k best site pairs by apc among j - i >= min_dist with n_used > 0 (apc descending, then (i, j)), and the relative gap
    between the k-th and the (k+1)-th"""
    L = apc_matrix.shape[0]
    cand = [(i, j) for i in range(L) for j in range(i + min_dist, L) if n_used[i, j] > 0]
    cand.sort(key=lambda ij: (-apc_matrix[ij], ij))
    last, nxt = apc_matrix[cand[k - 1]], apc_matrix[cand[k]]
    return cand[:k], float((last - nxt) / max(abs(last), abs(nxt)))


# ---------------------------------------------------------------- the recovery case (tests/test_gpu_coscan.py, section 5)
RECOVERY_STATES = list("ACGT")
RECOVERY_SITES, RECOVERY_LEAVES, RECOVERY_MIN_DIST = 40, 64, 7
RECOVERY_CONTACTS = [(k, k + 20) for k in range(10)]                 # ten contacting pairs, 20 sites apart
RECOVERY_FAVOURED = [(a, a) for a in range(4)]                       # the tilt: both sites in the same state
RECOVERY_GRID = [float(t) for t in np.exp(np.linspace(np.log(0.02), np.log(4.0), 32))]
RECOVERY_MODE = "cherry++"
# chosen on the CPU (test_coscan_cpu.py asserts it): with this seed and tilt the ten true pairs are the restatement's top ten by
# apc, and the tenth is RECOVERY_MARGIN (relative) above the best false pair
RECOVERY_SEED, RECOVERY_TILT = 2, 2.0     # (of seeds 0..5 at tilt 2: five recover all ten, seed 3 nine; tilt 1 recovers 5 to 8)
RECOVERY_MARGIN = 0.346506


def recovery_inputs(root, seed=RECOVERY_SEED, tilt=RECOVERY_TILT):
    """the files `simulate_msas` and `coevolution_scan` read for the recovery case, under `root`; -> their paths and the model"""
    import os
    from cherryml_amd.io import write_probability_distribution, write_rate_matrix
    S, L = len(RECOVERY_STATES), RECOVERY_SITES
    for d in ("trees", "rates", "contacts"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    with open(os.path.join(root, "trees", "fam.txt"), "w") as f:
        f.write(random_tree_text(RECOVERY_LEAVES, seed))
    with open(os.path.join(root, "rates", "fam.txt"), "w") as f:
        f.write(f"{L} sites\n" + " ".join(["1.0"] * L))
    cm = np.zeros((L, L), dtype=int)
    for i, j in RECOVERY_CONTACTS:
        cm[i, j] = cm[j, i] = 1
    with open(os.path.join(root, "contacts", "fam.txt"), "w") as f:
        f.write(f"{L} sites\n" + "\n".join("".join(str(v) for v in row) for row in cm) + "\n")
    Q1, pi1 = random_reversible(S, 1)
    Q2, pi2 = tilted_pair_model(Q1, pi1, RECOVERY_FAVOURED, tilt)
    pair_states = [a + b for a in RECOVERY_STATES for b in RECOVERY_STATES]
    p = {k: os.path.join(root, k + ".txt") for k in ("Q_1", "pi_1", "Q_2", "pi_2")}
    write_rate_matrix(Q1, RECOVERY_STATES, p["Q_1"])
    write_rate_matrix(Q2, pair_states, p["Q_2"])
    write_probability_distribution(pi1, RECOVERY_STATES, p["pi_1"])
    write_probability_distribution(pi2, pair_states, p["pi_2"])
    return dict(paths=p, tree_dir=os.path.join(root, "trees"), site_rates_dir=os.path.join(root, "rates"),
                contact_map_dir=os.path.join(root, "contacts"), Q1=Q1, pi1=pi1, Q2=Q2, pi2=pi2, seed=seed)


def recovery_restated(z):
    """the restatement's side of the recovery case: the alignment by tests/sim_stream.py (the simulator's stream in NumPy), the
    counter's sequence pairs by the counting oracle, the scan and apc by this module -> (top ten pairs, margin, apc)"""
    import os
    import sim_stream
    from cherryml_amd import _lib
    from cherryml_amd.simulation._simulate import _read_family, family_seed
    from oracle import counting_oracle as co
    fam = _read_family(z["tree_dir"], z["site_rates_dir"], z["contact_map_dir"], "fam", family_seed("fam", z["seed"]))
    lib = _lib.load()
    t1, t2 = sim_stream.model_tables(lib, z["Q1"], z["pi1"]), sim_stream.model_tables(lib, z["Q2"], z["pi2"])
    codes = sim_stream.simulate_family(t1, t2, len(RECOVERY_STATES), fam)
    row = {v: r for r, v in enumerate(fam["names"])}
    nodes, children, root = co.read_tree(os.path.join(z["tree_dir"], "fam.txt"))
    pairs = [(row[a], row[b], la, lb) for a, b, la, lb in co.transition_pairs(nodes, children, root, RECOVERY_MODE)]
    grid = np.array(RECOVERY_GRID)
    r = scan(codes, pairs, grid, log_bank(bank(z["Q1"], grid, z["pi1"])), log_bank(bank(z["Q2"], grid, z["pi2"])), True)
    a = apc(r["score"])
    top, margin = top_pairs(a, r["n_used"], RECOVERY_MIN_DIST, len(RECOVERY_CONTACTS))
    return top, margin, a


def random_family(S, L, n_pairs, grid, seed, gaps=0.25):
    """codes [2 n_pairs][L] with gaps, an all-gap sequence and an all-gap column (where there is room), and sequence pairs whose
    lengths cover the grid, one beyond each end when there are at least three"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, S, (2 * n_pairs, L)).astype(np.int8)
    codes[rng.random(codes.shape) < gaps] = -1
    order = rng.permutation(2 * n_pairs)
    if n_pairs >= 3:
        codes[order[2 * (n_pairs - 1)]] = -1   # the all-gap sequence: in the last pair
    if L >= 3:
        codes[:, L // 2] = -1
    else:                                      # one or two sites: the first pair (it is on the grid) has no gap
        codes[order[:2]] = rng.integers(0, S, (2, L))
    lens = np.exp(rng.uniform(np.log(grid[0]), np.log(grid[-1]), n_pairs))
    if n_pairs >= 3:
        lens[1], lens[2] = grid[0] * 0.5, grid[-1] * 2.0
    split = rng.uniform(0.2, 0.8, n_pairs)
    pairs = [(int(order[2 * k]), int(order[2 * k + 1]), float(lens[k] * split[k]), float(lens[k] * (1 - split[k])))
             for k in range(n_pairs)]
    return codes, pairs
