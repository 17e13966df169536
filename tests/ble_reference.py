"""What the FastCherries kernel tests share (no GPU, NumPy only): the vectorised NumPy restatement of the reference's two
bisections (branch_length_estimation.cpp:60-144; oracle/ble_oracle.py: get_branch_lengths, get_site_rates), of their coordinate
ascent (:146-241) and of the SiteRM site-rate gather (fast_site_rates.pyx:8-47), each recording how close every item came to a
tie; the per-site pair counts behind the initial bins (:10-58); banks, a generator that draws cherries from a bank, and the
REGION-ISOLATING inputs: families in which some cherries (sites) are observed only inside one part of a kernel's iteration
space, so that a kernel which skips that part returns the no-data default for them."""
import os
import sys
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nj_reference import log_bank, stationary, transition_matrices  # noqa: E402,F401

UNDECIDED = 1e-9    # an item whose margin is at most this is left out of a comparison (summation order: ~1e-13 relative)


# ------------------------------------------------------------------------------------------------ the restatement
def _bisection(count, top, sums, exact_ties):
    """The reference's bisection on 0 .. top for `count` items at once: sums(mid, mid + 1) -> (a, b); `a > b` keeps the lower
    half.  margin: the smallest |a - b| / max(|a|, |b|) an item met, inf where both were 0 at every step (`0 > 0` is false
    whatever the order of summation).  exact_ties: a step with a == b bit for bit (two identical bank entries: the same
    addends in the same order on both sides, here and in a kernel) does not lower the margin."""
    low, high = np.zeros(count, dtype=np.int64), np.full(count, top, dtype=np.int64)
    margin = np.full(count, np.inf)
    while np.any(low < high):
        live = low < high
        mid = np.where(live, low + (high - low) // 2, 0)
        a, b = sums(mid, np.minimum(mid + 1, top))
        scale = np.maximum(np.abs(a), np.abs(b))
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(scale > 0, np.abs(a - b) / scale, np.inf)
        if exact_ties:
            rel = np.where(a == b, np.inf, rel)
        margin = np.where(live, np.minimum(margin, rel), margin)
        lower = a > b
        high = np.where(live & lower, mid, high)
        low = np.where(live & ~lower, mid + 1, low)
    return low.astype(np.int32), margin


def _observed(cx, cy):
    X, Y = np.asarray(cx).astype(np.int64), np.asarray(cy).astype(np.int64)
    ok = (X >= 0) & (Y >= 0)
    return np.where(ok, X, 0), np.where(ok, Y, 0), ok


def branch_length_bisection(cx, cy, logP, site_to_rate, exact_ties=False):
    """get_branch_lengths (:60-103) for the cherries cx, cy [n, L] (-1 = gap): (index [n] int32, margin [n])"""
    X, Y, ok = _observed(cx, cy)
    sym = logP + logP.transpose(0, 1, 3, 2)
    rate = np.asarray(site_to_rate, dtype=np.int64)[None, :]

    def sums(m, m1):
        return (np.where(ok, sym[m[:, None], rate, X, Y], 0.0).sum(axis=1),
                np.where(ok, sym[m1[:, None], rate, X, Y], 0.0).sum(axis=1))
    return _bisection(X.shape[0], logP.shape[0] - 1, sums, exact_ties)


def site_rate_bisection(cx, cy, logP, lengths_index, priors, exact_ties=False):
    """get_site_rates (:105-144): (index [L] int32, margin [L]); both sides of a step start from their log prior"""
    X, Y, ok = _observed(cx, cy)
    sym = logP + logP.transpose(0, 1, 3, 2)
    t = np.asarray(lengths_index, dtype=np.int64)[:, None]
    priors = np.asarray(priors, dtype=np.float64)

    def sums(m, m1):
        return (np.where(ok, sym[t, m[None, :], X, Y], 0.0).sum(axis=0) + priors[m],
                np.where(ok, sym[t, m1[None, :], X, Y], 0.0).sum(axis=0) + priors[m1])
    return _bisection(X.shape[1], len(priors) - 1, sums, exact_ties)


def gather_argmax(cx, cy, tens, log_prior, exact_ties=False):
    """compute_optimal_site_rates (fast_site_rates.pyx:8-47): tens[rate, cherry, x, y]; per site the FIRST rate with the largest
    log_prior[r] + sum over cherries.  Returns (index [L] int32, gap [L]): gap = (best - second best) / max(|best|, |second|),
    inf with one rate.  exact_ties: totals equal to the best bit for bit (duplicated rates) are not the second best."""
    X, Y = np.asarray(cx).astype(np.int64), np.asarray(cy).astype(np.int64)
    n = X.shape[0]
    total = tens[:, np.arange(n)[:, None], X, Y].sum(axis=1) + np.asarray(log_prior, dtype=np.float64)[:, None]   # [R, L]
    best = np.argmax(total, axis=0)
    top = total.max(axis=0)
    others = np.ones_like(total, dtype=bool)
    others[best, np.arange(total.shape[1])] = False
    if exact_ties:
        others &= total != top[None, :]
    second = np.where(others, total, -np.inf).max(axis=0)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(second), (top - second) / np.maximum(np.abs(top), np.abs(second)), np.inf)
    return best.astype(np.int32), gap


def site_totals(all_seqs, S):
    """:10-34: per site the number of sequence PAIRS whose states differ, sum_k (non_missing - cnt_k) cnt_k: [L] int64"""
    seqs = np.asarray(all_seqs).astype(np.int64)
    L = seqs.shape[1]
    site = np.broadcast_to(np.arange(L)[None, :], seqs.shape)
    seen = seqs >= 0
    cnt = np.bincount(site[seen] * S + seqs[seen], minlength=L * S).reshape(L, S).astype(np.int64)
    return ((cnt.sum(axis=1, keepdims=True) - cnt) * cnt).sum(axis=1)


def initial_bins(total, weights):
    """:36-58: sites in the order of (total, site index); the i-th of them gets category rc, rc advancing by one when
    i >= round(weights[rc] * L), halves away from zero (std::round): [L] int32"""
    total = np.asarray(total)
    L = len(total)
    order = np.lexsort((np.arange(L), total))
    cut = [int(np.floor(w * L + 0.5)) for w in weights]
    out, rc = np.zeros(L, dtype=np.int32), 0
    for i in range(L):
        if rc < len(cut) and i >= cut[rc]:
            rc += 1
        out[order[i]] = rc
    return out


def ascent(cx, cy, all_seqs, logP, rates, weights, max_iters):
    """ble (:146-241; oracle/ble_oracle.py:ble) from the two bisections above and the oracle's initial bins.  Returns (length
    indices [n], rate indices [L], iterations, the smallest margin over every step of every bisection of the ascent)."""
    from oracle import ble_oracle as bo
    site_to_rate = bo.initial_site_rates(np.asarray(all_seqs), weights, logP.shape[2])
    lengths, m = branch_length_bisection(cx, cy, logP, site_to_rate)
    smallest = float(m.min())
    priors = bo.rate_priors(rates)
    match, iterations = False, 0
    while not match and max_iters:
        site_to_rate, m = site_rate_bisection(cx, cy, logP, lengths, priors)
        smallest = min(smallest, float(m.min()))
        new, m = branch_length_bisection(cx, cy, logP, site_to_rate)
        smallest = min(smallest, float(m.min()))
        match = bool(np.array_equal(new, lengths))
        lengths = new
        max_iters -= 1
        iterations += 1
    return lengths, np.asarray(site_to_rate, dtype=np.int32), iterations, smallest


# ------------------------------------------------------------------------------------------------ banks
GRID129 = np.array([0.03 * 1.1 ** i for i in range(-64, 65)])
RATES = {1: np.array([1.0]), 2: np.array([0.4, 2.0]), 4: np.array([0.25, 0.6, 1.2, 2.5]), 8: np.geomspace(1.0 / 8, 8.0, 8),
         20: np.geomspace(0.1, 10.0, 20)}


def small_grid(T):
    """T points of the 129-point grid's range (T = 1: its middle)"""
    return np.array([0.03]) if T == 1 else np.geomspace(GRID129[16], GRID129[-16], T)


def random_reversible(S, seed):
    """a reversible rate matrix on S states, one expected change per unit time: random exchangeabilities and frequencies"""
    rng = np.random.default_rng(seed)
    E = rng.uniform(0.2, 1.0, (S, S))
    E = E + E.T
    pi = rng.dirichlet(np.full(S, 5.0))
    Q = E * pi[None, :]
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q / -(pi * np.diag(Q)).sum()


@lru_cache(maxsize=None)
def bank(key):
    """(logP [T, R, S, S], grid [T], rates [R]) by eigendecomposition (nj_reference.log_bank)"""
    def lg():
        here = os.path.dirname(os.path.abspath(__file__))
        return np.ascontiguousarray(np.load(os.path.join(here, "golden", "data_lg.npz"))["lg"], dtype=np.float64)
    if key.startswith("lg"):                               # LG on the 129-point grid, R = 1, 2, 4, 8, 20
        Q, grid, rates = lg(), GRID129, RATES[int(key[2:])]
    elif key in ("T1", "T2R2", "T17", "R1", "R3"):
        T, R = {"T1": (1, 4), "T2R2": (2, 2), "T17": (17, 4), "R1": (17, 1), "R3": (17, 3)}[key]
        Q, grid, rates = lg(), small_grid(T), (np.array([0.4, 1.0, 2.5]) if R == 3 else RATES[R])
    elif key in ("S2", "S127"):
        Q, grid, rates = random_reversible(int(key[1:]), 7), small_grid(17), RATES[4]
    elif key == "tie_t":                                   # grid points 2k + 1 and 2k + 2 are the same matrix
        logP, grid, rates = bank("T17")
        logP = logP.copy()
        logP[2::2] = logP[1:-1:2]
        return logP, grid, rates
    elif key == "tie_r":                                   # rates 2 and 3 are the same, and so are their priors
        Q, grid, rates = lg(), small_grid(17), np.array([0.25, 0.6, 1.5, 1.5])
    logP = np.ascontiguousarray(log_bank(Q, grid, rates))
    if key == "tie_r":
        logP[:, 3] = logP[:, 2]
    return logP, grid, rates


def priors(rates):
    return 2.0 * np.log(rates) - 3.0 * rates               # Gamma(3, 3) up to a constant (:199-203)


# ------------------------------------------------------------------------------------------------ the generator
def draw_y(logP, t_idx, rate_idx, x, rng):
    """y [n, L] drawn from exp(logP[t_idx[c], rate_idx[s], x[c, s], :]), by rows of cherries to bound the memory"""
    n, L = x.shape
    S = logP.shape[2]
    y = np.empty((n, L), dtype=np.int64)
    step = max(1, (1 << 22) // (L * S))
    for c0 in range(0, n, step):
        c1 = min(n, c0 + step)
        P = np.exp(logP[t_idx[c0:c1, None], rate_idx[None, :], x[c0:c1]])
        cdf = np.cumsum(P, axis=2)
        u = rng.random((c1 - c0, L, 1)) * cdf[:, :, -1:]
        y[c0:c1] = np.minimum((u > cdf).sum(axis=2), S - 1)
    return y


def family(logP, n, L, seed, specials=True, t_from=0.25):
    """Cherries drawn from the bank itself (as tests/golden/make_golden_ble.py does, vectorised): cherry c at the true length
    index t[c]
    (uniform from T * t_from to 7 T / 8), site s at the true rate category r[s], x uniform, 8-15 % gaps in each of x and y.  With `specials`: cherry 1 has
    y == x and the last cherry is all gaps (n >= 4), site L - 2 is observed by nobody (L >= 5).
    Returns (cx, cy [n, L] int8, t [n], r [L])."""
    T, R, S, _ = logP.shape
    rng = np.random.default_rng(seed)
    lo = int(T * t_from)
    t = rng.integers(lo, max(lo + 1, T - T // 8), n)
    r = rng.integers(0, R, L)
    x = rng.integers(0, S, (n, L))
    y = draw_y(logP, t, r, x, rng)
    gap = rng.uniform(0.08, 0.15, 2)
    u = rng.random((2, n, L))
    x[u[0] < gap[0]] = -1
    y[u[1] < gap[1]] = -1
    if specials and n >= 4:
        y[1] = x[1]
        x[n - 1] = y[n - 1] = -1
    if specials and L >= 5:
        x[:, L - 2] = y[:, L - 2] = -1
    if S == 127 and n >= 3 and L >= 5:                      # code 126, the largest an int8 sequence can hold, on either side
        x[0, 0], y[0, 0], x[2, 1], y[2, 1] = 126, 125, 3, 126
    return x.astype(np.int8), y.astype(np.int8), t, r.astype(np.int32)


def equal_weights(R):
    """cumulative weights of R bins of equal size for the initial site rates"""
    return np.arange(1, R + 1) / R


# ------------------------------------------------------------------------------------------------ region-isolating inputs
# Each returns the arguments of one bisection and `regions`: [(name, items, keep)].  The cherries (sites) `items` are observed
# only inside the region; `keep` [n, L] is True outside it.  `blank(cx, cy, keep)` is the family as a kernel that skips the
# region sees it: every item of `items` then has no observation at all and gets the no-data default (T - 1 for a length; for a
# rate the bisection of the priors alone).
def blank(cx, cy, keep):
    return np.where(keep, cx, -1).astype(np.int8), np.where(keep, cy, -1).astype(np.int8)


def region_branch_lengths(logP, seed=600):
    """n = 8, L = 600 for ble_branch_lengths_kernel (512 hoisted sites, then the plain loop): cherry 0 is observed only at
    sites >= 512, cherry 1 only at sites < 512, cherry 2 only at site 599, cherry 3 only at site 0; cherries 4 .. 7 everywhere."""
    n, L = 8, 600
    cx, cy, _, r = family(logP, n, L, seed, specials=False)
    site = np.arange(L)
    only = [site >= 512, site < 512, site == 599, site == 0]
    for c, m in enumerate(only):
        cx[c, ~m] = cy[c, ~m] = -1
    for c, s in ((2, 599), (3, 0)):   # the single observed site must be observed: a change of state, away from both ends
        cx[c, s], cy[c, s] = 3, 7
    regions = []
    for c, (name, m) in enumerate(zip(("tail", "hoisted", "last site", "first site"), only)):
        keep = np.ones((n, L), dtype=bool)
        keep[:, m] = False
        regions.append((name, np.array([c]), keep))
    return cx, cy, r, regions


def _extreme_rate_sites(logP, n, L, seed):
    """a family whose sites are slow or fast in turn (two sites of one kind, then two of the other) and whose cherries are long
    enough for that to show: a slow site has y == x in every cherry, a fast one is drawn at the rate category R - 1.  The answers
    then stay away from the prior's own maximum, the answer of a site without observations."""
    T, R, S, _ = logP.shape
    rng = np.random.default_rng(seed)
    t = rng.integers(T // 2, T - T // 8, n)
    r = np.where((np.arange(L) // 2) % 2 == 0, 0, R - 1)
    x = rng.integers(0, S, (n, L))
    y = np.where(r[None, :] == 0, x, draw_y(logP, t, r, x, rng))
    u = rng.random((2, n, L))
    x[u[0] < 0.1] = -1
    y[u[1] < 0.1] = -1
    return x.astype(np.int8), y.astype(np.int8), t.astype(np.int32)


def region_site_rates_wave(logP, seed=2050):
    """n = 600, L = 2050 for ble_site_rates_kernel<1> (one hoisted group of 512 cherries, then the plain loop): sites with
    s % 3 == 0 are observed only in the cherries [512, 600), s % 3 == 1 only in [0, 512), the rest everywhere."""
    n, L = 600, 2050
    cx, cy, t = _extreme_rate_sites(logP, n, L, seed)
    cherry, site = np.arange(n)[:, None], np.arange(L)[None, :]
    tail, hoisted = (cherry >= 512) & (site % 3 == 0), (cherry < 512) & (site % 3 == 1)
    seen = tail | hoisted | (site % 3 == 2)
    cx[~seen] = cy[~seen] = -1
    regions = [("tail", np.arange(0, L, 3), seen & ~tail), ("hoisted", np.arange(1, L, 3), seen & ~hoisted)]
    return cx, cy, t, regions


def region_site_rates_quarters(logP, seed=2058):
    """n = 2050, L = 8 for ble_site_rates_kernel<4> (per = 576: the waves take [0, 576), [576, 1152), [1152, 1728),
    [1728, 2050); each starts with one hoisted group of 512 where it has one): site k < 4 is observed only in wave k's
    range, site 4 only in [512, 576) (wave 0's tail), site 5 only in [0, 512) (wave 0's hoisted group), sites 6, 7 everywhere."""
    n, L, per = 2050, 8, 576
    cx, cy, t = _extreme_rate_sites(logP, n, L, seed)
    cherry = np.arange(n)
    only = [(cherry >= per * k) & (cherry < min(n, per * (k + 1))) for k in range(4)] + [(cherry >= 512) & (cherry < 576), cherry < 512]
    regions = []
    for s, m in enumerate(only):
        cx[~m, s] = cy[~m, s] = -1
    seen = (cx >= 0) | (cy >= 0)
    for s, m in enumerate(only):
        keep = np.ones((n, L), dtype=bool)
        keep[m, s] = False
        name = f"wave {s}" if s < 4 else ("wave 0 tail" if s == 4 else "wave 0 hoisted")
        regions.append((name, np.array([s]), keep & seen))
    return cx, cy, t, regions


@lru_cache(maxsize=None)
def region_case(which):
    logP, _, rates = bank("lg4")
    if which == "branch_lengths":
        cx, cy, arg, regions = region_branch_lengths(logP)
        want, margin = branch_length_bisection(cx, cy, logP, arg)
    else:
        make = region_site_rates_wave if which == "site_rates<1>" else region_site_rates_quarters
        cx, cy, arg, regions = make(logP)
        want, margin = site_rate_bisection(cx, cy, logP, arg, priors(rates))
    return cx, cy, arg, regions, want, margin
