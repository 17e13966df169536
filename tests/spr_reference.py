"""A NumPy restatement of the subtree prune-and-regraft search (csrc/spr.hip.h, phylogeny_estimation/_spr.py; DESIGN.md section
25): the enumeration of the moves by distance, the grid indices a move is offered at, its application to a parent array, the scan
formula from the restated inside and outside messages of nni_reference.py, the greedy selection on touched sets and the search
loop with its halving rule.  Every decision of the search records its margin.  The cases are those of nni_cases.py; what is
expensive is computed once and shared (tests/test_spr_cpu.py, tests/test_gpu_spr.py)."""
import functools

import numpy as np
from scipy.special import logsumexp

import bl_cases
import bl_reference
import nni_cases
import nni_reference
from em_reference import _children, _preorder

MAX_RADIUS = 8   # CB_SPR_MAX_RADIUS of include/cherrybank.h


# ------------------------------------------------------------------------------------------------------ moves
def _below(ch, v):
    out, stack = set(), [v]
    while stack:
        w = stack.pop()
        out.add(w)
        stack += ch[w]
    return out


def route(parent, x, y):
    """The way from the prune point of x to the edge above y, or None where (x, y) is no move: ("below", [s, z1, ..., y]) for a
    target below s, else ("through", [g, a1, ..., ak], [z1, ..., zj = y]) -- up k >= 0 ancestors of g, then down j >= 0 nodes."""
    parent = np.asarray(parent)
    n = len(parent)
    if not (0 <= x < n and 0 <= y < n):
        return None
    ch = _children(parent)
    p = int(parent[x])
    if p < 0 or parent[p] < 0 or len(ch[p]) != 2:
        return None
    s = [c for c in ch[p] if c != x][0]
    g = int(parent[p])
    if parent[y] < 0 or y in (x, p, s) or y in _below(ch, x):
        return None
    up = [y]                                     # y and its ancestors
    while parent[up[-1]] >= 0:
        up.append(int(parent[up[-1]]))
    if s in up:
        return "below", up[:up.index(s) + 1][::-1]
    anc = [g]
    while anc[-1] not in up:
        anc.append(int(parent[anc[-1]]))
    return "through", anc, up[:up.index(anc[-1])][::-1]


def distance(parent, x, y):
    r = route(parent, x, y)
    if r is None:
        return None
    return len(r[1]) - 1 if r[0] == "below" else len(r[1]) + max(len(r[2]) - 1, 0)


def distance_by_definition(parent, x, y):
    """the issue's words: build T' (x pruned, p dissolved, s under g) and count the nodes of T' on the path between the merged
    edge g-s and the edge above y, by breadth-first search from both ends of the merged edge"""
    parent = np.asarray(parent)
    ch = _children(parent)
    p = int(parent[x])
    s = [c for c in ch[p] if c != x][0]
    g = int(parent[p])
    gone = _below(ch, x) | {p}
    par = {v: int(parent[v]) for v in range(len(parent)) if v not in gone}
    par[s] = g
    adj = {v: set() for v in par}
    for v, q in par.items():
        if q >= 0 and (v, q) != (s, g):
            adj[v].add(q), adj[q].add(v)
    dist, front = {g: 1, s: 1}, [g, s]
    while front:
        nxt = []
        for v in front:
            for w in adj[v]:
                if w not in dist:
                    dist[w] = dist[v] + 1
                    nxt.append(w)
        front = nxt
    return min(dist[y], dist[par[y]])


def moves(parent, radius=3):
    """[n, 2] (x, y): x ascending, then y ascending, every move of distance <= radius"""
    n = len(parent)
    out = []
    for x in range(n):
        for y in range(n):
            d = distance(parent, x, y)
            if d is not None and d <= radius:
                out.append((x, y))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def nearest(grid, t):
    """the lowest index with the smallest |log grid[k] - log t|"""
    return int(np.argmin(np.abs(np.log(np.asarray(grid, dtype=np.float64)) - np.log(t))))


def indices(grid, tau, parent, xy):
    """[n, 3] (tau_s, tau_p, tau_y): the prune point keeps its path length, the regraft edge is halved"""
    grid = np.asarray(grid, dtype=np.float64)
    ch = _children(parent)
    out = []
    for x, y in np.asarray(xy).reshape(-1, 2).tolist():
        p = int(parent[x])
        s = [c for c in ch[p] if c != x][0]
        h = nearest(grid, grid[tau[y]] / 2)
        out.append((nearest(grid, grid[tau[p]] + grid[tau[s]]), h, h))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def touched(parent, x, y):
    r = route(parent, x, y)
    p = int(parent[x])
    s = [c for c in _children(parent)[p] if c != x][0]
    return {x, p, s, int(parent[p]), y, int(parent[y])} | set(r[1]) | set(r[2] if r[0] == "through" else [])


def apply(parent, tau, mvs):
    """(parent, tau) after the moves (x, y, tau_s, tau_p, tau_y), which must have disjoint touched sets"""
    parent, tau = np.asarray(parent), np.asarray(tau)
    new, ntau = parent.copy(), tau.copy()
    seen = set()
    ch = _children(parent)
    for x, y, ts, tp, ty in np.asarray(mvs).reshape(-1, 5).tolist():
        assert route(parent, x, y) is not None, (x, y)
        t = touched(parent, x, y)
        assert not seen & t, (x, y)
        seen |= t
        p = int(parent[x])
        s = [c for c in ch[p] if c != x][0]
        new[s], new[p], new[y] = parent[p], parent[y], p
        ntau[s], ntau[p], ntau[y] = ts, tp, ty
    return new, ntau


# ------------------------------------------------------------------------------------------------------ the scan
def scan(parent, tau, codes, rates, grid, Q, pi, mvs, logP=None):
    """-> (ll_moves [m, L] by the scan formula of the issue, ll [L] of the tree itself)"""
    parent, tau, codes = np.asarray(parent), np.asarray(tau), np.asarray(codes)
    rates = np.asarray(rates, dtype=np.float64)
    logP = nni_reference._log_bank(grid, rates, Q) if logP is None else logP
    msg, U, ll = nni_reference.messages(parent, tau, codes, rates, grid, Q, pi, logP)
    ch = _children(parent)
    cat = np.searchsorted(np.unique(rates), rates)
    S, L = Q.shape[0], len(rates)

    def up(t, d):
        return logsumexp(logP[t, cat] + d[:, None, :], axis=2)

    def down(t, o):
        return logsumexp(o[:, :, None] + logP[t, cat], axis=1)

    def kids(w, *but):
        out = np.zeros((L, S))
        for c in ch[w]:
            if c not in but:
                out = out + msg[c]
        return out

    def inside(w):
        if ch[w]:
            return kids(w)
        k = codes[w]
        return np.where((k[:, None] < 0) | (k[:, None] == np.arange(S)[None, :]), 0.0, -np.inf)

    def walk_down(Uz, zs):
        """Uz = U'[zs[0]] -> O' at zs[-1]"""
        O = None
        for i in range(len(zs) - 1):
            O = Uz + kids(zs[i], zs[i + 1])
            if i + 2 < len(zs):
                Uz = down(tau[zs[i + 1]], O)
        return O

    mvs = np.asarray(mvs).reshape(-1, 5)
    res = np.zeros((len(mvs), L))
    with np.errstate(invalid="ignore"):
        for m, (x, y, ts, tp, ty) in enumerate(mvs.tolist()):
            r = route(parent, x, y)
            assert r is not None, (x, y)
            p = int(parent[x])
            s = [c for c in ch[p] if c != x][0]
            g = int(parent[p])
            if r[0] == "below":
                O = walk_down(down(ts, U[g] + kids(g, p)), r[1])
                I = inside(y)
            else:
                anc, zs = r[1], r[2]
                z1 = zs[0] if zs else -1
                m_up = up(ts, inside(s))                       # the message of the merged edge at g
                prev = p
                for i, a in enumerate(anc):
                    last = i + 1 == len(anc)
                    Ia = m_up + kids(a, prev, z1 if last else -1)   # I'(a), at the last one with msg[z1] left out
                    if not last:
                        m_up, prev = up(tau[a], Ia), a
                if not zs:
                    I = Ia
                    O = U[parent[y]] + kids(int(parent[y]), y)
                else:
                    O = U[anc[-1]] + Ia
                    if len(zs) > 1:
                        O = walk_down(down(tau[z1], O), zs)
                    I = inside(y)
            res[m] = logsumexp(O + up(tp, msg[x] + up(ty, I)), axis=1)
    return res, ll


def select(mvs, delta, parent, min_gain=0.0):
    """indices into mvs: by descending delta (ties: the lower index), delta > min_gain, no touched node used twice"""
    mvs, delta = np.asarray(mvs).reshape(-1, 5), np.asarray(delta)
    order = sorted((m for m in range(len(mvs)) if delta[m] > min_gain), key=lambda m: (-delta[m], m))
    used, taken = set(), []
    for m in order:
        t = touched(parent, int(mvs[m][0]), int(mvs[m][1]))
        if not used & t:
            used |= t
            taken.append(m)
    return np.array(taken, dtype=np.int64)


def full_moves(parent, tau, grid, radius):
    xy = moves(parent, radius)
    return np.concatenate([xy, indices(grid, tau, parent, xy)], axis=1).reshape(-1, 5)


def search(parent, tau, codes, rates, grid, Q, pi, num_spr_rounds, num_rounds, radius=3):
    """The loop of ml_spr_trees on one family -> dict(parent, tau, final, rounds = [dict(before, scanned, selected, applied,
    after)], margin = the smallest margin of a decision relative to |log-likelihood| -- delta > 0, the order of two positive
    deltas whose touched sets meet, accept or reject --, em_margin = the smallest relative argmax margin of an EM round)."""
    parent, tau = np.asarray(parent).copy(), np.asarray(tau).copy()
    P = bl_reference.bank(grid, np.unique(rates), Q)
    with np.errstate(divide="ignore"):
        logP = np.log(np.where(P > 0, P, 0.0))
    rounds, margin, em_margin = [], np.inf, np.inf
    final, moved = None, True
    for _ in range(num_spr_rounds):
        tau, em = nni_reference._em(parent, tau, codes, rates, grid, Q, pi, P, num_rounds)
        em_margin = min(em_margin, em)
        mvs = full_moves(parent, tau, grid, radius)
        ll_moves, ll = scan(parent, tau, codes, rates, grid, Q, pi, mvs, logP)
        before = float(ll.sum())
        delta = (ll_moves - ll[None, :]).sum(axis=1)
        if len(delta):
            margin = min(margin, float(np.abs(delta).min()) / abs(before))
            pos = [m for m in range(len(mvs)) if delta[m] > 0]
            sets = {m: touched(parent, int(mvs[m][0]), int(mvs[m][1])) for m in pos}
            for i, a in enumerate(pos):
                for b in pos[i + 1:]:
                    if sets[a] & sets[b]:
                        margin = min(margin, abs(float(delta[a] - delta[b])) / abs(before))
        sel = mvs[select(mvs, delta, parent)]
        rec = dict(before=before, scanned=len(mvs), selected=sel.tolist(), applied=[], after=before,
                   best=float(delta.max()) if len(delta) else 0.0, positive=int((delta > 0).sum()))
        rounds.append(rec)
        moved = False
        while len(sel):
            cand, ctau = apply(parent, tau, sel)
            after = float(nni_reference.site_ll(cand, ctau, codes, rates, grid, Q, pi, logP).sum())
            margin = min(margin, abs(after - before) / abs(before))
            if after > before:
                parent, tau, moved = cand, ctau, True
                rec.update(applied=sel.tolist(), after=after)
                break
            sel = sel[:len(sel) // 2]
        if not moved:
            final = before
            break
    if moved:
        tau, em = nni_reference._em(parent, tau, codes, rates, grid, Q, pi, P, num_rounds)
        em_margin = min(em_margin, em)
        final = float(nni_reference.site_ll(parent, tau, codes, rates, grid, Q, pi, logP).sum())
    return dict(parent=parent, tau=tau, final=final, rounds=rounds, margin=margin, em_margin=em_margin)


# ------------------------------------------------------------------------------------------------------ shared results
# the prototype's counts of the issue, per family in CASES order, for radius 1, 2 and 3
MOVE_COUNTS = {"s4": [[0, 8], [0, 28], [0, 28]], "s20": [[38, 78], [70, 188], [96, 302]], "s32": [[8, 0], [28, 0], [28, 0]],
               "s20one": [[78], [176], [306]], "s4small": [[4, 8], [12, 10], [12, 10]]}


@functools.lru_cache(maxsize=None)
def restated(name, radius=3):
    """per family (tau, moves [m, 5], ll_moves [m, L], ll [L]) of the restatement at the snapped input lengths"""
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    out = []
    for parent, length, codes, rates in fams:
        tau = bl_reference.snap(length, parent, grid)
        mvs = full_moves(parent, tau, grid, radius)
        ll_moves, ll = scan(parent, tau, codes, rates, grid, Q, pi, mvs)
        out.append((tau, mvs, ll_moves, ll))
    return out


@functools.lru_cache(maxsize=None)
def deep_family():
    """an 11-leaf caterpillar at S = 4: it has moves at the cap of 8 and, for the refusals, at distance 9"""
    return bl_cases.family(bl_cases.caterpillar(11), 4, [5, 6], [0.5, 2.0], bl_cases.GRID, 31)


SEARCH_START = (1, 16)   # the SPR of the true tree the search starts from: distance 3, three splits wrong
SEARCH_SPR_ROUNDS, SEARCH_EM_ROUNDS = 4, 3


@functools.lru_cache(maxsize=None)
def search_family():
    """nni_cases.search_family's alignment on its true tree with the move SEARCH_START applied at spr_indices' lengths
    -> dict(true_parent, start_parent, start_tau, codes, rates)"""
    f = nni_cases.search_family()
    mv = full_moves(f["true_parent"], f["tau"], bl_cases.GRID, MAX_RADIUS)
    mv = mv[(mv[:, 0] == SEARCH_START[0]) & (mv[:, 1] == SEARCH_START[1])]
    assert len(mv) == 1
    parent, tau = apply(f["true_parent"], f["tau"], mv)
    return dict(true_parent=f["true_parent"], start_parent=parent, start_tau=tau, codes=f["codes"], rates=f["rates"])


@functools.lru_cache(maxsize=None)
def restated_search():
    f = search_family()
    Q, pi = bl_cases.model(20)
    return search(f["start_parent"], f["start_tau"], f["codes"], f["rates"], bl_cases.GRID, Q, pi, SEARCH_SPR_ROUNDS,
                  SEARCH_EM_ROUNDS)
