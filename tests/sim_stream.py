"""A NumPy restatement of the simulator's random stream and jump chain (include/cherrybank.h, "MSA simulation";
DESIGN.md section 13), vectorised over the units of a family.  The tests compare the GPU's MSAs with it; it shares only the
alias tables with the library (cb_sim_alias_table)."""
import ctypes

import numpy as np

MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit words (held in uint64) -> (x0, x1, x2, x3)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & MASK, np.uint64(k1) & MASK
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & MASK
        k1 = (k1 + np.uint64(0xBB67AE85)) & MASK
    return c


def uniform(hi, lo):
    k = ((hi << np.uint64(32)) | lo) >> np.uint64(11)
    return k.astype(np.float64) * 2.0 ** -53 + 2.0 ** -54


def alias_table(lib, w):
    w = np.ascontiguousarray(w, dtype=np.float64)
    prob = np.empty(len(w))
    alias = np.empty(len(w), dtype=np.int32)
    rc = lib.cb_sim_alias_table(len(w), w.ctypes.data, prob.ctypes.data, alias.ctypes.data)
    assert rc == 0, lib.cb_last_error()
    return prob, alias


def alias_draw(prob, alias, n, row_off, u):
    x = u * float(n)
    k = np.minimum(x.astype(np.int64), n - 1)
    take = (x - k) < prob[row_off + k]
    return np.where(take, k, alias[row_off + k])


def model_tables(lib, Q, pi):
    """(prob [S*S], alias [S*S], exit [S], pi_prob, pi_alias): what cb_sim_model_create builds."""
    Q = np.asarray(Q, dtype=np.float64)
    S = Q.shape[0]
    prob, alias = np.zeros(S * S), np.zeros(S * S, dtype=np.int64)
    for s in range(S):
        w = Q[s].copy()
        w[s] = 0.0
        if w.sum() > 0:
            p, a = alias_table(lib, w)
            prob[s * S:(s + 1) * S], alias[s * S:(s + 1) * S] = p, a
        else:
            alias[s * S:(s + 1) * S] = s
    pp, pa = alias_table(lib, pi)
    return prob, alias, -np.diag(Q).copy(), pp, pa.astype(np.int64)


def simulate_family(t1, t2, S1, fam):
    """fam: the dict Simulator.run takes.  t1 / t2: model_tables of the single / pair model (t2 may be None).
    -> int8 codes [n_nodes][n_sites]."""
    seed = int(fam["seed"]) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    sa, sb = np.asarray(fam["site_a"]), np.asarray(fam["site_b"])
    rate = np.asarray(fam["rate"], dtype=np.float64)
    parent, length = np.asarray(fam["parent"]), np.asarray(fam["length"], dtype=np.float64)
    U, L, nn = len(sa), int(fam["n_sites"]), len(parent)
    out = np.zeros((nn, L), dtype=np.int8)
    u = np.arange(U, dtype=np.uint64)
    pair = sb >= 0
    groups = [(~pair, t1, S1)] + ([(pair, t2, S1 * S1)] if pair.any() else [])
    zero = np.zeros(U, dtype=np.uint64)
    x = philox4x32_10(u, zero, zero, zero, k0, k1)
    a = uniform(x[1], x[0])
    state = np.zeros(U, dtype=np.int64)
    for m, (prob, alias, ex, pp, pa), n in groups:
        state[m] = alias_draw(pp, pa, n, 0, a[m])

    def put(v, s):
        out[v, sa[~pair]] = s[~pair]
        out[v, sa[pair]] = s[pair] // S1
        out[v, sb[pair]] = s[pair] % S1

    put(0, state)
    for v in range(1, nn):
        p = parent[v]
        s = out[p, sa].astype(np.int64)
        s[pair] = s[pair] * S1 + out[p, sb[pair]].astype(np.int64)
        elapsed = length[v] * rate
        for m, (prob, alias, ex, pp, pa), n in groups:
            idx = np.flatnonzero(m)
            cur, t = s[idx], np.zeros(len(idx))
            j = 0
            while len(idx):
                jj = np.full(len(idx), j, dtype=np.uint64)
                x = philox4x32_10(u[idx], np.full(len(idx), v, dtype=np.uint64), jj, np.zeros(len(idx), dtype=np.uint64),
                                  k0, k1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    w = -np.log(uniform(x[1], x[0])) / ex[cur]
                go = (t + w) < elapsed[idx]
                s[idx[~go]] = cur[~go]
                idx, cur, t, x3, x2 = idx[go], cur[go], (t + w)[go], x[3][go], x[2][go]
                cur = alias_draw(prob, alias, n, cur * n, uniform(x3, x2))
                j += 1
        put(v, s)
    return out


def c_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)
