"""Python face of cb_coscan_* (csrc/coscan.hip.h): which pairs of sites of a family co-evolve.  For every site pair i < j the
log-likelihood of the family's counted sequence pairs (the very pairs `count_co_transitions` walks: counting._host.build_pairs)
under the pair model expm(t_q Q_2) minus their log-likelihood under the product of two single-site models expm(t_q Q_1), over
exactly the terms the counter adds for the contact list {(i, j)}.  `CoevolutionScanner` keeps both log banks on the device;
`coevolution_scan` is the stage (one `<family>.npz` and one ranked `<family>.txt` per family).  There is no CPU fallback."""
import ctypes
import logging
import os
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from .. import _lib, caching
from ..counting import _host
from ..counting._stage import PAIR_DTYPE, _device_index, _my_families, _normalise_mode
from ..io import read_rate_matrix

_KEYS = ("score", "pair_ll", "indep_ll", "n_used", "apc")
_HEADER = "i j score apc n_used"


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _check(rc: int, what: str):
    """every refusal of the scan is a CherryBankError that carries the library's text (it names the offending value)"""
    if rc != 0:
        raise _lib.CherryBankError(f"{what} failed ({rc}): {_lib.load().cb_last_error().decode('utf-8', 'replace')}")


def _require_device(what: str):
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError(f"{what}: no HIP device visible; the scan runs on the MI355X only (no CPU fallback)")


def average_product_correction(score: np.ndarray) -> np.ndarray:
    """apc[i,j] = score[i,j] - m_i m_j / m with m_i the mean of score[i,k] over k != i and m the mean over all i != j; the
    diagonal stays 0; m == 0 (or fewer than two sites): apc = score"""
    score = _f64(score)
    L = score.shape[0]
    if L < 2:
        return score.copy()
    off = score - np.diag(np.diag(score))
    m_i = off.sum(axis=1) / (L - 1)
    m = off.sum() / (L * (L - 1))
    if m == 0:
        return score.copy()
    apc = score - np.outer(m_i, m_i) / m
    np.fill_diagonal(apc, 0.0)
    return apc


class CoevolutionScanner(_lib.ResidentHandle):
    """The two log banks log expm(grid[q] Q_1) [B][S][S] and log expm(grid[q] Q_2) [B][S^2][S^2] resident on the device
    (`cb_coscan_create` / `_run` / `_destroy`; 2 <= S <= 20, B >= 2).  `pi_1` / `pi_2`: the stationary distribution of a
    reversible Q_1 / Q_2 (the bank's spectral path); None: scaling and squaring, any rate matrix."""
    _destroy = "cb_coscan_destroy"

    def __init__(self, Q_1, Q_2, grid, pi_1=None, pi_2=None, device: Optional[int] = None):
        Q_1, Q_2, grid = _f64(Q_1), _f64(Q_2), _f64(grid).reshape(-1)
        if Q_1.ndim != 2 or Q_1.shape[0] != Q_1.shape[1]:
            raise ValueError(f"CoevolutionScanner: Q_1 must be square (got {Q_1.shape})")
        self.S, self.B = Q_1.shape[0], grid.size
        if Q_2.shape != (self.S ** 2, self.S ** 2):
            raise ValueError(f"CoevolutionScanner: Q_2 must be [{self.S ** 2}, {self.S ** 2}] (got {Q_2.shape})")
        pi_1 = None if pi_1 is None else _f64(pi_1).reshape(-1)
        pi_2 = None if pi_2 is None else _f64(pi_2).reshape(-1)
        if (pi_1 is not None and pi_1.size != self.S) or (pi_2 is not None and pi_2.size != self.S ** 2):
            raise ValueError("CoevolutionScanner: pi_1 must be [S] and pi_2 [S^2]")
        _require_device("CoevolutionScanner")
        self.device = _device_index() if device is None else int(device)
        self.grid = grid
        self.last_kernel_ms = 0.0
        h = ctypes.c_void_p()
        _check(_lib.load().cb_coscan_create(self.device, self.S, self.B, grid.ctypes.data, Q_1.ctypes.data,
                                            None if pi_1 is None else pi_1.ctypes.data, Q_2.ctypes.data,
                                            None if pi_2 is None else pi_2.ctypes.data, ctypes.byref(h)), "cb_coscan_create")
        self._h = h

    def scan_records(self, n_sites: Sequence[int], seqs: Sequence[np.ndarray], pairs: Sequence[np.ndarray],
                     symmetric: bool = True) -> List[Dict[str, np.ndarray]]:
        """The families as `counting._stage._gather` leaves them: family f has n_sites[f] sites, the int8 codes `seqs[f]`
        (flat) and the `cb_count_pair` records `pairs[f]` whose seq_a / seq_b are byte offsets into seqs[f]."""
        h = self._handle()
        if len(n_sites) == 0:
            return []
        L = np.ascontiguousarray(n_sites, dtype=np.int32)
        chunks, recs, off = [], [], 0
        for s, p in zip(seqs, pairs):
            s = np.ascontiguousarray(s, dtype=np.int8).reshape(-1)
            p = np.array(p, dtype=PAIR_DTYPE)
            p["seq_a"] += off
            p["seq_b"] += off
            chunks.append(s), recs.append(p)
            off += s.size
        flat = np.ascontiguousarray(np.concatenate(chunks)) if chunks else np.zeros(0, np.int8)
        rec = np.ascontiguousarray(np.concatenate(recs)) if recs else np.zeros(0, PAIR_DTYPE)
        n_pairs = np.array([len(p) for p in recs], dtype=np.int64)
        n_out = int((L.astype(np.int64) ** 2).clip(min=0).sum())
        out = [np.empty(n_out) for _ in range(3)]
        used, ms = np.empty(n_out, dtype=np.int32), np.zeros(1)
        _check(_lib.load().cb_coscan_run(h, len(L), L.ctypes.data, flat.ctypes.data, flat.size, rec.ctypes.data,
                                         n_pairs.ctypes.data, int(bool(symmetric)), out[0].ctypes.data, out[1].ctypes.data,
                                         out[2].ctypes.data, used.ctypes.data, ms.ctypes.data), "cb_coscan_run")
        self.last_kernel_ms = float(ms[0])
        res, o = [], 0
        for n in L.tolist():
            cut = lambda a: a[o:o + n * n].reshape(n, n).copy()   # noqa: E731
            res.append(dict(score=cut(out[0]), pair_ll=cut(out[1]), indep_ll=cut(out[2]), n_used=cut(used)))
            o += n * n
        return res

    def scan(self, seqs_by_family: Sequence[np.ndarray], pairs_by_family: Sequence[Sequence], symmetric: bool = True
             ) -> List[Dict[str, np.ndarray]]:
        """Per family `score`, `pair_ll`, `indep_ll` (float64 [L, L]) and `n_used` (int32 [L, L]).  seqs_by_family[f]: int8 codes
        [n_sequences, L] (state index, -1 = a gap); pairs_by_family[f]: (row a, row b, len_a, len_b) per sequence pair -- rows
        of seqs_by_family[f], the pair's length is len_a + len_b (what `build_pairs` returns, on rows).  `symmetric`: the
        cherry modes (four terms, weight 0.25); False: `edge` (two terms, weight 0.5)."""
        n_sites, flat, recs = [], [], []
        for f, (codes, prs) in enumerate(zip(seqs_by_family, pairs_by_family)):
            codes = np.ascontiguousarray(codes, dtype=np.int8)
            if codes.ndim != 2:
                raise ValueError(f"CoevolutionScanner.scan: family {f}: codes must be [n_sequences, L] (got {codes.shape})")
            n, L = codes.shape
            rec = np.zeros(len(prs), dtype=PAIR_DTYPE)
            for k, (a, b, la, lb) in enumerate(prs):
                if not (0 <= int(a) < n and 0 <= int(b) < n):
                    raise ValueError(f"CoevolutionScanner.scan: family {f} pair {k}: rows ({a}, {b}) of {n} sequences")
                rec[k] = (int(a) * L, int(b) * L, 0, 0, 0, la, lb)
            n_sites.append(L), flat.append(codes.reshape(-1)), recs.append(rec)
        return self.scan_records(n_sites, flat, recs, symmetric)


def _is_reversible(Q: np.ndarray, pi: np.ndarray) -> bool:
    F = pi[:, None] * Q
    return bool(np.all(pi > 0) and np.abs(F - F.T).max() <= 1e-9 * np.abs(F).max())


def _write_family(out_dir: str, family: str, res: Dict[str, np.ndarray], min_dist: int):
    res = dict(res, apc=average_product_correction(res["score"]))
    tmp = os.path.join(out_dir, family + ".npz.tmp")
    with open(tmp, "wb") as f:
        np.savez(f, **{k: res[k] for k in _KEYS})
    os.replace(tmp, os.path.join(out_dir, family + ".npz"))
    i, j = np.nonzero(np.triu(res["n_used"] > 0, max(int(min_dist), 1)))
    order = np.lexsort((j, i, -res["apc"][i, j]))   # apc descending, then (i, j)
    tmp = os.path.join(out_dir, family + ".txt.tmp")
    with open(tmp, "w") as f:
        f.write(_HEADER + "\n")
        for a, b in zip(i[order].tolist(), j[order].tolist()):
            f.write(f"{a} {b} {float(res['score'][a, b])!r} {float(res['apc'][a, b])!r} {int(res['n_used'][a, b])}\n")
    os.replace(tmp, os.path.join(out_dir, family + ".txt"))


def read_coevolution_scan(output_scan_dir: str, family: str) -> Dict[str, np.ndarray]:
    """What `coevolution_scan` wrote for a family: `score`, `pair_ll`, `indep_ll`, `n_used`, `apc` ([L, L]) and `ranking`, the
    rows of `<family>.txt` as a structured array (i, j, score, apc, n_used)."""
    with np.load(os.path.join(output_scan_dir, family + ".npz")) as z:
        out = {k: z[k] for k in _KEYS}
    dt = np.dtype([("i", "<i4"), ("j", "<i4"), ("score", "<f8"), ("apc", "<f8"), ("n_used", "<i4")])
    with open(os.path.join(output_scan_dir, family + ".txt")) as f:
        lines = f.read().splitlines()
    if not lines or lines[0] != _HEADER:
        raise Exception(f"{family}.txt: expected the header {_HEADER!r}")
    rows = [ln.split(" ") for ln in lines[1:] if ln]
    out["ranking"] = np.array([(int(r[0]), int(r[1]), float(r[2]), float(r[3]), int(r[4])) for r in rows], dtype=dt)
    return out


def _family_records(tree_dir: str, msa_dir: str, family: str, amino_acids: List[str], mode: str):
    """One family as `cb_coscan_run` takes it, from the files the counting stages read: the int8 codes of the sequences its
    pairs name (flat), its site count (from the alignment, also when no pair is counted) and the `cb_count_pair` records of
    `build_pairs` -- the pairing, encoding and record layout of `counting._stage._gather`, without an auxiliary file."""
    names, children, root = _host.read_tree_arrays(os.path.join(tree_dir, family + ".txt"))
    msa = _host.read_msa(os.path.join(msa_dir, family + ".txt"))
    L = len(next(iter(msa.values()))) if msa else 0
    pairs = _host.build_pairs(children, root, mode)
    used = sorted({p[0] for p in pairs} | {p[1] for p in pairs})
    row_of = {u: r for r, u in enumerate(used)}
    codes = _host.encode_msa(msa, [names[u] for u in used], amino_acids) if used else np.zeros((0, L), dtype=np.int8)
    rec = np.array([(row_of[a] * L, row_of[b] * L, 0, 0, 0, la, lb) for a, b, la, lb in pairs], dtype=PAIR_DTYPE)
    return np.ascontiguousarray(codes.reshape(-1)), L, rec


@caching.cached_computation(exclude_args=["num_processes"], output_dirs=["output_scan_dir"], write_extra_log_files=True,
                            collective=True)
def coevolution_scan(
    tree_dir: str,
    msa_dir: str,
    families: List[str],
    amino_acids: List[str],
    rate_matrix_path: str,
    coevolution_rate_matrix_path: str,
    quantization_points: List[Union[str, float]],
    edge_or_cherry: str = "cherry",
    minimum_distance_for_nontrivial_contact: int = 7,
    output_scan_dir: Optional[str] = None,
    num_processes: int = 1,
) -> None:
    """Scan every site pair of every family.  Per family `<family>.npz` (`score`, `pair_ll`, `indep_ll`, `n_used`, `apc`) and
    `<family>.txt`: under the header "i j score apc n_used" the pairs with j - i >= minimum_distance_for_nontrivial_contact and
    n_used > 0, by `apc` descending, then (i, j).  A rate matrix that satisfies detailed balance with its stationary distribution
    takes the bank's spectral path, any other scaling and squaring.  Under torch.distributed the families are dealt round-robin
    to the ranks as in the counting stages; every rank writes its own families and no rank waits for another (the decorator's
    `collective=True` only makes every rank run its share instead of rank 0 alone).  `num_processes` is accepted and
    ignored."""
    from ..evaluation._likelihood import _stationary_distribution
    _require_device("coevolution_scan")
    logging.getLogger(__name__).info(f"Starting on {len(families)} families")
    mode = _normalise_mode(edge_or_cherry)
    os.makedirs(output_scan_dir, exist_ok=True)
    grid = np.array(sorted(float(q) for q in quantization_points), dtype=np.float64)
    pairs_of_amino_acids = [a + b for a in amino_acids for b in amino_acids]
    Q_1_df, Q_2_df = read_rate_matrix(rate_matrix_path), read_rate_matrix(coevolution_rate_matrix_path)
    if list(Q_1_df.index) != list(amino_acids) or list(Q_1_df.columns) != list(amino_acids):
        raise Exception(f"Q_1 states are:\n{list(Q_1_df.index)}\n\nbut expected amino acids:\n{amino_acids}")
    if list(Q_2_df.index) != pairs_of_amino_acids or list(Q_2_df.columns) != pairs_of_amino_acids:
        raise Exception(f"Q_2 states are:\n{list(Q_2_df.index)}\n\nbut expected pairs of amino acids:\n{pairs_of_amino_acids}")
    Q_1, Q_2 = _f64(Q_1_df.to_numpy()), _f64(Q_2_df.to_numpy())
    pi_1, pi_2 = _stationary_distribution(Q_1), _stationary_distribution(Q_2)
    chunk = 32
    mine = _my_families(families)
    with CoevolutionScanner(Q_1, Q_2, grid, pi_1 if _is_reversible(Q_1, pi_1) else None,
                            pi_2 if _is_reversible(Q_2, pi_2) else None) as scanner:
        for c0 in range(0, len(mine), chunk):
            fams, n_sites, seqs, recs = mine[c0:c0 + chunk], [], [], []
            for fam in fams:
                s, L, p = _family_records(tree_dir, msa_dir, fam, amino_acids, mode)
                n_sites.append(L), seqs.append(s), recs.append(p)
            live = [k for k, L in enumerate(n_sites) if L >= 1 and len(recs[k]) > 0]
            res = scanner.scan_records([n_sites[k] for k in live], [seqs[k] for k in live], [recs[k] for k in live],
                                       symmetric=mode != "edge")
            by_k = dict(zip(live, res))
            for k, fam in enumerate(fams):
                L = max(n_sites[k], 0)
                empty = dict(score=np.zeros((L, L)), pair_ll=np.zeros((L, L)), indep_ll=np.zeros((L, L)),
                             n_used=np.zeros((L, L), dtype=np.int32))
                _write_family(output_scan_dir, fam, by_k.get(k, empty), minimum_distance_for_nontrivial_contact)
