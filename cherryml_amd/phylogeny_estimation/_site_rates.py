"""Maximum-likelihood site rates on fixed full trees: every site at every candidate rate, on the GPU (csrc/sr.hip.h,
`cb_tree_site_rates`).

The tree, its lengths, the rate matrix and the root distribution are fixed; a site's rate is one of the family's candidates, and
candidate c puts expm(length x candidate x Q) on every edge.  `tree_site_rates` is the in-memory call, `ml_site_rates` the stage on
tree / MSA / site-rate directories (candidates: the `num_rate_categories` offered categories united with the rates of the input
file; a site moves only to a strictly better rate), `ml_lengths_and_site_rates` alternates the branch-length EM of `_ml_lengths.py`
with the scan, and `nj_ml_rates_trees` is the tree estimator `nj_trees` + `ml_lengths_and_site_rates`.

Rates are written as picked, with no mean-rate normalisation: every consumer reads length x rate only, and the lengths stay where
the length fit put them.

Out of scope: Gamma or mixture marginal likelihoods, continuous rates (outside a candidate list), the 400-state pair model and
S > 32, topology moves."""
import ctypes
import os
import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from .. import _lib
from ..caching import cached_computation
from ..io._tree import Tree, read_tree, write_tree
from ._fast_cherries import quantization_points_ble, rate_categories_ble
from ._ml_lengths import DEFAULT_MAX_BANK_BYTES, BranchLengthFitter, _batches

MAX_CANDIDATES = 64   # CB_SR_MAX_CANDS; also CB_BL_MAX_CATS, the fitter's bound on a family's distinct rates


def _scan(device, S, Q, pi_root, n_nodes, parent, length, n_units, codes, n_cands, cands, current, return_all):
    """the ctypes call on concatenated arrays -> (best, best_ll, ll_all or None, (bank ms, scan + pick ms))"""
    best = np.empty(int(n_units.sum()), dtype=np.int32)
    best_ll = np.empty(best.size)
    ll_all = np.empty(int((n_cands.astype(np.int64) * n_units).sum())) if return_all else None
    ms = (ctypes.c_double * 2)(0.0, 0.0)
    rc = _lib.load().cb_tree_site_rates(device, S, Q.ctypes.data, pi_root.ctypes.data, n_nodes.size, n_nodes.ctypes.data,
                                        parent.ctypes.data, length.ctypes.data, n_units.ctypes.data, codes.ctypes.data,
                                        n_cands.ctypes.data, cands.ctypes.data, None if current is None else current.ctypes.data,
                                        best.ctypes.data, best_ll.ctypes.data, None if ll_all is None else ll_all.ctypes.data,
                                        ctypes.addressof(ms))
    _lib.check(rc, "cb_tree_site_rates")
    return best, best_ll, ll_all, (ms[0], ms[1])


def tree_site_rates(trees: Sequence, leaf_codes: Sequence[np.ndarray], candidates: Sequence, current: Optional[Sequence], Q, pi_root,
                    device: Optional[int] = None, return_all: bool = False, profile: Optional[dict] = None) -> List[tuple]:
    """The ML candidate of every site of every family -> per family (best [n_sites] int32, best_ll [n_sites]) and, with
    `return_all`, the log-likelihoods [n_cands, n_sites] as a third member.

    trees: `io.Tree`s (any lengths >= 0); leaf_codes: per family int8 [n_nodes, n_sites], rows in `tree.nodes()` order (-1 = gap;
    only leaf rows are read); candidates: one list for all families or one list per family, strictly increasing, finite, > 0, at
    most 64; current: None, or per family the sites' present candidate indices (-1: none) -- among exactly equal maxima a site
    keeps it, and a site with fewer than two observed leaves always does (candidate 0 without one); Q [S, S], pi_root [S],
    2 <= S <= 32.  profile: a dict that receives `bank_kernel_ms` and `scan_kernel_ms`."""
    from ..counting._stage import _device_index
    from ..evaluation._likelihood import _pack_forest
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    pi_root = np.ascontiguousarray(pi_root, dtype=np.float64).reshape(-1)
    S = Q.shape[0]
    if Q.ndim != 2 or Q.shape != (S, S) or pi_root.shape != (S,):
        raise ValueError(f"tree_site_rates: Q must be square and pi_root of its size: {Q.shape}, {pi_root.shape}")
    n_fam = len(trees)
    if n_fam == 0 or len(leaf_codes) != n_fam or (current is not None and len(current) != n_fam):
        raise ValueError("tree_site_rates: need one tree, one code array and (with `current`) one index array per family "
                         "(at least one family)")
    if len(candidates) == 0:
        raise ValueError("tree_site_rates: no candidates")
    if np.ndim(candidates[0]) == 0:
        candidates = [candidates] * n_fam
    if len(candidates) != n_fam:
        raise ValueError(f"tree_site_rates: {len(candidates)} candidate lists for {n_fam} families")
    n_nodes, n_units, parent, length, _, codes = _pack_forest("tree_site_rates", trees, leaf_codes, None)
    cands, cur = [], []
    for f, cd in enumerate(candidates):
        cd = np.asarray(cd, dtype=np.float64)
        if cd.ndim != 1 or cd.size < 1:
            raise ValueError(f"tree_site_rates: family {f}: candidates must be a non-empty list of rates")
        if current is not None:
            k = np.asarray(current[f])
            if k.shape != (n_units[f],) or not np.issubdtype(k.dtype, np.integer):
                raise ValueError(f"tree_site_rates: family {f}: current must be [n_sites] integer indices (got {k.shape}, {k.dtype})")
            cur.append(k)
        cands.append(cd)
    n_cands = np.array([cd.size for cd in cands], dtype=np.int32)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dtype=dt)   # noqa: E731
    device = _device_index() if device is None else int(device)
    best, best_ll, ll_all, ms = _scan(device, S, Q, pi_root, n_nodes, parent, length, n_units, codes, n_cands,
                                      cat(cands, np.float64), cat(cur, np.int32) if current is not None else None, bool(return_all))
    if profile is not None:
        profile["bank_kernel_ms"], profile["scan_kernel_ms"] = ms
    cut = np.cumsum(n_units)[:-1]
    out = list(zip(np.split(best, cut), np.split(best_ll, cut)))
    if return_all:
        cut_all = np.cumsum(n_cands.astype(np.int64) * n_units)[:-1]
        out = [(b, l, a.reshape(int(c), int(u))) for (b, l), a, c, u in zip(out, np.split(ll_all, cut_all), n_cands, n_units)]
    return out


def _candidates(num_rate_categories: int, rates: np.ndarray, family: str) -> np.ndarray:
    """the offered categories united with the distinct rates of the family, ascending; at most 64"""
    cands = np.unique(np.concatenate([np.asarray(rate_categories_ble(num_rate_categories), dtype=np.float64), rates]))
    if cands.size > MAX_CANDIDATES:
        raise ValueError(f"family {family}: {num_rate_categories} offered categories and {np.unique(rates).size} distinct input rates "
                         f"make {cands.size} candidates (at most {MAX_CANDIDATES})")
    if not (np.all(np.isfinite(cands)) and cands[0] > 0.0):
        raise ValueError(f"family {family}: site rates must be finite and > 0")
    return cands


def _load(tree_dir, msa_dir, site_rates_dir, families, rate_matrix_path, num_rate_categories):
    """the stages' inputs: model, per family tree, MSA, rates, leaf codes, candidates and the rates' indices among them"""
    from ..counting._host import read_msa, read_site_rates
    from ..evaluation._likelihood import _family_units, _stationary_distribution
    from ..io import read_rate_matrix
    rm = read_rate_matrix(rate_matrix_path)
    alphabet = [str(c) for c in rm.columns]
    Q = np.ascontiguousarray(rm.to_numpy(), dtype=np.float64)
    fams = []
    for family in families:
        tree = read_tree(os.path.join(tree_dir, family + ".txt"))
        msa = read_msa(os.path.join(msa_dir, family + ".txt"))
        r = np.asarray(read_site_rates(os.path.join(site_rates_dir, family + ".txt")), dtype=np.float64)
        cands = _candidates(num_rate_categories, r, family)
        fams.append(dict(tree=tree, msa=msa, codes=_family_units(tree, msa, None, len(r), alphabet, False)[2], cands=cands,
                         index=np.searchsorted(cands, r).astype(np.int32)))
    return alphabet, Q, _stationary_distribution(Q), fams


def _write_rates_and_likelihoods(families, fams, alphabet, Q, pi_root, device, output_site_rates_dir, output_likelihood_dir):
    """the site-rate files (the picked candidates, as `nj_trees` writes them) and the likelihood files at them -> seconds"""
    from ..evaluation._likelihood import dp_likelihood_computation_batch, write_log_likelihood
    st = time.time()
    rates = [[float(x) for x in F["cands"][F["index"]]] for F in fams]
    for family, r in zip(families, rates):
        with open(os.path.join(output_site_rates_dir, family + ".txt"), "w") as f:
            f.write(f"{len(r)} sites\n" + " ".join(repr(x) for x in r))
    lls = dp_likelihood_computation_batch([F["tree"] for F in fams], [F["msa"] for F in fams], [None] * len(fams), rates, alphabet,
                                          pi_root, Q, device=device)
    for family, ll in zip(families, lls):
        write_log_likelihood(ll, os.path.join(output_likelihood_dir, family + ".txt"))
    return time.time() - st


def _require_device(who: str) -> None:
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError(f"{who}: no HIP device visible; the scan runs on the MI355X only (no CPU fallback)")


@cached_computation(output_dirs=["output_site_rates_dir", "output_likelihood_dir"])
def ml_site_rates(tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str,
                  num_rate_categories: int, output_site_rates_dir: Optional[str] = None,
                  output_likelihood_dir: Optional[str] = None, _version="1") -> None:
    """Refit the site rates of `<site_rates_dir>/<family>.txt` on the full trees `<tree_dir>/<family>.txt` under the rate matrix.
    Per family the candidates are `rate_categories_ble(num_rate_categories)` united with the distinct rates of the input file (at
    most 64, or the family is refused); the site's input rate is its `current`, so a site only moves to a strictly better rate and
    no site's likelihood goes down.  Writes `<output_site_rates_dir>/<family>.txt` in the existing format (the picked candidates,
    no mean-rate normalisation), `<family>.profiling` beside it and `<output_likelihood_dir>/<family>.txt` as `nj_trees` writes it
    (`dp_likelihood_computation_batch` on the input trees at the written rates)."""
    from ..counting._stage import _device_index
    if output_site_rates_dir is None or output_likelihood_dir is None:
        raise ValueError("output_site_rates_dir and output_likelihood_dir are required")
    _require_device("ml_site_rates")
    st_all = time.time()
    for d in (output_site_rates_dir, output_likelihood_dir):
        os.makedirs(d, exist_ok=True)
    alphabet, Q, pi_root, fams = _load(tree_dir, msa_dir, site_rates_dir, families, rate_matrix_path, num_rate_categories)
    device = _device_index()
    prof: Dict[str, float] = {}
    st = time.time()
    res = tree_site_rates([F["tree"] for F in fams], [F["codes"] for F in fams], [F["cands"] for F in fams],
                          [F["index"] for F in fams], Q, pi_root, device=device, profile=prof)
    t_scan = time.time() - st
    changed = []
    for F, (best, _) in zip(fams, res):
        changed.append(int((best != F["index"]).sum()))
        F["index"] = best
    t_ll = _write_rates_and_likelihoods(families, fams, alphabet, Q, pi_root, device, output_site_rates_dir, output_likelihood_dir)
    n = max(len(families), 1)
    for family, F, ch in zip(families, fams, changed):
        with open(os.path.join(output_site_rates_dir, family + ".profiling"), "w") as f:   # (times: shares of the one call)
            f.write(f"candidates: {F['cands'].size}\nsites_changed: {ch}\nbank_kernel_ms: {prof['bank_kernel_ms'] / n}\n"
                    f"scan_kernel_ms: {prof['scan_kernel_ms'] / n}\nscan_time: {t_scan / n}\nlikelihood_time: {t_ll / n}\n"
                    f"total_time: {(time.time() - st_all) / n}")


@cached_computation(output_dirs=["output_tree_dir", "output_site_rates_dir", "output_likelihood_dir"], exclude_args=["max_bank_bytes"])
def ml_lengths_and_site_rates(tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str,
                              num_rate_categories: int, num_outer_iterations: int = 3, num_rounds: int = 10,
                              quantization_grid_center: float = 0.03, quantization_grid_step: float = 1.1,
                              quantization_grid_num_steps: int = 64, output_tree_dir: Optional[str] = None,
                              output_site_rates_dir: Optional[str] = None, output_likelihood_dir: Optional[str] = None,
                              max_bank_bytes: int = DEFAULT_MAX_BANK_BYTES, _version="1") -> None:
    """Alternate the branch-length EM (`BranchLengthFitter`, at most `num_rounds` rounds on the current trees and rates) with the
    rate scan (at the new lengths, the current rates as `current`), at most `num_outer_iterations` times; stops when an outer
    iteration changes no length index and no rate in any family.  Neither half lowers a family's likelihood.

    A family's candidates are fixed for the whole stage: the offered categories united with the distinct rates of its input file.
    Every rate the stage ever holds is one of them, so with R <= 32 offered categories and an input fitted on R categories the
    list, and with it the fitter's count of distinct rates, never passes 64; both are checked.

    Writes `<output_tree_dir>/<family>.txt` (topology, node names and order untouched, every length a grid point),
    `<family>.rounds` -- per outer iteration `<k> lengths <ll at start> <ll at end> <indices changed>` and `<k> rates <ll before>
    <ll after> <sites changed>` (both sums of the scan's own columns), then `final <ll>` --, `<family>.profiling`, the site-rate
    files and the likelihood files like the two stages it is made of."""
    from ..counting._stage import _device_index
    if output_tree_dir is None or output_site_rates_dir is None or output_likelihood_dir is None:
        raise ValueError("output_tree_dir, output_site_rates_dir and output_likelihood_dir are required")
    if int(num_outer_iterations) < 1:
        raise ValueError(f"num_outer_iterations = {num_outer_iterations} (at least 1)")
    _require_device("ml_lengths_and_site_rates")
    st_all = time.time()
    for d in (output_tree_dir, output_site_rates_dir, output_likelihood_dir):
        os.makedirs(d, exist_ok=True)
    alphabet, Q, pi_root, fams = _load(tree_dir, msa_dir, site_rates_dir, families, rate_matrix_path, num_rate_categories)
    grid = np.array(quantization_points_ble(quantization_grid_center, quantization_grid_step, quantization_grid_num_steps))
    device = _device_index()
    logs: List[List[str]] = [[] for _ in families]
    prof = dict(fit_time=0.0, scan_time=0.0, passes_kernel_ms=0.0, mstep_kernel_ms=0.0, bank_kernel_ms=0.0, scan_kernel_ms=0.0,
                rounds=0, outer_iterations=0)
    final = [0.0] * len(families)
    for k in range(int(num_outer_iterations)):
        prof["outer_iterations"] = k + 1
        moved = 0
        # 1. the lengths at the current rates
        st = time.time()
        rates = [F["cands"][F["index"]] for F in fams]
        n_distinct = [np.unique(r).size for r in rates]
        if max(n_distinct) > MAX_CANDIDATES:                    # (a subset of the candidates: cannot happen)
            raise ValueError(f"a family holds {max(n_distinct)} distinct site rates (at most {MAX_CANDIDATES})")
        bank_bytes = [2 * grid.size * d * Q.size * 8 for d in n_distinct]
        for batch in _batches(bank_bytes, int(max_bank_bytes)):
            with BranchLengthFitter([fams[f]["tree"] for f in batch], [fams[f]["codes"] for f in batch], [rates[f] for f in batch],
                                    grid, Q, pi_root, device=device) as fit:
                start = fit.indices()
                ll_start = None
                live = np.ones(len(batch), dtype=bool)
                for _ in range(int(num_rounds)):
                    if not live.any():
                        break
                    n_changed, fam_ll = fit.round()
                    ll_start = fam_ll if ll_start is None else ll_start
                    prof["rounds"] += 1
                    prof["passes_kernel_ms"] += fit.last_kernel_ms[0]
                    prof["mstep_kernel_ms"] += fit.last_kernel_ms[1]
                    live &= n_changed > 0
                end, lengths = fit.indices(), fit.lengths()
                _, ll_end = fit.log_likelihoods()
                ll_start = ll_end if ll_start is None else ll_start
            for j, f in enumerate(batch):
                changed = int((start[j] != end[j]).sum())
                moved += changed
                logs[f].append(f"{k} lengths {float(ll_start[j])!r} {float(ll_end[j])!r} {changed}\n")
                t = Tree()
                t.add_nodes(fams[f]["tree"].nodes())
                t.add_edges([(u, v, lengths[j][v]) for u, v, _ in fams[f]["tree"].edges()])
                fams[f]["tree"] = t
        prof["fit_time"] += time.time() - st
        # 2. the rates at the new lengths
        st = time.time()
        p: Dict[str, float] = {}
        res = tree_site_rates([F["tree"] for F in fams], [F["codes"] for F in fams], [F["cands"] for F in fams],
                              [F["index"] for F in fams], Q, pi_root, device=device, return_all=True, profile=p)
        prof["bank_kernel_ms"] += p["bank_kernel_ms"]
        prof["scan_kernel_ms"] += p["scan_kernel_ms"]
        for f, (F, (best, best_ll, ll_all)) in enumerate(zip(fams, res)):
            before = float(ll_all[F["index"], np.arange(best.size)].sum())
            changed = int((best != F["index"]).sum())
            moved += changed
            final[f] = float(best_ll.sum())
            logs[f].append(f"{k} rates {before!r} {final[f]!r} {changed}\n")
            F["index"] = best
        prof["scan_time"] += time.time() - st
        if moved == 0:
            break
    t_ll = _write_rates_and_likelihoods(families, fams, alphabet, Q, pi_root, device, output_site_rates_dir, output_likelihood_dir)
    n = max(len(families), 1)
    for f, family in enumerate(families):
        write_tree(fams[f]["tree"], os.path.join(output_tree_dir, family + ".txt"))
        with open(os.path.join(output_tree_dir, family + ".rounds"), "w") as fh:
            fh.write("".join(logs[f]) + f"final {final[f]!r}\n")
        with open(os.path.join(output_tree_dir, family + ".profiling"), "w") as fh:   # (times: shares of the stage)
            fh.write("".join(f"{key}: {v if key in ('rounds', 'outer_iterations') else v / n}\n" for key, v in prof.items())
                     + f"likelihood_time: {t_ll / n}\ntotal_time: {(time.time() - st_all) / n}")


def nj_ml_rates_trees(*, msa_dir: str, families: List[str], rate_matrix_path: str, num_rate_categories: int, max_iters: int = 50,
                      num_processes: int = 1, num_rounds: int = 10, num_outer_iterations: int = 3,
                      output_tree_dir: Optional[str] = None, output_site_rates_dir: Optional[str] = None,
                      output_likelihood_dir: Optional[str] = None, remake=False, quantization_grid_center=0.03,
                      quantization_grid_step=1.1, quantization_grid_num_steps=64, verbose=True, seed=1234,
                      joiner="host") -> Dict[str, str]:
    """`nj_trees`, then `ml_lengths_and_site_rates` on its trees and site rates and the same grid: `nj_ml_trees`' interface plus
    `num_outer_iterations`, and under `functools.partial` a `tree_estimator` of the end-to-end pipelines.  Returns the three output
    directories of the refit -- the site-rate directory is the refitted one.  Both stages are cached on their own.  With no cache
    directory the three output directories are required and `nj_trees`' own files go to their `nj_trees` subdirectories.
    `joiner` is `nj_trees`'."""
    from ..caching import get_cache_dir
    from ._nj import nj_trees
    nj_out = dict(output_tree_dir=None, output_site_rates_dir=None, output_likelihood_dir=None)
    out = dict(output_tree_dir=output_tree_dir, output_site_rates_dir=output_site_rates_dir, output_likelihood_dir=output_likelihood_dir)
    if get_cache_dir() is None:
        if None in out.values():
            raise ValueError("output_tree_dir, output_site_rates_dir and output_likelihood_dir are required without a cache directory")
        nj_out = {key: os.path.join(d, "nj_trees") for key, d in out.items()}
    grid_args = dict(quantization_grid_center=quantization_grid_center, quantization_grid_step=quantization_grid_step,
                     quantization_grid_num_steps=quantization_grid_num_steps)
    nj = nj_trees(msa_dir=msa_dir, families=families, rate_matrix_path=rate_matrix_path, num_rate_categories=num_rate_categories,
                  max_iters=max_iters, num_processes=num_processes, remake=remake, verbose=verbose, seed=seed, joiner=joiner, **grid_args,
                  **nj_out)
    nj = nj if nj is not None else nj_out
    ml = ml_lengths_and_site_rates(tree_dir=nj["output_tree_dir"], msa_dir=msa_dir, site_rates_dir=nj["output_site_rates_dir"],
                                   families=families, rate_matrix_path=rate_matrix_path, num_rate_categories=num_rate_categories,
                                   num_outer_iterations=num_outer_iterations, num_rounds=num_rounds, **grid_args, **out)
    return ml if ml is not None else out
