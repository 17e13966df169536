"""Local branch supports on fixed trees (csrc/sup.hip.h, `cb_bl_supports`).

The edge above an internal non-root node v is judged against its nearest-neighbour interchanges -- the moves (v, c, s) of
`_nni.py` -- at the tree's own lengths.  With delta_m the log-likelihood gain of neighbour m (`nni_scan`'s delta) and
delta_m^r the same sum over a resample r of the sites (drawn with replacement, the same resample for every edge of a family):

    alrt = -2 max_m delta_m             the approximate likelihood-ratio statistic; negative where a neighbour beats the tree
    rell = share of the resamples in which no neighbour beats the tree (max_m delta_m^r <= 0)
    sh   = share of the resamples with -max_m delta_m > t^r, where t^r is the largest minus the second largest of 0 and the
           centred values delta_m^r - delta_m: the SH-like support of Guindon et al. (2010), centred at the exact expectation of
           the resample and not at the replicates' mean.  An edge with alrt <= 0 gets 0.

`BranchLengthFitter.branch_supports` forms them on the GPU from the scan's per-site log-likelihoods, which never leave the
device; `ml_branch_supports` is the stage on tree / MSA / site-rate directories, and `ml_nni_trees` / `nj_nni_trees` write the
supports of their final trees on request.  This is not FastTree's arithmetic (its SH-like test resamples the three topologies
around an edge with its own constants), and the neighbours keep the tree's lengths: PhyML's aLRT re-optimises them.

Felsenstein's bootstrap (rebuilding trees per replicate) is `_bootstrap.py`.  Out of scope: re-optimising lengths per neighbour,
supports under the 400-state model or S > 32, writing supports into the tree file format."""
import os
import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from .. import _lib
from ..caching import cached_computation
from ..io._tree import read_tree
from ._fast_cherries import quantization_points_ble
from ._ml_lengths import DEFAULT_MAX_BANK_BYTES, BranchLengthFitter, _batches

HEADER = "node alrt sh rell\n"


def write_supports(path: str, names: Sequence[str], result) -> None:
    """`<header>` and per internal non-root node, in `tree.nodes()` order, `name alrt sh rell`; `names` = `tree.nodes()`,
    `result` = one family's (nodes, alrt, sh, rell) of `branch_supports`"""
    nodes, alrt, sh, rell = result[:4]
    with open(path, "w") as fh:
        fh.write(HEADER + "".join(f"{names[int(v)]} {float(a)!r} {float(s)!r} {float(r)!r}\n"
                                  for v, a, s, r in zip(nodes, alrt, sh, rell)))


def read_supports(path: str) -> Dict[str, tuple]:
    """{node: (alrt, sh, rell)} of a file `write_supports` wrote"""
    lines = open(path).read().split("\n")
    if lines[0] + "\n" != HEADER:
        raise ValueError(f"{path}: not a branch-support file (header {lines[0]!r})")
    return {x[0]: (float(x[1]), float(x[2]), float(x[3])) for x in (ln.split() for ln in lines[1:] if ln)}


def support_seeds(families: Sequence[str], random_seed: int) -> List[int]:
    """the families' resampling seeds: `simulate_msas`' per-family seed, so a family's supports do not depend on its batch"""
    from ..simulation._simulate import family_seed
    return [family_seed(f, random_seed) for f in families]


def supports_of_trees(trees, codes, rates, grid, Q, pi_root, seeds, num_replicates: int, device, max_bank_bytes: int):
    """`branch_supports` of every tree as it is (no EM round), in handles under `max_bank_bytes` ->
    (per family (nodes, alrt, sh, rell), per family its profile)"""
    bank_bytes = [2 * len(grid) * np.unique(r).size * Q.size * 8 for r in rates]
    results: List[Optional[tuple]] = [None] * len(trees)
    profs: List[Dict[str, float]] = [{} for _ in trees]
    for batch in _batches(bank_bytes, int(max_bank_bytes)):
        st = time.time()
        with BranchLengthFitter([trees[f] for f in batch], [codes[f] for f in batch], [rates[f] for f in batch], grid, Q, pi_root,
                                device=device) as fit:
            t_create = time.time() - st
            st_sup = time.time()
            out = fit.branch_supports(num_replicates=num_replicates, seeds=[seeds[f] for f in batch])
            t_sup = time.time() - st_sup
            ms = fit.last_support_kernel_ms
        for k, f in enumerate(batch):
            results[f] = out[k]
            profs[f] = dict(create_time=t_create / len(batch), support_time=t_sup / len(batch), passes_kernel_ms=ms[0] / len(batch),
                            scan_kernel_ms=ms[1] / len(batch), resampling_kernel_ms=ms[2] / len(batch))   # (shares of the batch)
    return results, profs


@cached_computation(output_dirs=["output_support_dir"], exclude_args=["max_bank_bytes"])
def ml_branch_supports(tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str,
                       num_replicates: int = 1000, random_seed: int = 0, quantization_grid_center: float = 0.03,
                       quantization_grid_step: float = 1.1, quantization_grid_num_steps: int = 64,
                       output_support_dir: Optional[str] = None, max_bank_bytes: int = DEFAULT_MAX_BANK_BYTES, _version="1") -> None:
    """aLRT, SH-like and RELL support of every internal edge of `<tree_dir>/<family>.txt` under the rate matrix (root
    distribution = its stationary distribution) at the family's site rates, from `num_replicates` site resamples seeded by
    `simulation.family_seed(family, random_seed)`.  No EM round runs: the tree is taken as it is, its lengths snapped to the
    grid (center, step, num_steps) by the handle -- exact for the trees `ml_branch_lengths`, `ml_nni_trees` and
    `ml_lengths_and_site_rates` write on the same grid.  Per family:
    `<output_support_dir>/<family>.txt`: the header `node alrt sh rell`, then one line per internal non-root node in
    `tree.nodes()` order, `name alrt sh rell` (the support of the edge above it; sh and rell are shares of the replicates);
    `<output_support_dir>/<family>.profiling`.
    All families go in one handle unless their banks would exceed `max_bank_bytes`; then in batches in family order -- families
    are independent and each has its own seed, so the results do not depend on the batching."""
    from ..counting._host import read_msa, read_site_rates
    from ..counting._stage import _device_index
    from ..evaluation._likelihood import _family_units, _stationary_distribution
    from ..io import read_rate_matrix
    if output_support_dir is None:
        raise ValueError("output_support_dir is required")
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError("ml_branch_supports: no HIP device visible; the supports are computed on the MI355X only "
                                   "(no CPU fallback)")
    st_all = time.time()
    os.makedirs(output_support_dir, exist_ok=True)
    rm = read_rate_matrix(rate_matrix_path)
    alphabet = [str(c) for c in rm.columns]
    Q = np.ascontiguousarray(rm.to_numpy(), dtype=np.float64)
    pi_root = _stationary_distribution(Q)
    grid = np.array(quantization_points_ble(quantization_grid_center, quantization_grid_step, quantization_grid_num_steps))
    trees, rates, codes = [], [], []
    for family in families:
        tree = read_tree(os.path.join(tree_dir, family + ".txt"))
        msa = read_msa(os.path.join(msa_dir, family + ".txt"))
        r = np.asarray(read_site_rates(os.path.join(site_rates_dir, family + ".txt")), dtype=np.float64)
        trees.append(tree), rates.append(r)
        codes.append(_family_units(tree, msa, None, len(r), alphabet, False)[2])
    results, profs = supports_of_trees(trees, codes, rates, grid, Q, pi_root, support_seeds(families, random_seed),
                                       int(num_replicates), _device_index(), max_bank_bytes)
    t_total = (time.time() - st_all) / max(len(families), 1)
    for f, family in enumerate(families):
        write_supports(os.path.join(output_support_dir, family + ".txt"), list(trees[f].nodes()), results[f])
        with open(os.path.join(output_support_dir, family + ".profiling"), "w") as fh:
            fh.write("".join(f"{k}: {v}\n" for k, v in profs[f].items()) + f"total_time: {t_total}")
