"""Marginal maximum-likelihood ancestral reconstruction on fixed trees (csrc/anc.hip.h, `cb_bl_ancestral`).

Under the rate matrix, the family's site rates and the tree's lengths, the posterior distribution of the state at a node given
ALL leaves of a site is the normalised product of the node's inside and outside messages.  `BranchLengthFitter.ancestral_states`
forms it on the GPU for every node of every family from the messages the handle's passes leave resident: the most probable state,
its posterior (the confidence) and, on request, the whole distribution -- at the root, at the internal nodes and at the leaves,
where an observed character is returned as it is and a gapped one is imputed.  `ml_ancestral_sequences` is the stage on tree /
MSA / site-rate directories; it writes an alignment with one row per tree node, as `simulate_msas` does for its truth.

Out of scope: joint (max-product) reconstruction, parsimony, sampling from the posterior, pair posteriors, continuous lengths,
S > 32."""
import os
import time
from typing import Dict, List, Optional

import numpy as np

from .. import _lib
from ..caching import cached_computation
from ..io._tree import read_tree
from ._fast_cherries import quantization_points_ble
from ._ml_lengths import DEFAULT_MAX_BANK_BYTES, BranchLengthFitter, _batches


@cached_computation(output_dirs=["output_msa_dir", "output_confidence_dir"], exclude_args=["max_bank_bytes"])
def ml_ancestral_sequences(tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str,
                           impute_gaps: bool = True, write_posteriors: bool = False, quantization_grid_center: float = 0.03,
                           quantization_grid_step: float = 1.1, quantization_grid_num_steps: int = 64,
                           output_msa_dir: Optional[str] = None, output_confidence_dir: Optional[str] = None,
                           max_bank_bytes: int = DEFAULT_MAX_BANK_BYTES, _version="1") -> None:
    """Reconstruct the sequence of every node of `<tree_dir>/<family>.txt` from the leaves in `<msa_dir>/<family>.txt` by
    marginal maximum likelihood under the rate matrix (root distribution = its stationary distribution) at the family's site
    rates.  No EM round runs: the tree is taken as it is, its lengths snapped to the grid (center, step, num_steps) by the
    handle -- which is exact for the trees `ml_branch_lengths`, `ml_nni_trees` and `ml_lengths_and_site_rates` write on the same
    grid, whose lengths are grid points.  Per family:
    `<output_msa_dir>/<family>.txt`: an alignment as `write_msa` writes it with a row for EVERY node of the tree, in
    `tree.nodes()` order (`simulate_msas` writes the same rows, sorted by name): an observed leaf character (a letter of the matrix's alphabet) is
    copied from the input, an internal node gets its most probable letter, a gapped leaf character (anything else) gets its
    most probable letter when `impute_gaps`, else `-`; a site that is impossible under the model is `-`.
    `<output_msa_dir>/<family>.profiling`.
    `<output_confidence_dir>/<family>.npz`: `nodes` (the rows' names), `alphabet`, `state` int8 [n_nodes, n_sites] (the most
    probable state, whatever `impute_gaps` says; -1: impossible), `confidence` float64 [n_nodes, n_sites] (its posterior) and,
    with `write_posteriors`, `posterior` float64 [n_nodes, n_sites, S].
    All families go in one handle unless their banks would exceed `max_bank_bytes`; then in batches in family order -- families
    are independent, so the results do not depend on the batching."""
    from ..counting._host import read_msa, read_site_rates
    from ..counting._stage import _device_index
    from ..evaluation._likelihood import _family_units, _stationary_distribution
    from ..io import read_rate_matrix
    if output_msa_dir is None or output_confidence_dir is None:
        raise ValueError("output_msa_dir and output_confidence_dir are required")
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError("ml_ancestral_sequences: no HIP device visible; the reconstruction runs on the MI355X only "
                                   "(no CPU fallback)")
    st_all = time.time()
    for d in (output_msa_dir, output_confidence_dir):
        os.makedirs(d, exist_ok=True)
    rm = read_rate_matrix(rate_matrix_path)
    alphabet = [str(c) for c in rm.columns]
    Q = np.ascontiguousarray(rm.to_numpy(), dtype=np.float64)
    pi_root = _stationary_distribution(Q)
    grid = np.array(quantization_points_ble(quantization_grid_center, quantization_grid_step, quantization_grid_num_steps))
    device = _device_index()
    trees, rates, codes = [], [], []
    for family in families:
        tree = read_tree(os.path.join(tree_dir, family + ".txt"))
        msa = read_msa(os.path.join(msa_dir, family + ".txt"))
        r = np.asarray(read_site_rates(os.path.join(site_rates_dir, family + ".txt")), dtype=np.float64)
        trees.append(tree), rates.append(r)
        codes.append(_family_units(tree, msa, None, len(r), alphabet, False)[2])
    bank_bytes = [2 * grid.size * np.unique(r).size * Q.size * 8 for r in rates]
    results: List[Optional[tuple]] = [None] * len(families)
    profs: List[Dict[str, float]] = [{} for _ in families]
    for batch in _batches(bank_bytes, int(max_bank_bytes)):
        st = time.time()
        with BranchLengthFitter([trees[f] for f in batch], [codes[f] for f in batch], [rates[f] for f in batch], grid, Q, pi_root,
                                device=device) as fit:
            t_create = time.time() - st
            st_rec = time.time()
            out = fit.ancestral_states(posteriors=bool(write_posteriors))
            t_rec = time.time() - st_rec
            ms = fit.last_ancestral_kernel_ms
        for k, f in enumerate(batch):
            results[f] = tuple(x[k] for x in out)
            profs[f] = dict(create_time=t_create / len(batch), reconstruction_time=t_rec / len(batch),
                            passes_kernel_ms=ms[0] / len(batch), reconstruction_kernel_ms=ms[1] / len(batch))   # (shares of the batch)
    letters = np.array(alphabet + ["-"])   # state -1 -> '-'
    if any(len(a) != 1 for a in alphabet):
        raise ValueError("ml_ancestral_sequences: the alphabet of the rate matrix must be single letters")
    t_total = (time.time() - st_all) / max(len(families), 1)
    for f, family in enumerate(families):
        state, conf = results[f][0], results[f][1]
        nodes = list(trees[f].nodes())
        leaf = np.array([trees[f].is_leaf(v) for v in nodes])[:, None]
        shown = np.where(leaf & (codes[f] >= 0), codes[f], state).astype(np.int64)   # an observed character: the input's
        if not impute_gaps:
            shown = np.where(leaf & (codes[f] < 0), -1, shown)
        rows = letters[shown]
        # write_msa's format, but the rows in tree.nodes() order (write_msa sorts the names)
        with open(os.path.join(output_msa_dir, family + ".txt"), "w") as fh:
            fh.write("".join(f">{v}\n{''.join(rows[i])}\n" for i, v in enumerate(nodes)))
        arrays = dict(nodes=np.array(nodes), alphabet=np.array(alphabet), state=state, confidence=conf)
        if write_posteriors:
            arrays["posterior"] = results[f][2]
        np.savez(os.path.join(output_confidence_dir, family + ".npz"), **arrays)
        with open(os.path.join(output_msa_dir, family + ".profiling"), "w") as fh:
            fh.write("".join(f"{k}: {v}\n" for k, v in profs[f].items()) + f"total_time: {t_total}")
