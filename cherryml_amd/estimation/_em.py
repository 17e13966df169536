"""Full-tree EM for the 20-state model: `em_lg` (reference: cherryml/estimation/_em_lg.py:251, which runs the Historian binary)
with its E-step on the GPU (csrc/em.hip.h, the resident `cb_em_*` handle) and its M-step by this package's optimiser.

Model: independent sites under Q at their site rates; every edge length x site rate is put on the quantisation grid, so the
complete-data log-likelihood is log pi_root(x_root) + sum_edges log P_{q(t r)}[x_parent, x_child].  The root distribution is
fixed for the whole run, so the M-step is CherryML's own objective sum_b sum_ab E_b[a, b] log expm(t_b Q)[a, b] with the
expected counts E_b in place of the cherry counts -- the existing optimiser, warm-started at the current Q.  Its best iterate
includes the starting point (strict <), so no iteration lowers the likelihood (a generalised EM)."""
import ctypes
import logging
import os
import time
import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import _lib, caching

DEFAULT_GRID = [0.03 * 1.1 ** i for i in range(-64, 65)]   # the reference pipeline's grid (center 0.03, step 1.1, +-64)


class EStep(_lib.ResidentHandle):
    """The E-step resident on one GPU: trees, leaf codes, site-rate categories and the accumulation's task lists are uploaded
    once (`cb_em_create`); each `expected_counts(Q, pi_root)` sends only Q and pi_root.

    trees: `io.Tree`s; leaf_codes: per family an int8 array [n_nodes, n_sites] with rows in `tree.nodes()` order (-1 = gap;
    only leaf rows are read); site_rates: per family [n_sites]; grid: the quantisation points (increasing).  A context
    manager; `close()` frees the handle."""
    _destroy = "cb_em_destroy"

    def __init__(self, trees: Sequence, leaf_codes: Sequence[np.ndarray], site_rates: Sequence, grid: Sequence[float],
                 device: Optional[int] = None, num_states: int = 20):
        from ..counting._stage import _device_index
        from ..evaluation._likelihood import _pack_forest
        self.grid = np.ascontiguousarray(np.asarray(grid, dtype=np.float64).reshape(-1))
        if len(trees) == 0 or len(trees) != len(leaf_codes) or len(trees) != len(site_rates):
            raise ValueError("EStep: need one tree, one code array and one site-rate vector per family (at least one family)")
        self.S = None
        self.n_nodes, self.n_units, *self._args = _pack_forest("EStep", trees, leaf_codes, site_rates)
        self._n_edges_sites = int(sum((int(n) - 1) * int(u) for n, u in zip(self.n_nodes, self.n_units)))
        self.device = _device_index() if device is None else int(device)
        self.last_kernel_ms = 0.0
        self.last_unit_loglik: Optional[List[np.ndarray]] = None
        self.last_family_loglik: Optional[np.ndarray] = None
        self._create(int(num_states))

    def _create(self, S: int) -> None:
        par, ln, rt, cd = self._args
        h = ctypes.c_void_p()
        rc = _lib.load().cb_em_create(self.device, S, self.grid.size, self.grid.ctypes.data, self.n_nodes.size,
                                      self.n_nodes.ctypes.data, par.ctypes.data, ln.ctypes.data, self.n_units.ctypes.data,
                                      rt.ctypes.data, cd.ctypes.data, ctypes.byref(h))
        _lib.check(rc, "cb_em_create")
        self._h, self.S = h, S

    @property
    def num_edge_sites(self) -> int:
        """(non-root nodes) x (sites), summed over the families: the total mass of the expected counts"""
        return self._n_edges_sites

    def expected_counts(self, Q, pi_root) -> Tuple[np.ndarray, float]:
        """-> (E [B, S, S], log-likelihood of all families).  E[b, x, y] is the posterior expected number of (parent state x,
        child state y) over the edges and sites whose length x rate falls in bucket b."""
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        pi = np.ascontiguousarray(pi_root, dtype=np.float64).reshape(-1)
        S = Q.shape[0]
        if Q.shape != (S, S) or pi.shape != (S,):
            raise ValueError(f"EStep: Q must be square and pi_root of its size: {Q.shape}, {pi.shape}")
        h = self._handle()
        if S != self.S:
            raise ValueError(f"EStep: made for {self.S} states, got {S}")
        E = np.empty((self.grid.size, S, S))
        ll = np.empty(int(self.n_units.sum()))
        fam = np.empty(self.n_nodes.size)
        ms = ctypes.c_double(0.0)
        rc = _lib.load().cb_em_estep(h, Q.ctypes.data, pi.ctypes.data, E.ctypes.data, ll.ctypes.data, fam.ctypes.data,
                                     ctypes.byref(ms))
        _lib.check(rc, "cb_em_estep")
        self.last_kernel_ms = ms.value
        self.last_unit_loglik = np.split(ll, np.cumsum(self.n_units)[:-1])
        self.last_family_loglik = fam
        return E, float(fam.sum())


def m_step(grid: np.ndarray, E: np.ndarray, Q: np.ndarray, num_epochs: int, learning_rate: float, device: int) -> np.ndarray:
    """argmax_Q sum_b sum_ab E_b[a, b] log expm(t_b Q)[a, b] by the package's optimiser (pande-reversible parameterisation),
    started at Q; the best iterate includes the start."""
    import torch
    from ..bank import CherryBank
    from ._ratelearn._rate_matrix import RateMatrix
    S = Q.shape[0]
    mod = RateMatrix(num_states=S, mode="pande_reversible", mask=torch.ones(S, S, dtype=torch.float64),
                     pi=torch.ones(S, dtype=torch.float64) / S, pi_requires_grad=True, initialization=np.asarray(Q))
    u0 = mod.upper_diag.detach().numpy().copy()
    p0 = mod._pi.detach().numpy().copy()
    with CherryBank(np.asarray(grid, dtype=np.float64), np.ascontiguousarray(E), device=device, dtype="f64") as bank:
        r = bank.train_pande_reversible(u0, p0, num_epochs=int(num_epochs), lr=float(learning_rate), do_adam=True)
    return r["Q_best"]


def _all_reduce_f64(x: np.ndarray) -> np.ndarray:
    """sum over the ranks (float64; counting/_stage.py::_all_reduce_counts for real-valued counts)"""
    try:
        import torch
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
            t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return t.cpu().numpy()
    except ImportError:  # pragma: no cover
        pass
    return x


def _root_distribution(path: str, states: List[str]) -> np.ndarray:
    """the distribution at `path` in the order of `states` (the initialisation's alphabet), whatever the file's row order"""
    from ..io import read_probability_distribution
    df = read_probability_distribution(path)
    got = [str(x) for x in df.index]
    if sorted(got) != sorted(states):
        raise ValueError(f"em_lg: the root distribution's states {got} are not the rate matrix's {list(states)}")
    return df.reindex(states).to_numpy(dtype=np.float64).reshape(-1)


def _read_family(tree_dir, msa_dir, site_rates_dir, family, states):
    from ..counting._host import read_msa, read_site_rates
    from ..evaluation._likelihood import _family_units
    from ..io import read_tree
    tree = read_tree(os.path.join(tree_dir, family + ".txt"))
    msa = read_msa(os.path.join(msa_dir, family + ".txt"))
    rates = np.asarray(read_site_rates(os.path.join(site_rates_dir, family + ".txt")), dtype=np.float64)
    _, _, codes = _family_units(tree, msa, None, len(rates), states, False)
    return tree, codes, rates


@caching.cached_computation(output_dirs=["output_rate_matrix_dir"], write_extra_log_files=True, collective=True)
def em_lg(
    tree_dir: str,
    msa_dir: str,
    site_rates_dir: str,
    families: List[str],
    initialization_rate_matrix_path: str,
    output_rate_matrix_dir: Optional[str] = None,
    *,
    quantization_points: Optional[List[float]] = None,
    num_iterations: int = 20,
    m_step_epochs: int = 500,
    learning_rate: float = 0.1,
    tolerance: float = 1e-6,
    stationary_distribution_path: Optional[str] = None,
) -> None:
    """Learn Q by full-tree EM from `initialization_rate_matrix_path`.  Writes `result.txt` (the reference rate-matrix format,
    the initialisation's alphabet), `log_likelihoods.txt` (the log-likelihood before the first and after every iteration, a
    decrease included: EM then stops and keeps the better matrix) and
    `profiling.txt`.  The root distribution is `stationary_distribution_path` or the initialisation's stationary distribution,
    fixed for the run.  Stops after `num_iterations` or when an iteration gains less than `tolerance`.  Families are dealt
    over the ranks of torch.distributed as the counting stages deal them; counts and log-likelihoods are all-reduced."""
    from ..counting._stage import _device_index, _my_families, _run_local_then_agree
    from ..evaluation._likelihood import _stationary_distribution
    from ..io import read_rate_matrix, write_rate_matrix
    from ..caching._cached import _dist_state
    start = time.time()
    log = logging.getLogger(__name__)
    init = read_rate_matrix(initialization_rate_matrix_path)
    states = list(init.index)
    Q = init.to_numpy().astype(np.float64)
    S = len(states)
    pi_root = (_root_distribution(stationary_distribution_path, states)
               if stationary_distribution_path is not None else _stationary_distribution(Q))
    grid = np.array(sorted(float(q) for q in (quantization_points if quantization_points is not None else DEFAULT_GRID)))
    device = _device_index()
    if _lib.load().cb_device_count() <= 0:
        raise _lib.CherryBankError("em_lg: no HIP device visible; the E-step runs on the MI355X only (no CPU fallback)")
    mine = _my_families(families)
    log.info(f"EM on {len(mine)} of {len(families)} families")
    box = {}

    def local():
        fams = [_read_family(tree_dir, msa_dir, site_rates_dir, f, states) for f in mine]
        box["estep"] = EStep([f[0] for f in fams], [f[1] for f in fams], [f[2] for f in fams], grid, device=device,
                             num_states=S) if fams else None

    _run_local_then_agree(local, "em_lg")
    es = box["estep"]

    def agreed(fn, what):
        """run a rank-local step; under torch.distributed every rank raises if any rank failed, before the next collective"""
        out = {}
        _run_local_then_agree(lambda: out.setdefault("r", fn()), f"em_lg: {what}")
        return out["r"]

    def estep(Qc):
        local = (lambda: (np.zeros((grid.size, S, S)), 0.0)) if es is None else (lambda: es.expected_counts(Qc, pi_root))
        E, ll = agreed(local, "E-step")
        red = _all_reduce_f64(np.concatenate([E.reshape(-1), [ll]]))
        return red[:-1].reshape(grid.size, S, S), float(red[-1])

    try:
        E, ll = estep(Q)
        lls = [ll]   # every iteration's log-likelihood is recorded, a decrease included
        for it in range(int(num_iterations)):
            Q_new = agreed(lambda: m_step(grid, E, Q, m_step_epochs, learning_rate, device), "M-step")
            E_new, ll_new = estep(Q_new)
            lls.append(ll_new)
            log.info(f"EM iteration {it + 1}: log-likelihood {ll_new}")
            if ll_new < ll:
                # the M-step keeps its start among its candidates, so this is at most a rounding-level change; the result
                # stays the better matrix
                warnings.warn(f"em_lg: iteration {it + 1} lowered the log-likelihood from {ll!r} to {ll_new!r}; stopping")
                break
            Q, E, gain, ll = Q_new, E_new, ll_new - ll, ll_new
            if gain < tolerance:
                break
    finally:
        if es is not None:
            es.close()
    if _dist_state()[0] == 0:
        os.makedirs(output_rate_matrix_dir, exist_ok=True)
        write_rate_matrix(Q, states, os.path.join(output_rate_matrix_dir, "result.txt"))
        with open(os.path.join(output_rate_matrix_dir, "log_likelihoods.txt"), "w") as f:
            f.write("".join(f"{x!r}\n" for x in lls))
        with open(os.path.join(output_rate_matrix_dir, "profiling.txt"), "w") as f:
            f.write(f"Total time: {time.time() - start} seconds\n")
