"""`simulate_msas` (reference: cherryml/simulation/_simulate_msas.py:280-423, `_map_func` :94-252) on the GPU.

Host: reading the model, trees, site rates and contact maps, the reference's validation, the units of every family
(independent sites ascending, then the contacting pairs in `np.where` order) and the output files.  Device: cb_sim_model_run,
one thread per (family, unit) over every family of a batch (csrc/simulate.hip.h).  The random stream is counter-based
(include/cherrybank.h): the MSAs do not depend on batching or on how many ranks share the families.  With torch.distributed
initialised, every rank simulates its share of the families (dealt round-robin, as the counting stages deal them) and writes
their files; the files are the same as a one-rank run's."""
import ctypes
import hashlib
import logging
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from .. import _lib, caching
from ..counting._host import read_contact_map, read_site_rates
from ..counting._stage import _device_index, _my_families, _run_local_then_agree
from ..io import read_probability_distribution, read_rate_matrix, read_tree, write_msa

_STRATEGIES = ("all_transitions",)
_BATCH_BYTES = 1 << 28   # output bytes per cb_sim_model_run call, at most (families are batched up to this)


def family_seed(family: str, random_seed: int) -> int:
    """The reference's per-family seed (_simulate_msas.py:196-198); the Philox key is its low 64 bits."""
    return int(hashlib.md5(family.encode()).hexdigest()[:8], 16) + int(random_seed)


def _as_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


class Simulator:
    """The simulator model resident on one GPU: alias tables of Q1 / pi1 (S1 states) and, optionally, of Q2 / pi2 (S1^2
    states), built once.  `run` simulates a batch of families in one launch.  A context manager; `close()` frees it."""

    def __init__(self, Q1: np.ndarray, pi1: np.ndarray, Q2: Optional[np.ndarray] = None, pi2: Optional[np.ndarray] = None,
                 device: Optional[int] = None):
        self._lib = _lib.load()
        self.S1 = int(np.asarray(Q1).shape[0])
        self._keep = [np.ascontiguousarray(x, dtype=np.float64) for x in (Q1, pi1)]
        q2 = p2 = None
        if Q2 is not None:
            q2, p2 = np.ascontiguousarray(Q2, dtype=np.float64), np.ascontiguousarray(pi2, dtype=np.float64)
            if q2.shape != (self.S1 ** 2, self.S1 ** 2) or p2.shape != (self.S1 ** 2,):
                raise ValueError(f"Q2 / pi2 must have {self.S1 ** 2} states (S1 = {self.S1})")
        if self._keep[0].shape != (self.S1, self.S1) or self._keep[1].shape != (self.S1,):
            raise ValueError(f"Q1 must be square and pi1 of the same size: {self._keep[0].shape}, {self._keep[1].shape}")
        self.has_pairs = q2 is not None
        h = ctypes.c_void_p()
        rc = self._lib.cb_sim_model_create(_device_index() if device is None else int(device), self.S1,
                                           self._keep[0].ctypes.data, self._keep[1].ctypes.data, _as_ptr(q2), _as_ptr(p2),
                                           ctypes.byref(h))
        _lib.check(rc, "cb_sim_model_create")
        self._h = h
        self.last_kernel_ms = 0.0

    def run(self, families: Sequence[Dict]) -> List[np.ndarray]:
        """families: dicts with `seed` (int), `parent` (int[n], preorder, -1 at the root), `length` (float[n]), `n_sites`,
        `site_a`, `site_b` (int[U], -1 = independent site), `rate` (float[U]).  -> one int8 array [n_nodes][n_sites] per
        family (a pair's two columns hold the codes a and b of its state a * S1 + b)."""
        if self._h is None:
            raise _lib.CherryBankError("Simulator is closed")
        if not families:
            return []
        cat = lambda key, dt: np.ascontiguousarray(np.concatenate([np.asarray(f[key], dtype=dt) for f in families]))  # noqa
        seeds = np.array([int(f["seed"]) & 0xFFFFFFFFFFFFFFFF for f in families], dtype=np.uint64)
        n_nodes = np.array([len(f["parent"]) for f in families], dtype=np.int32)
        n_sites = np.array([int(f["n_sites"]) for f in families], dtype=np.int32)
        n_units = np.array([len(f["site_a"]) for f in families], dtype=np.int32)
        parent, length = cat("parent", np.int32), cat("length", np.float64)
        ua, ub, rate = cat("site_a", np.int32), cat("site_b", np.int32), cat("rate", np.float64)
        sizes = n_nodes.astype(np.int64) * n_sites
        out = np.empty(int(sizes.sum()), dtype=np.int8)
        ms = ctypes.c_double(0.0)
        rc = self._lib.cb_sim_model_run(self._h, len(families), seeds.ctypes.data, n_nodes.ctypes.data, parent.ctypes.data,
                                        length.ctypes.data, n_sites.ctypes.data, n_units.ctypes.data, ua.ctypes.data,
                                        ub.ctypes.data, rate.ctypes.data, out.ctypes.data, ctypes.byref(ms))
        _lib.check(rc, "cb_sim_model_run")
        self.last_kernel_ms = ms.value
        offs = np.concatenate([[0], np.cumsum(sizes)])
        return [out[offs[k]:offs[k + 1]].reshape(n_nodes[k], n_sites[k]) for k in range(len(families))]

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self._lib.cb_sim_model_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def _check_states(df, want: List[str], what: str, axis: str = "index") -> None:
    got = list(getattr(df, axis))
    if got != want:
        raise Exception(f"{what} {axis} is:\n{got}\nbut expected:\n{want}")


def _read_model(amino_acids, pi_1_path, Q_1_path, pi_2_path, Q_2_path):
    """The four model files with the reference's state-order checks (_simulate_msas.py:135-170)."""
    pairs = [a + b for a in amino_acids for b in amino_acids]
    pi_1, Q_1 = read_probability_distribution(pi_1_path), read_rate_matrix(Q_1_path)
    pi_2, Q_2 = read_probability_distribution(pi_2_path), read_rate_matrix(Q_2_path)
    _check_states(pi_1, list(amino_acids), "pi_1")
    _check_states(pi_2, pairs, "pi_2")
    _check_states(Q_1, list(amino_acids), "Q_1")
    _check_states(Q_1, list(amino_acids), "Q_1", "columns")
    _check_states(Q_2, pairs, "Q_2")
    _check_states(Q_2, pairs, "Q_2", "columns")
    return (Q_1.to_numpy(), pi_1.to_numpy().reshape(-1), Q_2.to_numpy(), pi_2.to_numpy().reshape(-1))


def family_units(site_rates: np.ndarray, contact_map: np.ndarray):
    """(site_a, site_b, rate) of a family: the independent sites ascending (their site rates), then the contacting pairs
    (i, j), i < j, in `np.where` order at rate 1 -- with the reference's checks (_simulate_msas.py:177-190, :234-238)."""
    num_sites = len(site_rates)
    i, j = np.where(np.asarray(contact_map) == 1)
    keep = i < j
    pairs = list(zip(i[keep].tolist(), j[keep].tolist()))
    sites = [s for p in pairs for s in p]
    if len(set(sites)) != len(sites):
        raise Exception(f"Each site can only be in contact with one other site. The contacting sites were: {pairs}")
    for a, b in pairs:
        if b >= num_sites:
            raise Exception(f"Site {(a, b)} out of range: {num_sites}")
    in_contact = np.zeros(num_sites, dtype=bool)
    in_contact[sites] = True
    indep = np.flatnonzero(~in_contact)
    site_a = np.concatenate([indep, np.array([p[0] for p in pairs], dtype=np.int64)]).astype(np.int32)
    site_b = np.concatenate([np.full(len(indep), -1), np.array([p[1] for p in pairs], dtype=np.int64)]).astype(np.int32)
    rate = np.concatenate([np.asarray(site_rates, dtype=np.float64)[indep], np.ones(len(pairs))])
    return site_a, site_b, rate


def _read_family(tree_dir, site_rates_dir, contact_map_dir, family, seed):
    tree = read_tree(os.path.join(tree_dir, family + ".txt"))
    site_rates = read_site_rates(os.path.join(site_rates_dir, family + ".txt"))
    contact_map = read_contact_map(os.path.join(contact_map_dir, family + ".txt"))
    order = tree.preorder_traversal()
    index = {v: k for k, v in enumerate(order)}
    parent = np.full(len(order), -1, dtype=np.int32)
    length = np.zeros(len(order), dtype=np.float64)
    for k, v in enumerate(order[1:], start=1):
        p, t = tree.parent(v)
        parent[k], length[k] = index[p], t
    site_a, site_b, rate = family_units(site_rates, contact_map)
    return dict(names=order, seed=seed, parent=parent, length=length, n_sites=len(site_rates),
                site_a=site_a, site_b=site_b, rate=rate)


def _write_family(path: str, names: List[str], codes: np.ndarray, alphabet: np.ndarray) -> None:
    rows = alphabet[codes.astype(np.intp)]                 # [n_nodes][n_sites] single bytes
    seqs = [r.tobytes().decode("ascii") for r in rows]
    write_msa(dict(zip(names, seqs)), path)


@caching.cached_computation(
    exclude_args=["num_processes", "use_cpp_implementation", "cpp_command_line_prefix", "cpp_command_line_suffix"],
    output_dirs=["output_msa_dir"], write_extra_log_files=True, collective=True)
def simulate_msas(
    tree_dir: str,
    site_rates_dir: str,
    contact_map_dir: str,
    families: List[str],
    amino_acids: List[str],
    pi_1_path: str,
    Q_1_path: str,
    pi_2_path: str,
    Q_2_path: str,
    strategy: str,
    random_seed: int,
    num_processes: Optional[int] = 1,
    use_cpp_implementation: bool = True,
    cpp_command_line_prefix: str = "",
    cpp_command_line_suffix: str = "0",
    output_msa_dir: Optional[str] = None,
) -> None:
    """Simulate one MSA per family: a sequence for EVERY node of the tree (internal nodes included), written as
    `write_msa` writes it.  Sites in no contact evolve under Q_1 at their site rate; each contacting pair (every site in at
    most one contact) evolves as one unit under Q_2 at rate 1; root states from pi_1 / pi_2.  `strategy` must be
    "all_transitions" (the exact jump chain; the only one the reference implements).  The family seed is the reference's
    `int(md5(family)[:8], 16) + random_seed`; the stream is this package's (Philox, include/cherrybank.h), so the MSAs
    match the reference's in distribution, not bit for bit.  `num_processes`, `use_cpp_implementation` and
    `cpp_command_line_*` are accepted and ignored: one GPU launch covers a whole batch of families."""
    log = logging.getLogger(__name__)
    if strategy not in _STRATEGIES:
        raise Exception(f"Unknown strategy: {strategy}")
    amino_acids = list(amino_acids)
    Q1, pi1, Q2, pi2 = _read_model(amino_acids, pi_1_path, Q_1_path, pi_2_path, Q_2_path)
    alphabet = np.frombuffer("".join(amino_acids).encode("ascii"), dtype=np.uint8)
    if len(alphabet) != len(amino_acids):
        raise ValueError("simulate_msas: every state must be one ASCII character")
    mine = _my_families(families)
    log.info(f"Simulating MSAs for {len(mine)} of {len(families)} families")
    os.makedirs(output_msa_dir, exist_ok=True)

    def local():
        fams = [_read_family(tree_dir, site_rates_dir, contact_map_dir, f, family_seed(f, random_seed)) for f in mine]
        if not fams:
            return
        with Simulator(Q1, pi1, Q2, pi2) as sim:
            start = 0
            while start < len(fams):
                stop, size = start, 0
                while stop < len(fams) and (stop == start or size + len(fams[stop]["parent"]) * fams[stop]["n_sites"]
                                            <= _BATCH_BYTES):
                    size += len(fams[stop]["parent"]) * fams[stop]["n_sites"]
                    stop += 1
                for k, codes in zip(range(start, stop), sim.run(fams[start:stop])):
                    _write_family(os.path.join(output_msa_dir, mine[k] + ".txt"), fams[k]["names"], codes, alphabet)
                start = stop

    _run_local_then_agree(local, "simulate_msas")
