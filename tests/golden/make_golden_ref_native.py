#!/usr/bin/env python3
"""Outputs of the reference's own C++ (oracle/_ref/*.so, built by oracle/Makefile from the reference's sources) on
the inputs of the CPU tests that check against it, stored so that those tests run from the repository alone.

Written: tests/golden/ref_native.npz
  expm_grid [17], expm_P [17,20,20]   libref_expm.so ref_expm (r8mat_expm1, Pade) of t * LG over every 8th
                                      point of the quantisation grid (test_oracle_golden.py)
  pair<k>_seqs [n,L] int8 / _seed / _pairs [m,2]
                                      libref_fc.so ref_divide_and_pair on 25 random families
                                      (test_fast_cherries_cpu.py), -1 = unknown
  w<R> [R]                            libref_fc.so ref_initial_weights for R = 2, 5, 20, 41 rate categories
  rnd<k>_bank_idx [N] int32, rnd<k>_bank [N]
                                      libref_ble.so ref_log_bank of ble.npz's Q on grid_sr with rnd<k>_rates
                                      ([T,R,20,20], all of it computed): N = 2048 entries at seeded flat positions
                                      (test_oracle_golden.py)

Usage:  make -C oracle && python tests/golden/make_golden_ref_native.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from cherryml_amd.phylogeny_estimation._fast_cherries import rate_categories_ble  # noqa: E402
from oracle import ble_oracle as bo  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")

# the inputs of the tests, regenerated exactly as they draw them
EXPM_GRID = np.array([float("%.8f" % (0.03 * 1.1 ** i)) for i in range(-64, 65)])[::8]
N_PAIR_TRIALS = 25
WEIGHT_RS = (2, 5, 20, 41)


def pairing_inputs():
    rng = np.random.default_rng(123)
    for trial in range(N_PAIR_TRIALS):
        n, L = int(rng.integers(2, 120)), int(rng.integers(1, 50))
        seqs = np.tile(rng.integers(0, 20, size=L), (n, 1))
        flip = rng.random((n, L)) < rng.uniform(0.02, 0.7)
        seqs[flip] = rng.integers(0, 20, size=int(flip.sum()))
        seqs[rng.random((n, L)) < 0.15] = -1
        yield seqs, 7 + trial


BANK_SAMPLE = 2048


def bank_sample(size, k):
    """sorted distinct flat positions into a [T,R,S,S] bank, fixed per case"""
    return np.sort(np.random.default_rng(1000 + k).choice(size, BANK_SAMPLE, replace=False)).astype(np.int32)


def main():
    out = {}
    expm = C.CDLL(os.path.join(REF, "libref_expm.so"))
    expm.ref_expm.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    Q = np.load(os.path.join(HERE, "data_lg.npz"))["lg"]
    P = np.empty((len(EXPM_GRID), 20, 20))
    for b, t in enumerate(EXPM_GRID):
        A = np.asfortranarray(t * Q)
        o = np.empty((20, 20), order="F")
        assert expm.ref_expm(20, A.ctypes.data, o.ctypes.data) == 0
        P[b] = np.ascontiguousarray(o)
    out["expm_grid"], out["expm_P"] = EXPM_GRID, P

    fc = C.CDLL(os.path.join(REF, "libref_fc.so"))
    for k, (seqs, seed) in enumerate(pairing_inputs()):
        n, L = seqs.shape
        s32 = np.ascontiguousarray(seqs, dtype=np.int32)
        pairs = np.zeros(2 * n, dtype=np.int32)
        m = fc.ref_divide_and_pair(s32.ctypes.data_as(C.c_void_p), n, L, seed, pairs.ctypes.data_as(C.c_void_p))
        out[f"pair{k}_seqs"] = seqs.astype(np.int8)
        out[f"pair{k}_seed"] = np.int64(seed)
        out[f"pair{k}_pairs"] = pairs[:2 * m].reshape(m, 2)
    for R in WEIGHT_RS:
        r = np.array(rate_categories_ble(R))
        w = np.zeros(R)
        fc.ref_initial_weights(r.ctypes.data_as(C.c_void_p), R, w.ctypes.data_as(C.c_void_p))
        out[f"w{R}"] = w

    assert bo.ref_available(), "run `make -C oracle` first"
    z = np.load(os.path.join(HERE, "ble.npz"))
    for k in range(3):
        bank = bo.ref_log_bank(z["Q"], z["grid_sr"], z[f"rnd{k}_rates"]).reshape(-1)
        idx = bank_sample(bank.size, k)
        out[f"rnd{k}_bank_idx"], out[f"rnd{k}_bank"] = idx, bank[idx]

    path = os.path.join(HERE, "ref_native.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
