"""Time the co-evolution scan (`cb_coscan_*`, csrc/coscan.hip.h) and the stage `coevolution_scan` on the 32 demo families
(tests/golden/demo32_co_inputs.npz: trees and alignments) under LG and the demo co-evolution matrix
(tests/golden/coevo_demo_full.npz: the reference's 50-epoch Q_2 and its 129-point grid), in `cherry` mode.  Reports the creation
of the two log banks, the scan kernel's time, the wall time of the call and of the stage, and gathers per second: a contributing
(site pair, sequence pair) costs 8 gathers (4 of log P2, 4 of log P1), a visited one the LDS reads only.

    python profiles/tools/time_coscan.py [--baseline] [--out profiles/coscan_demo32.json]

The same call is timed once more with the sequence pairs in index order instead of bucket order (test hook
CB_COSCAN_INDEX_ORDER): what walking the buckets in one order is worth.

--baseline is the only route to these numbers without the entry point: one `cb_count_co_transitions` call with the contact
list [(i, j)] plus a dot product with the log bank per site pair, on 32 sampled pairs of the largest family, with the values
checked equal (the log bank of the baseline is the NumPy restatement's, tests/coscan_reference.py, and is not timed).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
AA = list("ARNDCQEGHILKMFPSTWYV")


def _from_support(vals, mask):
    keep = (mask != 0) | np.eye(len(mask), dtype=bool)
    Q = np.zeros(mask.shape)
    Q[keep] = vals
    return Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from conftest import load_golden

    from cherryml_amd import CoevolutionScanner, _lib, coevolution_scan
    from cherryml_amd.coevolution._scan import _family_records
    from cherryml_amd.evaluation._likelihood import _stationary_distribution
    from cherryml_amd.io import write_rate_matrix
    z = load_golden("demo32_co_inputs.npz")
    fams = [str(f) for f in z["families"]]
    co = load_golden("coevo_demo_full.npz")
    mask = np.unpackbits(co["mask_packed"])[:160000].reshape(400, 400)
    Q2 = np.ascontiguousarray(_from_support(co["traj_Q_best_support_f64"], mask))
    Q1 = np.ascontiguousarray(load_golden("likelihood.npz")["lg"], dtype=np.float64)
    grid = np.ascontiguousarray(co["t"], dtype=np.float64)
    pi1, pi2 = _stationary_distribution(Q1), _stationary_distribution(Q2)
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {}
        for kind in ("tree", "msa"):
            d = os.path.join(tmp, kind)
            os.makedirs(d)
            off, blob = z[f"{kind}_offsets"], z[f"{kind}_bytes"].tobytes()
            for k, fam in enumerate(fams):
                with open(os.path.join(d, fam + ".txt"), "wb") as f:
                    f.write(blob[off[k]:off[k + 1]])
            dirs[kind] = d
        paths = {k: os.path.join(tmp, k + ".txt") for k in ("Q1", "Q2")}
        write_rate_matrix(Q1, AA, paths["Q1"])
        write_rate_matrix(Q2, [a + b for a in AA for b in AA], paths["Q2"])
        stage_walls = []
        for i in range(2):   # twice: the first call pays the first use of the device
            t0 = time.perf_counter()
            coevolution_scan(tree_dir=dirs["tree"], msa_dir=dirs["msa"], families=fams, amino_acids=AA, rate_matrix_path=paths["Q1"],
                             coevolution_rate_matrix_path=paths["Q2"], quantization_points=[float(t) for t in grid],
                             edge_or_cherry="cherry", output_scan_dir=os.path.join(tmp, f"scan{i}"))
            stage_walls.append(time.perf_counter() - t0)
        n_sites, seqs, recs = [], [], []
        for fam in fams:
            s, L, p = _family_records(dirs["tree"], dirs["msa"], fam, AA, "cherry")
            n_sites.append(L), seqs.append(s), recs.append(p)
    t0 = time.perf_counter()
    sc = CoevolutionScanner(Q1, Q2, grid, pi1, pi2)
    create_s = time.perf_counter() - t0
    calls, calls_index_order = [], []
    with sc:
        for order, dst in (("", calls), ("1", calls_index_order)):
            os.environ["CB_TEST_HOOKS"] = "1" if order else ""
            os.environ["CB_COSCAN_INDEX_ORDER"] = order
            for _ in range(1 + args.repeats):
                t0 = time.perf_counter()
                res = sc.scan_records(n_sites, seqs, recs, symmetric=True)
                dst.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, scan_kernel_ms=sc.last_kernel_ms))
            del dst[0]
            if not order:
                kept = res
        os.environ.pop("CB_TEST_HOOKS"), os.environ.pop("CB_COSCAN_INDEX_ORDER")
        contributing = int(sum(int(np.triu(r["n_used"], 1).sum()) for r in kept))
        site_pairs = int(sum(L * (L - 1) // 2 for L in n_sites))
        kms = float(np.mean([c["scan_kernel_ms"] for c in calls]))
        worst_order = max(float(np.max(np.abs(a["score"] - b["score"]) / np.maximum(1.0, np.abs(a["score"])))) for a, b in zip(kept, res))
        rec = dict(what="cb_coscan_run and coevolution_scan on the 32 demo families under LG and the demo co-evolution matrix, "
                        "cherry mode, one MI355X",
                   families=len(fams), sites=int(sum(n_sites)), largest_family_sites=int(max(n_sites)),
                   sequence_pairs=int(sum(len(p) for p in recs)), site_pairs=site_pairs, grid_points=int(grid.size),
                   contributing_site_pair_x_sequence_pair=contributing, gathers=8 * contributing,
                   bank_create_s=create_s, calls=calls, gathers_per_second=8 * contributing / (kms * 1e-3),
                   calls_in_pair_index_order=calls_index_order,
                   index_order_over_bucket_order_kernel_time=float(np.mean([c["scan_kernel_ms"] for c in calls_index_order]) / kms),
                   max_score_difference_between_the_orders=worst_order,
                   stage=dict(wall_s=stage_walls))
        if args.baseline:
            import coscan_reference as cr
            from cherryml_amd.counting._stage import PAIR_DTYPE
            k = int(np.argmax(n_sites))
            L = n_sites[k]
            lp2 = cr.log_bank(cr.bank(Q2, grid, pi2))
            rng = np.random.default_rng(0)
            sample = []
            while len(sample) < 32:
                i, j = sorted(rng.integers(0, L, 2).tolist())
                if i < j and (i, j) not in sample:
                    sample.append((i, j))
            p = np.array(recs[k], dtype=PAIR_DTYPE)
            p["n"] = 1
            lib = _lib.load()
            ms, worst = [], 0.0
            for i, j in sample:
                contacts = np.array([i, j], dtype=np.int32)
                C = np.zeros((grid.size, 400, 400), dtype=np.uint64)
                t0 = time.perf_counter()
                _lib.check(lib.cb_count_co_transitions(0, 20, grid.size, grid.ctypes.data, seqs[k].ctypes.data, seqs[k].size,
                                                       contacts.ctypes.data, 1, p.ctypes.data, len(p), 1, 0, C.ctypes.data),
                           "cb_count_co_transitions")
                nz = np.nonzero(C)
                x = 0.25 * float(np.sum(C[nz].astype(np.float64) * lp2[nz]))
                ms.append((time.perf_counter() - t0) * 1e3)
                worst = max(worst, abs(x - kept[k]["pair_ll"][i, j]) / max(1.0, abs(x)))
            assert worst <= 1e-10, worst
            per_pair = float(np.mean(ms[1:]))
            rec["baseline"] = dict(what="one cb_count_co_transitions call with the contact list [(i, j)] and a dot product with the "
                                        "log bank per site pair, 32 sampled pairs of the largest family (pair_ll only)",
                                   family=fams[k], sites=int(L), ms_per_site_pair=per_pair,
                                   extrapolated_s_for_the_family=per_pair * 1e-3 * L * (L - 1) / 2,
                                   extrapolated_s_for_the_32_families=per_pair * 1e-3 * site_pairs,
                                   max_pair_ll_difference=worst, bar=1e-10)
    print(json.dumps(rec, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
