"""Time the branch supports (`cb_bl_supports`: the NNI scan, then csrc/sup.hip.h `sup_weights_kernel` / `sup_gemm_kernel` /
`sup_edge_kernel` on the scan's buffer) and the stage `ml_branch_supports` on the `nj_ml_trees` output of the 32 demo families
(tests/golden/demo32_co_inputs.npz alignments) under LG, with 1000 replicates.  Reports the edges and moves, the kernel time of
the passes, of the scan and of the resampling (the three new kernels together: HIP events around them), the wall time of the
call, the creation of the handle and the wall time of the stage.

    python profiles/tools/time_sup.py [--baseline] [--out profiles/sup_demo32.json]

--baseline is the only route to these numbers without the entry point: `nni_scan(per_site=True)` copies ll'[move][site] to the
host, where the same multiplicities (tests/sup_reference.py, timed on their own) meet it in a NumPy product and the edge
reduction; it reports the time of each part and the largest distance of the entry point's values and counts to it, against the
bars of tests/test_gpu_sup.py.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
AA = list("ARNDCQEGHILKMFPSTWYV")
KEYS3 = ("output_tree_dir", "output_site_rates_dir", "output_likelihood_dir")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-rounds", type=int, default=10)
    ap.add_argument("--num-rate-categories", type=int, default=20)
    ap.add_argument("--num-replicates", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from conftest import load_golden
    from time_nj import _msas

    from cherryml_amd import BranchLengthFitter, ml_branch_supports, nj_ml_trees
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation._likelihood import _family_units, _stationary_distribution
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    from cherryml_amd.simulation._simulate import family_seed
    fams, texts = _msas()
    Q = np.ascontiguousarray(load_golden("likelihood.npz")["lg"], dtype=np.float64)
    pi = _stationary_distribution(Q)
    grid = np.array(quantization_points_ble(0.03, 1.1, 64))
    R = args.num_replicates
    with tempfile.TemporaryDirectory() as tmp:
        msa = os.path.join(tmp, "msa")
        os.makedirs(msa)
        for fam, text in zip(fams, texts):
            with open(os.path.join(msa, fam + ".txt"), "wb") as f:
                f.write(text)
        qpath = os.path.join(tmp, "lg.txt")
        write_rate_matrix(Q, AA, qpath)
        ml = nj_ml_trees(msa_dir=msa, families=fams, rate_matrix_path=qpath, num_rate_categories=args.num_rate_categories,
                         num_rounds=args.num_rounds, **{k: os.path.join(tmp, "ml_" + k) for k in KEYS3})
        trees = [read_tree(os.path.join(ml["output_tree_dir"], fam + ".txt")) for fam in fams]
        rates = [np.asarray(read_site_rates(os.path.join(ml["output_site_rates_dir"], fam + ".txt"))) for fam in fams]
        codes = [_family_units(t, read_msa(os.path.join(msa, fam + ".txt")), None, len(r), AA, False)[2]
                 for t, r, fam in zip(trees, rates, fams)]
        # the stage, as a user calls it (twice: the first call pays the first use of the device)
        stage_walls = []
        for i in range(2):
            t0 = time.perf_counter()
            ml_branch_supports(tree_dir=ml["output_tree_dir"], msa_dir=msa, site_rates_dir=ml["output_site_rates_dir"], families=fams,
                               rate_matrix_path=qpath, num_replicates=R, output_support_dir=os.path.join(tmp, f"sup{i}"))
            stage_walls.append(time.perf_counter() - t0)
    seeds = [family_seed(f, 0) for f in fams]
    t0 = time.perf_counter()
    fit = BranchLengthFitter(trees, codes, rates, grid, Q, pi)
    create_s = time.perf_counter() - t0
    calls = []
    with fit:
        moves = fit.nni_moves()
        for _ in range(1 + args.repeats):
            t0 = time.perf_counter()
            got = fit.branch_supports(R, seeds)
            ms = fit.last_support_kernel_ms
            calls.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, passes_kernel_ms=ms[0], scan_kernel_ms=ms[1],
                              resampling_kernel_ms=ms[2]))
        full = fit.branch_supports(R, seeds, per_replicate=True)
        fam_ll = fit.log_likelihoods()[1]
        calls = calls[1:]
        n_moves, n_edges = int(sum(len(m) for m in moves)), int(sum(len(g[0]) for g in got))
        move_sites = int(sum(len(m) * len(r) for m, r in zip(moves, rates)))
        sh = np.concatenate([g[2] for g in got])
        rec = dict(what="cb_bl_supports and ml_branch_supports on the nj_ml_trees output of the 32 demo families under LG, one MI355X",
                   families=len(fams), nodes=int(sum(len(t.nodes()) for t in trees)), sites=int(sum(len(r) for r in rates)),
                   replicates=R, edges=n_edges, moves=n_moves, move_sites=move_sites,
                   product_flops=2.0 * move_sites * R, weight_bytes=8.0 * R * int(sum(len(r) for r in rates)),
                   handle_create_s=create_s, calls=calls,
                   resampling_kernel_us_per_edge=float(np.mean([c["resampling_kernel_ms"] for c in calls]) * 1e3 / n_edges),
                   edges_with_sh_at_least_0_95=int((sh >= 0.95).sum()), edges_with_sh_below_0_5=int((sh < 0.5).sum()),
                   edges_with_alrt_not_positive=int(sum(int((g[1] <= 0).sum()) for g in got)),
                   stage=dict(wall_s=stage_walls, num_replicates=R))
        if args.baseline:
            import sup_reference
            t0 = time.perf_counter()
            W = [sup_reference.weights(len(r), R, s) for r, s in zip(rates, seeds)]
            weights_s = time.perf_counter() - t0
            lls = fit.log_likelihoods()[0]
            scan_ms, host_ms = [], []
            worst_rep = worst_alrt = 0.0
            count_diff = undecided = 0
            for rep in range(1 + args.repeats):
                t0 = time.perf_counter()
                _, _, ll_moves = fit.nni_scan(moves, per_site=True)
                t1 = time.perf_counter()
                ref = [sup_reference.supports(m, x, l, R, s, W=w) for m, x, l, s, w in zip(moves, ll_moves, lls, seeds, W)]
                t2 = time.perf_counter()
                scan_ms.append((t1 - t0) * 1e3), host_ms.append((t2 - t1) * 1e3)
            for k, (s, g) in enumerate(zip(ref, full)):
                if len(s["nodes"]) == 0:
                    continue
                scale = max(1.0, abs(fam_ll[k]))
                worst_rep = max(worst_rep, float(np.abs(g[4] - s["delta_rep"]).max()) / scale)
                worst_alrt = max(worst_alrt, float(np.abs(g[1] - s["alrt"]).max()) / scale)
                bar = 1e-9 * abs(s["fam_ll"])
                undecided += int((s["sh_margin"] <= bar).sum() + (s["rell_margin"] <= bar).sum())
                count_diff += int((np.rint(g[2] * R) != s["sh_count"]).sum() + (np.rint(g[3] * R) != s["rell_count"]).sum())
            rec["baseline"] = dict(what="nni_scan(per_site=True), then the product with the same multiplicities and the edge "
                                        "reduction in NumPy on the host (tests/sup_reference.py)",
                                   scan_per_site_call_ms=scan_ms[1:], host_product_and_reduction_ms=host_ms[1:],
                                   host_weights_s_not_counted=weights_s,
                                   max_delta_rep_difference_over_fam_ll=worst_rep, bar_delta_rep=1e-10,
                                   max_alrt_difference_over_fam_ll=worst_alrt, bar_alrt=2e-10,
                                   decisions_undecided_at_1e_9=undecided, edge_counts_that_differ=count_diff)
    print(json.dumps(rec, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
