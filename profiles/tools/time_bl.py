"""Time the branch-length EM (`ml_branch_lengths`: csrc/bl.hip.h `bl_mstep_kernel` behind the EM passes of csrc/em.hip.h) on the
`nj_trees` output of the 32 demo families (tests/golden/demo32_co_inputs.npz alignments) under LG.  Reports the kernel time of
every round split into the passes and the M-step (HIP events, all families in one handle), the creation of the handle (banks
and their logarithms), the wall time of the stage, and per family the log-likelihood of the neighbour-joining tree, of the tree
snapped to the grid (the start of round 0) and after the last round.

    python profiles/tools/time_bl.py [--num-rounds 10] [--out profiles/bl_demo32.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-rounds", type=int, default=10)
    ap.add_argument("--num-rate-categories", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from conftest import load_golden
    from time_nj import _msas

    from cherryml_amd import BranchLengthFitter, ml_branch_lengths, nj_trees
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation._likelihood import _family_units, _stationary_distribution
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    fams, texts = _msas()
    Q = np.ascontiguousarray(load_golden("likelihood.npz")["lg"], dtype=np.float64)
    with tempfile.TemporaryDirectory() as tmp:
        msa = os.path.join(tmp, "msa")
        os.makedirs(msa)
        for fam, text in zip(fams, texts):
            with open(os.path.join(msa, fam + ".txt"), "wb") as f:
                f.write(text)
        qpath = os.path.join(tmp, "lg.txt")
        write_rate_matrix(Q, AA, qpath)
        nj = {k: os.path.join(tmp, "nj_" + k) for k in ("output_tree_dir", "output_site_rates_dir", "output_likelihood_dir")}
        nj_trees(msa_dir=msa, families=fams, rate_matrix_path=qpath, num_rate_categories=args.num_rate_categories, **nj)
        ll_nj = [float(open(os.path.join(nj["output_likelihood_dir"], fam + ".txt")).readline()) for fam in fams]
        # the stage, as a user calls it
        out = {k: os.path.join(tmp, "ml_" + k) for k in ("output_tree_dir", "output_likelihood_dir")}
        t0 = time.perf_counter()
        ml_branch_lengths(tree_dir=nj["output_tree_dir"], msa_dir=msa, site_rates_dir=nj["output_site_rates_dir"], families=fams,
                          rate_matrix_path=qpath, num_rounds=args.num_rounds, **out)
        stage_wall = time.perf_counter() - t0
        rounds_files = [open(os.path.join(out["output_tree_dir"], fam + ".rounds")).read().split("\n")[:-1] for fam in fams]
        ll_file = [float(open(os.path.join(out["output_likelihood_dir"], fam + ".txt")).readline()) for fam in fams]
        # the handle alone, round by round
        trees = [read_tree(os.path.join(nj["output_tree_dir"], fam + ".txt")) for fam in fams]
        rates = [np.asarray(read_site_rates(os.path.join(nj["output_site_rates_dir"], fam + ".txt"))) for fam in fams]
        codes = [_family_units(t, read_msa(os.path.join(msa, fam + ".txt")), None, len(r), AA, False)[2]
                 for t, r, fam in zip(trees, rates, fams)]
    grid = quantization_points_ble(0.03, 1.1, 64)
    t0 = time.perf_counter()
    with BranchLengthFitter(trees, codes, rates, grid, Q, _stationary_distribution(Q)) as fit:
        create_s = time.perf_counter() - t0
        per_round = []
        for _ in range(args.num_rounds):
            t0 = time.perf_counter()
            n_changed, fam_ll = fit.round()
            per_round.append(dict(passes_kernel_ms=fit.last_kernel_ms[0], mstep_kernel_ms=fit.last_kernel_ms[1],
                                  wall_ms=(time.perf_counter() - t0) * 1e3, families_live=int(np.count_nonzero(n_changed)),
                                  indices_changed=int(n_changed.sum()), log_likelihood_at_start=float(fam_ll.sum())))
        ll_final = fit.log_likelihoods()[1]
    families = {fam: dict(leaves=len(t.leaves()), sites=int(len(r)), rate_categories=int(np.unique(r).size), nj_tree=ll_nj[k],
                          snapped=float(rounds_files[k][0].split()[1]), after_last_round=float(rounds_files[k][-1].split()[1]),
                          likelihood_file=ll_file[k], rounds_run=len(rounds_files[k]) - 1)
                for k, (fam, t, r) in enumerate(zip(fams, trees, rates))}
    rec = dict(what=f"ml_branch_lengths on the nj_trees output of the 32 demo families under LG, {args.num_rounds} rounds, "
                    f"{args.num_rate_categories} rate categories, grid of {len(grid)} points, one MI355X",
               families=len(fams), edges=int(sum(t.num_edges() for t in trees)), edge_sites=int(sum(t.num_edges() * len(r)
                                                                                                   for t, r in zip(trees, rates))),
               handle_create_s=create_s, rounds=per_round, stage_wall_s=stage_wall,
               handle_equals_stage=bool(all(float(ll_final[k]) == families[f]["after_last_round"] for k, f in enumerate(fams))),
               total_log_likelihood=dict(nj_tree=float(sum(ll_nj)), snapped=float(sum(v["snapped"] for v in families.values())),
                                         after_last_round=float(sum(v["after_last_round"] for v in families.values()))),
               per_family=families)
    print(json.dumps({k: v for k, v in rec.items() if k != "per_family"}, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
