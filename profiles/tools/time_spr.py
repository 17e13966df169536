"""Time the SPR scan (`cb_bl_spr_scan`: csrc/spr.hip.h `spr_scan_kernel` and nni.hip.h `nni_sum_kernel` on the resident messages
of the branch-length handle) and the search stage `ml_spr_trees` on the `nj_ml_trees` output of the 32 demo families
(tests/golden/demo32_co_inputs.npz alignments) under LG.  Reports the moves and (move, site) pairs per radius 1 to 4, the kernel
time of the passes and of the scan (HIP events) and the wall time of the call at the search radius, the NNI scan's on the same
handle, and for the stage its wall time, its handles and per round the summed log-likelihood before and after the moves and the
moves selected and applied -- beside `ml_nni_trees` at equal round counts.

    python profiles/tools/time_spr.py [--baseline] [--out profiles/spr_demo32.json]

--baseline takes 32 radius-3 moves of the largest family, evenly spaced over its list, and evaluates each as a rearranged tree
through `tree_likelihood_batch`, one call per move; it reports the time per move and the largest per-site distance to the scan.
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


def _stage_record(out, fams, ext, wall):
    logs, profs = [], []
    for fam in fams:
        rows = [ln.split() for ln in open(os.path.join(out["output_tree_dir"], fam + ext)).read().split("\n")[:-1]]
        logs.append(([r for r in rows if r[0] != "final"], float(rows[-1][1])))
        profs.append(dict(ln.split(": ") for ln in open(os.path.join(out["output_tree_dir"], fam + ".profiling")).read().split("\n")))
    n_rounds = max(len(rows) for rows, _ in logs)
    return dict(wall_s=wall, rounds_run=n_rounds, handles_created=int(max(int(p["handles"]) for p in profs)),
                handle_create_s=float(sum(float(p["create_time"]) for p in profs)),
                scan_call_s=float(sum(float(p["scan_time"]) for p in profs)),
                scan_kernel_ms=float(sum(float(p["scan_kernel_ms"]) for p in profs)),
                fit_s=float(sum(float(p["fit_time"]) for p in profs)),
                families_still_moving_in_the_last_round=int(sum(len(rows) == n_rounds and int(rows[-1][4]) > 0 for rows, _ in logs)),
                per_round=[dict(round=i, families=int(sum(i < len(rows) for rows, _ in logs)),
                                log_likelihood_before=float(sum(float(rows[i][1]) for rows, _ in logs if i < len(rows))),
                                log_likelihood_after=float(sum(float(rows[i][5]) for rows, _ in logs if i < len(rows))),
                                scanned=int(sum(int(rows[i][2]) for rows, _ in logs if i < len(rows))),
                                selected=int(sum(int(rows[i][3]) for rows, _ in logs if i < len(rows))),
                                applied=int(sum(int(rows[i][4]) for rows, _ in logs if i < len(rows))))
                           for i in range(n_rounds)],
                log_likelihood_in=float(sum(float(rows[0][1]) for rows, _ in logs)),
                log_likelihood_final=float(sum(fin for _, fin in logs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-rounds", type=int, default=10)
    ap.add_argument("--num-search-rounds", type=int, default=10)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--num-rate-categories", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from conftest import load_golden
    from time_nj import _msas

    from cherryml_amd import BranchLengthFitter, apply_spr, ml_nni_trees, ml_spr_trees, nj_ml_trees
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation import tree_likelihood_batch
    from cherryml_amd.evaluation._likelihood import _family_units, _stationary_distribution
    from cherryml_amd.io import Tree, read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation import enumerate_spr_moves
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    from cherryml_amd.phylogeny_estimation._nni import _parent_array
    fams, texts = _msas()
    Q = np.ascontiguousarray(load_golden("likelihood.npz")["lg"], dtype=np.float64)
    pi = _stationary_distribution(Q)
    grid = np.array(quantization_points_ble(0.03, 1.1, 64))
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
        # the stages, as a user calls them, at equal round counts
        common = dict(tree_dir=ml["output_tree_dir"], msa_dir=msa, site_rates_dir=ml["output_site_rates_dir"], families=fams,
                      rate_matrix_path=qpath, num_rounds=args.num_rounds)
        out = {k: os.path.join(tmp, "spr_" + k) for k in ("output_tree_dir", "output_likelihood_dir")}
        t0 = time.perf_counter()
        ml_spr_trees(num_spr_rounds=args.num_search_rounds, spr_radius=args.radius, **common, **out)
        spr_stage = _stage_record(out, fams, ".spr", time.perf_counter() - t0)
        out = {k: os.path.join(tmp, "nni_" + k) for k in ("output_tree_dir", "output_likelihood_dir")}
        t0 = time.perf_counter()
        ml_nni_trees(num_nni_rounds=args.num_search_rounds, **common, **out)
        nni_stage = _stage_record(out, fams, ".nni", time.perf_counter() - t0)
    parents = [_parent_array(t) for t in trees]
    per_radius = []
    for radius in (1, 2, 3, 4):
        n = [len(enumerate_spr_moves(p, radius)) for p in parents]
        per_radius.append(dict(radius=radius, moves=int(sum(n)), move_sites=int(sum(k * len(r) for k, r in zip(n, rates)))))
    # the scan alone, on one handle over all families: once to warm up, then timed
    t0 = time.perf_counter()
    fit = BranchLengthFitter(trees, codes, rates, grid, Q, pi)
    create_s = time.perf_counter() - t0
    calls, nni_calls = [], []
    with fit:
        t0 = time.perf_counter()
        moves = fit.spr_moves(args.radius)
        enumerate_s = time.perf_counter() - t0
        for _ in range(1 + args.repeats):
            t0 = time.perf_counter()
            _, delta = fit.spr_scan(moves)
            calls.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, passes_kernel_ms=fit.last_spr_kernel_ms[0],
                              scan_kernel_ms=fit.last_spr_kernel_ms[1]))
            t0 = time.perf_counter()
            _, nni_delta = fit.nni_scan()
            nni_calls.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, passes_kernel_ms=fit.last_nni_kernel_ms[0],
                                  scan_kernel_ms=fit.last_nni_kernel_ms[1]))
        big = int(np.argmax([len(m) for m in moves]))
        pick = np.unique(np.linspace(0, len(moves[big]) - 1, 32).astype(int))
        only = [m[:0] for m in moves]
        only[big] = moves[big][pick]
        ll_scan = fit.spr_scan(only, per_site=True)[2][big]
        tau = fit.indices()[big]
    calls, nni_calls = calls[1:], nni_calls[1:]
    n_moves = int(sum(len(m) for m in moves))
    scan_ms = float(np.mean([c["scan_kernel_ms"] for c in calls]))
    rec = dict(what="cb_bl_spr_scan and ml_spr_trees on the nj_ml_trees output of the 32 demo families under LG, one MI355X",
               families=len(fams), nodes=int(sum(len(t.nodes()) for t in trees)), sites=int(sum(len(r) for r in rates)),
               radius=args.radius, per_radius=per_radius, moves_scanned=n_moves, enumerate_and_indices_s=enumerate_s,
               handle_create_s=create_s, calls=calls, nni_calls_on_the_same_handle=nni_calls,
               scan_kernel_us_per_move=scan_ms * 1e3 / n_moves,
               scan_kernel_over_nni_scan_kernel=scan_ms / float(np.mean([c["scan_kernel_ms"] for c in nni_calls])),
               moves_with_positive_delta=int(sum(int((d > 0).sum()) for d in delta)),
               best_gain_over_best_nni_gain=[float(d.max() / max(e.max(), 1e-300)) if len(d) and len(e) and e.max() > 0 else None
                                             for d, e in zip(delta, nni_delta)][:8],
               stage=dict(num_search_rounds=args.num_search_rounds, num_rounds=args.num_rounds, spr=spr_stage, nni=nni_stage))
    if args.baseline:
        index = {v: i for i, v in enumerate(trees[big].nodes())}
        fitted = Tree()
        fitted.add_nodes(trees[big].nodes())
        fitted.add_edges([(u, v, float(grid[tau[index[v]]])) for u, v, _ in trees[big].edges()])
        walls, worst = [], 0.0
        for rep in range(1 + args.repeats):
            t0 = time.perf_counter()
            for k, mv in enumerate(moves[big][pick]):
                want = tree_likelihood_batch([apply_spr(fitted, [mv], grid)], [codes[big]], None, Q, pi, [rates[big]])[0]
                worst = max(worst, float(np.abs(np.asarray(want) - ll_scan[k]).max()))
            walls.append((time.perf_counter() - t0) * 1e3 / len(pick))
        rec["baseline"] = dict(what=f"{len(pick)} moves of the largest family ({fams[big]}: {len(trees[big].nodes())} nodes, "
                                    f"{len(rates[big])} sites, {len(moves[big])} moves), one tree_likelihood_batch call per "
                                    "rearranged tree",
                               wall_ms_per_move=walls[1:], max_abs_per_site_difference_to_the_scan=worst)
    print(json.dumps(rec, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
