"""Time the bootstrap from the search's own trees (`cb_bl_bootstrap_best`: the NNI scan, then `sup_weights_kernel` and
csrc/ufb.hip.h `ufb_gemm_kernel` / `ufb_merge_kernel` on the scan's buffer) and the stage `ml_nni_trees` with and without
`output_bootstrap_dir` on the `nj_ml_trees` output of the 32 demo families (tests/golden/demo32_co_inputs.npz alignments) under
LG, with 1000 replicates.  Reports the moves, the kernel time of the passes, of the scan and of the resampling and reduction
(HIP events around them), the wall time of the call (three calls after a warm-up), the launches of a call, the stage's wall time
with and without the bootstrap and the time it spent in the new call, and the mean ufboot next to the mean SH-like support over
the final trees' edges.

    python profiles/tools/time_ufboot.py [--baseline] [--out profiles/ufboot_demo32.json]

--baseline is the only route to these numbers without the entry point: `nni_scan(per_site=True)` copies ll'[move][site] to the
host, where the same multiplicities (tests/sup_reference.py, timed on their own) meet it in a NumPy product and an argmax; it
reports the time of each part and compares the choices with the entry point's where the replicate is decided.
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


def _profile_sum(directory, fams, key):
    total = 0.0
    for fam in fams:
        for line in open(os.path.join(directory, fam + ".profiling")).read().split("\n"):
            if line.startswith(key + ": "):
                total += float(line.split(": ")[1])
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-rounds", type=int, default=10)
    ap.add_argument("--num-nni-rounds", type=int, default=10)
    ap.add_argument("--num-rate-categories", type=int, default=20)
    ap.add_argument("--num-replicates", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from conftest import load_golden
    from time_nj import _msas

    from cherryml_amd import BranchLengthFitter, ml_nni_trees, nj_ml_trees
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation._likelihood import _family_units, _stationary_distribution
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation import read_supports, read_ufboot_supports
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
        # the stage, as a user calls it: a warm-up (the first use of the device), then without and with the bootstrap, then
        # with the bootstrap and the local supports (for the mean SH-like support of the same edges)
        stage = {}
        for name, extra in (("warm_up", {}), ("plain", {}), ("bootstrap", dict(boot=True)), ("bootstrap_and_supports", dict(boot=True, sup=True))):
            out = os.path.join(tmp, "nni_" + name)
            kw = dict(output_tree_dir=os.path.join(out, "trees"), output_likelihood_dir=os.path.join(out, "ll"))
            if extra.get("boot"):
                kw.update(output_bootstrap_dir=os.path.join(out, "boot"), num_bootstrap_replicates=R)
            if extra.get("sup"):
                kw.update(output_support_dir=os.path.join(out, "sup"), num_support_replicates=R)
            t0 = time.perf_counter()
            ml_nni_trees(tree_dir=ml["output_tree_dir"], msa_dir=msa, site_rates_dir=ml["output_site_rates_dir"], families=fams,
                         rate_matrix_path=qpath, num_nni_rounds=args.num_nni_rounds, num_rounds=args.num_rounds, **kw)
            stage[name] = dict(wall_s=time.perf_counter() - t0)
            print(f"stage {name}: {stage[name]['wall_s']:.2f} s", file=sys.stderr, flush=True)
            if extra.get("boot"):
                rows = [[int(x) for x in ln.split()] for fam in fams
                        for ln in open(os.path.join(kw["output_bootstrap_dir"], fam + ".choices")).read().split("\n") if ln]
                stage[name].update(bootstrap_calls_wall_s=_profile_sum(kw["output_tree_dir"], fams, "bootstrap_time"),
                                   resampling_and_reduction_kernel_ms=_profile_sum(kw["output_tree_dir"], fams, "bootstrap_kernel_ms"),
                                   passes_and_scan_kernel_ms=_profile_sum(kw["output_tree_dir"], fams, "bootstrap_scan_kernel_ms"),
                                   contributions=len(rows), candidates=int(sum(r[2] for r in rows)),
                                   replicates_won_by_a_tree=int(sum(r[3] for r in rows)),
                                   replicates_won_by_a_neighbour=int(sum(r[4] for r in rows)))
            if extra.get("sup"):
                ufb, sh = [], []
                for fam in fams:
                    a = read_ufboot_supports(os.path.join(kw["output_bootstrap_dir"], fam + ".txt"))
                    b = read_supports(os.path.join(kw["output_support_dir"], fam + ".txt"))
                    assert list(a) == list(b)
                    ufb += list(a.values())
                    sh += [x[1] for x in b.values()]
                ufb, sh = np.array(ufb), np.array(sh)
                ok = np.isfinite(sh)
                stage[name].update(edges=int(ok.sum()), mean_ufboot=float(ufb[ok].mean()), mean_sh=float(sh[ok].mean()),
                                   edges_with_ufboot_at_least_0_95=int((ufb[ok] >= 0.95).sum()),
                                   edges_with_sh_at_least_0_95=int((sh[ok] >= 0.95).sum()))
        del stage["warm_up"]
    seeds = [family_seed(f, 0) for f in fams]
    t0 = time.perf_counter()
    fit = BranchLengthFitter(trees, codes, rates, grid, Q, pi)
    create_s = time.perf_counter() - t0
    calls = []
    with fit:
        moves = fit.nni_moves()
        for _ in range(1 + args.repeats):
            t0 = time.perf_counter()
            got = fit.bootstrap_best(R, seeds, base=True)
            ms = fit.last_ufboot_kernel_ms
            calls.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, passes_kernel_ms=ms[0], scan_kernel_ms=ms[1],
                              resampling_and_reduction_kernel_ms=ms[2]))
        fam_ll = fit.log_likelihoods()[1]
        calls = calls[1:]
        n_moves = int(sum(len(m) for m in moves))
        move_sites = int(sum(len(m) * len(r) for m, r in zip(moves, rates)))
        sites = int(sum(len(r) for r in rates))
        with_moves = int(sum(len(m) > 0 for m in moves))
        # per (move tile of 16, replicate tile of 128) a workgroup reads 16 rows of ll' and 128 rows of W, L doubles each
        tiles = [((len(m) + 15) // 16, (R + 127) // 128, len(r)) for m, r in zip(moves, rates)]
        rec = dict(what="cb_bl_bootstrap_best and ml_nni_trees(output_bootstrap_dir) on the nj_ml_trees output of the 32 demo "
                        "families under LG, one MI355X",
                   families=len(fams), nodes=int(sum(len(t.nodes()) for t in trees)), sites=sites, replicates=R, moves=n_moves,
                   move_sites=move_sites, product_flops=2.0 * (move_sites + sites) * R, weight_bytes=8.0 * R * sites,
                   operand_bytes_through_l2=float(sum(8.0 * L * (16 * a * b + 128 * a * b) for a, b, L in tiles)),
                   result_bytes=float(sum((8 + 4) * R * (1 + min(a, max(1, 1024 // b))) for a, b, _ in tiles)),
                   launches_per_call=dict(passes="as cb_bl_supports", weights=len(fams), base=len(fams), scan=with_moves,
                                          scan_sum=with_moves, product_with_argmax=with_moves, merge=len(fams)),
                   handle_create_s=create_s, calls=calls,
                   replicates_won_by_the_tree=int(sum(int((g[1] == -1).sum()) for g in got)),
                   stage=stage, num_nni_rounds=args.num_nni_rounds, num_rounds=args.num_rounds)
        if args.baseline:
            import sup_reference
            t0 = time.perf_counter()
            W = [sup_reference.weights(len(r), R, s).T.astype(np.float64) for r, s in zip(rates, seeds)]
            weights_s = time.perf_counter() - t0
            lls = fit.log_likelihoods()[0]
            scan_ms, host_ms = [], []
            for rep in range(1 + args.repeats):
                t0 = time.perf_counter()
                _, delta, ll_moves = fit.nni_scan(moves, per_site=True)
                t1 = time.perf_counter()
                ref = []
                for x, l, w, dl in zip(ll_moves, lls, W, delta):
                    base = np.where(np.isfinite(l), l, 0.0) @ w
                    d = np.where(np.isfinite(x) & np.isfinite(l)[None, :], x - l[None, :], 0.0)
                    cand = np.vstack([base[None, :], np.where(np.isfinite(dl)[:, None], base[None, :] + d @ w, -np.inf)])
                    ref.append(cand)
                arg = [np.argmax(c, axis=0) for c in ref]
                t2 = time.perf_counter()
                scan_ms.append((t1 - t0) * 1e3), host_ms.append((t2 - t1) * 1e3)
            worst = 0.0
            undecided = differ = 0
            for k, (cand, a, g) in enumerate(zip(ref, arg, got)):
                scale = max(1.0, abs(fam_ll[k]))
                top = np.sort(cand, axis=0)[-2:] if len(cand) > 1 else np.vstack([np.full(R, -np.inf), cand[0]])
                decided = top[1] - top[0] > 1e-9 * scale
                worst = max(worst, float(np.abs(g[0] - cand[a, np.arange(R)]).max()) / scale)
                undecided += int((~decided).sum())
                differ += int((g[1][decided] != a[decided] - 1).sum())
            rec["baseline"] = dict(what="nni_scan(per_site=True), then the product with the same multiplicities and the argmax in "
                                        "NumPy on the host",
                                   scan_per_site_call_ms=scan_ms[1:], host_product_and_argmax_ms=host_ms[1:],
                                   host_weights_s_not_counted=weights_s, max_score_difference_over_fam_ll=worst, bar_score=1e-10,
                                   replicates_undecided_at_1e_9=undecided, decided_choices_that_differ=differ)
    print(json.dumps(rec, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
