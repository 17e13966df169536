"""Time the marginal ancestral reconstruction (`cb_bl_ancestral`: csrc/anc.hip.h `anc_post_kernel` on the resident messages of
the branch-length handle) and the stage `ml_ancestral_sequences` on the `nj_ml_trees` output of the 32 demo families
(tests/golden/demo32_co_inputs.npz alignments) under LG.  Reports the (node, site) entries reconstructed, the kernel time of the
passes and of the reconstruction (HIP events) and the wall time of the call, with and without the posteriors, the launches, the
creation of the handle, the bytes the kernel moves, and for the stage (without posterior files) its wall time.

    python profiles/tools/time_anc.py [--baseline] [--out profiles/anc_demo32.json]

--baseline imputes gapped leaf characters the only way there is without the kernel: for a gapped leaf, S `tree_likelihood_batch`
calls, one per state put at its gapped sites, normalised per site.  It does so for a few gapped leaves of the smallest family,
reports the time per leaf and the largest distance to the kernel's posterior, and the ratio of that route over all gapped
leaves of the family to one `ancestral_states` call on the family alone (which also covers every internal node).
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--baseline-leaves", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from conftest import load_golden
    from time_nj import _msas
    from time_nni import _pass_launches

    from cherryml_amd import BranchLengthFitter, ml_ancestral_sequences, nj_ml_trees
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation import tree_likelihood_batch
    from cherryml_amd.evaluation._likelihood import _family_units, _stationary_distribution
    from cherryml_amd.io import Tree, read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    fams, texts = _msas()
    Q = np.ascontiguousarray(load_golden("likelihood.npz")["lg"], dtype=np.float64)
    pi = _stationary_distribution(Q)
    S = Q.shape[0]
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
        # the stage, as a user calls it (without the posterior files: on these families they would hold 2.4 GB)
        out = dict(output_msa_dir=os.path.join(tmp, "anc_msa"), output_confidence_dir=os.path.join(tmp, "anc_conf"))
        t0 = time.perf_counter()
        ml_ancestral_sequences(tree_dir=ml["output_tree_dir"], msa_dir=msa, site_rates_dir=ml["output_site_rates_dir"],
                               families=fams, rate_matrix_path=qpath, **out)
        stage = dict(wall_s=time.perf_counter() - t0)
        profs = [dict(ln.split(": ") for ln in open(os.path.join(out["output_msa_dir"], fam + ".profiling")).read().split("\n"))
                 for fam in fams]
        for key in ("create_time", "reconstruction_time"):
            stage[key + "_s"] = float(sum(float(p[key]) for p in profs))
    # the call alone, on one handle over all families: once to warm up, then timed
    t0 = time.perf_counter()
    fit = BranchLengthFitter(trees, codes, rates, grid, Q, pi)
    create_s = time.perf_counter() - t0
    calls = {False: [], True: []}
    with fit:
        for post in (False, True):
            for _ in range(1 + args.repeats):
                t0 = time.perf_counter()
                out = fit.ancestral_states(posteriors=post)
                calls[post].append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, passes_kernel_ms=fit.last_ancestral_kernel_ms[0],
                                        reconstruction_kernel_ms=fit.last_ancestral_kernel_ms[1]))
                state, conf = out[0], out[1]
                del out
        tau_all = fit.indices()
    entries = int(sum(len(t.nodes()) * len(r) for t, r in zip(trees, rates)))
    leaf_entries = int(sum(len(t.leaves()) * len(r) for t, r in zip(trees, rates)))
    gapped = int(sum(int((c[[t.is_leaf(v) for v in t.nodes()]] < 0).sum()) for t, c in zip(trees, codes)))
    # the message rows [S doubles] the kernel gathers, every row counted once per use: an internal node reads its children's messages
    # and (but the root) its U; a leaf reads its parent's U (but under the root) and its siblings' messages -- and the column of P
    # above it, which its tile's sites share through the caches and which is not counted
    rows = 0
    for t, r in zip(trees, rates):
        for v in t.nodes():
            if t.is_leaf(v):
                p = t.parent(v)[0]
                rows += len(r) * (len(t.children(p)) - 1 + (0 if t.is_root(p) else 1))
            else:
                rows += len(r) * (len(t.children(v)) + (0 if t.is_root(v) else 1))
    gather = rows * S * 8
    rec = dict(what="cb_bl_ancestral and ml_ancestral_sequences on the nj_ml_trees output of the 32 demo families under LG, one MI355X",
               families=len(fams), nodes=int(sum(len(t.nodes()) for t in trees)), sites=int(sum(len(r) for r in rates)),
               node_site_entries=entries, leaf_entries=leaf_entries, gapped_leaf_entries=gapped,
               reconstruction_launches=len(fams), pass_launches=int(sum(_pass_launches(t) for t in trees)),
               handle_create_s=create_s, calls_without_posteriors=calls[False][1:], calls_with_posteriors=calls[True][1:],
               reconstruction_kernel_ns_per_entry=float(np.mean([c["reconstruction_kernel_ms"] for c in calls[False][1:]]) * 1e6 / entries),
               reconstruction_kernel_ns_per_entry_with_posteriors=float(
                   np.mean([c["reconstruction_kernel_ms"] for c in calls[True][1:]]) * 1e6 / entries),
               bytes_model=dict(gathered_total=gather, gathered_per_entry=gather / entries, stored_state_conf_total=9 * entries,
                                stored_post_total=S * 8 * entries),
               mean_confidence_internal=float(np.mean([c[[not t.is_leaf(v) for v in t.nodes()]].mean() for t, c in zip(trees, conf)])),
               stage=stage)
    if args.baseline:
        order = np.argsort([len(t.nodes()) * len(r) for t, r in zip(trees, rates)])
        k = int(next(i for i in order if (codes[i][[trees[i].is_leaf(v) for v in trees[i].nodes()]] < 0).any()))
        nodes = list(trees[k].nodes())
        index = {v: i for i, v in enumerate(nodes)}
        fitted = Tree()
        fitted.add_nodes(nodes)
        fitted.add_edges([(u, v, float(grid[tau_all[k][index[v]]])) for u, v, _ in trees[k].edges()])
        with BranchLengthFitter([trees[k]], [codes[k]], [rates[k]], grid, Q, pi) as one:
            walls_one = []
            for _ in range(1 + args.repeats):
                t0 = time.perf_counter()
                _, _, post = one.ancestral_states(posteriors=True)
                walls_one.append((time.perf_counter() - t0) * 1e3)
        leaves = [i for i, v in enumerate(nodes) if trees[k].is_leaf(v) and (codes[k][i] < 0).any()]
        walls, worst = [], 0.0
        for rep in range(1 + args.repeats):
            t0 = time.perf_counter()
            for i in leaves[:args.baseline_leaves]:
                gaps = np.flatnonzero(codes[k][i] < 0)
                ll = []
                for a in range(S):
                    c = codes[k].copy()
                    c[i, gaps] = a
                    ll.append(np.asarray(tree_likelihood_batch([fitted], [c], None, Q, pi, [rates[k]])[0])[gaps])
                ll = np.array(ll)
                w = np.exp(ll - ll.max(axis=0, keepdims=True))
                worst = max(worst, float(np.abs((w / w.sum(axis=0, keepdims=True)).T - post[0][i, gaps]).max()))
            walls.append((time.perf_counter() - t0) * 1e3 / len(leaves[:args.baseline_leaves]))
        per_leaf = float(np.mean(walls[1:]))
        rec["baseline"] = dict(what=f"{len(leaves[:args.baseline_leaves])} of the {len(leaves)} gapped leaves of the smallest family "
                                    f"with gaps ({fams[k]}: {len(nodes)} nodes, {len(rates[k])} sites): {S} tree_likelihood_batch "
                                    "calls per leaf, one per state at its gapped sites",
                               wall_ms_per_leaf=walls[1:], max_abs_difference_to_the_kernels_posterior=worst,
                               ancestral_states_wall_ms_family_alone_with_posteriors=walls_one[1:],
                               ratio_all_gapped_leaves_to_one_call=per_leaf * len(leaves) / float(np.mean(walls_one[1:])))
    print(json.dumps(rec, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
