"""Time the site-rate scan (`cb_tree_site_rates`: csrc/sr.hip.h `sr_scan_kernel` / `sr_pick_kernel` behind the library's expm
bank) on the `nj_ml_trees` output of the 32 demo families (tests/golden/demo32_co_inputs.npz alignments) under LG.  Reports the
kernel time of the banks and of the scan with the pick (HIP events), the wall time of the call, the wall time of the alternating
stage `ml_lengths_and_site_rates` and the log-likelihood summed over the families after every half of every outer iteration.

    python profiles/tools/time_sr.py [--baseline] [--recovery] [--out profiles/sr_demo32.json]

--baseline times the only route to the same numbers without the scan: one `tree_likelihood_batch` call per candidate, every
unit rate of every family set to that candidate (the candidates of the scan are per family; the route takes, per call, the c-th
candidate of every family that has one).  --recovery runs the simulated experiment of EXPERIMENTS.md section 17.
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


def _rounds(path):
    rows = [ln.split() for ln in open(path).read().split("\n")[:-1]]
    return [r for r in rows if r[0] != "final"], float(rows[-1][1])


def demo(args):
    from conftest import load_golden
    from time_nj import _msas

    from cherryml_amd import ml_lengths_and_site_rates, nj_ml_trees, tree_site_rates
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation import tree_likelihood_batch
    from cherryml_amd.evaluation._likelihood import _family_units, _stationary_distribution
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation import rate_categories_ble
    fams, texts = _msas()
    Q = np.ascontiguousarray(load_golden("likelihood.npz")["lg"], dtype=np.float64)
    pi = _stationary_distribution(Q)
    R = args.num_rate_categories
    with tempfile.TemporaryDirectory() as tmp:
        msa = os.path.join(tmp, "msa")
        os.makedirs(msa)
        for fam, text in zip(fams, texts):
            with open(os.path.join(msa, fam + ".txt"), "wb") as f:
                f.write(text)
        qpath = os.path.join(tmp, "lg.txt")
        write_rate_matrix(Q, AA, qpath)
        ml = nj_ml_trees(msa_dir=msa, families=fams, rate_matrix_path=qpath, num_rate_categories=R, num_rounds=args.num_rounds,
                         **{k: os.path.join(tmp, "ml_" + k) for k in KEYS3})
        trees = [read_tree(os.path.join(ml["output_tree_dir"], fam + ".txt")) for fam in fams]
        rates = [np.asarray(read_site_rates(os.path.join(ml["output_site_rates_dir"], fam + ".txt"))) for fam in fams]
        codes = [_family_units(t, read_msa(os.path.join(msa, fam + ".txt")), None, len(r), AA, False)[2]
                 for t, r, fam in zip(trees, rates, fams)]
        ll_in = [float(open(os.path.join(ml["output_likelihood_dir"], fam + ".txt")).readline()) for fam in fams]
        # the alternating stage, as a user calls it
        out = {k: os.path.join(tmp, "sr_" + k) for k in KEYS3}
        t0 = time.perf_counter()
        ml_lengths_and_site_rates(tree_dir=ml["output_tree_dir"], msa_dir=msa, site_rates_dir=ml["output_site_rates_dir"],
                                  families=fams, rate_matrix_path=qpath, num_rate_categories=R,
                                  num_outer_iterations=args.num_outer_iterations, num_rounds=args.num_rounds, **out)
        stage_wall = time.perf_counter() - t0
        logs = [_rounds(os.path.join(out["output_tree_dir"], fam + ".rounds")) for fam in fams]
        ll_file = [float(open(os.path.join(out["output_likelihood_dir"], fam + ".txt")).readline()) for fam in fams]
    cands = [np.unique(np.r_[rate_categories_ble(R), r]) for r in rates]
    current = [np.searchsorted(c, r).astype(np.int32) for c, r in zip(cands, rates)]
    # the call alone: once to warm up, then timed
    calls = []
    for _ in range(1 + args.repeats):
        prof = {}
        t0 = time.perf_counter()
        res = tree_site_rates(trees, codes, cands, current, Q, pi, return_all=True, profile=prof)
        calls.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, **prof))
    calls = calls[1:]
    rec = dict(what=f"cb_tree_site_rates on the nj_ml_trees output of the 32 demo families under LG, {R} rate categories offered, "
                    "one MI355X",
               families=len(fams), nodes=int(sum(len(t.nodes()) for t in trees)), sites=int(sum(len(r) for r in rates)),
               candidates=dict(min=int(min(c.size for c in cands)), max=int(max(c.size for c in cands)),
                               total=int(sum(c.size for c in cands))),
               node_candidate_sites=int(sum(len(t.nodes()) * c.size * len(r) for t, c, r in zip(trees, cands, rates))),
               scan_and_pick_launches=int(sum(_height(t) + 2 for t in trees)),   # one per height, one pick (one chunk)
               calls=calls, sites_moved_by_one_scan=int(sum(int((b != k).sum()) for (b, _, _), k in zip(res, current))),
               log_likelihood_in=float(sum(ll_in)), log_likelihood_after_one_scan=float(sum(bl.sum() for _, bl, _ in res)),
               stage=dict(wall_s=stage_wall, num_outer_iterations=args.num_outer_iterations, num_rounds=args.num_rounds,
                          outer_iterations_run=int(max(len(rows) for rows, _ in logs) // 2),
                          per_half=[dict(half=f"{i // 2} {('lengths', 'rates')[i % 2]}",
                                         log_likelihood_before=float(sum(float(rows[i][2]) for rows, _ in logs if i < len(rows))),
                                         log_likelihood_after=float(sum(float(rows[i][3]) for rows, _ in logs if i < len(rows))),
                                         changed=int(sum(int(rows[i][4]) for rows, _ in logs if i < len(rows))))
                                    for i in range(max(len(rows) for rows, _ in logs))],
                          log_likelihood_final=float(sum(fin for _, fin in logs)), likelihood_files=float(sum(ll_file))))
    if args.baseline:
        # the only route to ll_all without the scan: tree_likelihood_batch per candidate at all-equal unit rates
        walls = []
        for _ in range(1 + args.repeats):
            t0 = time.perf_counter()
            worst = 0.0
            for c in range(max(cd.size for cd in cands)):
                have = [f for f in range(len(fams)) if c < cands[f].size]
                want = tree_likelihood_batch([trees[f] for f in have], [codes[f] for f in have], None, Q, pi,
                                             [np.full(len(rates[f]), cands[f][c]) for f in have])
                worst = max(worst, max(float(np.abs(np.asarray(w) - res[f][2][c]).max()) for f, w in zip(have, want)))
            walls.append((time.perf_counter() - t0) * 1e3)
        rec["baseline"] = dict(what="one tree_likelihood_batch call per candidate, every unit rate = the candidate",
                               wall_ms=walls[1:], max_abs_difference_to_the_scan=worst)
    return rec


def _height(tree):
    h = {}
    for v in tree.postorder_traversal():
        h[v] = 1 + max((h[c] for c, _ in tree.children(v)), default=-1)
    return max(h.values())


def recovery(args):
    """one 64-leaf tree with grid lengths, 400 sites whose true rates are the offered categories, leaves from simulate_msas;
    nj_trees gives a tree and FastCherries' rates, ml_lengths_and_site_rates refits lengths and rates"""
    from bl_cases import GRID, random_tree
    from conftest import load_golden

    from cherryml_amd import ml_lengths_and_site_rates, nj_trees, simulate_msas
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.io import Tree, write_contact_map, write_probability_distribution, write_rate_matrix, write_tree
    from cherryml_amd.phylogeny_estimation import rate_categories_ble
    z = load_golden("likelihood.npz")
    Q, pi = z["lg"], z["pi_lg"]
    R, L, n_leaves = args.num_rate_categories, 400, 64
    grid, rng = np.array(GRID), np.random.default_rng(2025)
    parent = random_tree(n_leaves, rng)
    length = np.where(parent >= 0, grid[rng.integers(50, 85, len(parent))], 0.0)
    offered = np.array(rate_categories_ble(R))
    true = rng.integers(0, R, L)
    tree = Tree()
    tree.add_nodes([f"n{v}" for v in range(len(parent))])
    tree.add_edges([(f"n{p}", f"n{v}", float(length[v])) for v, p in enumerate(parent) if p >= 0])
    with tempfile.TemporaryDirectory() as tmp:
        p = lambda *a: os.path.join(tmp, *a)   # noqa: E731
        for d in ("tree", "rates", "cm", "model", "msa"):
            os.makedirs(p(d))
        write_tree(tree, p("tree", "f.txt"))
        with open(p("rates", "f.txt"), "w") as f:
            f.write(f"{L} sites\n" + " ".join(repr(float(r)) for r in offered[true]))
        write_contact_map(np.zeros((L, L), dtype=int), p("cm", "f.txt"))
        pairs, I = [a + b for a in AA for b in AA], np.eye(20)
        write_rate_matrix(Q, AA, p("model", "Q1.txt"))
        write_probability_distribution(pi, AA, p("model", "p1.txt"))
        write_rate_matrix(np.kron(Q, I) + np.kron(I, Q), pairs, p("model", "Q2.txt"))
        write_probability_distribution(np.kron(pi, pi), pairs, p("model", "p2.txt"))
        simulate_msas(tree_dir=p("tree"), site_rates_dir=p("rates"), contact_map_dir=p("cm"), families=["f"], amino_acids=AA,
                      pi_1_path=p("model", "p1.txt"), Q_1_path=p("model", "Q1.txt"), pi_2_path=p("model", "p2.txt"),
                      Q_2_path=p("model", "Q2.txt"), strategy="all_transitions", random_seed=7, output_msa_dir=p("msa_all"))
        leaves = set(tree.leaves())
        with open(p("msa", "f.txt"), "w") as f:
            f.write("".join(f">{n}\n{s}\n" for n, s in read_msa(p("msa_all", "f.txt")).items() if n in leaves))
        nj = {k: p("nj_" + k) for k in KEYS3}
        nj_trees(msa_dir=p("msa"), families=["f"], rate_matrix_path=p("model", "Q1.txt"), num_rate_categories=R, **nj)
        out = {k: p("sr_" + k) for k in KEYS3}
        ml_lengths_and_site_rates(tree_dir=nj["output_tree_dir"], msa_dir=p("msa"), site_rates_dir=nj["output_site_rates_dir"],
                                  families=["f"], rate_matrix_path=p("model", "Q1.txt"), num_rate_categories=R,
                                  num_outer_iterations=args.num_outer_iterations, num_rounds=args.num_rounds, **out)

        def near(path):   # in log distance the nearest offered category: the true one, or the true one or a neighbour
            k = np.abs(np.log(np.asarray(read_site_rates(path)))[:, None] - np.log(offered)[None, :]).argmin(axis=1)
            return dict(true_category=float((k == true).mean()), true_or_neighbour=float((np.abs(k - true) <= 1).mean()))
        rows, final = _rounds(os.path.join(out["output_tree_dir"], "f.rounds"))
        return dict(what=f"{n_leaves} leaves, {L} sites, true rates uniform over the {R} offered categories, LG; nj_trees, then "
                         f"ml_lengths_and_site_rates ({args.num_outer_iterations} outer iterations of {args.num_rounds} rounds)",
                    fast_cherries=dict(log_likelihood=float(open(os.path.join(nj["output_likelihood_dir"], "f.txt")).readline()),
                                       **near(os.path.join(nj["output_site_rates_dir"], "f.txt"))),
                    refitted=dict(log_likelihood=float(open(os.path.join(out["output_likelihood_dir"], "f.txt")).readline()),
                                  **near(os.path.join(out["output_site_rates_dir"], "f.txt"))),
                    rounds=[" ".join(r) for r in rows], final=final)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-rounds", type=int, default=10)
    ap.add_argument("--num-outer-iterations", type=int, default=3)
    ap.add_argument("--num-rate-categories", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--recovery", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = demo(args)
    if args.recovery:
        rec["recovery"] = recovery(args)
    print(json.dumps(rec, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
