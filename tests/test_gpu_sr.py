"""The site-rate scan on the GPU (csrc/sr.hip.h, cb_tree_site_rates, tree_site_rates / ml_site_rates /
ml_lengths_and_site_rates / nj_ml_rates_trees): the scan against the NumPy restatement on integers and against the held-out
likelihood, determinism and batching, the stages with their files and caches, the pipeline that takes the estimator, and a small
simulated family."""
import os
import sys
from functools import partial

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bl_cases  # noqa: E402
import sr_cases  # noqa: E402
from conftest import load_golden  # noqa: E402

AA = list("ARNDCQEGHILKMFPSTWYV")


def _tree(parent, length):
    from cherryml_amd.io import Tree
    t = Tree()
    t.add_nodes([f"n{v}" for v in range(len(parent))])
    t.add_edges([(f"n{p}", f"n{v}", float(length[v])) for v, p in enumerate(parent) if p >= 0])
    return t


def _scan(name, fams, current, **kw):
    from cherryml_amd import tree_site_rates
    Q, pi = sr_cases.model_of(name)
    return tree_site_rates([_tree(f[0], f[1]) for f in fams], [f[2] for f in fams], [f[3] for f in fams], current, Q, pi,
                           return_all=True, **kw)


@pytest.mark.parametrize("name", sr_cases.CASES)
def test_the_scan_equals_the_restatement_on_integers(name):
    """the cases of tests/sr_cases.py: S = 4, 20, 32; a 3-leaf star, a 9-leaf caterpillar, a 17-leaf tree with a trifurcating root,
    a multifurcating internal node; 1, 2, 7 and 70 sites; 1, 5 and 40 candidates; lengths 0, on the grid, off it and beyond both
    ends; 25 % gaps, an all-gap leaf, an all-gap site, a site with exactly one observed leaf; current NULL, all -1 and a mix; two
    families of different size per call; a reversible model and one that is not, with a root distribution that is not its
    stationary one.  The log-likelihoods to 1e-10 of their size (of 1 below it: an all-gap site's is 0),
    the picks exactly on EVERY site with two or more observed leaves (tests/test_sr_cpu.py: all their margins exceed 1e-9)."""
    S, fams, current = sr_cases.case(name)
    want = sr_cases.restated(name)
    got = _scan(name, fams, current)
    for k, (r, (best, best_ll, ll_all)) in enumerate(zip(want, got)):
        assert ll_all.shape == r["ll"].shape and best.dtype == np.int32
        err = np.abs(ll_all - r["ll"]) / np.maximum(np.abs(r["ll"]), 1.0)
        decided = r["n_obs"] >= 2
        print(f"{name}[{k}]: max relative |d ll| = {err.max():.2e}; {decided.sum()} of {decided.size} sites decided by the "
              f"likelihoods, smallest margin {r['margin'][decided].min() if decided.any() else np.inf:.2e}")
        assert err.max() < 1e-10
        assert np.array_equal(best[decided], r["best"][decided]), (k, best, r["best"])
        keep = np.zeros(best.size, dtype=np.int64) if current is None else np.maximum(current[k], 0)
        assert np.array_equal(best[~decided], keep[~decided])               # the codes decide: current, or candidate 0
        assert np.array_equal(best_ll, ll_all[best, np.arange(best.size)])  # bit for bit


@pytest.mark.parametrize("name", sr_cases.CASES)
def test_every_column_equals_the_held_out_likelihood(name):
    """column c = tree_likelihood_batch on the same trees with every unit rate set to cands[c] (one batch: a copy of the family
    per candidate); the bar of test_the_fitted_likelihood_equals_the_held_out_likelihood, per site"""
    from cherryml_amd.evaluation import tree_likelihood_batch
    S, fams, current = sr_cases.case(name)
    Q, pi = sr_cases.model_of(name)
    got = _scan(name, fams, current)
    trees, codes, rates = [], [], []
    for parent, length, cd, cands in fams:
        for r in cands:
            trees.append(_tree(parent, length)), codes.append(cd), rates.append(np.full(cd.shape[1], r))
    want = tree_likelihood_batch(trees, codes, None, Q, pi, rates, reversible=name != "s4general")
    at = 0
    for k, (_, _, ll_all) in enumerate(got):
        w = np.array(want[at:at + ll_all.shape[0]])
        at += ll_all.shape[0]
        err = np.abs(ll_all - w).max()
        print(f"{name}[{k}]: against tree_likelihood_batch, max |d ll| = {err:.2e}")
        assert err < 1e-10


def _equal(a, b):
    return all(np.array_equal(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb))


def test_two_calls_agree_bitwise_and_a_family_alone_gets_its_batch_results(monkeypatch):
    S, fams, current = sr_cases.case("s20")
    both = _scan("s20", fams, current)
    assert _equal(both, _scan("s20", fams, current))
    for k, f in enumerate(fams):
        alone = _scan("s20", [f], [current[k]])
        assert _equal(alone, [both[k]]), k
    # the candidates in chunks of one (the bound on a chunk's messages, through the test hook): the same bits
    monkeypatch.setenv("CB_SR_MSG_BYTES", "1")
    assert _equal(both, _scan("s20", fams, current))
    monkeypatch.setenv("CB_SR_MSG_BYTES", str(3 * 17 * 7 * 20 * 8))   # three candidates of the first family at a time
    assert _equal(both, _scan("s20", fams, current))


def _demo_msas(tmp_path, k):
    z = load_golden("demo_e2e.npz")
    fams = [str(f) for f in z["families"]]
    small = sorted(range(len(fams)), key=lambda i: (len(str(z["text_msa"][i])), fams[i]))[:k]
    (tmp_path / "msa").mkdir()
    for i in small:
        (tmp_path / "msa" / f"{fams[i]}.txt").write_text(str(z["text_msa"][i]))
    return z, [fams[i] for i in small]


def _likelihood_file(path):
    lines = open(path).read().split("\n")
    return float(lines[0]), np.array([float(x) for x in lines[2].split()])


def _inputs(tree_dir, msa_dir, rates_dir, fam):
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation._likelihood import _family_units
    from cherryml_amd.io import read_tree
    tree = read_tree(os.path.join(tree_dir, fam + ".txt"))
    rates = np.asarray(read_site_rates(os.path.join(rates_dir, fam + ".txt")))
    return tree, rates, _family_units(tree, read_msa(os.path.join(msa_dir, fam + ".txt")), None, len(rates), AA, False)[2]


def test_ml_site_rates_its_files_and_its_cache(tmp_path, monkeypatch):
    from cherryml_amd import caching, ml_site_rates, nj_trees, tree_site_rates
    from cherryml_amd.evaluation._likelihood import _stationary_distribution
    from cherryml_amd.io import write_rate_matrix
    from cherryml_amd.phylogeny_estimation import _site_rates, rate_categories_ble
    z, fams = _demo_msas(tmp_path, 2)
    msa_dir, qpath = str(tmp_path / "msa"), str(tmp_path / "q0.txt")
    Q = np.ascontiguousarray(z["lg_Q_best_f64"], dtype=np.float64)
    write_rate_matrix(Q, AA, qpath)
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        nj = nj_trees(msa_dir=msa_dir, families=fams, rate_matrix_path=qpath, num_rate_categories=4)
        args = dict(tree_dir=nj["output_tree_dir"], msa_dir=msa_dir, site_rates_dir=nj["output_site_rates_dir"], families=fams,
                    rate_matrix_path=qpath, num_rate_categories=4)
        out = ml_site_rates(**args)
        monkeypatch.setattr(_site_rates, "_scan", lambda *a: pytest.fail("the second call ran the scan"))
        assert ml_site_rates(**args) == out                                      # the cache
        monkeypatch.undo()
    finally:
        caching.set_cache_dir(None)
    assert str(tmp_path / "cache" / "ml_site_rates") in out["output_site_rates_dir"]
    for fam in fams:
        tree, r_in, codes = _inputs(nj["output_tree_dir"], msa_dir, nj["output_site_rates_dir"], fam)
        _, r_out, _ = _inputs(nj["output_tree_dir"], msa_dir, out["output_site_rates_dir"], fam)
        cands = np.unique(np.r_[rate_categories_ble(4), r_in])
        assert 4 <= cands.size <= 8 and np.all(np.isin(r_out, cands))            # as picked: no normalisation
        current = np.searchsorted(cands, r_in).astype(np.int32)
        (best, best_ll, ll_all), = tree_site_rates([tree], [codes], cands, [current], Q, _stationary_distribution(Q), return_all=True)
        assert np.array_equal(cands[best], r_out)
        total, per_site = _likelihood_file(os.path.join(out["output_likelihood_dir"], fam + ".txt"))
        total_in, per_site_in = _likelihood_file(os.path.join(nj["output_likelihood_dir"], fam + ".txt"))
        print(f"{fam}: {int((best != current).sum())} of {best.size} sites moved, log-likelihood {total_in:.4f} -> {total:.4f}; "
              f"max |file - picked column| = {np.abs(per_site - best_ll).max():.2e}")
        assert np.abs(per_site - best_ll).max() < 1e-10 and abs(total - best_ll.sum()) < 1e-10 * best.size
        assert np.all(per_site >= per_site_in - 1e-10)                           # no site below its input rate's likelihood
        assert np.all(best_ll >= ll_all[current, np.arange(best.size)])          # (exactly, in the scan's own columns)
        assert total > total_in
        prof = open(os.path.join(out["output_site_rates_dir"], fam + ".profiling")).read()
        assert prof.split("\n")[-1].startswith("total_time: ") and "scan_kernel_ms: " in prof


def _rounds(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[-2].startswith("final ")
    rows = [ln.split() for ln in lines[:-2]]
    assert [(r[0], r[1]) for r in rows] == [(str(k // 2), ("lengths", "rates")[k % 2]) for k in range(len(rows))], rows
    lls = [float(x) for r in rows for x in r[2:4]] + [float(lines[-2].split()[1])]
    return rows, lls


def test_ml_lengths_and_site_rates_never_lowers_a_likelihood_and_its_output_is_a_fixed_point(tmp_path):
    from cherryml_amd import caching, ml_lengths_and_site_rates, nj_trees
    from cherryml_amd.io import write_rate_matrix
    z, fams = _demo_msas(tmp_path, 3)
    msa_dir, qpath = str(tmp_path / "msa"), str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        nj = nj_trees(msa_dir=msa_dir, families=fams, rate_matrix_path=qpath, num_rate_categories=4)
        args = dict(msa_dir=msa_dir, families=fams, rate_matrix_path=qpath, num_rate_categories=4, num_outer_iterations=40,
                    num_rounds=40)
        out = ml_lengths_and_site_rates(tree_dir=nj["output_tree_dir"], site_rates_dir=nj["output_site_rates_dir"], **args)
        again = ml_lengths_and_site_rates(tree_dir=out["output_tree_dir"], site_rates_dir=out["output_site_rates_dir"], **args)
    finally:
        caching.set_cache_dir(None)
    for fam in fams:
        rows, lls = _rounds(os.path.join(out["output_tree_dir"], fam + ".rounds"))
        print(f"{fam}: {len(rows) // 2} outer iterations, log-likelihoods {lls[0]:.4f} -> {lls[-1]:.4f}, changed "
              f"{[int(r[4]) for r in rows]}")
        assert len(rows) >= 4 and len(rows) < 80                                 # it moved, and it stopped by itself
        assert all(b >= a - 1e-10 * abs(a) for a, b in zip(lls, lls[1:])), lls   # rounding only
        assert lls[-1] > lls[0]
        total, per_site = _likelihood_file(os.path.join(out["output_likelihood_dir"], fam + ".txt"))
        total_nj, _ = _likelihood_file(os.path.join(nj["output_likelihood_dir"], fam + ".txt"))
        assert abs(total - lls[-1]) < 1e-10 * per_site.size and total > total_nj
        # a run from its own output changes nothing
        rows2, lls2 = _rounds(os.path.join(again["output_tree_dir"], fam + ".rounds"))
        assert len(rows2) == 2 and rows2[0][4] == "0" and rows2[1][4] == "0", rows2
        assert all(abs(x - lls[-1]) <= 1e-10 * abs(lls[-1]) for x in lls2), (lls2, lls[-1])
        for key in ("output_tree_dir", "output_site_rates_dir"):
            assert open(os.path.join(again[key], fam + ".txt")).read() == open(os.path.join(out[key], fam + ".txt")).read()


def test_the_em_pipeline_takes_nj_ml_rates_trees_as_its_tree_estimator(tmp_path):
    import cherryml_amd
    from cherryml_amd import caching, nj_ml_rates_trees
    from cherryml_amd.io import read_rate_matrix, write_rate_matrix
    z, fams = _demo_msas(tmp_path, 1)
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    cache = tmp_path / "cache"
    caching.set_cache_dir(str(cache))
    try:
        res = cherryml_amd.lg_end_to_end_with_em_optimizer(
            msa_dir=str(tmp_path / "msa"), families=fams,
            tree_estimator=partial(nj_ml_rates_trees, num_rate_categories=4, num_rounds=3, num_outer_iterations=2),
            initial_tree_estimator_rate_matrix_path=qpath, num_iterations=1, em_iterations=2, optimizer_initialization=qpath)
    finally:
        caching.set_cache_dir(None)
    Q = read_rate_matrix(res["learned_rate_matrix_path"]).to_numpy()
    assert Q.shape == (20, 20) and np.all(np.isfinite(Q)) and np.allclose(Q.sum(1), 0.0, atol=1e-9)
    dirs = res["tree_estimator_output_dirs_0"]
    for key in ("output_tree_dir", "output_site_rates_dir", "output_likelihood_dir"):   # the refitted ones, the rates included
        assert str(cache / "ml_lengths_and_site_rates") in dirs[key], dirs
    rows, _ = _rounds(os.path.join(dirs["output_tree_dir"], fams[0] + ".rounds"))
    assert 2 <= len(rows) <= 4
    assert len(os.listdir(cache / "nj_trees")) == 1 and len(os.listdir(cache / "ml_lengths_and_site_rates")) == 1


def test_a_simulated_family_is_no_less_likely_at_the_refitted_rates(tmp_path):
    """the small form of EXPERIMENTS section 17: 24 leaves, 160 sites whose true rates are the 4 offered categories, leaves from
    simulate_msas; nj_trees gives the tree and FastCherries' rates, the alternating stage refits both.  Asserted: the likelihood
    does not go down.  Printed: how many sites sit at the true category or a neighbour of it, before and after."""
    from cherryml_amd import ml_lengths_and_site_rates, nj_trees, simulate_msas
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.io import write_contact_map, write_probability_distribution, write_rate_matrix, write_tree
    from cherryml_amd.phylogeny_estimation import rate_categories_ble
    z = load_golden("likelihood.npz")
    Q, pi = z["lg"], z["pi_lg"]
    grid = np.array(bl_cases.GRID)
    rng = np.random.default_rng(77)
    parent = bl_cases.random_tree(24, rng)
    length = np.where(parent >= 0, grid[rng.integers(55, 85, len(parent))], 0.0)
    L = 160
    offered = np.array(rate_categories_ble(4))
    true = rng.permutation(np.repeat(np.arange(4), L // 4))
    for d in ("tree", "rates", "cm", "model"):
        (tmp_path / d).mkdir()
    tree = _tree(parent, length)
    write_tree(tree, str(tmp_path / "tree" / "f.txt"))
    (tmp_path / "rates" / "f.txt").write_text(f"{L} sites\n" + " ".join(repr(float(r)) for r in offered[true]))
    write_contact_map(np.zeros((L, L), dtype=int), str(tmp_path / "cm" / "f.txt"))
    pairs = [a + b for a in AA for b in AA]
    I = np.eye(20)
    write_rate_matrix(Q, AA, str(tmp_path / "model" / "Q1.txt"))
    write_probability_distribution(pi, AA, str(tmp_path / "model" / "p1.txt"))
    write_rate_matrix(np.kron(Q, I) + np.kron(I, Q), pairs, str(tmp_path / "model" / "Q2.txt"))
    write_probability_distribution(np.kron(pi, pi), pairs, str(tmp_path / "model" / "p2.txt"))
    simulate_msas(tree_dir=str(tmp_path / "tree"), site_rates_dir=str(tmp_path / "rates"), contact_map_dir=str(tmp_path / "cm"),
                  families=["f"], amino_acids=AA, pi_1_path=str(tmp_path / "model" / "p1.txt"),
                  Q_1_path=str(tmp_path / "model" / "Q1.txt"), pi_2_path=str(tmp_path / "model" / "p2.txt"),
                  Q_2_path=str(tmp_path / "model" / "Q2.txt"), strategy="all_transitions", random_seed=7,
                  output_msa_dir=str(tmp_path / "msa_all"))
    leaves = set(tree.leaves())
    (tmp_path / "msa").mkdir()
    (tmp_path / "msa" / "f.txt").write_text("".join(
        f">{name}\n{seq}\n" for name, seq in read_msa(str(tmp_path / "msa_all" / "f.txt")).items() if name in leaves))
    qpath = str(tmp_path / "model" / "Q1.txt")
    nj = {k: str(tmp_path / ("nj_" + k)) for k in ("output_tree_dir", "output_site_rates_dir", "output_likelihood_dir")}
    nj_trees(msa_dir=str(tmp_path / "msa"), families=["f"], rate_matrix_path=qpath, num_rate_categories=4, **nj)
    out = {k: str(tmp_path / ("ml_" + k)) for k in ("output_tree_dir", "output_site_rates_dir", "output_likelihood_dir")}
    ml_lengths_and_site_rates(tree_dir=nj["output_tree_dir"], msa_dir=str(tmp_path / "msa"), site_rates_dir=nj["output_site_rates_dir"],
                              families=["f"], rate_matrix_path=qpath, num_rate_categories=4, **out)
    ll_fc, _ = _likelihood_file(os.path.join(nj["output_likelihood_dir"], "f.txt"))
    ll_ml, _ = _likelihood_file(os.path.join(out["output_likelihood_dir"], "f.txt"))
    _, lls = _rounds(os.path.join(out["output_tree_dir"], "f.rounds"))

    def near(path):   # the share of sites whose rate is, in log distance, nearest to the true category or a neighbour of it
        r = np.asarray(read_site_rates(path))
        k = np.abs(np.log(r)[:, None] - np.log(offered)[None, :]).argmin(axis=1)
        return float((np.abs(k - true) <= 1).mean())
    print(f"log-likelihood at FastCherries' rates {ll_fc:.4f}, refitted {ll_ml:.4f} (rounds file {lls[0]:.4f} -> {lls[-1]:.4f}); "
          f"sites at the true category or a neighbour: FastCherries {near(os.path.join(nj['output_site_rates_dir'], 'f.txt')):.3f}, "
          f"refitted {near(os.path.join(out['output_site_rates_dir'], 'f.txt')):.3f}")
    assert ll_ml >= ll_fc
    assert all(b >= a - 1e-10 * abs(a) for a, b in zip(lls, lls[1:])), lls

