"""Branch-length EM on the GPU (csrc/bl.hip.h, cb_bl_*, BranchLengthFitter / ml_branch_lengths / nj_ml_trees): one round against
the NumPy restatement on integers, monotone rounds and fixed points, determinism and batching, the held-out likelihood, recovery
of simulated lengths, and the stage with the pipeline that takes it."""
import os
import sys
from functools import partial

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bl_cases  # noqa: E402
import bl_reference  # noqa: E402
from conftest import load_golden  # noqa: E402

AA = list("ARNDCQEGHILKMFPSTWYV")
MARGIN = 1e-9   # the rule of tests/test_gpu_nj.py: summation order moves a score by about 1e-13 of its size


def _tree(parent, length):
    from cherryml_amd.io import Tree
    t = Tree()
    t.add_nodes([f"n{v}" for v in range(len(parent))])
    t.add_edges([(f"n{p}", f"n{v}", float(length[v])) for v, p in enumerate(parent) if p >= 0])
    return t


def _fitter(S, grid, fams):
    from cherryml_amd import BranchLengthFitter
    Q, pi = bl_cases.model(S)
    return BranchLengthFitter([_tree(f[0], f[1]) for f in fams], [f[2] for f in fams], [f[3] for f in fams], grid, Q, pi)


@pytest.mark.parametrize("name", bl_cases.CASES)
def test_one_round_equals_the_restatement_on_integers(name):
    """S = 4, 20, 32; a 3-leaf star, a 9-leaf caterpillar, a 17-leaf tree with a trifurcating root, a multifurcating internal
    node; category segments of 1, 3, 4, 5 and > 64 sites; 1, 4 and 20 categories (a family's categories are its distinct rates,
    so "empty" categories are the rates of the shared list a family does not use); 25 % gaps and an all-gap leaf; input lengths
    0, off the grid and beyond its end; T = 129 and T = 5; two families of different size and category count per handle."""
    S, grid, fams = bl_cases.case(name)
    want = bl_cases.restated(name)
    with _fitter(S, grid, fams) as fit:
        start = fit.indices()
        site_ll, fam_ll0 = fit.log_likelihoods()
        n_changed, fam_ll = fit.round()
        got = fit.indices()
    edges = left_out = 0
    for k, (tau, r) in enumerate(want):
        assert np.array_equal(start[k], tau), (k, start[k], tau)          # the snapping: both clamps, the nearest point
        err = np.abs(site_ll[k] - r["ll"]).max()
        print(f"{name}[{k}]: max |d l_u| = {err:.2e}, smallest margin {r['margin'].min():.2e}")
        assert err < 1e-10                                                 # (the bar of test_estep_matches_the_numpy_restatement)
        assert fam_ll[k] == fam_ll0[k] and abs(fam_ll[k] - r["ll"].sum()) < 1e-9 * abs(fam_ll[k])
        sure = r["margin"] > MARGIN
        edges += int((tau >= 0).sum())
        left_out += int((~sure & (tau >= 0)).sum())
        assert np.array_equal(got[k][sure], r["tau"][sure]), (k, got[k], r["tau"])
        assert n_changed[k] == int((got[k] != start[k]).sum())
    assert left_out <= 0.02 * edges, (left_out, edges)


def _s20_families():
    return bl_cases.case("s20")[2] + bl_cases.case("s20one")[2]


def test_rounds_never_lower_a_likelihood_and_a_fixed_point_stays():
    fams = _s20_families()
    with _fitter(20, bl_cases.GRID, fams) as fit:
        lls, changed = [], []
        for _ in range(10):
            n_changed, fam_ll = fit.round()
            lls.append(fam_ll), changed.append(n_changed)
        lls = np.array(lls)
        print("log-likelihoods at the start of rounds 0 .. 9:\n", lls, "\nchanged:\n", np.array(changed))
        assert np.all(lls[1:] >= lls[:-1] - 1e-10 * np.abs(lls[:-1])), lls       # rounding only: an EM step cannot go down
        assert np.all(lls[-1] > lls[0])
        for _ in range(100):                                                     # on to the fixed point of every family
            if not n_changed.any():
                break
            prev = fam_ll
            n_changed, fam_ll = fit.round()
            assert np.all(fam_ll >= prev - 1e-10 * np.abs(prev))
        assert not n_changed.any(), n_changed
        at = fit.indices()
        again_changed, again_ll = fit.round()
        assert not again_changed.any() and np.array_equal(again_ll, fam_ll)      # bitwise
        assert all(np.array_equal(a, b) for a, b in zip(at, fit.indices()))
        assert np.array_equal(fit.log_likelihoods()[1], fam_ll)


def _five_rounds(fams):
    with _fitter(20, bl_cases.GRID, fams) as fit:
        for _ in range(5):
            fit.round()
        site_ll, fam_ll = fit.log_likelihoods()
        return fit.indices(), site_ll, fam_ll


def test_two_handles_agree_bitwise_and_a_family_alone_gets_its_batch_indices():
    fams = _s20_families()
    idx1, site1, fam1 = _five_rounds(fams)
    idx2, site2, fam2 = _five_rounds(fams)
    assert all(np.array_equal(a, b) for a, b in zip(idx1, idx2))
    assert all(np.array_equal(a, b) for a, b in zip(site1, site2)) and np.array_equal(fam1, fam2)
    for k, f in enumerate(fams):
        idx, _, fam = _five_rounds([f])
        assert np.array_equal(idx[0], idx1[k]), k
        assert fam[0] == fam1[k]


def test_the_fitted_likelihood_equals_the_held_out_likelihood():
    """the fitted lengths are grid points and the bank holds expm(grid[tau] rate Q): the model tree_likelihood evaluates, with
    another expm.  The bar of test_estep_loglik_equals_the_held_out_likelihood, per site; a family's sum moves by at most its
    number of sites times that."""
    from cherryml_amd.evaluation import tree_likelihood_batch
    fams = _s20_families()
    Q, pi = bl_cases.model(20)
    with _fitter(20, bl_cases.GRID, fams) as fit:
        for _ in range(5):
            fit.round()
        lengths = fit.lengths()
        site_ll, fam_ll = fit.log_likelihoods()
    trees = []
    for f, ln in zip(fams, lengths):
        assert set(ln.values()) <= set(bl_cases.GRID)
        trees.append(_tree(f[0], [ln.get(f"n{v}", 0.0) for v in range(len(f[0]))]))
    want = tree_likelihood_batch(trees, [f[2] for f in fams], None, Q, pi, [f[3] for f in fams])
    err = max(np.abs(a - b).max() for a, b in zip(site_ll, want))
    print(f"against tree_likelihood: max |d l_u| = {err:.2e}")
    assert err < 1e-10
    for k, w in enumerate(want):
        assert abs(fam_ll[k] - w.sum()) < 1e-10 * w.size


def test_simulated_lengths_are_recovered(tmp_path):
    """leaves simulated by simulate_msas on a 12-leaf tree whose lengths are grid points, 300 sites in 4 rate categories; the
    start is every index displaced by up to 15 steps"""
    from cherryml_amd import BranchLengthFitter, simulate_msas
    from cherryml_amd.counting._host import read_msa
    from cherryml_amd.evaluation._likelihood import _family_units
    from cherryml_amd.io import read_tree, write_contact_map, write_probability_distribution, write_rate_matrix, write_tree
    z = load_golden("likelihood.npz")
    Q, pi = z["lg"], z["pi_lg"]
    grid = np.array(bl_cases.GRID)
    rng = np.random.default_rng(2024)
    parent = bl_cases.random_tree(12, rng)
    true = rng.integers(40, 85, len(parent))
    true[parent < 0] = -1
    L = 300
    rates = rng.permutation(np.repeat([0.3, 0.8, 1.5, 3.0], L // 4))
    for d in ("tree", "rates", "cm", "model"):
        (tmp_path / d).mkdir()
    write_tree(_tree(parent, np.where(true >= 0, grid[true], 0.0)), str(tmp_path / "tree" / "f.txt"))
    (tmp_path / "rates" / "f.txt").write_text(f"{L} sites\n" + " ".join(repr(float(r)) for r in rates))
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
                  output_msa_dir=str(tmp_path / "msa"))
    tree = read_tree(str(tmp_path / "tree" / "f.txt"))
    codes = _family_units(tree, read_msa(str(tmp_path / "msa" / "f.txt")), None, L, AA, False)[2]
    start = np.where(true >= 0, np.clip(true + rng.integers(-15, 16, len(parent)), 0, grid.size - 1), -1)
    # the restatement first: its round from the start agrees with the handle's wherever its margin decides
    r = bl_reference.em_round(parent, start, codes, rates, grid, Q, pi)
    with BranchLengthFitter([tree], [codes], [rates], grid, Q, pi) as fit:
        ll_true = fit.log_likelihoods()[1][0]
        assert np.array_equal(fit.indices()[0], true)
    with BranchLengthFitter([_tree(parent, np.where(start >= 0, grid[start], 0.0))], [codes], [rates], grid, Q, pi) as fit:
        n_changed, fam_ll = fit.round()
        first = fit.indices()[0]
        sure = r["margin"] > MARGIN
        assert abs(fam_ll[0] - r["ll"].sum()) < 1e-9 * abs(fam_ll[0]) and np.array_equal(first[sure], r["tau"][sure])
        rounds = 1
        while n_changed.any() and rounds < 100:
            n_changed, _ = fit.round()
            rounds += 1
        final, ll_final = fit.indices()[0], fit.log_likelihoods()[1][0]
    e = true >= 0
    dist = lambda idx: float(np.abs(np.log(grid[idx[e]] / grid[true[e]])).sum())   # noqa: E731
    print(f"recovery: {rounds} rounds, log-likelihood start {fam_ll[0]:.4f}, true {ll_true:.4f}, final {ll_final:.4f}; "
          f"sum |log(t / t_true)| start {dist(start):.3f}, final {dist(final):.3f}")
    assert not n_changed.any()
    assert ll_final >= ll_true
    assert dist(final) < dist(start)


def _demo_msas(tmp_path, k):
    z = load_golden("demo_e2e.npz")
    fams = [str(f) for f in z["families"]]
    small = sorted(range(len(fams)), key=lambda i: (len(str(z["text_msa"][i])), fams[i]))[:k]
    (tmp_path / "msa").mkdir()
    for i in small:
        (tmp_path / "msa" / f"{fams[i]}.txt").write_text(str(z["text_msa"][i]))
    return z, [fams[i] for i in small]


def _total(path):
    return float(open(path).read().split("\n")[0])


def test_the_stage_its_files_and_its_cache(tmp_path, monkeypatch):
    from cherryml_amd import caching, ml_branch_lengths, nj_trees
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation import _ml_lengths
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    z, fams = _demo_msas(tmp_path, 2)
    msa_dir, qpath = str(tmp_path / "msa"), str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    grid = set(quantization_points_ble(0.03, 1.1, 64))
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        nj = nj_trees(msa_dir=msa_dir, families=fams, rate_matrix_path=qpath, num_rate_categories=4)
        args = dict(tree_dir=nj["output_tree_dir"], msa_dir=msa_dir, site_rates_dir=nj["output_site_rates_dir"], families=fams,
                    rate_matrix_path=qpath)
        out = ml_branch_lengths(**args)
        monkeypatch.setattr(_ml_lengths.BranchLengthFitter, "_create", lambda self: pytest.fail("the second call ran the fit"))
        assert ml_branch_lengths(**args) == out                                  # the cache
    finally:
        caching.set_cache_dir(None)
    for fam in fams:
        t_in = read_tree(os.path.join(nj["output_tree_dir"], fam + ".txt"))
        t_out = read_tree(os.path.join(out["output_tree_dir"], fam + ".txt"))
        assert t_out.nodes() == t_in.nodes()
        assert [(u, v) for u, v, _ in t_out.edges()] == [(u, v) for u, v, _ in t_in.edges()]
        assert all(t in grid for _, _, t in t_out.edges())
        lines = open(os.path.join(out["output_tree_dir"], fam + ".rounds")).read().split("\n")
        assert lines[-1] == "" and lines[-2].startswith("final ") and 2 <= len(lines) - 1 <= 11
        lls = [float(ln.split()[1]) for ln in lines[:-1]]
        assert [ln.split()[0] for ln in lines[:-2]] == [str(i) for i in range(len(lines) - 2)]
        assert all(b >= a - 1e-10 * abs(a) for a, b in zip(lls, lls[1:])), lls
        n_sites = int(open(os.path.join(out["output_likelihood_dir"], fam + ".txt")).read().split("\n")[1].split()[0])
        ll_file = _total(os.path.join(out["output_likelihood_dir"], fam + ".txt"))
        ll_nj = _total(os.path.join(nj["output_likelihood_dir"], fam + ".txt"))
        print(f"{fam}: log-likelihood nj_trees {ll_nj:.4f}, rounds {lls}, likelihood file {ll_file:.4f}")
        # the file is the held-out likelihood of the written tree, the last line the handle's: the identity of
        # test_the_fitted_likelihood_equals_the_held_out_likelihood, 1e-10 per site
        assert abs(ll_file - lls[-1]) < 1e-10 * n_sites
        assert ll_file > ll_nj, (fam, ll_file, ll_nj)
        prof = open(os.path.join(out["output_tree_dir"], fam + ".profiling")).read()
        assert prof.split("\n")[-1].startswith("total_time: ") and "mstep_kernel_ms: " in prof


def test_the_em_pipeline_takes_nj_ml_trees_as_its_tree_estimator(tmp_path):
    import cherryml_amd
    from cherryml_amd import caching, nj_ml_trees
    from cherryml_amd.io import read_rate_matrix, write_rate_matrix
    z, fams = _demo_msas(tmp_path, 1)
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    cache = tmp_path / "cache"
    caching.set_cache_dir(str(cache))
    try:
        res = cherryml_amd.lg_end_to_end_with_em_optimizer(
            msa_dir=str(tmp_path / "msa"), families=fams, tree_estimator=partial(nj_ml_trees, num_rate_categories=4, num_rounds=3),
            initial_tree_estimator_rate_matrix_path=qpath, num_iterations=1, em_iterations=2, optimizer_initialization=qpath)
    finally:
        caching.set_cache_dir(None)
    Q = read_rate_matrix(res["learned_rate_matrix_path"]).to_numpy()
    assert Q.shape == (20, 20) and np.all(np.isfinite(Q)) and np.allclose(Q.sum(1), 0.0, atol=1e-9)
    dirs = res["tree_estimator_output_dirs_0"]
    assert str(cache / "ml_branch_lengths") in dirs["output_tree_dir"] and str(cache / "nj_trees") in dirs["output_site_rates_dir"]
    lines = open(os.path.join(dirs["output_tree_dir"], fams[0] + ".rounds")).read().split("\n")
    assert len(lines) - 2 <= 3 and lines[-2].startswith("final ")
    assert len(os.listdir(cache / "nj_trees")) == 1 and len(os.listdir(cache / "ml_branch_lengths")) == 1
