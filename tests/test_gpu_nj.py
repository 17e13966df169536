"""Full trees on the GPU: `ble_pairwise_kernel` (all-pairs branch-length bisection) against a NumPy restatement of the
reference's bisection and against `ble_branch_lengths_kernel`, its identity with FastCherries' coordinate ascent, the stage
`nj_trees` with the pipelines that take it as their tree estimator, and the topology it recovers on simulated data.

Exactness.  Every check is on integers (grid indices).  The restatement (tests/nj_reference.py:pairwise_bisection) records per
pair the smallest |a - b| / max(|a|, |b|) met on the way; a pair is UNDECIDED when that is <= 1e-9 (the order of summation moves
the sums by ~1e-13 relative) and is left out of the comparison; a pair with no commonly observed site compares 0 > 0 at every
step, which is false whatever the order: decided, index T - 1.  With the fixed seeds below the smallest margin over all shapes,
found on the CPU with a bank by eigendecomposition, is 1.3e-07 (shape (37, 513)) and no pair is undecided.  Needs an MI355X."""
import os
import sys
from functools import partial

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nj_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

T = 129
GRID = np.array([0.03 * 1.1 ** i for i in range(-64, 65)])
RATES = np.array([0.25, 0.6, 1.2, 2.5])
UNDECIDED = 1e-9
SHAPES = [(37, 1), (37, 64), (37, 65), (37, 513), (24, 700), (2, 65), (3, 65), (130, 40)]


def lg():
    return np.ascontiguousarray(load_golden("data_lg.npz")["lg"], dtype=np.float64)


def family(n, L, gaps_only_last=True):
    """(seqs [n, L] int8, site_to_rate [L]): sequences evolved down a random tree from LG's stationary distribution at the four
    rates, 15 % gaps; sequence 1 is a copy of sequence 0 and the last sequence is all gaps (n = 2 has room for one of the two:
    `gaps_only_last` chooses)."""
    rng = np.random.default_rng(1000 * n + L)
    s2r = rng.integers(0, len(RATES), L).astype(np.int32)
    tree = ref.random_tree(n, rng, length=lambda rng: rng.uniform(0.02, 0.4))
    seqs = ref.evolve(tree, n, lg(), RATES[s2r], rng)
    seqs[rng.random(seqs.shape) < 0.15] = -1
    if n > 2 or not gaps_only_last:
        seqs[1] = seqs[0]
    if n > 2 or gaps_only_last:
        seqs[n - 1] = -1
    return seqs, s2r


def families(shape):
    n, L = shape
    return [family(n, L, True), family(n, L, False)] if n == 2 else [family(n, L)]


@pytest.fixture(scope="module")
def bank():
    from cherryml_amd.phylogeny_estimation import compute_log_transition_matrices
    return compute_log_transition_matrices(lg(), GRID, RATES)


def check_against_restatement(got, seqs, s2r, logP):
    n = seqs.shape[0]
    want, margin = ref.pairwise_bisection(seqs, logP, s2r)
    off = ~np.eye(n, dtype=bool)
    decided = (margin > UNDECIDED) & off
    print(f"n = {n}, L = {seqs.shape[1]}: smallest margin {margin[off].min():.2e}, undecided {int((~decided & off).sum()) // 2} of "
          f"{n * (n - 1) // 2} pairs, mismatches on decided pairs {int((got != want)[decided].sum()) // 2}")
    assert got.dtype == np.int32 and got.shape == (n, n)
    assert np.array_equal(got, got.T) and np.all(np.diag(got) == -1)
    assert (~decided & off).sum() <= 0.01 * off.sum()
    assert np.array_equal(got[decided], want[decided])
    return want, decided


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pairwise_kernel_equals_the_restatement(bank, shape):
    from cherryml_amd.phylogeny_estimation import pairwise_branch_lengths
    for seqs, s2r in families(shape):
        n = seqs.shape[0]
        prof = {}
        got = pairwise_branch_lengths(seqs, bank, s2r, profile=prof)
        assert prof["kernel_ms"] > 0.0
        want, decided = check_against_restatement(got, seqs, s2r, bank)
        if np.all(seqs[n - 1] == -1):                       # the all-gap sequence: no commonly observed site with anybody
            assert np.all(got[n - 1, :n - 1] == T - 1) and np.all(got[:n - 1, n - 1] == T - 1)
        if np.array_equal(seqs[0], seqs[1]):                # the copy: identical sequences are at the grid's first point
            assert decided[0, 1] and got[0, 1] == want[0, 1]
            assert got[0, 1] == (0 if np.any(seqs[0] >= 0) else T - 1)


# ------------------------------------------------------------------------------------------------ 2. the existing kernel
def test_pairwise_kernel_equals_the_cherry_kernel_on_the_materialised_pairs(bank):
    from cherryml_amd.phylogeny_estimation import branch_lengths, pairwise_branch_lengths
    seqs, s2r = family(37, 513)
    I, J = np.triu_indices(37, 1)
    got = pairwise_branch_lengths(seqs, bank, s2r)
    cherry = branch_lengths(seqs[I], seqs[J], bank, s2r)
    _, margin = ref.pairwise_bisection(seqs, bank, s2r)
    decided = margin[I, J] > UNDECIDED
    assert decided.mean() >= 0.99
    assert np.array_equal(got[I, J][decided], cherry[decided])
    assert np.array_equal(got[I, J], cherry)                # (the same sums in the same order: every pair in fact)


# ------------------------------------------------------------------------------------------------ 3. FastCherries
def demo_family(tmp_path=None):
    z = load_golden("demo_e2e.npz")
    k = [str(f) for f in z["families"]].index("1a92_1_A")
    text = str(z["text_msa"][k])
    if tmp_path is not None:
        (tmp_path / "msa").mkdir()
        (tmp_path / "msa" / "1a92_1_A.txt").write_text(text)
    lines = text.split("\n")
    names = [ln[1:] for ln in lines if ln.startswith(">")]
    seqs = [lines[i + 1] for i, ln in enumerate(lines) if ln.startswith(">")]
    return z, names, seqs


def test_pairwise_index_of_a_cherry_is_the_length_the_ascent_ended_on():
    from cherryml_amd.phylogeny_estimation import nj_distance_indices
    from cherryml_amd.phylogeny_estimation._fast_cherries import _encode_and_pair
    z, names, sequences = demo_family()
    assert (len(names), len(sequences[0])) == (180, 50)
    seqs, pairs = _encode_and_pair(sequences, list("ARNDCQEGHILKMFPSTWYV"), 1234, "lemire")
    for R in (4, 20):
        index, cherry_index, rate_index, grid, rates = nj_distance_indices(seqs, pairs, z["lg_Q_best_f64"], num_rate_categories=R)
        assert len(pairs) == 90 and len(grid) == 129 and len(rates) == R and rate_index.shape == (50,)
        a, b = np.array(pairs).T
        assert np.array_equal(index[a, b], cherry_index) and np.array_equal(index[b, a], cherry_index)


# ------------------------------------------------------------------------------------------------ 4. stage and pipelines
def valid_rate_matrix(path):
    from cherryml_amd.io import read_rate_matrix
    Q = read_rate_matrix(path).to_numpy()
    assert Q.shape == (20, 20) and np.all(np.isfinite(Q)) and np.allclose(Q.sum(1), 0.0, atol=1e-9)
    assert np.all(Q - np.diag(np.diag(Q)) >= 0.0) and np.all(np.diag(Q) < 0.0)


def test_nj_trees_stage_and_the_pipelines_that_take_it(tmp_path):
    import cherryml_amd
    from cherryml_amd import caching, nj_trees
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation._likelihood import dp_likelihood_computation
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    z, names, _ = demo_family(tmp_path)
    AA = list("ARNDCQEGHILKMFPSTWYV")
    fam, msa_dir = "1a92_1_A", str(tmp_path / "msa")
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    out = {k: str(tmp_path / k) for k in ("output_tree_dir", "output_site_rates_dir", "output_likelihood_dir")}
    nj_trees(msa_dir=msa_dir, families=[fam], rate_matrix_path=qpath, num_rate_categories=4, **out)
    # the tree: every sequence once as a leaf, 2n - 3 edges, none shorter than the grid's first point
    tree = read_tree(os.path.join(out["output_tree_dir"], fam + ".txt"))
    n = len(names)
    grid0 = quantization_points_ble(0.03, 1.1, 64)[0]
    assert sorted(tree.leaves()) == sorted(names) and len(set(names)) == n == 180
    assert tree.num_edges() == 2 * n - 3 and all(t >= grid0 for _, _, t in tree.edges())
    rates = read_site_rates(os.path.join(out["output_site_rates_dir"], fam + ".txt"))
    assert len(rates) == 50 and abs(np.mean(rates) - 1.0) <= 1e-12
    # the likelihood file: a fresh evaluation of the files it wrote
    lines = open(os.path.join(out["output_likelihood_dir"], fam + ".txt")).read().split("\n")
    total, per_site = float(lines[0]), np.array([float(x) for x in lines[2].split()])
    assert lines[1] == "50 sites" and per_site.shape == (50,)
    Q = z["lg_Q_best_f64"]
    ll, lls = dp_likelihood_computation(tree, read_msa(os.path.join(msa_dir, fam + ".txt")), None, rates, AA, ref.stationary(Q), Q)
    assert np.all(np.isfinite(per_site)) and np.allclose(per_site, lls, rtol=1e-12, atol=0.0)
    assert abs(per_site.sum() - total) <= 1e-12 * abs(total) and abs(ll - total) <= 1e-12 * abs(total)
    prof = open(os.path.join(out["output_tree_dir"], fam + ".profiling")).read()
    assert [ln.split(":")[0] for ln in prof.split("\n")] == ["pairing_time", "ble_time", "distance_time", "nj_time", "likelihood_time",
                                                            "total_time"]
    # the pipelines, two iterations each: the second estimates its trees under the matrix the first one learned.  (The EM
    # pipeline initialises from the cherries of its tree alone; the few cherries of ONE 50-site family's full tree leave some
    # amino acids uncounted, and the JTT-IPW matrix of such counts has a degenerate stationary distribution, which the M-step
    # refuses as a start: EM starts from the given matrix instead.)
    estimator = partial(nj_trees, num_rate_categories=4, max_iters=50)
    for name, run in (("cherry", partial(cherryml_amd.lg_end_to_end_with_cherryml_optimizer, edge_or_cherry="cherry++", num_epochs=30)),
                      ("em", partial(cherryml_amd.lg_end_to_end_with_em_optimizer, em_iterations=3, optimizer_initialization=qpath))):
        cache = tmp_path / f"cache_{name}"
        caching.set_cache_dir(str(cache))
        try:
            res = run(msa_dir=msa_dir, families=[fam], tree_estimator=estimator, initial_tree_estimator_rate_matrix_path=qpath,
                      num_iterations=2)
        finally:
            caching.set_cache_dir(None)
        valid_rate_matrix(res["learned_rate_matrix_path"])
        valid_rate_matrix(os.path.join(res["rate_matrix_dir_0"], "result.txt"))
        hashes = os.listdir(cache / "nj_trees")
        assert len(hashes) == 2                              # one tree estimation per iteration
        for h in hashes:
            d = cache / "nj_trees" / h / "output_tree_dir"
            assert (d / f"{fam}.txt").exists() and (d / "result.success").exists()
        assert res["tree_estimator_output_dirs_0"]["output_tree_dir"] != res["tree_estimator_output_dirs_1"]["output_tree_dir"]


# ------------------------------------------------------------------------------------------------ 5. topology
def test_simulated_data_gives_the_true_splits_back():
    from cherryml_amd.phylogeny_estimation import neighbor_joining, pairwise_branch_lengths
    n, L = 12, 2000
    rng = np.random.default_rng(12)
    on_grid = GRID[GRID >= 0.1][:12]                        # 0.1 .. 0.29
    truth = ref.random_tree(n, rng, length=lambda rng: float(on_grid[rng.integers(len(on_grid))]))
    seqs = ref.evolve(truth, n, lg(), np.ones(L), rng)
    logP = ref.log_bank(lg(), GRID, [1.0])                  # R = 1, rate 1
    s2r = np.zeros(L, dtype=np.int32)
    got = pairwise_branch_lengths(seqs, logP, s2r)
    want, decided = check_against_restatement(got, seqs, s2r, logP)
    assert np.all(decided | np.eye(n, dtype=bool))
    names = [f"t{i}" for i in range(n)]
    trees = []
    for index in (want, got):
        D = GRID[np.maximum(index, 0)]
        np.fill_diagonal(D, 0.0)
        trees.append(ref.splits(ref.adjacency(neighbor_joining(D, names, min_length=GRID[0])), names))
    true_splits = {frozenset(names[x] for x in s) for s in ref.splits(truth, list(range(n)))}
    assert len(true_splits) == n - 3
    assert trees[0] == true_splits                          # (verified on the CPU for this seed)
    assert trees[1] == true_splits
