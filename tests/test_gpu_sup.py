"""The branch supports on the GPU (csrc/sup.hip.h, cb_bl_supports, BranchLengthFitter.branch_supports / ml_branch_supports /
the support output of nj_nni_trees): every resampled delta, aLRT and count of every case against the NumPy restatement, before
any round and after one; determinism, batching, chunks and the number of replicates bit for bit; a call leaves the handle as it
was; the refusals; the simulated family's false edges against its true ones; the stage on demo families and its cache; the
search's files with and without supports."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bl_cases  # noqa: E402
import nni_cases  # noqa: E402
import nni_reference  # noqa: E402
import sup_reference  # noqa: E402
from conftest import load_golden  # noqa: E402

AA = list("ARNDCQEGHILKMFPSTWYV")
R = sup_reference.REPLICATES
DECIDED = ("s20", "s32", "s20one")     # tests/test_sup_cpu.py: every decision's margin is above 1e-9 |sum l|
VALUE_BAR = 1e-10                      # of max(1, |fam_ll|), on the resampled deltas: DESIGN.md section 18's bar on delta
MARGIN = 1e-9                          # of |fam_ll|: a decision with a margin up to this is undecided


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


def _seeds(n):
    return [sup_reference.family_seed(k) for k in range(n)]


def _compare(name, when, got, want, fam_ll, exact):
    """got: branch_supports(per_replicate=True) of the handle; want: per family the restatement's dict"""
    for k, ((nodes, alrt, sh, rell, rep), s) in enumerate(zip(got, want)):
        G = len(s["nodes"])
        assert nodes.dtype == np.int32 and np.array_equal(nodes, s["nodes"]), (name, k)
        assert alrt.shape == sh.shape == rell.shape == (G,) and rep.shape == (len(s["delta"]), R)
        if G == 0:
            continue
        bar = VALUE_BAR * max(1.0, abs(fam_ll[k]))
        err_rep, err_alrt = np.abs(rep - s["delta_rep"]).max(), np.abs(alrt - s["alrt"]).max()
        sh_count, rell_count = np.rint(sh * R).astype(np.int64), np.rint(rell * R).astype(np.int64)
        assert np.array_equal(sh_count / R, sh) and np.array_equal(rell_count / R, rell)
        bounds = sup_reference.bounds(s, MARGIN * abs(s["fam_ll"]))
        undecided = sum(b - a + d - c for a, b, c, d in bounds)
        print(f"{name}[{k}] {when}: {G} edges, {len(s['delta'])} moves, max |d delta_rep| = {err_rep:.2e}, max |d alrt| = "
              f"{err_alrt:.2e} (bar {bar:.2e}), undecided decisions {undecided}, sh in [{sh.min():.3f}, {sh.max():.3f}], "
              f"rell in [{rell.min():.3f}, {rell.max():.3f}]")
        assert err_rep <= bar, (name, k, when)
        assert err_alrt <= 2.0 * bar, (name, k, when)
        if exact:
            assert undecided == 0, (name, k, when)                 # no decision is left out
            assert np.array_equal(sh_count, s["sh_count"]) and np.array_equal(rell_count, s["rell_count"]), (name, k, when)
        for g, (a, b, c, d) in enumerate(bounds):
            assert a <= sh_count[g] <= b and c <= rell_count[g] <= d, (name, k, when, g)
        assert np.all(sh[alrt <= 0.0] == 0.0)


@pytest.mark.parametrize("name", nni_cases.CASES)
def test_supports_equal_the_restatement_before_any_round_and_after_one(name):
    """the cases of nni_cases.py (the 3-leaf star, which has no move, shares a handle with a family that has moves and gets
    empty arrays); after `round()` the call runs its own passes and is compared with the restatement AT the new indices"""
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    seeds = _seeds(len(fams))
    with _fitter(S, grid, fams) as fit:
        got0 = fit.branch_supports(R, seeds, per_replicate=True)
        assert all(x > 0.0 for x in fit.last_support_kernel_ms)
        fam0 = fit.log_likelihoods()[1]
        fit.round()
        got1 = fit.branch_supports(R, seeds, per_replicate=True)
        fam1 = fit.log_likelihoods()[1]
        tau1 = fit.indices()
    assert [len(g[0]) == 0 for g in got0] == [m == 0 for m in nni_cases.MOVE_COUNTS[name]]
    _compare(name, "at the start", got0, sup_reference.restated(name), fam0, name in DECIDED)
    want = []
    for k, ((parent, _, codes, rates), tau) in enumerate(zip(fams, tau1)):
        mvs = nni_reference.moves(parent)
        ll_moves, ll = nni_reference.scan(parent, tau, codes, rates, grid, Q, pi, mvs)
        want.append(sup_reference.supports(mvs, ll_moves, ll, R, seeds[k]))
    _compare(name, "after one round", got1, want, fam1, name in DECIDED)


def test_a_family_longer_than_one_histogram_window_equals_the_restatement():
    """16 384 + 37 sites in two shuffled rate categories on the 4-leaf ladder, beside a short family: sup_weights_kernel builds
    the long family's multiplicities in two windows, and the draws that land in the second must not be lost or counted twice"""
    L = 16384 + 37
    long_fam = bl_cases.family(nni_cases.LADDER4, 4, [9000, L - 9000], [0.5, 2.0], bl_cases.GRID, 23)
    fams = [nni_cases.case("s4small")[2][0], long_fam]
    Q, pi = bl_cases.model(4)
    seeds, n_rep = [5, 6], 24
    with _fitter(4, bl_cases.GRID, fams) as fit:
        got = fit.branch_supports(n_rep, seeds, per_replicate=True)
        fam_ll = fit.log_likelihoods()[1]
        tau = fit.indices()
    for k, (parent, _, codes, rates) in enumerate(fams):
        mvs = nni_reference.moves(parent)
        ll_moves, ll = nni_reference.scan(parent, tau[k], codes, rates, bl_cases.GRID, Q, pi, mvs)
        s = sup_reference.supports(mvs, ll_moves, ll, n_rep, seeds[k])
        err = np.abs(got[k][4] - s["delta_rep"]).max()
        print(f"family {k}: {len(ll)} sites, max |d delta_rep| = {err:.2e}, |fam_ll| = {abs(fam_ll[k]):.1f}")
        assert np.array_equal(got[k][0], s["nodes"])
        assert err <= VALUE_BAR * max(1.0, abs(fam_ll[k])) and np.abs(got[k][1] - s["alrt"]).max() <= 2 * VALUE_BAR * abs(fam_ll[k])
        lo_hi = sup_reference.bounds(s, MARGIN * abs(s["fam_ll"]))
        for g, (a, b, c, d) in enumerate(lo_hi):
            assert a <= round(got[k][2][g] * n_rep) <= b and c <= round(got[k][3][g] * n_rep) <= d


def _flat(x):
    if isinstance(x, (tuple, list)):
        return [z for y in x for z in _flat(y)]
    return [np.asarray(x)]


def _same(a, b):
    a, b = _flat(a), _flat(b)
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_two_calls_another_handle_a_family_alone_chunks_and_fewer_replicates_agree_bitwise(monkeypatch):
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]
    seeds = [11, (1 << 63) + 7, 1001]

    def run(which, n_rep=R):
        with _fitter(20, bl_cases.GRID, [fams[k] for k in which]) as fit:
            fit.round()
            return fit.branch_supports(n_rep, [seeds[k] for k in which], per_replicate=True)

    with _fitter(20, bl_cases.GRID, fams) as fit:
        fit.round()
        first = fit.branch_supports(R, seeds, per_replicate=True)
        assert _same(first, fit.branch_supports(R, seeds, per_replicate=True))                 # the same handle again
        assert _same([x[:4] for x in first], fit.branch_supports(R, seeds))                    # without the per-replicate output
        # one group per chunk, and chunks of a few groups, through the test hook: the same bits
        for bound in ("1", str(3 * 2 * (74 + R) * 8)):
            monkeypatch.setenv("CB_SUP_BYTES", bound)
            assert _same(first, fit.branch_supports(R, seeds, per_replicate=True)), bound
        monkeypatch.delenv("CB_SUP_BYTES")
        # a subset of the edges: every other group of the second family, none of the first
        moves = fit.nni_moves()
        keep = np.isin(moves[1][:, 0], first[1][0][::2])
        sub = fit.branch_supports(R, seeds, per_replicate=True, moves=[moves[0][:0], moves[1][keep], moves[2]])
        assert len(sub[0][0]) == 0 and _same(sub[2], first[2])
        assert _same(sub[1], (first[1][0][::2], first[1][1][::2], first[1][2][::2], first[1][3][::2], first[1][4][keep]))
        few = fit.branch_supports(64, seeds, per_replicate=True)                               # replicate r does not depend on R
        for a, b in zip(few, first):
            assert np.array_equal(a[4], b[4][:, :64]) and np.array_equal(a[1], b[1])
    assert _same(first, run([0, 1, 2]))                                                        # another handle
    for k in range(3):                                                                         # a family alone
        assert _same(run([k])[0], first[k]), k
    # another seed gives other resamples, the same aLRT
    with _fitter(20, bl_cases.GRID, fams[:1]) as fit:
        fit.round()
        other = fit.branch_supports(R, [12], per_replicate=True)[0]
    assert np.array_equal(other[1], first[0][1]) and not np.array_equal(other[4], first[0][4])


def test_supports_leave_the_handle_as_it_was():
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]

    def run(sup):
        out = []
        with _fitter(20, bl_cases.GRID, fams) as fit:
            if sup:
                fit.branch_supports(64)
            out.append(fit.round())
            if sup:
                fit.branch_supports(64, per_replicate=True)
            out.append((fit.indices(), fit.log_likelihoods()))
            out.append(fit.nni_scan(per_site=True))
            if sup:
                fit.branch_supports(16, moves=[m[:2] for m in fit.nni_moves()])
            out.append(fit.ancestral_states(posteriors=True))
            out.append(fit.round())
            if sup:
                fit.branch_supports(64)
            out.append((fit.round(), fit.indices(), fit.log_likelihoods(), fit.nni_scan(), fit.ancestral_states()))
        return out

    assert _same(run(False), run(True))


def test_the_refusals_name_the_value_and_the_handle_still_works():
    from cherryml_amd import _lib
    S, grid, fams = nni_cases.case("s4small")       # family 1: the ladder [-1, 0, 0, 1, 1, 3, 3]
    with _fitter(S, grid, fams) as fit:
        moves = fit.nni_moves()
        first = fit.branch_supports(R, [1, 2], per_replicate=True)
        ladder = moves[1]                                                       # v = 1 twice, then v = 3 twice
        assert ladder[:, 0].tolist() == [1, 1, 3, 3]
        for bad_moves, n_rep, match in [
                ([moves[0], ladder[[0, 2, 1, 3]]], R, "family 1 move 2: v = 1 comes back"),
                ([moves[0], ladder], 0, "n_rep = 0 "),
                ([moves[0], ladder], 65537, "n_rep = 65537 "),
                ([moves[0], np.array([ladder[0], (3, 5, 2)])], R, "family 1 move 1: s = 2 is not a child of parent[v] = 1"),
                ([moves[0], np.array([ladder[0], (7, 5, 4)])], R, "family 1 move 1: v = 7 (0 <= index < 7)"),
                ([moves[0], np.array([ladder[0], (0, 1, 2)])], R, "family 1 move 1: v = 0 is the root")]:
            with pytest.raises(_lib.CherryBankError) as e:
                fit.branch_supports(n_rep, [1, 2], moves=bad_moves)
            assert "cb_bl_supports" in str(e.value) and match in str(e.value), (match, str(e.value))
        assert _same(first, fit.branch_supports(R, [1, 2], per_replicate=True))  # bitwise, after six refusals
        n_changed, _ = fit.round()
        assert n_changed.any()


def test_on_the_simulated_family_every_false_edge_has_less_support_than_every_true_edge():
    """nni_cases.search_family on its start tree at its true indices, seed 1: every decision is decided (test_sup_cpu.py), so
    the counts are the restatement's, and the three edges the start tree has wrong stay below every true edge"""
    f = nni_cases.search_family()
    mvs, s, true = sup_reference.restated_search_family()
    grid = np.array(bl_cases.GRID)
    fam = (f["start_parent"], np.where(f["tau"] >= 0, grid[f["tau"]], 0.0), f["codes"], f["rates"])
    with _fitter(20, bl_cases.GRID, [fam]) as fit:
        got = fit.branch_supports(R, [1], per_replicate=True)
        fam_ll = fit.log_likelihoods()[1]
        assert np.array_equal(fit.indices()[0], f["tau"])
    _compare("search family", "start tree, true indices", got, [s], fam_ll, True)
    nodes, _, sh, _, _ = got[0]
    false_edges = [sh[g] for g, v in enumerate(nodes.tolist()) if not true[v]]
    true_edges = [sh[g] for g, v in enumerate(nodes.tolist()) if true[v]]
    print("false edges", false_edges, "true edges", true_edges)
    assert len(false_edges) >= 3 and max(false_edges) < min(true_edges)


# ---------------------------------------------------------------------------------------------------------- the stages
def _demo_msas(tmp_path, k):
    z = load_golden("demo_e2e.npz")
    fams = [str(f) for f in z["families"]]
    small = sorted(range(len(fams)), key=lambda i: (len(str(z["text_msa"][i])), fams[i]))[:k]
    (tmp_path / "msa").mkdir()
    for i in small:
        (tmp_path / "msa" / f"{fams[i]}.txt").write_text(str(z["text_msa"][i]))
    return z, [fams[i] for i in small]


def _handle_supports(tree_dir, msa_dir, rates_dir, fams, qpath, n_rep, random_seed):
    """branch_supports on a handle built here from the stage's inputs"""
    from cherryml_amd import BranchLengthFitter
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation._likelihood import _family_units, _stationary_distribution
    from cherryml_amd.io import read_rate_matrix, read_tree
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    from cherryml_amd.simulation._simulate import family_seed
    rm = read_rate_matrix(qpath)
    Q = np.ascontiguousarray(rm.to_numpy(), dtype=np.float64)
    trees, codes, rates = [], [], []
    for fam in fams:
        tree = read_tree(os.path.join(tree_dir, fam + ".txt"))
        r = np.asarray(read_site_rates(os.path.join(rates_dir, fam + ".txt")), dtype=np.float64)
        trees.append(tree), rates.append(r)
        codes.append(_family_units(tree, read_msa(os.path.join(msa_dir, fam + ".txt")), None, len(r), [str(c) for c in rm.columns],
                                   False)[2])
    with BranchLengthFitter(trees, codes, rates, np.array(quantization_points_ble(0.03, 1.1, 64)), Q, _stationary_distribution(Q)) as fit:
        return trees, fit.branch_supports(n_rep, [family_seed(f, random_seed) for f in fams])


def _check_files(support_dir, fams, trees, want):
    from cherryml_amd.phylogeny_estimation import read_supports
    for fam, tree, (nodes, alrt, sh, rell) in zip(fams, trees, want):
        lines = open(os.path.join(support_dir, fam + ".txt")).read().split("\n")
        names = list(tree.nodes())
        internal = [v for v in names if not tree.is_leaf(v) and v != tree.root()]
        assert lines[0] == "node alrt sh rell" and lines[-1] == "" and [ln.split()[0] for ln in lines[1:-1]] == internal
        assert [names[v] for v in nodes] == internal and len(internal) >= 1
        got = read_supports(os.path.join(support_dir, fam + ".txt"))
        for v, a, s, r in zip(internal, alrt, sh, rell):
            assert got[v] == (a, s, r), (fam, v)                                 # the values of the handle, bit for bit
            assert 0.0 <= s <= 1.0 and 0.0 <= r <= 1.0 and (a > 0.0 or s == 0.0)


def test_the_stage_on_demo_families_its_files_and_its_cache(tmp_path, monkeypatch):
    from cherryml_amd import caching, ml_branch_supports, nj_ml_trees
    from cherryml_amd.io import write_rate_matrix
    from cherryml_amd.phylogeny_estimation import _ml_lengths
    z, fams = _demo_msas(tmp_path, 2)
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        ml = nj_ml_trees(msa_dir=str(tmp_path / "msa"), families=fams, rate_matrix_path=qpath, num_rate_categories=4, num_rounds=3)
        args = dict(tree_dir=ml["output_tree_dir"], msa_dir=str(tmp_path / "msa"), site_rates_dir=ml["output_site_rates_dir"],
                    families=fams, rate_matrix_path=qpath, num_replicates=200, random_seed=5)
        out = ml_branch_supports(**args)
        trees, want = _handle_supports(ml["output_tree_dir"], str(tmp_path / "msa"), ml["output_site_rates_dir"], fams, qpath, 200, 5)
        monkeypatch.setattr(_ml_lengths.BranchLengthFitter, "_create", lambda self: pytest.fail("the second call ran the stage"))
        assert ml_branch_supports(**args) == out                                 # the cache
    finally:
        caching.set_cache_dir(None)
    sdir = out["output_support_dir"]
    assert str(tmp_path / "cache" / "ml_branch_supports") in sdir
    _check_files(sdir, fams, trees, want)
    for fam in fams:
        prof = open(os.path.join(sdir, fam + ".profiling")).read()
        assert prof.split("\n")[-1].startswith("total_time: ") and "resampling_kernel_ms: " in prof


def test_nj_nni_trees_writes_the_same_files_with_and_without_supports(tmp_path):
    from cherryml_amd import caching, nj_nni_trees
    from cherryml_amd.io import write_rate_matrix
    z, fams = _demo_msas(tmp_path, 2)
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    args = dict(msa_dir=str(tmp_path / "msa"), families=fams, rate_matrix_path=qpath, num_rate_categories=4, num_rounds=3,
                num_nni_rounds=2)
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        plain = nj_nni_trees(**args)
        sup = nj_nni_trees(output_support_dir=str(tmp_path / "sup"), num_support_replicates=100, **args)
    finally:
        caching.set_cache_dir(None)
    assert plain["output_tree_dir"] != sup["output_tree_dir"] and set(plain) == set(sup)      # both ran
    for fam in fams:
        for key, ext in (("output_tree_dir", ".txt"), ("output_tree_dir", ".nni"), ("output_likelihood_dir", ".txt")):
            a, b = (open(os.path.join(d[key], fam + ext), "rb").read() for d in (plain, sup))
            assert a == b and len(a) > 0, (fam, key, ext)
    assert not os.path.exists(os.path.join(os.path.dirname(plain["output_tree_dir"]), "output_support_dir"))
    # the supports are the final trees': a handle built from the written trees gives the same values
    trees, want = _handle_supports(sup["output_tree_dir"], str(tmp_path / "msa"), sup["output_site_rates_dir"], fams, qpath, 100, 0)
    _check_files(str(tmp_path / "sup"), fams, trees, want)
