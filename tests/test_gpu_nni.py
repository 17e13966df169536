"""The NNI scan and search on the GPU (csrc/nni.hip.h, cb_bl_nni_scan, BranchLengthFitter.nni_scan / ml_nni_trees /
nj_nni_trees): every move of every case against the NumPy restatement, before any round and after one; the rearranged trees
through the held-out likelihood; determinism, batching, subsets and chunks bit for bit; a scan leaves the handle as it was; the
refusals; the search on a simulated family against the restated search; the stages on demo families and in the EM pipeline."""
import os
import sys
from functools import partial

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bl_cases  # noqa: E402
import nni_cases  # noqa: E402
import nni_reference  # noqa: E402
from conftest import load_golden  # noqa: E402

AA = list("ARNDCQEGHILKMFPSTWYV")


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


def _compare(name, when, fams, got, want, fam_ll):
    """got = (moves, delta, ll_moves) of the handle, want = per family (moves, ll_moves, ll) of the restatement"""
    moves, delta, ll_moves = got
    for k, (mvs, ll_ref, ll) in enumerate(want):
        assert moves[k].dtype == np.int32 and np.array_equal(moves[k], mvs), (name, k)
        assert ll_moves[k].shape == ll_ref.shape == (len(mvs), len(fams[k][3])) and delta[k].shape == (len(mvs),)
        if len(mvs) == 0:
            continue
        assert np.all(np.isfinite(ll_ref)) and np.all(np.isfinite(ll_moves[k]))
        err = np.abs(ll_moves[k] - ll_ref) / np.maximum(1.0, np.abs(ll_ref))
        want_delta = (ll_ref - ll[None, :]).sum(axis=1)
        derr = np.abs(delta[k] - want_delta).max() / abs(fam_ll[k])
        print(f"{name}[{k}] {when}: {len(mvs)} moves, max |d ll'| / max(1, |ll'|) = {err.max():.2e}, "
              f"max |d delta| / |fam_ll| = {derr:.2e}, delta in [{delta[k].min():.3f}, {delta[k].max():.3f}]")
        assert err.max() < 1e-10, (name, k, when)
        assert derr < 1e-10, (name, k, when)


@pytest.mark.parametrize("name", nni_cases.CASES)
def test_every_move_equals_the_restatement_before_any_round_and_after_one(name):
    """the cases of nni_cases.py; after `round()` the resident messages belong to the round's start and qb holds the new
    indices: the scan runs its own passes, and is compared with the restatement AT the new indices"""
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    with _fitter(S, grid, fams) as fit:
        assert [len(m) for m in fit.nni_moves()] == nni_cases.MOVE_COUNTS[name]
        got0 = fit.nni_scan(per_site=True)
        fam0 = fit.log_likelihoods()[1]
        tau0 = fit.indices()
        fit.round()
        got1 = fit.nni_scan(per_site=True)
        fam1 = fit.log_likelihoods()[1]
        tau1 = fit.indices()
        assert fit.last_nni_kernel_ms[0] > 0.0 and fit.last_nni_kernel_ms[1] > 0.0
    rest = nni_cases.restated(name)
    assert all(np.array_equal(a, r[0]) for a, r in zip(tau0, rest))
    _compare(name, "at the start", fams, got0, [r[1:] for r in rest], fam0)
    assert any(not np.array_equal(a, b) for a, b in zip(tau0, tau1))          # the round moved
    want = []
    for (parent, _, codes, rates), tau in zip(fams, tau1):
        mvs = nni_reference.moves(parent)
        want.append((mvs,) + nni_reference.scan(parent, tau, codes, rates, grid, Q, pi, mvs))
    _compare(name, "after one round", fams, got1, want, fam1)


def test_the_rearranged_trees_have_these_likelihoods_under_tree_likelihood_batch():
    """all moves of the 17-leaf family with one category: the rearranged trees with lengths grid[tau], one batch"""
    from cherryml_amd.evaluation import tree_likelihood_batch
    S, grid, fams = nni_cases.case("s20one")
    Q, pi = bl_cases.model(S)
    parent, _, codes, rates = fams[0]
    with _fitter(S, grid, fams) as fit:
        fit.round()
        moves, _, ll_moves = fit.nni_scan(per_site=True)
        tau = fit.indices()[0]
    length = np.where(tau >= 0, np.asarray(grid)[tau], 0.0)
    trees = [_tree(nni_reference.apply(parent, [mv]), length) for mv in moves[0]]
    want = tree_likelihood_batch(trees, [codes] * len(trees), None, Q, pi, [rates] * len(trees))
    err = max(np.abs(a - b).max() for a, b in zip(ll_moves[0], want))
    print(f"against tree_likelihood_batch on {len(trees)} rearranged trees: max |d ll'| = {err:.2e}")
    assert len(trees) == 34 and err < 1e-10


def _scan(fams, moves=None, rounds=1):
    with _fitter(20, bl_cases.GRID, fams) as fit:
        for _ in range(rounds):
            fit.round()
        return fit.nni_scan(moves, per_site=True)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_two_scans_a_family_alone_a_subset_and_chunks_agree_bitwise(monkeypatch):
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]
    with _fitter(20, bl_cases.GRID, fams) as fit:
        fit.round()
        moves, delta, ll = fit.nni_scan(per_site=True)
        _, delta2, ll2 = fit.nni_scan(per_site=True)                          # the same handle again
        assert _same(delta, delta2) and _same(ll, ll2)
        assert _same(fit.nni_scan()[1], delta)                                # without the per-site output
        # a subset of the list (every third move, the families' lists of different length; one family with none)
        sub = [moves[0][::3], moves[1][:0], moves[2][1::3]]
        _, dsub, lsub = fit.nni_scan(sub, per_site=True)
        assert _same(dsub, [delta[0][::3], delta[1][:0], delta[2][1::3]]) and _same(lsub, [ll[0][::3], ll[1][:0], ll[2][1::3]])
        # the moves in chunks of one, and of three of the second family, through the test hook: the same bits
        for bound in ("1", str(3 * 74 * 8)):
            monkeypatch.setenv("CB_NNI_LL_BYTES", bound)
            _, d3, l3 = fit.nni_scan(per_site=True)
            assert _same(d3, delta) and _same(l3, ll), bound
        monkeypatch.delenv("CB_NNI_LL_BYTES")
    _, delta4, ll4 = _scan(fams)                                              # another handle
    assert _same(delta, delta4) and _same(ll, ll4)
    for k, f in enumerate(fams):                                              # a family alone
        _, d1, l1 = _scan([f])
        assert np.array_equal(d1[0], delta[k]) and np.array_equal(l1[0], ll[k]), k


def test_a_scan_leaves_the_handle_as_it_was():
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]

    def run(scan):
        out = []
        with _fitter(20, bl_cases.GRID, fams) as fit:
            if scan:
                fit.nni_scan()
            out.append(fit.round())
            if scan:
                fit.nni_scan(per_site=True)
            out.append((fit.indices(), fit.log_likelihoods()))
            if scan:
                fit.nni_scan([m[:1] for m in fit.nni_moves()])
            out.append(fit.round())
            out.append(fit.round())
            for _ in range(100):                                              # on to every family's fixed point
                n_changed, fam_ll = fit.round()
                if not n_changed.any():
                    break
            if scan:
                fit.nni_scan()
            out.append((fit.round(), fit.indices(), fit.log_likelihoods()))
        return out

    def flat(x):
        if isinstance(x, (tuple, list)):
            return [z for y in x for z in flat(y)]
        return [np.asarray(x)]

    a, b = flat(run(False)), flat(run(True))
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_fam_ll_of_the_c_entry_point_is_cb_bl_gets_and_a_skipped_family_has_none_after_a_round():
    from cherryml_amd import _lib
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]
    with _fitter(20, bl_cases.GRID, fams) as fit:
        fit.round()                                                           # every family's likelihood is the old indices' now
        moves = fit.nni_moves()
        some = [moves[0], moves[1][:0], moves[2][:2]]
        n_moves = np.array([len(m) for m in some], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(some).reshape(-1), dtype=np.int32)
        delta, fam, ms = np.zeros(int(n_moves.sum())), np.zeros(3), np.zeros(2)

        def call():
            rc = _lib.load().cb_bl_nni_scan(fit._handle(), n_moves.ctypes.data, flat.ctypes.data, delta.ctypes.data, None,
                                            fam.ctypes.data, ms.ctypes.data)
            assert rc == 0, _lib.load().cb_last_error()
        call()
        first = fam.copy()
        want = fit.log_likelihoods()[1]
        assert np.isnan(first[1]) and first[0] == want[0] and first[2] == want[2]   # bitwise; no pass ran for family 1
        call()
        assert np.array_equal(fam, want) and ms[0] > 0 and ms[1] > 0
        assert np.array_equal(delta, np.concatenate(fit.nni_scan(some)[1]))


def test_the_refusals_name_the_value_and_the_handle_still_works():
    from cherryml_amd import _lib
    S, grid, fams = nni_cases.case("s4small")       # family 1: the ladder [-1, 0, 0, 1, 1, 3, 3]
    with _fitter(S, grid, fams) as fit:
        moves, delta = fit.nni_scan()
        good = moves[0]
        for bad, match in [((7, 5, 4), "family 1 move 1: v = 7 (0 <= index < 7)"),
                           ((3, -1, 4), "family 1 move 1: c = -1 (0 <= index < 7)"),
                           ((3, 5, 9), "family 1 move 1: s = 9 (0 <= index < 7)"),
                           ((0, 1, 2), "family 1 move 1: v = 0 is the root"),
                           ((5, 6, 6), "family 1 move 1: v = 5 is a leaf"),
                           ((3, 4, 4), "family 1 move 1: c = 4 is not a child of v = 3"),
                           ((3, 5, 3), "family 1 move 1: s = 3 equals v"),
                           ((3, 5, 2), "family 1 move 1: s = 2 is not a child of parent[v] = 1")]:
            with pytest.raises(_lib.CherryBankError) as e:
                fit.nni_scan([good, np.array([moves[1][0], bad])])
            assert "cb_bl_nni_scan" in str(e.value) and match in str(e.value), (bad, str(e.value))
        n_moves = np.array([1, -2], dtype=np.int32)
        out = np.zeros(4)
        rc = _lib.load().cb_bl_nni_scan(fit._handle(), n_moves.ctypes.data, np.ascontiguousarray(good).ctypes.data,
                                        out.ctypes.data, None, None, None)
        assert rc == _lib.CB_EINVAL and "family 1: n_moves = -2" in _lib.load().cb_last_error().decode()
        again = fit.nni_scan()[1]
        assert all(np.array_equal(x, y) for x, y in zip(delta, again))        # bitwise, after nine refusals
        n_changed, _ = fit.round()
        assert n_changed.any()


# ---------------------------------------------------------------------------------------------------------- the search
def _nni_lines(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[-2].startswith("final ")
    rounds = [ln.split() for ln in lines[:-2]]
    assert [r[0] for r in rounds] == [str(i) for i in range(len(rounds))]
    lls = [x for r in rounds for x in (float(r[1]), float(r[5]))] + [float(lines[-2].split()[1])]
    assert all(b >= a for a, b in zip(lls, lls[1:])), lls                     # no number below the one before it
    return [(float(r[1]), int(r[2]), int(r[3]), int(r[4]), float(r[5])) for r in rounds], lls[-1]


def test_the_search_on_a_simulated_family_takes_the_restated_searchs_moves(tmp_path):
    """nni_cases.search_family: 12 leaves, 400 sites, the start three moves from the true tree; its seed is chosen so that every
    decision of the restated search has a margin above 1e-9 |log-likelihood| (tests/test_nni_cpu.py asserts it), so the stage must
    scan, select, apply and accept as the restatement does, round by round, and end on the same tree at the same lengths"""
    from cherryml_amd import ml_nni_trees
    from cherryml_amd.io import read_tree, write_rate_matrix, write_tree
    f, r = nni_cases.search_family(), nni_cases.restated_search()
    assert r["margin"] > 1e-9 and r["em_margin"] > 1e-9
    Q, _ = bl_cases.model(20)
    grid = np.array(bl_cases.GRID)
    parent = f["start_parent"]
    leaves = sorted(set(range(len(parent))) - set(parent.tolist()))
    for d in ("tree", "msa", "rates"):
        (tmp_path / d).mkdir()
    write_tree(_tree(parent, np.where(f["tau"] >= 0, grid[f["tau"]], 0.0)), str(tmp_path / "tree" / "f.txt"))
    (tmp_path / "msa" / "f.txt").write_text("".join(f">n{v}\n{''.join(AA[k] for k in f['codes'][v])}\n" for v in leaves))
    (tmp_path / "rates" / "f.txt").write_text(f"{len(f['rates'])} sites\n" + " ".join(repr(float(x)) for x in f["rates"]))
    write_rate_matrix(Q, AA, str(tmp_path / "q.txt"))
    ml_nni_trees(tree_dir=str(tmp_path / "tree"), msa_dir=str(tmp_path / "msa"), site_rates_dir=str(tmp_path / "rates"),
                 families=["f"], rate_matrix_path=str(tmp_path / "q.txt"), num_nni_rounds=nni_cases.SEARCH_NNI_ROUNDS,
                 num_rounds=nni_cases.SEARCH_EM_ROUNDS, quantization_grid_num_steps=64, output_tree_dir=str(tmp_path / "out"),
                 output_likelihood_dir=str(tmp_path / "ll"))
    rounds, final = _nni_lines(str(tmp_path / "out" / "f.nni"))
    print("stage:", rounds, final, "\nrestated:", [(x["before"], x["scanned"], len(x["selected"]), len(x["applied"]), x["after"])
                                                    for x in r["rounds"]], r["final"])
    assert len(rounds) == len(r["rounds"])
    for got, want in zip(rounds, r["rounds"]):
        assert got[1:4] == (want["scanned"], len(want["selected"]), len(want["applied"]))
        assert abs(got[0] - want["before"]) < 1e-9 * abs(want["before"]) and abs(got[4] - want["after"]) < 1e-9 * abs(want["after"])
    assert abs(final - r["final"]) < 1e-9 * abs(final)
    out = read_tree(str(tmp_path / "out" / "f.txt"))
    assert out.nodes() == [f"n{v}" for v in range(len(parent))]
    index = {v: i for i, v in enumerate(out.nodes())}
    got_parent, got_tau = np.full(len(parent), -1), np.full(len(parent), -1)
    for u, v, t in out.edges():
        got_parent[index[v]] = index[u]
        got_tau[index[v]] = int(np.argmin(np.abs(np.log(grid / t))))
        assert abs(t / grid[got_tau[index[v]]] - 1.0) < 1e-12                 # a grid point
    assert np.array_equal(got_parent, r["parent"])                            # the moves applied are the restatement's
    assert np.array_equal(got_tau, r["tau"])
    assert nni_reference.splits(got_parent) == nni_reference.splits(f["true_parent"])


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


def test_the_stage_on_demo_families_its_files_and_its_cache(tmp_path, monkeypatch):
    from cherryml_amd import caching, nj_ml_trees, nj_nni_trees
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation import _ml_lengths
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    z, fams = _demo_msas(tmp_path, 2)
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    grid = set(quantization_points_ble(0.03, 1.1, 64))
    args = dict(msa_dir=str(tmp_path / "msa"), families=fams, rate_matrix_path=qpath, num_rate_categories=4, num_rounds=3)
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        ml = nj_ml_trees(**args)
        out = nj_nni_trees(num_nni_rounds=2, **args)
        monkeypatch.setattr(_ml_lengths.BranchLengthFitter, "_create", lambda self: pytest.fail("the second call ran the search"))
        assert nj_nni_trees(num_nni_rounds=2, **args) == out                   # the cache
    finally:
        caching.set_cache_dir(None)
    assert str(tmp_path / "cache" / "ml_nni_trees") in out["output_tree_dir"]
    assert out["output_site_rates_dir"] == ml["output_site_rates_dir"]         # nj_trees ran once
    for fam in fams:
        t_in = read_tree(os.path.join(ml["output_tree_dir"], fam + ".txt"))
        t_out = read_tree(os.path.join(out["output_tree_dir"], fam + ".txt"))
        assert t_out.nodes() == t_in.nodes() and set(t_out.leaves()) == set(t_in.leaves())
        assert [v for _, v, _ in t_out.edges()] == [v for _, v, _ in t_in.edges()]
        assert all(t in grid for _, _, t in t_out.edges())
        rounds, final = _nni_lines(os.path.join(out["output_tree_dir"], fam + ".nni"))
        assert 1 <= len(rounds) <= 2 and all(r[1] > 0 and r[2] >= r[3] for r in rounds)
        ll_file = _total(os.path.join(out["output_likelihood_dir"], fam + ".txt"))
        ll_ml = _total(os.path.join(ml["output_likelihood_dir"], fam + ".txt"))
        print(f"{fam}: nj_ml_trees {ll_ml:.4f}, NNI rounds {rounds}, final {final:.4f}, likelihood file {ll_file:.4f}")
        assert abs(ll_file - final) < 1e-9 * abs(final)
        assert final >= ll_ml - 1e-9 * abs(ll_ml)                               # (the first round's EM is nj_ml_trees' fit)
        moved = [(u, v) for u, v, _ in t_out.edges()] != [(u, v) for u, v, _ in t_in.edges()]
        assert moved or sum(r[3] for r in rounds) == 0 or len(rounds) > 1       # a move applied shows in the tree
        assert not moved or sum(r[3] for r in rounds) > 0
        prof = open(os.path.join(out["output_tree_dir"], fam + ".profiling")).read()
        assert prof.split("\n")[-1].startswith("total_time: ") and "scan_kernel_ms: " in prof


def test_the_em_pipeline_takes_nj_nni_trees_as_its_tree_estimator(tmp_path):
    import cherryml_amd
    from cherryml_amd import caching, nj_nni_trees
    from cherryml_amd.io import read_rate_matrix, write_rate_matrix
    z, fams = _demo_msas(tmp_path, 1)
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    cache = tmp_path / "cache"
    caching.set_cache_dir(str(cache))
    try:
        res = cherryml_amd.lg_end_to_end_with_em_optimizer(
            msa_dir=str(tmp_path / "msa"), families=fams,
            tree_estimator=partial(nj_nni_trees, num_rate_categories=4, num_rounds=3, num_nni_rounds=1),
            initial_tree_estimator_rate_matrix_path=qpath, num_iterations=1, em_iterations=2, optimizer_initialization=qpath)
    finally:
        caching.set_cache_dir(None)
    Q = read_rate_matrix(res["learned_rate_matrix_path"]).to_numpy()
    assert Q.shape == (20, 20) and np.all(np.isfinite(Q)) and np.allclose(Q.sum(1), 0.0, atol=1e-9)
    dirs = res["tree_estimator_output_dirs_0"]
    assert str(cache / "ml_nni_trees") in dirs["output_tree_dir"] and str(cache / "nj_trees") in dirs["output_site_rates_dir"]
    rounds, _ = _nni_lines(os.path.join(dirs["output_tree_dir"], fams[0] + ".nni"))
    assert len(rounds) == 1
