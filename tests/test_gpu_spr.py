"""The SPR scan and search on the GPU (csrc/spr.hip.h, cb_bl_spr_scan, BranchLengthFitter.spr_scan / ml_spr_trees /
nj_spr_trees): every radius-3 move of every case against the NumPy restatement, before any round and after one, and every move
up to the cap of the caterpillars; rearranged trees through the held-out likelihood; determinism, batching, subsets and chunks
bit for bit; a scan leaves the handle as it was; the refusals; the search on a simulated family against the restated search; the
stages on demo families and in the EM pipeline."""
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
import spr_reference  # noqa: E402
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
    """got = (moves, delta, ll_moves) of the handle, want = per family (moves, ll_moves, ll) of the restatement
    -> the worst |d ll'| / max(1, |ll'|) met"""
    moves, delta, ll_moves = got
    worst = 0.0
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
        worst = max(worst, float(err.max()))
    return worst


@pytest.mark.parametrize("name", nni_cases.CASES)
def test_every_radius_3_move_equals_the_restatement_before_any_round_and_after_one(name):
    """the cases of nni_cases.py; after `round()` the resident messages belong to the round's start: the scan runs its own
    passes, and is compared with the restatement AT the new indices (the moves' three indices follow them)"""
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    with _fitter(S, grid, fams) as fit:
        assert [len(m) for m in fit.spr_moves()] == spr_reference.MOVE_COUNTS[name][2]
        assert [len(m) for m in fit.spr_moves(1)] == spr_reference.MOVE_COUNTS[name][0]
        got0 = fit.spr_scan(per_site=True)
        fam0 = fit.log_likelihoods()[1]
        tau0 = fit.indices()
        fit.round()
        got1 = fit.spr_scan(per_site=True)
        fam1 = fit.log_likelihoods()[1]
        tau1 = fit.indices()
        assert fit.last_spr_kernel_ms[0] > 0.0 and fit.last_spr_kernel_ms[1] > 0.0
    rest = spr_reference.restated(name)
    assert all(np.array_equal(a, r[0]) for a, r in zip(tau0, rest))
    worst = _compare(name, "at the start", fams, got0, [r[1:] for r in rest], fam0)
    assert any(not np.array_equal(a, b) for a, b in zip(tau0, tau1))          # the round moved
    want = []
    for (parent, _, codes, rates), tau in zip(fams, tau1):
        mvs = spr_reference.full_moves(parent, tau, grid, 3)
        want.append((mvs,) + spr_reference.scan(parent, tau, codes, rates, grid, Q, pi, mvs))
    worst = max(worst, _compare(name, "after one round", fams, got1, want, fam1))
    print(f"{name}: the worst |d ll'| / max(1, |ll'|) met = {worst:.2e}")


def test_every_move_up_to_the_cap_of_the_caterpillars_at_any_three_indices():
    """the 9-leaf caterpillar of s20 (distances 1 to 7) and the 11-leaf one of spr_reference.deep_family (1 to 8, the cap), each
    move at three indices that are not spr_indices'"""
    for S, grid, fam in ((20, bl_cases.GRID, nni_cases.case("s20")[2][0]), (4, bl_cases.GRID, spr_reference.deep_family())):
        Q, pi = bl_cases.model(S)
        parent, _, codes, rates = fam
        with _fitter(S, grid, [fam]) as fit:
            tau = fit.indices()[0]
            mvs = spr_reference.full_moves(parent, tau, grid, spr_reference.MAX_RADIUS)
            mvs[:, 2:] = (mvs[:, 2:] + np.arange(len(mvs))[:, None] * np.array([3, 5, 7])) % len(grid)
            got = fit.spr_scan([mvs], per_site=True)
            fam_ll = fit.log_likelihoods()[1]
        dist = [spr_reference.distance(parent, int(x), int(y)) for x, y in mvs[:, :2]]
        assert max(dist) == (7 if S == 20 else 8)
        _compare(f"caterpillar S = {S}", "every distance", [fam], got,
                 [(mvs,) + spr_reference.scan(parent, tau, codes, rates, grid, Q, pi, mvs)], fam_ll)


def test_the_rearranged_trees_have_these_likelihoods_under_tree_likelihood_batch():
    """about 40 evenly spaced radius-3 moves of the 17-leaf family of s20: the rearranged trees with lengths grid[tau], one batch"""
    from cherryml_amd.evaluation import tree_likelihood_batch
    S, grid, fams = nni_cases.case("s20")
    Q, pi = bl_cases.model(S)
    parent, _, codes, rates = fams[1]
    with _fitter(S, grid, [fams[1]]) as fit:
        fit.round()
        every = fit.spr_moves()[0]
        pick = every[::max(len(every) // 40, 1)]
        moves, _, ll_moves = fit.spr_scan([pick], per_site=True)
        tau = fit.indices()[0]
    trees = []
    for mv in moves[0]:
        cand, ctau = spr_reference.apply(parent, tau, [mv])
        trees.append(_tree(cand, np.where(ctau >= 0, np.asarray(grid)[ctau], 0.0)))
    want = tree_likelihood_batch(trees, [codes] * len(trees), None, Q, pi, [rates] * len(trees))
    err = max(np.abs(a - b).max() for a, b in zip(ll_moves[0], want))
    print(f"against tree_likelihood_batch on {len(trees)} rearranged trees: max |d ll'| = {err:.2e}")
    assert 40 <= len(trees) <= 45 and err < 1e-10


def _scan(fams, moves=None, rounds=1):
    with _fitter(20, bl_cases.GRID, fams) as fit:
        for _ in range(rounds):
            fit.round()
        return fit.spr_scan(moves, per_site=True)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_two_scans_a_family_alone_a_subset_and_chunks_agree_bitwise(monkeypatch):
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]
    with _fitter(20, bl_cases.GRID, fams) as fit:
        fit.round()
        moves, delta, ll = fit.spr_scan(per_site=True)
        _, delta2, ll2 = fit.spr_scan(per_site=True)                          # the same handle again
        assert _same(delta, delta2) and _same(ll, ll2)
        assert _same(fit.spr_scan()[1], delta)                                # without the per-site output
        # a subset of the list (every third move, the families' lists of different length; one family with none)
        sub = [moves[0][::3], moves[1][:0], moves[2][1::3]]
        _, dsub, lsub = fit.spr_scan(sub, per_site=True)
        assert _same(dsub, [delta[0][::3], delta[1][:0], delta[2][1::3]]) and _same(lsub, [ll[0][::3], ll[1][:0], ll[2][1::3]])
        # the moves in chunks of one, and of three of the second family, through the test hook: the same bits
        for bound in ("1", str(3 * 74 * 8)):
            monkeypatch.setenv("CB_SPR_LL_BYTES", bound)
            _, d3, l3 = fit.spr_scan(per_site=True)
            assert _same(d3, delta) and _same(l3, ll), bound
        monkeypatch.delenv("CB_SPR_LL_BYTES")
    _, delta4, ll4 = _scan(fams)                                              # another handle
    assert _same(delta, delta4) and _same(ll, ll4)
    for k, f in enumerate(fams):                                              # a family alone
        _, d1, l1 = _scan([f])
        assert np.array_equal(d1[0], delta[k]) and np.array_equal(l1[0], ll[k]), k


def test_a_scan_leaves_the_handle_as_it_was():
    """two handles, one that scans and one that does not: round(), indices(), log_likelihoods() and nni_scan() bit for bit;
    the scanning handle scans before a round, between rounds and at its fixed point"""
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]

    def run(scan):
        out = []
        with _fitter(20, bl_cases.GRID, fams) as fit:
            if scan:
                fit.spr_scan()
            out.append(fit.nni_scan(per_site=True)[1:])
            out.append(fit.round())
            if scan:
                fit.spr_scan(per_site=True)
            out.append((fit.indices(), fit.log_likelihoods()))
            if scan:
                fit.spr_scan([m[:1] for m in fit.spr_moves()])
            out.append(fit.round())
            out.append(fit.nni_scan(per_site=True)[1:])
            out.append(fit.round())
            for _ in range(100):                                              # on to every family's fixed point
                n_changed, fam_ll = fit.round()
                if not n_changed.any():
                    break
            if scan:
                fit.spr_scan()
            out.append((fit.round(), fit.indices(), fit.log_likelihoods(), fit.nni_scan(per_site=True)[1:]))
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
        moves = fit.spr_moves()
        some = [moves[0], moves[1][:0], moves[2][:2]]
        n_moves = np.array([len(m) for m in some], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(some).reshape(-1), dtype=np.int32)
        delta, fam, ms = np.zeros(int(n_moves.sum())), np.zeros(3), np.zeros(2)

        def call():
            rc = _lib.load().cb_bl_spr_scan(fit._handle(), n_moves.ctypes.data, flat.ctypes.data, delta.ctypes.data, None,
                                            fam.ctypes.data, ms.ctypes.data)
            assert rc == 0, _lib.load().cb_last_error()
        call()
        first = fam.copy()
        want = fit.log_likelihoods()[1]
        assert np.isnan(first[1]) and first[0] == want[0] and first[2] == want[2]   # bitwise; no pass ran for family 1
        call()
        assert np.array_equal(fam, want) and ms[0] > 0 and ms[1] > 0
        assert np.array_equal(delta, np.concatenate(fit.spr_scan(some)[1]))


def test_the_refusals_name_the_value_and_the_handle_still_works():
    from cherryml_amd import _lib
    # family 0: the ladder [-1, 0, 0, 1, 1, 3, 3]; family 1: the 11-leaf caterpillar, internal nodes 0 .. 9 in a chain, leaf k
    # (node 10 + k) under internal min(k, 9): x = 19 (p = 9, s = 20, g = 8) is at distance 9 of leaf 10 and of leaf 11
    fams = [nni_cases.case("s4small")[2][1], spr_reference.deep_family()]
    with _fitter(4, bl_cases.GRID, fams) as fit:
        moves, delta = fit.spr_scan()
        T = len(bl_cases.GRID)
        for bad, match in [((21, 3, 1, 1, 1), "family 1 move 1: x = 21 (0 <= index < 21)"),
                           ((19, -1, 1, 1, 1), "family 1 move 1: y = -1 (0 <= index < 21)"),
                           ((0, 3, 1, 1, 1), "family 1 move 1: x = 0 is the root"),
                           ((1, 3, 1, 1, 1), "family 1 move 1: p = parent[x] = 0 is the root"),
                           ((19, 0, 1, 1, 1), "family 1 move 1: y = 0 is the root"),
                           ((19, 19, 1, 1, 1), "family 1 move 1: y = 19 equals x"),
                           ((19, 9, 1, 1, 1), "family 1 move 1: y = 9 equals p"),
                           ((19, 20, 1, 1, 1), "family 1 move 1: y = 20 equals s"),
                           ((5, 18, 1, 1, 1), "family 1 move 1: y = 18 lies in the subtree of x = 5"),
                           ((19, 10, 1, 1, 1), "family 1 move 1: y = 10 is at distance 9 of x = 19 (at most 8)"),
                           ((19, 1, T, 1, 1), f"family 1 move 1: tau_s = {T} (0 <= index < {T})"),
                           ((19, 1, 1, -1, 1), f"family 1 move 1: tau_p = -1 (0 <= index < {T})"),
                           ((19, 1, 1, 1, T + 5), f"family 1 move 1: tau_y = {T + 5} (0 <= index < {T})")]:
            with pytest.raises(_lib.CherryBankError) as e:
                fit.spr_scan([moves[0], np.array([moves[1][0], bad])])
            assert "cb_bl_spr_scan" in str(e.value) and match in str(e.value), (bad, str(e.value))
        n_moves = np.array([1, -2], dtype=np.int32)
        out = np.zeros(4)
        rc = _lib.load().cb_bl_spr_scan(fit._handle(), n_moves.ctypes.data, np.ascontiguousarray(moves[0]).ctypes.data,
                                        out.ctypes.data, None, None, None)
        assert rc == _lib.CB_EINVAL and "family 1: n_moves = -2" in _lib.load().cb_last_error().decode()
        again = fit.spr_scan()[1]
        assert all(np.array_equal(x, y) for x, y in zip(delta, again))        # bitwise, after the refusals
        n_changed, _ = fit.round()
        assert n_changed.any()
    # p not binary: the 11-node tree of s4 has a trifurcating internal node
    S, grid, fams = nni_cases.case("s4")
    parent = fams[1][0]
    arity = np.bincount(parent[parent >= 0], minlength=len(parent))
    p = [v for v in range(len(parent)) if arity[v] == 3 and parent[v] >= 0][0]
    x = [v for v in range(len(parent)) if parent[v] == p][0]
    with _fitter(S, grid, fams) as fit:
        with pytest.raises(_lib.CherryBankError) as e:
            fit.spr_scan([np.zeros((0, 5)), np.array([(x, int(parent[p]), 1, 1, 1)])])
        assert f"family 1 move 0: p = parent[x] = {p} has 3 children (exactly 2)" in str(e.value), str(e.value)
        assert all(np.all(np.isfinite(d)) for d in fit.spr_scan()[1])


# ---------------------------------------------------------------------------------------------------------- the search
def _spr_lines(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[-2].startswith("final ")
    rounds = [ln.split() for ln in lines[:-2]]
    assert [r[0] for r in rounds] == [str(i) for i in range(len(rounds))]
    lls = [x for r in rounds for x in (float(r[1]), float(r[5]))] + [float(lines[-2].split()[1])]
    assert all(b >= a for a, b in zip(lls, lls[1:])), lls                     # no number below the one before it
    return [(float(r[1]), int(r[2]), int(r[3]), int(r[4]), float(r[5])) for r in rounds], lls[-1]


def test_the_search_on_a_simulated_family_takes_the_restated_searchs_moves(tmp_path):
    """spr_reference.search_family: the 12-leaf family of nni_cases, started one radius-3 SPR from its true tree (three splits
    wrong); every decision of the restated search has a margin above 1e-9 |log-likelihood| (tests/test_spr_cpu.py asserts it),
    so the stage must scan, select, apply and accept as the restatement does and end on the same tree at the same lengths"""
    from cherryml_amd import ml_spr_trees
    from cherryml_amd.io import read_tree, write_rate_matrix, write_tree
    f, r = spr_reference.search_family(), spr_reference.restated_search()
    assert r["margin"] > 1e-9 and r["em_margin"] > 1e-9
    Q, _ = bl_cases.model(20)
    grid = np.array(bl_cases.GRID)
    parent = f["start_parent"]
    leaves = sorted(set(range(len(parent))) - set(parent.tolist()))
    for d in ("tree", "msa", "rates"):
        (tmp_path / d).mkdir()
    write_tree(_tree(parent, np.where(f["start_tau"] >= 0, grid[f["start_tau"]], 0.0)), str(tmp_path / "tree" / "f.txt"))
    (tmp_path / "msa" / "f.txt").write_text("".join(f">n{v}\n{''.join(AA[k] for k in f['codes'][v])}\n" for v in leaves))
    (tmp_path / "rates" / "f.txt").write_text(f"{len(f['rates'])} sites\n" + " ".join(repr(float(x)) for x in f["rates"]))
    write_rate_matrix(Q, AA, str(tmp_path / "q.txt"))
    ml_spr_trees(tree_dir=str(tmp_path / "tree"), msa_dir=str(tmp_path / "msa"), site_rates_dir=str(tmp_path / "rates"),
                 families=["f"], rate_matrix_path=str(tmp_path / "q.txt"), num_spr_rounds=spr_reference.SEARCH_SPR_ROUNDS,
                 num_rounds=spr_reference.SEARCH_EM_ROUNDS, quantization_grid_num_steps=64, output_tree_dir=str(tmp_path / "out"),
                 output_likelihood_dir=str(tmp_path / "ll"))
    rounds, final = _spr_lines(str(tmp_path / "out" / "f.spr"))
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
    from cherryml_amd import caching, nj_ml_trees, nj_spr_trees
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
        out = nj_spr_trees(num_spr_rounds=2, **args)
        monkeypatch.setattr(_ml_lengths.BranchLengthFitter, "_create", lambda self: pytest.fail("the second call ran the search"))
        assert nj_spr_trees(num_spr_rounds=2, **args) == out                   # the cache
    finally:
        caching.set_cache_dir(None)
    assert str(tmp_path / "cache" / "ml_spr_trees") in out["output_tree_dir"]
    assert out["output_site_rates_dir"] == ml["output_site_rates_dir"]         # nj_trees ran once
    for fam in fams:
        t_in = read_tree(os.path.join(ml["output_tree_dir"], fam + ".txt"))
        t_out = read_tree(os.path.join(out["output_tree_dir"], fam + ".txt"))
        assert t_out.nodes() == t_in.nodes() and set(t_out.leaves()) == set(t_in.leaves())
        assert [v for _, v, _ in t_out.edges()] == [v for _, v, _ in t_in.edges()]
        assert all(t in grid for _, _, t in t_out.edges())
        rounds, final = _spr_lines(os.path.join(out["output_tree_dir"], fam + ".spr"))
        assert 1 <= len(rounds) <= 2 and all(r[1] > 0 and r[2] >= r[3] for r in rounds)
        ll_file = _total(os.path.join(out["output_likelihood_dir"], fam + ".txt"))
        ll_ml = _total(os.path.join(ml["output_likelihood_dir"], fam + ".txt"))
        print(f"{fam}: nj_ml_trees {ll_ml:.4f}, SPR rounds {rounds}, final {final:.4f}, likelihood file {ll_file:.4f}")
        assert abs(ll_file - final) < 1e-9 * abs(final)
        assert final >= ll_ml - 1e-9 * abs(ll_ml)                               # (the first round's EM is nj_ml_trees' fit)
        moved = [(u, v) for u, v, _ in t_out.edges()] != [(u, v) for u, v, _ in t_in.edges()]
        assert moved or sum(r[3] for r in rounds) == 0 or len(rounds) > 1       # a move applied shows in the tree
        assert not moved or sum(r[3] for r in rounds) > 0
        prof = open(os.path.join(out["output_tree_dir"], fam + ".profiling")).read()
        assert prof.split("\n")[-1].startswith("total_time: ") and "scan_kernel_ms: " in prof


def test_the_em_pipeline_takes_nj_spr_trees_as_its_tree_estimator(tmp_path):
    import cherryml_amd
    from cherryml_amd import caching, nj_spr_trees
    from cherryml_amd.io import read_rate_matrix, write_rate_matrix
    z, fams = _demo_msas(tmp_path, 1)
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    cache = tmp_path / "cache"
    caching.set_cache_dir(str(cache))
    try:
        res = cherryml_amd.lg_end_to_end_with_em_optimizer(
            msa_dir=str(tmp_path / "msa"), families=fams,
            tree_estimator=partial(nj_spr_trees, num_rate_categories=4, num_rounds=3, num_spr_rounds=1),
            initial_tree_estimator_rate_matrix_path=qpath, num_iterations=1, em_iterations=2, optimizer_initialization=qpath)
    finally:
        caching.set_cache_dir(None)
    Q = read_rate_matrix(res["learned_rate_matrix_path"]).to_numpy()
    assert Q.shape == (20, 20) and np.all(np.isfinite(Q)) and np.allclose(Q.sum(1), 0.0, atol=1e-9)
    dirs = res["tree_estimator_output_dirs_0"]
    assert str(cache / "ml_spr_trees") in dirs["output_tree_dir"] and str(cache / "nj_trees") in dirs["output_site_rates_dir"]
    rounds, _ = _spr_lines(os.path.join(dirs["output_tree_dir"], fams[0] + ".spr"))
    assert len(rounds) == 1
