"""The bootstrap supports from the search's own trees on the GPU (csrc/ufb.hip.h, cb_bl_bootstrap_best,
BranchLengthFitter.bootstrap_best / ufboot_supports / the bootstrap output of nj_nni_trees): every replicate's best score, its
base and its code of every case against the NumPy restatement, before any round and after one; the score and the code bit for
bit from branch_supports' resampled deltas; the simulated search family's 256 choices and nine supports; determinism, batching,
subsets, chunks and the number of replicates bit for bit; a call leaves the handle as it was; the refusals; the stage on demo
families, its files with and without the bootstrap and its cache.

The shapes (nni_cases.py): the 3-leaf star sharing a handle, the 4-leaf trees, S = 4, 20 and 32, 1, 3 and 7 sites (under one
k-step of 4) and 60 to 82 sites (several slabs of 32, not a multiple of 4), R = 256 (two replicate tiles of 128), 70 (a ragged
tile) and 64."""
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
import ufb_reference  # noqa: E402
from conftest import load_golden  # noqa: E402

AA = list("ARNDCQEGHILKMFPSTWYV")
R = ufb_reference.REPLICATES
VALUE_BAR = 1e-10      # of max(1, |fam_ll|), on base and score: DESIGN.md section 18's bar on delta, of which they are reweightings
MARGIN = 1e-9          # of max(1, |fam_ll|): the search family's replicates must be decided above this


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


def _compare(name, when, got, want, fam_ll):
    """got: bootstrap_best(base=True) of the handle; want: per family ufb_reference.best's dict"""
    for k, ((score, code, base), s) in enumerate(zip(got, want)):
        n_rep = len(s["score"])
        assert score.shape == code.shape == base.shape == (n_rep,) and code.dtype == np.int32
        bar = VALUE_BAR * max(1.0, abs(fam_ll[k]))
        err_base, err_score = np.abs(base - s["base"]).max(), np.abs(score - s["score"]).max()
        assert code.min() >= -1 and code.max() < len(s["cand"]) - 2, (name, k, when)
        chosen = s["cand"][code + 2, np.arange(n_rep)]               # the restated score of the candidate the GPU chose
        err_chosen = np.abs(chosen - s["score"]).max()
        decided = s["margin"] > bar
        print(f"{name}[{k}] {when}: {len(s['cand']) - 2} moves, max |d base| = {err_base:.2e}, max |d score| = {err_score:.2e}, "
              f"chosen within {err_chosen:.2e} of the best (bar {bar:.2e}), {int(decided.sum())} of {n_rep} decided")
        assert err_base <= bar and err_score <= bar, (name, k, when)                         # every replicate
        assert err_chosen <= bar, (name, k, when)                                             # decided or not
        assert np.array_equal(code[decided], s["code"][decided]), (name, k, when)


@pytest.mark.parametrize("name", nni_cases.CASES)
def test_best_equals_the_restatement_before_any_round_and_after_one(name):
    """after `round()` the call runs its own passes and is compared with the restatement AT the new indices; the 3-leaf star,
    which has no move, gets its own resampled log-likelihood (code -1)"""
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    seeds = _seeds(len(fams))
    with _fitter(S, grid, fams) as fit:
        got0 = fit.bootstrap_best(R, seeds, base=True)
        assert all(x > 0.0 for x in fit.last_ufboot_kernel_ms[::2])
        fam0 = fit.log_likelihoods()[1]
        ragged = fit.bootstrap_best(70, seeds, base=True)
        fit.round()
        got1 = fit.bootstrap_best(R, seeds, base=True)
        fam1 = fit.log_likelihoods()[1]
        tau1 = fit.indices()
    _compare(name, "at the start", got0, ufb_reference.restated(name), fam0)
    for k, n_moves in enumerate(nni_cases.MOVE_COUNTS[name]):
        if n_moves == 0:
            assert np.all(got0[k][1] == -1) and np.array_equal(got0[k][0], got0[k][2])
        for a, b in zip(ragged[k], got0[k]):                                                  # a ragged replicate tile
            assert np.array_equal(a, b[:70]), (name, k)
    want = []
    for k, ((parent, _, codes, rates), tau) in enumerate(zip(fams, tau1)):
        mvs = nni_reference.moves(parent)
        ll_moves, ll = nni_reference.scan(parent, tau, codes, rates, grid, Q, pi, mvs)
        want.append(ufb_reference.best(ll_moves, ll, R, seeds[k]))
    _compare(name, "after one round", got1, want, fam1)


def _from_delta_rep(base, rep, delta):
    """(score, code) of max(base, max_m fl(base + delta_rep[m])) over the moves with a finite delta: the first that attains it"""
    cand = np.vstack([base[None, :], np.where(np.isfinite(delta)[:, None], base[None, :] + rep, -np.inf)])
    arg = np.argmax(cand, axis=0)
    return cand[arg, np.arange(len(base))], (arg - 1).astype(np.int32)


@pytest.mark.parametrize("name", nni_cases.CASES)
def test_score_and_code_are_bitwise_those_of_the_branch_supports_resampled_deltas(name):
    S, grid, fams = nni_cases.case(name)
    seeds = _seeds(len(fams))
    with _fitter(S, grid, fams) as fit:
        for when in ("at the start", "after one round"):
            got = fit.bootstrap_best(R, seeds, base=True)
            sup = fit.branch_supports(R, seeds, per_replicate=True)
            _, delta = fit.nni_scan()
            for k, (score, code, base) in enumerate(got):
                want_score, want_code = _from_delta_rep(base, sup[k][4], delta[k])
                assert np.array_equal(score, want_score) and np.array_equal(code, want_code), (name, k, when)
            fit.round()


# ------------------------------------------------------------------------------------------------------------ the search
def _replay(tree, codes, rates, grid, Q, pi, nni_rounds, em_rounds, n_rep, seed):
    """ml_nni_trees' loop on one family alone, one fresh handle per tree, with bootstrap_best on every handle whose tree is
    accepted -> (the final tree, the contributing trees, (t [n_rep], code [n_rep]))"""
    from cherryml_amd import BranchLengthFitter, apply_nni, select_nni
    from cherryml_amd.io import Tree
    from cherryml_amd.phylogeny_estimation._nni import _parent_array
    contribs, best = [], None
    t_arr, c_arr = np.full(n_rep, -1, dtype=np.int64), np.full(n_rep, -2, dtype=np.int64)
    rnd, before, fitted, sel, cur = 0, None, None, None, tree
    while True:
        with BranchLengthFitter([cur], [codes], [rates], grid, Q, pi) as fit:
            go = True
            if before is not None:
                if fit.log_likelihoods()[1][0] > before:
                    rnd += 1
                else:
                    go = False
            if go:
                for _ in range(em_rounds):
                    if fit.round()[0][0] == 0:
                        break
                lengths, ll = fit.lengths()[0], float(fit.log_likelihoods()[1][0])
                want = rnd < nni_rounds
                if want:
                    moves, delta = fit.nni_scan()
                    picked = moves[0][select_nni(moves[0], delta[0], _parent_array(cur))]
                score, code = fit.bootstrap_best(n_rep, [seed], best=None if best is None else [best])[0]
        if not go:
            if len(sel) > 1:
                sel = sel[:len(sel) // 2]
                cur = apply_nni(fitted, sel)
                continue
            return fitted, contribs, (t_arr, c_arr)
        t = Tree()
        t.add_nodes(cur.nodes())
        t.add_edges([(u, v, lengths[v]) for u, v, _ in cur.edges()])
        won = code != -2
        t_arr[won], c_arr[won], best = len(contribs), code[won], score
        contribs.append(t)
        if not want or len(picked) == 0:
            return t, contribs, (t_arr, c_arr)
        fitted, before, sel, cur = t, ll, picked, apply_nni(t, picked)


def test_the_search_family_chooses_the_restated_trees_and_gets_the_restated_supports():
    """nni_cases.search_family, seed 1: 2 contributions, 50 candidates; every replicate's margin is above 1e-9 |sum l| (1.57e-2
    against 2.7e-6: tests/test_ufb_cpu.py), so all 256 (t, code) pairs and the nine supports are the restatement's exactly"""
    from cherryml_amd.phylogeny_estimation import ufboot_supports
    from cherryml_amd.phylogeny_estimation._nni import _parent_array
    f = nni_cases.search_family()
    final_parent, contribs, c, (want_nodes, want_share) = ufb_reference.restated_search()
    bar = MARGIN * max(1.0, abs(float(contribs[-1]["ll"].sum())))
    assert int((c["margin"] <= bar).sum()) == 0                                # none is undecided, none is left out
    grid = np.array(bl_cases.GRID)
    Q, pi = bl_cases.model(20)
    start = _tree(f["start_parent"], np.where(f["tau"] >= 0, grid[f["tau"]], 0.0))
    final, trees, (t_arr, code) = _replay(start, f["codes"], f["rates"], bl_cases.GRID, Q, pi, nni_cases.SEARCH_NNI_ROUNDS,
                                          nni_cases.SEARCH_EM_ROUNDS, R, 1)
    assert len(trees) == len(contribs) == 2
    for tree, want in zip(trees, contribs):
        assert np.array_equal(_parent_array(tree), want["parent"])
    assert np.array_equal(_parent_array(final), final_parent)
    assert np.array_equal(t_arr, c["t"]) and np.array_equal(code, c["code"])   # all 256 pairs
    nodes, share = ufboot_supports(final, trees, (t_arr, code))
    print("ufboot", dict(zip(nodes.tolist(), share.tolist())))
    assert np.array_equal(nodes, want_nodes) and np.array_equal(share, want_share)


# ------------------------------------------------------------------------------------------------------- bit for bit
def _same(a, b):
    def flat(x):
        return [z for y in x for z in flat(y)] if isinstance(x, (tuple, list)) else [np.asarray(x)]
    a, b = flat(a), flat(b)
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_two_calls_another_handle_a_family_alone_subsets_chunks_and_fewer_replicates_agree_bitwise(monkeypatch):
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]
    Q, pi = bl_cases.model(20)
    seeds = [11, (1 << 63) + 7, 1001]

    def run(which, n_rep=R):
        with _fitter(20, bl_cases.GRID, [fams[k] for k in which]) as fit:
            fit.round()
            return fit.bootstrap_best(n_rep, [seeds[k] for k in which], base=True)

    with _fitter(20, bl_cases.GRID, fams) as fit:
        fit.round()
        first = fit.bootstrap_best(R, seeds, base=True)
        assert _same(first, fit.bootstrap_best(R, seeds, base=True))                           # the same handle again
        assert _same([x[:2] for x in first], fit.bootstrap_best(R, seeds))                     # without the base
        # one move tile per chunk, and chunks of a few tiles, through the test hook: the same bits
        for bound in ("1", str(2 * 16 * 82 * 8)):   # (34 moves: 16 + 16 + 2, and 32 + 2)
            monkeypatch.setenv("CB_UFB_BYTES", bound)
            assert _same(first, fit.bootstrap_best(R, seeds, base=True)), bound
        monkeypatch.delenv("CB_UFB_BYTES")
        # a subset of the moves in another order, ungrouped: none of the first family's, a shuffled half of the second's
        moves = fit.nni_moves()
        sup = fit.branch_supports(R, seeds, per_replicate=True)
        _, delta = fit.nni_scan()
        tau = fit.indices()
        fam_ll = fit.log_likelihoods()[1]
        keep = np.random.default_rng(5).permutation(len(moves[1]))[:len(moves[1]) // 2]
        assert len(keep) > 16 and np.any(np.diff(moves[1][keep, 0]) < 0)
        sub = fit.bootstrap_best(R, seeds, base=True, moves=[moves[0][:0], moves[1][keep], moves[2]])
        assert np.all(sub[0][1] == -1) and np.array_equal(sub[0][0], first[0][2]) and _same(sub[2], first[2])
        want_score, want_code = _from_delta_rep(first[1][2], sup[1][4][keep], delta[1][keep])
        assert np.array_equal(sub[1][0], want_score) and np.array_equal(sub[1][1], want_code)
        parent, _, codes, rates = fams[1]
        ll_moves, ll = nni_reference.scan(parent, tau[1], codes, rates, bl_cases.GRID, Q, pi, moves[1][keep])
        _compare("s20[1]", "a shuffled half of the moves", [sub[1]], [ufb_reference.best(ll_moves, ll, R, seeds[1])], fam_ll[1:2])
        few = fit.bootstrap_best(64, seeds, base=True)                                         # replicate r does not depend on R
        for a, b in zip(few, first):
            assert all(np.array_equal(x, y[:64]) for x, y in zip(a, b))
        # an incoming best nothing beats stays, one everything beats never does; a call's own result, fed back, stays too
        stay = fit.bootstrap_best(R, seeds, best=[np.full(R, np.inf)] * 3)
        assert all(np.all(code == -2) and np.all(score == np.inf) for score, code in stay)
        assert _same([x[:2] for x in first], fit.bootstrap_best(R, seeds, best=[np.full(R, -np.inf)] * 3))
        assert not any(np.any(x[1] == -2) for x in first)
        again = fit.bootstrap_best(R, seeds, best=[x[0] for x in first])
        assert all(np.all(code == -2) and np.array_equal(score, x[0]) for (score, code), x in zip(again, first))
    assert _same(first, run([0, 1, 2]))                                                        # another handle
    for k in range(3):                                                                         # a family alone
        assert _same(run([k])[0], first[k]), k


def test_the_call_leaves_the_handle_as_it_was():
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]

    def run(ufb):
        out = []
        with _fitter(20, bl_cases.GRID, fams) as fit:
            if ufb:
                fit.bootstrap_best(64)
            out.append(fit.round())
            if ufb:
                fit.bootstrap_best(64, base=True)
            out.append((fit.indices(), fit.log_likelihoods()))
            out.append(fit.nni_scan(per_site=True))
            if ufb:
                fit.bootstrap_best(16, moves=[m[:2] for m in fit.nni_moves()])
            out.append(fit.branch_supports(64, per_replicate=True))
            out.append(fit.ancestral_states(posteriors=True))
            out.append(fit.round())
            if ufb:
                fit.bootstrap_best(64)
            out.append((fit.round(), fit.indices(), fit.log_likelihoods(), fit.nni_scan(), fit.branch_supports(32),
                        fit.ancestral_states()))
        return out

    assert _same(run(False), run(True))


def test_the_refusals_name_the_value_and_the_handle_still_works():
    from cherryml_amd import _lib
    S, grid, fams = nni_cases.case("s4small")       # family 1: the ladder [-1, 0, 0, 1, 1, 3, 3]
    with _fitter(S, grid, fams) as fit:
        moves = fit.nni_moves()
        first = fit.bootstrap_best(R, [1, 2], base=True)
        ladder = moves[1]
        assert ladder[:, 0].tolist() == [1, 1, 3, 3]
        nan = np.zeros(R)
        nan[37] = np.nan
        for bad_moves, n_rep, best, match in [
                ([moves[0], ladder], 0, None, "n_rep = 0 "),
                ([moves[0], ladder], 65537, None, "n_rep = 65537 "),
                ([moves[0], ladder], R, [np.zeros(R), nan], "family 1 replicate 37"),
                ([moves[0], np.array([ladder[0], (3, 5, 2)])], R, None, "family 1 move 1: s = 2 is not a child of parent[v] = 1"),
                ([moves[0], np.array([ladder[0], (7, 5, 4)])], R, None, "family 1 move 1: v = 7 (0 <= index < 7)"),
                ([moves[0], np.array([ladder[0], (0, 1, 2)])], R, None, "family 1 move 1: v = 0 is the root")]:
            with pytest.raises(_lib.CherryBankError) as e:
                fit.bootstrap_best(n_rep, [1, 2], moves=bad_moves, best=None if best is None else [b[:max(n_rep, 0)] for b in best])
            assert "cb_bl_bootstrap_best" in str(e.value) and match in str(e.value), (match, str(e.value))
        assert _same(first, fit.bootstrap_best(R, [1, 2], base=True))            # bitwise, after six refusals
        mixed = fit.bootstrap_best(R, [1, 2], base=True, moves=[moves[0], ladder[[0, 2, 1, 3]]])   # ungrouped moves are no refusal:
        assert np.array_equal(mixed[1][0], first[1][0]) and np.array_equal(mixed[1][2], first[1][2])   # the same maximum
        n_changed, _ = fit.round()
        assert n_changed.any()


# ---------------------------------------------------------------------------------------------------------- the stage
def _demo_msas(tmp_path, k):
    z = load_golden("demo_e2e.npz")
    fams = [str(f) for f in z["families"]]
    small = sorted(range(len(fams)), key=lambda i: (len(str(z["text_msa"][i])), fams[i]))[:k]
    (tmp_path / "msa").mkdir()
    for i in small:
        (tmp_path / "msa" / f"{fams[i]}.txt").write_text(str(z["text_msa"][i]))
    return z, [fams[i] for i in small]


def test_nj_nni_trees_writes_the_same_files_with_and_without_the_bootstrap_and_the_replayed_supports(tmp_path, monkeypatch):
    from cherryml_amd import caching, nj_nni_trees
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation._likelihood import _family_units, _stationary_distribution
    from cherryml_amd.io import read_rate_matrix, read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation import _ml_lengths, read_ufboot_supports, ufboot_supports
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    from cherryml_amd.simulation._simulate import family_seed
    z, fams = _demo_msas(tmp_path, 2)
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    n_rep, seed = 100, 3
    args = dict(msa_dir=str(tmp_path / "msa"), families=fams, rate_matrix_path=qpath, num_rate_categories=4, num_rounds=3,
                num_nni_rounds=2, num_support_replicates=50)
    boot_args = dict(output_bootstrap_dir=str(tmp_path / "boot"), num_bootstrap_replicates=n_rep, bootstrap_seed=seed)
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        plain = nj_nni_trees(output_support_dir=str(tmp_path / "sup0"), **args)
        assert not os.path.exists(str(tmp_path / "boot"))
        boot = nj_nni_trees(output_support_dir=str(tmp_path / "sup1"), **args, **boot_args)
        with monkeypatch.context() as mp:
            mp.setattr(_ml_lengths.BranchLengthFitter, "_create", lambda self: pytest.fail("the second call ran the stage"))
            assert nj_nni_trees(output_support_dir=str(tmp_path / "sup1"), **args, **boot_args) == boot   # the cache
    finally:
        caching.set_cache_dir(None)
    assert plain["output_tree_dir"] != boot["output_tree_dir"] and set(plain) == set(boot)        # both ran
    for fam in fams:
        for key, ext in (("output_tree_dir", ".txt"), ("output_tree_dir", ".nni"), ("output_likelihood_dir", ".txt")):
            a, b = (open(os.path.join(d[key], fam + ext), "rb").read() for d in (plain, boot))
            assert a == b and len(a) > 0, (fam, key, ext)
        a, b = (open(str(tmp_path / d / (fam + ".txt")), "rb").read() for d in ("sup0", "sup1"))
        assert a == b and len(a) > 0, fam
    # the bootstrap files against a replay of each family ALONE on fresh handles (a family's file does not depend on its batch)
    rm = read_rate_matrix(qpath)
    Q = np.ascontiguousarray(rm.to_numpy(), dtype=np.float64)
    grid = np.array(quantization_points_ble(0.03, 1.1, 64))
    nj_tree_dir = os.path.join(os.path.dirname(boot["output_site_rates_dir"]), "output_tree_dir")   # nj_trees' cached output
    for fam in fams:
        start = read_tree(os.path.join(nj_tree_dir, fam + ".txt"))
        rates = np.asarray(read_site_rates(os.path.join(boot["output_site_rates_dir"], fam + ".txt")), dtype=np.float64)
        codes = _family_units(start, read_msa(os.path.join(args["msa_dir"], fam + ".txt")), None, len(rates),
                              [str(c) for c in rm.columns], False)[2]
        final, trees, choice = _replay(start, codes, rates, grid, Q, _stationary_distribution(Q), 2, 3, n_rep, family_seed(fam, seed))
        nodes, share = ufboot_supports(final, trees, choice)
        names = list(final.nodes())
        internal = [v for v in names if not final.is_leaf(v) and v != final.root()]
        lines = open(str(tmp_path / "boot" / (fam + ".txt"))).read().split("\n")
        assert lines[0] == "node ufboot" and lines[-1] == "" and [ln.split()[0] for ln in lines[1:-1]] == internal
        assert [names[v] for v in nodes] == internal and len(internal) >= 1
        got = read_ufboot_supports(str(tmp_path / "boot" / (fam + ".txt")))
        written = read_tree(os.path.join(boot["output_tree_dir"], fam + ".txt"))
        assert list(written.nodes()) == names and sorted((u, v) for u, v, _ in written.edges()) == sorted((u, v) for u, v, _ in final.edges())
        for v, s in zip(internal, share):
            assert got[v] == s, (fam, v)                                          # the replay's value, bit for bit
            assert 0.0 <= s <= 1.0 and round(s * n_rep) / n_rep == s
        rows = [[int(x) for x in ln.split()] for ln in open(str(tmp_path / "boot" / (fam + ".choices"))).read().split("\n") if ln]
        assert [r[0] for r in rows] == list(range(len(trees))) and sum(r[3] + r[4] for r in rows) == n_rep
        for t, r in enumerate(rows):
            assert r[3] == int(np.sum((choice[0] == t) & (choice[1] == -1))) and r[4] == int(np.sum((choice[0] == t) & (choice[1] >= 0)))
