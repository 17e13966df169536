"""The marginal ancestral reconstruction on the GPU (csrc/anc.hip.h, cb_bl_ancestral, BranchLengthFitter.ancestral_states /
ml_ancestral_sequences): every (node, site) of every case against the NumPy restatement, before any round and after one; the
imputation of an all-gap leaf through the held-out likelihood; two calls, handles, batches, output sets and node chunks bit for
bit; a reconstruction leaves the handle as it was; the refusal; a site that is impossible under a reducible model; the stage on
demo families."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import anc_reference  # noqa: E402
import bl_cases  # noqa: E402
import bl_reference  # noqa: E402
import nni_cases  # noqa: E402
from conftest import load_golden  # noqa: E402

AA = list("ARNDCQEGHILKMFPSTWYV")


def _tree(parent, length):
    from cherryml_amd.io import Tree
    t = Tree()
    t.add_nodes([f"n{v}" for v in range(len(parent))])
    t.add_edges([(f"n{p}", f"n{v}", float(length[v])) for v, p in enumerate(parent) if p >= 0])
    return t


def _fitter(S, grid, fams, model=None):
    from cherryml_amd import BranchLengthFitter
    Q, pi = bl_cases.model(S) if model is None else model
    return BranchLengthFitter([_tree(f[0], f[1]) for f in fams], [f[2] for f in fams], [f[3] for f in fams], grid, Q, pi)


@functools.lru_cache(maxsize=None)
def _restated_at_the_start(name):
    """per family (tau, post, ll) of the restatement at the snapped input lengths"""
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    out = []
    for parent, length, codes, rates in fams:
        tau = bl_reference.snap(length, parent, grid)
        out.append((tau,) + anc_reference.posteriors(parent, tau, codes, rates, grid, Q, pi))
    return out


def _compare(name, when, got, want):
    """got = (states, confidence, posteriors) of the handle, want = per family (post, ll) of the restatement"""
    states, confs, posts = got
    for k, (ref, ll) in enumerate(want):
        state, conf, post = states[k], confs[k], posts[k]
        assert state.dtype == np.int8 and conf.dtype == np.float64 and post.dtype == np.float64
        assert post.shape == ref.shape and state.shape == conf.shape == ref.shape[:2]
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(post)) and np.all(np.isfinite(conf))
        ref_state, _, margin = anc_reference.states(ref)
        err = np.abs(post - ref) / np.maximum(1.0, np.abs(ll))[None, :, None]
        sums = np.abs(post.sum(axis=2) - 1.0).max()
        print(f"{name}[{k}] {when}: {state.size} (node, site) entries, max |d post| / max(1, |l_u|) = {err.max():.2e}, "
              f"max |d post| = {np.abs(post - ref).max():.2e}, max |sum post - 1| = {sums:.2e}, smallest margin {margin.min():.2e}")
        assert np.array_equal(state, ref_state), (name, k, when)              # at EVERY (node, site): test_anc_cpu.py's margins
        assert err.max() <= 1e-10, (name, k, when)
        assert np.array_equal(conf, np.take_along_axis(post, state.astype(np.int64)[:, :, None], axis=2)[:, :, 0])   # bit for bit
        assert sums <= 1e-12, (name, k, when)


@pytest.mark.parametrize("name", nni_cases.CASES)
def test_every_node_and_site_equals_the_restatement_before_any_round_and_after_one(name):
    """the cases of nni_cases.py; after `round()` the resident messages belong to the round's start and qb holds the new
    indices: the reconstruction runs its own passes, and is compared with the restatement AT the new indices"""
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    with _fitter(S, grid, fams) as fit:
        got0 = fit.ancestral_states(posteriors=True)
        tau0 = fit.indices()
        fit.round()
        got1 = fit.ancestral_states(posteriors=True)
        tau1 = fit.indices()
        assert fit.last_ancestral_kernel_ms[0] > 0.0 and fit.last_ancestral_kernel_ms[1] > 0.0
    rest = _restated_at_the_start(name)
    assert all(np.array_equal(a, r[0]) for a, r in zip(tau0, rest))
    _compare(name, "at the start", got0, [r[1:] for r in rest])
    assert any(not np.array_equal(a, b) for a, b in zip(tau0, tau1))          # the round moved
    want = [anc_reference.posteriors(parent, tau, codes, rates, grid, Q, pi) for (parent, _, codes, rates), tau in zip(fams, tau1)]
    _compare(name, "after one round", got1, want)
    # observed leaves: their own state, posterior exactly 1
    for (parent, _, codes, _), state, conf in zip(fams, got1[0], got1[1]):
        leaves = sorted(set(range(len(parent))) - set(parent.tolist()))
        obs = codes[leaves] >= 0
        assert np.array_equal(state[leaves][obs], codes[leaves][obs]) and np.all(conf[leaves][obs] == 1.0)


def test_the_imputed_leaf_has_the_posterior_tree_likelihood_batch_gives_its_s_variants():
    """the all-gap leaf of the 17-leaf family of `s20`: its code replaced at every site by each of the S states, the S variants
    scored by the held-out likelihood at the lengths grid[tau] in one batch; their normalised likelihoods are its posterior"""
    from cherryml_amd.evaluation import tree_likelihood_batch
    S, grid, fams = nni_cases.case("s20")
    Q, pi = bl_cases.model(S)
    parent, _, codes, rates = fams[1]
    leaf = sorted(set(range(len(parent))) - set(parent.tolist()))[0]
    assert np.all(codes[leaf] == -1)
    with _fitter(S, grid, fams) as fit:
        _, _, posts = fit.ancestral_states(posteriors=True)
        tau = fit.indices()[1]
    tree = _tree(parent, np.where(tau >= 0, np.asarray(grid)[tau], 0.0))
    variants = []
    for a in range(S):
        c = codes.copy()
        c[leaf] = a
        variants.append(c)
    ll = np.array(tree_likelihood_batch([tree] * S, variants, None, Q, pi, [rates] * S))     # [S, sites]
    want = np.exp(ll - ll.max(axis=0, keepdims=True))
    want = (want / want.sum(axis=0, keepdims=True)).T
    err = np.abs(posts[1][leaf] - want).max()
    print(f"the all-gap leaf against {S} tree_likelihood_batch variants: max |d post| = {err:.2e}")
    assert want.shape == posts[1][leaf].shape and err <= 1e-10


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _reconstruct(fams, rounds=1):
    with _fitter(20, bl_cases.GRID, fams) as fit:
        for _ in range(rounds):
            fit.round()
        return fit.ancestral_states(posteriors=True)


def test_two_calls_handles_a_family_alone_the_outputs_asked_for_and_chunks_agree_bitwise(monkeypatch):
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]
    with _fitter(20, bl_cases.GRID, fams) as fit:
        fit.round()
        state, conf, post = fit.ancestral_states(posteriors=True)
        state2, conf2, post2 = fit.ancestral_states(posteriors=True)          # the same handle again
        assert _same(state, state2) and _same(conf, conf2) and _same(post, post2)
        state3, conf3 = fit.ancestral_states()                                # without the posteriors
        assert _same(state, state3) and _same(conf, conf3)
        # the nodes in chunks of one, and of three of the second family (74 sites), through the test hook: the same bits
        for bound in (str(74 * 20 * 8), str(3 * 74 * 20 * 8)):
            monkeypatch.setenv("CB_ANC_POST_BYTES", bound)
            s4, c4, p4 = fit.ancestral_states(posteriors=True)
            assert _same(s4, state) and _same(c4, conf) and _same(p4, post), bound
        monkeypatch.delenv("CB_ANC_POST_BYTES")
    s5, c5, p5 = _reconstruct(fams)                                           # another handle
    assert _same(state, s5) and _same(conf, c5) and _same(post, p5)
    for k, f in enumerate(fams):                                              # a family alone
        s1, c1, p1 = _reconstruct([f])
        assert np.array_equal(s1[0], state[k]) and np.array_equal(c1[0], conf[k]) and np.array_equal(p1[0], post[k]), k


def test_a_reconstruction_leaves_the_handle_as_it_was():
    fams = nni_cases.case("s20")[2] + nni_cases.case("s20one")[2]

    def run(rec):
        out = []
        with _fitter(20, bl_cases.GRID, fams) as fit:
            if rec:
                fit.ancestral_states()
            out.append(fit.nni_scan(per_site=True))
            out.append(fit.round())
            if rec:
                fit.ancestral_states(posteriors=True)
            out.append((fit.indices(), fit.log_likelihoods(), fit.nni_scan(per_site=True)))
            out.append(fit.round())
            if rec:
                fit.ancestral_states()
            out.append(fit.round())
            for _ in range(100):                                              # on to every family's fixed point
                n_changed, fam_ll = fit.round()
                if not n_changed.any():
                    break
            assert not n_changed.any()
            if rec:
                fit.ancestral_states(posteriors=True)
            out.append((fit.round(), fit.indices(), fit.log_likelihoods(), fit.nni_scan(per_site=True)))
        return out

    def flat(x):
        if isinstance(x, (tuple, list)):
            return [z for y in x for z in flat(y)]
        return [np.asarray(x)]

    a, b = flat(run(False)), flat(run(True))
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_fam_ll_of_the_c_entry_point_is_cb_bl_gets():
    from cherryml_amd import _lib
    fams = nni_cases.case("s20")[2]
    with _fitter(20, bl_cases.GRID, fams) as fit:
        fit.round()                                                           # every family's likelihood is the old indices' now
        state = np.zeros(int((fit.n_nodes.astype(np.int64) * fit.n_units).sum()), dtype=np.int8)
        fam, ms = np.zeros(2), np.zeros(2)
        rc = _lib.load().cb_bl_ancestral(fit._handle(), state.ctypes.data, None, None, fam.ctypes.data, ms.ctypes.data)
        assert rc == 0, _lib.load().cb_last_error()
        assert np.array_equal(fam, fit.log_likelihoods()[1]) and ms[0] > 0 and ms[1] > 0
        assert np.array_equal(state, np.concatenate([s.reshape(-1) for s in fit.ancestral_states()[0]]))


def test_the_refusal_names_the_function_and_the_handle_still_works():
    from cherryml_amd import _lib
    S, grid, fams = nni_cases.case("s4small")
    with _fitter(S, grid, fams) as fit:
        before = fit.ancestral_states(posteriors=True)
        conf = np.zeros(int((fit.n_nodes.astype(np.int64) * fit.n_units).sum()))
        rc = _lib.load().cb_bl_ancestral(fit._handle(), None, conf.ctypes.data, None, None, None)
        assert rc == _lib.CB_EINVAL and "cb_bl_ancestral" in _lib.load().cb_last_error().decode()
        rc = _lib.load().cb_bl_ancestral(None, conf.ctypes.data, None, None, None, None)
        assert rc == _lib.CB_EINVAL and "cb_bl_ancestral" in _lib.load().cb_last_error().decode()
        after = fit.ancestral_states(posteriors=True)
        assert all(_same(x, y) for x, y in zip(before, after))
        n_changed, _ = fit.round()
        assert n_changed.any()


def test_a_site_that_is_impossible_under_a_reducible_model_gets_no_state_and_the_others_are_unaffected():
    """cb_bl_create admits a block-diagonal Q (em_check_model asks for finite entries and off-diagonals >= 0): states {0, 1} never
    reach {2, 3}, so a site whose leaves lie in both blocks has likelihood 0 -- state -1, confidence 0, a zero posterior and no
    NaN -- while the sites beside it in the same tile are those of the restatement"""
    Q = np.array([[-1.0, 1.0, 0.0, 0.0], [2.0, -2.0, 0.0, 0.0], [0.0, 0.0, -3.0, 3.0], [0.0, 0.0, 0.5, -0.5]])
    pi = np.array([0.1, 0.2, 0.3, 0.4])
    grid = bl_cases.GRID5
    bad = 5
    fams = []
    for parent, seed in ((bl_cases.star3(), 0), (nni_cases.LADDER4, 1)):
        rng = np.random.default_rng(seed)
        leaves = sorted(set(range(len(parent))) - set(parent.tolist()))
        sites = 21
        block = rng.integers(0, 2, sites)                                     # every site inside one block ...
        codes = np.full((len(parent), sites), -1, dtype=np.int8)
        for v in leaves:
            codes[v] = 2 * block + rng.integers(0, 2, sites)
        codes[leaves[1], 3] = -1                                              # (a gap beside the impossible site)
        codes[leaves[0], bad], codes[leaves[-1], bad] = 0, 3                  # ... but one
        length = np.where(parent >= 0, 0.2, 0.0)
        rates = np.where(np.arange(sites) % 2 == 0, 0.5, 2.0)
        fams.append((parent, length, codes, rates))
    with _fitter(4, grid, fams, model=(Q, pi)) as fit:
        states, confs, posts = fit.ancestral_states(posteriors=True)
        states2, confs2 = fit.ancestral_states()
    assert _same(states, states2) and _same(confs, confs2)
    for (parent, length, codes, rates), state, conf, post in zip(fams, states, confs, posts):
        assert np.all(np.isfinite(conf)) and np.all(np.isfinite(post))
        assert np.all(state[:, bad] == -1) and np.all(conf[:, bad] == 0.0) and np.all(post[:, bad] == 0.0)
        tau = bl_reference.snap(length, parent, grid)
        ref, ll = anc_reference.posteriors(parent, tau, codes, rates, grid, Q, pi)
        assert ll[bad] == -np.inf and np.all(ref[:, bad] == 0.0)
        ok = np.arange(len(rates)) != bad
        assert np.all(np.isfinite(ll[ok]))
        ref_state, _, margin = anc_reference.states(ref)
        assert margin[:, ok].min() > 1e-9
        assert np.array_equal(state[:, ok], ref_state[:, ok])
        assert (np.abs(post - ref)[:, ok] / np.maximum(1.0, np.abs(ll[ok]))[None, :, None]).max() <= 1e-10
        assert np.abs(post[:, ok].sum(axis=2) - 1.0).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------- the stage
def _demo_msas(tmp_path, k):
    z = load_golden("demo_e2e.npz")
    fams = [str(f) for f in z["families"]]
    small = sorted(range(len(fams)), key=lambda i: (len(str(z["text_msa"][i])), fams[i]))[:k]
    (tmp_path / "msa").mkdir()
    for i in small:
        (tmp_path / "msa" / f"{fams[i]}.txt").write_text(str(z["text_msa"][i]))
    return z, [fams[i] for i in small]


def _rows(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1 and all(ln.startswith(">") for ln in lines[:-1:2])
    return [ln[1:] for ln in lines[:-1:2]], lines[1:-1:2]


def test_the_stage_on_demo_families_its_files_and_its_cache(tmp_path, monkeypatch):
    from cherryml_amd import caching, ml_ancestral_sequences, nj_ml_trees
    from cherryml_amd.counting._host import read_msa
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation import _ml_lengths
    z, fams = _demo_msas(tmp_path, 2)
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(z["lg_Q_best_f64"], AA, qpath)
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        ml = nj_ml_trees(msa_dir=str(tmp_path / "msa"), families=fams, rate_matrix_path=qpath, num_rate_categories=4, num_rounds=3)
        args = dict(tree_dir=ml["output_tree_dir"], msa_dir=str(tmp_path / "msa"), site_rates_dir=ml["output_site_rates_dir"],
                    families=fams, rate_matrix_path=qpath)
        out = ml_ancestral_sequences(write_posteriors=True, **args)
        kept = ml_ancestral_sequences(impute_gaps=False, **args)
        monkeypatch.setattr(_ml_lengths.BranchLengthFitter, "_create", lambda self: pytest.fail("the second call ran the stage"))
        assert ml_ancestral_sequences(write_posteriors=True, **args) == out    # the cache
    finally:
        caching.set_cache_dir(None)
    assert str(tmp_path / "cache" / "ml_ancestral_sequences") in out["output_msa_dir"]
    assert kept["output_msa_dir"] != out["output_msa_dir"]
    gaps = 0
    for fam in fams:
        tree = read_tree(os.path.join(ml["output_tree_dir"], fam + ".txt"))
        msa = read_msa(str(tmp_path / "msa" / f"{fam}.txt"))
        names, seqs = _rows(os.path.join(out["output_msa_dir"], fam + ".txt"))
        names_kept, seqs_kept = _rows(os.path.join(kept["output_msa_dir"], fam + ".txt"))
        assert names == names_kept == list(tree.nodes())                      # one row per tree node, in order
        conf = np.load(os.path.join(out["output_confidence_dir"], fam + ".npz"))
        conf_kept = np.load(os.path.join(kept["output_confidence_dir"], fam + ".npz"))
        assert sorted(conf.files) == ["alphabet", "confidence", "nodes", "posterior", "state"]
        assert sorted(conf_kept.files) == ["alphabet", "confidence", "nodes", "state"]
        assert [str(v) for v in conf["nodes"]] == names and [str(a) for a in conf["alphabet"]] == AA
        state, confidence, posterior = conf["state"], conf["confidence"], conf["posterior"]
        n_sites = len(next(iter(msa.values())))
        assert state.dtype == np.int8 and state.shape == confidence.shape == (len(names), n_sites)
        assert posterior.shape == (len(names), n_sites, 20)
        assert np.array_equal(conf_kept["state"], state) and np.array_equal(conf_kept["confidence"], confidence)
        assert np.all(state >= 0) and np.all(confidence > 0.0) and np.all(confidence <= 1.0)
        assert np.abs(posterior.sum(axis=2) - 1.0).max() <= 1e-12
        assert np.array_equal(confidence, np.take_along_axis(posterior, state.astype(np.int64)[:, :, None], axis=2)[:, :, 0])
        for i, v in enumerate(names):
            assert len(seqs[i]) == len(seqs_kept[i]) == n_sites
            assert seqs[i] == "".join(AA[k] for k in state[i])                # letters = alphabet[state]
            if tree.is_leaf(v):
                for a, b, c in zip(msa[v], seqs[i], seqs_kept[i]):
                    if a in AA:
                        assert a == b == c                                    # observed leaf characters unchanged
                    else:
                        assert b in AA and c == "-"                           # imputed, or kept a gap
                        gaps += 1
            else:
                assert seqs_kept[i] == seqs[i]
        prof = open(os.path.join(out["output_msa_dir"], fam + ".profiling")).read()
        assert prof.split("\n")[-1].startswith("total_time: ") and "reconstruction_kernel_ms: " in prof
        print(f"{fam}: {len(names)} nodes x {n_sites} sites, mean confidence at internal nodes "
              f"{confidence[[not tree.is_leaf(v) for v in names]].mean():.4f}")
    assert gaps > 0
