"""The site-rate scan without a GPU: the NumPy restatement against brute-force enumeration, its pick rule, the margins of the
GPU cases, the restated alternating stage, the entry point's validation (on the host before any device work), the loud failure
with no GPU, and the new kernels' resources."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

import bl_reference  # noqa: E402
import sr_cases  # noqa: E402
import sr_reference  # noqa: E402
from cherryml_amd import _lib  # noqa: E402
from test_em_cpu import GRID, TREES, _random_Q  # noqa: E402

MARGIN = 1e-9   # the rule of sections 15 and 16 (tests/test_gpu_nj.py, tests/test_gpu_bl.py)


@pytest.mark.parametrize("n_int", [3, 4])
def test_restatement_equals_brute_force(n_int):
    """S = 4, three and four internal nodes (one of them multifurcating); the bar of tests/test_bl_cpu.py"""
    parent, length = TREES[n_int]
    S, L = 4, 6
    rng = np.random.default_rng(40 + n_int)
    codes = rng.integers(0, S, (len(parent), L)).astype(np.int8)
    codes[rng.random(codes.shape) < 0.25] = -1
    codes[:, 0] = -1                                     # an all-gap site
    Q, pi = _random_Q(S, 7)
    cands = [0.07, 0.5, 1.0, 2.3]
    r = sr_reference.scan(parent, length, codes, cands, Q, pi)
    for c, rate in enumerate(cands):
        assert np.max(np.abs(r["ll"][c] - sr_reference.brute_force(parent, length, codes, rate, Q, pi))) < 1e-12
    assert np.all(np.abs(r["ll"][:, 0]) < 1e-12)          # no observation: probability one at every rate
    decided = r["n_obs"] >= 2
    assert decided.sum() >= 3
    assert np.array_equal(r["best"][decided], np.argmax(r["ll"], axis=0)[decided]) and np.all(r["best"][~decided] == 0)
    assert np.array_equal(r["best_ll"], r["ll"][r["best"], np.arange(L)])


def test_the_pick_rule():
    inf = np.inf
    ll = np.array([[-3.0, -2.0, -2.0, -inf, -5.0, -1.0],
                   [-1.0, -2.0, -2.0, -inf, -4.0, -9.0],
                   [-1.0, -2.5, -2.0, -inf, -4.5, -9.0]])
    n_obs = np.array([2, 3, 2, 2, 1, 0])
    best, margin = sr_reference.pick(ll, n_obs)
    assert best.tolist() == [1, 0, 0, 0, 0, 0]            # the lowest index among exact maxima; sites 4, 5: the codes decide
    assert margin[0] == 0.0 and margin[1] == 0.0 and np.all(np.isinf(margin[4:]))
    best, _ = sr_reference.pick(ll, n_obs, current=[2, 2, 2, 1, 2, -1])
    assert best.tolist() == [2, 0, 2, 1, 2, 0]            # current wins only where it is an exact maximum (-inf everywhere too)
    best, margin = sr_reference.pick(ll[:1], n_obs)
    assert best.tolist() == [0] * 6 and np.all(np.isinf(margin))


@pytest.mark.parametrize("name", sr_cases.CASES)
def test_the_restatement_decides_every_site_of_the_gpu_cases(name):
    """the cases of tests/test_gpu_sr.py are compared on integers wherever a site has two or more observed leaves: their seeds
    are chosen so that every such site has a margin above 1e-9 (none is left out)"""
    S, fams, current = sr_cases.case(name)
    for k, r in enumerate(sr_cases.restated(name)):
        decided = r["n_obs"] >= 2
        print(f"{name}[{k}]: {decided.sum()} of {decided.size} sites decided by the likelihoods, smallest margin "
              f"{r['margin'][decided].min() if decided.any() else np.inf:.2e}")
        assert np.all(r["margin"][decided] > MARGIN), r["margin"]
        assert np.all(np.isfinite(r["ll"]))
        if decided.size >= 7:
            assert not decided[0] and not decided[1] and r["n_obs"][0] == 0 and r["n_obs"][1] == 1
            want = 0 if current is None else max(int(current[k][1]), 0)
            assert r["best"][1] == want and r["best"][0] == 0
    assert sum(int((r["n_obs"] >= 2).sum()) for r in sr_cases.restated(name)) >= 1


def test_the_restated_stage_never_lowers_a_likelihood_and_a_fixed_point_stays():
    parent, length = TREES[4]
    S, L = 4, 40
    rng = np.random.default_rng(17)
    Q, pi = _random_Q(S, 3)
    cands = np.array([0.3, 0.8, 1.5, 3.0])
    grid = GRID[30:100:3]
    true = rng.integers(0, len(cands), L)
    tau_true = np.where(parent >= 0, rng.integers(8, 20, len(parent)), -1)
    import bl_cases
    codes = bl_cases.simulate(parent, tau_true, cands[true], grid, Q, pi, rng, gap_fraction=0.1)
    tau0 = bl_reference.snap(length, parent, grid)
    index0 = np.full(L, 1)
    tau, index, trace = sr_reference.alternate(parent, tau0, codes, index0, cands, grid, Q, pi, n_outer=30, n_rounds=5)
    trace = np.array(trace)
    print("log-likelihoods (start of the fit, before the pick, after it) per outer iteration:\n", trace.reshape(-1, 3))
    assert len(trace) >= 6 and trace[-1] > trace[0]                      # the stage moved
    assert np.all(np.diff(trace) >= -1e-12 * np.abs(trace[:-1])), trace  # neither half goes down
    assert not np.array_equal(index, index0) and not np.array_equal(tau, tau0)
    tau2, index2, trace2 = sr_reference.alternate(parent, tau, codes, index, cands, grid, Q, pi, n_outer=30, n_rounds=5)
    assert np.array_equal(tau2, tau) and np.array_equal(index2, index) and len(trace2) == 3   # one outer iteration: nothing moves
    assert np.all(np.abs(np.array(trace2) - trace[-1]) <= 1e-12 * abs(trace[-1]))


# ------------------------------------------------------------------------------- validation before any device work
def _call(S=20, n_fam=1, parent=None, length=None, codes=None, cands=None, current=None, Q=None, pi=None, n_cands=None, null=None):
    parent = np.ascontiguousarray(TREES[3][0] if parent is None else parent, dtype=np.int32)
    length = np.ascontiguousarray(TREES[3][1] if length is None else length, dtype=np.float64)
    cands = np.ascontiguousarray([0.5, 1.0, 2.0] if cands is None else cands, dtype=np.float64)
    codes = np.ascontiguousarray(np.zeros((len(parent), 2)) if codes is None else codes, dtype=np.int8)
    U = codes.shape[1]
    Q0, pi0 = _random_Q(min(max(S, 2), 32), 1)
    Q = np.ascontiguousarray(Q0 if Q is None else Q, dtype=np.float64)
    pi = np.ascontiguousarray(pi0 if pi is None else pi, dtype=np.float64)
    cur = None if current is None else np.ascontiguousarray(current, dtype=np.int32)
    nn, nu = np.array([len(parent)], np.int32), np.array([U], np.int32)
    nc = np.array([len(cands) if n_cands is None else n_cands], np.int32)
    best, best_ll = np.zeros(U, np.int32), np.zeros(U)
    args = dict(Q=Q.ctypes.data, pi=pi.ctypes.data, nn=nn.ctypes.data, parent=parent.ctypes.data, length=length.ctypes.data,
                nu=nu.ctypes.data, codes=codes.ctypes.data, nc=nc.ctypes.data, cands=cands.ctypes.data,
                cur=None if cur is None else cur.ctypes.data, best=best.ctypes.data, best_ll=best_ll.ctypes.data)
    if null:
        args[null] = None
    rc = _lib.load().cb_tree_site_rates(0, S, args["Q"], args["pi"], n_fam, args["nn"], args["parent"], args["length"], args["nu"],
                                        args["codes"], args["nc"], args["cands"], args["cur"], args["best"], args["best_ll"], None,
                                        None)
    return rc, (_lib.load().cb_last_error() or b"").decode()


def _bad_Q(i, j, x):
    Q, _ = _random_Q(20, 1)
    Q[i, j] = x
    return Q


@pytest.mark.parametrize("kw,match", [
    (dict(null="Q"), "NULL argument"),
    (dict(null="cands"), "NULL argument"),
    (dict(null="best_ll"), "NULL argument"),
    (dict(S=33), "S = 33"),
    (dict(S=1), "S = 1"),
    (dict(n_fam=0), "families = 0"),
    (dict(n_cands=0), "0 candidates"),
    (dict(cands=np.linspace(0.1, 3.0, 65)), "65 candidates"),
    (dict(cands=[0.5, 0.5, 2.0]), "strictly increasing (candidate 1 = 0.5)"),
    (dict(cands=[0.5, 0.4, 2.0]), "strictly increasing (candidate 1 = 0.4)"),
    (dict(cands=[0.0, 0.4, 2.0]), "positive, finite and strictly increasing (candidate 0 = 0)"),
    (dict(cands=[-1.0, 0.4, 2.0]), "candidate 0 = -1"),
    (dict(cands=[0.5, 1.0, np.inf]), "candidate 2 = inf"),
    (dict(cands=[0.5, np.nan, 2.0]), "candidate 1 = nan"),
    (dict(current=[0, 3]), "current[1] = 3"),
    (dict(current=[-2, 0]), "current[0] = -2"),
    (dict(codes=np.full((7, 2), 20)), "state code 20 out of range"),
    (dict(codes=np.full((7, 2), -2)), "state code -2 out of range"),
    (dict(length=[0.0, 0.1, -0.4, 0.05, 0.9, 0.23, 0.031]), "length[2] = -0.4"),
    (dict(length=[0.0, 0.1, 0.4, np.nan, 0.9, 0.23, 0.031]), "length[3] = nan"),
    (dict(length=[0.0, 0.1, 0.4, 0.3, np.inf, 0.23, 0.031]), "length[4] = inf"),
    (dict(parent=[-1, 0, 0, 1, 1, 2, -1]), "two roots (0 and 6)"),
    (dict(parent=[1, 0, 0, 1, 1, 2, 2]), "no root"),
    (dict(parent=[-1, 2, 1, 1, 1, 2, 2]), "not a tree"),
    (dict(parent=[-1, 0, 0, 1, 1, 2, 9]), "parent[6] = 9"),
    (dict(Q=_bad_Q(2, 5, -0.1)), "Q[2][5] = -0.1"),
    (dict(Q=_bad_Q(3, 3, np.nan)), "Q[3][3] = nan"),
    (dict(pi=np.r_[-0.1, np.ones(19)]), "pi_root[0] = -0.1"),
    (dict(pi=np.zeros(20)), "pi_root sums to 0"),
])
def test_cb_tree_site_rates_validates_before_any_device_work(kw, match):
    """CB_EINVAL with the value named -- also on a machine with no GPU, where any device work would have given CB_EHIP first"""
    rc, msg = _call(**kw)
    assert rc == _lib.CB_EINVAL, (rc, msg)
    assert "cb_tree_site_rates" in msg and match in msg, msg


def test_sixty_four_candidates_are_accepted_and_the_root_length_is_ignored():
    rc, msg = _call(cands=np.linspace(0.1, 3.0, 64), current=[63, -1])
    assert rc != _lib.CB_EINVAL, msg
    rc, msg = _call(length=[np.nan, 0.1, 0.4, 0.05, 0.9, 0.23, 0.031])
    assert rc != _lib.CB_EINVAL, msg


def _star():
    from cherryml_amd.io import Tree
    t = Tree()
    t.add_nodes(["r", "a", "b"])
    t.add_edges([("r", "a", 0.1), ("r", "b", 0.2)])
    return t


def test_tree_site_rates_validates_in_python_before_it_loads_the_library(monkeypatch):
    from cherryml_amd.phylogeny_estimation import _site_rates
    called = []
    monkeypatch.setattr(_site_rates, "_scan", lambda *a: called.append(1))
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    Q, pi = _random_Q(20, 1)
    codes = np.zeros((3, 4), np.int8)
    with pytest.raises(ValueError, match="codes must be"):
        _site_rates.tree_site_rates([_star()], [np.zeros((2, 4), np.int8)], [0.5, 1.0], None, Q, pi, device=0)
    with pytest.raises(ValueError, match="one tree"):
        _site_rates.tree_site_rates([], [], [0.5, 1.0], None, Q, pi, device=0)
    with pytest.raises(ValueError, match="one tree"):
        _site_rates.tree_site_rates([_star()], [codes], [0.5, 1.0], [], Q, pi, device=0)
    with pytest.raises(ValueError, match="Q must be square"):
        _site_rates.tree_site_rates([_star()], [codes], [0.5, 1.0], None, Q, pi[:5], device=0)
    with pytest.raises(ValueError, match="no candidates"):
        _site_rates.tree_site_rates([_star()], [codes], [], None, Q, pi, device=0)
    with pytest.raises(ValueError, match="2 candidate lists for 1 families"):
        _site_rates.tree_site_rates([_star()], [codes], [[0.5], [1.0]], None, Q, pi, device=0)
    with pytest.raises(ValueError, match="current must be"):
        _site_rates.tree_site_rates([_star()], [codes], [0.5, 1.0], [np.zeros(3, np.int32)], Q, pi, device=0)
    with pytest.raises(ValueError, match="current must be"):
        _site_rates.tree_site_rates([_star()], [codes], [0.5, 1.0], [np.zeros(4)], Q, pi, device=0)
    assert not called


def test_the_union_of_candidates_is_sorted_distinct_and_bounded():
    from cherryml_amd.phylogeny_estimation import rate_categories_ble
    from cherryml_amd.phylogeny_estimation._site_rates import _candidates
    offered = rate_categories_ble(4)
    c = _candidates(4, np.array([offered[1], 0.9, 0.9, 7.0]), "f")
    assert np.array_equal(c, np.unique(offered + [0.9, 7.0])) and c.size == 6
    assert _candidates(32, np.linspace(0.011, 0.3, 32), "f").size == 64          # R <= 32 offered + R of the input: at most 64
    with pytest.raises(ValueError, match="65 candidates"):
        _candidates(32, np.linspace(0.011, 0.3, 33), "f")


def test_no_gpu_means_the_scan_fails_loudly(tmp_path):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    rc, msg = _call()
    assert rc == _lib.CB_EHIP and "no HIP device" in msg, (rc, msg)
    from cherryml_amd import ml_lengths_and_site_rates, ml_site_rates, nj_ml_rates_trees, tree_site_rates
    Q, pi = _random_Q(20, 1)
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        tree_site_rates([_star()], [np.zeros((3, 4), np.int8)], [0.5, 1.0], None, Q, pi, device=0)
    dirs = dict(tree_dir="t", msa_dir="m", site_rates_dir="s", families=["f"], rate_matrix_path="q", num_rate_categories=4,
                output_site_rates_dir=str(tmp_path / "s"), output_likelihood_dir=str(tmp_path / "l"))
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        ml_site_rates(**dirs)
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        ml_lengths_and_site_rates(output_tree_dir=str(tmp_path / "t"), **dirs)
    assert callable(nj_ml_rates_trees)


# ---------------------------------------------------------------------------------------------------------- resources
def test_sr_kernels_have_no_scratch_and_no_vgpr_spills():
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if k.startswith("sr_")}
    assert {"sr_scan_kernel", "sr_pick_kernel"} <= {k.split("(")[0] for k in hits}, hits
    for name, m in hits.items():
        print(name, m)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)
