"""Branch-length EM without a GPU: the NumPy restatement of a round against brute-force enumeration and its monotonicity, the
handle's validation (on the host before any device work), the loud failure with no GPU, and the new kernels' resources."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

import bl_reference  # noqa: E402
from cherryml_amd import _lib  # noqa: E402
from test_em_cpu import GRID, TREES, _random_Q  # noqa: E402


@pytest.mark.parametrize("S,n_int", [(4, 3), (4, 4), (20, 3)])
def test_restatement_equals_brute_force(S, n_int):
    parent, length = TREES[n_int]
    rng = np.random.default_rng(S + n_int)
    L = 6
    codes = rng.integers(0, S, (len(parent), L)).astype(np.int8)
    codes[rng.random(codes.shape) < 0.25] = -1            # gaps
    rates = np.array([0.5, 1.0, 2.3, 0.5, 1.0, 0.07])[:L]  # several categories
    Q, pi = _random_Q(S, 7)
    tau = bl_reference.snap(length, parent, GRID)
    r = bl_reference.em_round(parent, tau, codes, rates, GRID, Q, pi)
    E2, ll2 = bl_reference.brute_force(parent, tau, codes, rates, GRID, Q, pi)
    assert np.max(np.abs(r["ll"] - ll2)) < 1e-12
    assert set(r["E"]) == set(E2)
    big = max(1.0, max(np.abs(e).max() for e in E2.values()))
    assert max(np.abs(r["E"][k] - E2[k]).max() for k in E2) < 1e-12 * big
    mass = sum(e.sum() for e in r["E"].values())
    assert abs(mass - (len(parent) - 1) * L) < 1e-10 * mass


def test_rounds_of_the_restatement_never_lower_a_likelihood_and_a_fixed_point_stays():
    parent, length = TREES[4]
    S, L = 4, 60
    rng = np.random.default_rng(11)
    codes = rng.integers(0, S, (len(parent), L)).astype(np.int8)
    codes[rng.random(codes.shape) < 0.1] = -1
    rates = rng.choice([0.3, 0.8, 1.5, 3.0], L)
    Q, pi = _random_Q(S, 3)
    P = bl_reference.bank(GRID, np.unique(rates), Q)
    tau = bl_reference.snap(length, parent, GRID)
    lls, fixed = [], None
    for k in range(200):
        r = bl_reference.em_round(parent, tau, codes, rates, GRID, Q, pi, P=P)
        lls.append(r["ll"].sum())
        if np.array_equal(r["tau"], tau):
            fixed = k
            break
        tau = r["tau"]
    lls = np.array(lls)
    assert len(lls) >= 3, lls                                   # the start is no fixed point: the rounds moved
    assert np.all(np.diff(lls[:11]) >= -1e-12 * np.abs(lls[:10])), lls   # ten rounds (and every later one) never go down
    assert np.all(np.diff(lls) >= -1e-12 * np.abs(lls[:-1])), lls
    assert fixed is not None, "no fixed point within 200 rounds"
    again = bl_reference.em_round(parent, tau, codes, rates, GRID, Q, pi, P=P)
    assert np.array_equal(again["tau"], tau) and again["ll"].sum() == lls[-1]


@pytest.mark.parametrize("name", ["s4", "s20", "s32", "s20one"])
def test_the_restatement_decides_every_edge_of_the_gpu_cases(name):
    """the cases of tests/test_gpu_bl.py are compared on integers wherever the restatement's margin exceeds 1e-9: their seeds are
    chosen so that this is every edge"""
    import bl_cases
    for tau, r in bl_cases.restated(name):
        edges = tau >= 0
        assert edges.sum() >= 3 and np.all(r["margin"][edges] > 1e-9), r["margin"]


# ------------------------------------------------------------------------------- validation before any device work
def _create(S=20, grid=None, parent=None, length=None, rates=None, codes=None, Q=None, pi=None):
    grid = np.ascontiguousarray(GRID if grid is None else grid, dtype=np.float64)
    parent = np.ascontiguousarray(TREES[3][0] if parent is None else parent, dtype=np.int32)
    length = np.ascontiguousarray(TREES[3][1] if length is None else length, dtype=np.float64)
    rates = np.ascontiguousarray([1.0, 0.5] if rates is None else rates, dtype=np.float64)
    codes = np.ascontiguousarray(np.zeros((len(parent), len(rates))) if codes is None else codes, dtype=np.int8)
    Q0, pi0 = _random_Q(min(max(S, 2), 32), 1)
    Q = np.ascontiguousarray(Q0 if Q is None else Q, dtype=np.float64)
    pi = np.ascontiguousarray(pi0 if pi is None else pi, dtype=np.float64)
    h = ctypes.c_void_p()
    nn, nu = np.array([len(parent)], np.int32), np.array([len(rates)], np.int32)
    rc = _lib.load().cb_bl_create(0, S, len(grid), grid.ctypes.data, Q.ctypes.data, pi.ctypes.data, 1, nn.ctypes.data,
                                  parent.ctypes.data, length.ctypes.data, nu.ctypes.data, rates.ctypes.data, codes.ctypes.data,
                                  ctypes.byref(h))
    if rc == 0:
        _lib.load().cb_bl_destroy(h)
    return rc, (_lib.load().cb_last_error() or b"").decode()


def _bad_Q(i, j, x):
    Q, _ = _random_Q(20, 1)
    Q[i, j] = x
    return Q


@pytest.mark.parametrize("kw,match", [
    (dict(S=33), "S = 33"),
    (dict(S=1), "S = 1"),
    (dict(grid=[0.1]), "T = 1"),
    (dict(grid=[0.1, 0.05, 0.2]), "strictly increasing (grid[1] = 0.05)"),
    (dict(grid=[0.0, 0.05, 0.2]), "positive and strictly increasing (grid[0] = 0)"),
    (dict(rates=[1.0, -0.5]), "site rate 1 = -0.5"),
    (dict(rates=[0.0, 1.0]), "site rate 0 = 0"),
    (dict(rates=[1.0, np.inf]), "site rate 1 = inf"),
    (dict(rates=[np.nan, 1.0]), "site rate 0 = nan"),
    (dict(rates=np.linspace(0.1, 3.0, 65), codes=np.zeros((7, 65))), "65 distinct site rates"),
    (dict(codes=np.full((7, 2), 20)), "state code 20 out of range"),
    (dict(codes=np.full((7, 2), -2)), "state code -2 out of range"),
    (dict(parent=[-1, 0, 0, 1, 1, 2, -1]), "two roots (0 and 6)"),
    (dict(parent=[1, 0, 0, 1, 1, 2, 2]), "no root"),
    (dict(parent=[-1, 2, 1, 1, 1, 2, 2]), "not a tree"),
    (dict(parent=[-1, 0, 0, 1, 1, 2, 9]), "parent[6] = 9"),
    (dict(length=[0.0, 0.1, -0.4, 0.05, 0.9, 0.23, 0.031]), "length[2] = -0.4"),
    (dict(length=[0.0, 0.1, 0.4, np.nan, 0.9, 0.23, 0.031]), "length[3] = nan"),
    (dict(Q=_bad_Q(2, 5, -0.1)), "Q[2][5] = -0.1"),
    (dict(Q=_bad_Q(3, 3, np.nan)), "Q[3][3] = nan"),
    (dict(pi=np.r_[-0.1, np.ones(19)]), "pi_root[0] = -0.1"),
    (dict(pi=np.zeros(20)), "pi_root sums to 0"),
])
def test_cb_bl_create_validates_before_any_device_work(kw, match):
    """CB_EINVAL with the value named -- also on a machine with no GPU, where any device work would have given CB_EHIP first"""
    rc, msg = _create(**kw)
    assert rc == _lib.CB_EINVAL, (rc, msg)
    assert "cb_bl_create" in msg and match in msg, msg


def test_sixty_four_distinct_rates_are_accepted():
    rc, msg = _create(rates=np.linspace(0.1, 3.0, 64), codes=np.zeros((7, 64)))
    assert rc != _lib.CB_EINVAL, msg


def _star():
    from cherryml_amd.io import Tree
    t = Tree()
    t.add_nodes(["r", "a", "b"])
    t.add_edges([("r", "a", 0.1), ("r", "b", 0.2)])
    return t


def test_the_fitter_validates_in_python_before_any_device_work(monkeypatch):
    from cherryml_amd.phylogeny_estimation import _ml_lengths
    called = []
    monkeypatch.setattr(_ml_lengths.BranchLengthFitter, "_create", lambda self: called.append(1))
    Q, pi = _random_Q(20, 1)
    with pytest.raises(ValueError, match="codes must be"):
        _ml_lengths.BranchLengthFitter([_star()], [np.zeros((3, 4), np.int8)], [np.ones(5)], GRID, Q, pi)
    with pytest.raises(ValueError, match="one tree"):
        _ml_lengths.BranchLengthFitter([], [], [], GRID, Q, pi)
    with pytest.raises(ValueError, match="Q must be square"):
        _ml_lengths.BranchLengthFitter([_star()], [np.zeros((3, 4), np.int8)], [np.ones(4)], GRID, Q, pi[:5])
    assert not called


def test_no_gpu_means_the_fit_fails_loudly(tmp_path):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    rc, msg = _create()
    assert rc == _lib.CB_EHIP and "no HIP device" in msg, (rc, msg)
    from cherryml_amd import BranchLengthFitter, ml_branch_lengths
    Q, pi = _random_Q(20, 1)
    with pytest.raises(_lib.CherryBankError):
        BranchLengthFitter([_star()], [np.zeros((3, 4), np.int8)], [np.ones(4)], GRID, Q, pi)
    with pytest.raises(_lib.CherryBankError):
        ml_branch_lengths(tree_dir="t", msa_dir="m", site_rates_dir="s", families=["f"], rate_matrix_path="q",
                          output_tree_dir=str(tmp_path / "t"), output_likelihood_dir=str(tmp_path / "l"))


def test_the_batches_keep_the_family_order_and_the_bound():
    from cherryml_amd.phylogeny_estimation._ml_lengths import _batches
    assert _batches([3, 3, 3, 9, 1, 1], 6) == [[0, 1], [2], [3], [4, 5]]
    assert _batches([1, 1], 100) == [[0, 1]]


# ---------------------------------------------------------------------------------------------------------- resources
def test_bl_kernels_have_no_scratch_and_no_vgpr_spills():
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if k.startswith("bl_")}
    assert {"bl_log_kernel", "bl_mstep_kernel"} <= {k.split("(")[0] for k in hits}, hits
    for name, m in hits.items():
        print(name, m)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)
