"""Full-tree EM without a GPU: the NumPy restatement against brute-force enumeration, the E-step's validation (raised on the
host before any device work), the loud failure with no GPU, the EM pipeline's backend check, and the new kernels' resources."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

import em_reference  # noqa: E402
from cherryml_amd import _lib  # noqa: E402

GRID = [0.03 * 1.1 ** i for i in range(-64, 65)]


def _random_Q(S, seed):
    rng = np.random.default_rng(seed)
    pi = rng.dirichlet(np.ones(S))
    R = rng.uniform(0.2, 2.0, (S, S))
    R = (R + R.T) / 2
    Q = R * pi[None, :]
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q / -np.dot(pi, np.diag(Q)), pi


# two small trees: 3 and 4 internal nodes (node 0 the root)
TREES = {
    3: (np.array([-1, 0, 0, 1, 1, 2, 2]), np.array([0.0, 0.11, 0.4, 0.05, 0.9, 0.23, 0.031])),
    4: (np.array([-1, 0, 0, 0, 1, 1, 2, 2, 3, 3, 3]), np.array([0.0, 0.2, 0.07, 0.5, 0.3, 0.012, 1.3, 0.08, 0.15, 0.6, 0.04])),
}


@pytest.mark.parametrize("S,n_int", [(4, 3), (4, 4), (20, 3)])
def test_restatement_equals_brute_force(S, n_int):
    parent, length = TREES[n_int]
    rng = np.random.default_rng(S + n_int)
    L = 6
    codes = rng.integers(0, S, (len(parent), L)).astype(np.int8)
    codes[rng.random(codes.shape) < 0.25] = -1            # gaps
    rates = np.array([0.5, 1.0, 2.3, 0.5, 1.0, 0.0])[:L]  # several categories, one of them rate 0
    Q, pi = _random_Q(S, 7)
    E1, ll1 = em_reference.estep(parent, length, codes, rates, GRID, Q, pi)
    E2, ll2 = em_reference.estep_brute_force(parent, length, codes, rates, GRID, Q, pi)
    assert np.max(np.abs(ll1 - ll2)) < 1e-12
    assert np.max(np.abs(E1 - E2)) < 1e-12 * max(1.0, np.abs(E2).max())
    assert abs(E1.sum() - (len(parent) - 1) * L) < 1e-10 * E1.sum()


def test_quantize_takes_the_nearest_point_in_ratio_and_clamps():
    g = np.array(GRID)
    assert em_reference.quantize(0.03, g) == 64
    assert em_reference.quantize(0.03 * 1.1 ** 0.49, g) == 64 and em_reference.quantize(0.03 * 1.1 ** 0.51, g) == 65
    assert em_reference.quantize(0.0, g) == 0 and em_reference.quantize(1e6, g) == len(g) - 1


# ------------------------------------------------------------------------------- validation before any device work
def _create(S=20, grid=None, parent=None, length=None, rates=None, codes=None):
    grid = np.ascontiguousarray(GRID if grid is None else grid, dtype=np.float64)
    parent = np.ascontiguousarray(TREES[3][0] if parent is None else parent, dtype=np.int32)
    length = np.ascontiguousarray(TREES[3][1] if length is None else length, dtype=np.float64)
    rates = np.ascontiguousarray([1.0, 0.5] if rates is None else rates, dtype=np.float64)
    codes = np.ascontiguousarray(np.zeros((len(parent), len(rates))) if codes is None else codes, dtype=np.int8)
    h = ctypes.c_void_p()
    nn, nu = np.array([len(parent)], np.int32), np.array([len(rates)], np.int32)
    rc = _lib.load().cb_em_create(0, S, len(grid), grid.ctypes.data, 1, nn.ctypes.data, parent.ctypes.data, length.ctypes.data,
                                  nu.ctypes.data, rates.ctypes.data, codes.ctypes.data, ctypes.byref(h))
    if rc == 0:
        _lib.load().cb_em_destroy(h)
    return rc, (_lib.load().cb_last_error() or b"").decode()


@pytest.mark.parametrize("kw,match", [
    (dict(S=33), "S = 33"),
    (dict(S=1), "S = 1"),
    (dict(grid=[0.1, 0.05, 0.2]), "strictly increasing"),
    (dict(grid=[0.0, 0.05, 0.2]), "positive"),
    (dict(rates=[1.0, -0.5]), "site rate"),
    (dict(codes=np.full((7, 2), 20)), "out of range"),
    (dict(codes=np.full((7, 2), -2)), "out of range"),
    (dict(parent=[-1, 0, 0, 1, 1, 2, -1]), "two roots"),
    (dict(parent=[1, 0, 0, 1, 1, 2, 2]), "no root"),
    (dict(parent=[-1, 2, 1, 1, 1, 2, 2]), "not a tree"),
    (dict(parent=[-1, 0, 0, 1, 1, 2, 9]), "parent"),
    (dict(length=[0.0, 0.1, -0.4, 0.05, 0.9, 0.23, 0.031]), "length"),
])
def test_cb_em_create_validates_before_any_device_work(kw, match):
    rc, msg = _create(**kw)
    assert rc == _lib.CB_EINVAL, (rc, msg)
    assert match in msg, msg


def test_internal_rows_are_not_validated():
    codes = np.zeros((7, 2))
    codes[0:3] = 99                          # internal rows (nodes 0, 1, 2) are ignored
    rc, msg = _create(codes=codes)
    assert rc != _lib.CB_EINVAL, msg


def test_estep_validates_in_python_before_any_device_work(monkeypatch):
    from cherryml_amd.estimation import _em
    from cherryml_amd.io import Tree
    called = []
    monkeypatch.setattr(_em.EStep, "_create", lambda self, S: called.append(S))
    t = Tree()
    t.add_nodes(["r", "a", "b"])
    t.add_edges([("r", "a", 0.1), ("r", "b", 0.2)])
    with pytest.raises(ValueError, match="codes must be"):
        _em.EStep([t], [np.zeros((3, 4), np.int8)], [np.ones(5)], GRID)
    with pytest.raises(ValueError, match="one tree"):
        _em.EStep([], [], [], GRID)
    assert not called


def test_no_gpu_means_the_estep_fails_loudly():
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    rc, msg = _create()
    assert rc == _lib.CB_EHIP and "no HIP device" in msg, (rc, msg)
    from cherryml_amd.estimation import EStep
    from cherryml_amd.io import Tree
    t = Tree()
    t.add_nodes(["r", "a", "b"])
    t.add_edges([("r", "a", 0.1), ("r", "b", 0.2)])
    with pytest.raises(_lib.CherryBankError):
        EStep([t], [np.zeros((3, 4), np.int8)], [np.ones(4)], GRID)


def test_the_root_distribution_is_read_in_the_rate_matrix_order(tmp_path):
    from cherryml_amd.estimation._em import _root_distribution
    from cherryml_amd.io import write_probability_distribution
    states = list("ARND")
    p = np.array([0.1, 0.2, 0.3, 0.4])
    path = str(tmp_path / "pi.txt")
    write_probability_distribution(p[::-1], states[::-1], path)     # the file lists the states in another order
    assert np.array_equal(_root_distribution(path, states), p)
    with pytest.raises(ValueError, match="not the rate matrix's"):
        _root_distribution(path, list("ARNC"))


@pytest.mark.parametrize("backend", ["xrate", "historian"])
def test_the_pipeline_refuses_the_external_backends(backend):
    from cherryml_amd import lg_end_to_end_with_em_optimizer
    with pytest.raises(ValueError, match="XRATE / Historian binaries"):
        lg_end_to_end_with_em_optimizer(msa_dir="x", families=["f"], tree_estimator=None,
                                        initial_tree_estimator_rate_matrix_path=None, em_backend=backend)


def test_em_lg_takes_no_historian_flags():
    from cherryml_amd import em_lg
    with pytest.raises(TypeError):
        em_lg(tree_dir="t", msa_dir="m", site_rates_dir="s", families=["f"], initialization_rate_matrix_path="q",
              output_rate_matrix_dir="o", extra_command_line_args="-band 0")


# ---------------------------------------------------------------------------------------------------------- resources
def test_em_kernels_have_no_scratch_and_no_spills():
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if k.startswith("em_")}
    assert {"em_up_kernel", "em_down_kernel", "em_acc_kernel", "em_reduce_kernel"} <= {k.split("(")[0] for k in hits}, hits
    for name, m in hits.items():
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (name, m)
