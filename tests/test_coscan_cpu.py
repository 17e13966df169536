"""The co-evolution scan without a GPU: the NumPy restatement against a brute-force form through the counting oracle's count
tensor, the product model (score = 0), the average product correction, the header against the binding, the loud failure with no
GPU, and the new kernels' resources."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

import coscan_reference as cr  # noqa: E402
from cherryml_amd import _lib  # noqa: E402
from cherryml_amd.coevolution import _scan  # noqa: E402
from oracle import counting_oracle as co  # noqa: E402

# The product model Q_2 = Q_1 (x) I + I (x) Q_1 has score = 0 exactly; what is left is the two banks' rounding.  Measured on the
# restatement over PRODUCT_CASES, |score| / max(1, |pair_ll|) per site pair: 4.6e-15 with its Taylor expm, 7.04e-14 with its
# eigendecomposition (pi (x) pi has repeated eigenvalues).  The bar is ten times the larger and holds for the GPU's two paths too.
PRODUCT_MEASURED = 7.04e-14
PRODUCT_BAR = 10 * PRODUCT_MEASURED
PRODUCT_CASES = [(4, 5, 9, 12), (4, 5, 17, 70), (2, 5, 9, 12)]
assert PRODUCT_BAR <= 1e-9


def product_case(S, B, L, n):
    grid = np.exp(np.linspace(np.log(0.05), np.log(4.0), B))
    Q1, pi1 = cr.random_reversible(S, 3)
    codes, pairs = cr.random_family(S, L, n, grid, 11)
    return grid, Q1, pi1, cr.product_model(Q1), np.kron(pi1, pi1), codes, pairs


def _close(a, b, bar):
    return np.all(np.abs(a - b) <= bar * np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("S,L,n,symmetric,spectral", [(2, 5, 3, True, False), (3, 6, 7, True, True), (3, 6, 7, False, False),
                                                      (4, 4, 5, True, True)])
def test_restatement_equals_brute_force(S, L, n, symmetric, spectral):
    grid = np.array([0.05, 0.2, 0.8, 3.0])
    Q1, pi1 = cr.random_reversible(S, 5)
    Q2, pi2 = cr.random_reversible(S * S, 6)
    P1, P2 = cr.bank(Q1, grid, pi1 if spectral else None), cr.bank(Q2, grid, pi2 if spectral else None)
    assert P1.min() > 0 and P2.min() > 0
    codes, pairs = cr.random_family(S, L, n, grid, S + L)
    r = cr.scan(codes, pairs, grid, cr.log_bank(P1), cr.log_bank(P2), symmetric)
    b = cr.brute_force(codes, pairs, grid, cr.log_bank(P1), cr.log_bank(P2), symmetric, co.co_count_pair)
    for key in ("score", "pair_ll", "indep_ll"):
        assert _close(r[key], b[key], 1e-12), key
        assert np.array_equal(r[key], r[key].T) and np.all(np.diag(r[key]) == 0)
    assert np.array_equal(r["n_used"], b["n_used"])
    assert r["n_used"].max() > 0 and r["n_used"].max() <= n - (2 if n >= 3 else 0)   # the two off-grid pairs never count
    if L >= 3:
        assert np.all(r["n_used"][L // 2] == 0)                                      # the all-gap column


def test_the_two_expms_of_the_restatement_agree():
    Q, pi = cr.random_reversible(9, 2)
    grid = np.array([0.01, 0.3, 7.0])
    assert np.abs(cr.bank(Q, grid) - cr.bank(Q, grid, pi)).max() < 1e-13
    assert np.abs(cr.bank(Q, grid).sum(axis=2) - 1).max() < 1e-13


@pytest.mark.parametrize("S,B,L,n", PRODUCT_CASES)
@pytest.mark.parametrize("spectral", [False, True])
def test_the_product_model_scores_nothing(S, B, L, n, spectral):
    grid, Q1, pi1, Q2, pi2, codes, pairs = product_case(S, B, L, n)
    P1, P2 = cr.bank(Q1, grid, pi1 if spectral else None), cr.bank(Q2, grid, pi2 if spectral else None)
    assert P1.min() > 0 and P2.min() > 0
    r = cr.scan(codes, pairs, grid, cr.log_bank(P1), cr.log_bank(P2), True)
    rel = np.abs(r["score"]) / np.maximum(1.0, np.abs(r["pair_ll"]))
    print("product model: |score| / max(1, |pair_ll|) =", rel.max())
    assert np.abs(r["pair_ll"]).max() > 5
    assert rel.max() <= PRODUCT_BAR


def test_the_average_product_correction_follows_the_formula():
    rng = np.random.default_rng(1)
    for L in (1, 2, 7):
        s = rng.normal(0, 3, (L, L))
        s = s + s.T
        np.fill_diagonal(s, 0.0)
        got, want = _scan.average_product_correction(s), cr.apc(s)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert np.all(np.diag(got) == 0)
    z = np.zeros((4, 4))
    assert np.array_equal(_scan.average_product_correction(z), z)              # m == 0: apc = score
    s = np.array([[0.0, 1.0, -1.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    assert np.array_equal(_scan.average_product_correction(s), s)


def test_the_recovery_case_s_seed_and_tilt_decide_the_top_ten_on_the_cpu(tmp_path):
    """the seed-selection rule of the NNI search test: the GPU test compares sets, so the restatement's own decision must be clear"""
    z = cr.recovery_inputs(str(tmp_path))
    top, margin, _ = cr.recovery_restated(z)
    print("recovery: top ten", top, "relative gap to the best false pair", margin)
    assert sorted(top) == cr.RECOVERY_CONTACTS
    assert all(j - i >= cr.RECOVERY_MIN_DIST for i, j in cr.RECOVERY_CONTACTS) and len(cr.RECOVERY_CONTACTS) == 10
    assert margin > 1e-6 and abs(margin - cr.RECOVERY_MARGIN) < 1e-5


def test_the_header_declares_and_the_binding_lists_the_three_entry_points():
    header = open(os.path.join(ROOT, "include", "cherrybank.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int cb_coscan_create(int device, int S, int B, const double *grid, const double *Q1, const double *pi1, "
            "const double *Q2, const double *pi2, cb_coscan *out);") in flat
    assert ("int cb_coscan_run(cb_coscan h, int n_fam, const int *L, const int8_t *seqs, int64_t seqs_bytes, "
            "const cb_count_pair *pairs, const int64_t *n_pairs, int symmetric, double *score, double *pair_ll, "
            "double *indep_ll, int *n_used, double *kernel_ms);") in flat
    assert "int cb_coscan_destroy(cb_coscan h);" in flat
    import ctypes as C
    for name, n_args in (("cb_coscan_create", 9), ("cb_coscan_run", 13), ("cb_coscan_destroy", 1)):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args
        assert hasattr(_lib.load(), name)
    # by value: device, S, B; the family count, seqs_bytes (64 bits) and the mode
    assert _lib.SIGNATURES["cb_coscan_create"][1][:3] == [C.c_int] * 3
    run = _lib.SIGNATURES["cb_coscan_run"][1]
    assert (run[1], run[4], run[7]) == (C.c_int, C.c_int64, C.c_int)
    assert all(a is C.c_void_p for k, a in enumerate(run) if k not in (1, 4, 7))


def test_create_refuses_on_the_host_before_any_device_work():
    import ctypes
    Q1, _ = cr.random_reversible(4, 1)
    Q2, _ = cr.random_reversible(16, 1)
    grid = np.array([0.5, 0.25])
    h = ctypes.c_void_p()
    rc = _lib.load().cb_coscan_create(0, 4, 2, grid.ctypes.data, Q1.ctypes.data, None, Q2.ctypes.data, None, ctypes.byref(h))
    msg = _lib.load().cb_last_error().decode()
    assert rc == _lib.CB_EINVAL and "grid[1] = 0.25" in msg and not h.value, (rc, msg)
    rc = _lib.load().cb_coscan_create(0, 21, 2, grid.ctypes.data, Q1.ctypes.data, None, Q2.ctypes.data, None, ctypes.byref(h))
    assert rc == _lib.CB_EINVAL and "S = 21" in _lib.load().cb_last_error().decode()


def test_no_hip_device_means_the_scan_fails_loudly(tmp_path, monkeypatch):
    import cherryml_amd

    real = _lib.load()

    class NoDevice:
        def __getattr__(self, name):
            return getattr(real, name)

        def cb_device_count(self):
            return 0

    lib = NoDevice()
    monkeypatch.setattr(_scan._lib, "load", lambda: lib)
    Q1, _ = cr.random_reversible(4, 1)
    Q2, _ = cr.random_reversible(16, 1)
    with pytest.raises(_lib.CherryBankError, match="CoevolutionScanner: no HIP device"):
        cherryml_amd.CoevolutionScanner(Q1, Q2, [0.1, 1.0])
    with pytest.raises(_lib.CherryBankError, match="coevolution_scan: no HIP device"):
        cherryml_amd.coevolution_scan(tree_dir="t", msa_dir="m", families=["f"], amino_acids=list("ACGT"), rate_matrix_path="q",
                                      coevolution_rate_matrix_path="q2", quantization_points=[0.1, 1.0],
                                      output_scan_dir=str(tmp_path / "scan"))
    assert callable(cherryml_amd.read_coevolution_scan)


def test_the_library_itself_says_so_where_there_is_no_device():
    import ctypes
    if _lib.load().cb_device_count() > 0:
        return   # (with a device the message above cannot come from the library: tests/test_gpu_coscan.py runs it there)
    Q1, _ = cr.random_reversible(4, 1)
    Q2, _ = cr.random_reversible(16, 1)
    grid = np.array([0.25, 0.5])
    h = ctypes.c_void_p()
    rc = _lib.load().cb_coscan_create(0, 4, 2, grid.ctypes.data, Q1.ctypes.data, None, Q2.ctypes.data, None, ctypes.byref(h))
    msg = _lib.load().cb_last_error().decode()
    assert rc == _lib.CB_EHIP and "cb_coscan_create: no HIP device" in msg, (rc, msg)


def test_coscan_kernels_have_no_scratch_and_no_vgpr_spills():
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if "coscan_" in k}
    names = {k.split("(")[0].replace("void ", "") for k in hits}
    assert {"coscan_log_kernel", "coscan_kernel<true>", "coscan_kernel<false>"} <= names, hits
    for name, m in hits.items():
        print(name, m)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (name, m)
