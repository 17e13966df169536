"""Pin the oracle (oracle/ratelearn_oracle.py) against vectors produced by the
real reference (tests/golden/make_golden.py).  CPU only."""
import numpy as np
import pytest
import torch

from conftest import load_golden, relerr
from oracle import ratelearn_oracle as orc

EVAL_CASES = ["toy3_init", "toy3_mask", "s20_mask", "s20_symmask", "s400_mask"]


@pytest.mark.parametrize("case", EVAL_CASES)
def test_single_evaluation_f64(case):
    g = load_golden(f"eval_{case}.npz")
    if case == "s400_mask":
        torch.set_num_threads(8)
    r = orc.evaluate(g["upper_diag"], g["log_pi"], g["mask"], g["t"], g["C"], torch.float64)
    assert relerr(r["Q"], g["Q_f64"]) < 1e-14
    assert abs(r["loss"] - float(g["loss_f64"])) < 1e-13 * abs(float(g["loss_f64"]))
    assert relerr(r["dQ"], g["dQ_f64"]) < 1e-12
    assert relerr(r["d_upper"], g["d_upper_f64"]) < 1e-12
    assert relerr(r["d_log_pi"], g["d_log_pi_f64"]) < 1e-11


@pytest.mark.parametrize("case", EVAL_CASES[:4])
def test_single_evaluation_as_is_f32(case):
    g = load_golden(f"eval_{case}.npz")
    r = orc.evaluate(g["upper_diag"], g["log_pi"], g["mask"], g["t"], g["C"], torch.float32)
    assert relerr(r["Q"], g["Q_f32"]) < 1e-7
    assert abs(r["loss"] - float(g["loss_f32"])) < 1e-7 * abs(float(g["loss_f32"]))
    assert relerr(r["dQ"], g["dQ_f32"]) < 1e-5
    assert relerr(r["d_upper"], g["d_upper_f32"]) < 1e-5


def test_init_inversion_matches_reference_params():
    for case in ["toy3_init", "toy3_mask"]:
        g = load_golden(f"eval_{case}.npz")
        u, p = orc.invert_pande_reversible(g["init"], g["mask"])
        # the reference stores these in float32 parameters
        assert np.allclose(np.float32(p), g["log_pi"], rtol=0, atol=1e-6)
        fin = np.isfinite(g["upper_diag"])
        assert np.array_equal(np.isfinite(u), fin)
        assert np.allclose(np.float32(u[fin]), g["upper_diag"][fin], rtol=1e-6, atol=1e-6)


def test_mask_incompatible_initialisation_raises():
    g = load_golden("eval_toy3_init.npz")
    m = load_golden("eval_toy3_mask.npz")["mask"]
    with pytest.raises(ValueError):
        orc.invert_pande_reversible(g["init"], m)


@pytest.mark.parametrize("case", ["toy3_init", "toy3_mask", "s20_mask", "s20_symmask"])
def test_trajectory_f64(case):
    e = load_golden(f"eval_{case}.npz")
    g = load_golden(f"traj_{case}.npz")
    kw = dict(initialization=e["init"]) if "init" in e else dict(
        upper_diag=g["upper_diag0_f64"], log_pi=g["log_pi0_f64"])
    r = orc.train(e["t"], e["C"], e["mask"], num_epochs=int(g["num_epochs"]),
                  dtype=torch.float64, **kw)
    assert np.allclose(r["loss"], g["loss_f64"], rtol=1e-11, atol=0)
    for k in ["Q_best", "Q_last", "Q_1", "Q_2"]:
        assert relerr(r[k], g[k + "_f64"]) < 1e-9, k


@pytest.mark.parametrize("case", ["toy3_init", "toy3_mask"])
def test_trajectory_as_is_f32(case):
    """float32 mode reproduces `quantized_transitions_mle` as a user runs it
    (output files hold ~8 significant digits)."""
    e = load_golden(f"eval_{case}.npz")
    g = load_golden(f"traj_{case}.npz")
    r = orc.train(e["t"], e["C"], e["mask"], initialization=e["init"],
                  num_epochs=int(g["num_epochs"]), dtype=torch.float32)
    assert np.allclose(r["loss"], g["loss_f32"], rtol=2e-6, atol=0)
    assert relerr(r["Q_best"], g["Q_best_f32"]) < 1e-4
    assert relerr(r["result"], g["result_f32"]) < 1e-4


def test_trajectory_random_init_as_is_f32():
    """No initialisation: parameters come from torch.manual_seed(0) randn."""
    e = load_golden("eval_s20_mask.npz")
    g = load_golden("traj_s20_mask.npz")
    r = orc.train(e["t"], e["C"], e["mask"], num_epochs=int(g["num_epochs"]),
                  dtype=torch.float32)
    assert np.allclose(r["loss"], g["loss_f32"], rtol=5e-6, atol=0)
    assert relerr(r["Q_best"], g["Q_best_f32"]) < 1e-3


def test_trajectory_lg_bank_f64():
    g = load_golden("traj_lgbank.npz")
    r = orc.train(g["t"], g["C"], None, initialization=g["init"],
                  num_epochs=int(g["num_epochs"]), dtype=torch.float64)
    assert np.allclose(r["loss"], g["loss_f64"], rtol=1e-10, atol=0)
    assert relerr(r["Q_best"], g["Q_best_f64"]) < 1e-8
    # distance of the f64 recipe to the as-is float32 reference (reported, loose)
    assert relerr(r["Q_best"], g["Q_best_f32"]) < 1e-3


@pytest.mark.slow
def test_trajectory_s400_f64():
    torch.set_num_threads(8)
    e = load_golden("eval_s400_mask.npz")
    g = load_golden("traj_s400_mask.npz")
    r = orc.train(e["t"], e["C"], e["mask"], upper_diag=g["upper_diag0_f64"],
                  log_pi=g["log_pi0_f64"], num_epochs=3, dtype=torch.float64)
    assert np.allclose(r["loss"], g["loss_f64"], rtol=1e-11, atol=0)
    assert relerr(r["Q_best"], g["Q_best_f64"]) < 1e-9


def test_siterm_with_initialisation():
    for name in ["siterm_dna.npz", "siterm_aa.npz"]:
        g = load_golden(name)
        E = g["lpe_init"].shape[0]
        r = orc.siterm_train(g["counts"], g["times"], E, initialization=g["init"])
        assert np.allclose(r["loss_per_epoch_per_site"], g["lpeps_init"], rtol=1e-10, atol=0)
        assert relerr(r["res"], g["res_init"]) < 1e-9


def test_siterm_random_init():
    g = load_golden("siterm_dna.npz")
    r = orc.siterm_train(g["counts"], g["times"], g["lpe_rand"].shape[0])
    assert np.allclose(r["loss_per_epoch_per_site"], g["lpeps_rand"], rtol=1e-5, atol=0)
    assert relerr(r["res"], g["res_rand"]) < 1e-4


def test_jtt_ipw_reference_goldens():
    """The reference's own golden files (tests/estimation_tests/jtt_ipw_test.py:12-74)."""
    g = load_golden("jtt_ipw_toy.npz")
    ones = np.ones((3, 3))
    for key, mask, ipw in [("Q1_JTT_IPW_on_toy_matrix", ones, True),
                           ("Q1_JTT_IPW_on_toy_matrix_mask", g["mask"], True),
                           ("Q1_JTT_on_toy_matrix", ones, False),
                           ("Q1_JTT_on_toy_matrix_mask", g["mask"], False)]:
        got = orc.jtt_ipw(g["t"], g["C"], mask.astype(float), use_ipw=ipw)
        np.testing.assert_almost_equal(got, g[key], decimal=7)


def test_oracle_expm_against_reference_native_pade():
    """oracle/_ref/libref_expm.so = the reference's vendored r8mat_expm1 (Pade, FastCherries'
    bank: io_helpers.cpp:150-174), built from the reference's own sources by oracle/Makefile; its
    outputs are stored by tests/golden/make_golden_ref_native.py.
    Cross-checks the oracle's expm (torch.matrix_exp, f64) on the LG matrix over the grid."""
    Q = load_golden("data_lg.npz")["lg"]
    z = load_golden("ref_native.npz")
    grid = np.array([float("%.8f" % (0.03 * 1.1 ** i)) for i in range(-64, 65)])[::8]
    assert np.array_equal(grid, z["expm_grid"])
    P = orc.expm_bank(Q, grid)
    for b in range(len(grid)):
        assert np.abs(z["expm_P"][b] - P[b]).max() < 5e-14


# ---- SiteRM count / pseudocount assembly -------------------------------------
def _assembly_case(z, c):
    from cherryml_amd.io._tree import Tree
    tree = Tree()
    tree.add_nodes([str(v) for v in z[c + "_nodes"]])
    for u, v, t in zip(z[c + "_edges_u"], z[c + "_edges_v"], z[c + "_edges_t"]):
        tree.add_edge(str(u), str(v), float(t))
    msa = {str(k): str(s) for k, s in zip(z[c + "_msa_names"], z[c + "_msa_seqs"])}
    raw = np.zeros(tuple(z[c + "_raw_shape"]))
    raw[tuple(z[c + "_raw_nz"].T)] = z[c + "_raw_val"]
    return tree, msa, raw


ASSEMBLY_CASES = ["t2_eq_cherry", "t2_eq_edges", "t2_eq_edges_rev", "t2_uneq_cherry", "t2_uneq_edges",
                  "t2_uneq_edges_rev", "t2_some_missing", "rand_cherry"]


@pytest.mark.parametrize("case", ASSEMBLY_CASES)
def test_siterm_assembly_oracle_against_reference(case):
    from oracle import siterm_assembly_oracle as sa
    z = load_golden("siterm_assembly.npz")
    tree, msa, raw_ref = _assembly_case(z, case)
    grid = sorted(z[case + "_grid"].tolist())
    alphabet = [str(a) for a in z[case + "_alphabet"]]
    tr = sa.cherry_transitions(tree, msa) if str(z[case + "_strategy"]) == "cherry++" else sa.edge_transitions(tree, msa)
    assert [a for a, _, _ in tr] == [str(a) for a in z[case + "_tr_a"]]
    assert [b for _, b, _ in tr] == [str(b) for b in z[case + "_tr_b"]]
    assert np.array_equal(np.array([t for _, _, t in tr]), z[case + "_tr_t"])
    raw = sa.raw_count_matrices(tr, grid, alphabet, bool(z[case + "_reverse"]))
    assert np.array_equal(raw, raw_ref)
    prior = sa.count_prior_matrices(z[case + "_Q0"], grid)
    assert np.allclose(prior, z[case + "_prior"], rtol=1e-12, atol=1e-15)
    mixed = sa.mixed_count_matrices(raw, z[case + "_prior"], z[case + "_site_rates"], grid, float(z[case + "_lambda"]))
    cc, tt, init = sa.compactify(mixed, grid, z[case + "_Q0"], z[case + "_site_rates"])
    assert cc.shape == z[case + "_counts"].shape
    assert np.array_equal(tt, z[case + "_times"])
    assert np.array_equal(init, z[case + "_init"])
    assert np.allclose(cc, z[case + "_counts"], rtol=1e-14, atol=0)


# ---- FastCherries branch-length / site-rate estimation ------------------------
def test_ble_oracle_known_answers_of_the_reference_tests():
    """tests/test_branch_length_estimation.cpp: expected indices typed into the reference's tests."""
    from oracle import ble_oracle as bo
    z = load_golden("ble.npz")
    bank = bo.log_bank(z["Q"], z["grid_bl"], z["rates_bl"])
    for k in range(3):
        got = bo.get_branch_lengths(z[f"bl{k}_x"], z[f"bl{k}_y"], bank, z["s2r_bl"])
        assert list(got) == list(z[f"bl{k}_expected"]), k
    bank = bo.log_bank(z["Q"], z["grid_sr"], z["rates_sr"])
    pri = bo.rate_priors(z["rates_sr"])
    for k in range(6):
        x = z[f"sr{k}_x"]
        got = bo.get_site_rates(x, z[f"sr{k}_y"], bank, z["lengths_sr"][:len(x)], pri)
        assert list(got) == list(z[f"sr{k}_expected"]), k


@pytest.mark.parametrize("k", [0, 1, 2])
def test_ble_oracle_against_compiled_reference_outputs(k):
    from oracle import ble_oracle as bo
    z = load_golden("ble.npz")
    rates, grid = z[f"rnd{k}_rates"], z["grid_sr"]
    bank = bo.log_bank(z["Q"], grid, rates)
    cx, cy = z[f"rnd{k}_x"], z[f"rnd{k}_y"]
    assert list(bo.get_branch_lengths(cx, cy, bank, z[f"rnd{k}_s2r"])) == list(z[f"rnd{k}_bl"])
    assert list(bo.get_site_rates(cx, cy, bank, z[f"rnd{k}_li"], bo.rate_priors(rates))) == list(z[f"rnd{k}_sr"])
    lengths, site_rates, _, _ = bo.ble(cx, cy, np.concatenate([cx, cy]), bank, grid, rates, z[f"rnd{k}_weights"], 50)
    assert np.array_equal(lengths, z[f"rnd{k}_ble_lengths"])
    assert np.array_equal(site_rates, z[f"rnd{k}_ble_rates"])
    # the bank itself against the reference's native Pade expm (make_golden_ref_native.py: 2048 entries of the whole
    # [T,R,S,S] bank at seeded positions)
    zr = load_golden("ref_native.npz")
    assert np.allclose(bank.reshape(-1)[zr[f"rnd{k}_bank_idx"]], zr[f"rnd{k}_bank"], rtol=1e-9, atol=1e-12)


def test_siterm_site_rate_gather_oracle():
    from oracle import ble_oracle as bo
    z = load_golden("ble.npz")
    got = bo.compute_optimal_site_rates(z["gather_x"], z["gather_y"], z["gather_tensor"], z["gather_grid"],
                                        z["gather_prior"])
    assert np.array_equal(got, z["gather_expected"])


# ---- held-out log-likelihood (evaluation/_likelihood.py) --------------------------------------
def _likelihood_case(z, c):
    from cherryml_amd.io._tree import Tree
    tree = Tree()
    tree.add_nodes([str(v) for v in z[c + "_nodes"]])
    for u, v, t in zip(z[c + "_eu"], z[c + "_ev"], z[c + "_et"]):
        tree.add_edge(str(u), str(v), float(t))
    msa = {str(k): str(s) for k, s in zip(z[c + "_names"], z[c + "_seqs"])}
    cm = z[c + "_contact_map"] if bool(z[c + "_has_cm"]) else None
    return tree, msa, cm, [float(r) for r in z[c + "_rates"]]


LIKELIHOOD_CASES = [("wag3", "wag", False), ("wag4", "wag", False), ("wag4_gaps", "wag", False), ("wagxwag3", "wag", True),
                    ("rand_single", "lg", False), ("rand_pair", "wag", True), ("demo_single", "lg", False)]


def _chain_product(Q):
    """Q x Q: generator of two independent copies (markov_chain: chain_product), state = i1 * S + i2"""
    n = Q.shape[0]
    I = np.eye(n)
    return np.kron(Q, I) + np.kron(I, Q)


@pytest.mark.parametrize("case,model,pair", LIKELIHOOD_CASES)
def test_likelihood_oracle_against_reference(case, model, pair):
    from oracle import likelihood_oracle as lo
    z = load_golden("likelihood.npz")
    tree, msa, cm, rates = _likelihood_case(z, case)
    aa = [str(a) for a in z["amino_acids"]]
    Q1, pi1 = z[model], z["pi_" + model]
    Q2 = _chain_product(Q1) if pair else None
    pi2 = np.kron(pi1, pi1) if pair else None
    ll, lls = lo.log_likelihood(tree, msa, cm, rates, aa, pi1, Q1, pi2, Q2)
    assert abs(ll - float(z[case + "_ll_rev"])) < 1e-9 * abs(ll)
    assert np.allclose(lls, z[case + "_lls_rev"], rtol=1e-9, atol=1e-12)
    if case + "_published" in z:   # the value typed into the reference's tests (FastTree-verified, 4 decimals)
        pub = z[case + "_published"]
        assert np.allclose(ll if pub.ndim == 0 else lls, pub, atol=1e-4)


def test_oracle_siterm_matches_reference_on_cfg4_sites():
    """The oracle's SiteRM loop on 3 of the bench-tensor sites (B = 129, N = 20) and 2 of the 21-state non-symmetric
    sites the reference was run on (tests/golden/make_golden_siterm_cfg4.py): first 8 epochs of the loss curves."""
    import os
    import sys
    from oracle import ratelearn_oracle as orc
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden_siterm_cfg4 import nonsymmetric_21_state_problem
    z = load_golden("siterm_cfg4.npz")
    k = np.array([0, 1, 17])
    sel = z["sites20"][k]
    r = orc.siterm_train(z["banks20"][sel % 2], z["times20"][k], 8, initialization=z["init20"][k])
    assert np.allclose(r["loss_per_epoch_per_site"], z["lpeps20"][:8, k], rtol=1e-9, atol=0)
    T, C, Q0 = nonsymmetric_21_state_problem(L=24)
    r = orc.siterm_train(C[:2], T[:2], 8, initialization=Q0[:2])
    assert np.allclose(r["loss_per_epoch_per_site"], z["lpeps21"][:8, :2], rtol=1e-9, atol=0)


@pytest.mark.parametrize("case", ["toy3", "s20"])
@pytest.mark.parametrize("mode", ["default", "pande", "stationary", "stationary_reversible"])
def test_oracle_other_parameterisations_against_reference(mode, case):
    """rate.py:98-128, 190-218 ("default", "pande", "stationary", "stationary_reversible"): the oracle's restatement against the
    reference itself (tests/golden/make_golden_modes.py: float64 module, one evaluation + 30 epochs of train_quantization;
    the 20-state case carries the reference's own non-symmetric random mask)."""
    z = load_golden("modes.npz")
    k = f"{mode}_{case}"
    t, C, mask = z[f"{case}_t"], z[f"{case}_C"], z[f"{case}_mask"]
    lower = z[f"{k}_lower"] if f"{k}_lower" in z else None
    ev = orc.evaluate_mode(mode, z[f"{k}_upper"], lower, z[f"{k}_log_pi"], mask, t, C)
    assert abs(ev["loss"] - float(z[f"{k}_loss"])) <= 1e-13 * abs(float(z[f"{k}_loss"]))
    assert relerr(ev["Q"], z[f"{k}_Q"]) < 1e-14 and relerr(ev["dQ"], z[f"{k}_dQ"]) < 1e-12
    assert relerr(ev["d_upper"], z[f"{k}_d_upper"]) < 1e-12
    if lower is not None:
        assert relerr(ev["d_lower"], z[f"{k}_d_lower"]) < 1e-12
    if mode != "default":
        assert relerr(ev["d_log_pi"], z[f"{k}_d_log_pi"]) < 1e-11
    tr = orc.train_mode(mode, z[f"{k}_upper"], lower, z[f"{k}_log_pi"], mask, t, C, 30, 0.05)
    assert np.allclose(tr["loss"], z[f"{k}_traj_loss"], rtol=1e-10, atol=0)
    assert relerr(tr["Q_best"], z[f"{k}_Q_best"]) < 1e-9 and relerr(tr["Q_last"], z[f"{k}_Q_last"]) < 1e-9
