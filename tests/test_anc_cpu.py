"""The marginal ancestral reconstruction without a GPU: the restatement (tests/anc_reference.py) against brute-force enumeration of
the states of ALL nodes, its normalisation, observed leaves and normaliser, the margin of every most probable state on the cases
the GPU tests compare (none may be left out there), its accuracy and calibration on a simulated family whose internal states are
known, the loud failure with no GPU, and the new kernel's resources."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

import anc_reference  # noqa: E402
import bl_cases  # noqa: E402
import bl_reference  # noqa: E402
import nni_cases  # noqa: E402
from cherryml_amd import _lib  # noqa: E402

MARGIN = 1e-9


def _restated(name):
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    out = []
    for parent, length, codes, rates in fams:
        tau = bl_reference.snap(length, parent, grid)
        out.append((tau,) + anc_reference.posteriors(parent, tau, codes, rates, grid, Q, pi))
    return out


@pytest.mark.parametrize("name,k", [("s4", 0), ("s4small", 0), ("s4small", 1)])
def test_at_four_states_the_restatement_equals_brute_force_over_all_nodes(name, k):
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    parent, _, codes, rates = fams[k]
    assert S == 4 and len(parent) <= 7
    tau, post, ll = _restated(name)[k]
    want, want_ll = anc_reference.brute_force(parent, tau, codes, rates, grid, Q, pi)
    print(f"{name}[{k}]: max |d post| = {np.abs(post - want).max():.2e}, max |d ll| = {np.abs(ll - want_ll).max():.2e}")
    assert np.abs(post - want).max() < 1e-12
    assert np.abs(ll - want_ll).max() < 1e-12


@pytest.mark.parametrize("name", nni_cases.CASES)
def test_posteriors_sum_to_one_observed_leaves_are_one_hot_and_the_normaliser_is_the_likelihood(name):
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    for (parent, _, codes, rates), (tau, post, ll) in zip(fams, _restated(name)):
        assert post.shape == (len(parent), len(rates), S) and np.all(np.isfinite(ll))
        assert np.abs(post.sum(axis=2) - 1.0).max() < 1e-12
        leaves = sorted(set(range(len(parent))) - set(parent.tolist()))
        seen = 0
        for v in leaves:
            obs = np.flatnonzero(codes[v] >= 0)
            seen += len(obs)
            assert np.array_equal(post[v, obs], np.eye(S)[codes[v, obs]])
        assert seen > 0
        norm = anc_reference.normaliser(parent, tau, codes, rates, grid, Q, pi)
        assert np.abs(norm - ll[None, :]).max() < 1e-12 * max(1.0, np.abs(ll).max())


def test_every_most_probable_state_of_the_gpu_cases_is_decided():
    """the GPU tests compare `state` at EVERY (node, site) of these cases: none is within rounding of a tie"""
    worst, count = np.inf, 0
    for name in nni_cases.CASES:
        for tau, post, ll in _restated(name):
            state, conf, margin = anc_reference.states(post)
            assert np.all(state >= 0) and np.all(conf > 0)
            worst, count = min(worst, margin.min()), count + margin.size
    print(f"smallest margin of a most probable state over {count} (node, site) entries: {worst:.3e}")
    assert worst > MARGIN


# ------------------------------------------------------------------------------------------------------ a simulated family
def _simulated_states():
    """nni_cases.search_family's draw again, keeping the states of EVERY node: -> (family, x [n_nodes, sites])"""
    f = nni_cases.search_family()
    rng = np.random.default_rng(nni_cases.SEARCH_SEED)
    parent = bl_cases.random_tree(12, rng)
    n = len(parent)
    tau = rng.integers(48, 72, n)
    tau[parent < 0] = -1
    rates = rng.permutation(np.repeat(nni_cases.SEARCH_RATES, 100))
    Q, pi = bl_cases.model(20)
    P = bl_reference.bank(nni_cases.GRID, np.unique(rates), Q)
    cat = np.searchsorted(np.unique(rates), rates)
    x = np.zeros((n, len(rates)), dtype=np.int64)
    root, _, order = bl_reference._preorder(parent)
    x[root] = rng.choice(20, len(rates), p=pi)
    for v in order[1:]:
        rows = np.clip(P[tau[v], cat, x[parent[v]]], 0.0, None)
        cdf = np.cumsum(rows / rows.sum(axis=1, keepdims=True), axis=1)
        x[v] = np.minimum((rng.random(len(rates))[:, None] > cdf).sum(axis=1), 19)
    assert np.array_equal(parent, f["true_parent"]) and np.array_equal(tau, f["tau"]) and np.array_equal(rates, f["rates"])
    leaves = sorted(set(range(n)) - set(parent.tolist()))
    assert np.array_equal(x[leaves], f["codes"][leaves])           # the same draw
    return f, x


def test_on_a_simulated_family_the_restated_map_states_are_accurate_and_calibrated():
    f, x = _simulated_states()
    Q, pi = bl_cases.model(20)
    parent = f["true_parent"]
    post, _ = anc_reference.posteriors(parent, f["tau"], f["codes"], f["rates"], nni_cases.GRID, Q, pi)
    state, conf, _ = anc_reference.states(post)
    internal = sorted(set(parent[parent >= 0].tolist()))
    acc = float((state[internal] == x[internal]).mean())
    mean_conf = float(conf[internal].mean())
    root = int(np.flatnonzero(parent < 0)[0])
    print(f"simulated family, {len(internal)} internal nodes x {x.shape[1]} sites: MAP accuracy {acc:.4f}, mean confidence "
          f"{mean_conf:.4f}; at the root: accuracy {float((state[root] == x[root]).mean()):.4f}, "
          f"mean confidence {float(conf[root].mean()):.4f}")
    assert acc >= mean_conf - 0.05


# ------------------------------------------------------------------------------------------------------ no GPU, resources
def test_no_gpu_means_the_reconstruction_fails_loudly(tmp_path):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cherryml_amd import ml_ancestral_sequences
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        ml_ancestral_sequences(tree_dir="t", msa_dir="m", site_rates_dir="s", families=["f"], rate_matrix_path="q",
                               output_msa_dir=str(tmp_path / "a"), output_confidence_dir=str(tmp_path / "c"))


def test_anc_kernels_have_no_scratch_and_no_vgpr_spills():
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if k.startswith("anc_")}
    assert {"anc_post_kernel"} <= {k.split("(")[0] for k in hits}, hits
    for name, m in hits.items():
        print(name, m)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)
