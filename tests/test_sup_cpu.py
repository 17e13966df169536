"""The branch supports without a GPU: the restatement's resampling (every replicate draws L sites; a replicate does not depend on
the number of replicates), aLRT against the restated scan, SH-like is 0 where aLRT is not positive, which cases decide every
decision well above the GPU tests' value bar (and which do not), the simulated family's false edges against its true ones, the
loud failure with no GPU, the new kernels' resources and the new symbol."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

import nni_cases  # noqa: E402
import sup_reference  # noqa: E402
from cherryml_amd import _lib  # noqa: E402

R = sup_reference.REPLICATES
MARGIN = 1e-9            # of |sum_u l_u|: ten times the bar of tests/test_gpu_sup.py on the resampled deltas
DECIDED = ["s20", "s32", "s20one"]


@pytest.mark.parametrize("L", [1, 3, 4, 7, 82, 401])
def test_the_weights_of_every_replicate_sum_to_the_number_of_sites(L):
    W = sup_reference.weights(L, R, 1 + 1000 * L)
    assert W.shape == (R, L) and W.min() >= 0 and np.all(W.sum(axis=1) == L)
    if L > 1:
        assert len({tuple(w) for w in W.tolist()}) > 1           # the replicates differ, and so do the seeds
        assert not np.array_equal(W, sup_reference.weights(L, R, 2 + 1000 * L))


def test_the_first_replicates_do_not_depend_on_the_number_of_replicates():
    for L, seed in ((7, 1), (82, 1001), (401, (1 << 63) + 5)):
        assert np.array_equal(sup_reference.weights(L, 256, seed)[:64], sup_reference.weights(L, 64, seed))


@pytest.mark.parametrize("name", nni_cases.CASES)
def test_alrt_is_minus_twice_the_best_restated_delta_and_sh_is_zero_where_it_is_not_positive(name):
    for (_, mvs, ll_moves, ll), s in zip(nni_cases.restated(name), sup_reference.restated(name)):
        delta = (ll_moves - ll[None, :]).sum(axis=1)
        vs = sorted(set(mvs[:, 0].tolist()))
        assert s["nodes"].tolist() == vs                            # nni_moves()' groups: v ascending
        assert len(s["alrt"]) == len(vs)
        for g, v in enumerate(vs):
            assert s["alrt"][g] == -2.0 * delta[mvs[:, 0] == v].max()
            assert 0 <= s["sh_count"][g] <= R and 0 <= s["rell_count"][g] <= R
            if s["alrt"][g] <= 0.0:
                assert s["sh_count"][g] == 0
        if len(mvs):
            assert s["delta_rep"].shape == (len(mvs), R)


def _smallest_margin(s):
    return min(s["sh_margin"].min(), s["rell_margin"].min()) / abs(s["fam_ll"])


@pytest.mark.parametrize("name", DECIDED)
def test_every_decision_of_the_large_alphabet_cases_is_decided(name):
    """measured here: 2.7e-8 and 1.1e-7 (s20), 1.5e-6 (s32), 1.7e-8 (s20one) of |sum l|"""
    seen = 0
    for k, s in enumerate(sup_reference.restated(name)):
        if len(s["nodes"]) == 0:
            continue
        m = _smallest_margin(s)
        print(f"{name}[{k}]: {len(s['nodes'])} edges x {R} replicates x 2 decisions, smallest margin {m:.2e} |sum l|")
        assert m > MARGIN, (name, k, m)
        seen += 1
    assert seen >= 1


def test_the_four_state_cases_have_undecided_decisions_and_the_gpu_test_brackets_them():
    """7 to 82 sites with many d = 0: exact and rounding-level ties.  The GPU test compares their counts with
    sup_reference.bounds, which must leave room exactly there"""
    for name in ("s4", "s4small"):
        for k, s in enumerate(sup_reference.restated(name)):
            if len(s["nodes"]) == 0:
                continue
            bar = MARGIN * abs(s["fam_ll"])
            und = int((s["sh_margin"] <= bar).sum() + (s["rell_margin"] <= bar).sum())
            print(f"{name}[{k}]: {und} of {2 * s['sh_margin'].size} decisions undecided")
            assert und > 0, (name, k)
            for g, (a, b, c, d) in enumerate(sup_reference.bounds(s, bar)):
                assert a <= s["sh_count"][g] <= b and c <= s["rell_count"][g] <= d
    for name in DECIDED:
        for s in sup_reference.restated(name):
            for g, (a, b, c, d) in enumerate(sup_reference.bounds(s, MARGIN * abs(s["fam_ll"]))):
                assert a == b == s["sh_count"][g] and c == d == s["rell_count"][g]


def test_on_the_simulated_family_every_false_edge_has_less_support_than_every_true_edge():
    """nni_cases.search_family on its start tree (three moves from the true one) at its true indices, seed 1: the probe gave at
    most 0.14 on the false edges against at least 0.95 on the true ones, smallest margin 2.4e-6 |sum l|"""
    mvs, s, true = sup_reference.restated_search_family()
    sh = s["sh_count"] / R
    false_edges = [sh[g] for g, v in enumerate(s["nodes"].tolist()) if not true[v]]
    true_edges = [sh[g] for g, v in enumerate(s["nodes"].tolist()) if true[v]]
    print("false edges", false_edges, "true edges", true_edges, "smallest margin", _smallest_margin(s))
    assert len(false_edges) >= 3 and len(true_edges) >= 3
    assert max(false_edges) < min(true_edges)
    assert _smallest_margin(s) > MARGIN


# ------------------------------------------------------------------------------------------------------ no GPU, resources
def test_no_gpu_means_the_stage_fails_loudly(tmp_path):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cherryml_amd import ml_branch_supports
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        ml_branch_supports(tree_dir="t", msa_dir="m", site_rates_dir="s", families=["f"], rate_matrix_path="q",
                           output_support_dir=str(tmp_path / "s"))


def test_sup_kernels_have_no_scratch_and_no_vgpr_spills():
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if k.startswith("sup_")}
    assert {"sup_weights_kernel", "sup_gemm_kernel", "sup_edge_kernel"} <= {k.split("(")[0] for k in hits}, hits
    for name, m in hits.items():
        print(name, m)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)


def test_the_header_declares_cb_bl_supports_and_the_binding_has_it():
    header = open(os.path.join(ROOT, "include", "cherrybank.h")).read()
    assert "int cb_bl_supports(cb_bl h, int n_rep, const uint64_t *seeds, const int *n_moves, const int *moves, double *alrt" in header
    fn = _lib.load().cb_bl_supports
    assert len(fn.argtypes) == 11
    from cherryml_amd import BranchLengthFitter
    import cherryml_amd.phylogeny_estimation as pe
    assert callable(BranchLengthFitter.branch_supports) and callable(pe.ml_branch_supports)
