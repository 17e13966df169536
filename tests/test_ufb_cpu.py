"""The bootstrap supports from the search's own trees without a GPU: the restated search family reproduces the figures the
feature was specified with (contributions, candidates, every replicate decided, the nine supports as exact multiples of 1/256),
which cases have undecided replicates (exact ties of two moves at a multifurcation) and which have none, a replicate does not
depend on the number of replicates, carrying the best over contributions is one argmax over their union, `ufboot_supports` on
hand-made choices against the restatement, the file round trip, the loud failure with no GPU, the new kernels' resources and
the new symbol."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

import nni_cases  # noqa: E402
import nni_reference  # noqa: E402
import sup_reference  # noqa: E402
import ufb_reference  # noqa: E402
from cherryml_amd import _lib  # noqa: E402

R = ufb_reference.REPLICATES
MARGIN = 1e-9            # of max(1, |sum_u l_u|): ten times the GPU tests' bar on the scores


def _tree(parent):
    from cherryml_amd.io import Tree
    t = Tree()
    t.add_nodes([f"n{v}" for v in range(len(parent))])
    t.add_edges([(f"n{p}", f"n{v}", 0.125) for v, p in enumerate(parent) if p >= 0])
    return t


def test_the_restated_search_family_gives_the_specified_figures():
    """2 contributions (3 moves applied in round 0, none in round 1) with 25 candidates each; the smallest margin over all 256
    replicates is 1.57e-2 against a bar of 2.7e-6; the final tree is the true one; supports 1 (six times), 248 / 256, 211 / 256
    and 165 / 256; six (t, code) pairs, the round-1 tree itself with 113 replicates and one round-0 neighbour with 1"""
    final, contribs, c, (nodes, share) = ufb_reference.restated_search()
    f = nni_cases.search_family()
    assert [x["nni_round"] for x in contribs] == [0, 1]
    assert sum(1 + len(x["moves"]) for x in contribs) == 50
    search = nni_cases.restated_search()
    assert np.array_equal(final, search["parent"]) and [len(r["applied"]) for r in search["rounds"]] == [3, 0]
    assert nni_reference.splits(final) == nni_reference.splits(f["true_parent"])
    bar = MARGIN * max(1.0, abs(float(contribs[-1]["ll"].sum())))
    print(f"smallest margin {c['margin'].min():.3e}, bar {bar:.2e}, pairs {c['pairs']}")
    assert int((c["margin"] <= bar).sum()) == 0                       # every replicate is decided
    assert 1.5e-2 < c["margin"].min() < 1.6e-2 and 2.6e-6 < bar < 2.8e-6
    counts = share * R
    assert np.array_equal(counts, np.rint(counts)) and len(nodes) == 9
    assert sorted(counts.tolist(), reverse=True) == [256.0] * 6 + [248.0, 211.0, 165.0]
    assert len(c["pairs"]) == 6 and c["pairs"][(1, -1)] == 113
    assert sorted(v for (t, _), v in c["pairs"].items() if t == 0) == [1]
    assert sum(c["pairs"].values()) == R and not np.any(c["code"] == -2)


def test_the_random_cases_have_exact_ties_and_the_families_without_moves_have_none():
    """two moves at a multifurcation give the same unrooted tree: 21 to 166 of 256 replicates per family are undecided"""
    for name in nni_cases.CASES:
        for k, (r, n_moves) in enumerate(zip(ufb_reference.restated(name), nni_cases.MOVE_COUNTS[name])):
            und = int((r["margin"] <= MARGIN * max(1.0, abs(r["fam_ll"]))).sum())
            print(f"{name}[{k}]: {n_moves} moves, {und} of {R} replicates undecided")
            assert r["cand"].shape == (2 + n_moves, R)
            if n_moves == 0:
                assert und == 0 and np.all(r["code"] == -1) and np.array_equal(r["score"], r["base"])
            else:
                assert 21 <= und <= 166, (name, k, und)
            assert not np.any(r["code"] == -2)


def test_the_first_replicates_do_not_depend_on_the_number_of_replicates():
    for k, (_, _, ll_moves, ll) in enumerate(nni_cases.restated("s20")):
        seed = sup_reference.family_seed(k)
        few, many = ufb_reference.best(ll_moves, ll, 64, seed), ufb_reference.restated("s20")[k]
        assert np.array_equal(sup_reference.weights(len(ll), 64, seed), sup_reference.weights(len(ll), R, seed)[:64])
        # (NumPy's product may sum in another order at another shape: the values to rounding, the codes where decided)
        bar = 1e-12 * abs(many["fam_ll"])
        for key in ("score", "base"):
            assert np.abs(few[key] - many[key][:64]).max() <= bar, (k, key)
        decided = many["margin"][:64] > bar
        assert decided.sum() >= 20 and np.array_equal(few["code"][decided], many["code"][:64][decided])


def test_carrying_the_best_over_two_contributions_is_one_argmax_over_their_union():
    _, contribs, c, _ = ufb_reference.restated_search()
    assert len(contribs) == 2
    union = c["union"]                                   # the candidates of contribution 0, then those of contribution 1
    arg = np.argmax(union, axis=0)                       # the first of equal maxima
    n0 = 1 + len(contribs[0]["moves"])
    assert np.array_equal(c["score"], union[arg, np.arange(R)])
    assert np.array_equal(c["t"], (arg >= n0).astype(np.int64))
    assert np.array_equal(c["code"], np.where(arg >= n0, arg - n0, arg) - 1)
    # an incoming best that nothing beats stays (code -2); the carried score never falls
    first = ufb_reference.best(contribs[0]["ll_moves"], contribs[0]["ll"], R, 1)
    again = ufb_reference.best(contribs[0]["ll_moves"], contribs[0]["ll"], R, 1, incoming=first["score"])
    assert np.all(again["code"] == -2) and np.array_equal(again["score"], first["score"])
    assert np.all(c["score"] >= first["score"])


def test_ufboot_supports_on_hand_made_choices_equals_the_restatement():
    """the 17-leaf tree with a trifurcating root (s20, family 1): contribution 0 is the tree, contribution 1 the tree after a
    move below the root; the choices take the trees themselves (code -1), a move at the multifurcation (p is the root, which
    has three children) and moves elsewhere"""
    from cherryml_amd.phylogeny_estimation import bootstrap_tree, enumerate_nni_moves, ufboot_supports
    from cherryml_amd.phylogeny_estimation._nni import _parent_array
    parent0 = np.asarray(nni_cases.case("s20")[2][1][0])
    moves0 = nni_reference.moves(parent0)
    assert np.array_equal(moves0, enumerate_nni_moves(parent0))
    root = int(np.flatnonzero(parent0 < 0)[0])
    at_root = [m for m, (v, _, _) in enumerate(moves0.tolist()) if parent0[v] == root]
    deep = [m for m, (v, _, _) in enumerate(moves0.tolist()) if parent0[v] != root]
    assert int((parent0 == root).sum()) == 3 and len(at_root) >= 2 and len(deep) >= 2
    parent1 = nni_reference.apply(parent0, [moves0[deep[0]]])
    moves1 = nni_reference.moves(parent1)
    contribs = [dict(parent=parent0, moves=moves0), dict(parent=parent1, moves=moves1)]
    t = np.array([0, 0, 0, 1, 1, 1, 0, 1, 0, 0])
    code = np.array([-1, at_root[0], at_root[1], -1, 0, len(moves1) - 1, deep[0], 3, deep[1], -1])
    trees = [_tree(parent0), _tree(parent1)]
    for final_parent, final_tree in ((parent1, trees[1]), (parent0, trees[0])):
        nodes, share = ufboot_supports(final_tree, trees, (t, code))
        want_nodes, want = ufb_reference.supports(final_parent, contribs, t, code)
        print(nodes, share, want)
        assert np.array_equal(nodes, want_nodes) and np.array_equal(share, want)
        assert share.min() < 1.0 and share.max() == 1.0 and np.allclose(share * 10, np.rint(share * 10), atol=1e-12)
    # the tree a replicate chose
    assert np.array_equal(_parent_array(bootstrap_tree(trees, 0, deep[0])), parent1)
    assert bootstrap_tree(trees, 1, -1) is trees[1]
    for bad_t, bad_code in ((2, -1), (0, len(moves0)), (0, -2)):
        with pytest.raises(ValueError):
            bootstrap_tree(trees, bad_t, bad_code)
    # the restated search family through the package's host code
    final, sc, c, (want_nodes, want) = ufb_reference.restated_search()
    nodes, share = ufboot_supports(_tree(final), [_tree(x["parent"]) for x in sc], (c["t"], c["code"]))
    assert np.array_equal(nodes, want_nodes) and np.array_equal(share, want)


def test_the_support_file_round_trip(tmp_path):
    from cherryml_amd.phylogeny_estimation import read_ufboot_supports, write_ufboot_supports
    from cherryml_amd.phylogeny_estimation._ufboot import choices_lines, update_choice
    names = [f"n{v}" for v in range(7)]
    nodes, share = np.array([1, 3]), np.array([211 / 256, 1.0])
    path = str(tmp_path / "fam.txt")
    write_ufboot_supports(path, names, nodes, share)
    lines = open(path).read().split("\n")
    assert lines[0] == "node ufboot" and lines[-1] == "" and [ln.split()[0] for ln in lines[1:-1]] == ["n1", "n3"]
    assert read_ufboot_supports(path) == {"n1": 211 / 256, "n3": 1.0}
    (tmp_path / "other.txt").write_text("node alrt sh rell\n")
    with pytest.raises(ValueError, match="not a ufboot support file"):
        read_ufboot_supports(str(tmp_path / "other.txt"))
    choice = (np.full(4, -1, dtype=np.int64), np.full(4, -2, dtype=np.int64))
    update_choice(choice, 0, np.array([-1, 3, -1, 0]))
    update_choice(choice, 1, np.array([-2, -2, 5, -1]))
    assert choice[0].tolist() == [0, 0, 1, 1] and choice[1].tolist() == [-1, 3, 5, -1]
    assert choices_lines([0, 1], [25, 25], choice) == ["0 0 25 1 1\n", "1 1 25 1 1\n"]


# ------------------------------------------------------------------------------------------------------ no GPU, resources
def test_no_gpu_means_the_stage_fails_loudly(tmp_path):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cherryml_amd import ml_nni_trees, nj_nni_trees
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        ml_nni_trees(tree_dir="t", msa_dir="m", site_rates_dir="s", families=["f"], rate_matrix_path="q",
                     output_tree_dir=str(tmp_path / "t"), output_likelihood_dir=str(tmp_path / "l"),
                     output_bootstrap_dir=str(tmp_path / "b"), num_bootstrap_replicates=64, bootstrap_seed=3)
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        nj_nni_trees(msa_dir="m", families=["f"], rate_matrix_path="q", num_rate_categories=4,
                     output_bootstrap_dir=str(tmp_path / "b"), num_bootstrap_replicates=64, bootstrap_seed=3)


def test_ufb_kernels_have_no_scratch_and_no_vgpr_spills():
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if "ufb_" in k}
    names = set(hits)
    assert any("ufb_gemm_kernel<true>" in k for k in names) and any("ufb_gemm_kernel<false>" in k for k in names), hits
    assert any(k.startswith("ufb_merge_kernel") for k in names), hits
    for name, m in hits.items():
        print(name, m)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (name, m)


def test_the_header_declares_cb_bl_bootstrap_best_and_the_binding_has_it():
    header = open(os.path.join(ROOT, "include", "cherrybank.h")).read()
    assert ("int cb_bl_bootstrap_best(cb_bl h, int n_rep, const uint64_t *seeds, const int *n_moves, const int *moves, "
            "double *best_score,") in header
    fn = _lib.load().cb_bl_bootstrap_best
    assert len(fn.argtypes) == 10
    import cherryml_amd
    import cherryml_amd.phylogeny_estimation as pe
    assert callable(cherryml_amd.BranchLengthFitter.bootstrap_best)
    for name in ("ufboot_supports", "read_ufboot_supports", "write_ufboot_supports", "bootstrap_tree"):
        assert name in cherryml_amd.__all__ and hasattr(cherryml_amd, name) and hasattr(pe, name)
