"""The NNI search without a GPU: the restated scan formula against re-pruning of the rearranged tree and against brute-force
enumeration, the enumeration and application of moves, the selection against its restatement, the restated search (monotone; it
ends where no single move gains; the seed of the GPU search test decides everything and recovers the true splits), the loud
failure with no GPU, and the new kernels' resources."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

import bl_cases  # noqa: E402
import bl_reference  # noqa: E402
import nni_cases  # noqa: E402
import nni_reference  # noqa: E402
from cherryml_amd import _lib  # noqa: E402

MARGIN = 1e-9


def _tree(parent, length=None):
    from cherryml_amd.io import Tree
    t = Tree()
    t.add_nodes([f"n{v}" for v in range(len(parent))])
    t.add_edges([(f"n{p}", f"n{v}", 0.1 * (v + 1) if length is None else float(length[v])) for v, p in enumerate(parent) if p >= 0])
    return t


def _parent_of(tree):
    index = {v: i for i, v in enumerate(tree.nodes())}
    parent = np.full(len(index), -1)
    for u, v, _ in tree.edges():
        parent[index[v]] = index[u]
    return parent


# ------------------------------------------------------------------------------------------------------ the scan formula
@pytest.mark.parametrize("name", nni_cases.CASES)
def test_the_scan_formula_equals_pruning_of_the_rearranged_tree(name):
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    for (parent, _, codes, rates), (tau, mvs, ll_moves, ll) in zip(fams, nni_cases.restated(name)):
        assert np.abs(ll - nni_reference.site_ll(parent, tau, codes, rates, grid, Q, pi)).max() == 0.0
        for m, mv in enumerate(mvs):
            want = nni_reference.site_ll(nni_reference.apply(parent, [mv]), tau, codes, rates, grid, Q, pi)
            assert np.all(np.abs(ll_moves[m] - want) < 1e-12 * np.maximum(1.0, np.abs(want))), (name, mv)


@pytest.mark.parametrize("name,k", [("s4small", 0), ("s4small", 1), ("s4", 1)])
def test_at_four_states_the_scan_formula_equals_brute_force(name, k):
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    parent, _, codes, rates = fams[k]
    tau, mvs, ll_moves, _ = nni_cases.restated(name)[k]
    assert len(mvs) > 0
    for m, mv in enumerate(mvs):
        want = bl_reference.brute_force(nni_reference.apply(parent, [mv]), tau, codes, rates, grid, Q, pi)[1]
        assert np.all(np.abs(ll_moves[m] - want) < 1e-12 * np.maximum(1.0, np.abs(want))), (name, mv)


# ------------------------------------------------------------------------------------------------------ moves
@pytest.mark.parametrize("name", nni_cases.CASES)
def test_enumeration_and_apply(name):
    from cherryml_amd.phylogeny_estimation import apply_nni, enumerate_nni_moves
    _, _, fams = nni_cases.case(name)
    counts = []
    for parent, length, _, _ in fams:
        mvs = enumerate_nni_moves(parent)
        counts.append(len(mvs))
        assert mvs.dtype == np.int32 and mvs.shape == (len(mvs), 3)
        assert np.array_equal(mvs, nni_reference.moves(parent))
        assert [tuple(m) for m in mvs.tolist()] == sorted({tuple(m) for m in mvs.tolist()})   # v, then c, then s; no repeats
        tree = _tree(parent, length)
        arity = np.bincount(parent[parent >= 0], minlength=len(parent))
        for v, c, s in mvs.tolist():
            p = parent[v]
            assert p >= 0 and arity[v] > 0 and parent[c] == v and parent[s] == p and s != v
            moved = apply_nni(tree, [(v, c, s)])
            new = _parent_of(moved)
            assert np.array_equal(new, nni_reference.apply(parent, [(v, c, s)]))
            assert moved.nodes() == tree.nodes() and set(moved.leaves()) == set(tree.leaves())
            assert np.array_equal(np.bincount(new[new >= 0], minlength=len(parent)), arity)
            assert [(b, t) for _, b, t in moved.edges()] == [(b, t) for _, b, t in tree.edges()]   # every node keeps its edge
            assert moved.root() == tree.root()
            assert len(moved.postorder_traversal()) == len(parent)                                  # still one tree
            back = apply_nni(moved, [(v, s, c)])
            assert np.array_equal(_parent_of(back), parent) and back.edges() == tree.edges()
    assert counts == nni_cases.MOVE_COUNTS[name]


def test_apply_nni_refuses_overlapping_moves_and_what_is_no_move():
    from cherryml_amd.phylogeny_estimation import apply_nni
    parent = bl_cases.caterpillar(9)
    tree = _tree(parent)
    mvs = nni_reference.moves(parent)
    a = mvs[0]
    for b in mvs[1:]:
        fa, fb = {int(parent[a[0]]), *map(int, a)}, {int(parent[b[0]]), *map(int, b)}
        if fa & fb:
            with pytest.raises(ValueError, match="share node"):
                apply_nni(tree, [a, b])
        else:
            assert np.array_equal(_parent_of(apply_nni(tree, [a, b])), nni_reference.apply(parent, [a, b]))
    assert any(not ({int(parent[a[0]]), *map(int, a)} & {int(parent[b[0]]), *map(int, b)}) for b in mvs[1:])
    v, c, s = (int(x) for x in a)
    for bad, match in (((0, c, s), "no move"), ((v, s, c), "no move"), ((v, c, v), "no move"), ((v, c, 99), "outside"),
                       ((c, c, s), "no move")):
        with pytest.raises(ValueError, match=match):
            apply_nni(tree, [bad])


def test_select_nni_matches_the_restatement():
    from cherryml_amd.phylogeny_estimation import select_nni
    rng = np.random.default_rng(3)
    for parent in (bl_cases.caterpillar(9), bl_cases.random_tree(17, np.random.default_rng(5)), nni_cases.BIN4, bl_cases.star3()):
        mvs = nni_reference.moves(parent)
        for trial in range(20):
            delta = rng.normal(size=len(mvs))
            if trial % 2:
                delta = np.round(delta)            # ties, and zeros (not above min_gain)
            gain = [0.0, 0.5][trial % 3 == 0]
            got = select_nni(mvs, delta, parent, min_gain=gain)
            assert np.array_equal(got, nni_reference.select(mvs, delta, parent, gain))
            assert np.array_equal(got, select_nni(mvs, delta, parent, min_gain=gain))     # deterministic
            assert np.all(delta[got] > gain) and np.all(np.diff(delta[got]) <= 0)         # ordered
            ties = np.flatnonzero(np.diff(delta[got]) == 0)
            assert np.all(got[ties] < got[ties + 1])                                      # ties: the lower index first
            used = [x for m in got for x in {int(parent[mvs[m][0]]), *map(int, mvs[m])}]
            assert len(used) == len(set(used))                                            # disjoint
            # greedy: every move left out is below the bar or meets a taken move of at least its gain
            for m in set(range(len(mvs))) - set(got.tolist()):
                if delta[m] > gain:
                    four = {int(parent[mvs[m][0]]), *map(int, mvs[m])}
                    assert any(four & {int(parent[mvs[k][0]]), *map(int, mvs[k])} and delta[k] >= delta[m] for k in got)
    assert len(select_nni(np.zeros((0, 3)), [], bl_cases.star3())) == 0
    with pytest.raises(ValueError, match="deltas"):
        select_nni(mvs, [1.0], parent)


# ------------------------------------------------------------------------------------------------------ the search
def test_the_restated_search_never_lowers_a_likelihood_and_ends_where_no_move_gains():
    f, r = nni_cases.search_family(), nni_cases.restated_search()
    Q, pi = bl_cases.model(20)
    lls = [x for rec in r["rounds"] for x in (rec["before"], rec["after"])] + [r["final"]]
    print("restated search:", [(rec["before"], len(rec["selected"]), len(rec["applied"]), rec["after"]) for rec in r["rounds"]],
          r["final"], "margin", r["margin"], "em margin", r["em_margin"])
    assert all(b >= a for a, b in zip(lls, lls[1:])), lls
    assert sum(len(rec["applied"]) for rec in r["rounds"]) >= 3
    assert r["rounds"][-1]["applied"] == [] and len(r["rounds"]) < nni_cases.SEARCH_NNI_ROUNDS   # it ended by itself
    mvs = nni_reference.moves(r["parent"])
    ll_moves, ll = nni_reference.scan(r["parent"], r["tau"], f["codes"], f["rates"], nni_cases.GRID, Q, pi, mvs)
    assert np.all((ll_moves - ll[None, :]).sum(axis=1) <= 0.0)
    assert ll.sum() == r["final"]


def test_the_seed_of_the_gpu_search_decides_everything_and_recovers_the_true_splits():
    f, r = nni_cases.search_family(), nni_cases.restated_search()
    assert nni_reference.splits(f["start_parent"]) != nni_reference.splits(f["true_parent"])
    assert len(nni_reference.splits(f["true_parent"]) - nni_reference.splits(f["start_parent"])) == 3   # three moves apart
    assert r["margin"] > MARGIN and r["em_margin"] > MARGIN, (r["margin"], r["em_margin"])
    assert nni_reference.splits(r["parent"]) == nni_reference.splits(f["true_parent"])


# ------------------------------------------------------------------------------------------------------ no GPU, resources
def test_no_gpu_means_the_search_fails_loudly(tmp_path):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cherryml_amd import ml_nni_trees, nj_nni_trees
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        ml_nni_trees(tree_dir="t", msa_dir="m", site_rates_dir="s", families=["f"], rate_matrix_path="q",
                     output_tree_dir=str(tmp_path / "t"), output_likelihood_dir=str(tmp_path / "l"))
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        nj_nni_trees(msa_dir="m", families=["f"], rate_matrix_path="q", num_rate_categories=4, output_tree_dir=str(tmp_path / "t"),
                     output_site_rates_dir=str(tmp_path / "s"), output_likelihood_dir=str(tmp_path / "l"))


def test_nni_kernels_have_no_scratch_and_no_vgpr_spills():
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if k.startswith("nni_")}
    assert {"nni_scan_kernel", "nni_sum_kernel"} <= {k.split("(")[0] for k in hits}, hits
    for name, m in hits.items():
        print(name, m)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)
