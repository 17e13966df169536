"""The SPR search without a GPU: the restated scan formula against re-pruning of the rearranged tree and against brute-force
enumeration, the enumeration against the definition of the distance and the counted moves, the shapes of the ways the formula
branches on, the indices a move is offered at, the application and selection of moves against their restatements, the restated
search (monotone; the start of the GPU search test decides everything and recovers the true tree in one move), the loud failure
with no GPU, and the new kernel's resources."""
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
import spr_reference  # noqa: E402
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


def _agree(got, want, what):
    """1e-12 max(1, |ll|) where finite; infinite sites in place"""
    inf = ~np.isfinite(want)
    assert np.array_equal(got[inf], want[inf]), what
    assert np.all(np.abs(got[~inf] - want[~inf]) < 1e-12 * np.maximum(1.0, np.abs(want[~inf]))), what


# ------------------------------------------------------------------------------------------------------ the scan formula
@pytest.mark.parametrize("name", nni_cases.CASES)
def test_the_scan_formula_equals_pruning_of_the_rearranged_tree(name):
    S, grid, fams = nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    for (parent, _, codes, rates), (tau, mvs, ll_moves, ll) in zip(fams, spr_reference.restated(name)):
        assert np.array_equal(ll, nni_reference.site_ll(parent, tau, codes, rates, grid, Q, pi))
        for m, mv in enumerate(mvs):
            cand, ctau = spr_reference.apply(parent, tau, [mv])
            _agree(ll_moves[m], nni_reference.site_ll(cand, ctau, codes, rates, grid, Q, pi), (name, mv))


@pytest.mark.parametrize("name,k", [("s20", 0), ("s4", 1), ("deep", 0)])
def test_the_scan_formula_at_every_distance_up_to_the_cap(name, k):
    """the 9-leaf caterpillar (distances up to 7), the 11-node tree, and the 11-leaf caterpillar of spr_reference.deep_family,
    which reaches the cap of 8 (and 9, which is not enumerated): every move, at indices that differ from the tree's"""
    S, grid, fams = (4, bl_cases.GRID, [spr_reference.deep_family()]) if name == "deep" else nni_cases.case(name)
    Q, pi = bl_cases.model(S)
    parent, length, codes, rates = fams[k]
    tau = bl_reference.snap(length, parent, grid)
    mvs = spr_reference.full_moves(parent, tau, grid, spr_reference.MAX_RADIUS)
    dist = [spr_reference.distance(parent, int(x), int(y)) for x, y in mvs[:, :2]]
    print(name, len(mvs), "moves, by distance", np.bincount(dist).tolist())
    assert max(dist) == {"s20": 7, "s4": 2, "deep": 8}[name] and set(dist) == set(range(1, max(dist) + 1))
    mvs[:, 2:] = (mvs[:, 2:] + np.arange(len(mvs))[:, None] * np.array([3, 5, 7])) % len(grid)   # any three indices
    ll_moves, _ = spr_reference.scan(parent, tau, codes, rates, grid, Q, pi, mvs)
    for m, mv in enumerate(mvs):
        cand, ctau = spr_reference.apply(parent, tau, [mv])
        _agree(ll_moves[m], nni_reference.site_ll(cand, ctau, codes, rates, grid, Q, pi), (name, mv))


@pytest.mark.parametrize("k", [0, 1])
def test_at_four_states_the_scan_formula_equals_brute_force(k):
    S, grid, fams = nni_cases.case("s4small")
    Q, pi = bl_cases.model(S)
    parent, _, codes, rates = fams[k]
    tau, mvs, ll_moves, _ = spr_reference.restated("s4small")[k]
    assert len(mvs) > 0
    for m, mv in enumerate(mvs):
        cand, ctau = spr_reference.apply(parent, tau, [mv])
        _agree(ll_moves[m], bl_reference.brute_force(cand, ctau, codes, rates, grid, Q, pi)[1], mv)


# ------------------------------------------------------------------------------------------------------ moves
@pytest.mark.parametrize("name", nni_cases.CASES)
def test_enumeration_against_the_definition_and_the_counted_moves(name):
    from cherryml_amd.phylogeny_estimation import enumerate_spr_moves
    _, _, fams = nni_cases.case(name)
    for r in (1, 2, 3, 8):
        counts = []
        for parent, _, _, _ in fams:
            xy = enumerate_spr_moves(parent, r)
            counts.append(len(xy))
            assert xy.dtype == np.int32 and xy.shape == (len(xy), 2)
            assert np.array_equal(xy, spr_reference.moves(parent, r))
            assert [tuple(m) for m in xy.tolist()] == sorted({tuple(m) for m in xy.tolist()})   # x, then y; no repeats
            # the definition: every pair of nodes, the distance counted on the pruned tree
            ch = bl_reference._preorder(parent)[1]
            want = []
            for x in range(len(parent)):
                p = parent[x]
                if p < 0 or parent[p] < 0 or len(ch[p]) != 2:
                    continue
                s = [c for c in ch[p] if c != x][0]
                for y in range(len(parent)):
                    if parent[y] < 0 or y in (x, p, s) or y in spr_reference._below(ch, x):
                        continue
                    if spr_reference.distance_by_definition(parent, x, y) <= r:
                        want.append((x, y))
            assert [tuple(m) for m in xy.tolist()] == want
        if r <= 3:
            assert counts == spr_reference.MOVE_COUNTS[name][r - 1], (name, r)
    with pytest.raises(ValueError, match="radius"):
        enumerate_spr_moves(fams[0][0], 9)


def test_every_shape_of_way_the_formula_branches_on_is_among_the_cases():
    seen = set()
    for name in nni_cases.CASES:
        _, _, fams = nni_cases.case(name)
        for parent, _, codes, _ in fams:
            ch = bl_reference._preorder(parent)[1]
            for x, y in spr_reference.moves(parent, 3).tolist():
                p = parent[x]
                s, g = [c for c in ch[p] if c != x][0], parent[p]
                r = spr_reference.route(parent, x, y)
                if r[0] == "below":
                    seen.add("below s")
                else:
                    if y == g:
                        seen.add("y = g")
                    if parent[y] == g and parent[g] < 0:
                        seen.add("sibling of p, g the root")
                    if parent[y] == g and len(ch[g]) > 2:
                        seen.add("sibling at a multifurcating g")
                    if len(r[1]) > 1 and len(r[2]) > 0:
                        seen.add("up and then down")
                    if len(r[1]) > 1 and len(r[2]) == 0:
                        seen.add("y an ancestor of g")
                for w, what in ((y, "leaf y"), (x, "leaf x"), (s, "leaf s")):
                    if not ch[w]:
                        seen.add(what)
                if not ch[s] and np.any(codes[s] < 0) and r[0] == "through":
                    seen.add("leaf s with a gap")
    assert seen == {"below s", "y = g", "sibling of p, g the root", "sibling at a multifurcating g", "up and then down",
                    "y an ancestor of g", "leaf y", "leaf x", "leaf s", "leaf s with a gap"}, seen


def test_spr_indices_keep_the_path_halve_the_target_and_clamp():
    from cherryml_amd.phylogeny_estimation import spr_indices
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    grid = np.array(quantization_points_ble(0.03, 1.1, 64))
    parent = nni_cases.LADDER4                    # [-1, 0, 0, 1, 1, 3, 3]: x = 5 has p = 3, s = 6, g = 1
    tau = np.array([-1, 64, 64, 64, 64, 64, 64])
    assert spr_indices(grid, tau, parent, [(5, 4)]).tolist() == [[71, 57, 57]]     # 2 grid[64] -> 71, grid[64] / 2 -> 57
    assert spr_indices(grid, tau, parent, [(5, 4)]).dtype == np.int32
    top = len(grid) - 1
    tau = np.array([-1, 0, 0, top, 0, 0, top])
    assert spr_indices(grid, tau, parent, [(5, 4), (5, 1)]).tolist() == [[top, 0, 0], [top, 0, 0]]   # both ends clamp
    tau = np.array([-1, 3, 3, 0, top, 0, 0])
    assert spr_indices(grid, tau, parent, [(5, 4)]).tolist() == [[7, top - 7, top - 7]]
    for g, t in ((bl_cases.GRID5, np.array([-1, 1, 4, 2, 3, 0, 1])), (bl_cases.GRID, np.array([-1, 5, 100, 70, 128, 0, 90]))):
        for parent in (nni_cases.LADDER4, nni_cases.BIN4):
            xy = spr_reference.moves(parent, 3)
            got = spr_indices(g, t, parent, xy)
            assert np.array_equal(got, spr_reference.indices(g, t, parent, xy)) and got.min() >= 0 and got.max() < len(g)
    g5 = np.array(bl_cases.GRID5)                 # T = 5: 0.05 + 0.2 is nearest to 0.2, 0.8 / 2 to 0.2 (|log| 0.69 both ways: the lower)
    assert spr_indices(g5, np.array([-1, 1, 1, 1, 3, 1, 2]), nni_cases.LADDER4, [(5, 4)]).tolist() == [[2, 2, 2]]
    assert spr_indices(g5, np.array([-1, 1, 1, 1, 3, 1, 2]), nni_cases.LADDER4, np.zeros((0, 2))).shape == (0, 3)


@pytest.mark.parametrize("name", nni_cases.CASES)
def test_apply_spr_keeps_nodes_leaves_arities_and_untouched_edges(name):
    from cherryml_amd.phylogeny_estimation import apply_spr
    _, grid, fams = nni_cases.case(name)
    grid = np.asarray(grid)
    for (parent, _, _, _), (tau, mvs, _, _) in zip(fams, spr_reference.restated(name)):
        length = np.where(tau >= 0, grid[tau], 0.0)
        tree = _tree(parent, length)
        arity = np.bincount(parent[parent >= 0], minlength=len(parent))
        ch = bl_reference._preorder(parent)[1]
        for mv in mvs[::3].tolist():
            x, y, ts, tp, ty = mv
            moved = apply_spr(tree, [mv], grid)
            want, wtau = spr_reference.apply(parent, tau, [mv])
            new = _parent_of(moved)
            assert np.array_equal(new, want)
            assert moved.nodes() == tree.nodes() and set(moved.leaves()) == set(tree.leaves()) and moved.root() == tree.root()
            assert np.array_equal(np.bincount(new[new >= 0], minlength=len(parent)), arity)
            assert len(moved.postorder_traversal()) == len(parent)                            # still one tree
            p = parent[x]
            s = [c for c in ch[p] if c != x][0]
            for (_, b, t), (_, b0, t0) in zip(moved.edges(), tree.edges()):                   # the edges keep their order
                v = int(b[1:])
                assert b == b0 and t == (grid[wtau[v]] if v in (s, p, y) else t0)


def test_apply_spr_refuses_overlapping_moves_and_what_is_no_move():
    from cherryml_amd.phylogeny_estimation import apply_spr
    parent = bl_cases.caterpillar(9)
    grid = np.asarray(bl_cases.GRID)
    tau = np.where(parent >= 0, 60, -1)
    tree = _tree(parent, np.where(tau >= 0, grid[tau], 0.0))
    mvs = spr_reference.full_moves(parent, tau, grid, 2)
    a = mvs[0]
    clean = 0
    for b in mvs:
        if spr_reference.touched(parent, int(a[0]), int(a[1])) & spr_reference.touched(parent, int(b[0]), int(b[1])):
            with pytest.raises(ValueError, match="share node"):
                apply_spr(tree, [a, b], grid)
        else:
            clean += 1
            assert np.array_equal(_parent_of(apply_spr(tree, [a, b], grid)), spr_reference.apply(parent, tau, [a, b])[0])
    assert clean > 0
    x, y = int(a[0]), int(a[1])
    p = int(parent[x])
    s = [c for c in range(len(parent)) if parent[c] == p and c != x][0]
    for bad, match in (((0, y), "no move"), ((1, y), "no move"), ((x, 0), "no move"), ((x, x), "no move"), ((x, p), "no move"),
                       ((x, s), "no move"), ((x, 99), "no move"), ((2, 5), "no move")):   # (2, 5): 5 lies below 2
        with pytest.raises(ValueError, match=match):
            apply_spr(tree, [bad + (60, 60, 60)], grid)
    with pytest.raises(ValueError, match="outside"):
        apply_spr(tree, [(x, y, 60, len(grid), 60)], grid)


def test_select_spr_matches_the_restatement_and_its_sets_apply_cleanly():
    from cherryml_amd.phylogeny_estimation import apply_spr, select_spr
    rng = np.random.default_rng(3)
    grid = np.asarray(bl_cases.GRID)
    for parent in (bl_cases.caterpillar(9), bl_cases.random_tree(17, np.random.default_rng(5)), nni_cases.BIN4, bl_cases.star3()):
        tau = np.where(parent >= 0, 60, -1)
        mvs = spr_reference.full_moves(parent, tau, grid, 3)
        tree = _tree(parent, np.where(tau >= 0, grid[tau], 0.0))
        for trial in range(12):
            delta = rng.normal(size=len(mvs))
            if trial % 2:
                delta = np.round(delta)            # ties, and zeros (not above min_gain)
            gain = [0.0, 0.5][trial % 3 == 0]
            got = select_spr(mvs, delta, parent, min_gain=gain)
            assert np.array_equal(got, spr_reference.select(mvs, delta, parent, gain))
            assert np.array_equal(got, select_spr(mvs[:, :2], delta, parent, min_gain=gain))  # only x and y are read
            assert np.all(delta[got] > gain) and np.all(np.diff(delta[got]) <= 0)         # ordered
            ties = np.flatnonzero(np.diff(delta[got]) == 0)
            assert np.all(got[ties] < got[ties + 1])                                      # ties: the lower index first
            sets = [spr_reference.touched(parent, int(mvs[m][0]), int(mvs[m][1])) for m in got]
            assert sum(len(t) for t in sets) == len(set().union(*sets)) if sets else True   # disjoint
            for m in set(range(len(mvs))) - set(got.tolist()):                            # greedy
                if delta[m] > gain:
                    t = spr_reference.touched(parent, int(mvs[m][0]), int(mvs[m][1]))
                    assert any(t & sets[i] and delta[k] >= delta[m] for i, k in enumerate(got))
            if len(got):                                                                  # the set applies, to one tree
                moved = apply_spr(tree, mvs[got], grid)
                assert np.array_equal(_parent_of(moved), spr_reference.apply(parent, tau, mvs[got])[0])
                assert len(moved.postorder_traversal()) == len(parent)
                assert nni_reference.splits(_parent_of(moved)) is not None
    assert len(select_spr(np.zeros((0, 5)), [], bl_cases.star3())) == 0
    with pytest.raises(ValueError, match="deltas"):
        select_spr(mvs, [1.0], parent)


# ------------------------------------------------------------------------------------------------------ the search
def test_the_restated_search_decides_everything_and_recovers_the_true_tree_in_one_move():
    """the start: SPR (x = 1, y = 16) of the true tree of nni_cases.search_family, three splits wrong.  The smallest margins
    met, relative to |log-likelihood|: 1.9e-5 among the scan's decisions, 1.6e-5 among the EM argmaxes."""
    f, r = spr_reference.search_family(), spr_reference.restated_search()
    print("restated search:", [(x["before"], x["scanned"], x["positive"], x["best"], x["selected"], x["after"]) for x in r["rounds"]],
          r["final"], "margin", r["margin"], "em margin", r["em_margin"])
    assert spr_reference.distance(f["true_parent"], *spr_reference.SEARCH_START) == 3
    assert len(nni_reference.splits(f["true_parent"]) - nni_reference.splits(f["start_parent"])) == 3
    lls = [x for rec in r["rounds"] for x in (rec["before"], rec["after"])] + [r["final"]]
    assert all(b >= a for a, b in zip(lls, lls[1:])), lls
    assert r["margin"] > MARGIN and r["em_margin"] > MARGIN, (r["margin"], r["em_margin"])
    first = r["rounds"][0]
    assert first["scanned"] == 156 and first["positive"] == 12 and abs(first["best"] - 33.07) < 0.01    # the issue's prototype
    assert abs(first["before"] + 2705.08) < 0.01 and abs(r["final"] + 2665.54) < 0.01
    assert len(first["applied"]) == 1 and r["rounds"][-1]["applied"] == [] and len(r["rounds"]) == 2   # it ended by itself
    assert nni_reference.splits(r["parent"]) == nni_reference.splits(f["true_parent"])
    assert r["final"] >= nni_cases.restated_search()["final"] - 1e-6 * abs(r["final"])   # where the NNI test ends from its start


# ------------------------------------------------------------------------------------------------------ no GPU, resources
def test_no_gpu_means_the_search_fails_loudly(tmp_path):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cherryml_amd import ml_spr_trees, nj_spr_trees
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        ml_spr_trees(tree_dir="t", msa_dir="m", site_rates_dir="s", families=["f"], rate_matrix_path="q",
                     output_tree_dir=str(tmp_path / "t"), output_likelihood_dir=str(tmp_path / "l"))
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        nj_spr_trees(msa_dir="m", families=["f"], rate_matrix_path="q", num_rate_categories=4, output_tree_dir=str(tmp_path / "t"),
                     output_site_rates_dir=str(tmp_path / "s"), output_likelihood_dir=str(tmp_path / "l"))


def test_the_exports():
    import cherryml_amd
    from cherryml_amd import phylogeny_estimation as pe
    for name in ("apply_spr", "select_spr", "ml_spr_trees", "nj_spr_trees"):
        assert name in cherryml_amd.__all__ and hasattr(cherryml_amd, name) and hasattr(pe, name)
    assert hasattr(pe, "enumerate_spr_moves") and hasattr(pe, "spr_indices")
    assert hasattr(cherryml_amd.BranchLengthFitter, "spr_scan") and hasattr(cherryml_amd.BranchLengthFitter, "spr_moves")


def test_spr_kernels_have_no_scratch_and_no_vgpr_spills():
    """the scan's kernel and the sum it shares with the NNI scan"""
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if k.startswith(("spr_scan_kernel", "nni_sum_kernel"))}
    assert {"spr_scan_kernel", "nni_sum_kernel"} <= {k.split("(")[0] for k in hits}, hits
    for name, m in hits.items():
        print(name, m)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (name, m)
