"""Felsenstein's bootstrap on the device, what holds without a GPU: the restatement's Philox draws against the published
known-answer vectors and against the supports' restatement, the weighted bisection against the unweighted one, the packed splits
of trees and of join records against nj_reference.splits, the root edges, the support file, `cb_boot_nj`'s refusals before any
device work, and the new kernels' resources."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import boot_reference as boot  # noqa: E402
import nj_reference as ref  # noqa: E402
import njd_reference as njd  # noqa: E402
from cherryml_amd import _lib  # noqa: E402
from cherryml_amd.io import Tree  # noqa: E402
from cherryml_amd.phylogeny_estimation import (neighbor_joining, read_bootstrap_supports, splits_of_join_records,  # noqa: E402
                                               supports_of_records, tree_splits, write_bootstrap_supports)
from conftest import load_golden  # noqa: E402
from sim_stream import philox4x32_10  # noqa: E402


def leaf_names(n):
    return [f"t{i}" for i in range(n)]


def path_matrix(adj, leaves):
    """nj_reference.path_lengths, symmetric bit for bit (the two directions of a path add its edges in different orders)"""
    D = ref.path_lengths(adj, leaves)
    return np.maximum(D, D.T)


def unpacked(packed, names):
    """packed canonical bitsets -> a set of frozensets of names"""
    bits = np.unpackbits(packed, axis=1)[:, :len(names)] if len(packed) else np.zeros((0, len(names)), dtype=np.uint8)
    assert len(packed) == 0 or not np.unpackbits(packed, axis=1)[:, len(names):].any()      # the pad bits are 0
    return {frozenset(names[k] for k in np.nonzero(row)[0]) for row in bits}


# ------------------------------------------------------------------------------------------------ the draws
def test_philox_known_answers():
    for counter, key, want in boot.PHILOX_KAT:
        got = philox4x32_10(*[np.array([c], dtype=np.uint64) for c in counter], *key)
        assert tuple(int(x[0]) for x in got) == want


def test_weights_are_the_supports_draw_rule_on_another_stream():
    import sup_reference
    for L, B, seed in ((1, 3, 5), (31, 4, 2 ** 40 + 7), (513, 5, 1)):
        W = boot.weights(L, B, seed)
        assert W.shape == (B, L) and np.all(W.sum(axis=1) == L) and W.min() >= 0
        assert np.array_equal(boot.weights(L, B, seed, tag=sup_reference.TAG), sup_reference.weights(L, B, seed))
        if L > 1:
            assert not np.array_equal(W, sup_reference.weights(L, B, seed))       # a stream of its own
        site = boot.draws(L, B, seed)                                            # draw by draw, one word at a time
        for b in range(B):
            hist = np.zeros(L, dtype=np.int64)
            for j in range(L):
                x = philox4x32_10(*[np.array([c], dtype=np.uint64) for c in (j >> 2, b, 0, boot.TAG)], seed & 0xFFFFFFFF, seed >> 32)
                s = (int(x[j & 3][0]) * L) >> 32
                assert s == site[b, j]
                hist[s] += 1
            assert np.array_equal(hist, W[b])
    # a replicate's row depends on its number, not on how many are drawn with it
    assert np.array_equal(boot.weights(65, 70, 9)[:5], boot.weights(65, 5, 9))
    assert np.array_equal(boot.weights(65, 3, 9, rep0=4), boot.weights(65, 70, 9)[4:7])


# ------------------------------------------------------------------------------------------------ the bisection
def small_family(n, L, seed):
    rng = np.random.default_rng(seed)
    rates = np.array([0.5, 2.0])
    s2r = rng.integers(0, 2, L).astype(np.int32)
    lg = np.ascontiguousarray(load_golden("data_lg.npz")["lg"], dtype=np.float64)
    tree = ref.random_tree(n, rng, length=lambda rng: rng.uniform(0.05, 0.5))
    seqs = ref.evolve(tree, n, lg, rates[s2r], rng)
    seqs[rng.random(seqs.shape) < 0.15] = -1
    grid = np.array([0.03 * 1.1 ** i for i in range(-8, 9)])
    return seqs, s2r, ref.log_bank(lg, grid, rates), grid


def test_weighted_bisection_with_unit_weights_is_the_pairwise_bisection():
    seqs, s2r, logP, _ = small_family(9, 40, 1)
    want, margin = ref.pairwise_bisection(seqs, logP, s2r)
    got, m = boot.weighted_bisection(seqs, logP, s2r, np.ones((2, 40)))
    for b in range(2):
        assert np.array_equal(got[b], want) and np.array_equal(m[b], margin)
    # a doubled alignment: every sum doubles exactly, every decision and margin stays
    got2, m2 = boot.weighted_bisection(seqs, logP, s2r, 2 * np.ones((1, 40)))
    assert np.array_equal(got2[0], want) and np.array_equal(m2[0], margin)
    # weights are multiplicities: a resampled alignment with its columns repeated gives the same indices on decided pairs
    W = boot.weights(40, 3, 11)
    got3, m3 = boot.weighted_bisection(seqs, logP, s2r, W)
    for b in range(3):
        cols = np.repeat(np.arange(40), W[b])
        mat, _ = ref.pairwise_bisection(seqs[:, cols], logP, s2r[cols])
        decided = m3[b] > 1e-9
        assert np.array_equal(mat[decided], got3[b][decided])


# ------------------------------------------------------------------------------------------------ splits
@pytest.mark.parametrize("n", [4, 5, 9, 40])
def test_packed_splits_equal_the_reference_splits(n):
    rng = np.random.default_rng(100 + n)
    names = leaf_names(n)
    for _ in range(3):
        truth = ref.random_tree(n, rng)
        D = path_matrix(truth, list(range(n)))
        want = {frozenset(names[x] for x in s) for s in ref.splits(truth, list(range(n)))}
        assert len(want) == n - 3
        tree = neighbor_joining(D, names)
        assert ref.splits(ref.adjacency(tree), names) == want                  # (an additive matrix gives its tree back)
        got = tree_splits(tree, names)
        assert got.dtype == np.uint8 and got.shape == (n - 3, (n + 7) // 8)
        assert unpacked(got, names) == want
        rec = njd.join(D)
        got = splits_of_join_records(n, rec["join_nodes"], rec["final_nodes"])
        assert got.dtype == np.uint8 and got.shape == (n - 3, (n + 7) // 8)
        assert unpacked(got, names) == want == boot.record_splits(names, rec)
        assert np.array_equal(got, tree_splits(tree, names))                    # canonical: rows unique and sorted
        # another leaf order is another canonical side, the same bipartitions
        order = [names[k] for k in rng.permutation(n)]
        assert {frozenset(s) if order[0] not in s else frozenset(names) - s for s in want} == unpacked(tree_splits(tree, order), order)


def test_two_and_three_leaves_have_no_splits():
    for n in (2, 3):
        rec = njd.join(njd.integer_matrix(n, 1))
        assert splits_of_join_records(n, rec["join_nodes"], rec["final_nodes"]).shape[0] == 0
        assert tree_splits(neighbor_joining(njd.integer_matrix(n, 1), leaf_names(n))).shape[0] == 0
    with pytest.raises(ValueError, match="joins"):
        splits_of_join_records(5, np.zeros((1, 2), dtype=np.int32), np.array([0, 1, 2]))
    with pytest.raises(ValueError, match="leaves of the tree"):
        tree_splits(neighbor_joining(njd.integer_matrix(4, 1), leaf_names(4)), ["a", "b", "c", "d"])


def rooted(edges):
    tree = Tree()
    for u, v in edges:
        for x in (u, v):
            if not tree.is_node(x):
                tree.add_node(x)
        tree.add_edge(u, v, 0.1)
    return tree


def test_root_edges_and_trivial_edges():
    # a bifurcating root: the edges above A and B are one split; C cuts off ab | cde as well as A does
    names = ["a", "b", "c", "d", "e"]
    tree = rooted([("root", "A"), ("root", "B"), ("A", "a"), ("A", "b"), ("B", "c"), ("B", "C"), ("C", "d"), ("C", "e")])
    assert unpacked(tree_splits(tree, names), names) == {frozenset("de"), frozenset("cde")} == ref.splits(ref.adjacency(tree), names)
    per_node = boot.node_splits(tree, names)
    assert [(v, real) for v, _, real in per_node] == [("A", True), ("B", True), ("C", True)]
    assert per_node[0][1] == per_node[1][1] == frozenset("cde")
    # replicates: two trees with (ab | cde, abc | de), one with (ab | cde, abd | ce)
    with_de = njd.join(path_matrix(ref.adjacency(tree), names))
    other = rooted([("root", "A"), ("root", "B"), ("A", "a"), ("A", "b"), ("B", "d"), ("B", "C"), ("C", "c"), ("C", "e")])
    with_ce = njd.join(path_matrix(ref.adjacency(other), names))
    assert boot.record_splits(names, with_ce) == {frozenset("ce"), frozenset("cde")}
    records = [(r["join_nodes"], r["join_len"], r["final_nodes"], r["final_D"]) for r in (with_de, with_ce, with_de)]
    nodes, support = supports_of_records(tree, names, records)
    assert [tree.nodes()[v] for v in nodes] == ["A", "B", "C"]
    assert support.tolist() == [1.0, 1.0, 2 / 3]                               # A and B: the same number
    # the root's child next to a single leaf: its edge is in every tree
    tree = rooted([("root", "a"), ("root", "X"), ("X", "b"), ("X", "Y"), ("Y", "c"), ("Y", "d")])
    nodes, support = supports_of_records(tree, ["a", "b", "c", "d"], [(np.array([[2, 3]], dtype=np.int32), None,
                                                                       np.array([0, 1, 4], dtype=np.int32), None)])
    assert [tree.nodes()[v] for v in nodes] == ["X", "Y"] and support.tolist() == [1.0, 1.0]
    nodes, support = supports_of_records(tree, ["a", "b", "c", "d"], [(np.array([[1, 3]], dtype=np.int32), None,
                                                                       np.array([0, 2, 4], dtype=np.int32), None)])
    assert support.tolist() == [1.0, 0.0]
    with pytest.raises(ValueError, match="at least one replicate"):
        supports_of_records(tree, ["a", "b", "c", "d"], [])


def test_support_file_round_trip(tmp_path):
    tree = rooted([("root", "A"), ("root", "B"), ("A", "a"), ("A", "b"), ("B", "c"), ("B", "C"), ("C", "d"), ("C", "e")])
    nodes = np.array([k for k, v in enumerate(tree.nodes()) if v in "ABC"])
    support = np.array([1.0, 1.0, 37 / 50])
    path = str(tmp_path / "f.txt")
    write_bootstrap_supports(path, tree.nodes(), nodes, support)
    lines = open(path).read().split("\n")
    assert lines[0] == "node bootstrap" and [ln.split()[0] for ln in lines[1:] if ln] == ["A", "B", "C"]
    assert read_bootstrap_supports(path) == {"A": 1.0, "B": 1.0, "C": 37 / 50}    # (repr round-trips a float64)
    (tmp_path / "g.txt").write_text("node alrt sh rell\n")
    with pytest.raises(ValueError, match="not a bootstrap-support file"):
        read_bootstrap_supports(str(tmp_path / "g.txt"))


# ------------------------------------------------------------------------------------------------ the C entry
def test_the_header_declares_and_the_binding_lists_cb_boot_nj():
    header = open(os.path.join(ROOT, "include", "cherrybank.h")).read()
    assert "int cb_boot_nj(int device, int S, int T, int R, const double *logP, const double *grid, const int8_t *seqs, int n, int L," in header
    assert "cb_boot_nj" in _lib.SIGNATURES and len(_lib.SIGNATURES["cb_boot_nj"][1]) == 20
    assert hasattr(_lib.load(), "cb_boot_nj")


def _boot_nj(null=None, logP=None, grid=None, seqs=None, s2r=None, weights=None, **sizes):
    """a call on a small valid problem (S = 4, T = 5, R = 2, n = 4, L = 6, n_rep = 3) with what the case changes"""
    z = dict(S=4, T=5, R=2, n=4, L=6, n_rep=3)
    rng = np.random.default_rng(0)
    P = rng.random((5, 2, 4, 4)) + 0.1
    arr = dict(logP=np.log(P / P.sum(axis=3, keepdims=True)) if logP is None else logP,
               grid=np.array([0.1, 0.2, 0.4, 0.8, 1.6]) if grid is None else np.asarray(grid, dtype=np.float64),
               seqs=rng.integers(-1, 4, (4, 6)).astype(np.int8) if seqs is None else np.asarray(seqs, dtype=np.int8),
               s2r=rng.integers(0, 2, 6).astype(np.int32) if s2r is None else np.asarray(s2r, dtype=np.int32),
               join_nodes=np.zeros((3, 2), np.int32), join_len=np.zeros((3, 2)), final_nodes=np.zeros((3, 3), np.int32),
               final_D=np.zeros((3, 9)))
    arr = {k: np.ascontiguousarray(v) for k, v in arr.items()}
    ptr = {k: v.ctypes.data for k, v in arr.items()}
    if weights is not None:
        arr["weights"] = np.ascontiguousarray(weights, dtype=np.float64)
    ptr["weights"] = arr["weights"].ctypes.data if weights is not None else None
    if null:
        ptr[null] = None
    z.update(sizes)
    rc = _lib.load().cb_boot_nj(0, z["S"], z["T"], z["R"], ptr["logP"], ptr["grid"], ptr["seqs"], z["n"], z["L"], ptr["s2r"], z["n_rep"],
                                7, ptr["weights"], ptr["join_nodes"], ptr["join_len"], ptr["final_nodes"], ptr["final_D"], None, None,
                                None)
    return rc, (_lib.load().cb_last_error() or b"").decode()


def _bank_with(value):
    P = np.full((5, 2, 4, 4), np.log(0.25))
    P[3, 1, 2, 0] = value
    return P


def _seqs_with(value):
    s = np.zeros((4, 6), dtype=np.int8)
    s[2, 5] = value
    return s


def _weights_with(value):
    W = np.ones((3, 6))
    W[1, 4] = value
    return W


REFUSALS = [(dict(null=k), "NULL") for k in ("logP", "grid", "seqs", "s2r", "join_nodes", "join_len", "final_nodes", "final_D")] + [
    (dict(n=1), "n = 1 sequences"),
    (dict(L=0), "L = 0 sites"),
    (dict(S=1), "S = 1 states"),
    (dict(S=128), "S = 128 states"),
    (dict(T=0), "T = 0 grid points"),
    (dict(R=0), "R = 0 rate categories"),
    (dict(T=2000), "T = 2000 grid points (at most 1024)"),
    (dict(R=140000, S=127), "R = 140000 rate categories"),
    (dict(n=50000), "n = 50000 sequences: the matrix"),
    (dict(n_rep=0), "n_rep = 0 replicates"),
    (dict(n_rep=-3), "n_rep = -3 replicates"),
    (dict(seqs=_seqs_with(4)), "state code 4 out of range (sequence 2, site 5)"),
    (dict(seqs=_seqs_with(-2)), "state code -2 out of range (sequence 2, site 5)"),
    (dict(s2r=[0, 1, 0, 2, 0, 0]), "rate index 2 out of range (site 3)"),
    (dict(s2r=[0, 1, 0, 0, -1, 0]), "rate index -1 out of range (site 4)"),
    (dict(grid=[0.1, 0.2, np.nan, 0.8, 1.6]), "grid[2] = nan"),
    (dict(grid=[0.1, 0.2, 0.4, 0.8, np.inf]), "grid[4] = inf"),
    (dict(grid=[0.0, 0.2, 0.4, 0.8, 1.6]), "grid[0] = 0"),
    (dict(grid=[-0.1, 0.2, 0.4, 0.8, 1.6]), "grid[0] = -0.1"),
    (dict(grid=[0.1, 0.2, 0.2, 0.8, 1.6]), "grid[2] = 0.2"),
    (dict(grid=[0.1, 0.2, 0.4, 0.3, 1.6]), "grid[3] = 0.3"),
    (dict(logP=_bank_with(-np.inf)), "logP entry 120 = -inf"),
    (dict(logP=_bank_with(np.nan)), "logP entry 120 = nan"),
    (dict(logP=_bank_with(np.inf)), "logP entry 120 = inf"),
    (dict(weights=_weights_with(-1.0)), "weights[1][4] = -1"),
    (dict(weights=_weights_with(np.nan)), "weights[1][4] = nan"),
    (dict(weights=_weights_with(np.inf)), "weights[1][4] = inf"),
    (dict(weights=_weights_with(0.5)), "weights[1][4] = 0.5"),
]


@pytest.mark.parametrize("kw,match", REFUSALS, ids=[f"{sorted(k)[0]}-{m}" for k, m in REFUSALS])
def test_cb_boot_nj_validates_before_any_device_work(kw, match):
    rc, msg = _boot_nj(**kw)
    assert rc == _lib.CB_EINVAL, (rc, msg)
    assert msg.startswith("cb_boot_nj") and match in msg, msg


def test_no_gpu_means_the_bootstrap_fails_loudly(tmp_path):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cherryml_amd import bootstrap_nj_records, nj_bootstrap_supports
    rc, msg = _boot_nj()
    assert rc == _lib.CB_EHIP and "no HIP device" in msg, (rc, msg)
    rc, msg = _boot_nj(weights=np.ones((3, 6)))
    assert rc == _lib.CB_EHIP and "no HIP device" in msg, (rc, msg)
    seqs, s2r, logP, grid = small_family(5, 12, 2)
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        bootstrap_nj_records(seqs, logP, s2r, grid, 4, 1)
    with pytest.raises(ValueError, match="n_rep = 0"):
        bootstrap_nj_records(seqs, logP, s2r, grid, 0, 1)
    with pytest.raises(ValueError, match=r"weights must be \[num_replicates, L\]"):
        bootstrap_nj_records(seqs, logP, s2r, grid, 4, 1, weights=np.ones((3, 12)))
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        nj_bootstrap_supports(tree_dir=str(tmp_path), msa_dir=str(tmp_path), site_rates_dir=str(tmp_path), families=["f"],
                              rate_matrix_path=str(tmp_path / "q.txt"), output_support_dir=str(tmp_path / "s"))


def test_the_stage_is_exported_and_cached():
    import inspect

    import cherryml_amd
    for name in ("bootstrap_nj_records", "bootstrap_supports", "nj_bootstrap_supports", "splits_of_join_records", "tree_splits"):
        assert name in cherryml_amd.__all__ and hasattr(cherryml_amd, name)
    sig = inspect.signature(cherryml_amd.nj_bootstrap_supports).parameters
    assert sig["num_replicates"].default == 100 and sig["random_seed"].default == 0 and sig["quantization_grid_num_steps"].default == 64
    with pytest.raises(ValueError, match="output_support_dir is required"):
        cherryml_amd.nj_bootstrap_supports(tree_dir="t", msa_dir="m", site_rates_dir="s", families=["f"], rate_matrix_path="q")


# ------------------------------------------------------------------------------------------------ resources
def test_the_new_kernels_have_no_scratch_and_stay_within_the_lds_limit():
    sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    meta = kernel_meta()
    for kernel in ("boot_weights_kernel", "boot_pairwise_kernel"):
        hits = {k: v for k, v in meta.items() if k.startswith(kernel)}
        assert len(hits) == 1, (kernel, sorted(hits))
        for name, m in hits.items():
            print(name, m)
            assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)
            assert 0 < m["lds"] <= 64 << 10, (name, m)          # the static limit of a workgroup
            # 42 KiB of LDS let three workgroups share a CU, three waves a SIMD: 512 / 3 registers (in eights) keep that
            assert m["vgpr"] <= 168, (name, m)
    for kernel in ("nj_rowsum_kernel", "nj_argmin_kernel", "nj_join_kernel"):   # the joins: compiled once, in cb_nj.hip
        assert len([k for k in meta if k.startswith(kernel)]) == 1
