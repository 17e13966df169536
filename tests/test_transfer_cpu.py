"""The transfer bootstrap, what holds without a GPU: the restatement tests/transfer_reference.py on a hand-worked example and its
properties on random trees, the declaration, binding and export of `cb_transfer_support`, its refusals before any device work,
the behaviour without a device, the Python exports, the support file, and the new kernels' resources."""
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import transfer_reference as tr  # noqa: E402
from cherryml_amd import _lib  # noqa: E402
from cherryml_amd.io import Tree  # noqa: E402
from cherryml_amd.phylogeny_estimation import (read_transfer_supports, supports_of_records, transfer_distances,  # noqa: E402
                                               transfer_supports_of_records, write_transfer_supports)

CASES, CHAIN_SLACK = tr.CASES, tr.CHAIN_SLACK


def rows(*leaf_sets, n=6):
    out = np.zeros((len(leaf_sets), n), dtype=bool)
    for r, s in enumerate(leaf_sets):
        out[r, list(s)] = True
    return out


def as_tree(adj, n):
    """the adjacency dict as a Tree rooted at the internal node n: leaf k is `t<k>`"""
    name = {u: (f"t{u}" if u < n else f"i{u}") for u in adj}
    tree = Tree()
    tree.add_node(name[n])
    stack, seen = [n], {n}
    while stack:
        u = stack.pop()
        for v in sorted(adj[u]):
            if v not in seen:
                seen.add(v)
                tree.add_node(name[v])
                tree.add_edge(name[u], name[v], 0.1)
                stack.append(v)
    return tree, [f"t{k}" for k in range(n)]


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_hand_worked_six_leaves():
    a, b, c, d, e, f = range(6)
    ref = rows({a, b}, {c, d}, {e, f})                                          # ((a,b),(c,d),(e,f))
    other = np.array([[a, c], [6, b], [d, e]], dtype=np.int32)                   # (((a,c),b),((d,e),f)): {ac}, {abc}, {de}
    same = np.array([[a, b], [c, d], [e, f]], dtype=np.int32)
    assert tr.leaf_sets(6, other).tolist() == rows({a, c}, {a, b, c}, {d, e}).tolist()
    got = tr.distances(ref, 6, np.stack([other, same]))
    # {ab}: 2 from {ac}, 1 from {abc}, min(4, 2) from {de};  {cd}: 2, 3, 2 -- clamped to p - 1 = 1;  {ef}: 2, min(5, 1), 2
    assert got["raw"].tolist() == [[1, 0], [2, 0], [1, 0]] and got["p"].tolist() == [2, 2, 2]
    assert got["min_dist"].tolist() == [[1, 0], [1, 0], [1, 0]]
    assert got["sum_dist"].tolist() == [1, 1, 1] and got["present"].tolist() == [1, 1, 1]
    bootstrap, transfer = tr.supports(got["sum_dist"], got["present"], got["p"], 2)
    assert bootstrap.tolist() == [0.5, 0.5, 0.5] and transfer.tolist() == [0.5, 0.5, 0.5]
    alone = tr.distances(ref, 6, other[None])
    assert alone["min_dist"][:, 0].tolist() == [1, 1, 1]                         # delta = 1 = p - 1
    assert tr.supports(alone["sum_dist"], alone["present"], alone["p"], 1)[1].tolist() == [0.0, 0.0, 0.0]
    assert tr.distances(ref, 6, same[None])["min_dist"].tolist() == [[0], [0], [0]]
    assert tr.final_nodes(6, other).tolist() == [5, 7, 8] and tr.final_nodes(6, same).tolist() == [6, 7, 8]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_every_gpu_case_holds_zeros_clamped_values_and_unclamped_minima(case):
    n, n_ref, n_rep = case
    ref, joins = tr.make_case(*case)
    assert ref.shape == (n_ref, n) and joins.shape == (n_rep, n - 3, 2) and joins.dtype == np.int32
    got = tr.distances(ref, n, joins)
    raw, p = got["raw"], got["p"][:, None]
    assert (raw == 0).any() and (raw > p - 1).any()                              # exact matches; the clamp is active
    assert ((raw > 0) & (raw < p - 1)).any() == (n >= 8)                         # minima the clamp leaves alone
    assert got["min_dist"].max() <= (p - 1).max() and got["min_dist"].min() == 0
    if n_rep >= 3:                                                               # a copy of the reference: every split is there
        assert np.all(got["min_dist"][:, 2::3] == 0) and not np.all(got["min_dist"][:, 1::3] == 0)
    assert len({r.tobytes() for r in ref}) == n_ref
    sides = ref[:, 0]
    assert n_ref < 4 or (sides.any() and not sides.all())                        # both sides are given


def test_properties_on_random_trees():
    for n, B, seed in ((4, 3, 0), (7, 6, 1), (12, 9, 2), (40, 7, 3)):
        rng = np.random.default_rng(seed)
        adj = tr.random_topology(n, rng)
        tree, names = as_tree(adj, n)
        ref = tr.leaf_sets(n, tr.join_records(adj, n, rng))
        joins = np.stack([tr.join_records(o, n, rng) for o in
                          [adj, tr.move_leaves(adj, [int(rng.integers(n))], rng)] + [tr.random_topology(n, rng) for _ in range(B - 2)]])
        got = tr.distances(ref, n, joins)
        flipped = tr.distances(~ref, n, joins)
        for k in ("raw", "min_dist", "sum_dist", "present", "p"):
            assert np.array_equal(got[k], flipped[k]), k                          # the other side of every split
        bootstrap, transfer = tr.supports(got["sum_dist"], got["present"], got["p"], B)
        # 0 <= bootstrap <= transfer <= 1, exactly, over the common denominator B (p - 1) ...
        full = B * (got["p"] - 1)
        assert np.all((0 <= got["present"]) & (got["present"] * (got["p"] - 1) <= full - got["sum_dist"]) & (got["sum_dist"] >= 0))
        # ... and in float64 up to the three roundings of the two expressions (two divisions and a difference of numbers <= 1)
        assert np.all((0 <= bootstrap) & (bootstrap <= transfer + CHAIN_SLACK) & (transfer <= 1))
        assert np.all(got["min_dist"][:, 0] == 0) and np.all(bootstrap >= 1 / B)    # the tree itself is replicate 0
        # the exact matches are Felsenstein's count
        records = [(j, None, tr.final_nodes(n, j), None) for j in joins]
        nodes, support = supports_of_records(tree, names, records)
        below = {frozenset(np.nonzero(r)[0]): k / B for r, k in zip(ref, got["present"])}
        below.update({frozenset(range(n)) - s: v for s, v in list(below.items())})
        leaves_below = {}
        for v in tree.postorder_traversal():
            leaves_below[v] = frozenset([int(v[1:])]) if tree.is_leaf(v) else frozenset().union(*[leaves_below[c] for c, _ in tree.children(v)])
        assert len(nodes) == n - 3
        assert support.tolist() == [below[leaves_below[tree.nodes()[int(v)]]] for v in nodes]


def test_fewer_than_four_leaves_need_no_device():
    tree = Tree()
    for v in ("r", "a", "X", "b", "c"):
        tree.add_node(v)
    for u, v in (("r", "a"), ("r", "X"), ("X", "b"), ("X", "c")):
        tree.add_edge(u, v, 0.1)
    record = (np.zeros((0, 2), dtype=np.int32), None, np.array([0, 1, 2], dtype=np.int32), None)
    nodes, bootstrap, transfer = transfer_supports_of_records(tree, ["a", "b", "c"], [record, record])
    assert [tree.nodes()[int(v)] for v in nodes] == ["X"] and bootstrap.tolist() == [1.0] and transfer.tolist() == [1.0]
    with pytest.raises(ValueError, match="at least one replicate"):
        transfer_supports_of_records(tree, ["a", "b", "c"], [])
    with pytest.raises(ValueError, match="leaves of the tree"):
        transfer_supports_of_records(tree, ["a", "b", "d"], [record])


# ------------------------------------------------------------------------------------------------ the C entry
def test_the_header_declares_and_the_binding_lists_cb_transfer_support():
    header = open(os.path.join(ROOT, "include", "cherrybank.h")).read()
    assert ("int cb_transfer_support(int device, int n, int n_ref, const uint8_t *ref_sets, int n_rep, const int *join_nodes, "
            "int *min_dist,") in header
    assert "cb_transfer_support" in _lib.SIGNATURES and len(_lib.SIGNATURES["cb_transfer_support"][1]) == 10
    assert hasattr(_lib.load(), "cb_transfer_support")


SAME = [[0, 1], [2, 3], [4, 5]]


def _transfer(null=None, ref=(0b11000000, 0b00110000), joins=(SAME, SAME), **sizes):
    """a call on a small valid problem (n = 6, n_ref = 2, n_rep = 2) with what the case changes"""
    z = dict(n=6, n_ref=2, n_rep=2)
    z.update(sizes)
    arr = dict(ref_sets=np.array(ref, dtype=np.uint8).reshape(-1, 1), join_nodes=np.array(joins, dtype=np.int32),
               sum_dist=np.zeros(8, dtype=np.int64), present=np.zeros(8, dtype=np.int32), min_dist=np.zeros(64, dtype=np.int32))
    arr = {k: np.ascontiguousarray(v) for k, v in arr.items()}
    ptr = {k: v.ctypes.data for k, v in arr.items()}
    if null:
        ptr[null] = None
    rc = _lib.load().cb_transfer_support(0, z["n"], z["n_ref"], ptr["ref_sets"], z["n_rep"], ptr["join_nodes"], ptr["min_dist"],
                                         ptr["sum_dist"], ptr["present"], None)
    return rc, (_lib.load().cb_last_error() or b"").decode()


REFUSALS = [(dict(null=k), f"{k} is NULL") for k in ("ref_sets", "join_nodes", "sum_dist", "present")] + [
    (dict(n=3), "n = 3 leaves"),
    (dict(n=-1), "n = -1 leaves"),
    (dict(n=50000), "n = 50000 leaves: the matrix"),
    (dict(n_ref=0), "n_ref = 0 reference sets"),
    (dict(n_rep=0), "n_rep = 0 replicates"),
    (dict(n_rep=-3), "n_rep = -3 replicates"),
    (dict(ref=(0b11000000, 0b00110001)), "ref_sets[1]: pad bit set (byte 0 = 0x31"),
    (dict(ref=(0b11000010, 0b00110000)), "ref_sets[0]: pad bit set (byte 0 = 0xc2"),
    (dict(ref=(0b11000000, 0b00000000)), "ref_sets[1] holds 0 of 6 leaves"),
    (dict(ref=(0b11111100, 0b00110000)), "ref_sets[0] holds 6 of 6 leaves"),
    (dict(ref=(0b11000000, 0b00000100)), "ref_sets[1] holds 1 of 6 leaves"),
    (dict(ref=(0b11000000, 0b11011100)), "ref_sets[1] holds 5 of 6 leaves"),
    (dict(joins=(SAME, [[0, 1], [2, -1], [4, 5]])), "join_nodes[1][1][1] = -1 outside [0, 7)"),
    (dict(joins=([[6, 1], [2, 3], [4, 5]], SAME)), "join_nodes[0][0][0] = 6 outside [0, 6)"),
    (dict(joins=(SAME, [[0, 1], [2, 3], [8, 5]])), "join_nodes[1][2][0] = 8 outside [0, 8)"),
    (dict(joins=(SAME, [[0, 1], [2, 3], [4, 11]])), "join_nodes[1][2][1] = 11 outside [0, 8)"),
    (dict(joins=([[0, 1], [2, 0], [4, 5]], SAME)), "join_nodes[0][1][1] = 0 is a member twice"),
    (dict(joins=(SAME, [[0, 1], [6, 2], [6, 3]])), "join_nodes[1][2][0] = 6 is a member twice"),
    (dict(joins=(SAME, [[0, 1], [2, 2], [4, 5]])), "join_nodes[1][1][1] = 2 is a member twice"),
]


@pytest.mark.parametrize("kw,match", REFUSALS, ids=[f"{sorted(k)[0]}-{m}" for k, m in REFUSALS])
def test_cb_transfer_support_validates_before_any_device_work(kw, match):
    rc, msg = _transfer(**kw)
    assert rc == _lib.CB_EINVAL, (rc, msg)
    assert msg.startswith("cb_transfer_support") and match in msg, msg


def test_the_python_face_raises_what_the_library_refuses():
    ref = np.array([[0b11000000], [0b00110000]], dtype=np.uint8)
    joins = np.array([SAME, SAME], dtype=np.int32)
    with pytest.raises(ValueError, match=r"ref_sets must be \[n_ref, ceil\(n / 8\)\]"):
        transfer_distances(np.zeros((2, 2), dtype=np.uint8), 6, joins)
    with pytest.raises(ValueError, match=r"join_nodes must be \[n_rep, n - 3, 2\]"):
        transfer_distances(ref, 6, joins[:, :2])
    with pytest.raises(ValueError, match="cb_transfer_support: n_rep = 0 replicates"):
        transfer_distances(ref, 6, joins[:0])
    with pytest.raises(ValueError, match=r"ref_sets\[1\] holds 1 of 6 leaves"):
        transfer_distances(np.array([[0b11000000], [0b00100000]], dtype=np.uint8), 6, joins)
    bad = joins.copy()
    bad[1, 2, 0] = 1
    with pytest.raises(ValueError, match=r"join_nodes\[1\]\[2\]\[0\] = 1 is a member twice"):
        transfer_distances(ref, 6, bad)


def test_no_gpu_means_the_transfer_bootstrap_fails_loudly(tmp_path):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cherryml_amd import nj_transfer_supports
    rc, msg = _transfer()
    assert rc == _lib.CB_EHIP and msg.startswith("cb_transfer_support") and "no HIP device" in msg, (rc, msg)
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        transfer_distances(np.array([[0b11000000]], dtype=np.uint8), 6, np.array([SAME], dtype=np.int32))
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        transfer_distances(np.array([[0b11000000]], dtype=np.uint8), 6, np.array([SAME], dtype=np.int32), per_replicate=True, profile={})
    with pytest.raises(_lib.CherryBankError, match="nj_transfer_supports: no HIP device"):
        nj_transfer_supports(tree_dir=str(tmp_path), msa_dir=str(tmp_path), site_rates_dir=str(tmp_path), families=["f"],
                             rate_matrix_path=str(tmp_path / "q.txt"), output_support_dir=str(tmp_path / "s"))


def test_the_stage_is_exported_with_its_siblings_signature():
    import cherryml_amd
    from cherryml_amd import phylogeny_estimation
    for name in ("transfer_distances", "transfer_supports_of_records", "transfer_bootstrap_supports", "nj_transfer_supports",
                 "read_transfer_supports", "write_transfer_supports"):
        assert name in cherryml_amd.__all__ and hasattr(cherryml_amd, name) and hasattr(phylogeny_estimation, name)
    new = inspect.signature(cherryml_amd.nj_transfer_supports).parameters
    old = inspect.signature(cherryml_amd.nj_bootstrap_supports).parameters
    assert list(new) == list(old) and all(new[k].default == old[k].default for k in new)
    assert new["num_replicates"].default == 100 and new["random_seed"].default == 0
    with pytest.raises(ValueError, match="output_support_dir is required"):
        cherryml_amd.nj_transfer_supports(tree_dir="t", msa_dir="m", site_rates_dir="s", families=["f"], rate_matrix_path="q")
    face = inspect.signature(transfer_distances).parameters
    assert list(face) == ["ref_sets", "n", "join_nodes", "device", "profile", "per_replicate"]
    assert face["device"].default == 0 and face["profile"].default is None and face["per_replicate"].default is False
    assert list(inspect.signature(transfer_supports_of_records).parameters)[:3] == ["tree", "names", "records"]
    assert list(inspect.signature(cherryml_amd.transfer_bootstrap_supports).parameters) == [
        "tree", "names", "seqs", "logP", "site_to_rate", "grid", "num_replicates", "seed", "weights", "device", "profile"]


def test_support_file_round_trip(tmp_path):
    names = ["root", "A", "a", "b", "B", "c", "C", "d", "e"]
    nodes = np.array([1, 4, 6])
    path = str(tmp_path / "f.txt")
    write_transfer_supports(path, names, nodes, np.array([1.0, 1.0, 37 / 50]), np.array([1.0, 1.0, 1.0 - 13 / (50 * 2)]))
    lines = open(path).read().split("\n")
    assert lines[0] == "node bootstrap transfer" and [ln.split()[0] for ln in lines[1:] if ln] == ["A", "B", "C"]
    assert lines[3] == f"C {37 / 50!r} {1.0 - 13 / 100!r}"
    assert read_transfer_supports(path) == {"A": (1.0, 1.0), "B": (1.0, 1.0), "C": (37 / 50, 1.0 - 13 / 100)}    # (repr round-trips)
    (tmp_path / "g.txt").write_text("node bootstrap\nA 1.0\n")
    with pytest.raises(ValueError, match="not a transfer-support file"):
        read_transfer_supports(str(tmp_path / "g.txt"))


# ------------------------------------------------------------------------------------------------ resources
def test_the_new_kernels_have_no_scratch_and_stay_within_the_lds_limit():
    sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    meta = kernel_meta()
    for kernel in ("tb_sets_kernel", "tb_distance_kernel"):
        hits = {k: v for k, v in meta.items() if k.startswith(kernel)}
        assert len(hits) == 1, (kernel, sorted(hits))
        for name, m in hits.items():
            print(name, m)
            assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (name, m)
            assert 0 <= m["lds"] <= 64 << 10, (name, m)          # the static limit of a workgroup
    (dist,) = [m for k, m in meta.items() if k.startswith("tb_distance_kernel")]
    assert dist["lds"] > 0
    assert dist["vgpr"] <= 128, dist                              # two workgroups of four waves a CU at least
