"""Neighbour joining without a GPU: `neighbor_joining` gives an additive matrix its tree back (path lengths, edge and leaf
counts, the fixed node names), clamps negative lengths, breaks ties as documented and refuses bad input; `cb_ble_pairwise`
validates every argument on the host before any device work and fails loudly with no GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nj_reference as ref  # noqa: E402
from cherryml_amd import _lib  # noqa: E402
from cherryml_amd.phylogeny_estimation import neighbor_joining  # noqa: E402


# ------------------------------------------------------------------------------------------------ additive recovery
@pytest.mark.parametrize("n", [2, 3, 4, 5, 9, 40])
def test_an_additive_matrix_gives_its_tree_back(n):
    rng = np.random.default_rng(100 + n)
    truth = ref.random_tree(n, rng)                       # edge lengths uniform in [0.05, 1]
    D = ref.path_lengths(truth, list(range(n)))
    D = np.maximum(D, D.T)
    names = [f"leaf{i}" for i in range(n)]
    tree = neighbor_joining(D, names)
    got = ref.path_lengths(ref.adjacency(tree), names)
    err = np.abs(got - D).max()
    print(f"n = {n}: worst path-length error {err:.2e} (max D {D.max():.3f})")
    assert err <= 1e-12 * D.max()
    assert sorted(tree.leaves()) == sorted(names)
    assert tree.num_edges() == (2 * n - 3 if n >= 3 else 2)
    assert tree.root() == "root"
    assert sorted(tree.internal_nodes()) == sorted(["root"] + [f"internal-{k}" for k in range(max(n - 3, 0))])
    if n >= 4:                                            # the same splits as the tree the matrix came from
        relabel = {i: names[i] for i in range(n)}
        want = {frozenset(relabel[x] for x in s) for s in ref.splits(truth, list(range(n)))}
        first = relabel[0]
        want = {s if first not in s else frozenset(names) - s for s in want}
        assert ref.splits(ref.adjacency(tree), names) == want


def test_two_leaves_hang_off_the_root_at_half_the_distance():
    tree = neighbor_joining([[0.0, 0.5], [0.5, 0.0]], ["a", "b"])
    assert tree.edges() == [("root", "a", 0.25), ("root", "b", 0.25)]


def test_internal_nodes_are_named_in_join_order():
    # ((a, b), (c, d), e): a and b, the cherry farther from the rest, are joined first, then c and d
    adj = {}
    for u, v, t in [("a", "x", 0.3), ("b", "x", 0.3), ("c", "y", 0.1), ("d", "y", 0.1), ("x", "z", 0.2), ("y", "z", 0.2),
                    ("e", "z", 1.0)]:
        adj.setdefault(u, {})[v] = t
        adj.setdefault(v, {})[u] = t
    names = list("abcde")
    D = ref.path_lengths(adj, names)
    D = np.maximum(D, D.T)
    tree = neighbor_joining(D, names)
    assert [c for c, _ in tree.children("internal-0")] == ["a", "b"]
    assert [c for c, _ in tree.children("internal-1")] == ["c", "d"]
    assert [c for c, _ in tree.children("root")] == ["e", "internal-0", "internal-1"]
    assert tree.nodes()[0] == "root"


def test_a_negative_raw_length_is_clamped_to_min_length():
    # d(a, b) = 0.1 but a is much farther from everything else than b: l_b = d/2 + (r_b - r_a) / (2 (m - 2)) < 0
    D = np.array([[0.0, 0.1, 1.0, 1.0], [0.1, 0.0, 0.2, 0.2], [1.0, 0.2, 0.0, 0.3], [1.0, 0.2, 0.3, 0.0]])
    raw = {v: t for _, v, t in neighbor_joining(D, list("abcd"), min_length=-np.inf).edges()}
    assert min(raw.values()) < 0.0
    tree = neighbor_joining(D, list("abcd"), min_length=0.03)
    got = {v: t for _, v, t in tree.edges()}
    assert min(got.values()) == 0.03
    assert all(got[v] == max(raw[v], 0.03) for v in raw)


def test_tied_minima_join_the_first_pair_of_the_active_list():
    # two equally good cherries (a, b) and (c, d): the first in (i, j) order is joined, whatever the order of the names
    D = np.array([[0, 2, 4, 4, 4], [2, 0, 4, 4, 4], [4, 4, 0, 2, 4], [4, 4, 2, 0, 4], [4, 4, 4, 4, 0]], dtype=np.float64)
    tree = neighbor_joining(D, list("abcde"))
    assert [c for c, _ in tree.children("internal-0")] == ["a", "b"]
    p = [2, 3, 0, 1, 4]                                   # (c, d) first in the list
    tree = neighbor_joining(D[np.ix_(p, p)], [list("abcde")[k] for k in p])
    assert [c for c, _ in tree.children("internal-0")] == ["c", "d"]
    # the joined node goes to the END of the active list: that list is now a, b, e, internal-0, where (a, b) ties with
    # (e, internal-0) -- the same split of four nodes -- and comes first
    assert [c for c, _ in tree.children("internal-1")] == ["a", "b"]


# ------------------------------------------------------------------------------------------------ validation
def test_neighbor_joining_refuses_bad_input():
    ok = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, 1.5], [2.0, 1.5, 0.0]])
    with pytest.raises(ValueError, match="at least two"):
        neighbor_joining([[0.0]], ["a"])
    with pytest.raises(ValueError, match="square"):
        neighbor_joining(ok[:2], ["a", "b", "c"])
    with pytest.raises(ValueError, match="square"):
        neighbor_joining(ok, ["a", "b"])
    bad = ok.copy()
    bad[0, 1] = 1.25
    with pytest.raises(ValueError, match="symmetric"):
        neighbor_joining(bad, ["a", "b", "c"])
    with pytest.raises(ValueError, match="distinct"):
        neighbor_joining(ok, ["a", "b", "a"])
    with pytest.raises(ValueError, match="own node names"):
        neighbor_joining(ok, ["a", "root", "c"])


# ------------------------------------------------------------------------------------------------ the C entry
def _pairwise(S=20, T=5, R=2, n=3, L=4, seqs=None, s2r=None, null=None):
    logP = np.zeros((T, R, max(S, 1), max(S, 1)))
    seqs = np.ascontiguousarray(np.zeros((max(n, 1), max(L, 1))) if seqs is None else seqs, dtype=np.int8)
    s2r = np.ascontiguousarray(np.zeros(max(L, 1)) if s2r is None else s2r, dtype=np.int32)
    out = np.zeros((max(n, 1), max(n, 1)), dtype=np.int32)
    ptr = dict(logP=logP.ctypes.data, seqs=seqs.ctypes.data, s2r=s2r.ctypes.data, out=out.ctypes.data)
    if null:
        ptr[null] = None
    rc = _lib.load().cb_ble_pairwise(0, S, T, R, ptr["logP"], ptr["seqs"], n, L, ptr["s2r"], ptr["out"], None)
    return rc, (_lib.load().cb_last_error() or b"").decode()


@pytest.mark.parametrize("kw,match", [
    (dict(null="logP"), "NULL"),
    (dict(null="seqs"), "NULL"),
    (dict(null="s2r"), "NULL"),
    (dict(null="out"), "NULL"),
    (dict(n=1), "n = 1"),
    (dict(n=0), "n = 0"),
    (dict(L=0), "L = 0"),
    (dict(S=1), "S = 1"),
    (dict(S=128), "S = 128"),
    (dict(seqs=[[0, 1, 2, 3], [0, 20, 2, 3], [0, 1, 2, 3]]), "state code 20"),
    (dict(seqs=[[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, -2, 3]]), "state code -2"),
    (dict(s2r=[0, 1, 2, 0]), "rate index 2"),
    (dict(s2r=[0, -1, 1, 0]), "rate index -1"),
])
def test_cb_ble_pairwise_validates_before_any_device_work(kw, match):
    rc, msg = _pairwise(**kw)
    assert rc == _lib.CB_EINVAL, (rc, msg)
    assert match in msg, msg


def test_no_gpu_means_the_pairwise_pass_fails_loudly():
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    rc, msg = _pairwise(seqs=[[0, 1, -1, 3], [0, 19, 2, 3], [-1, -1, -1, -1]], s2r=[0, 1, 1, 0])
    assert rc == _lib.CB_EHIP and "no HIP device" in msg, (rc, msg)
    from cherryml_amd.phylogeny_estimation import pairwise_branch_lengths
    with pytest.raises(_lib.CherryBankError):
        pairwise_branch_lengths(np.zeros((3, 4), np.int8), np.zeros((5, 2, 20, 20)), np.zeros(4, np.int32))


def test_the_python_face_checks_shapes_before_the_library():
    from cherryml_amd.phylogeny_estimation import pairwise_branch_lengths
    with pytest.raises(ValueError, match=r"\[n, L\]"):
        pairwise_branch_lengths(np.zeros(4, np.int8), np.zeros((5, 2, 20, 20)), np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="one rate index per site"):
        pairwise_branch_lengths(np.zeros((3, 4), np.int8), np.zeros((5, 2, 20, 20)), np.zeros(5, np.int32))


# ------------------------------------------------------------------------------------------------ resources
def test_the_pairwise_kernel_has_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if k.startswith("ble_pairwise_kernel")}
    assert len(hits) == 1, sorted(hits)
    for name, m in hits.items():
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["lds"] == 0, (name, m)
        assert m["vgpr"] <= 128, (name, m)               # four waves per SIMD (512 registers per lane)
