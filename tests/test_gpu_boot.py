"""Felsenstein's bootstrap on the GPU (`cb_boot_nj`: csrc/boot.hip.h and the join kernels of csrc/nj.hip.h) against the NumPy
restatement tests/boot_reference.py: the drawn weights, the grid indices of every replicate and pair, the existing distance pass,
the joins, the independence of a replicate from the call it is in, the supports and the stage.

Exactness.  Weights, indices, join records and supports are compared exactly.  The restatement records per replicate and pair the
smallest |a - b| / max(|a|, |b|) the bisection met; an entry is UNDECIDED when that is <= 1e-9 (the order of summation moves the
sums by ~1e-13 relative) and is left out of the comparison of the indices, at most 1 % of the off-diagonal entries of a case; an
entry with no commonly observed site of positive weight compares 0 > 0 at every step: decided, index T - 1.  With the seeds below,
found on the CPU with a bank by eigendecomposition, the smallest margin over all cases is 8.3e-11 (case 37x64x64, its one
undecided entry of 42624; the next case, 37x513x17, has 6.6e-08 and none undecided); the supports family (12 x 300, 50
replicates) has smallest margin 3.1e-07, and its joins with more than four active nodes are decided by 1.2e-04 at least.
Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boot_reference as boot  # noqa: E402
import nj_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = {129: np.array([0.03 * 1.1 ** i for i in range(-64, 65)]), 64: np.array([0.03 * 1.1 ** i for i in range(-32, 32)])}
RATES = np.array([0.25, 0.6, 1.2, 2.5])
UNDECIDED = 1e-9
# (n, L, B, T, explicit weights?)
CASES = [(37, 513, 17, 129, False), (9, 65, 65, 64, False), (4, 33, 16, 129, True), (2, 1, 1, 64, False), (3, 31, 15, 64, True),
         (37, 64, 64, 129, True), (9, 32, 1, 64, False)]
SEED = 20
FIELDS = ("join_nodes", "join_len", "final_nodes", "final_D")


def case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-T{c[3]}-{'given' if c[4] else 'drawn'}"


def lg():
    return np.ascontiguousarray(load_golden("data_lg.npz")["lg"], dtype=np.float64)


def family(n, L):
    """test_gpu_nj.family: sequences evolved down a random tree from LG's stationary distribution at the four rates, 15 % gaps;
    sequence 1 is a copy of sequence 0 and the last sequence is all gaps (n = 2: the all-gap sequence alone)"""
    rng = np.random.default_rng(1000 * n + L)
    s2r = rng.integers(0, len(RATES), L).astype(np.int32)
    tree = ref.random_tree(n, rng, length=lambda rng: rng.uniform(0.02, 0.4))
    seqs = ref.evolve(tree, n, lg(), RATES[s2r], rng)
    seqs[rng.random(seqs.shape) < 0.15] = -1
    if n > 2:
        seqs[1] = seqs[0]
    seqs[n - 1] = -1
    return seqs, s2r


def given_weights(L, B):
    """multiplicities of no particular sum: 0 .. 3 per site; the last replicate of several draws nothing at all"""
    W = np.random.default_rng(7 * L + B).integers(0, 4, (B, L)).astype(np.float64)
    if B > 1:
        W[B - 1] = 0.0
    return W


def case_inputs(case):
    n, L, B, T, given = case
    seqs, s2r = family(n, L)
    return seqs, s2r, (given_weights(L, B) if given else boot.weights(L, B, SEED).astype(np.float64))


@functools.lru_cache(maxsize=None)
def banks(T):
    from cherryml_amd.phylogeny_estimation import compute_log_transition_matrices
    return compute_log_transition_matrices(lg(), GRIDS[T], RATES)


@functools.lru_cache(maxsize=None)
def restated(case):
    """(index [B, n, n], margin [B, n, n]) of the case by the restatement, once for all tests"""
    seqs, s2r, W = case_inputs(case)
    return boot.weighted_bisection(seqs, banks(case[3]), s2r, W)


@functools.lru_cache(maxsize=None)
def device(case):
    """(records, index, weights) of the case from the device, once for all tests"""
    from cherryml_amd.phylogeny_estimation import bootstrap_nj_records
    n, L, B, T, given = case
    seqs, s2r, W = case_inputs(case)
    prof = {}
    out = bootstrap_nj_records(seqs, banks(T), s2r, GRIDS[T], B, SEED, weights=W if given else None, profile=prof,
                               return_index=True, return_weights=True)
    assert prof["distance_kernel_ms"] > 0.0 and (given or prof["weights_kernel_ms"] > 0.0) and (n <= 3 or prof["join_kernel_ms"] > 0.0)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. weights
def test_drawn_weights_equal_the_restatement():
    from cherryml_amd.phylogeny_estimation import bootstrap_nj_records
    seqs, s2r = family(4, 65)
    rows = {}
    for B in (1, 17, 70):
        _, W = bootstrap_nj_records(seqs, banks(64), s2r, GRIDS[64], B, 9, return_weights=True)
        assert W.shape == (B, 65) and W.dtype == np.float64
        assert np.array_equal(W, boot.weights(65, B, 9)) and np.all(W.sum(axis=1) == 65)
        rows[B] = W
    assert np.array_equal(rows[1], rows[70][:1]) and np.array_equal(rows[17], rows[70][:17])
    _, other = bootstrap_nj_records(seqs, banks(64), s2r, GRIDS[64], 17, 10, return_weights=True)
    assert np.array_equal(other, boot.weights(65, 17, 10)) and not np.any(np.all(other == rows[17], axis=1))
    seqs, s2r = family(4, 513)                                  # more draws than threads
    _, W = bootstrap_nj_records(seqs, banks(64), s2r, GRIDS[64], 3, 2 ** 40 + 5, return_weights=True)
    assert np.array_equal(W, boot.weights(513, 3, 2 ** 40 + 5))


# ------------------------------------------------------------------------------------------------ 2. indices
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_indices_equal_the_restatement(case):
    n, L, B, T, given = case
    seqs, s2r, W = case_inputs(case)
    records, got, w_out = device(case)
    want, margin = restated(case)
    off = ~np.eye(n, dtype=bool)[None, :, :].repeat(B, axis=0)
    decided = (margin > UNDECIDED) & off
    print(f"{case_id(case)}: smallest margin {margin[off].min():.2e}, undecided {int((~decided & off).sum()) // 2} of "
          f"{B * n * (n - 1) // 2} entries, mismatches on decided entries {int((got != want)[decided].sum()) // 2}")
    assert np.array_equal(w_out, W)
    assert got.dtype == np.int32 and got.shape == (B, n, n)
    assert np.array_equal(got, got.transpose(0, 2, 1)) and np.all(got[:, np.arange(n), np.arange(n)] == -1)
    assert (~decided & off).sum() <= 0.01 * off.sum()
    assert np.array_equal(got[decided], want[decided])
    # no commonly observed site of positive weight: decided, T - 1
    obs = (seqs >= 0).astype(np.float64)
    common = np.einsum("bl,il,jl->bij", W, obs, obs)
    empty = (common == 0) & off
    assert empty.any() and np.all(margin[empty] == np.inf) and np.all(got[empty] == T - 1)
    if n > 2:                                                   # the copy: identical sequences are at the grid's first point
        seen = common[:, 0, 1] > 0
        assert np.all(got[seen, 0, 1] == 0) and np.all(decided[seen, 0, 1])


# ------------------------------------------------------------------------------------------------ 3. the code that exists
def test_unit_weights_give_the_pairwise_kernels_indices():
    from cherryml_amd.phylogeny_estimation import bootstrap_nj_records, pairwise_branch_lengths
    for n, L, T in ((37, 513, 129), (9, 65, 64)):
        seqs, s2r = family(n, L)
        _, got = bootstrap_nj_records(seqs, banks(T), s2r, GRIDS[T], 2, 0, weights=np.ones((2, L)), return_index=True)
        want = pairwise_branch_lengths(seqs, banks(T), s2r)
        _, margin = ref.pairwise_bisection(seqs, banks(T), s2r)
        decided = margin > UNDECIDED
        assert decided[~np.eye(n, dtype=bool)].mean() >= 0.99
        for b in range(2):
            assert np.array_equal(got[b][decided], want[decided]) and np.all(np.diag(got[b]) == -1)


def test_drawn_replicates_give_the_indices_of_the_materialised_alignment():
    from cherryml_amd.phylogeny_estimation import pairwise_branch_lengths
    case = CASES[1]                                             # 9 x 65, drawn
    seqs, s2r, W = case_inputs(case)
    _, got, _ = device(case)
    _, margin = restated(case)
    for b in range(3):
        cols = np.repeat(np.arange(seqs.shape[1]), W[b].astype(np.int64))
        assert len(cols) == seqs.shape[1]
        want = pairwise_branch_lengths(seqs[:, cols], banks(case[3]), s2r[cols])
        decided = margin[b] > UNDECIDED
        assert decided[~np.eye(9, dtype=bool)].mean() >= 0.99
        assert np.array_equal(got[b][decided], want[decided])


# ------------------------------------------------------------------------------------------------ 4. joins
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_join_records_are_those_of_the_join_kernels_on_the_same_matrices(case):
    from cherryml_amd.phylogeny_estimation import nj_join_records
    n, L, B, T, given = case
    records, index, _ = device(case)
    want = nj_join_records([GRIDS[T][np.maximum(index[b], 0)] for b in range(B)], zero_diagonal=True)
    assert len(records) == len(want) == B
    for got, exp in zip(records, want):
        assert got[0].shape == (max(n - 3, 0), 2) and got[2].shape == (3,) and got[3].shape == (3, 3)
        assert all(same_bits(a, b) for a, b in zip(got, exp))


# ------------------------------------------------------------------------------------------------ 5. independence
def test_a_replicate_does_not_depend_on_the_call(monkeypatch):
    from cherryml_amd.phylogeny_estimation import bootstrap_nj_records
    seqs, s2r = family(9, 65)

    def run(B):
        return bootstrap_nj_records(seqs, banks(64), s2r, GRIDS[64], B, SEED, return_index=True, return_weights=True)

    def check(small, big):
        assert same_bits(small[1], big[1][:len(small[0])]) and same_bits(small[2], big[2][:len(small[0])])
        for a, b in zip(small[0], big[0]):
            assert all(same_bits(x, y) for x, y in zip(a, b))

    big = run(70)
    check(run(5), big)
    check(device(CASES[1]), big)                                # (65 replicates of the same family and seed)
    monkeypatch.setenv("CB_TEST_HOOKS", "1")
    monkeypatch.setenv("CB_BOOT_BYTES", "64")                   # one replicate per chunk
    check(run(5), big)
    monkeypatch.setenv("CB_BOOT_BYTES", str(8 * 81 * 16))       # chunks of 16: 16 + 16 + 16 + 16 + 6
    chunked = run(70)
    check(chunked, big)
    check(big, chunked)


# ------------------------------------------------------------------------------------------------ 6. supports
@functools.lru_cache(maxsize=None)
def supports_family():
    """12 leaves x 300 sites evolved at rate 1 down a random tree with lengths 0.05 .. 0.3, 5 % gaps: no undecided entry in any
    of the 50 replicates (found on the CPU)"""
    rng = np.random.default_rng(1203)
    truth = ref.random_tree(12, rng, length=lambda rng: rng.uniform(0.05, 0.3))
    s2r = rng.integers(0, len(RATES), 300).astype(np.int32)
    seqs = ref.evolve(truth, 12, lg(), RATES[s2r], rng)
    seqs[rng.random(seqs.shape) < 0.05] = -1
    return seqs, s2r, [f"t{i}" for i in range(12)]


def test_supports_equal_the_end_to_end_restatement():
    from cherryml_amd.phylogeny_estimation import (bootstrap_nj_records, bootstrap_supports, neighbor_joining,
                                                   neighbor_joining_device, tree_splits)
    seqs, s2r, names = supports_family()
    B, T = 50, 129
    grid, bank = GRIDS[T], banks(T)
    _, index = bootstrap_nj_records(seqs, bank, s2r, grid, 1, 0, weights=np.ones((1, 300)), return_index=True)
    tree = neighbor_joining_device(boot.distance_matrix(grid, index[0]), names, min_length=grid[0])
    want = boot.supports(tree, names, seqs, bank, s2r, grid, B, SEED)
    off = ~np.eye(12, dtype=bool)
    print(f"smallest margin {want['margin'][:, off].min():.2e}")
    assert np.all(want["margin"][:, off] > UNDECIDED)           # a condition on the inputs
    prof = {}
    nodes, support = bootstrap_supports(tree, names, seqs, bank, s2r, grid, B, SEED, profile=prof)
    assert [tree.nodes()[v] for v in nodes] == want["nodes"] == [v for v in tree.nodes() if not tree.is_leaf(v) and not tree.is_root(v)]
    assert len(nodes) == 12 - 3
    print("supports:", support.tolist())
    assert np.array_equal(support, want["support"])
    counts = support * B
    assert np.array_equal(counts, np.rint(counts)) and np.all((counts >= 0) & (counts <= B))
    assert 0 < len(set(support.tolist()))
    assert set(prof) == {"weights_kernel_ms", "distance_kernel_ms", "join_kernel_ms"}
    # every replicate the alignment itself: the tree's own splits are in every replicate, any other split in none
    ones = np.ones((7, 300))
    _, support = bootstrap_supports(tree, names, seqs, bank, s2r, grid, 7, SEED, weights=ones)
    assert np.all(support == 1.0)
    own = {r.tobytes() for r in tree_splits(tree, names)}
    rng = np.random.default_rng(5)
    D = ref.path_lengths(ref.random_tree(12, rng), list(range(12)))
    other = neighbor_joining(np.maximum(D, D.T), names)
    nodes, support = bootstrap_supports(other, names, seqs, bank, s2r, grid, 7, SEED, weights=ones)
    boot_nodes = boot.node_splits(other, names)
    packed = {v: np.packbits(np.array([x in part for x in names]))for v, part, _ in boot_nodes}
    expect = [1.0 if packed[other.nodes()[v]].tobytes() in own else 0.0 for v in nodes]
    assert support.tolist() == expect and 0.0 in expect


# ------------------------------------------------------------------------------------------------ 7. the stage
def test_the_stage_on_nj_trees_output(tmp_path):
    from cherryml_amd import caching, nj_bootstrap_supports, nj_trees
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation import read_bootstrap_supports
    AA = list("ARNDCQEGHILKMFPSTWYV")
    msa_dir = tmp_path / "msa"
    msa_dir.mkdir()
    fams = ["fam_a", "fam_b"]
    for k, (fam, n, L) in enumerate(zip(fams, (8, 11), (60, 90))):
        rng = np.random.default_rng(50 + k)
        truth = ref.random_tree(n, rng, length=lambda rng: rng.uniform(0.05, 0.4))
        seqs = ref.evolve(truth, n, lg(), np.ones(L), rng)
        (msa_dir / f"{fam}.txt").write_text("".join(f">s{i}\n{''.join(AA[c] for c in seqs[i])}\n" for i in range(n)))
    qpath = str(tmp_path / "lg.txt")
    write_rate_matrix(lg(), AA, qpath)
    out = {k: str(tmp_path / k) for k in ("output_tree_dir", "output_site_rates_dir", "output_likelihood_dir")}
    nj_trees(msa_dir=str(msa_dir), families=fams, rate_matrix_path=qpath, num_rate_categories=4, **out)
    kw = dict(tree_dir=out["output_tree_dir"], msa_dir=str(msa_dir), site_rates_dir=out["output_site_rates_dir"],
              rate_matrix_path=qpath, num_replicates=20, random_seed=3)
    nj_bootstrap_supports(families=fams, output_support_dir=str(tmp_path / "sup"), **kw)
    nj_bootstrap_supports(families=fams[::-1], output_support_dir=str(tmp_path / "sup_reversed"), **kw)
    for fam in fams:
        tree = read_tree(os.path.join(out["output_tree_dir"], fam + ".txt"))
        text = open(tmp_path / "sup" / f"{fam}.txt").read()
        assert text.startswith("node bootstrap\n")
        got = read_bootstrap_supports(str(tmp_path / "sup" / f"{fam}.txt"))
        inner = [v for v in tree.nodes() if not tree.is_leaf(v) and not tree.is_root(v)]
        assert list(got) == inner and len(inner) == len(tree.leaves()) - 3
        assert all(abs(s * 20 - round(s * 20)) == 0 and 0 <= s <= 1 for s in got.values())
        assert text == open(tmp_path / "sup_reversed" / f"{fam}.txt").read()
        prof = open(tmp_path / "sup" / f"{fam}.profiling").read()
        assert [ln.split(":")[0] for ln in prof.split("\n")] == ["bank_time", "weights_kernel_ms", "distance_kernel_ms", "join_kernel_ms",
                                                                "total_time"]
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        first = nj_bootstrap_supports(families=fams, **kw)
        path = os.path.join(first["output_support_dir"], "fam_a.txt")
        stamp = os.stat(path).st_mtime_ns
        assert open(path).read() == open(tmp_path / "sup" / "fam_a.txt").read()
        assert nj_bootstrap_supports(families=fams, **kw) == first and os.stat(path).st_mtime_ns == stamp      # a cache hit
    finally:
        caching.set_cache_dir(None)
    assert len(os.listdir(tmp_path / "cache" / "nj_bootstrap_supports")) == 1
