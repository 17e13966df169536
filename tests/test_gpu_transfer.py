"""The transfer distances on the GPU (`cb_transfer_support`: csrc/transfer.hip.h) against the NumPy restatement
tests/transfer_reference.py, bit for bit -- everything is integers, there is no tolerance: min_dist, sum_dist and present of every
case, the independence of a replicate's column from the call and the chunks, the other side of every split, the supports of a
small real family against Felsenstein's, and the stage.

The cases (transfer_reference.CASES; tests/test_transfer_cpu.py checks on the CPU what values each holds): n = 4 (one join), 5,
8; the word edges 31, 32, 33, 63, 64, 65; 257; 1030 and 2100 leaves, whose rows of 17 and 33 words pass the 16 words the distance kernel stages at once, in
two and in three chunks with a partial last one; n_ref = 1, 65 (one reference tile and one row) and others that are no multiple of
the tile; n_rep = 1 and 70.  The bound on 0 <= bootstrap <= transfer <= 1 in float64 is transfer_reference.CHAIN_SLACK.
Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nj_reference as ref  # noqa: E402
import transfer_reference as tr  # noqa: E402
from transfer_reference import CASES, CHAIN_SLACK  # noqa: E402

pytestmark = pytest.mark.gpu

RATES = np.array([0.25, 0.6, 1.2, 2.5])
GRID = np.array([0.03 * 1.1 ** i for i in range(-64, 65)])
SEED = 20


def case_id(c):
    return "x".join(map(str, c))


def packed(rows):
    return np.packbits(np.asarray(rows, dtype=bool), axis=1)


@functools.lru_cache(maxsize=None)
def inputs(case):
    return tr.make_case(*case)


@functools.lru_cache(maxsize=None)
def restated(case):
    rows, joins = inputs(case)
    return tr.distances(rows, case[0], joins)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. the distances
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_distances_equal_the_restatement(case):
    from cherryml_amd.phylogeny_estimation import transfer_distances
    n, n_ref, n_rep = case
    rows, joins = inputs(case)
    want = restated(case)
    prof = {}
    sum_dist, present, min_dist = transfer_distances(packed(rows), n, joins, profile=prof, per_replicate=True)
    print(f"{case_id(case)}: {int((min_dist != want['min_dist']).sum())} of {min_dist.size} distances differ; kernels {prof}")
    assert min_dist.shape == (n_ref, n_rep) and min_dist.dtype == np.int32
    assert sum_dist.shape == (n_ref,) and sum_dist.dtype == np.int64 and present.shape == (n_ref,) and present.dtype == np.int32
    assert same_bits(min_dist, want["min_dist"]) and same_bits(sum_dist, want["sum_dist"]) and same_bits(present, want["present"])
    assert set(prof) == {"sets_kernel_ms", "distance_kernel_ms"} and prof["sets_kernel_ms"] > 0.0 and prof["distance_kernel_ms"] > 0.0
    # without the per-replicate matrix: the same sums
    again = transfer_distances(packed(rows), n, joins)
    assert len(again) == 2 and same_bits(again[0], sum_dist) and same_bits(again[1], present)


# ------------------------------------------------------------------------------------------------ 2. independence
def test_a_replicates_column_does_not_depend_on_the_call(monkeypatch):
    from cherryml_amd.phylogeny_estimation import transfer_distances
    case = (33, 30, 70)
    rows, joins = inputs(case)
    want = restated(case)["min_dist"]
    words = (33 - 3) * 1 * 8                                    # bytes of a replicate's leaf sets: 30 rows of one word

    def run(B):
        return transfer_distances(packed(rows), 33, joins[:B], per_replicate=True)

    def check(out, B):
        assert same_bits(out[2], np.ascontiguousarray(want[:, :B]))
        assert same_bits(out[0], want[:, :B].sum(axis=1).astype(np.int64))
        assert same_bits(out[1], (want[:, :B] == 0).sum(axis=1).astype(np.int32))

    for B in (1, 17, 70):
        check(run(B), B)
    monkeypatch.setenv("CB_TEST_HOOKS", "1")
    monkeypatch.setenv("CB_TBE_BYTES", "8")                     # below one replicate: every replicate alone
    check(run(17), 17)
    monkeypatch.setenv("CB_TBE_BYTES", str(16 * words))         # chunks of 16: 16 + 16 + 16 + 16 + 6
    check(run(70), 70)
    monkeypatch.setenv("CB_TBE_BYTES", str(3 * words + 5))      # chunks of 3, the last of 1
    check(run(70), 70)
    # a replicate whose rows pass the kernel's word chunk, alone in its chunk and with the other
    big = (2100, 5, 2)
    rows, joins = inputs(big)
    monkeypatch.setenv("CB_TBE_BYTES", "8")
    out = transfer_distances(packed(rows), 2100, joins, per_replicate=True)
    assert same_bits(out[2], restated(big)["min_dist"])
    one = transfer_distances(packed(rows), 2100, joins[1:], per_replicate=True)
    assert same_bits(one[2], np.ascontiguousarray(restated(big)["min_dist"][:, 1:]))


# ------------------------------------------------------------------------------------------------ 3. the other side
@pytest.mark.parametrize("case", [(8, 5, 6), (33, 30, 70), (65, 62, 17), (1030, 7, 3)], ids=case_id)
def test_complementing_every_reference_row_changes_nothing(case):
    from cherryml_amd.phylogeny_estimation import transfer_distances
    rows, joins = inputs(case)
    got = transfer_distances(packed(rows), case[0], joins, per_replicate=True)
    flipped = transfer_distances(packed(~rows), case[0], joins, per_replicate=True)
    assert all(same_bits(a, b) for a, b in zip(got, flipped))
    assert same_bits(got[2], restated(case)["min_dist"])


# ------------------------------------------------------------------------------------------------ 4. a real family
def lg():
    return np.ascontiguousarray(load_golden("data_lg.npz")["lg"], dtype=np.float64)


def test_supports_of_a_small_family_against_felsensteins():
    """test_gpu_boot.supports_family: 12 leaves x 300 sites, 50 replicates"""
    from cherryml_amd.phylogeny_estimation import (bootstrap_nj_records, bootstrap_supports, compute_log_transition_matrices,
                                                   neighbor_joining_device, transfer_bootstrap_supports,
                                                   transfer_supports_of_records)
    rng = np.random.default_rng(1203)
    truth = ref.random_tree(12, rng, length=lambda rng: rng.uniform(0.05, 0.3))
    s2r = rng.integers(0, len(RATES), 300).astype(np.int32)
    seqs = ref.evolve(truth, 12, lg(), RATES[s2r], rng)
    seqs[rng.random(seqs.shape) < 0.05] = -1
    names = [f"t{i}" for i in range(12)]
    bank = compute_log_transition_matrices(lg(), GRID, RATES)
    B = 50
    _, index = bootstrap_nj_records(seqs, bank, s2r, GRID, 1, 0, weights=np.ones((1, 300)), return_index=True)
    D = GRID[np.maximum(index[0], 0)]
    np.fill_diagonal(D, 0.0)
    tree = neighbor_joining_device(D, names, min_length=GRID[0])
    nodes_f, support = bootstrap_supports(tree, names, seqs, bank, s2r, GRID, B, SEED)
    prof = {}
    nodes, bootstrap, transfer = transfer_bootstrap_supports(tree, names, seqs, bank, s2r, GRID, B, SEED, profile=prof)
    print("bootstrap:", bootstrap.tolist(), "\ntransfer: ", transfer.tolist())
    assert same_bits(nodes, nodes_f) and same_bits(bootstrap, support) and len(nodes) == 12 - 3
    assert transfer.dtype == np.float64 and np.all((0 <= bootstrap) & (bootstrap <= transfer + CHAIN_SLACK) & (transfer <= 1))
    assert set(prof) == {"weights_kernel_ms", "distance_kernel_ms", "join_kernel_ms", "transfer_sets_kernel_ms",
                         "transfer_distance_kernel_ms"}
    # the same numbers from the records and the restatement, the formula as the issue states it
    records = bootstrap_nj_records(seqs, bank, s2r, GRID, B, SEED)
    again = transfer_supports_of_records(tree, names, records)
    assert all(same_bits(a, b) for a, b in zip(again, (nodes, bootstrap, transfer)))
    below = {}
    for v in tree.postorder_traversal():
        below[v] = {names.index(v)} if tree.is_leaf(v) else set().union(*[below[c] for c, _ in tree.children(v)])
    rows = np.zeros((len(nodes), 12), dtype=bool)
    for r, v in enumerate(nodes):
        rows[r, sorted(below[tree.nodes()[int(v)]])] = True
    want = tr.distances(rows, 12, np.stack([r[0] for r in records]))
    want_bootstrap, want_transfer = tr.supports(want["sum_dist"], want["present"], want["p"], B)
    assert same_bits(bootstrap, want_bootstrap) and same_bits(transfer, want_transfer)


# ------------------------------------------------------------------------------------------------ 5. the stage
def test_the_stage_on_nj_trees_output(tmp_path):
    from cherryml_amd import caching, nj_bootstrap_supports, nj_transfer_supports, nj_trees
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation import read_bootstrap_supports, read_transfer_supports
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
    nj_transfer_supports(families=fams, output_support_dir=str(tmp_path / "tbe"), **kw)
    nj_transfer_supports(families=fams[1:], output_support_dir=str(tmp_path / "tbe_alone"), **kw)
    nj_bootstrap_supports(families=fams, output_support_dir=str(tmp_path / "sup"), **kw)
    for fam in fams:
        tree = read_tree(os.path.join(out["output_tree_dir"], fam + ".txt"))
        text = open(tmp_path / "tbe" / f"{fam}.txt").read()
        assert text.startswith("node bootstrap transfer\n")
        got = read_transfer_supports(str(tmp_path / "tbe" / f"{fam}.txt"))
        inner = [v for v in tree.nodes() if not tree.is_leaf(v) and not tree.is_root(v)]
        assert list(got) == inner and len(inner) == len(tree.leaves()) - 3
        assert {v: s for v, (s, _) in got.items()} == read_bootstrap_supports(str(tmp_path / "sup" / f"{fam}.txt"))
        assert all(0 <= s <= t + CHAIN_SLACK and t <= 1 for s, t in got.values())
        prof = open(tmp_path / "tbe" / f"{fam}.profiling").read()
        assert [ln.split(":")[0] for ln in prof.split("\n")] == ["bank_time", "weights_kernel_ms", "distance_kernel_ms", "join_kernel_ms",
                                                                "transfer_sets_kernel_ms", "transfer_distance_kernel_ms", "total_time"]
    # a family's numbers do not depend on the other families of the call
    assert open(tmp_path / "tbe_alone" / "fam_b.txt").read() == open(tmp_path / "tbe" / "fam_b.txt").read()
    assert not os.path.exists(tmp_path / "tbe_alone" / "fam_a.txt")
    with pytest.raises(ValueError, match="not a transfer-support file"):
        read_transfer_supports(str(tmp_path / "sup" / "fam_a.txt"))
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        first = nj_transfer_supports(families=fams, **kw)
        path = os.path.join(first["output_support_dir"], "fam_a.txt")
        stamp = os.stat(path).st_mtime_ns
        assert open(path).read() == open(tmp_path / "tbe" / "fam_a.txt").read()
        assert nj_transfer_supports(families=fams, **kw) == first and os.stat(path).st_mtime_ns == stamp      # a cache hit
    finally:
        caching.set_cache_dir(None)
    assert len(os.listdir(tmp_path / "cache" / "nj_transfer_supports")) == 1
