"""Neighbour joining on the GPU (`cb_nj_batch`, csrc/nj.hip.h): the join records against the NumPy restatement of the device's
arithmetic (tests/njd_reference.py), bit for bit, at the sizes where the kernels change course -- one join, the lane-stride edges
63 / 64 / 65, several strides, several row blocks and more than one candidate workgroup --; a batch against every family alone,
under the default chunk bound, with one family per chunk and on a second call; `neighbor_joining_device` against the host's
`neighbor_joining`; the refusals; the stage `nj_trees(joiner="device")` and the pipelines that take it.

Exactness.  Device and restatement do the same operations in the same order, so every output is compared bit for bit, ties
included.  The host sums its rows in another order: where all sums are exact (integer matrices) the trees are equal bit for
bit; on the random and grid-valued matrices (the ones tests/test_njd_cpu.py shows to be decided: every join with m > 4 has a
margin above 1e-9, the sums differ by ~1e-15 relative) splits are equal and path lengths agree within 1e-10 max D.  At m = 4 a
pair ties with its complement in exact arithmetic and rounding decides: the same unrooted tree either way.  Needs an MI355X."""
import os
import sys
from functools import partial

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import njd_reference as njd  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [4, 5, 8, 63, 64, 65, 130, 257]
KINDS = ["integer", "random", "grid", "equal"]
AA = list("ARNDCQEGHILKMFPSTWYV")
FIELDS = ("join_nodes", "join_len", "final_nodes", "final_D")


def matrix(kind, n):
    if kind == "integer":
        return njd.integer_matrix(n, n)
    if kind == "random":
        return njd.random_matrix(n, 10 * n)
    if kind == "grid":
        return njd.grid_matrix(n, 10 * n)
    return njd.ones_matrix(n) * 0.37


def leaf_names(n):
    return [f"t{i}" for i in range(n)]


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def records(Ds, **kw):
    from cherryml_amd.phylogeny_estimation import nj_join_records
    return [dict(zip(FIELDS, rec)) for rec in nj_join_records(Ds, **kw)]


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("n", SIZES)
def test_join_records_equal_the_restatement_bit_for_bit(n):
    prof = {}
    Ds = [matrix(kind, n) for kind in KINDS]
    got = records(Ds, profile=prof)
    assert prof["kernel_ms"] > 0.0
    for kind, D, rec in zip(KINDS, Ds, got):
        want = njd.join(D)
        print(f"{kind} n = {n}: {int(want['tie'].sum())} tied joins of {n - 3}, smallest margin "
              f"{want['margin'].min() if n > 3 else np.inf:.2e}")
        assert rec["join_nodes"].shape == (n - 3, 2) and np.array_equal(rec["join_nodes"], want["join_nodes"]), kind
        for key in ("join_len", "final_nodes", "final_D"):
            assert same_bits(rec[key], want[key]), (kind, key)
        if kind == "equal":                                     # exact ties and margins of an ulp: only the same bits decide alike
            assert want["tie"].any() and (n < 8 or want["margin"].min() < 1e-12)


# ------------------------------------------------------------------------------------------------ 2. batch, chunks, repeat
def test_a_batch_equals_every_family_alone(monkeypatch):
    sizes = [2, 3, 4, 65, 130, 5]
    Ds = [matrix("random" if k % 2 else "grid", n) for k, n in enumerate(sizes)]
    alone = [records([D])[0] for D in Ds]
    for n, D, rec in zip(sizes, Ds, alone):
        want = njd.join(D)
        assert all(same_bits(rec[key], want[key]) for key in FIELDS), n
        if n <= 3:                                              # the leaves themselves, unused slots -1 / 0
            assert rec["join_nodes"].shape == (0, 2) and list(rec["final_nodes"]) == list(range(n)) + [-1] * (3 - n)
            assert np.array_equal(rec["final_D"][:n, :n], D) and not rec["final_D"][n:].any() and not rec["final_D"][:, n:].any()

    def check(batch):
        for n, a, b in zip(sizes, alone, batch):
            assert all(same_bits(a[key], b[key]) for key in FIELDS), n

    check(records(Ds))
    check(records(Ds))                                          # a second call
    check(list(reversed(records(list(reversed(Ds))))))          # another order
    monkeypatch.setenv("CB_TEST_HOOKS", "1")
    monkeypatch.setenv("CB_NJ_BYTES", "64")                     # one family per chunk
    check(records(Ds))
    monkeypatch.setenv("CB_NJ_BYTES", str(8 * (65 * 65 + 16 + 9 + 4)))   # chunks of several families: (2, 3, 4, 65), (130), (5)
    check(records(Ds))


# ------------------------------------------------------------------------------------------------ 3. the host
@pytest.mark.parametrize("n", [4, 5, 9, 24, 40, 70])
def test_integer_matrices_give_the_hosts_tree_bit_for_bit(n):
    from cherryml_amd.phylogeny_estimation import neighbor_joining, neighbor_joining_device
    for D in (njd.integer_matrix(n, n), njd.ones_matrix(n)):
        for min_length in (0.0, 1.5):
            assert neighbor_joining_device(D, leaf_names(n), min_length=min_length).edges() == \
                neighbor_joining(D, leaf_names(n), min_length=min_length).edges()


def test_decided_matrices_give_the_hosts_splits_and_path_lengths():
    from cherryml_amd.phylogeny_estimation import neighbor_joining, neighbor_joining_device_batch
    cases = [(kind, n) for n in (5, 12, 65, 130) for kind in ("random", "grid")]
    Ds = [matrix(kind, n) for kind, n in cases]
    trees = neighbor_joining_device_batch(Ds, [leaf_names(n) for _, n in cases])
    for (kind, n), D, tree in zip(cases, Ds, trees):
        names = leaf_names(n)
        got, want = njd.adjacency(tree), njd.adjacency(neighbor_joining(D, names))
        err = np.abs(njd.path_lengths(got, names) - njd.path_lengths(want, names)).max()
        print(f"{kind} n = {n}: worst path-length difference to the host {err:.2e} (max D {D.max():.3f})")
        assert njd.splits(got, names) == njd.splits(want, names), (kind, n)
        assert err <= 1e-10 * D.max(), (kind, n)
        assert tree.root() == "root" and sorted(tree.leaves()) == sorted(names) and tree.num_edges() == 2 * n - 3


def test_additive_matrices_give_their_trees_back():
    from cherryml_amd.phylogeny_estimation import neighbor_joining_device_batch
    sizes = [2, 3, 4, 9, 40, 130]
    truths, Ds = [], []
    for n in sizes:
        truths.append(njd.random_tree(n, np.random.default_rng(100 + n)))
        D = njd.path_lengths(truths[-1], list(range(n)))
        Ds.append(np.maximum(D, D.T))
    trees = neighbor_joining_device_batch(Ds, [leaf_names(n) for n in sizes])
    for n, truth, D, tree in zip(sizes, truths, Ds, trees):
        names = leaf_names(n)
        err = np.abs(njd.path_lengths(njd.adjacency(tree), names) - D).max()
        print(f"n = {n}: worst path-length error {err:.2e} (max D {D.max():.3f})")
        assert err <= 1e-10
        assert sorted(tree.internal_nodes()) == sorted(["root"] + [f"internal-{k}" for k in range(max(n - 3, 0))])
        if n >= 4:
            want = {frozenset(names[x] for x in s) for s in njd.splits(truth, list(range(n)))}
            assert njd.splits(njd.adjacency(tree), names) == want


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_the_refusals_name_the_value_and_a_valid_call_follows():
    from cherryml_amd import _lib
    from cherryml_amd.phylogeny_estimation import nj_join_records
    good = [njd.integer_matrix(3, 2), njd.integer_matrix(6, 3)]
    want = records(good)

    def bad(i, j, value, mirror=True):
        D = good[1].copy()
        D[i, j] = value
        if mirror:
            D[j, i] = value
        return [good[0], D]

    for Ds, match in [(bad(1, 2, -0.5), "family 1: D[1][2] = -0.5"), (bad(0, 3, np.inf), "family 1: D[0][3] = inf"),
                      (bad(2, 3, np.nan), "family 1: D[2][3] = nan"), (bad(2, 2, 0.125), "family 1: the diagonal entry D[2][2] = 0.125"),
                      (bad(4, 1, 2.5, mirror=False), "family 1: D[4][1] = 2.5 but D[1][4] = "),
                      ([good[0], np.zeros((1, 1))], "family 1: n = 1")]:
        with pytest.raises(_lib.CherryBankError) as e:
            nj_join_records(Ds)
        assert "cb_nj_batch" in str(e.value) and match in str(e.value), str(e.value)
    n = np.array([3], dtype=np.int32)
    out = np.zeros(64)
    rc = _lib.load().cb_nj_batch(0, 0, n.ctypes.data, good[0].ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                                 out.ctypes.data, None)
    assert rc == _lib.CB_EINVAL and "n_fam = 0" in _lib.load().cb_last_error().decode()
    rc = _lib.load().cb_nj_batch(0, 1, n.ctypes.data, None, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data, None)
    assert rc == _lib.CB_EINVAL and "NULL" in _lib.load().cb_last_error().decode()
    again = records(good)
    assert all(same_bits(a[key], b[key]) for a, b in zip(want, again) for key in FIELDS)


# ------------------------------------------------------------------------------------------------ 5. the stage
def demo_families(tmp_path):
    """the two smallest of the 32 demo families (180 x 50 and 1005 x 413) as MSA files: (names per family, msa_dir)"""
    z = load_golden("demo32_co_inputs.npz")
    off, blob = z["msa_offsets"], z["msa_bytes"].tobytes()
    texts = {str(f): blob[off[k]:off[k + 1]].decode() for k, f in enumerate(z["families"])}
    fams = sorted(texts, key=lambda f: (texts[f].count(">"), f))[:2]
    (tmp_path / "msa").mkdir()
    for f in fams:
        (tmp_path / "msa" / f"{f}.txt").write_text(texts[f])
    return fams, str(tmp_path / "msa")


def test_nj_trees_with_the_device_joiner_and_the_pipelines_that_take_it(tmp_path):
    import cherryml_amd
    from cherryml_amd import caching, nj_ml_trees, nj_trees
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.evaluation._likelihood import dp_likelihood_computation
    from cherryml_amd.io import read_tree, write_rate_matrix
    from cherryml_amd.phylogeny_estimation import nj_distance_indices
    from cherryml_amd.phylogeny_estimation._fast_cherries import _encode_and_pair, _read_msa_file
    import nj_reference as ref
    fams, msa_dir = demo_families(tmp_path)
    Q = np.ascontiguousarray(load_golden("demo_e2e.npz")["lg_Q_best_f64"], dtype=np.float64)
    qpath = str(tmp_path / "q0.txt")
    write_rate_matrix(Q, AA, qpath)
    out = {j: {k: str(tmp_path / j / k) for k in ("output_tree_dir", "output_site_rates_dir", "output_likelihood_dir")}
           for j in ("host", "device")}
    for joiner in ("host", "device"):
        nj_trees(msa_dir=msa_dir, families=fams, rate_matrix_path=qpath, num_rate_categories=4, joiner=joiner, **out[joiner])
    keys = ["pairing_time", "ble_time", "distance_time", "nj_time", "likelihood_time", "total_time"]
    for k in out["host"]:                                       # the same files, the same .profiling keys
        assert sorted(os.listdir(out["device"][k])) == sorted(os.listdir(out["host"][k])), k
    for fam in fams:
        for joiner in ("host", "device"):
            prof = open(os.path.join(out[joiner]["output_tree_dir"], fam + ".profiling")).read().split("\n")
            assert [ln.split(":")[0] for ln in prof] == keys and all(float(ln.split(": ")[1]) >= 0.0 for ln in prof)
        names, sequences = _read_msa_file(os.path.join(msa_dir, fam + ".txt"))
        tree = read_tree(os.path.join(out["device"]["output_tree_dir"], fam + ".txt"))
        assert sorted(tree.leaves()) == sorted(names) and tree.num_edges() == 2 * len(names) - 3
        # the tree the restatement builds from the same distance indices
        seqs, pairs = _encode_and_pair(sequences, AA, 1234, "lemire")
        index, _, rate_index, grid, rates = nj_distance_indices(seqs, pairs, Q, num_rate_categories=4)
        mean_rate = 0.0
        for r in rates[rate_index]:
            mean_rate += float(r)
        mean_rate /= len(rate_index)
        D = grid[np.maximum(index, 0)] * mean_rate
        np.fill_diagonal(D, 0.0)
        assert tree.edges() == njd.edges(names, njd.join(D, with_margins=False), min_length=float(grid[0])), fam
        # the likelihood file: a fresh evaluation of the files the stage wrote
        site_rates = read_site_rates(os.path.join(out["device"]["output_site_rates_dir"], fam + ".txt"))
        lines = open(os.path.join(out["device"]["output_likelihood_dir"], fam + ".txt")).read().split("\n")
        total, per_site = float(lines[0]), np.array([float(x) for x in lines[2].split()])
        ll, lls = dp_likelihood_computation(tree, read_msa(os.path.join(msa_dir, fam + ".txt")), None, site_rates, AA,
                                            ref.stationary(Q), Q)
        assert np.all(np.isfinite(per_site)) and np.allclose(per_site, lls, rtol=1e-9, atol=0.0)
        assert abs(ll - total) <= 1e-9 * abs(total)
    # the cache: the joiner is part of the key, a second call is a hit
    small = fams[:1]
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        first = nj_trees(msa_dir=msa_dir, families=small, rate_matrix_path=qpath, num_rate_categories=4, joiner="device")
        path = os.path.join(first["output_tree_dir"], small[0] + ".txt")
        stamp = os.stat(path).st_mtime_ns
        assert nj_trees(msa_dir=msa_dir, families=small, rate_matrix_path=qpath, num_rate_categories=4, joiner="device") == first
        assert os.stat(path).st_mtime_ns == stamp and len(os.listdir(tmp_path / "cache" / "nj_trees")) == 1
        host = nj_trees(msa_dir=msa_dir, families=small, rate_matrix_path=qpath, num_rate_categories=4)
        assert host != first and len(os.listdir(tmp_path / "cache" / "nj_trees")) == 2
        ml = nj_ml_trees(msa_dir=msa_dir, families=small, rate_matrix_path=qpath, num_rate_categories=4, num_rounds=2, joiner="device")
        assert len(os.listdir(tmp_path / "cache" / "nj_trees")) == 2       # (the device joiner's trees again: a hit)
        refit = read_tree(os.path.join(ml["output_tree_dir"], small[0] + ".txt"))
        assert sorted(refit.leaves()) == sorted(read_tree(path).leaves())
        # the EM pipeline with the device joiner as its tree estimator, one iteration
        res = cherryml_amd.lg_end_to_end_with_em_optimizer(
            msa_dir=msa_dir, families=small, tree_estimator=partial(nj_trees, num_rate_categories=4, joiner="device"),
            initial_tree_estimator_rate_matrix_path=qpath, num_iterations=1, em_iterations=3, optimizer_initialization=qpath)
    finally:
        caching.set_cache_dir(None)
    learned = cherryml_amd.io.read_rate_matrix(res["learned_rate_matrix_path"]).to_numpy()
    assert learned.shape == (20, 20) and np.all(np.isfinite(learned)) and np.allclose(learned.sum(1), 0.0, atol=1e-9)
    assert res["tree_estimator_output_dirs_0"]["output_tree_dir"] == first["output_tree_dir"]      # (the cached device trees)
