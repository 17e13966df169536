"""Neighbour joining on the device, what holds without a GPU: the NumPy restatement of the device's arithmetic
(tests/njd_reference.py) against `neighbor_joining` -- bit for bit where every sum is exact, by splits and path lengths where the
order of the row sums shows --, the inputs of the GPU tests (every join with more than four active nodes is decided by a margin
far above that rounding), `cb_nj_batch`'s refusals before any device work, the Python face and the kernels' resources.

At m = 4 the criterion of a pair equals that of the complementary pair in exact arithmetic and rounding decides which is joined:
the unrooted tree and its lengths are the same either way, so comparisons with the host are on splits and path lengths."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import njd_reference as njd  # noqa: E402
from cherryml_amd import _lib  # noqa: E402
from cherryml_amd.phylogeny_estimation import neighbor_joining  # noqa: E402

EXACT_N = [4, 5, 9, 24, 40, 70]
DECIDED = [(kind, n) for n in (5, 12, 65, 130) for kind in ("random", "grid")]
MARGIN = 1e-9


def decided_matrix(kind, n):
    """the random and grid-valued matrices the CPU and the GPU tests share (seeds: 10 n)"""
    return njd.random_matrix(n, 10 * n) if kind == "random" else njd.grid_matrix(n, 10 * n)


def leaf_names(n):
    return [f"t{i}" for i in range(n)]


# ------------------------------------------------------------------------------------------------ restatement against the host
@pytest.mark.parametrize("n", EXACT_N)
def test_restatement_equals_the_host_bit_for_bit_where_sums_are_exact(n):
    for D in (njd.integer_matrix(n, n), njd.ones_matrix(n)):
        rec = njd.join(D)
        assert rec["join_nodes"].shape == (n - 3, 2) and rec["join_len"].shape == (n - 3, 2)
        want = neighbor_joining(D, leaf_names(n), min_length=-np.inf).edges()
        assert njd.edges(leaf_names(n), rec, min_length=-np.inf) == want      # joins, lengths, ties and the root step
    assert njd.join(njd.ones_matrix(n))["tie"].all()


def test_restatement_row_sums_follow_the_lane_order():
    rng = np.random.default_rng(7)
    for m in (1, 5, 63, 64, 65, 130, 200):
        V = rng.random((3, m)) - 0.25
        got = njd.row_sums(V)
        for i in range(3):                                     # lane by lane, as the kernel's loop is written
            lanes = np.zeros(64)
            for k in range(m):
                lanes[k % 64] = lanes[k % 64] + V[i, k]
            for off in (32, 16, 8, 4, 2, 1):
                lanes = lanes + lanes[np.arange(64) ^ off]
            assert got[i] == lanes[0] and np.all(lanes == lanes[0])


@pytest.mark.parametrize("kind,n", DECIDED, ids=lambda v: str(v))
def test_restatement_gives_the_hosts_tree_on_decided_matrices(kind, n):
    D = decided_matrix(kind, n)
    rec = njd.join(D)
    big = rec["m"] > 4
    margin = rec["margin"][big].min() if big.any() else np.inf
    print(f"{kind} n = {n}: smallest margin over the joins with m > 4: {margin:.2e}, exact ties there: {int(rec['tie'][big].sum())}")
    assert margin > MARGIN                                     # a condition on the inputs
    names = leaf_names(n)
    got, want = njd.edge_adjacency(njd.edges(names, rec)), njd.adjacency(neighbor_joining(D, names))
    assert njd.splits(got, names) == njd.splits(want, names)
    err = np.abs(njd.path_lengths(got, names) - njd.path_lengths(want, names)).max()
    print(f"worst path-length difference {err:.2e} (max D {D.max():.3f})")
    assert err <= 1e-10 * D.max()


# ------------------------------------------------------------------------------------------------ the C entry
def test_the_header_declares_and_the_binding_lists_cb_nj_batch():
    header = open(os.path.join(ROOT, "include", "cherrybank.h")).read()
    assert "int cb_nj_batch(int device, int n_fam, const int *n, const double *D, int *join_nodes, double *join_len" in header
    assert "cb_nj_batch" in _lib.SIGNATURES and len(_lib.SIGNATURES["cb_nj_batch"][1]) == 9
    assert hasattr(_lib.load(), "cb_nj_batch")


def _nj_batch(n=(3,), D=None, null=None, n_fam=None):
    n = np.ascontiguousarray(n, dtype=np.int32)
    if D is None:
        D = np.concatenate([njd.integer_matrix(max(int(k), 2), 1).reshape(-1) for k in n if k < 1000] or [np.zeros(4)])
    D = np.ascontiguousarray(D, dtype=np.float64)
    joins = max(int(np.maximum(n.astype(np.int64) - 3, 0).sum()), 1) if n.max() < 1000 else 1
    out = dict(n=n, D=D, join_nodes=np.zeros((joins, 2), np.int32), join_len=np.zeros((joins, 2)),
               final_nodes=np.zeros((len(n), 3), np.int32), final_D=np.zeros((len(n), 9)))
    ptr = {k: v.ctypes.data for k, v in out.items()}
    if null:
        ptr[null] = None
    rc = _lib.load().cb_nj_batch(0, len(n) if n_fam is None else n_fam, ptr["n"], ptr["D"], ptr["join_nodes"], ptr["join_len"],
                                 ptr["final_nodes"], ptr["final_D"], None)
    return rc, (_lib.load().cb_last_error() or b"").decode()


def _bad(i, j, value, mirror=True, n=4):
    D = njd.integer_matrix(n, 3)
    D[i, j] = value
    if mirror:
        D[j, i] = value
    return np.concatenate([njd.integer_matrix(3, 2).reshape(-1), D.reshape(-1)])


REFUSALS = [
    (dict(null="n"), "NULL"),
    (dict(null="D"), "NULL"),
    (dict(null="join_nodes"), "NULL"),
    (dict(null="join_len"), "NULL"),
    (dict(null="final_nodes"), "NULL"),
    (dict(null="final_D"), "NULL"),
    (dict(n_fam=0), "n_fam = 0"),
    (dict(n_fam=-2), "n_fam = -2"),
    (dict(n=(3, 1)), "family 1: n = 1"),
    (dict(n=(0,)), "family 0: n = 0"),
    (dict(n=(3, 50000)), "family 1: n = 50000"),
    (dict(n=(3, 4), D=_bad(1, 2, -0.5)), "family 1: D[1][2] = -0.5"),
    (dict(n=(3, 4), D=_bad(0, 3, np.inf)), "family 1: D[0][3] = inf"),
    (dict(n=(3, 4), D=_bad(2, 3, np.nan)), "family 1: D[2][3] = nan"),
    (dict(n=(3, 4), D=_bad(2, 1, 2.5, mirror=False)), "family 1: D[2][1] = 2.5 but D[1][2] = "),
    (dict(n=(3, 4), D=_bad(2, 2, 0.125)), "family 1: the diagonal entry D[2][2] = 0.125"),
]


@pytest.mark.parametrize("kw,match", REFUSALS, ids=[m for _, m in REFUSALS])
def test_cb_nj_batch_validates_before_any_device_work(kw, match):
    rc, msg = _nj_batch(**kw)
    assert rc == _lib.CB_EINVAL, (rc, msg)
    assert msg.startswith("cb_nj_batch") and match in msg, msg


def test_no_gpu_means_the_device_joiner_fails_loudly(tmp_path):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cherryml_amd import neighbor_joining_device, neighbor_joining_device_batch, nj_trees
    rc, msg = _nj_batch(n=(3, 5))
    assert rc == _lib.CB_EHIP and "no HIP device" in msg, (rc, msg)
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        neighbor_joining_device(njd.integer_matrix(5, 1), leaf_names(5))
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        neighbor_joining_device_batch([njd.integer_matrix(5, 1), njd.ones_matrix(2)], [leaf_names(5), leaf_names(2)])
    with pytest.raises(_lib.CherryBankError, match="no HIP device"):
        nj_trees(msa_dir=str(tmp_path), families=["f"], rate_matrix_path=str(tmp_path / "q.txt"), num_rate_categories=4,
                 output_tree_dir=str(tmp_path / "t"), output_site_rates_dir=str(tmp_path / "s"),
                 output_likelihood_dir=str(tmp_path / "l"), joiner="device")


# ------------------------------------------------------------------------------------------------ the Python face
def test_an_unknown_joiner_is_refused(tmp_path):
    from cherryml_amd import nj_ml_rates_trees, nj_ml_trees, nj_nni_trees, nj_trees
    from cherryml_amd.phylogeny_estimation import nj_tree_family
    kw = dict(msa_dir=str(tmp_path), families=["f"], rate_matrix_path=str(tmp_path / "q.txt"), num_rate_categories=4,
              output_tree_dir=str(tmp_path / "t"), output_site_rates_dir=str(tmp_path / "s"), output_likelihood_dir=str(tmp_path / "l"))
    with pytest.raises(ValueError, match="joiner must be one of .* got 'bogus'"):
        nj_trees(joiner="bogus", **kw)
    with pytest.raises(ValueError, match="joiner"):
        nj_tree_family(["a", "b"], ["AR", "AN"], np.zeros((20, 20)), list("ARNDCQEGHILKMFPSTWYV"), joiner="bogus")
    import inspect
    for stage in (nj_ml_trees, nj_ml_rates_trees, nj_nni_trees):
        assert inspect.signature(stage).parameters["joiner"].default == "host"
    for stage in (nj_ml_trees, nj_ml_rates_trees):              # (nj_nni_trees asks for a device first)
        with pytest.raises(ValueError, match="joiner"):
            stage(joiner="bogus", **kw)


def test_the_joiner_enters_the_cache_key(tmp_path):
    from cherryml_amd import caching, nj_trees
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        kw = dict(msa_dir=str(tmp_path), families=["f"], rate_matrix_path=str(tmp_path / "missing.txt"), num_rate_categories=4)
        for joiner in ("host", "device"):
            with pytest.raises(Exception):
                nj_trees(joiner=joiner, **kw)
    finally:
        caching.set_cache_dir(None)
    assert len(os.listdir(tmp_path / "cache" / "nj_trees")) == 2


def test_the_device_face_raises_the_hosts_value_errors():
    from cherryml_amd.phylogeny_estimation import neighbor_joining_device, neighbor_joining_device_batch
    ok = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, 1.5], [2.0, 1.5, 0.0]])
    bad = ok.copy()
    bad[0, 1] = 1.25
    cases = [(([[0.0]], ["a"]), "at least two"), ((ok[:2], ["a", "b", "c"]), "square"), ((ok, ["a", "b"]), "square"),
             ((bad, ["a", "b", "c"]), "symmetric"), ((ok, ["a", "b", "a"]), "distinct"), ((ok, ["a", "root", "c"]), "own node names")]
    for args, match in cases:
        with pytest.raises(ValueError, match=match) as host:
            neighbor_joining(*args)
        with pytest.raises(ValueError, match=match) as dev:
            neighbor_joining_device(*args)
        assert str(dev.value) == str(host.value)
        with pytest.raises(ValueError, match=match):
            neighbor_joining_device_batch([ok, args[0]], [["a", "b", "c"], args[1]])
    with pytest.raises(ValueError, match="one list of names per matrix"):
        neighbor_joining_device_batch([ok], [])


# ------------------------------------------------------------------------------------------------ resources
def test_the_three_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    meta = kernel_meta()
    for kernel in ("nj_rowsum_kernel", "nj_argmin_kernel", "nj_join_kernel"):
        hits = {k: v for k, v in meta.items() if k.startswith(kernel)}
        assert len(hits) == 1, (kernel, sorted(hits))
        for name, m in hits.items():
            print(name, m)
            assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)
            assert m["vgpr"] <= 128, (name, m)              # four waves per SIMD at least
