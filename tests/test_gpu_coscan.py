"""The co-evolution scan on the GPU, through the C ABI (cb_coscan_*) and the Python class / stage: parity with the NumPy
restatement (tests/coscan_reference.py), with the existing co-transition counter, the product model, bitwise stability, and the
stage's files.  Every case's restatement is computed once and shared."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import coscan_reference as cr  # noqa: E402
from cherryml_amd import CoevolutionScanner, _lib, caching, coevolution_scan, read_coevolution_scan  # noqa: E402
from cherryml_amd.counting._stage import PAIR_DTYPE  # noqa: E402
from oracle import counting_oracle as co  # noqa: E402
from test_coscan_cpu import PRODUCT_BAR, PRODUCT_CASES, product_case  # noqa: E402

pytestmark = pytest.mark.gpu

# name: (S, B, spectral, symmetric, [(L, sequence pairs)]).  L = 17 and 33: one more than one and two 16-site tile edges
CASES = {
    "s2_b5_general_cherry": (2, 5, False, True, [(1, 1), (2, 3), (17, 70)]),
    "s4_b129_spectral_cherry": (4, 129, True, True, [(33, 70), (17, 3)]),
    "s4_b5_general_edge": (4, 5, False, False, [(33, 70), (2, 1)]),
    "s20_b5_spectral_cherry": (20, 5, True, True, [(17, 3), (33, 70)]),
    "s20_b129_spectral_edge": (20, 129, True, False, [(17, 70)]),
    "s20_b5_general_cherry": (20, 5, False, True, [(2, 3)]),
}


def _grid(B):
    return np.exp(np.linspace(np.log(0.05), np.log(5.0), B))


@functools.lru_cache(maxsize=None)
def case(name):
    """the model, the families and the restatement's results of a case (read-only, shared by the tests)"""
    S, B, spectral, symmetric, fams = CASES[name]
    grid = _grid(B)
    if spectral:
        (Q1, pi1), (Q2, pi2) = cr.random_reversible(S, 1), cr.random_reversible(S * S, 2)
    else:
        Q1, pi1, Q2, pi2 = cr.random_general(S, 1), None, cr.random_general(S * S, 2), None
    P1, P2 = cr.bank(Q1, grid, pi1), cr.bank(Q2, grid, pi2)
    assert P1.min() > 0 and P2.min() > 0          # on the CPU: the banks of the tests are positive
    lp1, lp2 = cr.log_bank(P1), cr.log_bank(P2)
    families = [cr.random_family(S, L, n, grid, 100 * L + n) for L, n in fams]
    want = [cr.scan(c, p, grid, lp1, lp2, symmetric) for c, p in families]
    return dict(S=S, grid=grid, Q1=Q1, pi1=pi1, Q2=Q2, pi2=pi2, lp2=lp2, symmetric=symmetric, families=families, want=want)


def _scanner(z):
    return CoevolutionScanner(z["Q1"], z["Q2"], z["grid"], z["pi1"], z["pi2"])


def _worst(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if want.size else 0.0


# ------------------------------------------------------------------------------------------------ 1. restatement parity
@pytest.mark.parametrize("name", list(CASES))
def test_the_scan_equals_the_restatement(name):
    z = case(name)
    with _scanner(z) as sc:
        got = sc.scan([c for c, _ in z["families"]], [p for _, p in z["families"]], symmetric=z["symmetric"])
    assert len(got) == len(z["want"])
    for (codes, _), g, w in zip(z["families"], got, z["want"]):
        L = codes.shape[1]
        for key in ("score", "pair_ll", "indep_ll"):
            assert g[key].shape == (L, L) and g[key].dtype == np.float64
            print(name, L, key, "worst |difference| / max(1, |x|):", _worst(g[key], w[key]))
        for key in ("score", "pair_ll", "indep_ll"):
            assert _worst(g[key], w[key]) <= 1e-10, (name, L, key)
        assert g["n_used"].dtype == np.int32 and np.array_equal(g["n_used"], w["n_used"])
        if L == 1:
            assert all(np.array_equal(g[k], np.zeros((1, 1))) for k in g)    # one site: no pair, an empty result
        else:
            assert w["n_used"].max() > 0 and np.abs(w["score"]).max() > 0    # the case compares something


# ------------------------------------------------------------------------------------------ 2. against the existing counter
def test_the_scan_equals_the_counter_s_tensor_against_the_log_bank():
    z = case("s4_b129_spectral_cherry")
    S, grid = z["S"], z["grid"]
    codes, pairs = z["families"][0]
    L = codes.shape[1]
    with _scanner(z) as sc:
        got = sc.scan([codes], [pairs])[0]
    seqs = np.ascontiguousarray(codes.reshape(-1))
    rec = np.array([(a * L, b * L, 0, 1, 0, la, lb) for a, b, la, lb in pairs], dtype=PAIR_DTYPE)
    lib = _lib.load()
    for i, j in [(0, 1), (0, 32), (3, 17), (15, 16), (20, 31), (31, 32)]:
        contacts = np.array([i, j], dtype=np.int32)
        C = np.zeros((len(grid), S * S, S * S), dtype=np.uint64)
        _lib.check(lib.cb_count_co_transitions(0, S, len(grid), grid.ctypes.data, seqs.ctypes.data, seqs.size, contacts.ctypes.data,
                                               1, rec.ctypes.data, len(rec), 1, 0, C.ctypes.data), "cb_count_co_transitions")
        assert int(C.sum()) == 4 * int(got["n_used"][i, j])          # four terms per contributing sequence pair, exactly
        nz = np.nonzero(C)
        x = 0.25 * float(np.sum(C[nz].astype(np.float64) * z["lp2"][nz]))
        assert abs(x - got["pair_ll"][i, j]) <= 1e-10 * max(1.0, abs(x)), (i, j, x, got["pair_ll"][i, j])
    assert got["n_used"][0, 1] > 0


# ---------------------------------------------------------------------------------------------------- 3. product model
@pytest.mark.parametrize("S,B,L,n", PRODUCT_CASES)
@pytest.mark.parametrize("spectral", [False, True])
def test_the_product_model_scores_nothing_on_the_gpu(S, B, L, n, spectral):
    grid, Q1, pi1, Q2, pi2, codes, pairs = product_case(S, B, L, n)
    with CoevolutionScanner(Q1, Q2, grid, pi1 if spectral else None, pi2 if spectral else None) as sc:
        g = sc.scan([codes], [pairs])[0]
    rel = np.abs(g["score"]) / np.maximum(1.0, np.abs(g["pair_ll"]))
    print("product model on the GPU: |score| / max(1, |pair_ll|) =", rel.max())
    assert np.abs(g["pair_ll"]).max() > 5
    assert rel.max() <= PRODUCT_BAR


# ------------------------------------------------------------------------------------------------- 4. bitwise stability
def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.int64) if b[k].dtype == np.float64 else b[k]) for k in a)


def test_runs_handles_and_batches_agree_bitwise():
    z = case("s4_b129_spectral_cherry")
    codes, pairs = [c for c, _ in z["families"]], [p for _, p in z["families"]]
    with _scanner(z) as sc, _scanner(z) as other:
        first = sc.scan(codes, pairs)
        again = sc.scan(codes, pairs)
        elsewhere = other.scan(codes, pairs)
        alone = [sc.scan([c], [p])[0] for c, p in zip(codes, pairs)]
        swapped = sc.scan(codes[::-1], pairs[::-1])[::-1]
    for f in range(len(codes)):
        assert _same_bits(first[f], again[f]) and _same_bits(first[f], elsewhere[f])
        assert _same_bits(first[f], alone[f]) and _same_bits(first[f], swapped[f])
        for key in ("score", "pair_ll", "indep_ll", "n_used"):
            m = first[f][key]
            assert np.array_equal(m, m.T) and np.all(np.diag(m) == 0), key
        assert np.array_equal(first[f]["score"].view(np.int64), first[f]["score"].T.view(np.int64))
        assert np.all(np.isfinite(first[f]["score"]))


# ----------------------------------------------------------------------------------------------------------- 5. recovery
def test_the_scan_recovers_the_simulated_contacts(tmp_path):
    """a random 64-leaf tree, 40 sites, ten contacting pairs 20 apart evolving under a Q_2 tilted towards equal states
    (cr.tilted_pair_model); seed RECOVERY_SEED = 2 and tilt 2.0 were chosen on the CPU, where the ten true pairs are the
    restatement's top ten by apc with a relative gap of 0.3465 to the best false pair (test_coscan_cpu.py)"""
    from cherryml_amd import simulate_msas
    z = cr.recovery_inputs(str(tmp_path))
    p = z["paths"]
    msas = str(tmp_path / "msas")
    simulate_msas(tree_dir=z["tree_dir"], site_rates_dir=z["site_rates_dir"], contact_map_dir=z["contact_map_dir"], families=["fam"],
                  amino_acids=cr.RECOVERY_STATES, pi_1_path=p["pi_1"], Q_1_path=p["Q_1"], pi_2_path=p["pi_2"], Q_2_path=p["Q_2"],
                  strategy="all_transitions", random_seed=z["seed"], output_msa_dir=msas)
    out = str(tmp_path / "scan")
    coevolution_scan(tree_dir=z["tree_dir"], msa_dir=msas, families=["fam"], amino_acids=cr.RECOVERY_STATES,
                     rate_matrix_path=p["Q_1"], coevolution_rate_matrix_path=p["Q_2"], quantization_points=cr.RECOVERY_GRID,
                     edge_or_cherry=cr.RECOVERY_MODE, minimum_distance_for_nontrivial_contact=cr.RECOVERY_MIN_DIST,
                     output_scan_dir=out)
    rank = read_coevolution_scan(out, "fam")["ranking"]
    top = {(int(i), int(j)) for i, j in zip(rank["i"][:10], rank["j"][:10])}
    print("recovery on the GPU: top ten", sorted(top), "apc gap", (rank["apc"][9] - rank["apc"][10]) / abs(rank["apc"][9]))
    assert top == set(cr.RECOVERY_CONTACTS)


# ------------------------------------------------------------------------------------------------------ 6. the stage
ACGT = list("ACGT")


def _write_rate_matrix(path, Q, states):
    from cherryml_amd.io import write_rate_matrix
    write_rate_matrix(Q, states, path)


def _stage_inputs(tmp_path):
    """two families on disk: eight leaves in four cherries (30 sites, gaps), and two cherries (12 sites)"""
    rng = np.random.default_rng(4)
    (tmp_path / "trees").mkdir()
    (tmp_path / "msas").mkdir()
    fams = {}
    for fam, n_cherries, L in (("fam_a", 4, 30), ("fam_b", 2, 12)):
        nodes, edges = ["root"], []
        for k in range(n_cherries):
            nodes += [f"p{k}", f"x{k}", f"y{k}"]
            edges += [("root", f"p{k}", 0.3), (f"p{k}", f"x{k}", float(rng.uniform(0.05, 1.0))),
                      (f"p{k}", f"y{k}", float(rng.uniform(0.05, 1.0)))]
        (tmp_path / "trees" / f"{fam}.txt").write_text(
            f"{len(nodes)} nodes\n" + "\n".join(nodes) + f"\n{len(edges)} edges\n" + "\n".join(f"{u} {v} {t!r}" for u, v, t in edges) + "\n")
        seqs = {v: "".join(rng.choice(list("ACGT-"), L, p=[0.22, 0.22, 0.22, 0.22, 0.12])) for v in nodes}
        (tmp_path / "msas" / f"{fam}.txt").write_text("".join(f">{v}\n{s}\n" for v, s in seqs.items()))
        fams[fam] = L
    Q1, _ = cr.random_reversible(4, 1)
    Q2, _ = cr.random_reversible(16, 2)
    _write_rate_matrix(str(tmp_path / "q1.txt"), Q1, ACGT)
    _write_rate_matrix(str(tmp_path / "q2.txt"), Q2, [a + b for a in ACGT for b in ACGT])
    return fams, Q1, Q2


def _stage_want(tmp_path, fam, grid, Q1, Q2, mode):
    nodes, children, root = co.read_tree(str(tmp_path / "trees" / f"{fam}.txt"))
    msa = co.read_msa(str(tmp_path / "msas" / f"{fam}.txt"))
    row = {v: r for r, v in enumerate(nodes)}
    codes = np.array([["ACGT".find(ch) for ch in msa[v]] for v in nodes], dtype=np.int8)
    pairs = [(row[a], row[b], la, lb) for a, b, la, lb in co.transition_pairs(nodes, children, root, mode)]
    return cr.scan(codes, pairs, grid, cr.log_bank(cr.bank(Q1, grid)), cr.log_bank(cr.bank(Q2, grid)), mode != "edge")


@pytest.mark.parametrize("mode", ["cherry", "edge"])
def test_the_stage_writes_what_the_scanner_computes(tmp_path, mode):
    fams, Q1, Q2 = _stage_inputs(tmp_path)
    grid = [0.05, 0.2, 0.6, 1.5, 4.0]
    out = str(tmp_path / "scan")
    coevolution_scan(tree_dir=str(tmp_path / "trees"), msa_dir=str(tmp_path / "msas"), families=list(fams), amino_acids=ACGT,
                     rate_matrix_path=str(tmp_path / "q1.txt"), coevolution_rate_matrix_path=str(tmp_path / "q2.txt"),
                     quantization_points=grid, edge_or_cherry=mode, minimum_distance_for_nontrivial_contact=7, output_scan_dir=out)
    for fam, L in fams.items():
        with np.load(os.path.join(out, fam + ".npz")) as z:
            assert sorted(z.files) == ["apc", "indep_ll", "n_used", "pair_ll", "score"]
            got = {k: z[k] for k in z.files}
        want = _stage_want(tmp_path, fam, np.array(grid), Q1, Q2, mode)
        for key in ("score", "pair_ll", "indep_ll"):
            assert got[key].shape == (L, L) and _worst(got[key], want[key]) <= 1e-10, (fam, key)
        assert np.array_equal(got["n_used"], want["n_used"]) and got["n_used"].max() > 0
        apc = cr.apc(got["score"])
        assert np.abs(got["apc"] - apc).max() <= 1e-12 * max(1.0, np.abs(apc).max())
        lines = open(os.path.join(out, fam + ".txt")).read().splitlines()
        assert lines[0] == "i j score apc n_used"
        rows = [ln.split(" ") for ln in lines[1:]]
        listed = [(int(r[0]), int(r[1])) for r in rows]
        masked = [(i, j) for i in range(L) for j in range(i + 7, L) if got["n_used"][i, j] > 0]
        assert sorted(listed) == masked and len(masked) > 0                          # the distance mask, nothing else
        assert listed == sorted(masked, key=lambda ij: (-got["apc"][ij], ij))        # apc descending, then (i, j)
        for r, (i, j) in zip(rows, listed):
            assert (float(r[2]), float(r[3]), int(r[4])) == (got["score"][i, j], got["apc"][i, j], got["n_used"][i, j])
        back = read_coevolution_scan(out, fam)
        assert all(np.array_equal(back[k], got[k]) for k in got)
        assert [(int(a), int(b)) for a, b in zip(back["ranking"]["i"], back["ranking"]["j"])] == listed
        assert np.array_equal(back["ranking"]["apc"], [got["apc"][ij] for ij in listed])


def test_the_second_call_is_a_cache_hit(tmp_path, monkeypatch):
    from cherryml_amd.coevolution import _scan
    fams, _, _ = _stage_inputs(tmp_path)
    kw = dict(tree_dir=str(tmp_path / "trees"), msa_dir=str(tmp_path / "msas"), families=list(fams), amino_acids=ACGT,
              rate_matrix_path=str(tmp_path / "q1.txt"), coevolution_rate_matrix_path=str(tmp_path / "q2.txt"),
              quantization_points=[0.05, 0.5, 4.0])
    before = caching.get_cache_dir()
    caching.set_cache_dir(str(tmp_path / "cache"))
    try:
        first = coevolution_scan(**kw)
        assert os.path.exists(os.path.join(first["output_scan_dir"], "result.success"))
        assert os.path.exists(os.path.join(first["output_scan_dir"], "fam_a.npz"))

        def boom(*a, **k):
            raise AssertionError("the stage ran again")

        monkeypatch.setattr(_scan, "CoevolutionScanner", boom)
        assert coevolution_scan(num_processes=3, **kw) == first          # a hit: nothing runs, the same directory
        with pytest.raises(AssertionError, match="ran again"):
            coevolution_scan(**dict(kw, minimum_distance_for_nontrivial_contact=3))   # another key: it would run
    finally:
        caching.set_cache_dir(before)


def test_refusals_name_the_value_and_leave_the_scanner_usable():
    z = case("s2_b5_general_cherry")
    codes, pairs = z["families"][2]
    L = codes.shape[1]
    Q21 = cr.random_general(21, 1)
    with pytest.raises(_lib.CherryBankError, match="S = 21"):
        CoevolutionScanner(Q21, cr.random_general(441, 2), z["grid"])
    with pytest.raises(_lib.CherryBankError, match=r"B = 1 "):
        CoevolutionScanner(z["Q1"], z["Q2"], [0.5])
    with _scanner(z) as sc:
        good = sc.scan([codes], [pairs])[0]
        bad = codes.copy()
        bad[pairs[0][0], 5] = 2
        with pytest.raises(_lib.CherryBankError, match=r"state code 2 out of range \[-1, 2\) at site 5"):
            sc.scan([bad], [pairs])
        bad[pairs[0][0], 5] = -2
        with pytest.raises(_lib.CherryBankError, match="state code -2 out of range"):
            sc.scan([bad], [pairs])
        flat = np.ascontiguousarray(codes.reshape(-1))
        rec = np.array([(a * L, b * L, 0, 0, 0, la, lb) for a, b, la, lb in pairs], dtype=PAIR_DTYPE)
        rec["seq_b"][4] = flat.size - L + 1
        with pytest.raises(_lib.CherryBankError, match=rf"sequence offset {flat.size - L + 1} \+ L = {L} lies beyond seqs_bytes = {flat.size}"):
            sc.scan_records([L], [flat], [rec])
        with pytest.raises(_lib.CherryBankError, match="family 1 has L = 0"):
            sc.scan([codes, np.zeros((2, 0), np.int8)], [pairs, []])
        assert _same_bits(sc.scan([codes], [pairs])[0], good)
    with pytest.raises(_lib.CherryBankError, match="closed"):
        sc.scan([codes], [pairs])
