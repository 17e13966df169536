"""The host side of FastCherries without a GPU: csrc/ble_layout.h (rate priors, per-site totals, initial bins, transposes, size
checks, the offsets of a batch) built into tests/ble_layout_driver.cpp with the host compiler under AddressSanitizer + UBSan and
run as a child process; every integer against tests/ble_reference.py and oracle/ble_oracle.py, every refusal against the
library's code and text.  Then, through the library itself, what each cb_ble* entry refuses before it looks for a device."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ble_reference as ref  # noqa: E402
from test_ble_cpu import staircase  # noqa: E402

CB_EINVAL = -1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ble_layout") / "ble_layout_driver")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "ble_layout_driver.cpp"), "-o", exe])
    return exe


def _arr(x, real=False):
    """an array of the case file; doubles as hexadecimal literals (exact)"""
    x = np.asarray(x).reshape(-1)
    return " ".join([str(x.size)] + [float(v).hex() if real else "%d" % v for v in x])


def _run(driver, tmp_path, what, ints, *arrays):
    path = tmp_path / "case.txt"
    path.write_text(" ".join([what] + ["%d" % v for v in ints]) + "\n" + "\n".join(arrays) + "\n")
    p = subprocess.run([driver, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert lines[0].startswith("rc ") and lines[1].startswith("msg")
    return int(lines[0][3:]), lines[1][4:], {ln.split()[0]: ln.split()[1:] for ln in lines[2:]}


def _ints(row):
    return [int(v) for v in row]


# ---------------------------------------------------------------- totals and bins
def _bins_cases():
    rng = np.random.default_rng(77)
    gaps = rng.integers(-1, 4, (9, 12))
    gaps[:, [0, 5, 11]] = -1                                # all-gap columns: total 0, first in the order
    equal = np.tile(np.array([[0], [1], [1], [-1]]), (1, 7))   # every site has the same total: the order is the site index
    below_one = rng.integers(-1, 5, (6, 10))
    return [
        # name, all_seqs [n_seqs, L], S, weights
        ("one_site", rng.integers(-1, 4, (5, 1)), 4, ref.equal_weights(3)),
        ("one_sequence", rng.integers(-1, 20, (1, 9)), 20, ref.equal_weights(4)),
        ("all_gap_columns", gaps, 4, ref.equal_weights(4)),
        ("equal_totals", equal, 2, ref.equal_weights(3)),
        ("halves_of_six", staircase(6, [4, 0, 5, 2, 1, 3]), 2, [0.25, 0.75, 1.0]),
        ("halves_of_ten", staircase(10, [7, 2, 9, 0, 4, 1, 8, 3, 6, 5]), 2, [0.25, 0.6, 1.0]),
        ("one_category", rng.integers(-1, 20, (7, 13)), 20, [1.0]),
        ("more_categories_than_sites", rng.integers(-1, 20, (7, 3)), 20, ref.equal_weights(8)),
        ("weights_end_below_one", below_one, 5, [0.2, 0.5, 0.7]),
        ("two_states", rng.integers(-1, 2, (11, 33)), 2, ref.equal_weights(4)),
        ("127_states", np.concatenate([rng.integers(-1, 127, (14, 21)), np.full((1, 21), 126)]), 127, ref.equal_weights(4)),
        ("random", rng.integers(-1, 20, (40, 65)), 20, ref.equal_weights(20)),
    ]


BINS = _bins_cases()


@pytest.mark.parametrize("name,seqs,S,weights", BINS, ids=[c[0] for c in BINS])
def test_totals_and_bins_equal_the_restatement_and_the_oracle(driver, tmp_path, name, seqs, S, weights):
    from oracle import ble_oracle as bo
    n_seqs, L = seqs.shape
    R = len(weights)
    rc, msg, got = _run(driver, tmp_path, "bins", (S, R, n_seqs, L), _arr(seqs), _arr(weights, real=True))
    assert (rc, msg) == (0, "")
    totals = ref.site_totals(seqs, S)
    assert _ints(got["totals"]) == totals.tolist()
    want = ref.initial_bins(totals, weights)
    assert np.array_equal(want, bo.initial_site_rates(seqs, weights, S))
    if name == "weights_end_below_one":
        # the reference's category runs past the last one (and its caller then reads rates[R]); the library stops at R - 1
        assert want.max() == R
        want = np.minimum(want, R - 1)
    assert want.max() <= R - 1
    assert _ints(got["bins"]) == want.tolist()
    # the resident entry's path (totals from the device, then the bins) is the per-call entries' path (sequences, then both)
    assert got["bins_from_totals"] == got["bins"]
    if name == "equal_totals":
        assert len(set(totals.tolist())) == 1 and want.tolist() == sorted(want.tolist()) and want.tolist() == [0, 0, 1, 1, 1, 2, 2]
    if name == "all_gap_columns":
        assert totals[[0, 5, 11]].tolist() == [0, 0, 0] and want[[0, 5, 11]].tolist() == [0, 0, 0]
    if name == "halves_of_six":
        assert want.tolist() == [0, 1, 1, 2, 0, 1]
    if name == "halves_of_ten":
        assert want.tolist() == [1, 1, 0, 2, 1, 2, 2, 0, 2, 0]
    if name == "more_categories_than_sites":
        assert R > L and len(set(want.tolist())) == L


def test_a_code_below_minus_one_is_a_gap_and_a_code_of_S_is_refused(driver, tmp_path):
    seqs = np.array([[0, 1, 2], [2, -3, 0], [1, 1, -128]])
    rc, msg, got = _run(driver, tmp_path, "bins", (3, 2, 3, 3), _arr(seqs), _arr([0.5, 1.0], real=True))
    assert (rc, msg) == (0, "")
    assert _ints(got["totals"]) == ref.site_totals(np.where(seqs < 0, -1, seqs), 3).tolist()
    seqs[2, 2] = 3
    rc, msg, got = _run(driver, tmp_path, "bins", (3, 2, 3, 3), _arr(seqs), _arr([0.5, 1.0], real=True))
    assert (rc, msg, got) == (CB_EINVAL, "cb_ble: state code out of range", {})


# ---------------------------------------------------------------- transposes
@pytest.mark.parametrize("n,L", [(1, 1), (3, 5), (64, 65)])
@pytest.mark.parametrize("at", [0, 37])
def test_transposes_are_exact(driver, tmp_path, n, L, at):
    """at > 0: into a family's place in the concatenated buffer of a batch; the bytes in front of it stay as they were"""
    c = np.random.default_rng(n * 100 + L).integers(-1, 127, (n, L))
    rc, msg, got = _run(driver, tmp_path, "transpose", (n, L, at), _arr(c))
    assert (rc, msg) == (0, "")
    assert _ints(got["t"]) == [-128] * at + c.T.reshape(-1).tolist()


# ---------------------------------------------------------------- the offsets of a batch
@pytest.mark.parametrize("n,L,n_seqs", [([4], [9], [8]), ([3, 70, 1], [5, 2049, 7], [6, 141, 1])], ids=["one", "three_ragged"])
def test_batch_offsets(driver, tmp_path, n, L, n_seqs):
    rc, msg, got = _run(driver, tmp_path, "offsets", (len(n),), _arr(n), _arr(L), _arr(n_seqs))
    assert (rc, msg) == (0, "")
    n, L, n_seqs = (np.array(v, dtype=np.int64) for v in (n, L, n_seqs))
    for key, steps in (("off_c", n * L), ("off_n", n), ("off_L", L), ("off_s", n_seqs * L)):
        assert _ints(got[key]) == [0] + np.cumsum(steps).tolist(), key


@pytest.mark.parametrize("which,family", [("n", 0), ("L", 1), ("n_seqs", 2), ("L", 2)])
def test_batch_offsets_name_the_family_with_a_zero_size(driver, tmp_path, which, family):
    sizes = dict(n=[3, 70, 1], L=[5, 2049, 7], n_seqs=[6, 141, 1])
    sizes[which][family] = 0
    rc, msg, got = _run(driver, tmp_path, "offsets", (3,), _arr(sizes["n"]), _arr(sizes["L"]), _arr(sizes["n_seqs"]))
    assert (rc, msg, got) == (CB_EINVAL, "cb_ble_batch: family %d has bad sizes" % family, {})


# ---------------------------------------------------------------- priors
@pytest.mark.parametrize("R", [1, 4, 20])
def test_priors(driver, tmp_path, R):
    """the C library's log and NumPy's may differ in the last place: 4 units in the last place of the larger of |2 log r| and
    |3 r| (2 log r - 3 r is at most about -2.8: no cancellation amplifies the difference)"""
    rates = ref.RATES[R]
    rc, msg, got = _run(driver, tmp_path, "priors", (R,), _arr(rates, real=True))
    assert (rc, msg) == (0, "")
    mine = np.array([float.fromhex(v) for v in got["priors"]])
    bound = 4 * np.spacing(np.maximum(np.abs(2 * np.log(rates)), np.abs(3 * rates)))
    assert mine.shape == (R,) and np.all(np.abs(mine - ref.priors(rates)) <= bound)


# ---------------------------------------------------------------- refusals of the size checks and the code scan
@pytest.mark.parametrize("sizes,ok", [((2, 1, 1, 1, 1), True), ((127, 129, 20, 2050, 2049), True), ((1, 4, 2, 2, 5), False),
                                      ((128, 4, 2, 2, 5), False), ((3, 0, 2, 2, 5), False), ((3, 4, 0, 2, 5), False),
                                      ((3, 4, 2, 0, 5), False), ((3, 4, 2, 2, 0), False), ((3, 4, 2, -1, 5), False)])
def test_size_check_keeps_code_and_text(driver, tmp_path, sizes, ok):
    rc, msg, _ = _run(driver, tmp_path, "sizes", sizes)
    assert (rc, msg) == ((0, "") if ok else (CB_EINVAL, "ble: bad sizes"))


def test_code_scan_keeps_code_and_text(driver, tmp_path):
    cx = np.array([[0, 1, 2, -1, 2], [2, 2, -7, 0, 1]])     # (any negative code is a gap here)
    cy = np.array([[2, 2, 2, 2, -128], [0, 0, 0, 0, 2]])
    assert _run(driver, tmp_path, "codes", (3, 2, 5), _arr(cx), _arr(cy))[:2] == (0, "")
    for which, at in ((0, (1, 4)), (1, (1, 4)), (0, (0, 0)), (1, (0, 2))):
        bad = [cx.copy(), cy.copy()]
        bad[which][at] = 3
        rc, msg, _ = _run(driver, tmp_path, "codes", (3, 2, 5), _arr(bad[0]), _arr(bad[1]))
        assert (rc, msg) == (CB_EINVAL, "ble: state code out of range"), (which, at)


# ---------------------------------------------------------------- through the library: what comes before the device check
def _call(entry, **kw):
    """entry(...) with small valid arguments (S = 3, T = 4, R = 2, n = 2, L = 5), each replaceable: an integer by its name, an
    array by its name (None passes NULL; `handle`: the address itself)"""
    from cherryml_amd import _lib
    S, T, R, n, L, device = (kw.pop(k, v) for k, v in (("S", 3), ("T", 4), ("R", 2), ("n", 2), ("L", 5), ("device", 0)))
    a = dict(logP=np.zeros((4, 2, 3, 3)), Q=np.zeros((3, 3)), grid=np.ones(4), rates=np.ones(2), weights=np.array([0.5, 1.0]),
             priors=np.zeros(2), tens=np.zeros((2, 2, 3, 3)), cx=np.zeros((2, 5), np.int8), cy=np.zeros((2, 5), np.int8),
             seqs=np.zeros((4, 5), np.int8), s2r=np.zeros(5, np.int32), li=np.zeros(2, np.int32), out_n=np.zeros(2, np.int32),
             out_L=np.zeros(5, np.int32), ns=np.array([2], np.int32), Ls=np.array([5], np.int32), nq=np.array([4], np.int32),
             handle=np.zeros(64), out_h=np.zeros(1, np.int64))
    n_seqs, n_fam, max_iters = kw.pop("n_seqs", 4), kw.pop("n_fam", 1), kw.pop("max_iters", 3)
    handle = kw.pop("handle") if isinstance(kw.get("handle"), int) else None
    for k in [k for k, v in kw.items() if v is not None]:
        a[k] = np.ascontiguousarray(kw.pop(k), dtype=a[k].dtype)
    p = {k: v.ctypes.data for k, v in a.items()}
    for k in kw:
        p[k] = None
    if handle is not None:
        p["handle"] = handle
    args = {
        "cb_ble_log_bank": (device, S, T, R, p["Q"], None, p["grid"], p["rates"], p["logP"]),
        "cb_ble_branch_lengths": (device, S, T, R, p["logP"], p["cx"], p["cy"], n, L, p["s2r"], p["out_n"]),
        "cb_ble_site_rates": (device, S, T, R, p["logP"], p["cx"], p["cy"], n, L, p["li"], p["priors"], p["out_L"]),
        "cb_ble": (device, S, T, R, p["logP"], p["cx"], p["cy"], n, L, p["seqs"], n_seqs, p["rates"], p["weights"], max_iters,
                   p["out_n"], p["out_L"], None, None),
        "cb_ble_batch": (device, S, T, R, p["logP"], n_fam, p["ns"], p["Ls"], p["cx"], p["cy"], p["seqs"], p["nq"], p["rates"],
                         p["weights"], max_iters, p["out_n"], p["out_L"], None, None),
        "cb_ble_bank_create": (device, S, T, R, p["logP"], p["rates"], p["out_h"]),
        # (the handle is not looked at before the sizes are: zero bytes stand in for one)
        "cb_ble_bank_run": (p["handle"], p["cx"], p["cy"], n, L, p["seqs"], n_seqs, p["weights"], max_iters, p["out_n"],
                            p["out_L"], None, None),
        "cb_site_rate_gather": (device, S, R, n, L, p["tens"], p["cx"], p["cy"], p["priors"], p["out_L"]),
    }[entry]
    lib = _lib.load()
    rc = getattr(lib, entry)(*args)
    return rc, (lib.cb_last_error() or b"").decode()


POINTERS = {
    "cb_ble_log_bank": ["Q", "grid", "rates", "logP"],
    "cb_ble_branch_lengths": ["logP", "cx", "cy", "s2r", "out_n"],
    "cb_ble_site_rates": ["logP", "cx", "cy", "li", "priors", "out_L"],
    "cb_ble": ["logP", "cx", "cy", "seqs", "rates", "weights", "out_n", "out_L"],
    "cb_ble_batch": ["logP", "ns", "Ls", "cx", "cy", "seqs", "nq", "rates", "weights", "out_n", "out_L"],
    "cb_ble_bank_create": ["logP", "rates", "out_h"],
    "cb_ble_bank_run": ["handle", "cx", "cy", "seqs", "weights", "out_n", "out_L"],
    "cb_site_rate_gather": ["tens", "cx", "cy", "priors", "out_L"],
}


@pytest.mark.parametrize("entry", sorted(POINTERS))
def test_every_entry_refuses_a_null_argument(entry):
    for name in POINTERS[entry]:
        assert _call(entry, **{name: None}) == (CB_EINVAL, entry + ": NULL argument"), name


BAD = dict(S_low=dict(S=1), S_high=dict(S=128), T=dict(T=0), R=dict(R=0), n=dict(n=0), L=dict(L=0))
BAD_SIZES = (
    [("cb_ble_log_bank", BAD[k], "cb_ble_log_bank: bad sizes") for k in ("S_low", "T", "R")]
    + [(e, BAD[k], "ble: bad sizes") for e in ("cb_ble_branch_lengths", "cb_ble_site_rates", "cb_ble") for k in BAD]
    + [("cb_site_rate_gather", BAD[k], "ble: bad sizes") for k in ("S_low", "S_high", "R", "n", "L")]
    + [("cb_ble_bank_create", BAD[k], "cb_ble_bank_create: bad sizes") for k in ("S_low", "S_high", "T", "R")]
    + [("cb_ble_bank_run", kw, "cb_ble_bank_run: bad sizes") for kw in (BAD["n"], BAD["L"], dict(n_seqs=0), dict(max_iters=-1))]
    + [("cb_ble_batch", kw, "cb_ble_batch: bad sizes") for kw in (dict(n_fam=0), dict(max_iters=-1))]
    + [("cb_ble_batch", kw, "cb_ble_batch: family 0 has bad sizes") for kw in (dict(ns=[0]), dict(Ls=[0]), dict(nq=[0]))]
    # the families' sizes come first, then S, T, R
    + [("cb_ble_batch", dict(BAD[k]), "ble: bad sizes") for k in ("S_low", "S_high", "T", "R")]
    + [("cb_ble_batch", dict(S=1, Ls=[0]), "cb_ble_batch: family 0 has bad sizes")]
)


@pytest.mark.parametrize("entry,kw,text", BAD_SIZES, ids=["%s-%s" % (e, "-".join("%s=%s" % i for i in kw.items())) for e, kw, _ in BAD_SIZES])
def test_every_entry_refuses_bad_sizes_before_it_looks_for_a_device(entry, kw, text):
    assert _call(entry, **kw) == (CB_EINVAL, text)
