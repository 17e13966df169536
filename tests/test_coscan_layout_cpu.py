"""The host layout of the co-evolution scan without a GPU: csrc/coscan_layout.h (a call's checks, the bucket of every sequence
pair, the order the kernel walks them in, the tile list and the families' offsets) built into tests/coscan_layout_driver.cpp with
the host compiler under AddressSanitizer + UBSan and run as a child process; every integer against a restatement in NumPy (the
quantisation rule is tests/coscan_reference.py's), every refusal against the library's code and text."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from coscan_reference import quantize  # noqa: E402

CB_EINVAL = -1
TILE = 16
GRID = [0.25, 1.0, 4.0, 16.0]   # powers of two: the ratio midpoints 0.5, 2, 8 are exact


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("coscan_layout") / "coscan_layout_driver")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "coscan_layout_driver.cpp"), "-o", exe])
    return exe


def _arr(x, real=False):
    x = np.asarray(x).reshape(-1)
    return " ".join([str(x.size)] + [float(v).hex() if real else "%d" % v for v in x])


def _run(driver, tmp_path, what, ints, *arrays):
    path = tmp_path / "case.txt"
    path.write_text(" ".join([what] + ["%d" % v for v in ints]) + "\n" + "\n".join(arrays) + "\n")
    p = subprocess.run([driver, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert lines[0].startswith("rc ") and lines[1].startswith("msg")
    return int(lines[0][3:]), lines[1][4:], {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in lines[2:]}


def _layout(driver, tmp_path, S, fams, grid=GRID, seqs=None):
    """fams: [(L, [(seq_a, seq_b, len_a, len_b)])]; seqs: the code buffer (default: zeros, large enough for every offset)"""
    recs = [r for _, prs in fams for r in prs]
    if seqs is None:
        need = max([max(r[0], r[1]) + L for L, prs in fams for r in prs] + [1])
        seqs = np.zeros(need, dtype=np.int8)
    col = lambda k, real=False: _arr([r[k] for r in recs], real)   # noqa: E731
    return _run(driver, tmp_path, "layout", (S, len(fams)), _arr(grid, real=True), _arr([L for L, _ in fams]), _arr(seqs),
                col(0), col(1), col(2, True), col(3, True), _arr([len(prs) for _, prs in fams]))


def expected(fams, grid=GRID):
    fam, pairs, tiles, n_out = [], [], [], 0
    for f, (L, prs) in enumerate(fams):
        kept = [(quantize(la + lb, np.asarray(grid)), k, a, b) for k, (a, b, la, lb) in enumerate(prs)]
        kept = sorted(x for x in kept if x[0] is not None)          # by bucket, ties by pair index
        fam += [n_out, len(pairs) // 4, L, len(kept)]
        for q, k, a, b in kept:
            pairs += [a, b, q, k]
        nt = -(-L // TILE)
        tiles += [v for ti in range(nt) for tj in range(ti, nt) for v in (f, ti, tj)]
        n_out += L * L
    return dict(n_out=[n_out], fam=fam, pairs=pairs, tiles=tiles)


def _random_pairs(rng, n, L, n_seq):
    lens = rng.choice([0.1, 0.25, 0.3, 0.5, 0.9, 1.0, 2.0, 3.0, 8.0, 15.9, 16.0, 16.5], n)
    return [(int(rng.integers(0, n_seq)) * L, int(rng.integers(0, n_seq)) * L, float(t) * 0.25, float(t) * 0.75) for t in lens]


@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 32, 33, 100])
def test_one_family_s_integers_equal_the_restatement(driver, tmp_path, L):
    rng = np.random.default_rng(L)
    fams = [(L, _random_pairs(rng, 23, L, 6))]
    rc, msg, got = _layout(driver, tmp_path, 4, fams)
    assert (rc, msg) == (0, "")
    want = expected(fams)
    assert got == want
    nt = -(-L // TILE)
    assert len(want["tiles"]) == 3 * nt * (nt + 1) // 2
    qs = want["pairs"][2::4]
    assert qs == sorted(qs) and len(qs) < 23                        # some pairs are off the grid and gone


def test_ties_keep_the_pair_index_order_and_dropped_pairs_leave_their_index_behind(driver, tmp_path):
    #             q: 1      off     0      1      3     off    0
    lens = [1.0, 0.1, 0.25, 0.9, 16.0, 16.5, 0.3]
    fams = [(3, [(3 * k, 3 * (k + 1), t, 0.0) for k, t in enumerate(lens)])]
    rc, msg, got = _layout(driver, tmp_path, 4, fams)
    assert (rc, msg) == (0, "")
    assert got["pairs"][2::4] == [0, 0, 1, 1, 3] and got["pairs"][3::4] == [2, 6, 0, 3, 4]
    assert got == expected(fams)


def test_three_families_keep_every_offset(driver, tmp_path):
    rng = np.random.default_rng(5)
    fams = [(17, _random_pairs(rng, 9, 17, 4)), (1, []), (40, _random_pairs(rng, 70, 40, 8))]
    # the second and third family's sequences lie behind the first's
    fams[2] = (40, [(a + 100, b + 100, la, lb) for a, b, la, lb in fams[2][1]])
    rc, msg, got = _layout(driver, tmp_path, 4, fams)
    assert (rc, msg) == (0, "")
    want = expected(fams)
    assert got == want
    assert want["fam"][0::4] == [0, 289, 290] and want["n_out"] == [289 + 1 + 1600]
    assert want["fam"][6:8] == [1, 0] and want["fam"][5] == want["fam"][9]      # the empty family: no pairs, one tile
    assert want["tiles"][3 * 3:3 * 4] == [1, 0, 0]


def test_the_buckets_follow_the_counter_s_rule_at_the_ends_and_the_ratio_midpoints(driver, tmp_path):
    lens = [0.0, 0.125, 0.25, 0.5, 2.0, 8.0, 1.0, 16.0, 32.0, 0.49999, 0.7, 3.99]
    rc, msg, got = _run(driver, tmp_path, "quantize", (), _arr(GRID, real=True), _arr(lens, real=True))
    assert (rc, msg) == (0, "")
    want = [quantize(t, np.asarray(GRID)) for t in lens]
    assert got["q"] == [-1 if q is None else q for q in want] == [-1, -1, 0, 1, 2, 3, 1, 3, -1, 0, 1, 2]
    grid = np.exp(np.linspace(np.log(1e-3), np.log(20.0), 129))
    lens = np.exp(np.random.default_rng(2).uniform(np.log(5e-4), np.log(40.0), 500))
    rc, msg, got = _run(driver, tmp_path, "quantize", (), _arr(grid, real=True), _arr(lens, real=True))
    assert got["q"] == [-1 if quantize(t, grid) is None else quantize(t, grid) for t in lens]


REFUSALS = [
    ("L_zero", 4, [(0, [])], None, "cb_coscan_run: family 0 has L = 0"),
    ("L_negative_in_the_second_family", 4, [(3, []), (-2, [])], None, "cb_coscan_run: family 1 has L = -2"),
    ("offset_beyond_the_buffer", 4, [(5, [(0, 6, 1.0, 0.0)])], np.zeros(10, np.int8),
     "cb_coscan_run: family 0 pair 0: sequence offset 6 + L = 5 lies beyond seqs_bytes = 10"),
    ("negative_offset", 4, [(5, [(0, 5, 1.0, 0.0), (-1, 0, 1.0, 0.0)])], np.zeros(10, np.int8),
     "cb_coscan_run: family 0 pair 1: sequence offset -1 + L = 5 lies beyond seqs_bytes = 10"),
    ("code_equal_to_S", 4, [(5, [(0, 5, 1.0, 0.0)])], np.array([0, 1, 2, 3, -1, 0, 1, 4, 3, 2], np.int8),
     "cb_coscan_run: family 0 pair 0: state code 4 out of range [-1, 4) at site 2"),
    ("code_below_minus_one_in_a_dropped_pair", 4, [(5, [(0, 5, 99.0, 0.0)])], np.array([0, 1, -2, 3, -1, 0, 1, 3, 3, 2], np.int8),
     "cb_coscan_run: family 0 pair 0: state code -2 out of range [-1, 4) at site 2"),
]


@pytest.mark.parametrize("name,S,fams,seqs,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_keep_code_and_text(driver, tmp_path, name, S, fams, seqs, text):
    rc, msg, got = _layout(driver, tmp_path, S, fams, seqs=seqs)
    assert (rc, msg, got) == (CB_EINVAL, text, {})


def test_the_last_sequence_may_end_with_the_buffer(driver, tmp_path):
    fams = [(5, [(0, 5, 1.0, 0.0)])]
    rc, msg, got = _layout(driver, tmp_path, 4, fams, seqs=np.array([0, 1, 2, 3, -1, 0, 1, 3, 3, 2], np.int8))
    assert (rc, msg) == (0, "") and got == expected(fams)


@pytest.mark.parametrize("S,grid,text", [
    (1, GRID, "cb_coscan_create: S = 1 (2 <= S <= 20: the pair model has S^2 <= 400 states)"),
    (21, GRID, "cb_coscan_create: S = 21 (2 <= S <= 20: the pair model has S^2 <= 400 states)"),
    (4, [1.0], "cb_coscan_create: B = 1 (at least 2 grid points)"),
    (4, [0.5, 0.25, 1.0], "cb_coscan_create: the grid must be positive and strictly increasing (grid[1] = 0.25)"),
    (4, [0.0, 0.25], "cb_coscan_create: the grid must be positive and strictly increasing (grid[0] = 0)"),
    (2, GRID, None), (20, GRID, None),
])
def test_the_model_s_checks(driver, tmp_path, S, grid, text):
    rc, msg, _ = _run(driver, tmp_path, "model", (S,), _arr(grid, real=True))
    assert (rc, msg) == ((0, "") if text is None else (CB_EINVAL, text))
