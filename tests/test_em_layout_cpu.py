"""The host layout of the tree EM handles without a GPU: csrc/em_layout.h (one family's validation and structures, the forest of a
handle, the way back from the device's unit order) built into tests/em_layout_driver.cpp with the host compiler under
AddressSanitizer + UBSan and run as a child process; every integer against a restatement in NumPy written here (the quantisation
rule is tests/em_reference.py's), every refusal against the library's code and text."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from em_reference import quantize  # noqa: E402

CB_EINVAL = -1
S = 4
GRID = [0.25, 1.0, 4.0, 16.0]   # powers of two: the ratio midpoints 0.5, 2, 8 are exact


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("em_layout") / "em_layout_driver")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "em_layout_driver.cpp"), "-o", exe])
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


def _family(driver, tmp_path, parent, length, rates, codes, f=0, grid=GRID):
    return _run(driver, tmp_path, "family", (S, f), _arr(grid, real=True), _arr(parent), _arr(length, real=True),
                _arr(rates, real=True), _arr(codes))


# ---------------------------------------------------------------- the restatement
def expected(parent, length, rates, grid=GRID):
    """every integer of EmFamHost from the parent array, the lengths and the site rates"""
    parent = np.asarray(parent)
    n = parent.size
    root = int(np.flatnonzero(parent == -1)[0])
    children = [np.flatnonzero(parent == v).tolist() for v in range(n)]            # ascending child index
    child_idx = [c for ch in children for c in ch]

    def height(v):                                                                 # the longest path down to a leaf
        return 1 + max(height(c) for c in children[v]) if children[v] else 0

    heights = np.array([height(v) for v in range(n)])
    level_nodes = sorted(range(n), key=lambda v: (heights[v], v))                  # ascending within a height
    bfs, depth = [root], {root: 0}
    for v in bfs:
        for c in children[v]:
            depth[c] = depth[v] + 1
            bfs.append(c)
    inner = [v for v in bfs if v != root and children[v]]                          # breadth first: depths never decrease
    n_depths = max(depth.values()) + 1
    rates = np.asarray(rates, dtype=np.float64)
    cats = np.unique(rates)
    ucat = np.searchsorted(cats, rates)
    perm = np.argsort(ucat, kind="stable")
    qb = [[0 if v == root else quantize(length[v] * c, grid) for c in cats] for v in range(n)]
    return dict(
        sizes=[n, rates.size, cats.size, root],
        child_ptr=np.concatenate([[0], np.cumsum([len(ch) for ch in children])]).tolist(),
        child_idx=child_idx + [0] * (max(n - 1, 1) - len(child_idx)),
        level_ptr=np.concatenate([[0], np.cumsum(np.bincount(heights))]).tolist(),
        level_nodes=level_nodes,
        depth_ptr=np.concatenate([[0], np.cumsum(np.bincount([depth[v] for v in inner], minlength=n_depths))]).tolist(),
        depth_nodes=inner if inner else [0],
        perm=perm.tolist(), unit_cat=ucat[perm].tolist(),
        cat_ptr=np.concatenate([[0], np.cumsum(np.bincount(ucat, minlength=cats.size))]).tolist(),
        qb=[q for row in qb for q in row], cats=cats.tolist())


def _codes(parent, U, seed):
    """leaf rows in [-1, S); the rows of internal nodes are not read: they hold codes out of range"""
    parent = np.asarray(parent)
    c = np.random.default_rng(seed).integers(-1, S, (parent.size, U))
    c[np.isin(np.arange(parent.size), parent)] = 99
    return c


def _check_family(got, want):
    for key, val in want.items():
        if key == "cats":
            assert [float.fromhex(v) for v in got[key]] == val
        else:
            assert _ints(got.get(key, [])) == val, key
    assert set(got) == set(want)


# ---------------------------------------------------------------- one family: trees, rates, lengths
MULTI_LAST = [8, 5, 5, 5, 7, 8, 7, 8, -1]       # root 8: children 0, 5, 7; 5: 1, 2, 3; 7: 4, 6
MULTI_MIDDLE = [4, 0, 0, 0, -1, 4, 5, 5, 4]     # root 4: children 0, 5, 8; 0: 1, 2, 3; 5: 6, 7
TREES = [
    ("one_node", [-1]),
    ("two_nodes", [-1, 0]),
    ("star_of_five_leaves", [-1, 0, 0, 0, 0, 0]),
    ("caterpillar_of_seven", [5, 6, 4, -1, 1, 3, 0]),   # the path 3 - 5 - 0 - 6 - 1 - 4 - 2: height n - 1
    ("multifurcating_root_last", MULTI_LAST),
    ("multifurcating_root_in_the_middle", MULTI_MIDDLE),
]
RATES = [
    ("one_unit", [1.0]),
    ("all_at_one_rate", [0.5] * 5),
    ("all_distinct", [2.0, 0.25, 1.0, 4.0, 0.5]),
    ("unsorted_with_ties", [1.0, 0.5, 1.0, 0.25, 0.5, 1.0, 0.25]),
    ("rate_zero", [0.0, 1.0, 0.0, 2.0]),
]
TREE_RATES = dict(one_node=0, two_nodes=1, star_of_five_leaves=2, caterpillar_of_seven=3, multifurcating_root_last=4,
                  multifurcating_root_in_the_middle=3)


def _lengths(n, seed):
    return np.random.default_rng(seed).uniform(0.05, 30.0, n)


@pytest.mark.parametrize("name,parent", TREES, ids=[t[0] for t in TREES])
def test_a_tree_s_structures_equal_the_restatement(driver, tmp_path, name, parent):
    rates = RATES[TREE_RATES[name]][1]
    length = _lengths(len(parent), 3)
    rc, msg, got = _family(driver, tmp_path, parent, length, rates, _codes(parent, len(rates), 5))
    assert (rc, msg) == (0, "")
    want = expected(parent, length, rates)
    _check_family(got, want)
    if name == "one_node":
        assert (want["child_idx"], want["depth_nodes"], want["depth_ptr"], want["level_ptr"]) == ([0], [0], [0, 0], [0, 1])
    if name == "star_of_five_leaves":
        assert want["depth_ptr"] == [0, 0, 0] and want["depth_nodes"] == [0]     # no internal node but the root: the padded list
    if name == "caterpillar_of_seven":
        assert want["level_ptr"] == list(range(8)) and want["level_nodes"] == [2, 4, 1, 6, 0, 5, 3]
        assert want["depth_nodes"] == [5, 0, 6, 1, 4]
    if name == "multifurcating_root_last":
        assert want["child_idx"] == [1, 2, 3, 4, 6, 0, 5, 7] and want["depth_nodes"] == [5, 7]
        assert want["level_nodes"] == [0, 1, 2, 3, 4, 6, 5, 7, 8]


@pytest.mark.parametrize("name,rates", RATES, ids=[r[0] for r in RATES])
def test_the_rate_categories_and_the_unit_order_equal_the_restatement(driver, tmp_path, name, rates):
    length = _lengths(len(MULTI_MIDDLE), 4)
    rc, msg, got = _family(driver, tmp_path, MULTI_MIDDLE, length, rates, _codes(MULTI_MIDDLE, len(rates), 6))
    assert (rc, msg) == (0, "")
    want = expected(MULTI_MIDDLE, length, rates)
    _check_family(got, want)
    if name == "unsorted_with_ties":       # stable: equal rates keep the caller's order
        assert want["perm"] == [3, 6, 1, 4, 0, 2, 5] and want["cat_ptr"] == [0, 2, 4, 7]
    if name == "all_distinct":
        assert want["perm"] == [1, 4, 2, 0, 3] and want["unit_cat"] == [0, 1, 2, 3, 4]
    if name == "all_at_one_rate":
        assert want["perm"] == [0, 1, 2, 3, 4] and want["cat_ptr"] == [0, 5]
    if name == "rate_zero":                # admitted: every edge of that category is at the grid's first point
        assert want["cats"][0] == 0.0 and all(q == 0 for q in want["qb"][0::3])


def test_lengths_at_below_and_above_the_grid_s_ends_and_at_ratio_midpoints(driver, tmp_path):
    #        below  below   at     midpoints (the upper point)  a point   at     above
    length = [0.0, 0.125, 0.25, 0.5, 2.0, 99.0, 8.0, 1.0, 16.0, 32.0]
    parent = [5, 5, 5, 5, 5, -1, 5, 5, 5, 5]
    rc, msg, got = _family(driver, tmp_path, parent, length, [1.0], _codes(parent, 1, 7))
    assert (rc, msg) == (0, "")
    want = expected(parent, length, [1.0])
    assert want["qb"] == [0, 0, 0, 1, 2, 0, 3, 1, 3, 3]     # (node 5 is the root: its length is not read)
    _check_family(got, want)


# ---------------------------------------------------------------- the forest of a handle
def _forest_inputs():
    fams = [(TREES[i][1], RATES[TREE_RATES[TREES[i][0]]][1]) for i in (0, 3, 4)]
    return [(p, _lengths(len(p), 10 + k), r, _codes(p, len(r), 20 + k)) for k, (p, r) in enumerate(fams)]


def _forest(driver, tmp_path, fams):
    cat = lambda k: np.concatenate([np.asarray(f[k]).reshape(-1) for f in fams])   # noqa: E731
    return _run(driver, tmp_path, "forest", (S,), _arr(GRID, real=True), _arr([len(f[0]) for f in fams]),
                _arr([len(f[2]) for f in fams]), _arr(cat(0)), _arr(cat(1), real=True), _arr(cat(2), real=True), _arr(cat(3)))


def test_a_forest_of_three_families_keeps_every_offset_and_every_family_s_arrays(driver, tmp_path):
    fams = _forest_inputs()
    rc, msg, got = _forest(driver, tmp_path, fams)
    assert (rc, msg) == (0, "")
    got = {k: _ints(v) for k, v in got.items()}
    n = np.array([len(f[0]) for f in fams])
    U = np.array([len(f[2]) for f in fams])
    want = [expected(p, ln, r) for p, ln, r, _ in fams]
    # each family's structures, through the driver's own per-family path as well as from the restatement
    for f, (p, ln, r, c) in enumerate(fams):
        rc, msg, alone = _family(driver, tmp_path, p, ln, r, c, f=f)
        assert (rc, msg) == (0, "")
        _check_family(alone, want[f])
    cum = lambda steps: [0] + np.cumsum(steps).tolist()   # noqa: E731
    assert got["n_fam"] == [3]
    assert got["off_n"] == cum(n) and got["off_u"] == cum(U) and got["off_c"] == cum(n * U)
    assert got["off_q"] == cum([n[f] * want[f]["sizes"][2] for f in range(3)])
    assert got["off_dep"] == cum([len(w["depth_nodes"]) for w in want])
    assert got["parent"] == [v for f in fams for v in f[0]]
    # child_ptr: every family's n + 1 entries, so family f starts at off_n[f] + f; child_idx: one slot per node, n - 1 used
    assert len(got["child_ptr"]) == n.sum() + 3 and len(got["child_idx"]) == n.sum()
    for f in range(3):
        on, w = got["off_n"][f], want[f]
        assert got["child_ptr"][on + f:on + f + n[f] + 1] == w["child_ptr"]
        assert got["child_idx"][on:on + n[f] - 1] == w["child_idx"][:n[f] - 1] and got["child_idx"][on + n[f] - 1] == 0
        assert got["level_nodes"][on:on + n[f]] == w["level_nodes"]
        assert got["depth_nodes"][got["off_dep"][f]:got["off_dep"][f + 1]] == w["depth_nodes"]
        assert got["qb"][got["off_q"][f]:got["off_q"][f + 1]] == w["qb"]
        assert got["unit_cat"][got["off_u"][f]:got["off_u"][f + 1]] == w["unit_cat"]
        # the codes' units in category order
        assert got["codes"][got["off_c"][f]:got["off_c"][f + 1]] == np.asarray(fams[f][3])[:, w["perm"]].reshape(-1).tolist()
    assert len(got["level_nodes"]) == n.sum() and len(got["qb"]) == got["off_q"][3] and len(got["codes"]) == got["off_c"][3]


def test_a_refused_family_names_itself_and_leaves_the_forest_as_it_was(driver, tmp_path):
    fams = _forest_inputs()
    fams[1] = ([5, 6, 4, -1, 1, 3, -1],) + fams[1][1:]
    rc, msg, got = _forest(driver, tmp_path, fams)
    assert (rc, msg) == (CB_EINVAL, "em_layout: family 1 has two roots (3 and 6)")
    assert _ints(got["n_fam"]) == [1] and _ints(got["off_n"]) == [0, 1] and _ints(got["parent"]) == [-1]
    assert len(got["child_ptr"]) == 2 and len(got["codes"]) == 1


# ---------------------------------------------------------------- the way back to the caller's unit order
@pytest.mark.parametrize("width", [1, 2, 20])
def test_scatter_and_sum(driver, tmp_path, width):
    rng = np.random.default_rng(width)
    perm = rng.permutation(11)
    src = np.round(rng.normal(0.0, 40.0, (11, width)))          # (whole numbers: the same values as bytes)
    src[:, 0] += rng.normal(0.0, 1e-9, 11) if width == 1 else 0.0   # width 1: a sum whose bits depend on the order
    rc, msg, got = _run(driver, tmp_path, "scatter", (width,), _arr(perm), _arr(src, real=True))
    assert (rc, msg) == (0, "")
    want = np.empty_like(src)
    want[perm] = src
    assert [float.fromhex(v) for v in got["dst"]] == want.reshape(-1).tolist()
    assert _ints(got["dst8"]) == want.astype(np.int8).reshape(-1).tolist()
    if width == 1:
        s = 0.0
        for x in want[:, 0]:       # in the caller's order, from unit 0 up
            s += float(x)
        assert float.fromhex(got["sum"][0]) == s
    else:
        assert "sum" not in got


# ---------------------------------------------------------------- refusals: code and text
def _refusals():
    ok = dict(parent=[-1, 0, 0], length=[0.0, 1.0, 2.0], rates=[1.0, 2.0], codes=[[9, 9], [0, 3], [-1, 2]])
    return [
        ("two_roots", dict(parent=[-1, 0, -1]), "family 0 has two roots (0 and 2)"),
        ("no_root", dict(parent=[1, 2, 0]), "family 0 has no root (parent -1)"),
        ("a_cycle", dict(parent=[-1, 2, 1]), "family 0: the parent array is not a tree (a cycle)"),
        ("parent_past_the_end", dict(parent=[-1, 0, 3]), "family 0: parent[2] = 3"),
        ("parent_below_minus_one", dict(parent=[-1, -2, 0]), "family 0: parent[1] = -2"),
        ("parent_equal_to_self", dict(parent=[-1, 1, 0]), "family 0: parent[1] = 1"),
        ("negative_length", dict(length=[0.0, 1.0, -0.5]), "family 0: length[2] = -0.5"),
        ("nan_length", dict(length=[0.0, np.nan, 1.0]), "family 0: length[1] = nan"),
        ("negative_rate", dict(rates=[1.0, -2.0]), "family 0: site rate 1 = -2"),
        ("leaf_code_equal_to_S", dict(codes=[[9, 9], [0, 3], [-1, 4]]),
         "family 0: state code 4 out of range [-1, S) at node 2 unit 1"),
        ("leaf_code_below_minus_one", dict(codes=[[9, 9], [-2, 3], [-1, 2]]),
         "family 0: state code -2 out of range [-1, S) at node 1 unit 0"),
        ("code_out_of_range_in_an_internal_row", dict(codes=[[-128, 127], [0, 3], [-1, 2]]), None),
    ], ok


REFUSALS, VALID = _refusals()


@pytest.mark.parametrize("name,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_keep_code_and_text(driver, tmp_path, name, change, text):
    a = dict(VALID, **change)
    rc, msg, got = _family(driver, tmp_path, a["parent"], a["length"], a["rates"], a["codes"])
    if text is None:
        assert (rc, msg) == (0, "")
        _check_family(got, expected(a["parent"], a["length"], a["rates"]))
    else:
        assert (rc, msg, got) == (CB_EINVAL, "em_layout: " + text, {})
