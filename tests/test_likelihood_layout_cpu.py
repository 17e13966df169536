"""The host side of the held-out likelihood without a GPU: csrc/tl_layout.h (argument checks, tree validation, levels, child
lists, bank slots, time tables, offsets) built into tests/tl_layout_driver.cpp with the host compiler under
AddressSanitizer + UBSan and run as a child process; every array against an independent NumPy restatement, every refusal
against the library's code and text."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CB_EINVAL, CB_EUNSUPPORTED = -1, -5
MODELS = [(20, 0, True, 1), (20, 0, True, 2), (20, 0, True, 3), (400, 20, True, 1), (400, 20, False, 1)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("tl_layout") / "tl_layout_driver")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "tl_layout_driver.cpp"), "-o", exe])
    return exe


# ---------------------------------------------------------------- cases
def _family(children, root, n_units, n_cats, S, S1, rng):
    """a family from {node: [children in visiting order]}: node labels scrambled, post-order by depth-first search"""
    nodes = sorted(set(children) | {c for cs in children.values() for c in cs})
    n = len(nodes)
    label = dict(zip(nodes, rng.permutation(n).tolist()))
    order, stack = [], [(root, False)]
    while stack:
        v, done = stack.pop()
        if done:
            order.append(label[v])
            continue
        stack.append((v, True))
        stack.extend((c, False) for c in reversed(children.get(v, [])))
    parent = np.full(n, -1)
    for v, cs in children.items():
        for c in cs:
            parent[label[c]] = label[v]
    alpha = S1 if S1 > 0 else S
    fam = dict(n=n, order=np.array(order), parent=parent, length=np.round(rng.uniform(0.0, 2.0, n), 3),
               n_units=n_units, cat_rate=np.round(np.sort(rng.uniform(0.1, 3.0, n_cats)), 3),
               unit_cat=rng.integers(0, n_cats, n_units), a=rng.integers(-1, alpha, (n, n_units)))
    fam["length"][label[root]] = 7.0   # (the root's length is no branch: the tables hold 0 for it)
    fam["b"] = rng.integers(-1, alpha, (n, n_units)) if S1 > 0 else None
    return fam


def _random_children(rng, n_leaves):
    """~n_leaves leaves joined 2 or 3 (at least once 3) at a time"""
    pool, children, k = list(range(n_leaves)), {}, n_leaves
    while len(pool) > 1:
        take = min(len(pool), 3 if k == n_leaves else int(rng.integers(2, 4)))
        kids = [pool.pop(int(i)) for i in sorted(rng.choice(len(pool), size=take, replace=False), reverse=True)]
        children[k] = kids
        pool.append(k)
        k += 1
    return children, pool[0]


def _families(S, S1, n_cats, which):
    rng = np.random.default_rng(1000 + S + n_cats)
    rand, rand_root = _random_children(rng, 30)
    assert max(len(c) for c in rand.values()) == 3
    shapes = {"one_node": ({}, 0, 3), "two_leaves": ({2: [0, 1]}, 2, 1),
              "caterpillar": ({5: [0, 1], 6: [5, 2], 7: [6, 3], 8: [7, 4]}, 8, 17), "random30": (rand, rand_root, 40)}
    fams = {}
    for name, (children, root, n_units) in shapes.items():
        if name == "one_node":
            children = {0: []}
        fams[name] = _family(children, root, n_units, n_cats, S, S1, rng)
    return list(fams.values()) if which == "batch" else [fams[which]]


def _arr(x, real=False):
    """an array of the case file; doubles as hexadecimal literals (exact; "nan" and "inf" as such)"""
    x = np.asarray(x).reshape(-1)
    return " ".join([str(x.size)] + [float(v).hex() if real else "%d" % v for v in x])


def _run(driver, tmp_path, S, S1, reversible, fams, n_fam=None, **override):
    cat = lambda k: np.concatenate([np.asarray(f[k]).reshape(-1) for f in fams])   # noqa: E731
    arrays = dict(n_nodes=_arr([f["n"] for f in fams]), postorder=_arr(cat("order")), parent=_arr(cat("parent")),
                  length=_arr(cat("length"), real=True), n_cats=_arr([len(f["cat_rate"]) for f in fams]),
                  cat_rate=_arr(cat("cat_rate"), real=True), n_units=_arr([f["n_units"] for f in fams]), unit_cat=_arr(cat("unit_cat")),
                  code_a=_arr(cat("a")), code_b=_arr(cat("b")) if S1 > 0 else "null",
                  ll=str(sum(f["n_units"] for f in fams)))
    arrays.update(override)
    path = tmp_path / "case.txt"
    path.write_text("%d %d %d %d\n" % (S, S1, reversible, len(fams) if n_fam is None else n_fam) + "\n".join(arrays.values()) + "\n")
    p = subprocess.run([driver, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert lines[0].startswith("rc ") and lines[1].startswith("msg")
    return int(lines[0][3:]), lines[1][4:], [ln.split() for ln in lines[2:]]


# ---------------------------------------------------------------- the layout, restated
def _expected(S, S1, reversible, fams):
    factored = S > 64 and reversible
    out = dict(factored=[int(factored)], family=[], level_ptr=[], level_nodes=[], child_ptr=[], child_idx=[], t_all=[], t_node=[],
               slot_all=[], off_n=[0], off_u=[0], off_c=[0], off_k=[0], off_t=[0])
    max_msg = max_bank = 0
    for f in fams:
        n, order, parent = f["n"], f["order"].tolist(), f["parent"]
        kids = {v: [c for c in order if parent[c] == v] for v in range(n)}          # children in post-order order
        height = {}
        for v in order:
            height[v] = 1 + max((height[c] for c in kids[v]), default=-1)
        root = order[-1]
        by_height = sorted(order, key=lambda v: height[v])                          # stable: post-order within a height
        n_levels = height[root] + 1
        t = np.where(np.arange(n) == root, 0.0, f["cat_rate"][:, None] * f["length"][None, :])   # [category][node]
        if factored:
            internal = [v for v in range(n) if kids[v] and v != root]
            out["slot_all"] += [internal.index(v) if v in internal else -1 for v in range(n)]
            out["t_node"] += t[0].tolist()
            bank = t[0][internal].tolist() if internal else [0.0]
        else:
            bank = t.reshape(-1).tolist()
        NU = -(-f["n_units"] // 32) * 32 if S > 64 else f["n_units"]
        out["family"].append([n, f["n_units"], len(f["cat_rate"]), root, n_levels, NU, len(bank)])
        out["level_ptr"].append(np.searchsorted([height[v] for v in by_height], np.arange(n_levels + 1)).tolist())
        out["level_nodes"] += by_height
        out["child_ptr"] += np.cumsum([0] + [len(kids[v]) for v in range(n)]).tolist()
        out["child_idx"] += [c for v in range(n) for c in kids[v]] + [0]            # (n - 1 children, one entry of padding)
        out["t_all"] += bank
        for key, step in (("off_n", n), ("off_u", f["n_units"]), ("off_c", n * f["n_units"]), ("off_k", len(f["cat_rate"])),
                          ("off_t", len(bank))):
            out[key].append(out[key][-1] + step)
        max_msg, max_bank = max(max_msg, n * S * NU), max(max_bank, len(bank))
    out["max_msg"], out["max_bank"] = [max_msg], [max_bank]
    return out


@pytest.mark.parametrize("which", ["one_node", "two_leaves", "caterpillar", "random30", "batch"])
@pytest.mark.parametrize("S,S1,reversible,n_cats", MODELS)
def test_layout_equals_the_numpy_restatement(driver, tmp_path, S, S1, reversible, n_cats, which):
    fams = _families(S, S1, n_cats, which)
    rc, msg, rows = _run(driver, tmp_path, S, S1, reversible, fams)
    assert (rc, msg) == (0, "")
    want = _expected(S, S1, reversible, fams)
    got = {}
    for row in rows:
        vals = [float.fromhex(x) for x in row[1:]] if row[0] in ("t_all", "t_node") else [int(x) for x in row[1:]]
        if row[0] in ("family", "level_ptr"):
            got.setdefault(row[0], []).append(vals)
        else:
            got[row[0]] = vals
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key   # (the time tables too: one product of two doubles, exact on both sides)
    if which in ("random30", "batch") and S > 64 and reversible:
        slots = [s for s in got["slot_all"][-fams[-1]["n"]:] if s >= 0]
        assert len(slots) > 3 and slots == list(range(len(slots)))   # ascending by node index


# ---------------------------------------------------------------- refusals: the library's codes and texts
def _chain():
    """0 <- 1 <- 2 (root 2), two units, two categories"""
    return dict(n=3, order=np.array([0, 1, 2]), parent=np.array([1, 2, -1]), length=np.array([0.5, 0.25, 0.0]), n_units=2,
                cat_rate=np.array([0.5, 2.0]), unit_cat=np.array([1, 0]), a=np.array([[3, -1], [0, 0], [0, 0]]), b=None)


def _with(**kw):
    f = _chain()
    f.update(kw)
    return f


PAIR = dict(cat_rate=np.array([1.0]), unit_cat=np.array([0, 0]), b=np.array([[0, 19], [0, 0], [0, 0]]))
REFUSALS = [
    ("no_family", 20, 0, [_chain()], dict(n_fam=0), CB_EINVAL, "cb_tree_likelihood: bad sizes (S = 20, families = 0)"),
    ("no_nodes", 20, 0, [_chain(), _with(n=0)], {}, CB_EINVAL, "cb_tree_likelihood: family 1 has bad sizes"),
    ("no_units", 20, 0, [_with(n_units=0)], {}, CB_EINVAL, "cb_tree_likelihood: family 0 has bad sizes"),
    ("no_categories", 20, 0, [_chain(), _chain(), _with(cat_rate=np.array([]))], {}, CB_EINVAL,
     "cb_tree_likelihood: family 2 has bad sizes"),
    ("postorder_too_large", 20, 0, [_with(order=np.array([0, 3, 2]))], {}, CB_EINVAL, "cb_tree_likelihood: postorder is not a permutation"),
    ("postorder_negative", 20, 0, [_with(order=np.array([-1, 1, 2]))], {}, CB_EINVAL, "cb_tree_likelihood: postorder is not a permutation"),
    ("postorder_repeats", 20, 0, [_with(order=np.array([0, 0, 2]))], {}, CB_EINVAL, "cb_tree_likelihood: postorder is not a permutation"),
    ("last_is_not_the_root", 20, 0, [_with(parent=np.array([1, 2, 0]))], {}, CB_EINVAL,
     "cb_tree_likelihood: the last node of postorder must be the root (parent -1)"),
    ("parent_before_child", 20, 0, [_with(order=np.array([1, 0, 2]))], {}, CB_EINVAL, "cb_tree_likelihood: node 1 precedes its child 0"),
    ("parent_out_of_range", 20, 0, [_with(parent=np.array([3, 2, -1]))], {}, CB_EINVAL, "cb_tree_likelihood: node 3 precedes its child 0"),
    ("length_negative", 20, 0, [_with(length=np.array([0.5, -0.25, 0.0]))], {}, CB_EINVAL, "cb_tree_likelihood: length[1] = -0.25"),
    ("length_nan", 20, 0, [_with(length=np.array([np.nan, 0.25, 0.0]))], {}, CB_EINVAL, "cb_tree_likelihood: length[0] = nan"),
    ("length_inf", 20, 0, [_with(length=np.array([np.inf, 0.25, 0.0]))], {}, CB_EINVAL, "cb_tree_likelihood: length[0] = inf"),
    ("unit_cat_too_large", 20, 0, [_with(unit_cat=np.array([1, 2]))], {}, CB_EINVAL, "cb_tree_likelihood: unit_cat[1] = 2"),
    ("unit_cat_negative", 20, 0, [_with(unit_cat=np.array([-1, 0]))], {}, CB_EINVAL, "cb_tree_likelihood: unit_cat[0] = -1"),
    ("cat_rate_negative", 20, 0, [_with(cat_rate=np.array([0.5, -2.0]))], {}, CB_EINVAL, "cb_tree_likelihood: cat_rate[1] = -2"),
    ("cat_rate_nan", 20, 0, [_with(cat_rate=np.array([np.nan, 2.0]))], {}, CB_EINVAL, "cb_tree_likelihood: cat_rate[0] = nan"),
    ("code_a_out_of_range", 20, 0, [_with(a=np.array([[3, 20], [0, 0], [0, 0]]))], {}, CB_EINVAL,
     "cb_tree_likelihood: state code out of range at node 0 unit 1"),
    ("code_a_out_of_range_pairs", 400, 20, [_with(**dict(PAIR, a=np.array([[20, 1], [0, 0], [0, 0]])))], {}, CB_EINVAL,
     "cb_tree_likelihood: state code out of range at node 0 unit 0"),
    ("code_b_out_of_range", 400, 20, [_with(**dict(PAIR, b=np.array([[0, 20], [0, 0], [0, 0]])))], {}, CB_EINVAL,
     "cb_tree_likelihood: state code out of range at node 0 unit 1"),
    ("two_categories_above_64_states", 400, 20, [_with(b=np.array([[0, 19], [0, 0], [0, 0]]))], {}, CB_EUNSUPPORTED,
     "cb_tree_likelihood: S > 64 takes one rate category (the reference evaluates pairs of sites at rate 1, "
     "_likelihood.py:214-230)"),
    ("null_argument", 20, 0, [_chain()], dict(parent="null"), CB_EINVAL, "cb_tree_likelihood: NULL argument"),
    ("null_results", 20, 0, [_chain()], dict(ll="null"), CB_EINVAL, "cb_tree_likelihood: NULL argument"),
    ("pairs_without_code_b", 400, 20, [_with(**PAIR)], dict(code_b="null"), CB_EINVAL,
     "cb_tree_likelihood: pair model needs S = S1 * S1 and code_b"),
]


@pytest.mark.parametrize("name,S,S1,fams,override,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_keep_code_and_text(driver, tmp_path, name, S, S1, fams, override, code, text):
    rc, msg, rows = _run(driver, tmp_path, S, S1, True, fams, **override)
    assert (rc, msg, rows) == (code, text, [])


def test_only_leaves_have_their_codes_checked(driver, tmp_path):
    """codes of internal nodes are never read by the kernels and never refused"""
    rc, msg, _ = _run(driver, tmp_path, 20, 0, True, [_with(a=np.array([[3, -1], [99, 0], [0, 120]]))])
    assert (rc, msg) == (0, "")
