"""tests/ble_reference.py (the vectorised restatement the GPU tests of the FastCherries kernels compare with) against the loop
oracle oracle/ble_oracle.py and the reference's own answers (tests/golden/ble.npz); the initial bins' rounding; the argument
checks of phylogeny_estimation/_ble.py that come before any device work; and the SENSITIVITY of the region-isolating inputs:
with a region's observations taken out -- what a kernel that skips the region sees -- every item built for that region changes
its answer.  No GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ble_reference as ref  # noqa: E402


def small_family(rng, n, L, S, gap=0.2):
    cx = rng.integers(0, S, (n, L))
    cy = np.where(rng.random((n, L)) < 0.6, cx, rng.integers(0, S, (n, L)))
    cx[rng.random((n, L)) < gap] = -1
    cy[rng.random((n, L)) < gap] = -1
    cx[0] = -1                                              # a cherry and a site nobody observes
    cy[:, L - 1] = -1
    return cx, cy


# ------------------------------------------------------------------------------------------------ restatement = oracle
@pytest.mark.parametrize("key,n,L", [("T17", 9, 23), ("S2", 7, 40), ("T2R2", 5, 12), ("T1", 4, 9), ("R1", 6, 11), ("R3", 11, 6)])
def test_restatement_equals_the_loop_oracle(key, n, L):
    from oracle import ble_oracle as bo
    logP, grid, rates = ref.bank(key)
    T, R, S, _ = logP.shape
    rng = np.random.default_rng(n * 100 + L)
    cx, cy = small_family(rng, n, L, S)
    s2r, li = rng.integers(0, R, L), rng.integers(0, T, n)
    pri = bo.rate_priors(rates)
    assert np.allclose(pri, ref.priors(rates), rtol=0, atol=0)
    got, margin = ref.branch_length_bisection(cx, cy, logP, s2r)
    assert got.dtype == np.int32 and np.array_equal(got, bo.get_branch_lengths(cx, cy, logP, s2r))
    assert got[0] == T - 1 and (margin[0] == np.inf or T == 1)
    assert np.all(margin > ref.UNDECIDED)
    got, margin = ref.site_rate_bisection(cx, cy, logP, li, pri)
    assert got.dtype == np.int32 and np.array_equal(got, bo.get_site_rates(cx, cy, logP, li, pri))
    assert np.all(margin > ref.UNDECIDED)
    seqs = np.concatenate([cx, cy, rng.integers(-1, S, (3, L))])
    w = ref.equal_weights(R)
    assert np.array_equal(ref.initial_bins(ref.site_totals(seqs, S), w), bo.initial_site_rates(seqs, w, S))
    for max_iters in (0, 1, 50):
        lengths, rate_index, iterations, smallest = ref.ascent(cx, cy, seqs, logP, rates, w, max_iters)
        want = bo.ble(cx, cy, seqs, logP, grid, rates, w, max_iters)
        assert smallest > ref.UNDECIDED and iterations <= max_iters
        assert np.array_equal(lengths, want[2]) and np.array_equal(rate_index, want[3])
        assert np.array_equal(grid[lengths], want[0]) and np.array_equal(rates[rate_index], want[1])


def test_gather_restatement_equals_the_loop_oracle():
    from oracle import ble_oracle as bo
    rng = np.random.default_rng(5)
    R, n, L, S = 4, 7, 11, 6
    tens = np.log(rng.dirichlet(np.full(S, 0.7), size=(R, n, S)))
    prior = rng.dirichlet(np.full(R, 3.0))
    tens[2], prior[2] = tens[0], prior[0]                   # rate 2 duplicates rate 0: the first of the two wins
    cx, cy = rng.integers(0, S, (n, L)), rng.integers(0, S, (n, L))
    labels = np.arange(R, dtype=np.float64)
    want = bo.compute_optimal_site_rates(cx, cy, tens, labels, prior)
    got, gap = ref.gather_argmax(cx, cy, tens, np.log(prior))
    assert np.array_equal(got, want.astype(np.int32)) and not np.any(got == 2) and np.any(got == 0)
    assert np.all(gap[got == 0] == 0.0) and np.all(gap[got != 0] > ref.UNDECIDED)
    got, gap = ref.gather_argmax(cx, cy, tens, np.log(prior), exact_ties=True)
    assert np.array_equal(got, want.astype(np.int32)) and np.all(gap > ref.UNDECIDED)
    assert ref.gather_argmax(cx, cy, tens[:1], np.log(prior[:1]))[1].min() == np.inf


def test_restatement_reproduces_the_reference_answers():
    """tests/golden/ble.npz: the answers typed into the reference's own tests, and three random families and the SiteRM gather
    through the compiled reference"""
    z = load_golden("ble.npz")
    bank = ref.log_bank(z["Q"], z["grid_bl"], z["rates_bl"])
    for k in range(3):
        got, _ = ref.branch_length_bisection(z[f"bl{k}_x"], z[f"bl{k}_y"], bank, z["s2r_bl"])
        assert list(got) == list(z[f"bl{k}_expected"]), k
    bank = ref.log_bank(z["Q"], z["grid_sr"], z["rates_sr"])
    for k in range(6):
        x = z[f"sr{k}_x"]
        got, _ = ref.site_rate_bisection(x, z[f"sr{k}_y"], bank, z["lengths_sr"][:len(x)], ref.priors(z["rates_sr"]))
        assert list(got) == list(z[f"sr{k}_expected"]), k
    for k in range(3):
        rates, grid = z[f"rnd{k}_rates"], z["grid_sr"]
        bank = ref.log_bank(z["Q"], grid, rates)
        cx, cy = z[f"rnd{k}_x"], z[f"rnd{k}_y"]
        got, margin = ref.branch_length_bisection(cx, cy, bank, z[f"rnd{k}_s2r"])
        assert np.all(margin > ref.UNDECIDED) and list(got) == list(z[f"rnd{k}_bl"])
        got, margin = ref.site_rate_bisection(cx, cy, bank, z[f"rnd{k}_li"], ref.priors(rates))
        assert np.all(margin > ref.UNDECIDED) and list(got) == list(z[f"rnd{k}_sr"])
        lengths, rate_index, _, smallest = ref.ascent(cx, cy, np.concatenate([cx, cy]), bank, rates, z[f"rnd{k}_weights"], 50)
        assert smallest > ref.UNDECIDED
        assert np.array_equal(grid[lengths], z[f"rnd{k}_ble_lengths"]) and np.array_equal(rates[rate_index], z[f"rnd{k}_ble_rates"])
    got, gap = ref.gather_argmax(z["gather_x"], z["gather_y"], z["gather_tensor"], np.log(z["gather_prior"]))
    assert np.all(gap > ref.UNDECIDED) and np.array_equal(z["gather_grid"][got], z["gather_expected"])


def test_site_totals_count_the_differing_pairs():
    rng = np.random.default_rng(3)
    seqs = rng.integers(-1, 5, (13, 37))
    want = [sum(1 for i in range(13) for k in range(i + 1, 13) if seqs[i, j] >= 0 and seqs[k, j] >= 0 and seqs[i, j] != seqs[k, j])
            for j in range(37)]
    got = ref.site_totals(seqs, 5)
    assert got.dtype == np.int64 and list(got) == [2 * v for v in want]      # (the reference's sum counts every pair twice)


# ------------------------------------------------------------------------------------------------ rounding
def staircase(L, order):
    """2 L sequences whose site order[i] has i * (2 L - i) differing pairs (i of the sequences hold another state): the sites in
    the order of their totals are `order`"""
    seqs = np.zeros((2 * L, L), dtype=np.int64)
    for i, j in enumerate(order):
        seqs[:i, j] = 1
    return seqs


def test_initial_bins_round_halves_away_from_zero():
    """branch_length_estimation.cpp:50 is (int)std::round.  L = 6, weights 0.25, 0.75, 1: the cuts are round(1.5) = 2,
    round(4.5) = 5 and 6, so the sites of ranks 0, 1 get category 0, ranks 2, 3, 4 category 1 and rank 5 category 2 (halves to
    even: cuts 2, 4, 6).  L = 10, weights 0.25, 0.6, 1: round(2.5) = 3, then 6, 10: ranks 0-2, 3-5, 6-9."""
    from oracle import ble_oracle as bo
    order = [4, 0, 5, 2, 1, 3]
    want = np.zeros(6, dtype=int)
    want[[5, 2, 1]], want[3] = 1, 2
    got = bo.initial_site_rates(staircase(6, order), [0.25, 0.75, 1.0], 2)
    assert list(got) == list(want) == [0, 1, 1, 2, 0, 1]
    assert list(ref.initial_bins(ref.site_totals(staircase(6, order), 2), [0.25, 0.75, 1.0])) == list(want)
    order = [7, 2, 9, 0, 4, 1, 8, 3, 6, 5]
    want = np.zeros(10, dtype=int)
    want[[0, 4, 1]], want[[8, 3, 6, 5]] = 1, 2
    got = bo.initial_site_rates(staircase(10, order), [0.25, 0.6, 1.0], 2)
    assert list(got) == list(want) == [1, 1, 0, 2, 1, 2, 2, 0, 2, 0]
    assert list(ref.initial_bins(ref.site_totals(staircase(10, order), 2), [0.25, 0.6, 1.0])) == list(want)


# ------------------------------------------------------------------------------------------------ argument checks
def test_wrong_lengths_raise_before_the_library_loads(monkeypatch):
    from cherryml_amd import _lib
    from cherryml_amd.phylogeny_estimation import branch_lengths, site_rates

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    bank = np.zeros((4, 2, 3, 3))
    cx = np.zeros((2, 5), dtype=np.int8)
    for s2r in (np.zeros(4), np.zeros(6), np.zeros((1, 5)), np.zeros((5, 1)), 0):
        with pytest.raises(ValueError):
            branch_lengths(cx, cx, bank, s2r)
    for li in (np.zeros(1), np.zeros(3), np.zeros((1, 2)), np.zeros((2, 1)), 0):
        with pytest.raises(ValueError):
            site_rates(cx, cx, bank, li, np.zeros(2))
    for pri in (np.zeros(1), np.zeros(3), np.zeros((1, 2))):
        with pytest.raises(ValueError):
            site_rates(cx, cx, bank, np.zeros(2), pri)
    with pytest.raises(AssertionError):                     # right lengths: the call goes on to the library
        branch_lengths(cx, cx, bank, np.zeros(5))
    with pytest.raises(AssertionError):
        site_rates(cx, cx, bank, np.zeros(2), np.zeros(2))


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("which", ["branch_lengths", "site_rates<1>", "site_rates<4>"])
def test_every_region_decides_the_items_built_for_it(which):
    """The standing form of a mutation check of the kernels: the restatement on the family WITHOUT a region's observations (what
    a kernel that skips that part of its loop sums) gives another answer for every item built for that region -- the no-data
    default -- and the same answer for the items that have nothing in the region."""
    logP, _, rates = ref.bank("lg4")
    cx, cy, arg, regions, want, margin = ref.region_case(which)
    if which == "branch_lengths":
        def run(x, y):
            return ref.branch_length_bisection(x, y, logP, arg)[0]
        default = logP.shape[0] - 1
        assert cx.shape == (8, 600)
    else:
        def run(x, y):
            return ref.site_rate_bisection(x, y, logP, arg, ref.priors(rates))[0]
        default = run(np.full((cx.shape[0], 1), -1), np.full((cx.shape[0], 1), -1))[0]
        assert cx.shape == ((600, 2050) if which == "site_rates<1>" else (2050, 8))
    assert np.all(margin > ref.UNDECIDED)
    seen = (cx >= 0) & (cy >= 0)
    for name, items, keep in regions:
        pick = (lambda a: a[items]) if which == "branch_lengths" else (lambda a: a[:, items])
        assert pick(seen).any(axis=1 if which == "branch_lengths" else 0).all(), name      # every item is observed,
        assert not pick(seen & keep).any(), name                                           # and only inside the region
        blanked = run(*ref.blank(cx, cy, keep))
        print(f"{which}, {name}: {len(items)} items, smallest margin {margin[items].min():.2e}, answers {np.unique(want[items])}, "
              f"without the region {np.unique(blanked[items])}")
        assert np.all(margin[items] > 1e-6), name
        assert np.all(blanked[items] == default) and np.all(want[items] != default), name
        outside = ~(seen & ~keep).any(axis=1 if which == "branch_lengths" else 0)             # (nothing observed in the region)
        assert outside.any() and not outside[items].any(), name
        assert np.array_equal(blanked[outside], want[outside]), name


# ------------------------------------------------------------------------------------------------ coverage
def test_the_gpu_shapes_reach_every_form_under_the_constants_of_the_source():
    """The table in tests/test_gpu_ble_forms.py holds for BLE_HOIST = 8, BLE_SR_HOIST = 8 and the launch rule `L < 2048`.  Both
    forms of ble_site_rates_kernel compute the same answers, so no comparison of results notices a moved threshold or group
    size: the shapes would silently stop reaching the forms they are there for.  This reads the three numbers from
    csrc/ble.hip.h and checks, from them, that the shapes of the GPU module still reach every form."""
    import re
    import test_gpu_ble_forms as forms
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cherryml_amd", "csrc", "ble.hip.h")).read()
    hoist = 64 * int(re.search(r"constexpr int BLE_HOIST = (\d+);", src).group(1))
    group = 64 * int(re.search(r"constexpr int BLE_SR_HOIST = (\d+);", src).group(1))
    launch = src[src.index("static inline void ble_launch_site_rates"):]
    rule = re.search(r"if \(L < (\d+)\)\s*hipLaunchKernelGGL\(ble_site_rates_kernel<4>.*?else\s*hipLaunchKernelGGL\(ble_site_rates_kernel<1>",
                     launch, re.S)
    assert rule is not None
    threshold = int(rule.group(1))
    assert (hoist, group, threshold) == (512, 512, 2048)

    def waves(n, L):
        """[(cherries in hoisted groups, cherries in the tail)] per wave of a site"""
        if L >= threshold:
            return [(n // group * group, n % group)]
        per = ((n + 3) // 4 + 63) // 64 * 64
        size = [max(0, min(n, (w + 1) * per) - min(n, w * per)) for w in range(4)]
        return [(s // group * group, s % group) for s in size]

    L_of = [L for _, L in forms.BL_SHAPES]
    assert any(L < hoist for L in L_of) and hoist in L_of and hoist + 1 in L_of and any(L > 2 * hoist for L in L_of)
    assert {n % 4 for n, _ in forms.BL_SHAPES} == {0, 1, 2, 3}
    assert all(L < threshold for _, L in forms.SR4_SHAPES) and all(L >= threshold for _, L in forms.SR1_SHAPES)
    assert threshold in [L for _, L in forms.SR1_SHAPES]
    four = {s: waves(*s) for s in forms.SR4_SHAPES}
    assert all(h == 0 for h, _ in four[(257, 3)]) and [t for _, t in four[(257, 3)]] == [128, 128, 1, 0]
    assert four[(1793, 3)] == [(512, 0)] * 3 + [(0, 257)] and all(h == 0 for h, _ in waves(1792, 3))   # the smallest such n
    assert four[(1985, 3)] == [(512, 0)] * 3 + [(0, 449)]
    assert four[(2050, 8)] == [(512, 64)] * 3 + [(0, 322)]
    one = {s: waves(*s)[0] for s in forms.SR1_SHAPES}
    assert one[(70, 2049)] == (0, 70) and one[(512, 2048)] == (512, 0) and one[(600, 2050)] == (512, 88)
    assert one[(1100, 2051)] == (1024, 76)
    # the region-isolating families: 600 sites past the hoisted 512; 600 cherries in form <1>; 2050 cherries (per = 576) in <4>
    assert ref.region_case("branch_lengths")[0].shape[1] > hoist
    assert waves(*ref.region_case("site_rates<1>")[0].shape) == [(512, 88)]
    assert waves(*ref.region_case("site_rates<4>")[0].shape) == [(512, 64)] * 3 + [(0, 322)]
