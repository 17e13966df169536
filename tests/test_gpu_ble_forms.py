"""The FastCherries kernels of csrc/ble.hip.h at every form they take, against the NumPy restatement tests/ble_reference.py.

Which form a shape (n cherries, L sites) reaches -- to be checked against `BLE_HOIST = 8` (512 sites) in
ble_branch_lengths_kernel, `BLE_SR_HOIST = 8` (groups of 512 cherries) in ble_site_rates_kernel and the rule `L < 2048` of
ble_launch_site_rates (`per` = a wave's quarter in form <4>, roundup64(ceil(n / 4))):

  kernel                       shape (n, L)                       form   hoisted part              tail
  ble_branch_lengths_kernel    (1,1) (5,64) (6,65) (3,512)        -      sites < 512 (all)         none
                               (7,513) (9,700) (4,1100) (8,600)   -      sites < 512               sites >= 512
  ble_site_rates_kernel        (1,1) (63,5) (64,5) (65,7)         <4>    none (per = 64)           all cherries
                               (257,3)                            <4>    none (per = 128)          all; wave 2 one cherry, wave 3 none
                               (1793,3) (1985,3)                  <4>    waves 0-2 (per = 512)     wave 3: 257 / 449 cherries
                                 (1793 is the smallest n with per = 512: ceil(n / 4) > 448; at 1792 per = 448, no hoisted group)
                               (2050,8)                           <4>    waves 0-2 (per = 576)     64 cherries in waves 0-2, wave 3: 322
                               (3,2048) (70,2049)                 <1>    none                      all cherries
                               (512,2048)                         <1>    one group                 none
                               (600,2050)                         <1>    one group                 88 cherries
                               (1100,2051)                        <1>    two groups                76 cherries
  site_rate_gather_kernel      (9,14) (64,5)                      -      one step of the lane loop
                               (65,6) (200,7)                     -      two / four steps
  ble_transpose_check_kernel,  every `BleBank.estimate` below: (37,91) (5,600) (5,6) one tile row, (70,2049) (130,2049)
  ble_site_totals_kernel       (2050,40) many tiles, ragged in both directions; S = 20

Exactness, as in tests/test_gpu_nj.py.  Every check is on integers.  The restatement records per item the smallest
|a - b| / max(|a|, |b|) met on the way; an item is UNDECIDED when that is <= 1e-9 (summation order moves the sums by ~1e-13
relative) and is left out; a test fails when more than 1 % of its items are undecided, and a whole ascent must have no undecided
step.  With the fixed seeds below, on the CPU: no item of any group is undecided, and the smallest margins are
  branch lengths, the seven shapes                        9.5e-05
  site rates, form <4> / form <1> / twenty categories     4.6e-03 / 2.6e-06 / 4.6e-07
  small T and R, S = 2 and 127                            1.8e-05
  region-isolating inputs, the items built for a region   4.9e-05
  tie banks, the steps that are no tie                    1.1e-04
  gather, the best total against the second best          1.1e-03
  ascents: (37,91) 6.1e-06 in 8 iterations, (70,2049) 4.2e-07 in 11, (2050,40) 1.3e-07 in 2, (5,600) 7.8e-06 in 4 (R = 4) and
  1.4e-05 in 5 (R = 8); stopped after 0 or 1 iterations 8.9e-06; the six-site family of the rounding test 3.4e-03;
  the small batch (3,5) (4,33) (65,64) (7,513): 1, 2, 7 and 5 iterations, 8.6e-07 (cut off after 4: 1, 2, 4, 4)
Needs an MI355X."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ble_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

UNDECIDED = ref.UNDECIDED
BL_SHAPES = [(1, 1), (5, 64), (6, 65), (3, 512), (7, 513), (4, 1100), (9, 700)]
SR4_SHAPES = [(1, 1), (63, 5), (64, 5), (65, 7), (257, 3), (1793, 3), (1985, 3), (2050, 8)]
SR1_SHAPES = [(3, 2048), (70, 2049), (512, 2048), (600, 2050), (1100, 2051)]
SMALL = [("T1", (6, 65)), ("R1", (6, 65)), ("T2R2", (6, 65)), ("T2R2", (70, 2049)), ("T17", (6, 65)),
         ("S2", (6, 65)), ("S2", (70, 2049)), ("S127", (6, 65)), ("S127", (70, 2049))]
GATHER_SHAPES = [(9, 14), (64, 5), (65, 6), (200, 7)]
ASCENTS = [("lg4", (37, 91)), ("lg4", (70, 2049)), ("lg4", (2050, 40)), ("lg4", (5, 600)), ("lg8", (5, 600))]


def ids(s):
    return f"{s[0]}x{s[1]}"


# ------------------------------------------------------------------------------------------------ banks
bank, priors = ref.bank, ref.priors


@pytest.fixture(scope="module")
def banks():
    return bank


# ------------------------------------------------------------------------------------------------ cases (no GPU)
@lru_cache(maxsize=None)
def bl_case(key, shape, exact_ties=False):
    logP = bank(key)[0]
    cx, cy, _, r = ref.family(logP, *shape, seed=10_000 * shape[0] + shape[1])
    want, margin = ref.branch_length_bisection(cx, cy, logP, r, exact_ties)
    return cx, cy, r, want, margin


@lru_cache(maxsize=None)
def sr_case(key, shape, exact_ties=False):
    logP, _, rates = bank(key)
    cx, cy, t, _ = ref.family(logP, *shape, seed=10_000 * shape[0] + shape[1] + 1, t_from=0.5)
    want, margin = ref.site_rate_bisection(cx, cy, logP, t, priors(rates), exact_ties)
    return cx, cy, t.astype(np.int32), want, margin


@lru_cache(maxsize=None)
def gather_case(shape, duplicate=False):
    n, L = shape
    R, S = 5, 21
    rng = np.random.default_rng(100 * n + L)
    prior = rng.dirichlet(np.full(R, 3.0))
    tens = np.log(rng.dirichlet(np.full(S, 0.7), size=(R, n, S)))
    if duplicate:                                          # rates 1 and 3 are duplicates of each other, and so are their priors
        tens[3] = tens[1]
        prior[3] = prior[1]
    cx, cy = rng.integers(0, S, size=(n, L)), rng.integers(0, S, size=(n, L))
    want, gap = ref.gather_argmax(cx, cy, tens, np.log(prior), exact_ties=duplicate)
    return cx, cy, tens, prior, want, gap


@lru_cache(maxsize=None)
def ascent_case(key, shape, max_iters=50, weights=None):
    logP, grid, rates = bank(key)
    cx, cy, _, _ = ref.family(logP, *shape, seed=10_000 * shape[0] + shape[1] + 2)
    seqs = np.concatenate([cx, cy])
    w = ref.equal_weights(len(rates)) if weights is None else np.array(weights)
    lengths, rate_index, iterations, margin = ref.ascent(cx, cy, seqs, logP, rates, w, max_iters)
    return cx, cy, seqs, w, lengths, rate_index, iterations, margin


region_case = ref.region_case


def compare(got, want, margin, what):
    decided = margin > UNDECIDED
    print(f"{what}: {len(want)} items, smallest margin {margin.min():.2e}, undecided {int((~decided).sum())}, mismatches on "
          f"decided items {int((got != want)[decided].sum())}")
    assert got.dtype == np.int32 and got.shape == want.shape
    assert (~decided).sum() <= 0.01 * len(want)
    assert np.array_equal(got[decided], want[decided])


def check_specials(got_lengths, cx, cy, T):
    """the all-gap cherry ends at T - 1 (`0 > 0` is false at every step), the cherry with y == x at the grid's first point"""
    n = cx.shape[0]
    if n >= 4:
        assert np.all(cx[n - 1] == -1) and got_lengths[n - 1] == T - 1
        assert np.array_equal(cx[1], cy[1]) and np.any(cx[1] >= 0) and got_lengths[1] == 0


# ------------------------------------------------------------------------------------------------ 1. branch lengths
@pytest.mark.parametrize("shape", BL_SHAPES, ids=ids)
def test_branch_lengths_equal_the_restatement(banks, shape):
    from cherryml_amd.phylogeny_estimation import branch_lengths
    logP = banks("lg4")[0]
    cx, cy, r, want, margin = bl_case("lg4", shape)
    got = branch_lengths(cx, cy, logP, r)
    compare(got, want, margin, f"branch lengths {shape}")
    check_specials(got, cx, cy, logP.shape[0])


def test_pairwise_kernel_agrees_with_branch_lengths_past_512_sites(banks):
    from cherryml_amd.phylogeny_estimation import branch_lengths, pairwise_branch_lengths
    logP = banks("lg4")[0]
    cx, _, r, _, _ = bl_case("lg4", (9, 700))
    seqs = cx[:8]
    I, J = np.triu_indices(len(seqs), 1)
    pair = pairwise_branch_lengths(seqs, logP, r)
    want, margin = ref.branch_length_bisection(seqs[I], seqs[J], logP, r)
    cherry = branch_lengths(seqs[I], seqs[J], logP, r)
    compare(cherry, want, margin, "materialised pairs of (9, 700)")
    assert np.array_equal(pair[I, J], cherry) and np.array_equal(pair[J, I], cherry)


def test_branch_lengths_region_by_region(banks):
    """a cherry observed only in the plain-loop tail (sites >= 512), only in the hoisted part, only at the last site, only at
    the first: each gets the no-data default T - 1 from a kernel that skips its region (tests/test_ble_cpu.py shows that)"""
    from cherryml_amd.phylogeny_estimation import branch_lengths
    logP = banks("lg4")[0]
    cx, cy, r, regions, want, margin = region_case("branch_lengths")
    got = branch_lengths(cx, cy, logP, r)
    compare(got, want, margin, "branch lengths by region (8, 600)")
    for name, items, _ in regions:
        assert np.all(margin[items] > UNDECIDED) and np.all(want[items] != logP.shape[0] - 1), name
        assert np.array_equal(got[items], want[items]), name


# ------------------------------------------------------------------------------------------------ 2. site rates
def check_spread(want, R, shape):
    share = np.bincount(want, minlength=R) / len(want)
    print(f"site rates {shape}: share of each category {np.round(share, 3)}")
    if R <= 4 and shape[1] >= 100:                          # (a family of three to eight sites cannot fill four categories,
        assert share.min() > 0.0                            # and three cherries seldom outweigh the prior of the fastest one)
        assert share.min() >= 0.05 or shape[0] < 64


@pytest.mark.parametrize("shape", SR4_SHAPES + SR1_SHAPES, ids=ids)
def test_site_rates_equal_the_restatement(banks, shape):
    from cherryml_amd.phylogeny_estimation import site_rates
    logP, _, rates = banks("lg4")
    cx, cy, t, want, margin = sr_case("lg4", shape)
    got = site_rates(cx, cy, logP, t, priors(rates))
    compare(got, want, margin, f"site rates {shape}")
    check_spread(want, len(rates), shape)


def test_site_rates_with_twenty_categories(banks):
    from cherryml_amd.phylogeny_estimation import site_rates
    logP, _, rates = banks("lg20")
    for shape in ((65, 7), (600, 2050)):
        cx, cy, t, want, margin = sr_case("lg20", shape)
        compare(site_rates(cx, cy, logP, t, priors(rates)), want, margin, f"site rates, R = 20, {shape}")
        assert len(np.unique(want)) >= min(shape[1] - 1, 5)


def test_the_two_forms_leave_nothing_behind(banks):
    """form <4>, then <1>, then <4> again (its LDS partial sums, the launch rule): each call as if it were the only one"""
    from cherryml_amd.phylogeny_estimation import site_rates
    logP, _, rates = banks("lg4")
    for shape in ((2050, 8), (600, 2050), (257, 3), (512, 2048), (2050, 8)):
        cx, cy, t, want, margin = sr_case("lg4", shape)
        compare(site_rates(cx, cy, logP, t, priors(rates)), want, margin, f"site rates {shape}")


@pytest.mark.parametrize("which", ["site_rates<1>", "site_rates<4>"])
def test_site_rates_region_by_region(banks, which):
    """sites observed only in the cherries of one part of the kernel's loop: the tail after the hoisted groups, the hoisted
    groups, one wave's quarter.  A kernel that skips the part gives them the prior's own answer (tests/test_ble_cpu.py)."""
    from cherryml_amd.phylogeny_estimation import site_rates
    logP, _, rates = banks("lg4")
    cx, cy, t, regions, want, margin = region_case(which)
    assert (cx.shape[1] >= 2048) == (which == "site_rates<1>")
    got = site_rates(cx, cy, logP, t, priors(rates))
    compare(got, want, margin, f"{which} by region {cx.shape}")
    default = ref.site_rate_bisection(cx[:, :1] * 0 - 1, cx[:, :1] * 0 - 1, logP, t, priors(rates))[0][0]
    for name, items, _ in regions:
        assert np.all(margin[items] > UNDECIDED) and np.all(want[items] != default), name
        assert np.array_equal(got[items], want[items]), name


# ------------------------------------------------------------------------------------------------ 3. small T, R; other S
@pytest.mark.parametrize("key,shape", SMALL, ids=lambda v: v if isinstance(v, str) else ids(v))
def test_small_banks_and_other_alphabets(banks, key, shape):
    from cherryml_amd.phylogeny_estimation import branch_lengths, site_rates
    logP, _, rates = banks(key)
    T, R, S, _ = logP.shape
    cx, cy, r, want, margin = bl_case(key, shape)
    if key == "S127":
        assert cx.max() == 126 and cy.max() == 126           # the largest code an int8 sequence can hold
    got = branch_lengths(cx, cy, logP, r)
    compare(got, want, margin, f"branch lengths, bank {key}, {shape}")
    check_specials(got, cx, cy, T)
    if T == 1:
        assert np.all(got == 0)
    cx, cy, t, want, margin = sr_case(key, shape)
    got = site_rates(cx, cy, logP, t, priors(rates))
    compare(got, want, margin, f"site rates, bank {key}, {shape}")
    if R == 1:
        assert np.all(got == 0)
    elif T > 1 and shape[1] >= 100:
        check_spread(want, R, shape)


# ------------------------------------------------------------------------------------------------ 4. exact ties
def test_equal_grid_points_move_the_bisection_up(banks):
    """grid points 2k + 1 and 2k + 2 hold the same matrix: both sides of such a step are the same addends in the same order, `a > b`
    is false and the bisection moves up.  No margin is needed for those steps; the other steps keep theirs."""
    from cherryml_amd.phylogeny_estimation import branch_lengths
    logP = banks("tie_t")[0]
    for shape in ((6, 65), (7, 513)):
        cx, cy, r, want, margin = bl_case("tie_t", shape, True)
        tied = bl_case("tie_t", shape)[4] == 0.0
        assert tied.mean() >= 0.25 and np.all(margin > UNDECIDED)
        got = branch_lengths(cx, cy, logP, r)
        assert np.array_equal(got, want), shape


def test_equal_rates_move_the_bisection_up(banks):
    from cherryml_amd.phylogeny_estimation import site_rates
    logP, _, rates = banks("tie_r")
    assert np.array_equal(logP[:, 2], logP[:, 3]) and priors(rates)[2] == priors(rates)[3]
    for shape in ((65, 7), (257, 33), (70, 2049), (600, 2050)):
        cx, cy, t, want, margin = sr_case("tie_r", shape, True)
        tied = sr_case("tie_r", shape)[4] == 0.0
        assert tied.any() and np.all(margin > UNDECIDED)
        assert not np.any(want == 2) and len(np.unique(want)) >= 2     # (2 against 3 is a tie: never the lower one)
        got = site_rates(cx, cy, logP, t, priors(rates))
        assert np.array_equal(got, want), shape


# ------------------------------------------------------------------------------------------------ 5. the SiteRM gather
def run_gather(case):
    from cherryml_amd._siterm import compute_optimal_site_rates
    cx, cy, tens, prior, want, gap = case
    cherries = [(list(map(int, cx[c])), list(map(int, cy[c])), 0.1) for c in range(cx.shape[0])]
    labels = [float(r) for r in range(tens.shape[0])]       # the grid only labels the answer: the label is the index
    got = np.array(compute_optimal_site_rates(cx.shape[1], cherries, tens, labels, list(prior)))
    return got.astype(np.int32)


@pytest.mark.parametrize("shape", GATHER_SHAPES, ids=ids)
def test_gather_equals_the_restatement(shape):
    case = gather_case(shape)
    got = run_gather(case)
    compare(got, case[4], case[5], f"gather {shape}")
    assert len(np.unique(case[4])) >= 2


def test_gather_returns_the_first_of_two_equal_maxima():
    case = gather_case((200, 7), True)
    assert np.any(case[4] == 1)
    got = run_gather(case)
    assert not np.any(got == 3)                              # the later duplicate
    compare(got, case[4], case[5], "gather with duplicated rates (200, 7)")
    case = gather_case((65, 6), True)
    got = run_gather(case)
    assert not np.any(got == 3)
    compare(got, case[4], case[5], "gather with duplicated rates (65, 6)")


# ------------------------------------------------------------------------------------------------ 6. ascents
def check_ascent(result, prof, case, grid, rates, what):
    _, _, _, _, lengths, rate_index, iterations, margin = case
    print(f"ascent {what}: {iterations} iterations, smallest margin {margin:.2e}")
    assert margin > UNDECIDED                                # one undecided step could change everything after it
    assert np.array_equal(result[0], grid[lengths]) and np.array_equal(result[1], rates[rate_index]), what
    assert prof["iterations"] == iterations, what


@pytest.mark.parametrize("key,shape", ASCENTS, ids=lambda v: v if isinstance(v, str) else ids(v))
def test_ascent_per_call_equals_the_restatement(banks, key, shape):
    from cherryml_amd.phylogeny_estimation import estimate_branch_lengths_and_site_rates
    logP, grid, rates = banks(key)
    case = ascent_case(key, shape)
    cx, cy, seqs, w = case[:4]
    prof = {}
    got = estimate_branch_lengths_and_site_rates(cx, cy, seqs, logP, grid, rates, w, 50, profile=prof)
    check_ascent(got, prof, case, grid, rates, f"per call {key} {shape}")


def test_ascent_through_one_resident_bank(banks):
    """the largest family first, then a small one in its workspace, then one with more cherries (the workspace grows)"""
    from cherryml_amd.phylogeny_estimation import BleBank
    for key, shapes in (("lg4", ((70, 2049), (37, 91), (2050, 40), (5, 600))), ("lg8", ((5, 600),))):
        logP, grid, rates = banks(key)
        with BleBank(logP, grid, rates) as resident:
            for shape in shapes:
                case = ascent_case(key, shape)
                cx, cy, seqs, w = case[:4]
                prof = {}
                got = resident.estimate(cx, cy, seqs, w, 50, profile=prof)
                check_ascent(got, prof, case, grid, rates, f"resident {key} {shape}")


def test_ascent_of_four_families_in_one_batch(banks):
    """forms <1> (2049 sites) and <4> side by side in one cb_ble_batch"""
    from cherryml_amd.phylogeny_estimation import estimate_branch_lengths_and_site_rates_batch
    logP, grid, rates = banks("lg4")
    shapes = [(37, 91), (70, 2049), (2050, 40), (5, 600)]
    cases = [ascent_case("lg4", s) for s in shapes]
    prof = {}
    got = estimate_branch_lengths_and_site_rates_batch([c[:3] for c in cases], logP, grid, rates, cases[0][3], 50, profile=prof)
    assert len(got) == 4
    for k, (shape, case) in enumerate(zip(shapes, cases)):
        check_ascent(got[k], {"iterations": prof["iterations"][k]}, case, grid, rates, f"batch {shape}")


@pytest.mark.parametrize("max_iters", [0, 1])
def test_ascent_stopped_early(banks, max_iters):
    """0: the lengths under the initial bins (and the bins themselves: the totals kernel of the resident entry); 1: one round"""
    from cherryml_amd.phylogeny_estimation import BleBank, estimate_branch_lengths_and_site_rates
    logP, grid, rates = banks("lg4")
    for shape in ((37, 91), (70, 2049)):
        case = ascent_case("lg4", shape, max_iters)
        cx, cy, seqs, w = case[:4]
        assert case[6] == max_iters
        if max_iters == 0:
            assert np.array_equal(case[5], ref.initial_bins(ref.site_totals(seqs, 20), w))
        prof = {}
        got = estimate_branch_lengths_and_site_rates(cx, cy, seqs, logP, grid, rates, w, max_iters, profile=prof)
        check_ascent(got, prof, case, grid, rates, f"per call, max_iters = {max_iters}, {shape}")
        with BleBank(logP, grid, rates) as resident:
            got = resident.estimate(cx, cy, seqs, w, max_iters, profile=prof)
        check_ascent(got, prof, case, grid, rates, f"resident, max_iters = {max_iters}, {shape}")


def test_initial_bins_round_halves_away_from_zero(banks):
    """L = 6, weights 0.25, 0.75, 1: the cuts are round(1.5) = 2 and round(4.5) = 5 (std::round; llround in the library), so the
    bins hold 2, 3 and 1 sites; halves to even would give 2, 2, 2"""
    from cherryml_amd.phylogeny_estimation import BleBank, estimate_branch_lengths_and_site_rates
    logP, grid, rates = banks("R3")
    weights = (0.25, 0.75, 1.0)
    for max_iters in (0, 50):
        case = ascent_case("R3", (5, 6), max_iters, weights)
        cx, cy, seqs, w = case[:4]
        if max_iters == 0:
            assert list(np.bincount(case[5], minlength=3)) == [2, 3, 1]
        prof = {}
        got = estimate_branch_lengths_and_site_rates(cx, cy, seqs, logP, grid, rates, w, max_iters, profile=prof)
        check_ascent(got, prof, case, grid, rates, f"per call, halves, max_iters = {max_iters}")
        with BleBank(logP, grid, rates) as resident:
            got = resident.estimate(cx, cy, seqs, w, max_iters, profile=prof)
        check_ascent(got, prof, case, grid, rates, f"resident, halves, max_iters = {max_iters}")


# ------------------------------------------------------------------------------------------------ 7. the range check
def test_resident_entry_finds_a_bad_code_in_the_last_tile(banks):
    """one code >= S in the last row and column of a (130, 2049) family (3 x 33 tiles of the transposing kernel, the last ones
    ragged) must raise, and the next family through the same bank must be right"""
    from cherryml_amd.phylogeny_estimation import BleBank
    logP, grid, rates = banks("lg4")
    cx, cy, _, _ = ref.family(logP, 130, 2049, seed=130)
    seqs = np.concatenate([cx, cy])
    w = ref.equal_weights(4)
    with BleBank(logP, grid, rates) as resident:
        for which in (0, 1):
            bad = [cx.copy(), cy.copy()]
            bad[which][129, 2048] = 20
            with pytest.raises(ValueError):
                resident.estimate(bad[0], bad[1], seqs, w, 1)
        case = ascent_case("lg4", (37, 91))
        prof = {}
        got = resident.estimate(*case[:4], 50, profile=prof)
        check_ascent(got, prof, case, grid, rates, "after the refused family")


# ------------------------------------------------------------------------------------------------ 8. one ascent behind three entries
@pytest.mark.parametrize("max_iters", [0, 1, 50])
def test_the_three_entries_agree_on_one_family(banks, max_iters):
    """cb_ble, the resident entry and a batch of one run the same loop: the same lengths, rates and iteration count"""
    from cherryml_amd.phylogeny_estimation import (BleBank, estimate_branch_lengths_and_site_rates,
                                                   estimate_branch_lengths_and_site_rates_batch)
    logP, grid, rates = banks("lg4")
    with BleBank(logP, grid, rates) as resident:
        for shape in ((37, 91), (70, 2049)):
            case = ascent_case("lg4", shape, max_iters)
            cx, cy, seqs, w = case[:4]
            per_call, one, batch = {}, {}, {}
            a = estimate_branch_lengths_and_site_rates(cx, cy, seqs, logP, grid, rates, w, max_iters, profile=per_call)
            b = resident.estimate(cx, cy, seqs, w, max_iters, profile=one)
            c = estimate_branch_lengths_and_site_rates_batch([(cx, cy, seqs)], logP, grid, rates, w, max_iters, profile=batch)
            assert len(c) == 1 and batch["iterations"] == [per_call["iterations"]] and one["iterations"] == per_call["iterations"]
            for got in (b, c[0]):
                assert np.array_equal(got[0], a[0]) and np.array_equal(got[1], a[1]), shape
            check_ascent(a, per_call, case, grid, rates, f"three entries, max_iters = {max_iters}, {shape}")


SMALL_BATCH = [(3, 5), (4, 33), (65, 64), (7, 513)]


@pytest.mark.parametrize("max_iters", [4, 50])
def test_a_batch_of_small_families_that_stop_at_different_rounds(banks, max_iters):
    """Four families in lockstep that leave the loop at different rounds.  With these seeds the restatement takes 1, 2, 7 and 5
    iterations; max_iters = 4 cuts the last two off while they are still moving.  Each family's lengths, rates and iteration
    count are those of its own cb_ble call, with the kernel time asked for and without."""
    from cherryml_amd.phylogeny_estimation import (estimate_branch_lengths_and_site_rates,
                                                   estimate_branch_lengths_and_site_rates_batch)
    logP, grid, rates = banks("lg4")
    cases = [ascent_case("lg4", s, max_iters) for s in SMALL_BATCH]
    # the precondition, on the CPU: the iteration counts differ, and the cut families would have gone on
    assert [ascent_case("lg4", s, 50)[6] for s in SMALL_BATCH] == [1, 2, 7, 5]
    assert [c[6] for c in cases] == ([1, 2, 4, 4] if max_iters == 4 else [1, 2, 7, 5])
    assert all(c[7] > UNDECIDED for c in cases)
    w = cases[0][3]
    prof = {}
    timed = estimate_branch_lengths_and_site_rates_batch([c[:3] for c in cases], logP, grid, rates, w, max_iters, profile=prof)
    plain = estimate_branch_lengths_and_site_rates_batch([c[:3] for c in cases], logP, grid, rates, w, max_iters)
    assert len(timed) == len(plain) == 4 and prof["kernel_ms"] > 0.0
    for k, (shape, case) in enumerate(zip(SMALL_BATCH, cases)):
        own = {}
        want = estimate_branch_lengths_and_site_rates(*case[:3], logP, grid, rates, w, max_iters, profile=own)
        bare = estimate_branch_lengths_and_site_rates(*case[:3], logP, grid, rates, w, max_iters)
        for got in (timed[k], plain[k], bare):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), shape
        assert prof["iterations"][k] == own["iterations"], shape
        check_ascent(want, own, case, grid, rates, f"small batch, max_iters = {max_iters}, {shape}")
