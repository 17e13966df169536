"""MSA simulation without a GPU: the random stream's building blocks (Philox against the Random123 known answers, the alias
tables of cb_sim_alias_table), the io writers, the reference's input validation (raised before any GPU work), the loud
failure without a GPU, and the kernel's resources."""
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

from sim_stream import alias_table, philox4x32_10, uniform  # noqa: E402

from cherryml_amd import _lib  # noqa: E402

SIM = os.path.join(ROOT, "tests", "golden", "simulation")


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    x = philox4x32_10(*[np.array([c], dtype=np.uint64) for c in ctr], *key)
    assert " ".join("%08x" % int(w[0]) for w in x) == want


def test_uniforms_lie_in_the_open_unit_interval_ends():
    lo = uniform(np.array([0], dtype=np.uint64), np.array([0], dtype=np.uint64))
    hi = uniform(np.array([0xFFFFFFFF], dtype=np.uint64), np.array([0xFFFFFFFF], dtype=np.uint64))
    assert lo[0] == 2.0 ** -54 and 0.0 < lo[0] and hi[0] <= 1.0


def _column_mass(prob, alias):
    n = len(prob)
    mass = prob.copy()
    np.add.at(mass, alias, 1.0 - prob)
    return mass / n


@pytest.mark.parametrize("n,zeros", [(1, 0), (2, 1), (20, 1), (20, 6), (400, 361), (400, 0)])
def test_alias_table_reproduces_its_weights(n, zeros):
    lib = _lib.load()
    rng = np.random.default_rng(n + zeros)
    w = rng.exponential(size=n) * 10.0 ** rng.uniform(-3, 3, size=n)
    w[rng.choice(n, size=zeros, replace=False)] = 0.0
    prob, alias = alias_table(lib, w)
    assert np.all((prob >= 0) & (prob <= 1)) and np.all((alias >= 0) & (alias < n))
    assert np.max(np.abs(_column_mass(prob, alias) - w / w.sum())) <= 1e-15
    dead = w == 0
    assert np.all(prob[dead] == 0.0)                          # the column itself is never taken ...
    assert not np.any(dead[alias[prob < 1.0]])                # ... nor is it anyone's alias


def test_alias_table_refuses_bad_weights():
    lib = _lib.load()
    for w in ([0.0, 0.0], [1.0, -1.0], [1.0, np.nan], [np.inf, 1.0]):
        w = np.array(w)
        prob, alias = np.empty(2), np.empty(2, dtype=np.int32)
        assert lib.cb_sim_alias_table(2, w.ctypes.data, prob.ctypes.data, alias.ctypes.data) == _lib.CB_EINVAL


def test_model_create_validates_before_looking_for_a_device():
    """A bad model is CB_EINVAL whether or not a GPU is there (the check comes first)."""
    import ctypes
    lib = _lib.load()
    pi = np.array([0.5, 0.5])
    h = ctypes.c_void_p()
    for Q in (np.array([[-1.0, -1.0], [1.0, -1.0]]), np.array([[1.0, 1.0], [1.0, -1.0]]), np.array([[-1.0, 0.0], [1.0, -1.0]])):
        assert lib.cb_sim_model_create(0, 2, Q.ctypes.data, pi.ctypes.data, None, None, ctypes.byref(h)) == _lib.CB_EINVAL
    assert lib.cb_sim_model_create(0, 1, pi.ctypes.data, pi.ctypes.data, None, None, ctypes.byref(h)) == _lib.CB_EINVAL


# ----------------------------------------------------------------------------------------------------------- io writers
def test_writers_round_trip_in_the_reference_byte_format(tmp_path):
    from cherryml_amd.io import read_contact_map, read_msa, read_site_rates, write_contact_map, write_msa, write_site_rates
    p = str(tmp_path / "a" / "msa.txt")
    write_msa({"seq2": "TS", "internal-0": "SS", "seq1": "ST"}, p)
    assert open(p).read() == ">internal-0\nSS\n>seq1\nST\n>seq2\nTS\n"
    assert read_msa(p) == {"internal-0": "SS", "seq1": "ST", "seq2": "TS"}
    p = str(tmp_path / "b" / "rates.txt")
    rates = [0.0, 0.6931471805599453, 1.5, 2.0]
    write_site_rates(rates, p)
    assert open(p).read() == "4 sites\n0.0 0.6931471805599453 1.5 2.0"
    assert read_site_rates(p).tolist() == rates
    p = str(tmp_path / "c" / "cm.txt")
    cm = np.array([[1, 0, 1], [0, 1, 0], [1, 0, 1]])
    write_contact_map(cm, p)
    assert open(p).read() == "3 sites\n101\n010\n101\n"
    assert np.array_equal(read_contact_map(p), cm)


# ------------------------------------------------------------------------------------------------ validation, no GPU work
def contact_map_with_pairs(num_sites, pairs):
    cm = np.eye(num_sites, dtype=int)
    for i, j in pairs:
        cm[i, j] = cm[j, i] = 1
    return cm


@pytest.fixture()
def inputs(tmp_path):
    from cherryml_amd.io import write_contact_map, write_site_rates
    fams = ["fam1", "fam2", "fam3"]
    for f in fams:
        write_contact_map(contact_map_with_pairs(10, [(0, 5), (2, 3)]), str(tmp_path / "cm" / (f + ".txt")))
        write_site_rates([1.0] * 10, str(tmp_path / "rates" / (f + ".txt")))
    return dict(tree_dir=os.path.join(SIM, "tree_dir"), site_rates_dir=str(tmp_path / "rates"),
                contact_map_dir=str(tmp_path / "cm"), families=fams, amino_acids=["S", "T"],
                pi_1_path=os.path.join(SIM, "normal_model", "pi_1.txt"), Q_1_path=os.path.join(SIM, "normal_model", "Q_1.txt"),
                pi_2_path=os.path.join(SIM, "normal_model", "pi_2.txt"), Q_2_path=os.path.join(SIM, "normal_model", "Q_2.txt"),
                strategy="all_transitions", random_seed=0, output_msa_dir=str(tmp_path / "out"))


@pytest.fixture()
def no_gpu_work(monkeypatch):
    from cherryml_amd.simulation import _simulate

    class Refuse:
        def __init__(self, *a, **k):
            raise AssertionError("the GPU model was created before the inputs were validated")
    monkeypatch.setattr(_simulate, "Simulator", Refuse)


def _swap_rows(src, dst, i, j):
    lines = open(src).read().strip().split("\n")
    lines[i], lines[j] = lines[j], lines[i]
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_a_site_in_two_contacts_raises(inputs, tmp_path, no_gpu_work):
    from cherryml_amd import simulate_msas
    from cherryml_amd.io import write_contact_map
    write_contact_map(contact_map_with_pairs(10, [(0, 5), (5, 7)]), os.path.join(inputs["contact_map_dir"], "fam2.txt"))
    with pytest.raises(Exception, match="only be in contact with one other site"):
        simulate_msas(**inputs)


def test_a_contact_out_of_range_raises(inputs, no_gpu_work):
    from cherryml_amd import simulate_msas
    from cherryml_amd.io import write_contact_map, write_site_rates
    write_contact_map(contact_map_with_pairs(12, [(0, 11)]), os.path.join(inputs["contact_map_dir"], "fam1.txt"))
    write_site_rates([1.0] * 10, os.path.join(inputs["site_rates_dir"], "fam1.txt"))
    with pytest.raises(Exception, match="out of range"):
        simulate_msas(**inputs)


@pytest.mark.parametrize("which,rows,match", [("pi_1_path", (1, 2), "pi_1 index"), ("pi_2_path", (2, 3), "pi_2 index"),
                                              ("Q_2_path", (1, 4), "Q_2 index")])
def test_a_wrong_state_order_raises(inputs, tmp_path, no_gpu_work, which, rows, match):
    from cherryml_amd import simulate_msas
    bad = str(tmp_path / "bad.txt")
    _swap_rows(inputs[which], bad, *rows)
    inputs[which] = bad
    with pytest.raises(Exception, match=match):
        simulate_msas(**inputs)


def test_wrong_q1_columns_raise(inputs, tmp_path, no_gpu_work):
    from cherryml_amd import simulate_msas
    Q = pd.read_csv(inputs["Q_1_path"], sep=r"\s+", index_col=0)
    bad = str(tmp_path / "q1.txt")
    Q[["T", "S"]].to_csv(bad, sep="\t")
    inputs["Q_1_path"] = bad
    with pytest.raises(Exception, match="Q_1 columns"):
        simulate_msas(**inputs)


@pytest.mark.parametrize("strategy", ["chain_jump", "node_states", "bogus"])
def test_an_unknown_strategy_raises(inputs, no_gpu_work, strategy):
    from cherryml_amd import simulate_msas
    inputs["strategy"] = strategy
    with pytest.raises(Exception, match="Unknown strategy"):
        simulate_msas(**inputs)


def test_no_gpu_means_simulate_msas_fails_loudly(inputs):
    if _lib.load().cb_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cherryml_amd import simulate_msas
    with pytest.raises(_lib.CherryBankError):
        simulate_msas(**inputs)
    assert not [f for f in os.listdir(inputs["output_msa_dir"]) if f.endswith(".txt")]


# ---------------------------------------------------------------------------------------------------------- resources
def test_sim_walk_has_no_scratch_and_no_spills():
    from cherryml_amd import _build
    from kernel_meta import kernel_meta
    _build.build()
    hits = {k: v for k, v in kernel_meta().items() if k.startswith("sim_walk")}
    assert hits, "no sim_walk in the built objects"
    for name, m in hits.items():
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (name, m)
