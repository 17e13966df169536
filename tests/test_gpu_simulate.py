"""MSA simulation on the MI355X: the reference's own two checks, an exact restatement of the stream (tests/sim_stream.py),
the transition law on one edge against expm, exact cases (copies, seeds, batching), a round trip simulate -> count -> learn
against the true LG, and two ranks against one."""
import os
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sim_stream  # noqa: E402
from conftest import load_golden  # noqa: E402

SIM = os.path.join(ROOT, "tests", "golden", "simulation")
FAMS3 = ["fam1", "fam2", "fam3"]
AA = list("ARNDCQEGHILKMFPSTWYV")


def synthetic_contact_map(num_sites, num_sites_in_contact, random_seed):
    """num_sites_in_contact random sites, paired up at random; symmetric, ones on the diagonal."""
    rng = np.random.default_rng(random_seed)
    sites = rng.permutation(num_sites)[:num_sites_in_contact]
    cm = np.eye(num_sites, dtype=int)
    for a, b in sites.reshape(-1, 2):
        cm[a, b] = cm[b, a] = 1
    return cm


def _ref_inputs(tmp_path, model, num_sites, num_in_contact, seed=0, copies=1):
    """The reference test's inputs.  copies > 1: the three trees again under further names (fam1_c1, ...), each with a
    contact map of its own -- more independent trees behind the same leaf-frequency bar."""
    import shutil
    from cherryml_amd.io import write_contact_map, write_site_rates
    fams = list(FAMS3) + [f"{f}_c{c}" for c in range(1, copies) for f in FAMS3]
    tree_dir = os.path.join(SIM, "tree_dir")
    if copies > 1:
        tree_dir = str(tmp_path / "trees")
        os.makedirs(tree_dir, exist_ok=True)
        for f in fams:
            shutil.copy(os.path.join(SIM, "tree_dir", f.split("_")[0] + ".txt"), os.path.join(tree_dir, f + ".txt"))
    cms = {}
    for i, f in enumerate(fams):
        cms[f] = synthetic_contact_map(num_sites, num_in_contact, i)
        write_contact_map(cms[f], str(tmp_path / "cm" / (f + ".txt")))
        write_site_rates([1.0 * np.log(1 + i) for i in range(num_sites)], str(tmp_path / "rates" / (f + ".txt")))
    kw = dict(tree_dir=tree_dir, site_rates_dir=str(tmp_path / "rates"),
              contact_map_dir=str(tmp_path / "cm"), families=fams, amino_acids=["S", "T"],
              pi_1_path=os.path.join(SIM, model, "pi_1.txt"), Q_1_path=os.path.join(SIM, model, "Q_1.txt"),
              pi_2_path=os.path.join(SIM, model, "pi_2.txt"), Q_2_path=os.path.join(SIM, model, "Q_2.txt"),
              strategy="all_transitions", random_seed=seed, output_msa_dir=str(tmp_path / "out"), num_processes=3)
    return kw, cms


def _leaf_counts(kw, cms, num_sites):
    from cherryml_amd.io import read_msa, read_tree
    C1, C2 = defaultdict(int), defaultdict(int)
    for f in kw["families"]:
        tree = read_tree(os.path.join(kw["tree_dir"], f + ".txt"))
        msa = read_msa(os.path.join(kw["output_msa_dir"], f + ".txt"))
        assert sorted(msa) == sorted(tree.nodes()), f"{f}: not every node has a sequence"
        assert all(len(s) == num_sites for s in msa.values())
        i, j = np.where(cms[f] == 1)
        pairs = [(a, b) for a, b in zip(i, j) if a < b]
        in_contact = {s for p in pairs for s in p}
        indep = [s for s in range(num_sites) if s not in in_contact]
        for v in tree.leaves():
            seq = msa[v]
            for s in indep:
                C1[seq[s]] += 1
            for a, b in pairs:
                C2[seq[a] + seq[b]] += 1
    return C1, C2


# ------------------------------------------------------------------------------ 1. the reference's own checks
def test_extreme_model(tmp_path):
    from cherryml_amd import simulate_msas
    kw, cms = _ref_inputs(tmp_path, "extreme_model", 100, 50)
    simulate_msas(**kw)
    C1, C2 = _leaf_counts(kw, cms, 100)
    assert C1["S"] / sum(C1.values()) >= 0.95, dict(C1)
    assert C2["TT"] / sum(C2.values()) >= 0.95, dict(C2)


def test_normal_model(tmp_path):
    """The reference's bar (every leaf frequency within 10 % of pi), on its three trees under 16 names each.  On the three
    trees alone the bar is about 1.2 sigma for the pair states (a handful of leaves per tree, and leaves of one tree share
    their ancestors: about 750 independent pair draws), so it fails for a sizeable share of random streams; 48 trees put it
    near 5 sigma."""
    from cherryml_amd import simulate_msas
    from cherryml_amd.io import read_probability_distribution
    kw, cms = _ref_inputs(tmp_path, "normal_model", 1000, 500, copies=16)
    simulate_msas(**kw)
    C1, C2 = _leaf_counts(kw, cms, 1000)
    for C, name in ((C1, "pi_1"), (C2, "pi_2")):
        pi = read_probability_distribution(os.path.join(SIM, "normal_model", name + ".txt"))
        n = sum(C.values())
        for state in pi.index:
            want = n * float(pi.loc[state].iloc[0])
            assert abs(C[state] - want) <= 0.10 * want, (name, state, C[state], want)


# ------------------------------------------------------------------------------ 2. exact restatement
def _lg():
    z = load_golden("likelihood.npz")
    return z["lg"], z["pi_lg"]


def _demo_dirs(tmp_path, n=32):
    from cherryml_amd.estimation_end_to_end import create_maximal_matching_contact_map
    z = load_golden("demo32_co_inputs.npz")
    fams = [str(f) for f in z["families"]][:n]
    dirs = {}
    for kind in ("tree", "contact_map"):
        d = tmp_path / kind
        d.mkdir(exist_ok=True)
        off, blob = z[f"{kind}_offsets"], z[f"{kind}_bytes"].tobytes()
        for k, fam in enumerate(fams):
            (d / f"{fam}.txt").write_bytes(blob[off[k]:off[k + 1]])
        dirs[kind] = str(d)
    dirs["matched"] = str(tmp_path / "matched")
    create_maximal_matching_contact_map(i_contact_map_dir=dirs["contact_map"], families=fams,
                                        minimum_distance_for_nontrivial_contact=7, num_processes=1,
                                        o_contact_map_dir=dirs["matched"])
    dirs["rates"] = os.path.join(SIM, "demo_site_rates")
    return dirs, fams


def _lg_pair_model():
    Q, pi = _lg()
    I = np.eye(20)
    return Q, pi, np.kron(Q, I) + np.kron(I, Q), np.kron(pi, pi)


def _compare(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got[0], want[0]), "a root character differs"
    bad = int(np.count_nonzero(got != want))
    print(f"restatement: {bad} of {got.size} characters differ")
    assert bad <= 1e-5 * got.size, bad
    return bad


def test_exact_restatement_reference_trees(tmp_path):
    from cherryml_amd import _lib
    from cherryml_amd.io import read_probability_distribution, read_rate_matrix
    from cherryml_amd.simulation import Simulator, family_seed
    from cherryml_amd.simulation._simulate import _read_family
    kw, _ = _ref_inputs(tmp_path, "normal_model", 1000, 500)
    m = os.path.join(SIM, "normal_model")
    Q1, Q2 = read_rate_matrix(os.path.join(m, "Q_1.txt")).to_numpy(), read_rate_matrix(os.path.join(m, "Q_2.txt")).to_numpy()
    p1 = read_probability_distribution(os.path.join(m, "pi_1.txt")).to_numpy().ravel()
    p2 = read_probability_distribution(os.path.join(m, "pi_2.txt")).to_numpy().ravel()
    fams = [_read_family(kw["tree_dir"], kw["site_rates_dir"], kw["contact_map_dir"], f, family_seed(f, 0)) for f in FAMS3]
    with Simulator(Q1, p1, Q2, p2) as sim:
        got = sim.run(fams)
    lib = _lib.load()
    t1, t2 = sim_stream.model_tables(lib, Q1, p1), sim_stream.model_tables(lib, Q2, p2)
    for f, g in zip(fams, got):
        _compare(g, sim_stream.simulate_family(t1, t2, 2, f))


def test_exact_restatement_demo_family_with_pairs(tmp_path):
    from cherryml_amd import _lib
    from cherryml_amd.simulation import Simulator, family_seed
    from cherryml_amd.simulation._simulate import _read_family
    dirs, fams = _demo_dirs(tmp_path, 2)
    Q1, p1, Q2, p2 = _lg_pair_model()
    fam = _read_family(dirs["tree"], dirs["rates"], dirs["matched"], fams[1], family_seed(fams[1], 7))
    assert (fam["site_b"] >= 0).sum() > 10
    with Simulator(Q1, p1, Q2, p2) as sim:
        got = sim.run([fam])[0]
    lib = _lib.load()
    _compare(got, sim_stream.simulate_family(sim_stream.model_tables(lib, Q1, p1), sim_stream.model_tables(lib, Q2, p2), 20, fam))


# ------------------------------------------------------------------------------ 3. the law of one edge
def _one_edge(Q1, p1, Q2, p2, n_units, pairs, t):
    from cherryml_amd.simulation import Simulator
    L = 2 * n_units if pairs else n_units
    u = np.arange(n_units, dtype=np.int32)
    fam = dict(seed=12345, parent=np.array([-1, 0]), length=np.array([0.0, t]), n_sites=L,
               site_a=2 * u if pairs else u, site_b=2 * u + 1 if pairs else np.full(n_units, -1),
               rate=np.ones(n_units))
    with Simulator(Q1, p1, Q2, p2) as sim:
        return sim.run([fam])[0]


@pytest.mark.parametrize("pairs", [False, True])
def test_one_edge_matches_expm(pairs):
    from scipy.linalg import expm
    Q1, p1, Q2, p2 = _lg_pair_model()
    n, t = 200000, 0.3
    a = 7 if not pairs else 7 * 20 + 13
    Q = Q2 if pairs else Q1
    e = np.zeros(Q.shape[0])
    e[a] = 1.0
    codes = _one_edge(Q1, e if not pairs else p1, Q2, e if pairs else p2, n, pairs, t)
    if pairs:
        root = codes[0, 0::2].astype(np.int64) * 20 + codes[0, 1::2]
        leaf = codes[1, 0::2].astype(np.int64) * 20 + codes[1, 1::2]
    else:
        root, leaf = codes[0].astype(np.int64), codes[1].astype(np.int64)
    assert np.all(root == a)
    want = n * expm(t * Q)[a]
    got = np.bincount(leaf, minlength=Q.shape[0])
    sigma = np.sqrt(np.maximum(want * (1 - want / n), 1e-12))
    z = np.abs(got - want) / sigma
    assert np.all(got[want < 1e-9] == 0)
    assert z.max() < 5.0, (int(z.argmax()), got[z.argmax()], want[z.argmax()])


# ------------------------------------------------------------------------------ 4. exact cases
def test_zero_length_and_zero_rate_copy_the_parent():
    from cherryml_amd.simulation import Simulator
    Q1, p1, Q2, p2 = _lg_pair_model()
    L = 3000
    rate = np.where(np.arange(L) % 2 == 0, 0.0, 2.0)
    fam = dict(seed=99, parent=np.array([-1, 0, 0, 1]), length=np.array([0.0, 0.0, 0.5, 0.7]), n_sites=L,
               site_a=np.arange(L), site_b=np.full(L, -1), rate=rate)
    with Simulator(Q1, p1) as sim:
        c = sim.run([fam])[0]
    assert np.array_equal(c[1], c[0])                          # zero-length branch
    assert np.array_equal(c[2, ::2], c[0, ::2]) and np.array_equal(c[3, ::2], c[0, ::2])   # site rate 0
    assert np.count_nonzero(c[2, 1::2] != c[0, 1::2]) > 100   # the other sites did move


def test_seeds_and_batching(tmp_path):
    from cherryml_amd import simulate_msas
    from cherryml_amd.io import write_probability_distribution, write_rate_matrix
    dirs, fams = _demo_dirs(tmp_path, 32)
    Q1, p1, Q2, p2 = _lg_pair_model()
    pairs = [a + b for a in AA for b in AA]
    mp = {}
    for name, M, st in (("Q1", Q1, AA), ("Q2", Q2, pairs)):
        mp[name] = str(tmp_path / "model" / f"{name}.txt")
        write_rate_matrix(M, st, mp[name])
    for name, p, st in (("p1", p1, AA), ("p2", p2, pairs)):
        mp[name] = str(tmp_path / "model" / f"{name}.txt")
        write_probability_distribution(p, st, mp[name])

    def run(out, families, seed):
        simulate_msas(tree_dir=dirs["tree"], site_rates_dir=dirs["rates"], contact_map_dir=dirs["matched"], families=families,
                      amino_acids=AA, pi_1_path=mp["p1"], Q_1_path=mp["Q1"], pi_2_path=mp["p2"], Q_2_path=mp["Q2"],
                      strategy="all_transitions", random_seed=seed, output_msa_dir=str(tmp_path / out))
        return {f: open(tmp_path / out / (f + ".txt"), "rb").read() for f in families}

    a, b = run("a", fams, 0), run("b", fams, 0)
    assert a == b
    c = run("c", fams, 1)
    assert all(a[f] != c[f] for f in fams)
    alone = run("d", [fams[5]], 0)
    assert alone[fams[5]] == a[fams[5]]


# ------------------------------------------------------------------------------ 5. round trip against the true LG
def test_round_trip_learns_lg_back(tmp_path):
    import cherryml_amd
    from cherryml_amd import simulate_msas
    from cherryml_amd.estimation_end_to_end._cherry import _grid
    from cherryml_amd.io import read_rate_matrix, write_contact_map, write_probability_distribution, write_rate_matrix
    dirs, fams = _demo_dirs(tmp_path, 32)
    Q, pi = _lg()
    pairs = [a + b for a in AA for b in AA]
    I = np.eye(20)
    m = tmp_path / "model"
    write_rate_matrix(Q, AA, str(m / "Q1.txt"))
    write_probability_distribution(pi, AA, str(m / "p1.txt"))
    write_rate_matrix(np.kron(Q, I) + np.kron(I, Q), pairs, str(m / "Q2.txt"))
    write_probability_distribution(np.kron(pi, pi), pairs, str(m / "p2.txt"))
    for f in fams:   # no contacts
        n = int(open(os.path.join(dirs["rates"], f + ".txt")).read().split()[0])
        write_contact_map(np.zeros((n, n), dtype=int), str(tmp_path / "nocm" / (f + ".txt")))
    simulate_msas(tree_dir=dirs["tree"], site_rates_dir=dirs["rates"], contact_map_dir=str(tmp_path / "nocm"), families=fams,
                  amino_acids=AA, pi_1_path=str(m / "p1.txt"), Q_1_path=str(m / "Q1.txt"), pi_2_path=str(m / "p2.txt"),
                  Q_2_path=str(m / "Q2.txt"), strategy="all_transitions", random_seed=0, output_msa_dir=str(tmp_path / "msa"))
    cherryml_amd.count_transitions(tree_dir=dirs["tree"], msa_dir=str(tmp_path / "msa"), site_rates_dir=dirs["rates"],
                                   families=fams, amino_acids=AA, quantization_points=_grid(0.03, 1.1, 64),
                                   edge_or_cherry="cherry", output_count_matrices_dir=str(tmp_path / "counts"))
    counts = str(tmp_path / "counts" / "result.txt")
    cherryml_amd.jtt_ipw(count_matrices_path=counts, mask_path=None, use_ipw=True, output_rate_matrix_dir=str(tmp_path / "jtt"),
                         normalize=False, max_time=None)
    cherryml_amd.quantized_transitions_mle(count_matrices_path=counts, initialization_path=str(tmp_path / "jtt" / "result.txt"),
                                           mask_path=None, output_rate_matrix_dir=str(tmp_path / "mle"), device="cuda",
                                           num_epochs=500)
    Qh = read_rate_matrix(str(tmp_path / "mle" / "result.txt")).to_numpy()
    off = ~np.eye(20, dtype=bool)
    w = np.broadcast_to(pi[:, None], (20, 20))[off]
    rel = np.abs(Qh[off] - Q[off]) / Q[off]
    err = float(np.sum(w * rel) / np.sum(w))
    print(f"round trip: pi-weighted mean relative error of the off-diagonal rates = {err:.4f}")
    assert err < 0.10, err


# ------------------------------------------------------------------------------ 6. two ranks on one GPU
_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
world = int(os.environ["WORLD_SIZE"])
if world > 1:
    dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=world)
torch.cuda.set_device(0)
import json
from cherryml_amd import simulate_msas
simulate_msas(**json.loads(sys.argv[2]))
if world > 1:
    dist.destroy_process_group()
'''


def test_two_ranks_write_the_files_of_one_rank(tmp_path):
    import json
    kw, _ = _ref_inputs(tmp_path, "normal_model", 1000, 500)
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    base.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29583")
    one = dict(kw, output_msa_dir=str(tmp_path / "one"))
    two = dict(kw, output_msa_dir=str(tmp_path / "two"))
    subprocess.run([sys.executable, str(script), ROOT, json.dumps(one)], env=dict(base, RANK="0", WORLD_SIZE="1"), check=True,
                   timeout=300)
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, json.dumps(two)], env=dict(base, RANK=str(r), WORLD_SIZE="2"))
             for r in range(2)]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    for f in FAMS3:
        assert open(tmp_path / "one" / (f + ".txt"), "rb").read() == open(tmp_path / "two" / (f + ".txt"), "rb").read(), f
