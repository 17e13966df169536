"""Full-tree EM on the GPU (csrc/em.hip.h, cb_em_*, estimation.EStep / em_lg): the E-step against the NumPy restatement and
against the held-out likelihood, posterior mass, the Fisher identity, determinism and splitting (batches, two ranks), a
monotone EM, and the round trip LG -> simulate -> em_lg -> LG."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import em_reference  # noqa: E402
from conftest import load_golden  # noqa: E402

SIM = os.path.join(ROOT, "tests", "golden", "simulation")
AA = list("ARNDCQEGHILKMFPSTWYV")
GRID = np.array([0.03 * 1.1 ** i for i in range(-64, 65)])


def _lg():
    z = load_golden("likelihood.npz")
    return z["lg"], z["pi_lg"]


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    """the 32 demo trees with leaves (and internal nodes) simulated under LG at the demo site rates"""
    from cherryml_amd import simulate_msas
    from cherryml_amd.io import write_contact_map, write_probability_distribution, write_rate_matrix
    tmp = tmp_path_factory.mktemp("em_demo")
    z = load_golden("demo32_co_inputs.npz")
    fams = [str(f) for f in z["families"]]
    tree_dir = tmp / "tree"
    tree_dir.mkdir()
    off, blob = z["tree_offsets"], z["tree_bytes"].tobytes()
    for k, fam in enumerate(fams):
        (tree_dir / f"{fam}.txt").write_bytes(blob[off[k]:off[k + 1]])
    rates = os.path.join(SIM, "demo_site_rates")
    Q, pi = _lg()
    m = tmp / "model"
    m.mkdir()
    pairs = [a + b for a in AA for b in AA]
    I = np.eye(20)
    write_rate_matrix(Q, AA, str(m / "Q1.txt"))
    write_probability_distribution(pi, AA, str(m / "p1.txt"))
    write_rate_matrix(np.kron(Q, I) + np.kron(I, Q), pairs, str(m / "Q2.txt"))
    write_probability_distribution(np.kron(pi, pi), pairs, str(m / "p2.txt"))
    (tmp / "nocm").mkdir()
    for f in fams:
        n = int(open(os.path.join(rates, f + ".txt")).read().split()[0])
        write_contact_map(np.zeros((n, n), dtype=int), str(tmp / "nocm" / (f + ".txt")))
    simulate_msas(tree_dir=str(tree_dir), site_rates_dir=rates, contact_map_dir=str(tmp / "nocm"), families=fams,
                  amino_acids=AA, pi_1_path=str(m / "p1.txt"), Q_1_path=str(m / "Q1.txt"), pi_2_path=str(m / "p2.txt"),
                  Q_2_path=str(m / "Q2.txt"), strategy="all_transitions", random_seed=0, output_msa_dir=str(tmp / "msa"))
    return dict(tmp=tmp, fams=fams, tree=str(tree_dir), msa=str(tmp / "msa"), rates=rates, Q=Q, pi=pi)


def _families(demo, fams, gap_fraction=0.0, seed=0):
    from cherryml_amd.estimation._em import _read_family
    rng = np.random.default_rng(seed)
    out = []
    for f in fams:
        tree, codes, rates = _read_family(demo["tree"], demo["msa"], demo["rates"], f, AA)
        if gap_fraction:
            codes[rng.random(codes.shape) < gap_fraction] = -1
        out.append((tree, codes, rates))
    return out


def _arrays(tree):
    from cherryml_amd.evaluation._likelihood import _tree_arrays
    _, _, parent, length = _tree_arrays(tree)
    return parent, length


def _smallest(demo, k):
    sizes = [(os.path.getsize(os.path.join(demo["msa"], f + ".txt")), f) for f in demo["fams"]]
    return [f for _, f in sorted(sizes)[:k]]


def test_estep_matches_the_numpy_restatement(demo):
    from cherryml_amd.estimation import EStep
    fams = _families(demo, _smallest(demo, 2), gap_fraction=0.1, seed=1)
    Q, pi = demo["Q"], demo["pi"]
    with EStep([f[0] for f in fams], [f[1] for f in fams], [f[2] for f in fams], GRID) as es:
        E, ll = es.expected_counts(Q, pi)
        units = es.last_unit_loglik
    E_ref, ll_ref = np.zeros_like(E), []
    for tree, codes, rates in fams:
        parent, length = _arrays(tree)
        e, l_u = em_reference.estep(parent, length, codes, rates, GRID, Q, pi)
        E_ref += e
        ll_ref.append(l_u)
    err_E = np.abs(E - E_ref).max() / np.abs(E_ref).max()
    err_l = max(np.abs(a - b).max() for a, b in zip(units, ll_ref))
    print(f"restatement: max |dE| / max|E| = {err_E:.2e}, max |d l_u| = {err_l:.2e}")
    assert err_E < 1e-10 and err_l < 1e-10
    assert abs(ll - sum(x.sum() for x in ll_ref)) < 1e-9 * abs(ll)


def test_estep_loglik_equals_the_held_out_likelihood(demo):
    """rates 1 and every branch length on a grid point: the quantised model IS the model tree_likelihood evaluates"""
    from cherryml_amd.estimation import EStep
    from cherryml_amd.evaluation import tree_likelihood_batch
    from cherryml_amd.io import Tree
    fams = _families(demo, _smallest(demo, 3), gap_fraction=0.05, seed=2)
    trees = []
    for tree, _, _ in fams:
        t = Tree()
        t.add_nodes(tree.nodes())
        t.add_edges([(p, c, float(GRID[em_reference.quantize(max(w, 1e-9), GRID)])) for p, c, w in tree.edges()])
        trees.append(t)
    ones = [np.ones(f[2].size) for f in fams]
    Q, pi = demo["Q"], demo["pi"]
    with EStep(trees, [f[1] for f in fams], ones, GRID) as es:
        es.expected_counts(Q, pi)
        units = es.last_unit_loglik
    want = tree_likelihood_batch(trees, [f[1] for f in fams], None, Q, pi, ones)
    err = max(np.abs(a - b).max() for a, b in zip(units, want))
    print(f"against tree_likelihood: max |d l_u| = {err:.2e}")
    assert err < 1e-10


def test_posterior_mass_determinism_and_batches(demo):
    from cherryml_amd.estimation import EStep
    fams = _families(demo, demo["fams"][:6], gap_fraction=0.05, seed=3)
    Q, pi = demo["Q"], demo["pi"]
    with EStep([f[0] for f in fams], [f[1] for f in fams], [f[2] for f in fams], GRID) as es:
        E1, ll1 = es.expected_counts(Q, pi)
        E2, ll2 = es.expected_counts(Q, pi)
        mass = es.num_edge_sites
        print(f"E-step kernel time: {es.last_kernel_ms:.3f} ms for 6 families")
    assert np.array_equal(E1, E2) and ll1 == ll2
    assert abs(E1.sum() - mass) < 1e-10 * mass
    parts = []
    for chunk in (fams[:2], fams[2:]):
        with EStep([f[0] for f in chunk], [f[1] for f in chunk], [f[2] for f in chunk], GRID) as es:
            parts.append(es.expected_counts(Q, pi))
    E_split, ll_split = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    assert np.abs(E_split - E1).max() < 1e-12 * np.abs(E1).max()
    assert abs(ll_split - ll1) < 1e-12 * abs(ll1)


def test_fisher_identity(demo):
    from scipy.linalg import expm, expm_frechet
    from cherryml_amd.estimation import EStep
    fams = _families(demo, _smallest(demo, 3), gap_fraction=0.05, seed=4)
    Q, pi = demo["Q"], demo["pi"]
    rng = np.random.default_rng(5)
    H = rng.uniform(-1.0, 1.0, Q.shape) * np.abs(Q)
    np.fill_diagonal(H, 0.0)
    np.fill_diagonal(H, -H.sum(axis=1))
    eps = 1e-5
    with EStep([f[0] for f in fams], [f[1] for f in fams], [f[2] for f in fams], GRID) as es:
        E, _ = es.expected_counts(Q, pi)
        lp = es.expected_counts(Q + eps * H, pi)[1]
        lm = es.expected_counts(Q - eps * H, pi)[1]
    fd = (lp - lm) / (2 * eps)
    grad = 0.0
    for b, t in enumerate(GRID):
        if E[b].any():
            grad += np.sum(E[b] / expm(t * Q) * expm_frechet(t * Q, t * H, compute_expm=False))
    print(f"Fisher identity: finite difference {fd:.10g}, expected-count gradient {grad:.10g}")
    assert abs(fd - grad) < 1e-6 * abs(grad)


def _cherry(demo, fams, tag):
    import cherryml_amd
    from cherryml_amd.estimation_end_to_end._cherry import _grid
    tmp = demo["tmp"] / tag
    cherryml_amd.count_transitions(tree_dir=demo["tree"], msa_dir=demo["msa"], site_rates_dir=demo["rates"], families=fams,
                                   amino_acids=AA, quantization_points=_grid(0.03, 1.1, 64), edge_or_cherry="cherry",
                                   output_count_matrices_dir=str(tmp / "counts"))
    counts = str(tmp / "counts" / "result.txt")
    cherryml_amd.jtt_ipw(count_matrices_path=counts, mask_path=None, use_ipw=True, output_rate_matrix_dir=str(tmp / "jtt"),
                         normalize=False, max_time=None)
    cherryml_amd.quantized_transitions_mle(count_matrices_path=counts, initialization_path=str(tmp / "jtt" / "result.txt"),
                                           mask_path=None, output_rate_matrix_dir=str(tmp / "mle"), device="cuda",
                                           num_epochs=500)
    return str(tmp / "jtt" / "result.txt"), str(tmp / "mle" / "result.txt")


def _err(Qh, Q, pi):
    off = ~np.eye(20, dtype=bool)
    w = np.broadcast_to(pi[:, None], (20, 20))[off]
    return float(np.sum(w * np.abs(Qh[off] - Q[off]) / Q[off]) / np.sum(w))


def test_em_is_monotone_from_the_cherry_estimate(demo):
    """em_lg records every iteration's log-likelihood, a decrease included: with tolerance -inf all 5 iterations run"""
    from cherryml_amd import em_lg
    fams = demo["fams"][:12]
    _, mle = _cherry(demo, fams, "mono")
    out = demo["tmp"] / "mono" / "em"
    em_lg(tree_dir=demo["tree"], msa_dir=demo["msa"], site_rates_dir=demo["rates"], families=fams,
          initialization_rate_matrix_path=mle, output_rate_matrix_dir=str(out), num_iterations=5, m_step_epochs=200,
          tolerance=-np.inf)
    lls = np.loadtxt(out / "log_likelihoods.txt")
    print("EM log-likelihoods from the cherry estimate:", lls)
    assert lls.shape == (6,), lls
    assert np.all(np.diff(lls) >= -1e-9 * np.abs(lls[:-1])), lls
    assert lls[-1] > lls[0]
    assert open(out / "profiling.txt").read().startswith("Total time: ")


def test_each_generalised_em_step_does_not_lower_the_likelihood(demo):
    """the E-step and M-step driven directly: every step, not only the recorded run, keeps the likelihood"""
    from cherryml_amd.estimation import EStep
    from cherryml_amd.estimation._em import m_step
    from cherryml_amd.evaluation._likelihood import _stationary_distribution
    from cherryml_amd.io import read_rate_matrix
    fams = demo["fams"][12:18]
    jtt, _ = _cherry(demo, fams, "steps")
    Q = read_rate_matrix(jtt).to_numpy()
    pi_root = _stationary_distribution(Q)
    data = _families(demo, fams)
    with EStep([d[0] for d in data], [d[1] for d in data], [d[2] for d in data], GRID) as es:
        E, ll = es.expected_counts(Q, pi_root)
        lls = [ll]
        for _ in range(5):
            Q = m_step(GRID, E, Q, 200, 0.1, 0)
            E, ll = es.expected_counts(Q, pi_root)
            lls.append(ll)
    print("direct EM steps from JTT-IPW:", lls)
    d = np.diff(lls)
    assert np.all(d >= -1e-9 * np.abs(np.array(lls[:-1]))), lls
    assert d[0] > 0, lls   # the first step from JTT-IPW gains: the M-step moves


def test_round_trip_learns_lg_back_with_em(demo):
    from cherryml_amd import em_lg
    from cherryml_amd.io import read_rate_matrix
    Q, pi = demo["Q"], demo["pi"]
    jtt, mle = _cherry(demo, demo["fams"], "rt")
    out = demo["tmp"] / "rt" / "em"
    em_lg(tree_dir=demo["tree"], msa_dir=demo["msa"], site_rates_dir=demo["rates"], families=demo["fams"],
          initialization_rate_matrix_path=jtt, output_rate_matrix_dir=str(out), num_iterations=10)
    res = read_rate_matrix(str(out / "result.txt"))
    assert list(res.index) == AA
    err_em, err_cherry = _err(res.to_numpy(), Q, pi), _err(read_rate_matrix(mle).to_numpy(), Q, pi)
    err_jtt = _err(read_rate_matrix(jtt).to_numpy(), Q, pi)
    lls = np.loadtxt(out / "log_likelihoods.txt")
    print(f"round trip: pi-weighted mean relative error EM = {err_em:.4f}, cherry = {err_cherry:.4f}, "
          f"JTT-IPW start = {err_jtt:.4f}; log-likelihoods {lls}")
    assert err_em < 0.10, err_em
    assert lls.size > 1 and lls[-1] > lls[0], lls      # EM moved away from its start ...
    assert err_em < err_jtt, (err_em, err_jtt)         # ... towards LG


_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
world = int(os.environ["WORLD_SIZE"])
if world > 1:
    dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=world)
torch.cuda.set_device(0)
from cherryml_amd.counting._stage import _my_families
from cherryml_amd.estimation._em import EStep, _all_reduce_f64, _read_family, DEFAULT_GRID
from cherryml_amd.io import read_rate_matrix, read_probability_distribution
tree, msa, rates, qp, pp, out = sys.argv[2:8]
fams = _my_families(sys.argv[8].split(","))
AA = list("ARNDCQEGHILKMFPSTWYV")
data = [_read_family(tree, msa, rates, f, AA) for f in fams]
Q = read_rate_matrix(qp).to_numpy()
pi = read_probability_distribution(pp).to_numpy().reshape(-1)
with EStep([d[0] for d in data], [d[1] for d in data], [d[2] for d in data], DEFAULT_GRID) as es:
    E, ll = es.expected_counts(Q, pi)
red = _all_reduce_f64(np.concatenate([E.reshape(-1), [ll]]))
if int(os.environ["RANK"]) == 0:
    np.save(out, red)
if world > 1:
    dist.destroy_process_group()
'''


def test_two_ranks_equal_one_rank(demo):
    tmp = demo["tmp"] / "ranks"
    tmp.mkdir()
    script = tmp / "worker.py"
    script.write_text(_WORKER)
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    base.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29587")
    fams = ",".join(demo["fams"][:5])
    args = [demo["tree"], demo["msa"], demo["rates"], str(demo["tmp"] / "model" / "Q1.txt"), str(demo["tmp"] / "model" / "p1.txt")]
    subprocess.run([sys.executable, str(script), ROOT, *args, str(tmp / "one.npy"), fams],
                   env=dict(base, RANK="0", WORLD_SIZE="1"), check=True, timeout=300)
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, *args, str(tmp / "two.npy"), fams],
                              env=dict(base, RANK=str(r), WORLD_SIZE="2")) for r in range(2)]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    one, two = np.load(tmp / "one.npy"), np.load(tmp / "two.npy")
    assert np.abs(one[:-1] - two[:-1]).max() < 1e-12 * np.abs(one[:-1]).max()
    assert abs(one[-1] - two[-1]) < 1e-12 * abs(one[-1])
