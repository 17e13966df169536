"""Time full-tree EM (`em_lg`, csrc/em.hip.h) on the 32 demo families (tests/golden/demo32_co_inputs.npz trees, site rates
tests/golden/simulation/demo_site_rates) with leaves simulated under LG.  Reports the E-step's device time (cb_em_estep's
kernel_ms: transition bank, inside and outside passes, accumulation and reduction), the whole `expected_counts` call, one
M-step (the optimiser, 500 epochs, warm-started) and the wall time per `em_lg` iteration; plus the number of kernel launches
one E-step makes (its passes are level-synchronous: one launch per tree height and per depth of every family).

    python profiles/tools/time_em.py [--repeats N] [--out profiles/em_demo32.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
AA = list("ARNDCQEGHILKMFPSTWYV")


def _launches(tree):
    """inside launches (heights) + outside launches (depths holding an internal non-root node)"""
    from cherryml_amd.evaluation._likelihood import _tree_arrays
    _, order, parent, _ = _tree_arrays(tree)
    n = parent.size
    height, depth, internal = np.zeros(n, int), np.zeros(n, int), np.zeros(n, bool)
    for v in order:
        if parent[v] >= 0:
            height[parent[v]] = max(height[parent[v]], height[v] + 1)
            internal[parent[v]] = True
    for v in order[::-1]:
        if parent[v] >= 0:
            depth[v] = depth[parent[v]] + 1
    return int(height.max() + 1) + len(set(depth[internal & (parent >= 0)].tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from conftest import load_golden

    from cherryml_amd import em_lg, simulate_msas
    from cherryml_amd.estimation._em import DEFAULT_GRID, EStep, _read_family, m_step
    from cherryml_amd.io import write_contact_map, write_probability_distribution, write_rate_matrix

    z = load_golden("demo32_co_inputs.npz")
    fams = [str(f) for f in z["families"]]
    lk = load_golden("likelihood.npz")
    Q, pi = lk["lg"], lk["pi_lg"]
    I = np.eye(20)
    pairs = [a + b for a in AA for b in AA]
    rates = os.path.join(ROOT, "tests", "golden", "simulation", "demo_site_rates")
    grid = np.array(DEFAULT_GRID)
    with tempfile.TemporaryDirectory() as tmp:
        td, cm = os.path.join(tmp, "tree"), os.path.join(tmp, "nocm")
        os.makedirs(td), os.makedirs(cm)
        off, blob = z["tree_offsets"], z["tree_bytes"].tobytes()
        for k, fam in enumerate(fams):
            with open(os.path.join(td, fam + ".txt"), "wb") as f:
                f.write(blob[off[k]:off[k + 1]])
            n = int(open(os.path.join(rates, fam + ".txt")).read().split()[0])
            write_contact_map(np.zeros((n, n), dtype=int), os.path.join(cm, fam + ".txt"))
        paths = {k: os.path.join(tmp, k + ".txt") for k in ("Q1", "Q2", "p1", "p2")}
        write_rate_matrix(Q, AA, paths["Q1"])
        write_rate_matrix(np.kron(Q, I) + np.kron(I, Q), pairs, paths["Q2"])
        write_probability_distribution(pi, AA, paths["p1"])
        write_probability_distribution(np.kron(pi, pi), pairs, paths["p2"])
        msa = os.path.join(tmp, "msa")
        simulate_msas(tree_dir=td, site_rates_dir=rates, contact_map_dir=cm, families=fams, amino_acids=AA,
                      pi_1_path=paths["p1"], Q_1_path=paths["Q1"], pi_2_path=paths["p2"], Q_2_path=paths["Q2"],
                      strategy="all_transitions", random_seed=0, output_msa_dir=msa)
        data = [_read_family(td, msa, rates, f, AA) for f in fams]
        chars = int(sum(c.size for _, c, _ in data))
        launches = int(sum(_launches(t) for t, _, _ in data)) + 2
        t0 = time.perf_counter()
        es = EStep([d[0] for d in data], [d[1] for d in data], [d[2] for d in data], grid)
        create_ms = (time.perf_counter() - t0) * 1e3
        kernel_ms, call_ms, mstep_ms = [], [], []
        with es:
            E, _ = es.expected_counts(Q, pi)   # warm-up
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                E, _ = es.expected_counts(Q, pi)
                call_ms.append((time.perf_counter() - t0) * 1e3)
                kernel_ms.append(es.last_kernel_ms)
        m_step(grid, E, Q, 500, 0.1, 0)   # warm-up
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            m_step(grid, E, Q, 500, 0.1, 0)
            mstep_ms.append((time.perf_counter() - t0) * 1e3)
        out = os.path.join(tmp, "em")
        t0 = time.perf_counter()
        em_lg(tree_dir=td, msa_dir=msa, site_rates_dir=rates, families=fams, initialization_rate_matrix_path=paths["Q1"],
              output_rate_matrix_dir=out, num_iterations=args.iterations, tolerance=-np.inf)
        em_wall = time.perf_counter() - t0
        n_it = len(open(os.path.join(out, "log_likelihoods.txt")).read().split()) - 1

    med = lambda x: float(np.median(x))  # noqa: E731
    rec = dict(
        what="em_lg E-step / M-step on the 32 demo families simulated under LG at the demo site rates, one MI355X",
        families=len(fams), node_characters=chars, grid_points=int(grid.size), estep_launches=launches,
        repeats=args.repeats, estep_create_ms=create_ms,
        estep_kernel_ms_median=med(kernel_ms), estep_kernel_ms=kernel_ms,
        estep_call_ms_median=med(call_ms), estep_call_ms=call_ms,
        mstep_500_epochs_ms_median=med(mstep_ms), mstep_ms=mstep_ms,
        em_lg_iterations=n_it, em_lg_wall_s=em_wall,
        em_lg_wall_per_iteration_s=em_wall / max(n_it, 1),
    )
    print(json.dumps(rec, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
