"""Time `simulate_msas` on the 32 demo families (tests/golden/demo32_co_inputs.npz: trees and contact maps, maximal
matchings of the contacts at distance >= 7; site rates tests/golden/simulation/demo_site_rates) under LG and the 400-state
product chain LG x I + I x LG.  Reports the kernel time of one batch (cb_sim_model_run, all 32 families in one launch), the
wall time of the whole `simulate_msas` call and the share of it spent writing the files; and, for scale, the test's NumPy
restatement of the same stream (tests/sim_stream.py) on one family.  That restatement is a correctness model, not a tuned
CPU simulator: the comparison only says how far a vectorised host loop is from the kernel.

    python profiles/tools/time_simulate.py [--repeats N] [--out profiles/simulate_demo32.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from conftest import load_golden

    import sim_stream
    from cherryml_amd import _lib, simulate_msas
    from cherryml_amd.estimation_end_to_end import create_maximal_matching_contact_map
    from cherryml_amd.io import write_probability_distribution, write_rate_matrix
    from cherryml_amd.simulation import Simulator, family_seed
    from cherryml_amd.simulation import _simulate

    z = load_golden("demo32_co_inputs.npz")
    fams = [str(f) for f in z["families"]]
    lk = load_golden("likelihood.npz")
    Q, pi = lk["lg"], lk["pi_lg"]
    I = np.eye(20)
    Q2, pi2 = np.kron(Q, I) + np.kron(I, Q), np.kron(pi, pi)
    pairs = [a + b for a in AA for b in AA]
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {}
        for kind in ("tree", "contact_map"):
            d = os.path.join(tmp, kind)
            os.makedirs(d)
            off, blob = z[f"{kind}_offsets"], z[f"{kind}_bytes"].tobytes()
            for k, fam in enumerate(fams):
                with open(os.path.join(d, fam + ".txt"), "wb") as f:
                    f.write(blob[off[k]:off[k + 1]])
            dirs[kind] = d
        cm = os.path.join(tmp, "matched")
        create_maximal_matching_contact_map(i_contact_map_dir=dirs["contact_map"], families=fams,
                                            minimum_distance_for_nontrivial_contact=7, num_processes=1, o_contact_map_dir=cm)
        rates = os.path.join(ROOT, "tests", "golden", "simulation", "demo_site_rates")
        paths = {k: os.path.join(tmp, k + ".txt") for k in ("Q1", "Q2", "p1", "p2")}
        write_rate_matrix(Q, AA, paths["Q1"])
        write_rate_matrix(Q2, pairs, paths["Q2"])
        write_probability_distribution(pi, AA, paths["p1"])
        write_probability_distribution(pi2, pairs, paths["p2"])
        kw = dict(tree_dir=dirs["tree"], site_rates_dir=rates, contact_map_dir=cm, families=fams, amino_acids=AA,
                  pi_1_path=paths["p1"], Q_1_path=paths["Q1"], pi_2_path=paths["p2"], Q_2_path=paths["Q2"],
                  strategy="all_transitions", random_seed=0)

        fam_data = [_simulate._read_family(dirs["tree"], rates, cm, f, family_seed(f, 0)) for f in fams]
        n_chars = int(sum(len(f["parent"]) * f["n_sites"] for f in fam_data))
        n_units = int(sum(len(f["site_a"]) for f in fam_data))
        n_pairs = int(sum((f["site_b"] >= 0).sum() for f in fam_data))
        kernel_ms, run_ms = [], []
        with Simulator(Q, pi, Q2, pi2) as sim:
            sim.run(fam_data)   # warm-up
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                sim.run(fam_data)
                run_ms.append((time.perf_counter() - t0) * 1e3)
                kernel_ms.append(sim.last_kernel_ms)

        # the whole call, and the part of it spent in _write_family
        write_s = [0.0]
        orig = _simulate._write_family

        def timed(*a, **k):
            t0 = time.perf_counter()
            orig(*a, **k)
            write_s[0] += time.perf_counter() - t0
        _simulate._write_family = timed
        wall_ms, write_ms = [], []
        try:
            for r in range(args.repeats):
                write_s[0] = 0.0
                t0 = time.perf_counter()
                simulate_msas(output_msa_dir=os.path.join(tmp, f"out{r}"), **kw)
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                write_ms.append(write_s[0] * 1e3)
        finally:
            _simulate._write_family = orig

        lib = _lib.load()
        t1, t2 = sim_stream.model_tables(lib, Q, pi), sim_stream.model_tables(lib, Q2, pi2)
        t0 = time.perf_counter()
        sim_stream.simulate_family(t1, t2, 20, fam_data[0])
        numpy_ms = (time.perf_counter() - t0) * 1e3

    med = lambda x: float(np.median(x))  # noqa: E731
    rec = dict(
        what="simulate_msas on the 32 demo families, LG + LG x I + I x LG, one MI355X",
        families=len(fams), characters=n_chars, units=n_units, pair_units=n_pairs, repeats=args.repeats,
        kernel_ms_median=med(kernel_ms), kernel_ms=kernel_ms,
        run_ms_median=med(run_ms), run_ms=run_ms,
        wall_ms_median=med(wall_ms), wall_ms=wall_ms,
        write_ms_median=med(write_ms), write_share=med(write_ms) / med(wall_ms),
        numpy_restatement_one_family_ms=numpy_ms, numpy_restatement_family=fams[0],
        numpy_restatement_family_characters=int(len(fam_data[0]["parent"]) * fam_data[0]["n_sites"]),
    )
    print(json.dumps(rec, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
