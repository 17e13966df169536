"""Time full-tree estimation (`nj_trees`: csrc/ble.hip.h `ble_pairwise_kernel` + neighbour joining on the host) on the 32 demo
families (tests/golden/demo32_co_inputs.npz alignments) under LG.  Reports per stage the sum over the families: FastCherries'
pairing and coordinate ascent, the pairwise distance pass (the kernel alone by HIP events, and the whole call with its uploads
and the n^2 read-back), neighbour joining, the likelihood of the trees, and the wall time of the stage.

`--baseline` times ONE family (default 1a4p_1_A, 1024 x 92) two ways at the same site rates: `pairwise_branch_lengths`, and the
only route to the same indices without it -- `branch_lengths` on the materialised arrays seqs[I], seqs[J] of all pairs.  The
indices are compared.  `branch_lengths` reports no device time: run this mode under `rocprofv3 --kernel-trace --stats` for the two
kernels' times side by side (`ble_pairwise_kernel`, `ble_branch_lengths_kernel`).

    python profiles/tools/time_nj.py [--out profiles/nj_demo32.json]
    python profiles/tools/time_nj.py --baseline [--family 1a4p_1_A] [--repeats 3] [--out ...]
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


def _msas():
    from conftest import load_golden
    z = load_golden("demo32_co_inputs.npz")
    off, blob = z["msa_offsets"], z["msa_bytes"].tobytes()
    return [str(f) for f in z["families"]], [blob[off[k]:off[k + 1]] for k in range(len(z["families"]))]


def baseline(args):
    from conftest import load_golden

    from cherryml_amd.phylogeny_estimation import branch_lengths, compute_log_transition_matrices, nj_distance_indices, \
        pairwise_branch_lengths, rate_categories_ble
    from cherryml_amd.phylogeny_estimation._fast_cherries import _encode_and_pair, quantization_points_ble
    fams, texts = _msas()
    lines = texts[fams.index(args.family)].decode().split("\n")
    sequences = [lines[i + 1] for i, ln in enumerate(lines) if ln.startswith(">")]
    Q = load_golden("likelihood.npz")["lg"]
    seqs, pairs = _encode_and_pair(sequences, AA, 1234, "lemire")
    n, L = seqs.shape
    grid, rates = quantization_points_ble(0.03, 1.1, 64), rate_categories_ble(args.num_rate_categories)
    logP = compute_log_transition_matrices(Q, grid, rates)
    _, _, s2r, _, _ = nj_distance_indices(seqs, pairs, Q, num_rate_categories=args.num_rate_categories, log_transition_matrices=logP)
    I, J = np.triu_indices(n, 1)
    new_ms, new_wall, old_wall = [], [], []
    for rep in range(args.repeats + 1):                    # alternating; the first round is the warm-up
        prof = {}
        t0 = time.perf_counter()
        index = pairwise_branch_lengths(seqs, logP, s2r, profile=prof)
        t1 = time.perf_counter()
        cherry = branch_lengths(seqs[I], seqs[J], logP, s2r)
        t2 = time.perf_counter()
        if rep:
            new_ms.append(prof["kernel_ms"]), new_wall.append((t1 - t0) * 1e3), old_wall.append((t2 - t1) * 1e3)
    same = bool(np.array_equal(index[I, J], cherry))
    return dict(what=f"all-pairs branch-length indices of {args.family} ({n} x {L}, {len(I)} pairs, {len(rates)} rate categories): "
                     "pairwise_branch_lengths against branch_lengths on the materialised pairs, one MI355X",
                pairs=int(len(I)), sites=int(L), indices_equal=same, repeats=args.repeats,
                pairwise_kernel_ms=new_ms, pairwise_call_ms=new_wall, materialised_call_ms=old_wall,
                pairwise_kernel_ms_median=float(np.median(new_ms)), pairwise_call_ms_median=float(np.median(new_wall)),
                materialised_call_ms_median=float(np.median(old_wall)),
                sequence_bytes_on_device=dict(pairwise=int(n * L), materialised=int(2 * len(I) * L)))


def stage(args):
    from conftest import load_golden

    from cherryml_amd import nj_trees
    from cherryml_amd.io import write_rate_matrix
    fams, texts = _msas()
    Q = load_golden("likelihood.npz")["lg"]
    keys = ("pairing_time", "ble_time", "distance_time", "nj_time", "likelihood_time", "total_time")
    with tempfile.TemporaryDirectory() as tmp:
        msa = os.path.join(tmp, "msa")
        os.makedirs(msa)
        for fam, text in zip(fams, texts):
            with open(os.path.join(msa, fam + ".txt"), "wb") as f:
                f.write(text)
        qpath = os.path.join(tmp, "lg.txt")
        write_rate_matrix(Q, AA, qpath)
        walls, sums = [], None
        for rep in range(args.repeats):                    # (seconds per round: no warm-up round)
            out = {k: os.path.join(tmp, f"{k}_{rep}") for k in ("output_tree_dir", "output_site_rates_dir", "output_likelihood_dir")}
            t0 = time.perf_counter()
            nj_trees(msa_dir=msa, families=fams, rate_matrix_path=qpath, num_rate_categories=args.num_rate_categories, **out)
            walls.append(time.perf_counter() - t0)
            sums = dict.fromkeys(keys, 0.0)
            for fam in fams:
                for ln in open(os.path.join(out["output_tree_dir"], fam + ".profiling")).read().split("\n"):
                    k, v = ln.split(": ")
                    sums[k] += float(v)
            lls = [float(open(os.path.join(out["output_likelihood_dir"], fam + ".txt")).readline()) for fam in fams]
    # the kernel alone, family by family (HIP events)
    from cherryml_amd.phylogeny_estimation import nj_distance_indices
    from cherryml_amd.phylogeny_estimation._fast_cherries import _encode_and_pair
    kernel_ms, pairs_total = 0.0, 0
    for text in texts:
        lines = text.decode().split("\n")
        sequences = [lines[i + 1] for i, ln in enumerate(lines) if ln.startswith(">")]
        seqs, pairs = _encode_and_pair(sequences, AA, 1234, "lemire")
        prof = {}
        nj_distance_indices(seqs, pairs, Q, num_rate_categories=args.num_rate_categories, profile=prof)
        kernel_ms += prof["kernel_ms"]
        pairs_total += seqs.shape[0] * (seqs.shape[0] - 1) // 2
    return dict(what="nj_trees on the 32 demo families under LG, one MI355X: seconds summed over the families (last repeat)",
                families=len(fams), sequence_pairs=int(pairs_total), rate_categories=args.num_rate_categories, repeats=args.repeats,
                pairwise_kernel_ms_total=kernel_ms, stage_seconds={k: sums[k] for k in keys}, stage_wall_s=walls,
                stage_wall_s_median=float(np.median(walls)), total_log_likelihood=float(sum(lls)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--family", default="1a4p_1_A")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--num-rate-categories", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = baseline(args) if args.baseline else stage(args)
    print(json.dumps(rec, indent=1))
    if args.out:
        old = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f)
        old["baseline" if args.baseline else "stage"] = rec
        with open(args.out, "w") as f:
            json.dump(old, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
