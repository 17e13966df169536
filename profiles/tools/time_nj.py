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

`--joiner device` times the stage with neighbour joining on the host and on the device (csrc/nj.hip.h, `cb_nj_batch`) side by
side, and the batched device call alone with its kernel time and launches; it writes profiles/njd_demo32.json.

    python profiles/tools/time_nj.py --joiner device [--repeats 2] [--out profiles/njd_demo32.json]
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


def device_joiner(args):
    """`nj_trees` on the 32 demo families with joiner="host" and joiner="device", alternating, `--repeats` rounds after one
    warm-up round: wall time of the whole call and the neighbour-joining share (the sum of `nj_time` over the families);
    then `neighbor_joining_device_batch` alone on the same 32 distance matrices: its wall time, the kernel time of the join
    launches by HIP events, and the launches (three per join of the largest family of a chunk)."""
    from conftest import load_golden

    from cherryml_amd import neighbor_joining_device_batch, nj_trees
    from cherryml_amd.io import write_rate_matrix
    from cherryml_amd.phylogeny_estimation import compute_log_transition_matrices, rate_categories_ble
    from cherryml_amd.phylogeny_estimation._fast_cherries import _read_msa_file, quantization_points_ble
    from cherryml_amd.phylogeny_estimation._nj import _family_distances
    fams, texts = _msas()
    Q = np.ascontiguousarray(load_golden("likelihood.npz")["lg"], dtype=np.float64)
    walls, shares = {"host": [], "device": []}, {"host": [], "device": []}
    with tempfile.TemporaryDirectory() as tmp:
        msa = os.path.join(tmp, "msa")
        os.makedirs(msa)
        for fam, text in zip(fams, texts):
            with open(os.path.join(msa, fam + ".txt"), "wb") as f:
                f.write(text)
        qpath = os.path.join(tmp, "lg.txt")
        write_rate_matrix(Q, AA, qpath)
        for rep in range(args.repeats + 1):                # the first round is the warm-up
            for joiner in ("host", "device"):
                out = {k: os.path.join(tmp, f"{k}_{joiner}_{rep}") for k in ("output_tree_dir", "output_site_rates_dir",
                                                                            "output_likelihood_dir")}
                t0 = time.perf_counter()
                nj_trees(msa_dir=msa, families=fams, rate_matrix_path=qpath, num_rate_categories=args.num_rate_categories,
                         joiner=joiner, **out)
                wall = time.perf_counter() - t0
                nj = 0.0
                for fam in fams:
                    prof = dict(ln.split(": ") for ln in open(os.path.join(out["output_tree_dir"], fam + ".profiling")).read().split("\n"))
                    nj += float(prof["nj_time"])
                if rep:
                    walls[joiner].append(wall), shares[joiner].append(nj)
        grid = quantization_points_ble(0.03, 1.1, 64)
        logP = compute_log_transition_matrices(Q, grid, rate_categories_ble(args.num_rate_categories))
        Ds, names_list = [], []
        for fam in fams:
            names, sequences = _read_msa_file(os.path.join(msa, fam + ".txt"))
            D, _, _ = _family_distances(names, sequences, Q, AA, args.num_rate_categories, 50, 1234, 0.03, 1.1, 64, 0, None, logP)
            Ds.append(D), names_list.append(names)
    batch_wall, kernel_ms = [], []
    for rep in range(args.repeats + 1):
        prof = {}
        t0 = time.perf_counter()
        neighbor_joining_device_batch(Ds, names_list, min_length=float(grid[0]), profile=prof)
        if rep:
            batch_wall.append(time.perf_counter() - t0), kernel_ms.append(prof["kernel_ms"])
    sizes = [len(v) for v in names_list]
    matrix_bytes = int(sum(8 * n * n for n in sizes))
    med = lambda v: float(np.median(v))                    # noqa: E731
    return dict(what="nj_trees on the 32 demo families under LG, one MI355X, neighbour joining on the host (NumPy) and on the "
                     "device (cb_nj_batch): seconds, medians over the repeats after one warm-up round",
                families=len(fams), leaves=sizes, rate_categories=args.num_rate_categories, repeats=args.repeats,
                host=dict(stage_wall_s=walls["host"], nj_s=shares["host"], stage_wall_s_median=med(walls["host"]),
                          nj_s_median=med(shares["host"])),
                device=dict(stage_wall_s=walls["device"], nj_s=shares["device"], stage_wall_s_median=med(walls["device"]),
                            nj_s_median=med(shares["device"]), batch_call_s=batch_wall, batch_call_s_median=med(batch_wall),
                            kernel_ms=kernel_ms, kernel_ms_median=med(kernel_ms), matrix_bytes=matrix_bytes,
                            chunks=1 if matrix_bytes <= 512 << 20 else None, launches=3 * (max(sizes) - 3)),
                stage_speedup=med(walls["host"]) / med(walls["device"]), nj_speedup=med(shares["host"]) / med(shares["device"]))


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
    ap.add_argument("--joiner", choices=("host", "device"), default="host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.joiner == "device":
        if args.baseline:
            ap.error("--baseline times the distance pass; it takes no --joiner device")
        args.out = args.out or os.path.join(ROOT, "profiles", "njd_demo32.json")
        rec, key = device_joiner(args), "joiner"
    else:
        rec, key = (baseline(args), "baseline") if args.baseline else (stage(args), "stage")
    print(json.dumps(rec, indent=1))
    if args.out:
        old = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f)
        old[key] = rec
        with open(args.out, "w") as f:
            json.dump(old, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
