"""Time Felsenstein's bootstrap (`nj_bootstrap_supports`: csrc/boot.hip.h `boot_weights_kernel` / `boot_pairwise_kernel`, then the
join kernels of csrc/nj.hip.h, all in `cb_boot_nj`) on the `nj_trees` output of the 32 demo families
(tests/golden/demo32_co_inputs.npz alignments) under LG, with 100 replicates.  Reports the sum over the families of the kernel
time of the weight draws, of the distance kernel and of the joins (HIP events), and the wall time of the stage.

    python profiles/tools/time_boot.py [--baseline] [--num-replicates 100] [--out profiles/boot_demo32.json]

--baseline is what the library could do before `cb_boot_nj`, on the same site multiplicities (tests/boot_reference.py, not timed):
per family and replicate the resampled alignment is materialised (every column repeated by its multiplicity) and goes through
`pairwise_branch_lengths`; the replicates' matrices are joined in one `neighbor_joining_device_batch` call per family; the splits are
counted as the stage counts them.  It reports the wall time of the three parts and whether the supports equal the stage's.

--transfer times the transfer bootstrap (`nj_transfer_supports`: the same replicates, then csrc/transfer.hip.h `tb_sets_kernel` /
`tb_distance_kernel` in `cb_transfer_support`) beside `nj_bootstrap_supports` in the same run: wall seconds of both stages, the
kernel times, the launches.  With --baseline it also forms, for the family of the most leaves only, the distances in NumPy and
checks that the device's are equal.  (profiles/transfer_demo32.json)

--one FAMILY runs a single `bootstrap_nj_records` call on that family (after one warm-up call) and prints its kernel times: the
target of a counter collection (`rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES -- python profiles/tools/time_boot.py --one ...`).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
AA = list("ARNDCQEGHILKMFPSTWYV")
KEYS3 = ("output_tree_dir", "output_site_rates_dir", "output_likelihood_dir")
KERNELS = ("weights_kernel_ms", "distance_kernel_ms", "join_kernel_ms")


def family_inputs(tree_dir, msa_dir, rates_dir, family, Q, grid):
    """(tree, leaf names, seqs [n, L], bank, site_to_rate) as the stage forms them"""
    from cherryml_amd.counting._host import read_msa, read_site_rates
    from cherryml_amd.io import read_tree
    from cherryml_amd.phylogeny_estimation import compute_log_transition_matrices
    tree = read_tree(os.path.join(tree_dir, family + ".txt"))
    msa = read_msa(os.path.join(msa_dir, family + ".txt"))
    rates = np.asarray(read_site_rates(os.path.join(rates_dir, family + ".txt")), dtype=np.float64)
    names = tree.leaves()
    lut = np.full(256, -1, dtype=np.int8)
    lut[[ord(a) for a in AA]] = np.arange(20)
    seqs = lut[np.frombuffer("".join(msa[v] for v in names).encode("latin-1"), dtype=np.uint8)].reshape(len(names), len(rates))
    unique_rates, s2r = np.unique(rates, return_inverse=True)
    return tree, names, seqs, compute_log_transition_matrices(Q, grid, unique_rates), s2r.astype(np.int32)


TRANSFER_KERNELS = KERNELS + ("transfer_sets_kernel_ms", "transfer_distance_kernel_ms")


def numpy_transfer_distances(rows, n, joins, block=16):
    """delta [n_ref, n_rep] of `cb_transfer_support` in NumPy, no packed sets: the replicates' leaf sets as 0 / 1 rows from the
    join records, h = |A| + |S| - 2 A.S as a float32 product (counts below 2^24 are exact), the minimum over both sides and the
    sets, the clamp p - 1; `block` replicates a product"""
    A = np.unpackbits(rows, axis=1)[:, :n].astype(np.float32)
    size = A.sum(axis=1)
    clamp = np.minimum(size, n - size) - 1
    out = np.zeros((len(rows), len(joins)), dtype=np.int32)
    for b0 in range(0, len(joins), block):
        part = joins[b0:b0 + block]
        sets = np.zeros((len(part), 2 * n - 3, n), dtype=np.float32)
        sets[:, np.arange(n), np.arange(n)] = 1.0
        for q in range(n - 3):
            k = np.arange(len(part))
            sets[:, n + q] = np.maximum(sets[k, part[:, q, 0]], sets[k, part[:, q, 1]])
        S = sets[:, n:].reshape(-1, n)
        h = size[:, None] + S.sum(axis=1)[None, :] - 2.0 * (A @ S.T)
        d = np.minimum(h, n - h).reshape(len(rows), len(part), n - 3).min(axis=2)
        out[:, b0:b0 + block] = np.minimum(d, clamp[:, None]).astype(np.int32)
    return out


def time_transfer(args, tmp, kw, inputs, grid):
    """--transfer: `nj_transfer_supports` beside `nj_bootstrap_supports` in the same run (each called twice, the second call
    reported), the kernel times of both from the .profiling files; --baseline: on the family of the most leaves the distances in
    NumPy (`numpy_transfer_distances`) against the device's, and the time of both"""
    from cherryml_amd import nj_bootstrap_supports, nj_transfer_supports
    from cherryml_amd.io import read_tree
    from cherryml_amd.phylogeny_estimation import (bootstrap_nj_records, read_bootstrap_supports, read_transfer_supports,
                                                   transfer_distances, tree_splits)
    from cherryml_amd.phylogeny_estimation._supports import support_seeds
    fams, B = kw["families"], kw["num_replicates"]
    rec = dict(what="nj_transfer_supports beside nj_bootstrap_supports on the nj_trees output of the 32 demo families under LG, one "
                    "MI355X: wall seconds of two calls each, kernel milliseconds summed over the families (second call)",
               families=len(fams), replicates=B)
    for stage, name, keys in ((nj_bootstrap_supports, "bootstrap", KERNELS), (nj_transfer_supports, "transfer", TRANSFER_KERNELS)):
        walls = []
        for i in range(2):
            out_dir = os.path.join(tmp, f"{name}{i}")
            t0 = time.perf_counter()
            stage(output_support_dir=out_dir, **kw)
            walls.append(time.perf_counter() - t0)
        sums = dict.fromkeys(keys + ("bank_time", "total_time"), 0.0)
        for fam in fams:
            for ln in open(os.path.join(out_dir, fam + ".profiling")).read().split("\n"):
                k, v = ln.split(": ")
                sums[k] += float(v)
        rec[name] = dict(stage_wall_s=walls, kernel_ms={k: sums[k] for k in keys}, bank_s=sums["bank_time"])
    both = [(read_bootstrap_supports(os.path.join(tmp, "bootstrap1", fam + ".txt")),
             read_transfer_supports(os.path.join(tmp, "transfer1", fam + ".txt"))) for fam in fams]
    rec["bootstrap_columns_equal"] = all({k: v[0] for k, v in t.items()} == s for s, t in both)
    share = np.array([v[0] for _, t in both for v in t.values()])
    tbe = np.array([v[1] for _, t in both for v in t.values()])
    rec["edges"] = int(len(share))
    rec["mean_bootstrap"], rec["mean_transfer"] = float(share.mean()), float(tbe.mean())
    rec["edges_bootstrap_below_0.7_transfer_at_least_0.7"] = int(((share < 0.7) & (tbe >= 0.7)).sum())
    rec["transfer_over_bootstrap_wall_s"] = rec["transfer"]["stage_wall_s"][1] - rec["bootstrap"]["stage_wall_s"][1]
    leaves = {fam: len(read_tree(os.path.join(kw["tree_dir"], fam + ".txt")).leaves()) for fam in fams}
    rec["leaves"] = [leaves[fam] for fam in fams]
    # two launches per chunk of replicates; a chunk holds 512 MiB of leaf sets, (n - 3) rows of ceil(n / 64) words a replicate
    per = {fam: max((512 << 20) // max((n - 3) * ((n + 63) // 64) * 8, 1), 1) for fam, n in leaves.items()}
    rec["transfer_launches"] = int(sum(2 * -(-B // per[fam]) for fam in fams if leaves[fam] >= 4))
    rec["xor_popcount_words"] = float(sum((n - 3) ** 2 * B * ((n + 63) // 64) for n in leaves.values()))
    if args.baseline:
        fam = max(fams, key=lambda f: leaves[f])
        seed = dict(zip(fams, support_seeds(fams, 0)))[fam]
        tree, names, seqs, bank, s2r = inputs(fam)
        records = bootstrap_nj_records(seqs, bank, s2r, grid, B, seed)
        joins = np.stack([np.asarray(r[0], dtype=np.int32) for r in records])
        rows, n = tree_splits(tree, names), len(names)
        prof = {}
        t0 = time.perf_counter()
        _, _, got = transfer_distances(rows, n, joins, profile=prof, per_replicate=True)
        t1 = time.perf_counter()
        want = numpy_transfer_distances(rows, n, joins)
        t2 = time.perf_counter()
        rec["baseline"] = dict(what="one family: the distances of all its splits to all replicates, cb_transfer_support against NumPy "
                                    "(float32 products for the Hamming distances, 16 host threads)", family=fam, leaves=n,
                               reference_splits=int(len(rows)), replicates=B, device_call_s=t1 - t0, numpy_s=t2 - t1,
                               equal=bool(np.array_equal(got, want)), **prof)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-rate-categories", type=int, default=20)
    ap.add_argument("--num-replicates", type=int, default=100)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--transfer", action="store_true")
    ap.add_argument("--one", default=None, metavar="FAMILY")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from conftest import load_golden
    from time_nj import _msas

    from cherryml_amd import nj_bootstrap_supports, nj_trees
    from cherryml_amd.io import write_rate_matrix
    from cherryml_amd.phylogeny_estimation import (bootstrap_nj_records, neighbor_joining_device_batch, pairwise_branch_lengths,
                                                   read_bootstrap_supports, supports_of_records)
    from cherryml_amd.phylogeny_estimation._fast_cherries import quantization_points_ble
    from cherryml_amd.phylogeny_estimation._supports import support_seeds
    fams, texts = _msas()
    Q = np.ascontiguousarray(load_golden("likelihood.npz")["lg"], dtype=np.float64)
    grid = np.array(quantization_points_ble(0.03, 1.1, 64))
    B = args.num_replicates
    with tempfile.TemporaryDirectory() as tmp:
        msa = os.path.join(tmp, "msa")
        os.makedirs(msa)
        for fam, text in zip(fams, texts):
            with open(os.path.join(msa, fam + ".txt"), "wb") as f:
                f.write(text)
        qpath = os.path.join(tmp, "lg.txt")
        write_rate_matrix(Q, AA, qpath)
        if args.one:
            fams = [args.one]
        nj = nj_trees(msa_dir=msa, families=fams, rate_matrix_path=qpath, num_rate_categories=args.num_rate_categories,
                      **{k: os.path.join(tmp, "nj_" + k) for k in KEYS3}) or {k: os.path.join(tmp, "nj_" + k) for k in KEYS3}
        if args.one:
            tree, names, seqs, bank, s2r = family_inputs(nj["output_tree_dir"], msa, nj["output_site_rates_dir"], args.one, Q, grid)
            for _ in range(2):
                prof = {}
                records = bootstrap_nj_records(seqs, bank, s2r, grid, B, 1, profile=prof)
            if args.transfer:                                  # (with --transfer: three calls of the distances on the records)
                from cherryml_amd.phylogeny_estimation import transfer_distances, tree_splits
                joins = np.stack([np.asarray(r[0], dtype=np.int32) for r in records])
                for _ in range(3):
                    prof = {}
                    transfer_distances(tree_splits(tree, names), len(names), joins, profile=prof)
            print(json.dumps(dict(family=args.one, leaves=int(seqs.shape[0]), sites=int(seqs.shape[1]), replicates=B,
                                  grid_points=len(grid), rate_categories=int(bank.shape[1]), **prof)))
            return
        kw = dict(tree_dir=nj["output_tree_dir"], msa_dir=msa, site_rates_dir=nj["output_site_rates_dir"], families=fams,
                  rate_matrix_path=qpath, num_replicates=B)
        if args.transfer:
            rec = time_transfer(args, tmp, kw, lambda fam: family_inputs(nj["output_tree_dir"], msa, nj["output_site_rates_dir"],
                                                                          fam, Q, grid), grid)
            print(json.dumps(rec, indent=1))
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(rec, f, indent=1)
                    f.write("\n")
            return
        walls, sums = [], None
        for i in range(2):                                     # (the first call pays the first use of the device)
            sup_dir = os.path.join(tmp, f"sup{i}")
            t0 = time.perf_counter()
            nj_bootstrap_supports(output_support_dir=sup_dir, **kw)
            walls.append(time.perf_counter() - t0)
            sums = dict.fromkeys(KERNELS + ("bank_time", "total_time"), 0.0)
            for fam in fams:
                for ln in open(os.path.join(sup_dir, fam + ".profiling")).read().split("\n"):
                    k, v = ln.split(": ")
                    sums[k] += float(v)
        stage_supports = {fam: read_bootstrap_supports(os.path.join(sup_dir, fam + ".txt")) for fam in fams}
        sizes = []
        base = dict(materialise_s=0.0, pairwise_s=0.0, pairwise_kernel_ms=0.0, join_s=0.0, join_kernel_ms=0.0, splits_s=0.0)
        equal = True
        for fam, seed in zip(fams, support_seeds(fams, 0)):
            tree, names, seqs, bank, s2r = family_inputs(nj["output_tree_dir"], msa, nj["output_site_rates_dir"], fam, Q, grid)
            sizes.append([int(seqs.shape[0]), int(seqs.shape[1])])
            if not args.baseline:
                continue
            import boot_reference
            W = boot_reference.weights(seqs.shape[1], B, seed)
            Ds = []
            for b in range(B):
                t0 = time.perf_counter()
                cols = np.repeat(np.arange(seqs.shape[1]), W[b])
                resampled, rates_b = np.ascontiguousarray(seqs[:, cols]), np.ascontiguousarray(s2r[cols])
                t1 = time.perf_counter()
                prof = {}
                index = pairwise_branch_lengths(resampled, bank, rates_b, profile=prof)
                D = grid[np.maximum(index, 0)]
                np.fill_diagonal(D, 0.0)
                Ds.append(D)
                base["materialise_s"] += t1 - t0
                base["pairwise_s"] += time.perf_counter() - t1
                base["pairwise_kernel_ms"] += prof["kernel_ms"]
            t0 = time.perf_counter()
            prof = {}
            neighbor_joining_device_batch(Ds, [names] * B, min_length=float(grid[0]), profile=prof)
            from cherryml_amd.phylogeny_estimation import nj_join_records
            t1 = time.perf_counter()
            base["join_s"] += t1 - t0
            base["join_kernel_ms"] += prof["kernel_ms"]
            records = nj_join_records(Ds, zero_diagonal=True)      # (the records the trees above were built from: not timed)
            t0 = time.perf_counter()
            nodes, support = supports_of_records(tree, names, records)
            base["splits_s"] += time.perf_counter() - t0
            got = {tree.nodes()[int(v)]: float(s) for v, s in zip(nodes, support)}
            equal = equal and got == stage_supports[fam]
    pairs = int(sum(n * (n - 1) // 2 for n, _ in sizes))
    rec = dict(what="nj_bootstrap_supports on the nj_trees output of the 32 demo families under LG, one MI355X: kernel milliseconds "
                    "summed over the families (second call), wall seconds of both calls",
               families=len(fams), leaves_sites=sizes, sequence_pairs=pairs, replicates=B, grid_points=len(grid),
               product_flops=2.0 * B * len(grid) * float(sum(n * (n - 1) // 2 * L for n, L in sizes)),
               kernel_ms={k: sums[k] for k in KERNELS}, bank_s=sums["bank_time"], stage_wall_s=walls)
    if args.baseline:
        base["wall_s"] = base["materialise_s"] + base["pairwise_s"] + base["join_s"] + base["splits_s"]
        rec["baseline"] = dict(what="per family and replicate: the resampled alignment materialised, pairwise_branch_lengths, then one "
                                    "neighbor_joining_device_batch call per family and the stage's split count", **base,
                               supports_equal_the_stages=equal,
                               distance_speedup_kernel=base["pairwise_kernel_ms"] / sums["distance_kernel_ms"],
                               wall_speedup=base["wall_s"] / walls[1])
    print(json.dumps(rec, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
