"""The topology search that `ml_nni_trees` (`_nni.py`) and `ml_spr_trees` (`_spr.py`, section 25) share:
the branch-length EM alternating with scan / select / apply of one kind of move, a candidate tree kept only if its likelihood at
the carried lengths is strictly higher.  `MoveKind` is what the two differ in; `search_trees` is the stage's body."""
import time
from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np

from ..io._tree import Tree
from ._ml_lengths import _batches, _read_stage_inputs, _StageInputs, _tree_at, _write_stage_outputs


class MoveKind(NamedTuple):
    stage: str        # the stage's name in its error messages
    log_ext: str      # <family><log_ext> is the family's log
    rounds_key: str   # the round counter's key in <family>.profiling
    # scan(fit, trees, want) -> (moves, delta, scan kernel ms): `trees` are the handle's, and a family not wanted gets no move
    scan: Callable
    select: Callable  # select(moves, delta, parent) -> the indices of the moves to apply
    apply: Callable   # apply(tree, moves, grid) -> the rearranged Tree


class HandleHooks:
    """What a stage adds to every handle of the search; the default adds nothing."""

    def on_handle(self, fit, fams: List[int], go: np.ndarray, ends: List[bool], prof: List[dict]) -> None:
        """inside the handle, after its scan.  fams: the families of the handle; go: whose tree on it is the input or an
        accepted candidate; ends: who ends on this tree at these lengths (no further round, or no move that gains)"""

    def on_accepted(self, k: int, f: int, tree: Tree, rnd: int) -> None:
        """after the handle, per family k of it (f of the stage) with go[k]: its tree at the fitted lengths, in its round rnd"""

    def finish(self, inp: _StageInputs, trees: List[Tree]) -> None:
        """after the search, before the final likelihoods: `trees` are the final ones"""


def search_trees(kind: MoveKind, num_search_rounds: int, num_rounds: int, max_bank_bytes: int, hooks: Optional[HandleHooks],
                 tree_dir: str, msa_dir: str, site_rates_dir: str, families: List[str], rate_matrix_path: str,
                 grid_args: Sequence, output_tree_dir: Optional[str], output_likelihood_dir: Optional[str]) -> None:
    """The body of `ml_nni_trees` and `ml_spr_trees`; their docstrings say what it does and writes."""
    from ._nni import _parent_array
    inp = _read_stage_inputs(kind.stage, "search", tree_dir, msa_dir, site_rates_dir, families, rate_matrix_path, grid_args,
                             output_tree_dir, output_likelihood_dir)
    hooks = hooks if hooks is not None else HandleHooks()
    F = len(families)
    trees = list(inp.trees)
    logs: List[List[str]] = [[] for _ in families]
    prof = [{"create_time": 0.0, "scan_time": 0.0, "scan_kernel_ms": 0.0, "fit_time": 0.0, "handles": 0, kind.rounds_key: 0,
             "moves_applied": 0} for _ in families]
    final_ll: List[Optional[float]] = [None] * F
    # Per family: rnd = its search round; trees[f] = the tree the next handle takes -- the input, or a candidate (fitted[f] with the
    # moves sel[f] applied) that has to beat before[f].  ONE handle per pass over the work list: on a candidate its
    # log_likelihoods() before any EM round decides (the lengths are the fitted ones: grid points snap to themselves), and the
    # accepted families go on in the same handle with the EM rounds and the scan of their next round.
    rnd = [0] * F
    before: List[Optional[float]] = [None] * F
    fitted: List[Optional[Tree]] = [None] * F
    sel: List[Optional[np.ndarray]] = [None] * F
    scanned, selected = [0] * F, [0] * F
    work = list(range(F))
    while work:
        nxt: List[int] = []
        for batch in _batches([inp.bank_bytes[f] for f in work], int(max_bank_bytes)):
            fams = [work[k] for k in batch]
            st = time.time()
            with inp.fitter(fams, [trees[f] for f in fams]) as fit:
                t_create = time.time() - st
                go = np.ones(len(fams), dtype=bool)            # the input tree, or an accepted candidate
                if any(before[f] is not None for f in fams):
                    _, ll0 = fit.log_likelihoods()
                    for k, f in enumerate(fams):
                        if before[f] is None:
                            continue
                        if ll0[k] > before[f]:
                            logs[f].append(f"{rnd[f]} {before[f]!r} {scanned[f]} {selected[f]} {len(sel[f])} {float(ll0[k])!r}\n")
                            prof[f]["moves_applied"] += len(sel[f])
                            rnd[f] += 1
                        else:
                            go[k] = False
                live = go.copy()                               # (a refused candidate's rounds are nobody's)
                for _ in range(int(num_rounds)):
                    if not live.any():
                        break
                    n_changed, _ = fit.round()
                    live &= n_changed > 0
                lengths = fit.lengths()
                _, fam_ll = fit.log_likelihoods()
                want = [bool(go[k]) and rnd[f] < int(num_search_rounds) for k, f in enumerate(fams)]
                st_scan = time.time()
                ms_scan = 0.0
                if any(want):
                    moves, delta, ms_scan = kind.scan(fit, [trees[f] for f in fams], want)
                t_scan = time.time() - st_scan
                picked = [moves[k][kind.select(moves[k], delta[k], _parent_array(trees[f]))] if want[k] else None
                          for k, f in enumerate(fams)]
                hooks.on_handle(fit, fams, go, [bool(go[k]) and (not want[k] or len(picked[k]) == 0) for k in range(len(fams))],
                                prof)
            for k, f in enumerate(fams):
                for key, x in (("create_time", t_create), ("scan_time", t_scan), ("scan_kernel_ms", ms_scan),
                               ("fit_time", time.time() - st)):
                    prof[f][key] += x / len(fams)              # (shares of the batch)
                prof[f]["handles"] += 1
                if not go[k]:                                  # refused: half of the moves, down to one, whose gain is exact
                    if len(sel[f]) > 1:
                        sel[f] = sel[f][:len(sel[f]) // 2]
                        trees[f] = kind.apply(fitted[f], sel[f], inp.grid)
                        nxt.append(f)
                    else:                                      # (rounding only)
                        logs[f].append(f"{rnd[f]} {before[f]!r} {scanned[f]} {selected[f]} 0 {before[f]!r}\n")
                        trees[f], final_ll[f] = fitted[f], before[f]
                    continue
                trees[f] = t = _tree_at(trees[f], lengths[k])
                ll = float(fam_ll[k])
                hooks.on_accepted(k, f, t, rnd[f])
                if not want[k]:                                # the topology of the last round's moves after its own EM rounds
                    final_ll[f] = ll
                    continue
                prof[f][kind.rounds_key] += 1
                s = picked[k]
                scanned[f], selected[f] = len(moves[k]), len(s)
                if len(s) == 0:                                # no move gains: finished
                    logs[f].append(f"{rnd[f]} {ll!r} {scanned[f]} 0 0 {ll!r}\n")
                    final_ll[f] = ll
                    continue
                fitted[f], before[f], sel[f] = t, ll, s
                trees[f] = kind.apply(t, s, inp.grid)
                nxt.append(f)
        work = nxt
    hooks.finish(inp, trees)
    for f in range(F):
        logs[f].append(f"final {final_ll[f]!r}\n")
    _write_stage_outputs(inp, trees, logs, kind.log_ext, prof)
