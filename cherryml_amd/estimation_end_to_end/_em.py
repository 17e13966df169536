"""`lg_end_to_end_with_em_optimizer` (reference: cherryml/estimation_end_to_end/_em.py:33-200): tree estimation, the JTT-IPW
initialisation from cherry counts, then full-tree EM -- here `estimation.em_lg` with its E-step on the GPU.  The reference's
backends are external programs (XRATE, Historian); only `em_backend="gpu"` is accepted."""
import os
from typing import Callable, Dict, List, Optional

from ..counting import count_transitions
from ..estimation import em_lg, jtt_ipw
from ._cherry import AMINO_ACIDS, _grid, _need_cache, _runtime


def lg_end_to_end_with_em_optimizer(
    msa_dir: str,
    families: List[str],
    tree_estimator: Optional[Callable],
    initial_tree_estimator_rate_matrix_path: Optional[str],
    num_iterations: Optional[int] = 1,
    quantization_grid_center: float = 0.03,
    quantization_grid_step: float = 1.1,
    quantization_grid_num_steps: int = 64,
    use_cpp_counting_implementation: bool = True,
    extra_em_command_line_args: str = "-log 6 -f 3 -mi 0.000001",
    cpp_counting_command_line_prefix: str = "",
    cpp_counting_command_line_suffix: str = "",
    num_processes_tree_estimation: int = 8,
    num_processes_counting: int = 8,
    num_processes_optimization: int = 2,
    optimizer_initialization: str = "jtt-ipw",
    sites_subset_dir: Optional[str] = None,
    em_backend: str = "gpu",
    tree_dir: Optional[str] = None,
    site_rates_dir: Optional[str] = None,
    em_iterations: int = 20,
) -> Dict:
    """The reference's keyword signature.  `extra_em_command_line_args` (the binaries' flags) is accepted and ignored;
    `tree_dir` / `site_rates_dir` (both or neither) stand in for the tree estimator on the first iteration, as in
    `lg_end_to_end_with_cherryml_optimizer`; `em_iterations` is em_lg's `num_iterations`."""
    if em_backend in ("xrate", "historian"):
        raise ValueError(f"em_backend={em_backend!r} runs the external XRATE / Historian binaries, which this package does not "
                         "ship or call; use em_backend='gpu'")
    if em_backend != "gpu":
        raise ValueError(f"Unknown EM backend: {em_backend}. Allowed: 'gpu'.")
    _need_cache()
    if sites_subset_dir is not None:
        raise NotImplementedError("sites_subset_dir is not supported by this build")
    if (tree_dir is None) != (site_rates_dir is None):
        raise ValueError("tree_dir and site_rates_dir must be either both provided or none provided")
    res: Dict = {}
    quantization_points = _grid(quantization_grid_center, quantization_grid_step, quantization_grid_num_steps)
    res["quantization_points"] = quantization_points
    t_count = t_jtt = t_opt = 0.0
    current = initial_tree_estimator_rate_matrix_path
    for iteration in range(num_iterations):
        if iteration == 0 and tree_dir is not None:
            dirs = {"output_tree_dir": tree_dir, "output_site_rates_dir": site_rates_dir}
        elif tree_estimator is None:
            raise NotImplementedError("provide tree_dir and site_rates_dir, or a tree_estimator callable")
        else:
            dirs = tree_estimator(msa_dir=msa_dir, families=families, rate_matrix_path=current,
                                  num_processes=num_processes_tree_estimation)
        res[f"tree_estimator_output_dirs_{iteration}"] = dirs
        count_dir = count_transitions(
            tree_dir=dirs["output_tree_dir"], msa_dir=msa_dir, site_rates_dir=dirs["output_site_rates_dir"],
            families=families, amino_acids=AMINO_ACIDS[:], quantization_points=quantization_points, edge_or_cherry="cherry",
            num_processes=num_processes_counting, use_cpp_implementation=use_cpp_counting_implementation,
            cpp_command_line_prefix=cpp_counting_command_line_prefix,
            cpp_command_line_suffix=cpp_counting_command_line_suffix)["output_count_matrices_dir"]
        res[f"count_matrices_dir_{iteration}"] = count_dir
        t_count += _runtime(os.path.join(count_dir, "profiling.txt"))
        jtt_dir = jtt_ipw(count_matrices_path=os.path.join(count_dir, "result.txt"), mask_path=None, use_ipw=True,
                          normalize=False)["output_rate_matrix_dir"]
        res[f"jtt_ipw_dir_{iteration}"] = jtt_dir
        t_jtt += _runtime(os.path.join(jtt_dir, "profiling.txt"))
        if optimizer_initialization == "jtt-ipw":
            init_path = os.path.join(jtt_dir, "result.txt")
        elif optimizer_initialization.endswith(".txt"):
            init_path = optimizer_initialization
        else:
            raise ValueError(f"Unknown optimizer_initialization = {optimizer_initialization}")
        rate_dir = em_lg(tree_dir=dirs["output_tree_dir"], msa_dir=msa_dir, site_rates_dir=dirs["output_site_rates_dir"],
                         families=families, initialization_rate_matrix_path=init_path,
                         quantization_points=[float(q) for q in quantization_points],
                         num_iterations=em_iterations)["output_rate_matrix_dir"]
        t_opt += _runtime(os.path.join(rate_dir, "profiling.txt"))
        res[f"rate_matrix_dir_{iteration}"] = rate_dir
        current = os.path.join(rate_dir, "result.txt")
    res["learned_rate_matrix_path"] = current
    res["time_tree_estimation"] = 0.0
    res["time_counting"], res["time_jtt_ipw"], res["time_optimization"] = t_count, t_jtt, t_opt
    res["total_cpu_time"] = t_count + t_jtt + t_opt
    res["profiling_str"] = (
        "EM runtimes:\n"
        f"time_tree_estimation (without parallelization): {res['time_tree_estimation']}\n"
        f"time_counting: {t_count}\ntime_jtt_ipw: {t_jtt}\ntime_optimization: {t_opt}\n"
        f"total_cpu_time: {res['total_cpu_time']}\n")
    return res
