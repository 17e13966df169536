"""cherryml_amd: MI355X-native composite-likelihood core with CherryML's API
surface for that path (see DESIGN.md / INTEGRATION.md)."""
from . import caching, counting, io  # noqa: F401
from .counting import count_co_transitions, count_transitions  # noqa: F401
from .estimation_end_to_end import (coevolution_end_to_end_with_cherryml_optimizer,  # noqa: F401
                                    lg_end_to_end_with_cherryml_optimizer)
from ._siterm import learn_site_specific_rate_matrices, quantized_transitions_mle_vectorized_over_sites  # noqa: F401
from .bank import CherryBank  # noqa: F401
from .evaluation import compute_log_likelihoods  # noqa: F401,E402
from .phylogeny_estimation import BranchLengthFitter, fast_cherries, ml_branch_lengths, nj_ml_trees, nj_trees  # noqa: F401,E402
from .phylogeny_estimation import ml_lengths_and_site_rates, ml_site_rates, nj_ml_rates_trees, tree_site_rates  # noqa: F401,E402
from .phylogeny_estimation import apply_nni, ml_nni_trees, nj_nni_trees, select_nni  # noqa: F401,E402
from .phylogeny_estimation import apply_spr, ml_spr_trees, nj_spr_trees, select_spr  # noqa: F401,E402
from .phylogeny_estimation import ml_ancestral_sequences  # noqa: F401,E402
from .phylogeny_estimation import ml_branch_supports  # noqa: F401,E402
from .phylogeny_estimation import neighbor_joining_device, neighbor_joining_device_batch  # noqa: F401,E402
from .phylogeny_estimation import (bootstrap_nj_records, bootstrap_supports, nj_bootstrap_supports,  # noqa: F401,E402
                                   splits_of_join_records, tree_splits)
from .phylogeny_estimation import (nj_transfer_supports, read_transfer_supports, transfer_bootstrap_supports,  # noqa: F401,E402
                                   transfer_distances, transfer_supports_of_records, write_transfer_supports)
from .phylogeny_estimation import (bootstrap_tree, read_ufboot_supports, ufboot_supports,  # noqa: F401,E402
                                   write_ufboot_supports)
from ._cherryml_public_api import cherryml_public_api  # noqa: F401,E402
from .simulation import simulate_msas  # noqa: F401,E402
from .estimation import (EStep, RateMatrix, RateMatrixLearner, em_lg, jtt_ipw, quantized_transitions_mle,  # noqa: F401
                         train_quantization)
from .estimation_end_to_end import lg_end_to_end_with_em_optimizer  # noqa: F401,E402
from .coevolution import CoevolutionScanner, coevolution_scan, read_coevolution_scan  # noqa: F401,E402

__all__ = [
    "CherryBank", "RateMatrix", "RateMatrixLearner", "train_quantization",
    "quantized_transitions_mle", "quantized_transitions_mle_vectorized_over_sites", "jtt_ipw",
    "learn_site_specific_rate_matrices", "cherryml_public_api", "compute_log_likelihoods", "fast_cherries",
    "io", "caching", "counting", "count_transitions", "count_co_transitions",
    "lg_end_to_end_with_cherryml_optimizer", "coevolution_end_to_end_with_cherryml_optimizer", "simulate_msas",
    "EStep", "em_lg", "lg_end_to_end_with_em_optimizer", "nj_trees",
    "BranchLengthFitter", "ml_branch_lengths", "nj_ml_trees",
    "tree_site_rates", "ml_site_rates", "ml_lengths_and_site_rates", "nj_ml_rates_trees",
    "apply_nni", "select_nni", "ml_nni_trees", "nj_nni_trees", "ml_ancestral_sequences", "ml_branch_supports",
    "apply_spr", "select_spr", "ml_spr_trees", "nj_spr_trees",
    "neighbor_joining_device", "neighbor_joining_device_batch",
    "bootstrap_nj_records", "bootstrap_supports", "nj_bootstrap_supports", "splits_of_join_records", "tree_splits",
    "transfer_distances", "transfer_supports_of_records", "transfer_bootstrap_supports", "nj_transfer_supports",
    "read_transfer_supports", "write_transfer_supports",
    "bootstrap_tree", "ufboot_supports", "read_ufboot_supports", "write_ufboot_supports",
    "CoevolutionScanner", "coevolution_scan", "read_coevolution_scan",
]
