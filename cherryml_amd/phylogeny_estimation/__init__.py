"""FastCherries: branch-length / site-rate estimation on the GPU (log-transition bank, the
two bisection passes, their coordinate ascent) and, around it, the reference's seeded divide-and-conquer
cherry pairing (host) and tree / site-rate files (`fast_cherries`, `fast_cherries_family`).  Full trees: the same bisection
for all pairs of sequences on the GPU (`pairwise_branch_lengths`) and neighbour joining on the host (`neighbor_joining`,
`nj_tree_family`, the stage `nj_trees`) or, with `joiner="device"`, on the GPU (`neighbor_joining_device`,
`neighbor_joining_device_batch`); maximum-likelihood lengths on a fixed tree by EM on the GPU (`BranchLengthFitter`,
the stages `ml_branch_lengths` and `nj_ml_trees`) and the maximum-likelihood rate category of every site on it
(`tree_site_rates`, the stages `ml_site_rates`, `ml_lengths_and_site_rates` and `nj_ml_rates_trees`); topology search by
nearest-neighbour interchange scored on the GPU from the fitter's resident messages (`BranchLengthFitter.nni_scan`,
`select_nni`, `apply_nni`, the stages `ml_nni_trees` and `nj_nni_trees`); marginal ancestral reconstruction from the same messages
(`BranchLengthFitter.ancestral_states`, the stage `ml_ancestral_sequences`); aLRT, SH-like and RELL supports of the internal edges
by resampling the scan's per-site log-likelihoods on the GPU (`BranchLengthFitter.branch_supports`, the stage
`ml_branch_supports`); Felsenstein's bootstrap of the neighbour-joining tree, the resampled distances as one matrix product per pair
of sequences and the joins on the GPU (`bootstrap_nj_records`, `bootstrap_supports`, the stage `nj_bootstrap_supports`); the transfer bootstrap of the same replicates, every split of the tree against every split of
every replicate by xor and popcount on the GPU (`transfer_distances`, `transfer_bootstrap_supports`, the stage
`nj_transfer_supports`); bootstrap supports from the NNI search's own trees, the best resampled candidate of every replicate kept
on the GPU while the search runs (`BranchLengthFitter.bootstrap_best`, `ufboot_supports`, the `output_bootstrap_dir` of
`ml_nni_trees` / `nj_nni_trees`); topology search by subtree prune-and-regraft scored on the GPU from the same resident messages
(`BranchLengthFitter.spr_scan`, `enumerate_spr_moves`, `spr_indices`, `select_spr`, `apply_spr`, the stages `ml_spr_trees` and
`nj_spr_trees`)."""
from ._ble import (  # noqa: F401
    BleBank,
    branch_lengths,
    compute_log_transition_matrices,
    estimate_branch_lengths_and_site_rates,
    estimate_branch_lengths_and_site_rates_batch,
    pairwise_branch_lengths,
    rate_priors,
    site_rates,
)
from ._fast_cherries import (  # noqa: F401,E402
    cherries_to_tree,
    divide_and_pair,
    fast_cherries,
    fast_cherries_families,
    fast_cherries_family,
    get_weights_for_initial_site_rates,
    rate_categories_ble,
)
from ._nj import neighbor_joining, nj_distance_indices, nj_tree_family, nj_trees  # noqa: F401,E402
from ._nj import neighbor_joining_device, neighbor_joining_device_batch, nj_join_records  # noqa: F401,E402
from ._ml_lengths import BranchLengthFitter, ml_branch_lengths, nj_ml_trees  # noqa: F401,E402
from ._site_rates import ml_lengths_and_site_rates, ml_site_rates, nj_ml_rates_trees, tree_site_rates  # noqa: F401,E402
from ._nni import apply_nni, enumerate_nni_moves, ml_nni_trees, nj_nni_trees, select_nni  # noqa: F401,E402
from ._spr import apply_spr, enumerate_spr_moves, ml_spr_trees, nj_spr_trees, select_spr, spr_indices  # noqa: F401,E402
from ._ancestral import ml_ancestral_sequences  # noqa: F401,E402
from ._supports import ml_branch_supports, read_supports, write_supports  # noqa: F401,E402
from ._bootstrap import (  # noqa: F401,E402
    bootstrap_nj_records,
    bootstrap_supports,
    nj_bootstrap_supports,
    read_bootstrap_supports,
    splits_of_join_records,
    supports_of_records,
    tree_splits,
    write_bootstrap_supports,
)
from ._transfer import (  # noqa: F401,E402
    nj_transfer_supports,
    read_transfer_supports,
    transfer_bootstrap_supports,
    transfer_distances,
    transfer_supports_of_records,
    write_transfer_supports,
)
from ._ufboot import bootstrap_tree, read_ufboot_supports, ufboot_supports, write_ufboot_supports  # noqa: F401,E402
