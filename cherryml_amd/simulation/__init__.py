"""MSA simulation (the reference's cherryml.simulation): `simulate_msas` with the reference's signature, on a resident
simulator model (`Simulator`, cb_sim_model_*)."""
from ._simulate import Simulator, family_seed, simulate_msas  # noqa: F401
