"""mdqtplasmasims_amd — MI355X-native engine for the Yukawa-OCP MD + per-ion quantum-trajectory
(MDQT) hot path of tlangin/MDQTPlasmaSims' laserCoolingPlusExpansionMDQTSpeedUp.cpp.

Native code: mdqtplasmasims_amd/csrc (HIP kernels for gfx950 + C++ host engine) built into
mdqtplasmasims_amd/lib/libmdqt.so with the C ABI of include/mdqt.h.  This package is the Python
mirror of the reference's function seam (engine.Simulation), the ensemble of independent jobs stepped in
batched launches (ensemble.Ensemble; pump_ensemble.PumpEnsemble for the optical-pumping programs) and the
multi-GPU driver (sharded);
mdmc.MonteCarloMD and mdlc.LaserCooling mirror the Monte-Carlo + MD programs and the three-level
laser-cooling program (include/mdmc.h, include/mdlc.h); mdmc_ensemble.MonteCarloEnsemble holds an array of
MC + MD jobs whose Metropolis chains anneal in one launch.
"""
from ._lib import MdqtError, LIB_PATH, CLI_PATH  # noqa: F401
from .engine import Simulation, default_params, device_count, slab  # noqa: F401
from .ensemble import Ensemble, job_params, sweep_params  # noqa: F401
from .pump_ensemble import PumpEnsemble  # noqa: F401
from .mdlc import LaserCooling, default_params as mdlc_default_params, sweep_params as mdlc_sweep_params  # noqa: F401
from .mdmc_ensemble import MonteCarloEnsemble, mdmc_job_params  # noqa: F401

__all__ = ["Simulation", "Ensemble", "job_params", "sweep_params", "MdqtError", "default_params", "device_count", "slab", "LIB_PATH", "CLI_PATH",
           "LaserCooling", "mdlc_default_params", "mdlc_sweep_params", "MonteCarloEnsemble", "mdmc_job_params", "PumpEnsemble"]
