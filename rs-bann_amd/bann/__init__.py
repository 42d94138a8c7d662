"""rs-bann_amd: MI355X-native branch-network HMC hot path (host-side mirror).

The compute lives in the in-tree HIP library ``rs-bann_amd/librsbann_amd.so``
(C ABI: ``include/bann.h``, ``include/bann_net.h``); this package only binds it.
"""
from ._lib import (ACTIVATIONS, HMC_STATUS, LIB_PATH, PRIORS, STEP_MODES, BannError, BannLibraryError,
                   load_library)
from . import arch, simulate
from .arch import InitConfig
from .context import BannContext
from .io import (list_model_files, write_branch_r2_csv, write_population_effect_sizes_json,
                 write_predictions_csv)
from .net import MCMCConfig, Net

__all__ = ["BannContext", "Net", "InitConfig", "arch", "simulate","list_model_files", "write_predictions_csv", "write_branch_r2_csv",
           "write_population_effect_sizes_json", "MCMCConfig", "BannError", "BannLibraryError", "load_library", "LIB_PATH", "ACTIVATIONS", "PRIORS",
           "STEP_MODES", "HMC_STATUS"]
