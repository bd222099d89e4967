"""deepmimo_amd - MI355X-native channel generation behind DeepMIMO's API.

Drop-in for ONE path of jmoraispk/DeepMIMO: ``dm.generate()`` / ``Dataset.compute_channels()`` /
``Dataset.channel`` (deepmimo/__init__.py:7-62 lists the reference's full public surface; the
names kept here are the ones that path needs).  The arithmetic runs in hand-written HIP kernels
for gfx950 behind a C-ABI shared library (include/deepmimo_amd.h); this package is the Python
host side that mirrors the reference's objects.

    import deepmimo_amd as dm
    ds = dm.Dataset({...float32 [n_ue, n_paths] ray matrices...})
    p = dm.ChannelGenParameters(); p.bs_antenna.shape = np.array([8, 8])
    H = ds.compute_channels(p)          # complex64 [n_ue, M_rx, M_tx, K]
"""
from . import consts
from .config import config
from .general_utils import DotDict
from .channel import ChannelGenParameters
from .dataset import Dataset, MacroDataset
from .geometry import (dft_codebook, focus_codebook, fraunhofer_distance, near_field_phase, near_field_response, pattern_gain,
                       steering_vec, wideband_array_response)
from .combiner import combine_rays, combiner_response, mu_partners, precode_rays, precoder_response
from .delay import delay_spread, tap_delays
from .core import generate, load
from .generator_utils import get_idxs_with_limits, LinearPath

__version__ = consts.VERSION


def __getattr__(name):
    # lives beside select_serving_beam in engine.py, whose import brings torch in: resolved on first use
    if name == "serving_clusters":
        from .engine import serving_clusters
        return serving_clusters
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["generate", "load", "Dataset", "MacroDataset", "ChannelGenParameters", "config", "steering_vec", "wideband_array_response", "near_field_response",
           "near_field_phase", "focus_codebook", "fraunhofer_distance", "dft_codebook", "tap_delays", "delay_spread",
           "pattern_gain", "combiner_response", "combine_rays", "precoder_response", "precode_rays", "mu_partners", "serving_clusters", "get_idxs_with_limits", "LinearPath", "DotDict", "consts"]
