"""pocomc_amd -- MI355X-native engine for pocoMC's flow-preconditioned MCMC step.

``Flow`` and the four MCMC kernels keep the reference's Python surface
(``pocomc/flow.py``, ``pocomc/mcmc.py``); their arithmetic runs in hand-written
gfx950 kernels behind the C ABI of ``include/pocomc_amd.h``.
"""
from .maf_spec import MAFSpec  # noqa: F401

__all__ = ["Flow", "MAFSpec", "Reparameterize", "Sampler", "Prior", "DevicePrior", "FlowPrior", "GaussianPrior", "TruncatedGaussianPrior", "GaussianMixturePrior", "KDEPrior", "JointPrior", "mcmc", "tools"]


def __getattr__(name):
    # torch / the shared library are only touched when the GPU classes are used
    if name == "Flow":
        from .flow import Flow
        return Flow
    if name == "Reparameterize":
        from .scaler import Reparameterize
        return Reparameterize
    if name in ("mcmc", "tools", "geometry", "prior", "sampler", "train"):
        import importlib
        return importlib.import_module("." + name, __name__)
    if name == "Sampler":
        from .sampler import Sampler
        return Sampler
    if name == "Prior":
        from .prior import Prior
        return Prior
    if name == "DevicePrior":
        from .prior import DevicePrior
        return DevicePrior
    if name == "FlowPrior":
        from .prior import FlowPrior
        return FlowPrior
    if name == "GaussianPrior":
        from .prior import GaussianPrior
        return GaussianPrior
    if name == "TruncatedGaussianPrior":
        from .prior import TruncatedGaussianPrior
        return TruncatedGaussianPrior
    if name == "GaussianMixturePrior":
        from .prior import GaussianMixturePrior
        return GaussianMixturePrior
    if name == "KDEPrior":
        from .prior import KDEPrior
        return KDEPrior
    if name == "JointPrior":
        from .prior import JointPrior
        return JointPrior
    raise AttributeError(name)
