"""vbq_amd -- MI355X-native hot path of Variational Bayesian Quantization.

A Python host over a C-ABI HIP extension (include/vbq.h, vbq_amd/csrc).  The package has no
CPU implementation of its kernels: on a machine without the built extension or without a
ROCm device the ops raise.

    vbq_amd.quantize(mu, sigma, lmbda, table=...)          one-call surface (api.py)
    vbq_amd.quantize_rows_to_budget(mu, sigma, total_bits) every row at exactly total_bits raw bits (rows_budget.py)
    vbq_amd.quantize_rows_to_budgets(mu, sigma, budgets)   the same at many budgets from one DP pass (include/vbq_budget.h)
    vbq_amd.ChannelwisePriorCDFQuantizer                   img-compression/quantizer.py:13-256
    vbq_amd.OptimalKmeansQuantizer / ChannelwiseOptimalKmeansWrapper   the k-means baseline fitted exactly on the device: 1-D DP,
                                                           every level count of every channel in one launch (include/vbq_kmeans.h)
    vbq_amd.LatentStore                                    latent files resident on the device: crops from device-side file ids and
                                                           origins, planned in a kernel, no synchronisation (vbq_amd/store)
    vbq_amd.utils                                          img-compression/utils.py solvers
    vbq_amd.embeddings                                     word-embeddings notebook cells 25-30; compress_to_bytes / decompress /
                                                           CompressedEmbeddings: the quantized matrix as rANS-coded bytes, rows on demand
    vbq_amd.priors                                         vae_models.py:14-43, learned_prior.py:6-334
    vbq_amd.dist                                           element-axis sharding + histogram all-reduce
    vbq_amd.LazyArray / vbq_amd.device_tensor              what compress_latents / compress hand out per lambda: ndarray-like views
                                                           over device tensors (lazy.py); device_tensor(x) = the tensor, no copy
"""
from ._lib import VBQError, lib, library_path  # noqa: F401
from . import ops  # noqa: F401
from .api import gaussian_table, quantize  # noqa: F401
from .baselines import ChannelwiseOptimalKmeansWrapper, OptimalKmeansQuantizer  # noqa: F401
from .lazy import LazyArray, device_tensor  # noqa: F401
from .quantizer import ChannelwisePriorCDFQuantizer  # noqa: F401
from .rows_budget import quantize_rows_to_budget, quantize_rows_to_budgets  # noqa: F401

__all__ = ["VBQError", "lib", "library_path", "ops", "quantize", "gaussian_table", "ChannelwisePriorCDFQuantizer", "LazyArray",
           "device_tensor", "quantize_rows_to_budget", "quantize_rows_to_budgets",
           "OptimalKmeansQuantizer", "ChannelwiseOptimalKmeansWrapper", "LatentStore"]


def __getattr__(name):
    # vbq_amd.LatentStore loads libvbq_store.so (vbq_amd/store) the first time it is asked for, as every library is loaded
    if name == "LatentStore":
        from .store import LatentStore
        return LatentStore
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
