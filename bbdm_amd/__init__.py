"""bbdm_amd -- the MI355X (gfx950) hot path of xuekt98/BBDM: denoising UNet + Brownian-Bridge scheduler as
hand-written HIP kernels behind a C-ABI (include/bbdm_hip.h), exposed through drop-in model classes.

    from bbdm_amd import BrownianBridgeModel, LatentBrownianBridgeModel      # same API as the reference classes
"""
from .model import BrownianBridgeModel, LatentBrownianBridgeModel, bridge_schedule, philox_normal  # noqa: F401
from .unet import UNetModel  # noqa: F401
from .cond_stage import SpatialRescaler  # noqa: F401
from .sampler import BridgeSampler, SamplingParams  # noqa: F401
from .latent_cache import CachedPairs, LatentCache  # noqa: F401
from .optim import EMA, FusedAdam, FusedRMSprop, FusedSGD, get_optimizer  # noqa: F401
from .metrics import SetEvaluator, diversity, metrics_from_dirs, pair_metrics  # noqa: F401
from .loss_meter import LossMeter, per_image_loss, validation_loss  # noqa: F401

__all__ = ["BrownianBridgeModel", "LatentBrownianBridgeModel", "UNetModel", "SpatialRescaler", "bridge_schedule",
           "BridgeSampler", "SamplingParams", "philox_normal", "FusedAdam", "FusedSGD", "FusedRMSprop", "EMA", "get_optimizer",
           "LatentCache", "CachedPairs", "SetEvaluator", "pair_metrics", "diversity", "metrics_from_dirs",
           "LossMeter", "per_image_loss", "validation_loss"]
