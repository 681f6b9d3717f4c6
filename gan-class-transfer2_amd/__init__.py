"""MI355X-native train step of relgukxilef/GAN-Class-Transfer2's denoising U-Net (train.py).

The directory name carries a hyphen (project convention); import it as `gan_class_transfer2_amd`
(the alias package next to it extends its __path__ here).
"""
from . import _lib, build, data, engine, model, sampler, trainer_math # noqa: F401
from .data import CachedImageDataset, ImageDataset, sample_picks  # noqa: F401
from .sampler import encode, generate, log_sample, make_log_sample  # noqa: F401
from . import image_out                          # noqa: F401
from .image_out import ImageWriter, SummarySink, generate_to_dir, grid_shape, image_grid, save_images, to_uint8  # noqa: F401
from ._lib import BF16, F16, F32, Gct2Error       # noqa: F401
from .engine import Topology, UNetEngine          # noqa: F401
from .model import (Adam, Block, Dense, Denoiser, DownShuffle, InverseTimeDecay, LambdaCallback, LossScaleOptimizer,  # noqa: F401
                    RMSprop, Residual, SGD, Sequential, Trainer, UpShuffle, WarmUp, alpha_dash, configure, identity, image_metrics,
                    regularizers, sign_gradient)
from .trainer_math import METRICS, NOISE_SCHEDULES, alpha_table, noise_table, ssim_window  # noqa: F401
from .trainer_math import GENERATE_STREAM, ddim_sigma2, sampling_timesteps                 # noqa: F401
from .trainer_math import check_mask, img2img_steps                                         # noqa: F401
from .trainer_math import SOLVERS, half_log_snr, multistep_coefficient                      # noqa: F401
from .trainer_math import quantile_rank                                                     # noqa: F401
from .trainer_math import guidance_launches, guidance_table                                 # noqa: F401
from .trainer_math import LOSS_WEIGHTINGS, loss_weight_table                                # noqa: F401
from . import distill                                                                       # noqa: F401
from .distill import Distiller, clone_denoiser, progressive_distill                         # noqa: F401
from .trainer_math import DISTILL_STREAM_EPS, DISTILL_STREAM_PAIR, distill_grid, distill_table  # noqa: F401
