"""Host-side mirror of the reference's Python model/train-loop surface (train.py:17-283, 498-523).

Same names, constructor arguments and defaults as /root/reference/train.py so a user of that script finds
`WarmUp`, `Adam`, `SGD`, `RMSprop`, `InverseTimeDecay`, `alpha_dash`, `Residual`, `Block`, `UpShuffle`, `DownShuffle`, `identity`, `Denoiser`, `Trainer`,
`compile`/`fit` and the module-level hyper-parameters here; tensors are NHWC torch tensors on the HIP device
and all arithmetic runs in libgct2.so (include/gct2.h).  There is no TensorFlow and no CPU fallback.

Module-level globals below ARE the config API, like the reference's (train.py:17-36); `configure(...)` sets
several at once.  `compute_dtype` is the one MI355X-specific knob.
"""
from __future__ import annotations

import ctypes
import sys
from typing import Callable, Dict, Iterable, List, Optional, Sequence as Seq

import numpy as np
import torch

from . import _lib
from . import trainer_math
from ._lib import BF16, CLIP_NONE, F16, F32, call
from .engine import TORCH_DTYPE, Topology, UNetEngine
from .trainer_math import clipping_mode

# ---- train.py:17-36 ---------------------------------------------------------------------------------
size = 256
pixel_size = 128 * 1
max_size = 512 * 1
block_depth = 0
octaves = 6  # bottleneck = 4x4

batch_size = 1
steps = 200

residual = False
concat = True

predict_x = True  # as opposed to epsilon
predict_scaled_epsilon = False
prediction_weighting = False
ordinary_differential_equation = False

# the v objective (Salimans & Ho 2022, "Progressive Distillation for Fast Sampling of Diffusion Models"; not in the reference): the
# network predicts v = sqrt(alpha) eps - sqrt(1 - alpha) x, and both estimates the sampler needs - x0 = sqrt(alpha) noised -
# sqrt(1 - alpha) pred and eps = sqrt(1 - alpha) noised + sqrt(alpha) pred - divide by nothing.  With it, predict_x is ignored; together
# with predict_scaled_epsilon, prediction_weighting or ordinary_differential_equation it is a ValueError.  A separate global, not one
# of the four switches of objective_switches(); Trainer reads it before every step, like training_loss
predict_v = False

# per-timestep loss weights (not in the reference): None (off), "min_snr" (min-SNR-gamma, Hang et al. 2023, with min_snr_gamma), a
# callable f(snr, t) -> weight or a sequence of `steps` floats (trainer_math.loss_weight_table).  The loss is the mean over the batch
# of lambda(t_b) times every image's own loss, not renormalised; "mse" and "l1" only.  With weights on the step is eager and runs the
# non-fused head path through gct2_objective_loss_fwd_bwd; single GPU.  Trainer reads both before every step, like training_loss
loss_weighting = None
min_snr_gamma = 5.0

mixed_precision = False

# train.py:254-280: which of Trainer.call's `return` lines is live - "mse" (train.py:272, the reference as committed), "l1"
# (train.py:268-270), "mse_pooled" (train.py:274-280: plus the MSE of 16 x 16 average pools) or "dct" (train.py:254-260, 265: the
# frequency-weighted 2-D DCT of the residual, squared and averaged); trainer_math.TRAINING_LOSSES
training_loss = "mse"

# train.py:80: `regularizer = None  # tf.keras.regularizers.l2(1e-6)` - the kernel_regularizer and bias_regularizer of every
# Conv2D, Conv2DTranspose and of the Dense(3) head (not of Residual's projection, train.py:107).  None, or regularizers.l2(...);
# Trainer reads it before every step, like training_loss
regularizer = None

# train.py:199, 203, 211-214: the commented-out per-timestep heads - `Dense(3,# * steps, ...`, `#tf.keras.layers.Reshape((size, size,
# steps, 3))` and `#prediction = tf.gather(prediction, t - 1, batch_dims=3)`.  True: the Denoiser's head is Dense(3 * steps) and every
# image reads the three outputs of its own timestep, so t finally reaches the network (gct2_dense_steps_fwd / gct2_dense_steps_bwd).
# Read when a Denoiser is constructed (it decides the head's shape); single GPU, non-fused head, parity unpinned (no TensorFlow here)
timestep_heads = False

# train.py:195-197: the commented-out `#tf.keras.layers.Dense(pixel_size, kernel_initializer='glorot_uniform', activation='relu'),`
# between the last Block(pixel_size) and the head.  True: every pixel's channels pass through a (Fu_0 + 3) -> pixel_size -> 3 perceptron
# instead of the linear map (gct2_dense2_fwd / gct2_dense2_bwd: one kernel per direction, the hidden activation is never stored).
# Read when a Denoiser is constructed (it adds dense_hidden.w / dense_hidden.b and changes dense.w's shape); single GPU, non-fused
# head, not together with timestep_heads, parity unpinned (no TensorFlow here)
hidden_dense = False

# train.py:199: the head's `kernel_initializer='glorot_uniform', #kernel_initializer='zeros'`: "glorot_uniform" (the reference as
# committed) or "zeros" (dense.w starts at zero: the first prediction is dense.b).  Read when a Denoiser's engine is built
head_initializer = "glorot_uniform"

# train.py:85-93: which `return` of alpha_dash is live - "quadratic" (train.py:93, the reference as committed), "exp2" (:88), "rational"
# (:89), "exp16" (:90), "cosine" (:91) or "quartic" (:92) (trainer_math.NOISE_SCHEDULES), or a callable f(t01) -> alpha, the user's own
# body on t01 = t / (steps + 1) - and the offset added behind it (1e-4 is the commented-out tail of train.py:93).  Trainer reads both
# before every step, like training_loss; a Denoiser's engine starts under them; alpha_dash(t) below and log_sample follow them
noise_schedule = "quadratic"
alpha_dash_offset = 0.0

warm_up = 2_000

# MI355X knob: None -> float32, or float16 when mixed_precision (train.py:38); "bfloat16" selects the
# bf16-operand / fp32-accumulate MFMA path that BASELINE.json's metric is quoted on.
compute_dtype: Optional[str] = None
# MI355X knob: in fp32 mode (the default above), run the engine's and the sampler's convolutions on the exact fp32 matrix cores
# instead of the one-thread-per-output kernels: the planned train step of the default network (UNetEngine(f32_matrix=True)) and,
# once block_depth, residual or concat leave that topology, the variant engine and its sampler (VariantEngine(f32_matrix=True):
# Block's 3x3 and the 1x1 projection too).  The eager per-layer calls (DownShuffle.call and the others) pass no call context and
# stay on the direct kernels.
f32_matrix_cores: bool = False

_DTYPES = {"float32": F32, "bfloat16": BF16, "float16": F16}


def configure(**kw) -> None:
    """set module-level hyper-parameters (the reference edits them in source, train.py:5-36)."""
    mod = sys.modules[__name__]
    for k, v in kw.items():
        if not hasattr(mod, k):
            raise AttributeError(f"unknown hyper-parameter {k!r}")
        if k == "head_initializer" and v not in trainer_math.HEAD_INITIALIZERS:
            raise ValueError(f"head_initializer must be one of {trainer_math.HEAD_INITIALIZERS}, got {v!r}")
        if k == "hidden_dense" and not isinstance(v, (bool, int)):
            raise ValueError(f"hidden_dense is a switch (True / False), got {v!r}")
        if k == "noise_schedule":
            v = trainer_math.check_noise_schedule(v, 0.0)[0]
        if k == "alpha_dash_offset":
            v = trainer_math.check_noise_schedule(None, v)[1]
        if k == "loss_weighting":
            v = trainer_math.check_loss_weighting(v)[0]
        if k == "min_snr_gamma":
            v = trainer_math.check_loss_weighting(None, v)[1]
        setattr(mod, k, v)


def objective_switches() -> Dict[str, bool]:
    """the four objective globals of train.py:29-32 as they stand NOW (Trainer.call and log_sample read them at call time)."""
    return dict(predict_x=bool(predict_x), predict_scaled_epsilon=bool(predict_scaled_epsilon),
                prediction_weighting=bool(prediction_weighting),
                ordinary_differential_equation=bool(ordinary_differential_equation))


def preferred_dtype_code() -> int:
    """train.py:38: preferred_type = float16 if mixed_precision else float32 (+ the bf16 knob)."""
    if compute_dtype is not None:
        return _DTYPES[compute_dtype]
    return F16 if mixed_precision else F32


# ---- optimizer pieces (train.py:47-83) -----------------------------------------------------------------
class L2:
    """tf.keras.regularizers.L2 [TF]: the penalty l2 * sum(w^2) per regularized tensor; the engines add its gradient 2 l2 w inside the
    optimizer kernels (gct2_optimizer_apply_reg) and report the penalty with the loss"""

    def __init__(self, l2=0.01):
        trainer_math.l2_coefficients(l2)                           # finite and >= 0 (ValueError)
        self.l2 = l2


class regularizers:
    """the tf.keras.regularizers namespace as far as train.py:80 uses it"""
    L2 = L2
    l2 = L2


def regularizer_l2(value) -> Optional[float]:
    """the module global `regularizer` as an engine's set_regularizer argument: None, or the factor of a regularizers.l2(...)"""
    if value is None:
        return None
    if not isinstance(value, L2):
        raise NotImplementedError(f"regularizer = {value!r}: only None and regularizers.l2(...) are built (no l1, l1_l2 or callables)")
    return value.l2


def sign_gradient(gradient):
    """train.py:47-48: [(tf.sign(g), v) for (g, v) in gradient] on (tensor, variable) pairs.  As an optimizer's
    gradient_transformers=[sign_gradient] it is recognised by identity and runs inside the optimizer kernel."""
    return [(torch.sign(g), v) for (g, v) in gradient]


def gradient_transform_name(gradient_transformers) -> str:
    """an optimizer's gradient_transformers argument as an engine's set_gradient_transform name: None or [] is "none",
    [sign_gradient] is "sign"; arbitrary callables are not built"""
    if gradient_transformers is None or (isinstance(gradient_transformers, (list, tuple)) and len(gradient_transformers) == 0):
        return "none"
    if isinstance(gradient_transformers, (list, tuple)) and len(gradient_transformers) == 1 and gradient_transformers[0] is sign_gradient:
        return "sign"
    raise NotImplementedError("gradient_transformers: only None, [] and [sign_gradient] are built (the transformer runs inside the "
                              "optimizer kernel; arbitrary callables are not supported)")


class WarmUp:
    """train.py:50-65: lr(step) = base*(step+1)/(warmup_steps+1) while step < warmup_steps, else base."""

    def __init__(self, base, warmup_steps):
        self.base = base
        self.warmup_steps = warmup_steps

    def __call__(self, step):
        return trainer_math.warmup_lr(step, self.base, self.warmup_steps)


class InverseTimeDecay:
    """tf.keras.optimizers.schedules.InverseTimeDecay [TF] (train.py:70, 73): lr(step) = initial / (1 + decay_rate * step / decay_steps),
    the quotient floored when staircase; float32 in Keras' order (trainer_math.inverse_time_decay_lr)."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False):
        trainer_math.inverse_time_decay_schedule(initial_learning_rate, decay_steps, decay_rate, staircase)      # decay_steps > 0 (ValueError)
        self.initial_learning_rate, self.decay_steps, self.decay_rate, self.staircase = initial_learning_rate, decay_steps, decay_rate, staircase

    def __call__(self, step):
        return trainer_math.inverse_time_decay_lr(step, self.initial_learning_rate, self.decay_steps, self.decay_rate, self.staircase)


class Optimizer:
    """what tf.keras optimizers share [TF]: the learning rate (a constant, WarmUp or InverseTimeDecay), use_ema / ema_momentum (the
    engine keeps an exponential moving average of the parameters, gct2_ema_update after every applied step; finalize_variable_values()
    overwrites the parameters with it, predict(..., use_ema=True) and log_sample(..., use_ema=True) read it), the three clipping
    arguments clipnorm / global_clipnorm / clipvalue (the engine clips per variable, all together or per element on its non-fused
    optimizer path), gradient_transformers (None or [sign_gradient], run behind the clipping step) and `iterations`."""

    def __init__(self, learning_rate, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None, clipnorm=None, global_clipnorm=None,
                 clipvalue=None, gradient_transformers=None):
        clipping_mode(clipnorm, global_clipnorm, clipvalue)        # Keras' rule: at most one of the three, each > 0 (ValueError)
        gradient_transform_name(gradient_transformers)             # None, [] or [sign_gradient] (NotImplementedError)
        self.gradient_transformers = gradient_transformers
        self.clipnorm, self.global_clipnorm, self.clipvalue = clipnorm, global_clipnorm, clipvalue
        if ema_overwrite_frequency is not None:
            raise NotImplementedError("ema_overwrite_frequency: periodic overwriting is not built; call "
                                      "optimizer.finalize_variable_values() where the parameters should become the averages")
        if use_ema and not (0.0 <= float(ema_momentum) <= 1.0):
            raise ValueError(f"ema_momentum must lie in [0, 1], got {ema_momentum!r}")
        self.learning_rate = learning_rate
        self.use_ema, self.ema_momentum, self.ema_overwrite_frequency = bool(use_ema), ema_momentum, None
        self.loss_scaling = False
        self._engine = None            # bound by Trainer.compile / train_step: the step counter lives with the engine

    @property
    def iterations(self) -> int:
        """optimizer.iterations [TF]: applied steps (a step skipped by the loss-scale logic does not count)."""
        return 0 if self._engine is None else self._engine.iterations

    def lr(self, step: int) -> float:
        return self.learning_rate(step) if callable(self.learning_rate) else float(self.learning_rate)

    def finalize_variable_values(self, var_list=None) -> None:
        """Keras' end-of-training hook [TF]: the model's parameters become their averages (var_list is ignored: the engine holds
        one arena)."""
        if self._engine is None:
            raise RuntimeError("finalize_variable_values: the optimizer is not bound to an engine yet (compile, then train)")
        self._engine.ema_overwrite()


class Adam(Optimizer):
    """tf.keras.optimizers.Adam hyper-parameters (train.py:75); the update itself is gct2_adam_keras_multi (epsilon added to sqrt(v),
    SURVEY.md A.6) - fused behind the weight gradients on one replica, gct2_adam_keras_clipped when the gradients are clipped."""

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, use_ema=False, ema_momentum=0.99,
                 ema_overwrite_frequency=None, clipnorm=None, global_clipnorm=None, clipvalue=None, gradient_transformers=None):
        super().__init__(learning_rate, use_ema, ema_momentum, ema_overwrite_frequency, clipnorm, global_clipnorm, clipvalue,
                         gradient_transformers)
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon


class SGD(Optimizer):
    """tf.keras.optimizers.SGD [TF] (train.py:69-70): plain, with momentum (Keras' velocity form) or Nesterov momentum; the update is
    gct2_optimizer_apply on the engine's non-fused optimizer path (include/gct2.h has the formulas; parity with TensorFlow unpinned)."""

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None,
                 clipnorm=None, global_clipnorm=None, clipvalue=None, gradient_transformers=None):
        trainer_math.optimizer_hyper("sgd", momentum, nesterov)     # momentum in [0, 1] (ValueError)
        super().__init__(learning_rate, use_ema, ema_momentum, ema_overwrite_frequency, clipnorm, global_clipnorm, clipvalue,
                         gradient_transformers)
        self.momentum, self.nesterov = momentum, bool(nesterov)


class RMSprop(Optimizer):
    """tf.keras.optimizers.RMSprop [TF] (train.py:73): epsilon outside the root without momentum, inside it with (optimizer_v2's two
    paths); gct2_optimizer_apply on the engine's non-fused optimizer path.  centered=True needs a third slot and is not built."""

    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, use_ema=False, ema_momentum=0.99,
                 ema_overwrite_frequency=None, clipnorm=None, global_clipnorm=None, clipvalue=None, gradient_transformers=None):
        trainer_math.optimizer_hyper("rmsprop", momentum, False, rho, epsilon)      # momentum, rho in [0, 1], epsilon >= 0 (ValueError)
        if centered:
            raise NotImplementedError("RMSprop(centered=True) keeps a third slot per parameter (the mean gradient), which is not built")
        super().__init__(learning_rate, use_ema, ema_momentum, ema_overwrite_frequency, clipnorm, global_clipnorm, clipvalue,
                         gradient_transformers)
        self.rho, self.momentum, self.epsilon, self.centered = rho, momentum, epsilon, False


class LossScaleOptimizer:
    """tf.keras.mixed_precision.LossScaleOptimizer (train.py:82-83): dynamic loss scaling."""

    def __init__(self, inner_optimizer: Optimizer):
        self.inner = inner_optimizer
        self.inner.loss_scaling = True

    def __getattr__(self, k):
        return getattr(self.inner, k)

    def finalize_variable_values(self, var_list=None) -> None:
        self.inner.finalize_variable_values(var_list)


def default_optimizer():
    """train.py:75,82-83"""
    opt = Adam(WarmUp(2e-5, warm_up))
    return LossScaleOptimizer(opt) if mixed_precision else opt


def engine_hyper_parameters(optimizer) -> Dict[str, object]:
    """an optimizer (train.py:67-78, 82-83) as the engines' hyper-parameter attributes / constructor arguments; a WarmUp or a constant
    gives base_lr and warm_up, an InverseTimeDecay gives lr_schedule, any other learning rate gives neither; SGD / RMSprop give
    optimizer_kind with their own hyper-parameters; use_ema / ema_momentum, clip_mode / clip and grad_transform are there only when the
    optimizer averages / clips / transforms (for the default optimizer the dictionary is what it always was)"""
    inner = getattr(optimizer, "inner", optimizer)
    if isinstance(inner, SGD):
        kw = dict(optimizer_kind="sgd", momentum=float(inner.momentum), nesterov=bool(inner.nesterov))
    elif isinstance(inner, RMSprop):
        kw = dict(optimizer_kind="rmsprop", rho=float(inner.rho), momentum=float(inner.momentum), epsilon=inner.epsilon)
    else:
        kw = dict(beta_1=inner.beta_1, beta_2=inner.beta_2, epsilon=inner.epsilon)
    lr = inner.learning_rate
    if isinstance(lr, WarmUp):
        kw.update(base_lr=lr.base, warm_up=lr.warmup_steps)
    elif isinstance(lr, InverseTimeDecay):
        kw.update(lr_schedule=trainer_math.inverse_time_decay_schedule(lr.initial_learning_rate, lr.decay_steps, lr.decay_rate, lr.staircase))
    elif not callable(lr):
        kw.update(base_lr=float(lr), warm_up=0)
    if getattr(inner, "use_ema", False):
        kw.update(use_ema=True, ema_momentum=float(inner.ema_momentum))
    mode, clip = clipping_mode(*(getattr(inner, k, None) for k in CLIP_ARGUMENTS))
    if mode != CLIP_NONE:
        kw.update(clip_mode=mode, clip=clip)
    transform = gradient_transform_name(getattr(inner, "gradient_transformers", None))
    if transform != "none":
        kw.update(grad_transform=transform)
    return kw


CLIP_ARGUMENTS = ("clipnorm", "global_clipnorm", "clipvalue")


OPTIMIZER_ARGUMENTS = ("momentum", "nesterov", "rho")


def apply_optimizer_kind(eng, hp: Dict[str, object]) -> None:
    """kind and schedule of engine_hyper_parameters' dictionary on an engine (set_optimizer's rule: another kind only while no step
    has been applied); a dictionary with base_lr and without lr_schedule means WarmUp / a constant, one with neither (a learning rate
    the engines do not know) leaves the schedule as it is, as it leaves base_lr and warm_up"""
    kind = hp.get("optimizer_kind", "adam")
    if kind != getattr(eng, "optimizer_kind", "adam") or kind != "adam":
        eng.set_optimizer(kind, **{k: hp[k] for k in OPTIMIZER_ARGUMENTS if k in hp})
    if ("lr_schedule" in hp or "base_lr" in hp) and hp.get("lr_schedule") != getattr(eng, "lr_schedule", None):
        eng.flush_deferred()
        eng.lr_schedule = hp.get("lr_schedule")


def clipping_arguments(optimizer) -> Dict[str, object]:
    """the optimizer's three clipping arguments as keyword arguments of an engine's set_clipping (all None: off)"""
    inner = getattr(optimizer, "inner", optimizer)
    return {k: getattr(inner, k, None) for k in CLIP_ARGUMENTS}


def alpha_dash(t):
    """train.py:85-93 (reads the module-level `steps`, `noise_schedule` and `alpha_dash_offset` when called, like the reference)"""
    return trainer_math.alpha_dash(t, steps, noise_schedule, alpha_dash_offset)


test_step = 25  # train.py:95


def identity(y_true, y_pred):
    """train.py:171-173: reduce_mean(y_pred), y_true ignored."""
    return torch.mean(y_pred)


# ---- eager layers (train.py:97-169) ---------------------------------------------------------------------
def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _code_of(t: torch.Tensor) -> int:
    return {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}[t.dtype]


def _as_compute(x: torch.Tensor, code: int) -> torch.Tensor:
    if not x.is_cuda:
        raise _lib.Gct2Error("layers run on the HIP device only (there is no CPU path)")
    return x.to(TORCH_DTYPE[code]).contiguous()


class Layer:
    def build(self, input_shape):
        pass

    def call(self, input):
        raise NotImplementedError

    def __call__(self, input):
        if not getattr(self, "_built", False):
            self.build(tuple(input[0].shape) if isinstance(input, (tuple, list)) else tuple(input.shape))
            self._built = True
        return self.call(input)


class Sequential(Layer):
    """the subset of tf.keras.Sequential the reference uses (train.py:130,183,191)."""

    def __init__(self, layers: Seq[Layer]):
        self.layers = list(layers)

    def call(self, input):
        for layer in self.layers:
            input = layer(input)
        return input


class Residual(Layer):
    """train.py:97-121: residual (input + Dense(module(input))), concat (the default) or plain module."""

    def __init__(self, module, highway=lambda x: x):
        self.module = module
        self.highway = highway
        self.dense = None

    def build(self, input_shape):
        if residual:                                             # train.py:104-108
            self.dense = Dense(input_shape[-1], use_bias=False)

    def call(self, input):
        if residual:                                             # train.py:111-112
            out = input.contiguous().clone()
            proj = self.dense(self.module(input)).to(out.dtype)
            C = out.shape[-1]
            call("gct2_add", _code_of(out), out.data_ptr(), C, proj.data_ptr(), C, out.numel() // C, C, _stream(out))
            return out
        if concat:
            return torch.cat([self.module(input).to(input.dtype), self.highway(input)], -1)
        return self.module(input)


class Block(Layer):
    """train.py:123-143: block_depth x [Conv2D(filters, 3, 1, 'same', relu)]; identity at block_depth = 0."""

    def __init__(self, filters):
        self.filters = filters
        self.convs = [Conv3x3(filters) for _ in range(block_depth)]

    def call(self, input):
        for conv in self.convs:
            input = conv(input)
        return input


class _ConvLayer(Layer):
    """shared storage for DownShuffle / UpShuffle: kernel/bias are fp32 master views (possibly into a
    Denoiser's parameter arena) plus a compute-dtype operand copy."""

    def __init__(self, filters):
        self.filters = filters
        self.kernel: Optional[torch.Tensor] = None      # fp32, Keras layout
        self.bias: Optional[torch.Tensor] = None
        self._operand = None                             # callable -> device pointer of compute-dtype kernel
        self.dtype_code = preferred_dtype_code()

    def _kernel_shape(self, cin):
        raise NotImplementedError

    def build(self, input_shape):
        if self.kernel is not None:
            return
        shp = self._kernel_shape(input_shape[-1])
        dev = torch.device("cuda", torch.cuda.current_device())
        self.kernel = ((torch.rand(shp) * 2 - 1) * trainer_math.glorot_limit(shp)).to(dev)
        self.bias = torch.zeros(self.filters, device=dev)

    def _operand_tensor(self) -> torch.Tensor:
        return self.kernel if self.dtype_code == F32 else self.kernel.to(TORCH_DTYPE[self.dtype_code])


class Conv3x3(_ConvLayer):
    """the Conv2D(filters, 3, 1, 'same', relu) of Block (train.py:131-139)."""

    def _kernel_shape(self, cin):
        return (3, 3, cin, self.filters)

    def call(self, input):
        x = _as_compute(input, self.dtype_code)
        B, H, W, C = x.shape
        y = torch.empty(B, H, W, self.filters, dtype=x.dtype, device=x.device)
        w = self._operand_tensor()
        call("gct2_conv2d_s1_fwd", None, self.dtype_code, x.data_ptr(), C, w.data_ptr(), self.bias.data_ptr(), y.data_ptr(), self.filters,
             B, H, W, C, self.filters, 3, 1, _stream(x))
        return y


class UpShuffle(_ConvLayer):
    """train.py:145-156: Conv2DTranspose(filters, 4, 2, 'same', relu)."""

    def _kernel_shape(self, cin):
        return (4, 4, self.filters, cin)

    def call(self, input):
        x = _as_compute(input, self.dtype_code)
        B, H, W, C = x.shape
        y = torch.empty(B, 2 * H, 2 * W, self.filters, dtype=x.dtype, device=x.device)
        w = self._operand_tensor()
        call("gct2_convT4s2_fwd", None, self.dtype_code, x.data_ptr(), C, w.data_ptr(), self.bias.data_ptr(), y.data_ptr(),
             self.filters, B, H, W, C, self.filters, 1, _stream(x))
        return y


class DownShuffle(_ConvLayer):
    """train.py:158-169: Conv2D(filters, 4, 2, 'same', relu)."""

    def _kernel_shape(self, cin):
        return (4, 4, cin, self.filters)

    def call(self, input):
        x = _as_compute(input, self.dtype_code)
        B, H, W, C = x.shape
        if H % 2 or W % 2:
            raise ValueError(f"DownShuffle needs even spatial dims, got {H}x{W}")
        y = torch.empty(B, H // 2, W // 2, self.filters, dtype=x.dtype, device=x.device)
        w = self._operand_tensor()
        call("gct2_conv4s2_fwd", None, self.dtype_code, x.data_ptr(), C, w.data_ptr(), self.bias.data_ptr(), y.data_ptr(),
             self.filters, B, H, W, C, self.filters, 1, _stream(x))
        return y


class Dense(Layer):
    """tf.keras.layers.Dense(units) on a rank-4 input: the Dense(3) head (train.py:198-202; fp32 output for the fp32 loss) and,
    with use_bias=False, the projection of Residual's residual=True mode (train.py:106; a 1 x 1 convolution in the compute dtype)."""

    def __init__(self, units, use_bias=True, gather_steps: int = 0, activation=None, kernel_initializer="glorot_uniform"):
        if activation not in (None, "relu"):
            raise ValueError(f"Dense: activation must be None or 'relu' (train.py:195-197), got {activation!r}")
        if activation == "relu" and not use_bias:
            raise ValueError("Dense: activation='relu' is built for the biased hidden layer of train.py:195-197 only")
        if kernel_initializer not in trainer_math.HEAD_INITIALIZERS:
            raise ValueError(f"Dense: kernel_initializer must be one of {trainer_math.HEAD_INITIALIZERS}, got {kernel_initializer!r}")
        self.activation = activation          # 'relu': the hidden Dense(pixel_size, relu) layer, a 1 x 1 convolution with ReLU in the compute dtype
        self.kernel_initializer = kernel_initializer
        self.units = units
        self.use_bias = use_bias
        self.gather_steps = gather_steps      # > 0: the per-timestep head Dense(3 * steps), evaluated by gather() on one slice per image
        self.kernel = None
        self.bias = None
        self.dtype_code = preferred_dtype_code()

    def build(self, input_shape):
        if self.kernel is not None:
            return
        shp = (input_shape[-1], self.units)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.kernel = ((torch.rand(shp) * 2 - 1) * trainer_math.glorot_limit(shp)).to(dev)
        if self.kernel_initializer == "zeros":
            self.kernel.zero_()
        self.bias = torch.zeros(self.units, device=dev) if self.use_bias else None

    def call(self, input):
        x = _as_compute(input, self.dtype_code)
        C = x.shape[-1]
        M = x.numel() // C
        if self.use_bias and self.units <= 4 and self.activation is None:
            y = torch.empty(*x.shape[:-1], self.units, dtype=torch.float32, device=x.device)
            call("gct2_dense_fwd", self.dtype_code, x.data_ptr(), C, self.kernel.data_ptr(), self.bias.data_ptr(), y.data_ptr(),
                 M, C, self.units, _stream(x))
            return y
        if self.gather_steps:
            raise _lib.Gct2Error("the per-timestep head needs the timesteps of the batch: Dense.gather(input, t_int)")
        w = self.kernel if self.dtype_code == F32 else self.kernel.to(TORCH_DTYPE[self.dtype_code])
        y = torch.empty(*x.shape[:-1], self.units, dtype=x.dtype, device=x.device)
        call("gct2_conv2d_s1_fwd", None, self.dtype_code, x.data_ptr(), C, w.data_ptr(), self.bias.data_ptr() if self.bias is not None else None,
             y.data_ptr(), self.units, M, 1, 1, C, self.units, 1, 1 if self.activation == "relu" else 0, _stream(x))
        return y

    def gather(self, input, t_int: torch.Tensor):
        """Dense + Reshape(.., steps, units / steps) + tf.gather(.., t - 1, batch_dims=3) (train.py:199, 203, 211-214) without forming
        the steps-fold output: image i gets the outputs of slice t_int[i] - 1 (gct2_dense_steps_fwd).  t_int: device int32[B] in
        1..steps; fp32 [B,H,W,units / steps]"""
        x = _as_compute(input, self.dtype_code)
        B, C = x.shape[0], x.shape[-1]
        cout = self.units // self.gather_steps
        y = torch.empty(*x.shape[:-1], cout, dtype=torch.float32, device=x.device)
        call("gct2_dense_steps_fwd", None, self.dtype_code, x.data_ptr(), C, self.kernel.data_ptr(), self.bias.data_ptr() if self.bias is not None else None,
             t_int.data_ptr(), y.data_ptr(), B, x.numel() // (B * C), C, cout, self.gather_steps, _stream(x))
        return y


def _timesteps(t, batch: int, nsteps: int) -> List[int]:
    """the t of Denoiser.call((x, t)) as `batch` checked ints: [B,1,1,1] from Trainer.call, [1] from log_sample (broadcast over the
    batch, train.py:207-209), a plain int or a sequence"""
    if torch.is_tensor(t):
        t = t.reshape(-1)
    return trainer_math.check_timesteps(t, batch, nsteps)


# ---- the model (train.py:175-283) -------------------------------------------------------------------------
class Denoiser(Layer):
    """train.py:175-215.  `self.middle` has the reference's nested structure (and is eagerly callable, one
    kernel launch + one concat copy per layer); `call` runs the planned zero-copy engine instead.
    Both read the SAME parameters: the layers' kernel/bias are views into the engine's arena."""

    def __init__(self, seed: int = 1234, device: Optional[torch.device] = None):
        self.topology = Topology(pixel_size, max_size, octaves)
        self.dtype_code = preferred_dtype_code()
        self._device = device
        self._seed = seed
        self.downs: List[DownShuffle] = [None] * octaves
        self.ups: List[UpShuffle] = [None] * octaves
        self.middle = Block(min(pixel_size * 2 ** octaves, max_size))
        for i in reversed(range(octaves)):
            filters = min(pixel_size * 2 ** i, max_size)
            self.downs[i] = DownShuffle(filters)
            self.ups[i] = UpShuffle(min(pixel_size * 2 ** i // 2, max_size))
            self.middle = Residual(
                Sequential([
                    self.downs[i],
                    Block(filters),
                    self.middle,
                    Block(filters),
                    self.ups[i],
                ])
            )
        # train.py:199, 203: Dense(3 * steps) + Reshape when the module switch is on (read here, like the reference's constructor would)
        self.timestep_heads, self._steps = bool(timestep_heads), steps
        self.head = Dense(3 * steps, gather_steps=steps) if self.timestep_heads else Dense(3, kernel_initializer=head_initializer)
        # train.py:195-197: Dense(pixel_size, relu) in front of the head when the module switch is on (read here as well)
        self.hidden_dense = bool(hidden_dense)
        trainer_math.check_head_options("Denoiser", self.hidden_dense, self.timestep_heads, head_initializer)
        self.head_initializer = head_initializer
        self.hidden = Dense(pixel_size, activation="relu") if self.hidden_dense else None
        self.middle = Sequential([
            Block(pixel_size),
            self.middle,
            Block(pixel_size),
        ] + ([self.hidden] if self.hidden_dense else []) + [
            self.head,
        ])
        self.engine: Optional[UNetEngine] = None

    def variant(self) -> bool:
        """any switch that leaves the default topology (train.py:20, 26, 27): those run on variants.VariantEngine."""
        return block_depth != 0 or residual or not concat

    def ensure_engine(self, **engine_kw):
        """build the engine on first use.  Whoever comes first - `denoiser(...)`, `trainable_variables`, the sampler callback at
        on_epoch_begin, or `trainer(...)` - the engine gets the objective switches of train.py:29-32 from the module-level
        globals (train.py reads them as module constants at call time; r02 took them from Trainer's constructor only, so an
        engine built by anything else silently trained the default objective)."""
        if self.engine is not None:
            return self.engine
        schedule = trainer_math.check_noise_schedule(noise_schedule, alpha_dash_offset)      # (ValueError before anything is built)
        # no optimizer known yet (train.py:505-509 calls the model before compile): the module-level mixed_precision
        # decides about loss scaling, as it decides about the LossScaleOptimizer wrapper in train.py:82-83
        kw = dict(steps=steps, warm_up=warm_up, seed=self._seed, loss_scaling=bool(mixed_precision), **objective_switches())
        if predict_v:                                 # (the v objective: a separate global, passed by keyword; ValueError on a clash)
            kw.update(predict_v=True)
        if self.timestep_heads:                       # (the head's shape was fixed when this Denoiser was constructed)
            kw.update(steps=self._steps, timestep_heads=True)
        if self.hidden_dense:                         # (... and so was the hidden layer in front of it)
            kw.update(hidden_dense=True)
        if self.head_initializer != "glorot_uniform":
            kw.update(head_initializer=self.head_initializer)
        if self.dtype_code == F32:
            kw["f32_matrix"] = bool(f32_matrix_cores)
        kw.update(engine_kw)
        if self.variant():
            from .variants import VariantEngine
            self.engine = VariantEngine(pixel_size, max_size, octaves, block_depth, residual, concat, self.dtype_code, self._device, **kw)
            self._bind_variant_parameters()
        else:
            self.engine = UNetEngine(self.topology, self.dtype_code, self._device, **kw)
            A = self.engine.arena
            for i in range(octaves):
                for layer, tag in ((self.downs[i], f"D{i}"), (self.ups[i], f"U{i}")):
                    layer.kernel, layer.bias = A.param(tag + ".w"), A.param(tag + ".b")
                    layer.dtype_code = self.dtype_code
                    layer._built = True
            self.head.kernel, self.head.bias = A.param("dense.w"), A.param("dense.b")
            self.head.dtype_code = self.dtype_code
            self.head._built = True
            if self.hidden_dense:
                self.hidden.kernel, self.hidden.bias = A.param("dense_hidden.w"), A.param("dense_hidden.b")
                self.hidden.dtype_code = self.dtype_code
                self.hidden._built = True
        if not trainer_math.default_noise_schedule(*schedule):     # alpha_dash's live line (train.py:85-93), like the objective switches
            self.engine.set_noise_schedule(*schedule)
        return self.engine

    def generate(self, n: int, **kw):
        """n new images from noise, fp32 [n,H,W,3] on the device: sampler.generate(self, n, ...) - strided DDIM sampling with
        num_steps, eta, clip_denoised, seed, first_index, batch_size, timesteps, noise, use_ema, use_graph, return_steps, size; init, strength
        and mask condition the run on images (image-to-image, inpainting); solver="dpm2m" is the second-order multistep solver
        (DPM-Solver++ 2M: one gct2_diffusion_step_multistep launch per step, eta = 0 only), "ddim" the default; clip_denoised="dynamic"
        with dynamic_percentile, dynamic_floor and return_thresholds is dynamic thresholding (a per-image order statistic of |x0| in the
        fixed bound's place: gct2_x0_quantile and one gct2_diffusion_step_dynamic launch per step); guide= with guidance_scale,
        guidance_interval and guide_use_ema is two-network guidance (a second Denoiser's prediction pushed away from, combined inside one
        gct2_diffusion_step_guided launch per step)"""
        from .sampler import generate
        return generate(self, n, **kw)

    def generate_to_dir(self, n: int, directory: str, **kw):
        """n new images as n PNG files in `directory`: image_out.generate_to_dir(self, n, directory, ...) - generate batch by batch, one
        gct2_image_grid_u8 launch and one copy per batch, the PNG encoder on a bounded thread pool beside the next batch; pattern, mode,
        writer, and every keyword of generate but return_steps.  Returns the paths"""
        from .image_out import generate_to_dir
        return generate_to_dir(self, n, directory, **kw)

    def encode(self, images, **kw):
        """images [n,H,W,3] into latents, fp32 [n,H,W,3] on the device: sampler.encode(self, images, ...) - strided DDIM inversion with
        num_steps, timesteps, batch_size, use_ema, use_graph, start_eps; generate(noise=latent, timesteps=...) decodes them;
        solver="dpm2m" runs the second-order multistep update up the schedule, "ddim" is the default"""
        from .sampler import encode
        return encode(self, images, **kw)

    def _bind_variant_parameters(self) -> None:
        """the nested eager layers of self.middle share the variant engine's parameters: both enumerate the layers in forward
        order (train.py:183-204), so the k-th layer with a kernel is the k-th (kernel[, bias]) group of the engine."""
        net = self.engine.net
        groups: Dict[str, Dict[str, torch.Tensor]] = {}
        for name, _ in net.specs:
            groups.setdefault(name.rsplit(".", 1)[0], {})[name.rsplit(".", 1)[1]] = net.view(net.p, name)
        order = list(groups)

        def walk(layer):
            if isinstance(layer, Sequential):
                for sub in layer.layers:
                    yield from walk(sub)
            elif isinstance(layer, Residual):
                yield from walk(layer.module)
                if residual:
                    layer.dense = Dense(0, use_bias=False)
                    layer._built = True                          # build() would replace the bound projection
                    yield layer.dense
            elif isinstance(layer, Block):
                yield from layer.convs
            else:
                yield layer

        layers = list(walk(self.middle))
        assert len(layers) == len(order), (len(layers), len(order))
        for layer, key in zip(layers, order):
            layer.kernel, layer.bias = groups[key]["w"], groups[key].get("b")
            if isinstance(layer, Dense):
                layer.units = layer.kernel.shape[-1]
            layer.dtype_code = self.dtype_code
            layer._built = True

    @property
    def trainable_variables(self) -> Dict[str, torch.Tensor]:
        eng = self.ensure_engine()
        if self.variant():
            return {k: eng.net.view(eng.net.p, k) for k in eng.net.shapes}
        A = eng.arena
        return {k: A.param(k) for k in A.shapes}

    def call(self, input):
        x, t = input            # t is ignored by the reference as well (train.py:208-210) - unless the per-timestep heads are on
        eng = self.ensure_engine()
        if self.timestep_heads:                      # train.py:211-214: tf.gather(prediction, t - 1, batch_dims=3)
            return eng.predict(x, _timesteps(t, x.shape[0], eng.steps)).clone()
        return eng.predict(x).clone()

    def call_eager(self, input):
        """the reference's literal layer-by-layer evaluation of self.middle (train.py:210)."""
        x, t = input
        eng = self.ensure_engine()
        if self.timestep_heads:                      # everything up to the head, then the head on each image's own slice
            vals = _timesteps(t, x.shape[0], eng.steps)
            for layer in self.middle.layers[:-1]:
                x = layer(x)
            return self.head.gather(x, torch.tensor(vals, dtype=torch.int32).to(x.device))
        return self.middle(x)


def _supported_learning_rate(hp: Dict[str, object]) -> None:
    if "base_lr" not in hp and "lr_schedule" not in hp:
        raise NotImplementedError("only WarmUp, InverseTimeDecay or constant learning rates are supported")


class LambdaCallback:
    """tf.keras.callbacks.LambdaCallback(on_epoch_begin=...) (train.py:519-521)."""

    def __init__(self, on_epoch_begin: Optional[Callable] = None, on_epoch_end: Optional[Callable] = None):
        self.on_epoch_begin = on_epoch_begin
        self.on_epoch_end = on_epoch_end


class Trainer(Layer):
    """train.py:217-283 + the Keras compile/fit driver (train.py:511-523)."""

    def __init__(self, denoiser: Denoiser):
        self.denoiser = denoiser
        self.optimizer = None
        self.loss_fn = None
        self.metrics = ()                                # compile(metrics=[...]): what evaluate and fit's validation report besides the loss

    def _engine(self) -> UNetEngine:
        trainer_math.training_loss_code(training_loss)   # an unknown name: ValueError, before anything is built or changed
        loss_kind = training_loss
        opt = self.optimizer
        kw = {}
        if opt is not None and self.denoiser.engine is None:
            kw = engine_hyper_parameters(opt)
            _supported_learning_rate(kw)
            kw["loss_scaling"] = bool(getattr(opt, "inner", opt).loss_scaling)
        l2 = regularizer_l2(regularizer)                 # anything but None / regularizers.l2: NotImplementedError, before anything is built
        schedule = trainer_math.check_noise_schedule(noise_schedule, alpha_dash_offset)      # an unknown name, a non-finite offset: ValueError
        built = getattr(getattr(self.denoiser, "engine", None), "timestep_heads", getattr(self.denoiser, "timestep_heads", None))
        if built is not None and bool(timestep_heads) != bool(built):       # (the head's shape is fixed with the Denoiser and its engine)
            raise ValueError(f"timestep_heads = {bool(timestep_heads)} now, but the Denoiser (and the engine behind it) was built with "
                             f"timestep_heads = {bool(built)}: the switch decides the shape of the Dense head "
                             "(train.py:199) - construct a new Denoiser after changing it")
        built = getattr(getattr(self.denoiser, "engine", None), "hidden_dense", getattr(self.denoiser, "hidden_dense", None))
        if built is not None and bool(hidden_dense) != bool(built):         # (... and so is the hidden layer in front of it)
            raise ValueError(f"hidden_dense = {bool(hidden_dense)} now, but the Denoiser (and the engine behind it) was built with "
                             f"hidden_dense = {bool(built)}: the switch adds the Dense(pixel_size, relu) layer of train.py:195-197 and "
                             "changes the head's shape - construct a new Denoiser after changing it")
        clipped = kw.pop("clip_mode", None) is not None
        kw.pop("clip", None)
        transform = kw.pop("grad_transform", None)
        kind = {k: kw.pop(k) for k in ("optimizer_kind", "lr_schedule") + OPTIMIZER_ARGUMENTS if k in kw}
        eng = self.denoiser.ensure_engine(**kw)
        if clipped:                                      # (a fresh engine: clipping is a setting, not a constructor argument)
            eng.set_clipping(**clipping_arguments(opt))
        if kind:                                         # (... and so are the optimizer kind and a schedule other than WarmUp)
            apply_optimizer_kind(eng, kind)
        if transform is not None:                        # (... and the gradient transformer)
            eng.set_gradient_transform(transform)
        # train.py:238-252 reads the objective globals every time Trainer.call runs: an engine built earlier (by denoiser(...),
        # trainable_variables, the log_sample callback) follows the switches as they stand now
        switches = objective_switches()
        trainer_math.check_predict_v(predict_v, switches["predict_scaled_epsilon"], switches["prediction_weighting"],
                                     switches["ordinary_differential_equation"])      # a clash: ValueError, before anything changes
        weighting = trainer_math.check_loss_weighting(loss_weighting, min_snr_gamma)
        if weighting[0] is not None and loss_kind not in trainer_math.WEIGHTED_TRAINING_LOSSES:
            raise ValueError(f"loss_weighting with training_loss {loss_kind!r}: per-timestep weights are built for "
                             f"{' and '.join(trainer_math.WEIGHTED_TRAINING_LOSSES)}")
        for k, v in switches.items():
            setattr(eng, k, v)
        if bool(predict_v) != bool(getattr(eng, "predict_v", False)):      # (... and the v objective)
            eng.flush_deferred()
            eng.predict_v = bool(predict_v)
        eng.training_loss = loss_kind                    # (... and the `return` of train.py:265-280 that is live now)
        if trainer_math.l2_coefficients(l2)[0] != getattr(eng, "l2", 0.0):     # (... and the regularizer of train.py:80)
            eng.set_regularizer(l2)
        if schedule != (getattr(eng, "noise_schedule", "quadratic"), getattr(eng, "alpha_dash_offset", 0.0)):     # (... and alpha_dash's live line)
            eng.set_noise_schedule(*schedule)
        have = (getattr(eng, "loss_weighting", None), getattr(eng, "min_snr_gamma", 5.0))
        if weighting[0] != have[0] or (weighting[0] is not None and weighting[1] != have[1]):     # (... and the per-timestep loss weights)
            eng.set_loss_weighting(*weighting)
        return eng

    def call(self, x):
        """returns the scalar fp32 loss for a freshly noised batch (train.py:223-272); no gradients."""
        eng = self._engine()
        x = x.to(eng.device, torch.float32).contiguous()
        if self.denoiser.variant():
            return eng.train_step(x, backward=False).clone()[0]
        eng.check_step_settings()                      # the weighting against the objective as it stands now (ValueError)
        b = eng.buffers(*x.shape[:3])
        eng.sample_noise(b)
        eng.noise_into_r0(b, x, unfused_head=True)     # forward(head=True) reads the image channels from R_0 itself
        eng.forward(b)
        if eng.loss_weighting is not None:             # the weighted loss: gct2_objective_loss_fwd_bwd's loss-only form
            return eng.objective_loss_and_dpred(b, x, grad=False).clone()[0]
        if eng.default_objective():
            return eng.loss_and_dpred(b, x, grad=False).clone()[0]
        target, w = eng.make_target(b, x)              # train.py:238-252
        if eng.objective_weighted():
            return eng.weighted_loss_and_dpred(b, target, w, grad=False).clone()[0]
        return eng.loss_and_dpred(b, target, grad=False).clone()[0]

    def compile(self, optimizer, loss, metrics=None):
        """train.py:511-514.  metrics (Keras' argument; None: none): names out of trainer_math.METRICS - "mse_x0", "psnr", "ssim" -
        that evaluate() and fit(validation_data=...) report by default; an unknown or repeated name is a ValueError and nothing changes."""
        metrics = trainer_math.check_metrics(metrics)
        if self.denoiser.engine is not None and optimizer is not None:
            eng, inner = self.denoiser.engine, getattr(optimizer, "inner", optimizer)
            hp = engine_hyper_parameters(optimizer)
            apply_optimizer_kind(eng, hp)                 # (first: a refused change of kind leaves the engine as it was)
            for k, v in hp.items():
                if k not in ("use_ema", "ema_momentum", "clip_mode", "clip", "grad_transform", "optimizer_kind", "lr_schedule") + OPTIMIZER_ARGUMENTS:
                    setattr(eng, k, v)
            if "clip_mode" in hp or getattr(eng, "clip_mode", CLIP_NONE) != CLIP_NONE:
                eng.set_clipping(**clipping_arguments(optimizer))      # (an optimizer without clipping switches it off)
            if hp.get("grad_transform", "none") != getattr(eng, "grad_transform", "none"):
                eng.set_gradient_transform(hp.get("grad_transform", "none"))      # (... and one without a transformer, that)
            if hp.get("use_ema"):                         # the averages start from the parameters as they stand now
                eng.enable_ema(hp["ema_momentum"])
            elif getattr(eng, "use_ema", False):
                eng.disable_ema()
            if inner.loss_scaling and eng.ls_state is None:
                eng.enable_loss_scaling()                 # train.py:505-514: the model is called before compile
            elif not inner.loss_scaling and eng.ls_state is not None:
                if eng.iterations != 0:
                    raise _lib.Gct2Error("the engine has already stepped with dynamic loss scaling; it cannot be dropped now")
                eng.ls_state, eng.loss_scaling = None, False
        self.optimizer, self.loss_fn, self.metrics = optimizer, loss, metrics
        inner = getattr(optimizer, "inner", optimizer)
        if inner is not None:
            inner._engine = self.denoiser.engine

    def train_step(self, data):
        """one Keras train_step on a (x, y) batch with y == x (train.py:293): returns {'loss': tensor}."""
        x = data[0] if isinstance(data, (tuple, list)) else data
        eng = self._engine()
        loss = eng.train_step(x)
        inner = getattr(self.optimizer, "inner", self.optimizer)
        if inner is not None:
            inner._engine = eng
        return {"loss": loss}

    def evaluate(self, dataset: Iterable, steps: Optional[int] = None, return_dict: bool = False, use_ema: bool = False, t=None,
                 seed: Optional[int] = None, metrics=None):
        """Keras' Model.evaluate on held-out data: the training loss as it stands now (objective, training_loss, noise schedule),
        averaged over every IMAGE `dataset` yields - (x, x) pairs or bare x batches, a partial last batch included.  steps: at most
        that many batches (None: until the dataset ends; an endless dataset then is a ValueError where it can be known).  Each image
        gets its timestep and noise from evaluation's own streams by its running index (TrainerState.evaluate_batch), so the figure
        does not depend on the batch size and no training state moves; t: one timestep (or one per image of a batch) instead;
        seed: instead of the engine's rng_seed.  use_ema: the averaged weights.  With an L2 regularizer the penalty of the weights
        read is added, as in the train step's loss.  One host synchronisation, at the end.
        return_dict: {"loss": float, "per_image": float32 [N] (the data term of every image), "t": int32 [N]} instead of the float.
        Under a loss_weighting the rows are multiplied by lambda(t) of their image, the loss is the weighted mean (not renormalised) and
        return_dict holds the weighted per_image plus "loss_weight", float32 [N]: the caller can divide.
        metrics: names out of trainer_math.METRICS (None: those of compile(); (): none) - the image-space metrics of every image's x0
        estimate against the clean image (gct2_image_metrics), whatever the objective predicts.  With any, the return value is
        [loss, m1, m2, ...] in the order asked, as Keras returns it, each the float64 mean over the images (inf for "psnr" when an
        image is reproduced exactly); return_dict adds each mean under its name and "per_image_<name>" float32 [N].  With none the
        return value is exactly the one above.  Still one host synchronisation."""
        metrics = self.metrics if metrics is None else trainer_math.check_metrics(metrics)
        if steps is not None and (isinstance(steps, bool) or not isinstance(steps, int) or steps < 1):
            raise ValueError(f"evaluate: steps must be a positive int or None, got {steps!r}")
        if steps is None and getattr(dataset, "finite", True) is False:
            raise ValueError("evaluate: the dataset never ends (an ImageDataset in training mode): pass steps, or build it with "
                             "ImageDataset.validation")
        eng = self._engine()
        rows, ts, lams, index = [], [], [], 0
        mrows = {n: [] for n in metrics}

        def run():
            nonlocal index
            for k, data in enumerate(dataset):
                x = data[0] if isinstance(data, (tuple, list)) else data
                if metrics:
                    r, tt, mm = eng.evaluate_batch(x, index0=index, t=t, seed=seed, metrics=metrics)
                    for n in metrics:
                        mrows[n].append(mm[n])
                else:
                    r, tt = eng.evaluate_batch(x, index0=index, t=t, seed=seed)
                rows.append(r)
                ts.append(tt)
                if "loss_weight" in eng.last_eval:             # (loss_weighting: r holds the weighted rows, this their weights)
                    lams.append(eng.last_eval["loss_weight"])
                index += int(x.shape[0])
                if steps is not None and k + 1 >= steps:       # (an endless dataset is not asked for a batch nobody reads)
                    break

        if use_ema:
            with eng.ema_weights():
                run()
                penalty = self._evaluation_penalty(eng)
        else:
            run()
            penalty = self._evaluation_penalty(eng)
        if not rows:
            raise ValueError("evaluate: the dataset yielded no batch")
        N = index
        if metrics:                                            # (one tensor, so that one copy brings everything to the host)
            everything = torch.cat(rows + [m for n in metrics for m in mrows[n]]).cpu().numpy()      # the one host synchronisation
            per_image = everything[:N]
            per_metric = {n: everything[(k + 1) * N:(k + 2) * N] for k, n in enumerate(metrics)}
        else:
            per_image = torch.cat(rows).cpu().numpy()          # the one host synchronisation
        t_all = torch.cat(ts).cpu().numpy()
        loss = float(np.mean(per_image, dtype=np.float64))
        if penalty is not None:
            loss += float(penalty.cpu()[0])
        weights = {"loss_weight": torch.cat(lams).cpu().numpy()} if lams else {}
        if not metrics:
            if return_dict:
                return {"loss": loss, "per_image": per_image, "t": t_all, **weights}
            return loss
        with np.errstate(invalid="ignore"):
            means = {n: float(np.mean(per_metric[n], dtype=np.float64)) for n in metrics}
        if return_dict:
            out = {"loss": loss, "per_image": per_image, "t": t_all, **weights}
            for n in metrics:
                out[n] = means[n]
                out["per_image_" + n] = per_metric[n]
            return out
        return [loss] + [means[n] for n in metrics]

    @staticmethod
    def _evaluation_penalty(eng) -> Optional[torch.Tensor]:
        """l2 * sum(w^2) over the regularized tensors of the weights evaluation just read (the averages inside ema_weights()), fp32 [1]
        on the device; None without a regularizer.  Scalars of its own: the train step's reported penalty stays what it was."""
        if not getattr(eng, "l2", 0.0) > 0.0:
            return None
        eng.flush_deferred()
        if getattr(eng, "_eval_l2_state", None) is None:       # (built once: the segment table, the partial sums, three scalars)
            eng._eval_l2_state = (eng._sumsq_tables(eng._l2_segments()), torch.zeros(3, dtype=torch.float32, device=eng._clip_device()))
        (table, nseg, npartials, partials, sumsq, _), scalars = eng._eval_l2_state
        p = eng._ema if eng._ema_reading else eng._fp32_parameters()
        zero, penalty, total = scalars[0:1].zero_(), scalars[1:2], scalars[2:3]
        s = eng._stream()
        _lib.call("gct2_grad_sumsq", p.data_ptr(), table.data_ptr(), nseg, npartials, 1.0, None, partials.data_ptr(), sumsq.data_ptr(), s)
        _lib.call("gct2_l2_penalty", zero.data_ptr(), sumsq.data_ptr() + 8 * nseg, float(eng.l2), penalty.data_ptr(), total.data_ptr(), s)
        return penalty

    def fit(self, dataset: Iterable, steps_per_epoch: int = 1000, epochs: int = 1, callbacks: Seq = (), verbose: int = 1,
            validation_data: Optional[Iterable] = None, validation_steps: Optional[int] = None, validation_freq: int = 1,
            validation_use_ema: bool = False):
        """train.py:516-523.  `dataset` yields (image, image) batches, NHWC in [-1, 1).
        validation_data (Keras' argument; None: nothing about fit changes): after every validation_freq-th epoch,
        evaluate(iter(validation_data), validation_steps, use_ema=validation_use_ema) goes into logs["val_loss"] and
        history["val_loss"] before on_epoch_end runs - pass something that can be iterated once per validation (a list of batches,
        an ImageDataset.validation).  The metrics of compile(metrics=[...]) go into logs["val_<name>"] and history["val_<name>"]."""
        if self.optimizer is None:
            raise RuntimeError("call compile(optimizer, loss) before fit (train.py:511)")
        if validation_data is not None:
            if isinstance(validation_freq, bool) or not isinstance(validation_freq, int) or validation_freq < 1:
                raise ValueError(f"fit: validation_freq must be a positive int, got {validation_freq!r}")
            if validation_steps is None and getattr(validation_data, "finite", True) is False:
                raise ValueError("fit: validation_data never ends (an ImageDataset in training mode): pass validation_steps, or build "
                                 "it with ImageDataset.validation")
        it = iter(dataset)
        history = {"loss": []}
        if validation_data is not None:
            history["val_loss"] = []
            for n in self.metrics:
                history["val_" + n] = []
        for epoch in range(epochs):
            logs: Dict[str, float] = {}
            for cb in callbacks:
                if getattr(cb, "on_epoch_begin", None):
                    cb.on_epoch_begin(epoch, logs)
            running = None
            for _ in range(steps_per_epoch):
                out = self.train_step(next(it))
                running = out["loss"] if running is None else running + out["loss"]
            logs["loss"] = float(running[0]) / steps_per_epoch     # one host sync per epoch
            history["loss"].append(logs["loss"])
            line = f"Epoch {epoch + 1}/{epochs} - loss: {logs['loss']:.6f}"
            if validation_data is not None and (epoch + 1) % validation_freq == 0:
                val = self.evaluate(iter(validation_data), validation_steps, use_ema=validation_use_ema)
                val = val if self.metrics else [val]
                for n, value in zip(("loss",) + self.metrics, val):
                    logs["val_" + n] = value
                    history["val_" + n].append(value)
                    line += f" - val_{n}: {value:.6f}"
            if verbose:
                print(line, flush=True)
            for cb in callbacks:
                if getattr(cb, "on_epoch_end", None):
                    cb.on_epoch_end(epoch, logs)
        return history


def image_metrics(a: torch.Tensor, b: torch.Tensor, max_val: float = 2.0, filter_size: int = 11, filter_sigma: float = 1.5,
                  k1: float = 0.01, k2: float = 0.03) -> Dict[str, torch.Tensor]:
    """tf.image.psnr / tf.image.ssim [TF] of two device image batches [B,H,W,C] (C in 1..4), e.g. samples against references:
    {"mse_x0", "psnr", "ssim"}, fp32 [B] device tensors, by one gct2_image_metrics launch on the current stream of a's device; no
    host synchronisation.  max_val: the dynamic range (2 for images in [-1, 1)); the window is trainer_math.ssim_window(filter_size,
    filter_sigma), both sides of the image at least filter_size."""
    if a.dim() != 4 or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"image_metrics: two NHWC batches of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.device.type != "cuda" or b.device != a.device:
        raise _lib.Gct2Error("image_metrics needs both batches on one HIP device (torch device 'cuda'); there is no CPU path")
    window = torch.from_numpy(trainer_math.ssim_window(filter_size, filter_sigma)).to(a.device)
    a, b = a.to(torch.float32).contiguous(), b.to(torch.float32).contiguous()
    B, H, W, Cc = a.shape
    need = ctypes.c_size_t(0)
    _lib.check(_lib.load().gct2_image_metrics_scratch(B, H, W, Cc, window.numel(), ctypes.byref(need)), "gct2_image_metrics_scratch")
    scratch = torch.zeros(max(4, need.value), dtype=torch.float32, device=a.device)
    out = torch.empty(3, B, dtype=torch.float32, device=a.device)
    _lib.call("gct2_image_metrics", a.data_ptr(), None, None, None, b.data_ptr(), window.data_ptr(), window.numel(), float(max_val), float(k1),
              float(k2), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), scratch.data_ptr(), scratch.numel(), B, H, W, Cc,
              torch.cuda.current_stream(a.device).cuda_stream)
    for keep in (a, b, window, scratch):                   # (the launch is asynchronous: its operands live until the stream has passed it)
        keep.record_stream(torch.cuda.current_stream(a.device))
    return {n: out[k] for k, n in enumerate(trainer_math.METRICS)}
