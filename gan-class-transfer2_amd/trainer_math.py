"""The host-side arithmetic of the reference's `Trainer` (train.py:50-93, 223-272), once, for every engine.

Pure functions (no GPU needed): the noise schedule, the WarmUp and InverseTimeDecay learning rates, the Adam step size, the Glorot limit and the
per-image coefficients of the objective.  `TrainerState` is what `UNetEngine` and `VariantEngine` inherit: the hyper-parameters,
the objective switches, the RNG stream positions, the step counter and the dynamic loss-scale state with its three calls.
The order of the float32 operations in every formula is the reference's; the golden fixture of tests/test_trainer_math_cpu.py
holds the values bit for bit.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import F32, Slot, call

LOSS_SCALE_GROWTH_INTERVAL = 2000   # tf.keras.mixed_precision.LossScaleOptimizer's dynamic_growth_steps default [TF]


# train.py:85-93: the body of alpha_dash holds six formulas, five of them commented out (the author moves the `return`), and a
# commented-out offset behind the live one.  In the order quadratic = :93 (live), exp2 = :88, rational = :89, exp16 = :90,
# cosine = :91, quartic = :92.  A schedule is one of these names or a callable f(t01) -> alpha (the user's own body, called on
# t01 = t / (steps + 1)), plus a float offset added behind the formula (0.0; 1e-4 is the tail of train.py:93)
NOISE_SCHEDULES = ("quadratic", "exp2", "rational", "exp16", "cosine", "quartic")

# the bodies on t01, written once for Python floats, torch tensors and numpy arrays: c(v) types a literal (the identity for Python
# floats and tensors, the array's dtype D for numpy, so that EVERY operation rounds in D) and cos is the cosine of that arithmetic.
# Python's ** is right-associative: 2**8**t is 2**(8**t); 256*256 is formed in D (it overflows float16, as the reference's would)
_SCHEDULE_BODIES = {
    "quadratic": lambda t, c, cos: (c(1) - t) ** 2 * c(0.25),                                          # train.py:93
    "exp2": lambda t, c, cos: c(1) - c(2) ** (t - c(1)),                                               # train.py:88
    "rational": lambda t, c, cos: ((c(2 ** 8) - c(2) ** (c(8) ** t))
                                   / (c(256) * c(2) ** (c(8) ** t) - c(2) ** (c(8) ** t) + c(2 ** 8))),   # train.py:89
    "exp16": lambda t, c, cos: (c(256) * c(256)) ** (c(-1) * t),                                       # train.py:90
    "cosine": lambda t, c, cos: cos(c(math.pi / 2) * t) ** 2,                                          # train.py:91
    "quartic": lambda t, c, cos: (c(1) - t) ** 4,                                                      # train.py:92
}


def check_noise_schedule(schedule=None, offset=0.0):
    """(schedule, offset) checked: a NOISE_SCHEDULES name (None is "quadratic") or a callable, and a finite float (ValueError)"""
    schedule = "quadratic" if schedule is None else schedule
    if isinstance(schedule, str):
        if schedule not in NOISE_SCHEDULES:
            raise ValueError(f"unknown noise_schedule {schedule!r} (one of {', '.join(NOISE_SCHEDULES)}, or a callable f(t01) -> alpha)")
    elif not callable(schedule):
        raise ValueError(f"noise_schedule must be one of {NOISE_SCHEDULES} or a callable f(t01) -> alpha, got {schedule!r}")
    try:
        off = float(offset)
    except (TypeError, ValueError):
        raise ValueError(f"alpha_dash_offset must be a finite float, got {offset!r}") from None
    if not math.isfinite(off):
        raise ValueError(f"alpha_dash_offset must be a finite float, got {offset!r}")
    return schedule, off


def default_noise_schedule(schedule=None, offset=0.0) -> bool:
    """the reference as committed (train.py:93 without its tail): the formula kernels and the torch formulas serve it"""
    return (schedule is None or (isinstance(schedule, str) and schedule == "quadratic")) and float(offset) == 0.0


def noise_schedule_name(schedule) -> str:
    """what a checkpoint and a message call a schedule: its name, or "custom" for a callable"""
    return schedule if isinstance(schedule, str) else "custom"


def alpha_dash(t, steps: int, schedule=None, offset=0.0):
    """train.py:85-93; `t` a python float (the sampler) or a tensor (float32: the train step's t_int).  The two-argument call is the
    reference as committed.  schedule / offset: another body (NOISE_SCHEDULES or a callable) evaluated in the arithmetic of `t` -
    Python floats for a Python float, which is how the sampler calls it (t = steps / 2 and t - 1 = 0 included).  "cosine" on a Python
    float is math.cos in double; TensorFlow would evaluate tf.cos of a Python float as a float32 tensor [TF]: a deviation, parity
    unpinned (there is no TensorFlow here)."""
    if default_noise_schedule(schedule, offset):
        return (1 - t / (steps + 1)) ** 2 * 0.25
    t01 = t / (steps + 1)
    if callable(schedule):
        a = schedule(t01)
    else:
        a = _SCHEDULE_BODIES[check_noise_schedule(schedule)[0]](t01, lambda v: v, torch.cos if torch.is_tensor(t01) else math.cos)
    return a + offset if offset else a


def _alpha_array(schedule, offset, t: np.ndarray, what: str) -> np.ndarray:
    """alpha on the array t of t01 values, every numpy operation rounded in t's dtype D; a callable is called once on the array and
    its result cast to D.  ValueError when the evaluation overflows or is invalid in D, or when an entry is non-finite or outside
    [0, 1] (an underflow to 0 is legal)."""
    schedule, offset = check_noise_schedule(schedule, offset)
    D, name = t.dtype.type, noise_schedule_name(schedule)
    try:
        with np.errstate(over="raise", invalid="raise", divide="raise", under="ignore"):
            if callable(schedule):
                a = np.asarray(schedule(t)).astype(D)
                if a.shape != t.shape:
                    raise ValueError(f"the noise schedule returned shape {a.shape} for {t.shape} timesteps")
            else:
                a = np.asarray(_SCHEDULE_BODIES[schedule](t, D, np.cos), dtype=D)
            if offset:
                a = a + D(offset)
    except (FloatingPointError, OverflowError, ZeroDivisionError) as e:
        raise ValueError(f"noise schedule {name!r} cannot be evaluated in {np.dtype(D).name} ({what}): {e}") from None
    if not (np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all()):
        bad = int(np.flatnonzero(~(np.isfinite(a) & (a >= 0) & (a <= 1)))[0])
        raise ValueError(f"noise schedule {name!r} (offset {offset!r}) in {np.dtype(D).name} ({what}): alpha = {a[bad]!r} at table "
                         f"entry {bad} is not a finite value in [0, 1]")
    return a


def noise_table(schedule, offset, steps: int, dtype: int) -> np.ndarray:
    """float32 [steps, 2], entry t - 1 = (sqrt(alpha_dash(t)), sqrt(1 - alpha_dash(t))): what gct2_noise_image_table reads.  Formed
    in the reference's operation order in D = float32 (F32 and BF16) or float16 (F16: Keras' mixed_float16, where t is an fp16
    tensor): t = arange(1..steps).astype(D) / D(steps + 1), a division like train.py:87, the body, the offset, then sa = sqrt(a)
    and sb = sqrt(D(1) - a) in D, widened to float32 (exactly).  ValueError as _alpha_array says."""
    D = np.float16 if dtype == _lib.F16 else np.float32
    if int(steps) < 1:
        raise ValueError(f"steps must be >= 1, got {steps!r}")
    with np.errstate(over="ignore"):
        t = np.arange(1, int(steps) + 1).astype(D) / D(int(steps) + 1)
    if not np.isfinite(t).all():
        raise ValueError(f"{steps} timesteps cannot be held in {np.dtype(D).name}")
    a = _alpha_array(schedule, offset, t, f"noise_table, steps {steps}")
    out = np.stack([np.sqrt(a), np.sqrt(D(1) - a)], axis=1)
    assert out.dtype == D
    return np.ascontiguousarray(out, dtype=np.float32)


def alpha_table(schedule, offset, steps: int) -> np.ndarray:
    """float32 [steps + 1]: alpha_dash(t) for t = 0 .. steps in float32 arithmetic (the arithmetic of the train step's torch formula):
    objective_coefficients gathers alpha(t) and alpha(t - 1) from it under a non-default schedule"""
    t = np.arange(0, int(steps) + 1).astype(np.float32) / np.float32(int(steps) + 1)
    return _alpha_array(schedule, offset, t, f"alpha_table, steps {steps}")


def warmup_lr(k: int, base_lr: float, warm_up: int) -> float:
    """WarmUp.__call__ (train.py:57-65) at optimizer.iterations = k, float32 arithmetic like the reference."""
    if k < warm_up:
        return float(np.float32(base_lr) * np.float32(k + 1) / np.float32(warm_up + 1))
    return float(np.float32(base_lr))


def inverse_time_decay_lr(k: int, initial: float, decay_steps: float, decay_rate: float, staircase: bool = False) -> float:
    """tf.keras.optimizers.schedules.InverseTimeDecay.__call__ [TF] at optimizer.iterations = k, float32 arithmetic in Keras' order:
    q = k / decay_steps (floored when staircase), lr = initial / (1 + decay_rate * q); gct2_loss_scale_begin_schedule computes the
    same on the device when the step counter lives there."""
    f = np.float32
    q = f(k) / f(decay_steps)
    if staircase:
        q = np.floor(q)
    return float(f(initial) / (f(1.0) + f(decay_rate) * q))


def adam_step_size(lr: float, k: int, beta_1: float, beta_2: float) -> float:
    """lr * sqrt(1 - b2^t) / (1 - b1^t), t = k + 1, with the betas as the float32 hyper-parameters Keras holds them as [TF];
    gct2_loss_scale_begin computes the same on the device when the step counter lives there."""
    tt = k + 1
    b1, b2 = float(np.float32(beta_1)), float(np.float32(beta_2))
    return lr * math.sqrt(1.0 - b2 ** tt) / (1.0 - b1 ** tt)


def glorot_limit(shape: Sequence[int]) -> float:
    """limit of Keras glorot_uniform for a kernel [..., fan-in channels, fan-out channels] (train.py:134,149,162)."""
    rf = int(np.prod(shape[:-2]))
    return math.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))


def default_objective(predict_x: bool, ordinary_differential_equation: bool) -> bool:
    """the network predicts the clean image and the target is the batch itself (train.py:243-244)"""
    return bool(predict_x and not ordinary_differential_equation)


def objective_weighted(predict_x: bool, prediction_weighting: bool, ordinary_differential_equation: bool) -> bool:
    """train.py:250-252: prediction and target both scaled by sqrt(1 - alpha_dash(t)) (epsilon branch only)."""
    return bool(not predict_x and not ordinary_differential_equation and prediction_weighting)


def check_predict_v(predict_v: bool, predict_scaled_epsilon: bool = False, prediction_weighting: bool = False,
                    ordinary_differential_equation: bool = False) -> bool:
    """predict_v checked against the reference's switches: it replaces predict_x (whose value is then ignored) and does not combine
    with predict_scaled_epsilon, prediction_weighting or ordinary_differential_equation (ValueError)"""
    if predict_v:
        clash = [k for k, on in (("predict_scaled_epsilon", predict_scaled_epsilon), ("prediction_weighting", prediction_weighting),
                                 ("ordinary_differential_equation", ordinary_differential_equation)) if on]
        if clash:
            raise ValueError(f"predict_v does not combine with {', '.join(clash)}: the v objective has one target, "
                             "sqrt(alpha) eps - sqrt(1 - alpha) x, and one pair of estimates")
    return bool(predict_v)


def weighting_objective(predict_x: bool = True, predict_scaled_epsilon: bool = False, prediction_weighting: bool = False,
                        ordinary_differential_equation: bool = False, predict_v: bool = False) -> Optional[str]:
    """what the network predicts, as loss_weight_table names it: "v", "x" or "eps"; None for the scaled-epsilon, ODE and
    prediction_weighting objectives, which have no named weighting"""
    if check_predict_v(predict_v, predict_scaled_epsilon, prediction_weighting, ordinary_differential_equation):
        return "v"
    if ordinary_differential_equation:
        return None
    if predict_x:
        return "x"
    return None if (predict_scaled_epsilon or prediction_weighting) else "eps"


LOSS_WEIGHTINGS = ("min_snr",)
WEIGHTED_TRAINING_LOSSES = ("mse", "l1")       # the kinds gct2_objective_loss_fwd_bwd computes


def check_loss_weighting(kind, gamma: float = 5.0):
    """(kind, gamma) checked: None (off), a LOSS_WEIGHTINGS name, a callable f(snr, t) -> weight or a sequence of floats (returned as
    a tuple: one weight per timestep 1..steps); gamma a finite float > 0 (ValueError)"""
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"min_snr_gamma must be a finite float > 0, got {gamma!r}") from None
    if not (math.isfinite(g) and g > 0.0):
        raise ValueError(f"min_snr_gamma must be a finite float > 0, got {gamma!r}")
    if kind is None or callable(kind):
        return kind, g
    if isinstance(kind, str):
        if kind not in LOSS_WEIGHTINGS:
            raise ValueError(f"unknown loss_weighting {kind!r} (one of {', '.join(LOSS_WEIGHTINGS)}, a callable f(snr, t) or a sequence of "
                             "`steps` floats)")
        return kind, g
    try:
        seq = tuple(float(v) for v in (kind.tolist() if hasattr(kind, "tolist") else kind))
    except (TypeError, ValueError):
        raise ValueError(f"loss_weighting must be None, one of {LOSS_WEIGHTINGS}, a callable f(snr, t) or a sequence of floats, "
                         f"got {kind!r}") from None
    return seq, g


def loss_weight_table(kind, gamma: float = 5.0, steps: int = 200, objective: Optional[str] = "x", schedule=None,
                      offset: float = 0.0) -> np.ndarray:
    """float32 [steps + 1]: lambda(t) of configure(loss_weighting=kind) for t = 1..steps, entry 0 zero; formed in Python floats
    (double) and rounded once.  SNR(t) = alpha / (1 - alpha) with alpha = alpha_table(schedule, offset, steps)[t] as a Python float
    (inf at alpha = 1).
      "min_snr" (Hang et al. 2023): the weight that makes the x0-space weight min(SNR, gamma) -
          objective "x":   min(SNR, gamma)
          objective "eps": 1 where SNR <= gamma, else gamma / SNR        (no 0 / 0 at alpha = 0)
          objective "v":   min(SNR, gamma) / (SNR + 1)                   (0 at SNR = inf)
          any other objective (None: scaled epsilon, ODE, prediction_weighting) is a ValueError
      a callable f(snr: float, t: int) -> float, or a sequence of `steps` floats (entry t - 1 is lambda(t)): under any objective.
    Every entry must be finite and >= 0 (ValueError)."""
    kind, gamma = check_loss_weighting(kind, gamma)
    steps = int(steps)
    if kind is None:
        raise ValueError("loss_weight_table: loss_weighting is None (off): there is no table")
    if steps < 1:
        raise ValueError(f"steps must be >= 1, got {steps!r}")
    alpha = alpha_table(schedule, offset, steps)
    snr = [0.0] * (steps + 1)
    for t in range(1, steps + 1):
        a = float(alpha[t])
        snr[t] = math.inf if a >= 1.0 else a / (1.0 - a)
    lam = [0.0] * (steps + 1)
    if isinstance(kind, str):
        if objective not in ("x", "eps", "v"):
            raise ValueError(f"loss_weighting {kind!r} is defined for the x, epsilon and v objectives; predict_scaled_epsilon, "
                             "prediction_weighting and ordinary_differential_equation take a callable or a table")
        for t in range(1, steps + 1):
            r = snr[t]
            if objective == "x":
                lam[t] = min(r, gamma)
            elif objective == "eps":
                lam[t] = 1.0 if r <= gamma else gamma / r
            else:
                lam[t] = 0.0 if math.isinf(r) else min(r, gamma) / (r + 1.0)
    elif callable(kind):
        for t in range(1, steps + 1):
            try:
                lam[t] = float(kind(snr[t], t))
            except (TypeError, ValueError) as e:
                raise ValueError(f"loss_weighting: the callable returned no float at timestep {t}: {e}") from None
    else:
        if len(kind) != steps:
            raise ValueError(f"loss_weighting: a table of {len(kind)} weights for {steps} timesteps")
        lam[1:] = kind
    with np.errstate(over="ignore"):
        out = np.asarray(lam, dtype=np.float64).astype(np.float32)
    bad = np.flatnonzero(~(np.isfinite(out) & (out >= 0)))
    if bad.size:
        raise ValueError(f"loss_weighting: the weight of timestep {int(bad[0])} is {lam[int(bad[0])]!r}: every weight must be finite "
                         "(in float32) and >= 0")
    return out


def objective_coefficients(t_int: torch.Tensor, steps: int, predict_x: bool = True, predict_scaled_epsilon: bool = False,
                           prediction_weighting: bool = False, ordinary_differential_equation: bool = False,
                           schedule=None, offset: float = 0.0, roots: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                           predict_v: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """per-image (a, c, w) of train.py:238-252: target = a x + c eps, prediction weight w (ones unless objective_weighted) -
    contiguous float32 vectors on t_int's device.  The default schedule keeps its torch formula; any other gathers sqrt(alpha) and
    sqrt(1 - alpha), formed on the host in float32 from alpha_table, at t or t - 1 (roots: those two [steps + 1] vectors already on
    the device - an engine keeps them).  predict_v (keyword only in practice; predict_x is then ignored): the v objective of Salimans &
    Ho 2022, target = sqrt(alpha) eps - sqrt(1 - alpha) x, (a, c, w) = (-sb, sa, 1) with the float32 roots at t."""
    t = t_int.to(torch.float32)
    one, zero = torch.ones_like(t), torch.zeros_like(t)
    tabled = not default_noise_schedule(schedule, offset)
    if tabled:
        if roots is None:
            roots = tuple(torch.from_numpy(r).to(t_int.device) for r in alpha_roots(schedule, offset, steps))
        at = lambda r, shift: r.index_select(0, (t_int.to(torch.int64) - shift).clamp(0, steps)).contiguous()
    if predict_v:
        check_predict_v(predict_v, predict_scaled_epsilon, prediction_weighting, ordinary_differential_equation)
        if tabled:
            return (-at(roots[1], 0)).contiguous(), at(roots[0], 0), one
        av = alpha_dash(t, steps)
        return (-(1 - av).sqrt()).contiguous(), av.sqrt().contiguous(), one
    if ordinary_differential_equation:                                # train.py:238-242
        if tabled:
            return at(roots[0], 1), at(roots[1], 1), one
        a1 = alpha_dash(t - 1, steps)
        return a1.sqrt().contiguous(), (1 - a1).sqrt().contiguous(), one
    if predict_x:                                                     # train.py:243-244
        return one, zero, one
    s = at(roots[1], 0) if tabled else (1 - alpha_dash(t, steps)).sqrt()
    c = s if predict_scaled_epsilon else one                          # train.py:245-248
    if prediction_weighting:                                          # train.py:250-252
        return zero, (c * s).contiguous(), s.contiguous()
    return zero, c.contiguous(), one


def alpha_roots(schedule, offset, steps: int) -> Tuple[np.ndarray, np.ndarray]:
    """(sqrt(alpha), sqrt(1 - alpha)) of alpha_table, float32 [steps + 1] each, every operation rounded in float32"""
    a = alpha_table(schedule, offset, steps)
    return np.sqrt(a), np.sqrt(np.float32(1.0) - a)


def check_schedule_marker(sd: dict, schedule, offset: float) -> None:
    """a checkpoint's "noise_schedule" entry ([index into NOISE_SCHEDULES or -1 for a callable, offset]; absent = the default)
    against an engine's schedule: two NAMED schedules that disagree are refused, nothing is loaded - a network trained under another
    schedule would continue (and sample) wrongly without any error.  A callable on either side cannot be compared and passes."""
    if "noise_schedule" in sd:
        code, have_off = int(sd["noise_schedule"][0]), float(sd["noise_schedule"][1])
        have = NOISE_SCHEDULES[code] if 0 <= code < len(NOISE_SCHEDULES) else "custom"
    else:
        have, have_off = "quadratic", 0.0
    want = noise_schedule_name(schedule)
    if "custom" not in (have, want) and (have, have_off) != (want, float(offset)):
        raise ValueError(f"the checkpoint was trained under noise schedule {have!r} with offset {have_off!r} and this engine runs "
                         f"{want!r} with offset {float(offset)!r} (set_noise_schedule before loading; nothing is loaded)")


def schedule_marker(schedule, offset: float) -> torch.Tensor:
    """the "noise_schedule" entry of a checkpoint (written only for a non-default schedule)"""
    code = NOISE_SCHEDULES.index(schedule) if isinstance(schedule, str) else -1
    return torch.tensor([float(code), float(offset)], dtype=torch.float64)


def ema_coefficients(momentum: float) -> Tuple[float, float]:
    """(momentum, 1 - momentum) as the two float32 factors of Keras' optimizer EMA [TF]: Python forms 1 - momentum in double and the
    product with a float32 tensor rounds it once - so does the host here (gct2_ema_update takes both factors)."""
    return float(np.float32(momentum)), float(np.float32(1.0 - float(momentum)))


def clipping_mode(clipnorm=None, global_clipnorm=None, clipvalue=None) -> Tuple[int, float]:
    """Keras' three optimizer clipping arguments [TF] as (gct2_adam_keras_clipped mode, threshold): at most one of them, each finite
    and > 0 (ValueError otherwise); all None is (CLIP_NONE, 0.0)"""
    given = [(k, m, v) for k, m, v in (("clipnorm", _lib.CLIP_NORM, clipnorm), ("global_clipnorm", _lib.CLIP_GLOBAL_NORM, global_clipnorm),
                                       ("clipvalue", _lib.CLIP_VALUE, clipvalue)) if v is not None]
    if len(given) > 1:
        raise ValueError(f"at most one of clipnorm, global_clipnorm and clipvalue can be set, got {', '.join(k for k, _, _ in given)}")
    if not given:
        return _lib.CLIP_NONE, 0.0
    name, mode, value = given[0]
    value = float(value)
    with np.errstate(all="ignore"):
        as_f32 = float(np.float32(value))                # what the C ABI receives
    if not (value > 0.0 and as_f32 > 0.0 and math.isfinite(as_f32)):
        raise ValueError(f"{name} must be a finite float32 > 0, got {given[0][2]!r}")
    return mode, value


OPTIMIZER_KINDS = {"adam": _lib.OPT_ADAM, "sgd": _lib.OPT_SGD, "rmsprop": _lib.OPT_RMSPROP}


def optimizer_hyper(kind: str = "adam", momentum: float = 0.0, nesterov: bool = False, rho: float = 0.9, epsilon: Optional[float] = None):
    """the hyper-parameters of an optimizer kind, checked the way tf.keras checks them (ValueError): (kind, momentum, nesterov, rho)
    and, only when given, epsilon"""
    if kind not in OPTIMIZER_KINDS:
        raise ValueError(f"unknown optimizer kind {kind!r} (one of {', '.join(OPTIMIZER_KINDS)})")
    momentum, rho = float(momentum), float(rho)
    if not (0.0 <= momentum <= 1.0):
        raise ValueError(f"momentum must lie in [0, 1], got {momentum!r}")
    if not (0.0 <= rho <= 1.0):
        raise ValueError(f"rho must lie in [0, 1], got {rho!r}")
    if epsilon is not None and not (float(epsilon) >= 0.0):
        raise ValueError(f"epsilon must be >= 0, got {epsilon!r}")
    return kind, momentum, bool(nesterov), rho


def inverse_time_decay_schedule(initial: float, decay_steps: float, decay_rate: float, staircase: bool = False) -> tuple:
    """the engines' lr_schedule tuple of an InverseTimeDecay (ValueError unless decay_steps > 0)"""
    if not (float(decay_steps) > 0.0):
        raise ValueError(f"decay_steps must be > 0, got {decay_steps!r}")
    return ("inverse_time_decay", float(initial), float(decay_steps), float(decay_rate), bool(staircase))


# Keras' gradient_transformers as the engines know them: none, or train.py:47-48's sign_gradient (gct2_optimizer_apply_reg transform)
GRADIENT_TRANSFORMS = {"none": _lib.GRAD_NONE, "sign": _lib.GRAD_SIGN}


def l2_coefficients(l2) -> Tuple[float, float]:
    """tf.keras.regularizers.l2(l2) [TF] as (l2 held as float32, c = (float)(2.0 * (double)(float)l2)): the factor of the reported
    penalty l2 * sum(w^2) and the factor of its gradient 2 l2 w (gct2_optimizer_apply_reg's l2_coeff).  None is (0.0, 0.0), off;
    negative or not finite in float32 is a ValueError"""
    if l2 is None:
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        held = float(np.float32(float(l2)))
        c = float(np.float32(2.0 * held))
    if not (float(l2) >= 0.0 and math.isfinite(held) and math.isfinite(c)):
        raise ValueError(f"the l2 regularization factor must be a finite float32 >= 0, got {l2!r}")
    return held, c


def coefficient_runs(segs, coeffs, total: int):
    """[(begin, end, coefficient)]: the maximal runs of neighbouring tensors with the same coefficient, together covering [0, total) -
    a run starts at its first tensor (the first run at 0) and ends where the next begins, alignment padding included"""
    runs = []
    for (begin, _), c in zip(segs, coeffs):
        if not runs:
            runs.append([0, total, c])
        elif runs[-1][2] != c:
            runs[-1][1] = begin
            runs.append([begin, total, c])
    return [tuple(r) for r in runs]


OBJECTIVE_SWITCHES = ("predict_x", "predict_scaled_epsilon", "prediction_weighting", "ordinary_differential_equation")

# the four ways Trainer.call turns target - prediction into the scalar Keras minimises (train.py:254-280: the author moves a `return`)
TRAINING_LOSSES = ("mse", "l1", "mse_pooled", "dct")
_LOSS_CODES = {"mse": _lib.LOSS_MSE, "l1": _lib.LOSS_L1, "mse_pooled": _lib.LOSS_MSE_POOLED, "dct": _lib.LOSS_DCT}


def training_loss_code(name: str) -> int:
    """the gct2_loss_fwd_bwd kind of a TRAINING_LOSSES name (ValueError for anything else)"""
    if name not in _LOSS_CODES:
        raise ValueError(f"unknown training_loss {name!r} (one of {', '.join(TRAINING_LOSSES)})")
    return _LOSS_CODES[name]


# the Philox stream ids of evaluation (TrainerState.evaluate_batch): the train step draws t from stream 1 and eps from stream 2
EVAL_STREAM_T, EVAL_STREAM_EPS = 3, 4


# ---- generation (sampler.generate; gct2_diffusion_start / gct2_diffusion_step) --------------------------------------------------------
# the Philox stream id of generation's noise: streams 1 and 2 are the train step's, 3 and 4 evaluation's
GENERATE_STREAM = 5
# the Philox stream ids of the device-resident image cache (data.CachedImageDataset; gct2_image_batch_cached): crop origin and flip of a
# running sample index, and the round keys of an epoch's permutation
DATA_STREAM_AUG = 6
DATA_STREAM_ORDER = 7


def sampling_timesteps(steps: int, num_steps: int) -> list:
    """the K = num_steps timesteps a strided sampler visits out of 1..steps, ascending: ceil(i steps / K) for i = 1..K (integer
    arithmetic).  Strictly increasing (steps / K >= 1), ends at `steps`; K = steps is 1..steps.  ValueError unless 1 <= K <= steps."""
    for name, v in (("steps", steps), ("num_steps", num_steps)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"sampling_timesteps: {name} must be an int, got {v!r}")
    steps, K = int(steps), int(num_steps)
    if not 1 <= K <= steps:
        raise ValueError(f"sampling_timesteps: num_steps must lie in 1..steps = 1..{steps}, got {K}")
    return [-((-i * steps) // K) for i in range(1, K + 1)]


def ddim_sigma2(a_t: float, a_prev: float, eta: float) -> float:
    """the variance of the noise a sampling step from alpha a_t to alpha a_prev adds (Song et al., DDIM, eq. 16, squared):
    eta^2 (1 - a_prev) / (1 - a_t) (1 - a_t / a_prev), clamped to [0, 1 - a_prev].  eta = 0 is the deterministic DDIM step, eta = 1
    the DDPM posterior variance.  Python floats; ValueError for eta < 0 (or NaN)."""
    eta, a_t, a_prev = float(eta), float(a_t), float(a_prev)
    if not eta >= 0.0:
        raise ValueError(f"ddim_sigma2: eta must be >= 0, got {eta!r}")
    if eta == 0.0 or a_prev <= 0.0 or a_t >= 1.0:
        return 0.0
    s = eta * eta * (1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev)
    return min(max(s, 0.0), 1.0 - a_prev)


def generate_offset(g: int, k: int, num_steps: int, per_image: int) -> int:
    """the first element of stream GENERATE_STREAM that image g (its running index over the whole generation) reads in slot k: 0 is
    the starting noise, 1..K the steps in sampling order.  Image g owns [g (K + 1) per_image, (g + 1) (K + 1) per_image): its noise
    depends on g and the seed alone, not on the batch it is drawn in; consecutive images are generate_image_stride apart."""
    K = int(num_steps)
    if not (g >= 0 and 0 <= k <= K and per_image >= 1):
        raise ValueError(f"generate_offset: image {g!r}, slot {k!r} of 0..{K}, per_image {per_image!r}")
    return (int(g) * (K + 1) + int(k)) * int(per_image)


def generate_image_stride(num_steps: int, per_image: int) -> int:
    return (int(num_steps) + 1) * int(per_image)


def img2img_steps(num_steps: int, strength: float) -> int:
    """how many of the K = num_steps sampling steps an image-conditioned generate runs: min(K, max(1, int(K strength + 0.5))), the
    steps at the low-noise end of the schedule (it starts at the K'-th timestep of sampling_timesteps).  strength = 1 is the whole
    schedule; ValueError unless 0 < strength <= 1."""
    K, strength = int(num_steps), float(strength)
    if K < 1:
        raise ValueError(f"img2img_steps: num_steps must be >= 1, got {num_steps!r}")
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"img2img_steps: strength must lie in (0, 1], got {strength!r}")
    return min(K, max(1, int(K * strength + 0.5)))


# ---- second-order multistep sampling (generate / encode with solver="dpm2m"; gct2_diffusion_step_multistep) ----------------------------
SOLVERS = ("ddim", "dpm2m")


def half_log_snr(a: float) -> float:
    """lambda of DPM-Solver (Lu et al. 2022): log(alpha / sigma) = 0.5 log(a / (1 - a)) at the cumulative alpha a, from Python floats.
    -inf at a <= 0, +inf at a >= 1."""
    a = float(a)
    if a <= 0.0:
        return -math.inf
    if a >= 1.0:
        return math.inf
    return 0.5 * math.log(a / (1.0 - a))


def multistep_coefficient(a_before: Optional[float], a_t: float, a_prev: float) -> float:
    """c1 of gct2_diffusion_step_multistep for the step from alpha a_t to alpha a_prev, when the step before was evaluated at alpha
    a_before: with h = lambda(a_prev) - lambda(a_t) and h_prev = lambda(a_t) - lambda(a_before) (half_log_snr), h / (2 h_prev) - the
    1 / (2 r) of DPM-Solver++ 2M, r = h_prev / h.  0.0 without history (a_before None), where one of the three lambdas is not finite
    (alpha 0 or 1: the ends of the process) and at h_prev == 0.  Either direction: descending alphas (generate) and ascending ones
    (encode) both give c1 > 0 on a monotone schedule."""
    if a_before is None:
        return 0.0
    l_before, l_t, l_prev = half_log_snr(a_before), half_log_snr(a_t), half_log_snr(a_prev)
    if not (math.isfinite(l_before) and math.isfinite(l_t) and math.isfinite(l_prev)):
        return 0.0
    h, h_prev = l_prev - l_t, l_t - l_before
    if h_prev == 0.0:
        return 0.0
    return h / (2.0 * h_prev)


# ---- dynamic thresholding (generate with clip_denoised="dynamic"; gct2_x0_quantile) -----------------------------------------------------
def quantile_rank(p: float, n: int) -> int:
    """the 1-based rank of the order statistic that stands for the p-quantile of n values, p in (0, 1]: min(n, max(1, ceil(p n))) - no
    interpolation (it differs from numpy.percentile's "linear" by less than one element's gap).  A Python int computed once on the
    host: the kernel never sees p.  ValueError for p outside (0, 1] or n < 1."""
    p, n = float(p), int(n)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"quantile_rank: p must lie in (0, 1], got {p!r}")
    if n < 1:
        raise ValueError(f"quantile_rank: n must be a positive int, got {n!r}")
    return min(n, max(1, math.ceil(p * n)))


# ---- two-network guidance (generate with guide=; gct2_diffusion_step_guided / gct2_x0_quantile_guided) -----------------------------------
def guidance_table(scale, steps: int, interval=None) -> list:
    """the guidance weight of every timestep as Python floats: entry t - 1 is w(t), t = 1..steps, of p = p_guide + w (p_main - p_guide).
    scale: a float (every timestep), a callable f(t: int) -> float, or a sequence of `steps` floats - the forms loss_weighting takes.
    interval = (t_lo, t_hi), ints with 1 <= t_lo <= t_hi <= steps: the weight holds for t_lo <= t <= t_hi and is 1.0 - the main network
    alone - elsewhere (Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval Improves Sample and Distribution Quality in
    Diffusion Models").  Every weight must be finite, also as the float32 the kernel receives; a bool is no weight (ValueError)."""
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"guidance_table: steps must be >= 1, got {steps!r}")
    if scale is None or isinstance(scale, (bool, np.bool_, str)):
        raise ValueError(f"guidance_scale must be a float, a callable f(t) or a sequence of {steps} floats, got {scale!r}")
    if callable(scale):
        raw = [scale(t) for t in range(1, steps + 1)]
    elif isinstance(scale, (int, float, np.integer, np.floating)):
        raw = [scale] * steps
    else:
        try:
            raw = list(scale.tolist() if hasattr(scale, "tolist") else scale)
        except TypeError:
            raise ValueError(f"guidance_scale must be a float, a callable f(t) or a sequence of {steps} floats, got {scale!r}") from None
        if len(raw) != steps:
            raise ValueError(f"guidance_scale: a table of {len(raw)} weights for {steps} timesteps")
    table = []
    for t, v in enumerate(raw, 1):
        try:
            if isinstance(v, (bool, np.bool_, str)):
                raise TypeError
            w = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"guidance_scale: the weight of timestep {t} is {v!r}, not a float") from None
        with np.errstate(over="ignore"):
            if not (math.isfinite(w) and math.isfinite(float(np.float32(w)))):
                raise ValueError(f"guidance_scale: the weight of timestep {t} is {w!r}: every weight must be finite (in float32)")
        table.append(w)
    if interval is not None:
        try:
            lo, hi = interval
        except (TypeError, ValueError):
            raise ValueError(f"guidance_interval must be (t_lo, t_hi), got {interval!r}") from None
        if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in (lo, hi)) or not 1 <= lo <= hi <= steps:
            raise ValueError(f"guidance_interval must be ints with 1 <= t_lo <= t_hi <= {steps}, got {interval!r}")
        table = [w if lo <= t <= hi else 1.0 for t, w in enumerate(table, 1)]
    return table


def guidance_launches(weights) -> Tuple[bool, list]:
    """what a guided run launches, from the weights of the steps it runs in sampling order (one batch): (start_copy, per step
    (guided_entry, pred_guide, write_views)).
      pred_guide    the step combines the two predictions: its weight is not exactly 1.0 (only then is the guide evaluated)
      write_views   the step stores its result into the guide engine's input views too: exactly when the NEXT step reads the guide
      guided_entry  the step is gct2_diffusion_step_guided (with the guided select under dynamic thresholding) - when it needs
                    pred_guide or the views; else the existing entry point, so an all-ones run is guide=None launch for launch
      start_copy    the first step run reads the guide: one gct2_diffusion_mix(fake, fake, alpha = 0) writes the guide's views, once
                    per batch"""
    guided = [float(w) != 1.0 for w in weights]
    steps = []
    for k, g in enumerate(guided):
        views = k + 1 < len(guided) and guided[k + 1]
        steps.append((g or views, g, views))
    return bool(guided and guided[0]), steps


# ---- progressive distillation (distill.Distiller; gct2_distill_start / _step / _target) -------------------------------------------------
# the Philox stream ids that belong to distillation alone: the pair of sample k at position k of stream 8, its noise at positions
# [k per_image, (k + 1) per_image) of stream 9
DISTILL_STREAM_PAIR = 8
DISTILL_STREAM_EPS = 9
# the columns of a row of distill_table (include/gct2.h GCT2_DISTILL_ROW)
DISTILL_COLUMNS = ("sa0", "sb0", "sa1", "sb1", "sa2", "sb2", "r", "den", "cx0", "ck0", "cx1", "ce1")


def distill_grid(steps: int, student_steps: int, timesteps=None) -> list:
    """the teacher's ascending grid of K = 2N timesteps for a student of N = student_steps steps: sampling_timesteps(steps, 2N), or an
    explicit strictly increasing list of 2N integers within 1..steps.  Pair j = 1..N is (t, t', t'') = (taus[2j-1], taus[2j-2],
    taus[2j-3]); pair 1 has no t''.  The student's grid taus[1::2] of the default is sampling_timesteps(steps, N)
    (ceil(2i steps / 2N) = ceil(i steps / N)): a distilled student is sampled with plain generate(num_steps=N).
    ValueError unless 1 <= N and 2N <= steps."""
    for name, v in (("steps", steps), ("student_steps", student_steps)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"distill_grid: {name} must be an int, got {v!r}")
    steps, N = int(steps), int(student_steps)
    if not (1 <= N and 2 * N <= steps):
        raise ValueError(f"distill_grid: the teacher takes 2 N = {2 * N} of steps = {steps} timesteps: 1 <= N and 2 N <= steps")
    if timesteps is None:
        return sampling_timesteps(steps, 2 * N)
    given = list(timesteps)
    if len(given) != 2 * N or any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) for t in given) or given[0] < 1 or \
            given[-1] > steps or any(b <= a for a, b in zip(given, given[1:])):
        raise ValueError(f"distill_grid: timesteps must be {2 * N} strictly increasing integers within 1..{steps}, got {given!r}")
    return [int(t) for t in given]


def distill_table(taus, steps: int, schedule=None, offset: float = 0.0, mode: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(float32 [N][12], int32 [N][2]) of an ascending grid taus of 2N timesteps: what gct2_distill_start / _step / _target read.
    Row j - 1 belongs to pair j, (t, t', t'') = (taus[2j-1], taus[2j-2], taus[2j-3]), alphas a0, a1, a2 = alpha_dash of them as
    Python floats: DISTILL_COLUMNS = {sa0, sb0, sa1, sb1, sa2, sb2, r, den, cx0, ck0, cx1, ce1}; the int part holds {t, t'}.
      sa, sb    (float)sqrt(a), (float)sqrt(1 - a): square roots in double, one cast each (gct2_diffusion_step's sa / sb at a_t = a)
      r, den    (float)(sb2 / sb0) and (float)(sa2 - (sb2 / sb0) sa0), in double from the double roots, rounded once
      cx0, ck0  sqrtf((float)a0), sqrtf(1.f - (float)a0): the pair gct2_diffusion_start_image forms at a = a0 - the teacher's z_t is the
                bits generate(init=) would start from
      cx1, ce1  sqrtf((float)a1), sqrtf(1.f - (float)a1): the pair gct2_diffusion_step re-noises with at a_prev = a1 - the teacher's
                first step is generate's step bit for bit (a float32 root of a float32 alpha can differ from sa1 / sb1 in the last place)
    The end point of pair 1 is a2 = 1, (sa2, sb2, r, den) = (1, 0, 0, 1): generate returns the last step's x0 estimate, not an image
    re-noised to alpha_dash(0) (0.25 on the default schedule), so the student's last estimate is trained onto what the teacher's
    generate returns.  ValueError if a den <= 0 (alpha is not strictly decreasing along the grid; on a monotone schedule
    den > sa2 - sa0 > 0), if an alpha leaves gct2_diffusion_step's range (a_t in [0, 1)), or - mode given, an objective code of
    include/gct2.h - if a_t = 0 under an objective that divides by sqrt(a_t) (the epsilon modes)."""
    taus = [int(t) for t in taus]
    if not taus or len(taus) % 2 or any(b <= a for a, b in zip(taus, taus[1:])):
        raise ValueError(f"distill_table: taus must be an even number of strictly increasing timesteps, got {taus!r}")
    N = len(taus) // 2
    tab, tt = np.zeros((N, len(DISTILL_COLUMNS)), dtype=np.float32), np.zeros((N, 2), dtype=np.int32)
    f32 = np.float32
    divides = mode in (_lib.SAMPLE_EPS, _lib.SAMPLE_SCALED_EPS)
    for j in range(1, N + 1):
        t, t1 = taus[2 * j - 1], taus[2 * j - 2]
        a0, a1 = float(alpha_dash(t, steps, schedule, offset)), float(alpha_dash(t1, steps, schedule, offset))
        a2 = float(alpha_dash(taus[2 * j - 3], steps, schedule, offset)) if j > 1 else 1.0
        for name, a in (("t", a0), ("t'", a1)):
            if not 0.0 <= a < 1.0:
                raise ValueError(f"distill_table: alpha({name}) = {a!r} of pair {j} is outside [0, 1)")
            if divides and not a > 0.0:
                raise ValueError(f"distill_table: alpha({name}) = 0 at pair {j}: the teacher's objective divides by sqrt(alpha)")
        if not 0.0 <= a2 <= 1.0:
            raise ValueError(f"distill_table: alpha(t'') = {a2!r} of pair {j} is outside [0, 1]")
        (sa0, sb0), (sa1, sb1), (sa2, sb2) = ((math.sqrt(a), math.sqrt(1.0 - a)) for a in (a0, a1, a2))
        r = sb2 / sb0
        den = sa2 - r * sa0
        if not f32(den) > 0:
            raise ValueError(f"distill_table: den = {den!r} at pair {j} (t, t', t'' = {t}, {t1}, {taus[2 * j - 3] if j > 1 else None}): "
                             "alpha must decrease strictly along the grid")
        A0, A1 = f32(a0), f32(a1)
        tab[j - 1] = [f32(sa0), f32(sb0), f32(sa1), f32(sb1), f32(sa2), f32(sb2), f32(r), f32(den),
                      np.sqrt(A0), np.sqrt(f32(1.0) - A0), np.sqrt(A1), np.sqrt(f32(1.0) - A1)]
        tt[j - 1] = [t, t1]
    return tab, tt


def check_mask(mask, n: int, H: int, W: int) -> torch.Tensor:
    """an inpainting mask as contiguous fp32 [n,H,W] (on the mask's device): [H,W] is shared by the n images, [n,H,W] and [n,H,W,1]
    carry one per image.  1 regenerates a pixel, 0 keeps it (gct2_diffusion_step_masked).  ValueError for any other shape."""
    m = torch.as_tensor(mask)
    shape = tuple(m.shape)
    if shape == (H, W):
        m = m[None].expand(n, H, W)
    elif shape == (n, H, W, 1):
        m = m[..., 0]
    elif shape != (n, H, W):
        raise ValueError(f"mask must be [H,W], [n,H,W] or [n,H,W,1] = [{n},{H},{W}(,1)], got {list(shape)}")
    return m.to(torch.float32).contiguous()


# ---- image metrics of evaluation (Keras compile(metrics=[...]); gct2_image_metrics) ---------------------------------------------------
# "mse_x0": the mean squared error of the x0 estimate against the clean image; "psnr", "ssim": tf.image.psnr / tf.image.ssim [TF] of
# the same pair.  Images live in [-1, 1): max_val = 2
METRICS = ("mse_x0", "psnr", "ssim")
METRICS_MAX_VAL, METRICS_K1, METRICS_K2 = 2.0, 0.01, 0.03


def check_metrics(names) -> Tuple[str, ...]:
    """metric names as a tuple (None and () are no metrics; one string is one name); an unknown or repeated name is a ValueError"""
    if names is None:
        return ()
    names = (names,) if isinstance(names, str) else tuple(names)
    for k, n in enumerate(names):
        if not isinstance(n, str) or n not in METRICS:
            raise ValueError(f"unknown metric {n!r} (one of {', '.join(METRICS)})")
        if n in names[:k]:
            raise ValueError(f"metric {n!r} is named twice")
    return names


def ssim_window(K: int = 11, sigma: float = 1.5) -> np.ndarray:
    """the 1-D taps of tf.image.ssim's Gaussian window [TF], float32 [K]: exp(-((i - (K - 1) / 2)^2) / (2 sigma^2)), normalised in
    float64 and then rounded once"""
    K = int(K)
    if not 1 <= K <= 16:
        raise ValueError(f"ssim_window: filter_size must lie in 1..16, got {K!r}")
    if not (float(sigma) > 0.0 and math.isfinite(float(sigma))):
        raise ValueError(f"ssim_window: filter_sigma must be a finite float > 0, got {sigma!r}")
    i = np.arange(K, dtype=np.float64) - (K - 1) / 2.0
    g = np.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    return (g / g.sum()).astype(np.float32)


def x0_mode(predict_x: bool, predict_scaled_epsilon: bool, ordinary_differential_equation: bool, predict_v: bool = False) -> int:
    """the gct2_diffusion_update mode of the objective switches (sampler.sample_mode: predict_v first - it ignores predict_x and
    refuses the other two -, then ODE, then predict_x, then the epsilon forms)"""
    if check_predict_v(predict_v, predict_scaled_epsilon, False, ordinary_differential_equation):
        return _lib.SAMPLE_V
    if ordinary_differential_equation:
        return _lib.SAMPLE_ODE
    if predict_x:
        return _lib.SAMPLE_X
    return _lib.SAMPLE_SCALED_EPS if predict_scaled_epsilon else _lib.SAMPLE_EPS


def x0_tables(steps: int, mode: int, schedule=None, offset: float = 0.0) -> Optional[Tuple[np.ndarray, np.ndarray]]:
    """float32 (u, v), [steps + 1] each: entry t holds the coefficients of x0 = u noised + v pred at timestep t (x0_coefficients);
    entry 0 is never gathered and holds zeros.  None for SAMPLE_X.  Every coefficient is formed from Python floats and rounded once."""
    if mode == _lib.SAMPLE_X:
        return None
    if mode not in (_lib.SAMPLE_EPS, _lib.SAMPLE_SCALED_EPS, _lib.SAMPLE_ODE, _lib.SAMPLE_V):
        raise ValueError(f"x0_tables: unknown mode {mode!r}")
    steps = int(steps)
    u, v = np.zeros(steps + 1, dtype=np.float32), np.zeros(steps + 1, dtype=np.float32)
    name = noise_schedule_name(check_noise_schedule(schedule, offset)[0])
    for t in range(1, steps + 1):
        a = float(alpha_dash(float(t), steps, schedule, offset))
        a1 = float(alpha_dash(float(t) - 1, steps, schedule, offset)) if mode == _lib.SAMPLE_ODE else a
        if not (0.0 <= a <= 1.0 and 0.0 <= a1 <= 1.0):
            raise ValueError(f"x0_tables: noise schedule {name!r} leaves [0, 1] at timestep {t} (alpha = {a!r})")
        try:
            if mode == _lib.SAMPLE_ODE:
                den = a1 ** 0.5 * (1 - a) ** 0.5 - a ** 0.5 * (1 - a1) ** 0.5
                uu, vv = -((1 - a1) ** 0.5) / den, (1 - a) ** 0.5 / den
            elif mode == _lib.SAMPLE_EPS:
                uu, vv = 1.0 / a ** 0.5, -((1 - a) ** 0.5) / a ** 0.5
            elif mode == _lib.SAMPLE_V:
                uu, vv = a ** 0.5, -((1 - a) ** 0.5)
            else:
                uu, vv = 1.0 / a ** 0.5, -1.0 / a ** 0.5
        except ZeroDivisionError:
            raise ValueError(f"x0_tables: the x0 estimate divides by zero at timestep {t} under noise schedule {name!r} (alpha = {a!r})") from None
        with np.errstate(over="ignore"):
            u[t], v[t] = uu, vv
    if not (np.isfinite(u).all() and np.isfinite(v).all()):
        raise ValueError(f"x0_tables: the x0 estimate has a coefficient beyond float32 under noise schedule {name!r}")
    return u, v


def x0_coefficients(t_int, steps: int, mode: int, schedule=None, offset: float = 0.0, tables=None):
    """per-image float32 (u, v) with x0 = u noised + v pred, the x_theta of gct2_diffusion_update (train.py:382-413) at each image's own
    timestep; (None, None) for SAMPLE_X (x0 = pred).  With a = alpha_dash(t) and a1 = alpha_dash(t - 1):
        SAMPLE_EPS         u = 1 / sqrt(a),  v = -sqrt(1 - a) / sqrt(a)
        SAMPLE_SCALED_EPS  u = 1 / sqrt(a),  v = -1 / sqrt(a)
        SAMPLE_ODE         D = sqrt(a1) sqrt(1 - a) - sqrt(a) sqrt(1 - a1),  u = -sqrt(1 - a1) / D,  v = sqrt(1 - a) / D
        SAMPLE_V           u = sqrt(a),  v = -sqrt(1 - a)
    each formed per timestep from Python floats (alpha_dash(t, steps, schedule, offset)), the way the sampler forms its coefficients,
    rounded to float32 once and gathered by t.  t_int: a tensor (the result stays on its device) or an array of integers in 1..steps;
    tables: the two [steps + 1] vectors of x0_tables already where t_int lives (an engine keeps them)."""
    if mode == _lib.SAMPLE_X:
        return None, None
    if torch.is_tensor(t_int):
        if tables is None:
            tables = tuple(torch.from_numpy(h).to(t_int.device) for h in x0_tables(steps, mode, schedule, offset))
        idx = t_int.to(torch.int64).clamp(0, int(steps))
        return tables[0].index_select(0, idx).contiguous(), tables[1].index_select(0, idx).contiguous()
    if tables is None:
        tables = x0_tables(steps, mode, schedule, offset)
    idx = np.asarray(t_int).astype(np.int64)
    return tables[0][idx], tables[1][idx]


def loss_by_timestep(per_image, t, steps: int, bins: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(counts int64 [bins], means float64 [bins]) of per-image losses grouped by timestep: which timesteps are hard.  Any per-image
    vector bins the same way: the per_image_psnr or per_image_ssim of Trainer.evaluate(metrics=...) give PSNR / SSIM by timestep.  per_image and
    t: N values each (arrays or tensors; t integers in 1..steps).  bins=None: one bin per timestep (bin k holds t = k + 1); else
    `bins` equal-width groups, timestep t in bin (t - 1) * bins // steps.  Host only, numpy float64; an empty bin's mean is NaN."""
    as_np = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    loss, tt = as_np(per_image).astype(np.float64).reshape(-1), as_np(t).reshape(-1)
    steps = int(steps)
    nb = steps if bins is None else int(bins)
    if steps < 1 or not 1 <= nb <= steps:
        raise ValueError(f"loss_by_timestep: bins = {bins!r} must lie in 1..steps = {steps}")
    if tt.shape != loss.shape:
        raise ValueError(f"loss_by_timestep: {loss.size} losses for {tt.size} timesteps")
    if tt.size and not np.issubdtype(tt.dtype, np.integer):
        raise ValueError(f"loss_by_timestep: timesteps must be integers, got {tt.dtype}")
    tt = tt.astype(np.int64)
    if tt.size and (tt.min() < 1 or tt.max() > steps):
        raise ValueError(f"loss_by_timestep: timesteps outside 1..{steps}")
    which = (tt - 1) * nb // steps
    counts = np.bincount(which, minlength=nb).astype(np.int64)
    sums = np.bincount(which, weights=loss, minlength=nb).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        means = np.where(counts > 0, sums / np.maximum(counts, 1), np.nan)
    return counts, means


def check_timesteps(t, batch: int, steps: int) -> list:
    """the timesteps of a batch for the per-timestep heads (train.py:211-214: tf.gather(prediction, t - 1, batch_dims=3)) as a list
    of `batch` Python ints in 1..steps.  t: one integer (every image), or a sequence / tensor / array of `batch` integers (a single
    element broadcasts, like the [1] tensor of log_sample).  ValueError for anything else: a float, a bool, a wrong length, a value
    outside 1..steps - the gather of the reference would read past the tensor there"""
    if torch.is_tensor(t):
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError(f"timesteps must be integers, got a tensor of {t.dtype}")
        vals = t.detach().reshape(-1).cpu().tolist()
    elif isinstance(t, np.ndarray):
        if not np.issubdtype(t.dtype, np.integer):
            raise ValueError(f"timesteps must be integers, got an array of {t.dtype}")
        vals = t.reshape(-1).tolist()
    elif isinstance(t, (list, tuple)):
        vals = list(t)
    else:
        vals = [t]
    for v in vals:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"timesteps must be integers, got {v!r}")
    if len(vals) == 1:
        vals = vals * batch
    if len(vals) != batch:
        raise ValueError(f"{len(vals)} timesteps for a batch of {batch}")
    vals = [int(v) for v in vals]
    for v in vals:
        if not 1 <= v <= steps:
            raise ValueError(f"timestep {v} outside 1..{steps}")
    return vals


def dct_basis(size: int) -> np.ndarray:
    """G of gct2_loss_fwd_bwd's DCT kind for the reference's dct2d (train.py:254-260): tf.signal.dct(norm='ortho') [TF] times
    frequency_weights = 1 / (k + 1), G[k, m] = 1/(k+1) * sigma_k * cos(pi (2m + 1) k / (2 size)), sigma_0 = sqrt(1/size), else
    sqrt(2/size); formed in float64 and rounded once to float32 [size, size]."""
    k = np.arange(size, dtype=np.float64)[:, None]
    m = np.arange(size, dtype=np.float64)[None, :]
    sigma = np.where(k == 0, math.sqrt(1.0 / size), math.sqrt(2.0 / size))
    return (sigma / (k + 1.0) * np.cos(np.pi * (2.0 * m + 1.0) * k / (2.0 * size))).astype(np.float32)


HEAD_INITIALIZERS = ("glorot_uniform", "zeros")       # train.py:199: the head's kernel_initializer (the default) / '#kernel_initializer='zeros''


def check_head_options(who: str, hidden_dense, timestep_heads, head_initializer) -> None:
    """the constructor arguments that shape the head, checked before anything is allocated"""
    if head_initializer not in HEAD_INITIALIZERS:
        raise ValueError(f"{who}: head_initializer must be one of {HEAD_INITIALIZERS}, got {head_initializer!r}")
    if hidden_dense and timestep_heads:
        raise ValueError(f"{who}: hidden_dense=True (the Dense(pixel_size, relu) layer of train.py:195-197) together with timestep_heads=True "
                         "(Dense(3 * steps) gathered by t, train.py:199-214) is not built: switch one of the two off")


def check_hidden_marker(sd: dict, hidden_dense: bool) -> None:
    """a checkpoint written with / without the hidden Dense layer against an engine of the other shape: refused, nothing is loaded"""
    have = "hidden_dense" in sd
    if have != bool(hidden_dense):
        say = lambda on: "the hidden Dense(pixel_size, relu) layer in front of the head" if on else "the plain head (no hidden Dense layer)"
        raise ValueError(f"the checkpoint holds {say(have)} and this engine {say(bool(hidden_dense))}: dense_hidden.w / dense_hidden.b exist "
                         "only with the layer and dense.w has another shape (hidden_dense is fixed when an engine is built; nothing is loaded)")


class TrainerState:
    """what a train-step engine holds besides its network: constructor arguments checked, then plain attributes that
    `Trainer.compile()` may rewrite between steps (base_lr, warm_up, beta_1, beta_2, epsilon) and `Trainer` sets before every
    step (the four objective switches of train.py:29-32; defaults = the reference's: the network predicts the clean image)."""

    # exponential moving average of the parameters (Keras Adam(use_ema=True) [TF]): off by default (class-level defaults: an engine
    # that never switches it on carries no state for it); enable_ema() / disable_ema() write them.  The averages themselves and the
    # switch between the two weight sets live where weight pointers are resolved (ParamArena / _Net): the three names below read them
    use_ema, ema_momentum = False, 0.99
    # gradient clipping (Keras Adam(clipnorm / global_clipnorm / clipvalue) [TF]): off by default, set_clipping() writes the pair; the
    # reduction's segment table and buffers (_clip_reduction) exist only after the first norm-clipped step
    clip_mode, clip = _lib.CLIP_NONE, 0.0
    _clip_table = None
    # the optimizer (train.py:67-78): Keras Adam by default; set_optimizer() switches to "sgd" (momentum, nesterov) or "rmsprop" (rho,
    # momentum, the engine's epsilon), which run on the non-fused optimizer path through gct2_optimizer_apply.  lr_schedule: None =
    # WarmUp of base_lr / warm_up (a constant is warm_up = 0), or ("inverse_time_decay", initial, decay_steps, decay_rate, staircase)
    optimizer_kind, momentum, nesterov, rho = "adam", 0.0, False, 0.9
    lr_schedule: Optional[tuple] = None
    # the training loss (train.py:254-280): one of TRAINING_LOSSES; `Trainer` sets it before every step from the module global.  "mse"
    # is gct2_mse_fwd_bwd (or the fused heads) as ever; the other kinds go through gct2_loss_fwd_bwd, whose scratch (and the DCT basis)
    # an engine allocates on first use of such a kind (_loss_resources)
    training_loss = "mse"
    # the L2 weight regularizer (train.py:80, tf.keras.regularizers.l2 as kernel_regularizer and bias_regularizer [TF]) and the
    # optimizer's gradient transformer (train.py:47-48, 71-74: sign_gradient): off by default, set_regularizer() /
    # set_gradient_transform() write them.  `l2` is the factor as the float32 Keras holds.  With either on, the step takes the
    # non-fused optimizer path through gct2_optimizer_apply_reg; the penalty's reduction, its two output scalars and the per-tensor
    # coefficient tables exist only after the first regularized step
    l2, grad_transform = 0.0, "none"
    _l2_state = None
    _reg_tables = None
    # per-timestep output heads (train.py:199, 203, 211-214: Dense(3 * steps), Reshape(.., steps, 3), tf.gather(prediction, t - 1,
    # batch_dims=3)): off by default; an ENGINE CONSTRUCTOR argument, because it decides the shape of dense.w / dense.b and with them
    # the arena layout.  With it on the head runs on the non-fused path through gct2_dense_steps_fwd / gct2_dense_steps_bwd, which
    # read the device-resident t_int of the step (or the one predict / the sampler wrote); single GPU only
    timestep_heads = False
    # the hidden Dense(pixel_size, relu) layer in front of the head (train.py:195-197, commented out in the reference): off by default;
    # an ENGINE CONSTRUCTOR argument like timestep_heads (it adds dense_hidden.w / dense_hidden.b and changes dense.w's shape).  With
    # it on the head pair runs through gct2_dense2_fwd / gct2_dense2_bwd on the non-fused head path; single GPU only, and not
    # together with timestep_heads
    hidden_dense = False
    # the noise schedule (train.py:85-93: which `return` of alpha_dash is live, and its offset): a NOISE_SCHEDULES name or a callable,
    # set_noise_schedule() writes the pair.  The default keeps the formula kernels (gct2_noise_image / _rng) and the torch formula of
    # the objective; any other goes through gct2_noise_image_table / _rng_table and host-built tables, which exist only after the
    # first use of such a schedule
    noise_schedule, alpha_dash_offset = "quadratic", 0.0
    _noise_tables = None
    # the image metrics of evaluation (evaluate_batch(metrics=...)): the [steps + 1] coefficient tables of the x0 estimate per (mode,
    # schedule, offset) and the SSIM window, on the device; they exist only after the first evaluation that asks for a metric
    _x0_tables = None
    # the v objective (Salimans & Ho 2022; configure(predict_v=True)): the network predicts v = sqrt(alpha) eps - sqrt(1 - alpha) x, the
    # target fits the (a, c, w) contract as (-sb, sa, 1) and neither estimate divides by a schedule root.  `Trainer` sets it before
    # every step; predict_x is ignored while it is on
    predict_v = False
    # per-timestep loss weights (configure(loss_weighting=..., min_snr_gamma=...)): None (off), "min_snr", a callable f(snr, t) or a
    # tuple of `steps` floats; set_loss_weighting() writes the pair.  With weights on the step is eager, takes the non-fused head path
    # and computes loss and gradient through gct2_objective_loss_fwd_bwd; the [steps + 1] tables exist only after the first use
    loss_weighting, min_snr_gamma = None, 5.0
    _weight_tables = None

    @property
    def _ema(self) -> Optional[torch.Tensor]:
        """fp32, arena length; None while the averages are off"""
        return self._ema_tensors()[0]

    @property
    def _ema_shadow(self) -> Optional[torch.Tensor]:
        """compute dtype (None in fp32 mode and while the averages are off)"""
        return self._ema_tensors()[1]

    @property
    def _ema_reading(self) -> bool:
        """inside ema_weights(): the forward launches read the averages"""
        return self._ema_selected()

    def __init__(self, dtype: int, device: Optional[torch.device], steps: int, base_lr: float, warm_up: int, beta_1: float,
                 beta_2: float, epsilon: float, loss_scaling: bool, rng_seed: int, predict_x: bool, predict_scaled_epsilon: bool,
                 prediction_weighting: bool, ordinary_differential_equation: bool, f32_matrix: bool, predict_v: bool = False):
        who = type(self).__name__
        check_predict_v(predict_v, predict_scaled_epsilon, prediction_weighting, ordinary_differential_equation)
        if f32_matrix and dtype != F32:
            raise ValueError(f"{who}: f32_matrix selects the fp32 matrix-core kernels and needs dtype F32")
        self.lib = _lib.load()
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise _lib.Gct2Error(f"{who} needs a HIP device (torch device 'cuda'); there is no CPU path")
        if self.device.index is None:                       # ("cuda" without an index: the current device - the stream registry keys on it)
            self.device = torch.device("cuda", torch.cuda.current_device())
        call("gct2_device_check")
        self.dtype, self.steps = dtype, steps
        # fp32 convolutions on the matrix cores (gct2_ctx_set_f32_math) in every call context the engine creates (_new_ctx); fixed at
        # construction, so neither the step-plan key nor the sampler's graph cache needs it beyond the contexts' versions
        self._f32_matrix = bool(f32_matrix)
        self.base_lr, self.warm_up = base_lr, warm_up
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon
        self.predict_x, self.predict_scaled_epsilon = predict_x, predict_scaled_epsilon
        self.prediction_weighting, self.ordinary_differential_equation = prediction_weighting, ordinary_differential_equation
        if predict_v:
            self.predict_v = True
        self.rng_seed, self.rng_offset_t, self.rng_offset_eps = rng_seed, 0, 0
        self._iterations = 0           # optimizer.iterations [TF] (with loss scaling the counter lives on the device)
        self.loss_scaling = loss_scaling
        self.ls_state = None
        if loss_scaling:
            self.enable_loss_scaling()

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    @property
    def f32_matrix(self) -> bool:
        """fp32 convolutions run on the matrix cores (constructor argument; read-only)"""
        return self._f32_matrix

    def _new_ctx(self) -> "_lib.Context":
        """every call context of an engine comes from here: the engine-wide settings of a context (the fp32 math mode) are applied once"""
        c = _lib.Context()
        if self._f32_matrix:
            c.set_f32_math(_lib.F32_MATH_MFMA)
        return c

    # ---- the objective (train.py:238-252) ------------------------------------------------------------------------------------
    def default_objective(self) -> bool:
        return not self.predict_v and default_objective(self.predict_x, self.ordinary_differential_equation)

    def objective_weighted(self) -> bool:
        return objective_weighted(self.predict_x, self.prediction_weighting, self.ordinary_differential_equation)

    def objective_coefficients(self, t_int: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        if self._default_schedule():
            return objective_coefficients(t_int, self.steps, *(getattr(self, k) for k in OBJECTIVE_SWITCHES), predict_v=self.predict_v)
        return objective_coefficients(t_int, self.steps, *(getattr(self, k) for k in OBJECTIVE_SWITCHES), schedule=self.noise_schedule,
                                      offset=self.alpha_dash_offset, roots=self._schedule_tables()[1:], predict_v=self.predict_v)

    # ---- per-timestep loss weights (min-SNR-gamma, Hang et al. 2023; a callable; a table) --------------------------------------------
    def set_loss_weighting(self, kind=None, gamma: float = 5.0) -> None:
        """which lambda(t) multiplies every image's loss: None (off), "min_snr" with its gamma, a callable f(snr, t) or a sequence of
        `steps` floats (loss_weight_table).  The table is formed here on the host, so an unknown name, a weight that is negative or not
        finite, a table of the wrong length, the named kind under an objective it is not defined for or a training loss the weighted
        kernel does not compute is a ValueError before anything changes or is launched.  A setting like set_noise_schedule: it holds
        from the next step on.  Optimizer launches the engine holds back are flushed first."""
        kind, gamma = check_loss_weighting(kind, gamma)
        why = getattr(self, "_weighting_forbidden", None)
        if why and kind is not None:
            raise ValueError(why)
        if kind is not None:
            self._weight_host(kind, gamma)
            self._check_weighted_loss(kind)
        self.flush_deferred()
        self.loss_weighting, self.min_snr_gamma = kind, gamma

    def _check_weighted_loss(self, kind) -> None:
        if kind is not None and self.training_loss not in WEIGHTED_TRAINING_LOSSES:
            raise ValueError(f"loss_weighting with training_loss {self.training_loss!r}: per-timestep weights are built for "
                             f"{' and '.join(WEIGHTED_TRAINING_LOSSES)} (gct2_objective_loss_fwd_bwd)")

    def _weighting_objective(self) -> Optional[str]:
        return weighting_objective(*(getattr(self, k) for k in OBJECTIVE_SWITCHES), predict_v=self.predict_v)

    def _weight_host(self, kind, gamma: float) -> dict:
        """the host table of (kind, gamma, schedule, offset, steps, objective), formed once per engine (a callable is held by the key)"""
        if self._weight_tables is None:
            self._weight_tables = {}
        objective = self._weighting_objective()
        key = (kind, float(gamma) if isinstance(kind, str) else 0.0, self.noise_schedule, float(self.alpha_dash_offset), int(self.steps),
               objective if isinstance(kind, str) else None)
        if key not in self._weight_tables:
            self._weight_tables[key] = dict(host=loss_weight_table(kind, gamma, self.steps, objective, self.noise_schedule,
                                                                   self.alpha_dash_offset))
        return self._weight_tables[key]

    def check_step_settings(self) -> None:
        """the settings `Trainer` rewrites between steps, checked together before a step, a Trainer.call or an evaluation launches
        anything: predict_v against the other switches, the weighting against the objective and the training loss (ValueError)"""
        check_predict_v(self.predict_v, self.predict_scaled_epsilon, self.prediction_weighting, self.ordinary_differential_equation)
        if self.loss_weighting is not None:
            self._check_weighted_loss(self.loss_weighting)
            self._weight_host(self.loss_weighting, self.min_snr_gamma)

    def _loss_weights(self, t_int: torch.Tensor) -> Optional[torch.Tensor]:
        """per-image float32 lambda(t) of the weighting as it stands, gathered by t from the table on the device (uploaded once per
        key); None while the weighting is off"""
        if self.loss_weighting is None:
            return None
        entry = self._weight_host(self.loss_weighting, self.min_snr_gamma)
        if "device" not in entry:
            entry["device"] = torch.from_numpy(entry["host"]).to(self.device)
        return entry["device"].index_select(0, t_int.to(torch.int64).clamp(0, self.steps)).contiguous()

    def _objective_loss_launch(self, store: dict, pred: torch.Tensor, x: torch.Tensor, eps: Optional[torch.Tensor], t_int: torch.Tensor,
                               dpred: Optional[torch.Tensor], loss: torch.Tensor, stream: int) -> tuple:
        """gct2_objective_loss_fwd_bwd of the current objective, training loss ("mse" / "l1") and weighting on an fp32 [B,H,W,C]
        prediction: the target is formed inside the kernel from x and eps, no target plane is written; dpred = None: the loss only.
        Returns the per-image vectors (a, c, w, lam) it read: the caller keeps them alive until the stream has passed the launch."""
        B, H, W, Cc = pred.shape
        code = training_loss_code(self.training_loss)
        key = ("objective", B, H, W, Cc)
        if key not in store:
            need = C.c_size_t(0)
            _lib.check(self.lib.gct2_objective_loss_scratch(code, B, H, W, Cc, C.byref(need)), "gct2_objective_loss_scratch")
            store[key] = torch.zeros(need.value, dtype=torch.float32, device=self.device)
        scratch = store[key]
        a = c = w = None
        if not self.default_objective():
            a, c, w = self.objective_coefficients(t_int)
            if not self.objective_weighted():
                w = None
        lam = self._loss_weights(t_int)
        ptr = lambda v: None if v is None else v.data_ptr()
        call("gct2_objective_loss_fwd_bwd", code, pred.data_ptr(), x.data_ptr(), None if a is None else eps.data_ptr(), ptr(a), ptr(c), ptr(w),
             ptr(lam), ptr(dpred), loss.data_ptr(), scratch.data_ptr(), scratch.numel(), B, H, W, Cc, self._ls_ptr(), stream)
        return a, c, w, lam

    # ---- the noise schedule (train.py:85-93) ------------------------------------------------------------------------------------
    def set_noise_schedule(self, schedule="quadratic", offset: float = 0.0) -> None:
        """which body of alpha_dash is live: a NOISE_SCHEDULES name or a callable f(t01) -> alpha, and the offset added behind it.
        Both tables are formed here on the host, so an unknown name, a non-finite offset, an alpha outside [0, 1] or a formula that
        overflows in this engine's arithmetic (float16 for F16) is a ValueError before anything changes or is launched.  A setting like
        set_regularizer: it holds from the next step on.  Optimizer launches the engine holds back are flushed first."""
        schedule, offset = check_noise_schedule(schedule, offset)
        if not default_noise_schedule(schedule, offset):
            self._schedule_host(schedule, offset)
        self.flush_deferred()
        self.noise_schedule, self.alpha_dash_offset = schedule, offset

    def _default_schedule(self) -> bool:
        return default_noise_schedule(self.noise_schedule, self.alpha_dash_offset)

    def _schedule_host(self, schedule, offset: float) -> dict:
        """the host tables of (schedule identity, offset, steps, dtype), formed once per engine (a callable is held by the key, so
        its identity cannot be recycled)"""
        if self._noise_tables is None:
            self._noise_tables = {}
        key = (schedule, float(offset), int(self.steps), int(self.dtype))
        if key not in self._noise_tables:
            self._noise_tables[key] = dict(host=(noise_table(schedule, offset, self.steps, self.dtype),) + alpha_roots(schedule, offset, self.steps))
        return self._noise_tables[key]

    def _schedule_tables(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(coef [steps, 2], sqrt(alpha) [steps + 1], sqrt(1 - alpha) [steps + 1]) of the current schedule on the device: uploaded on
        first use and kept for the engine's lifetime (step plans hold the address of coef)"""
        entry = self._schedule_host(self.noise_schedule, self.alpha_dash_offset)
        if "device" not in entry:
            entry["device"] = tuple(torch.from_numpy(h).to(self.device) for h in entry["host"])
        return entry["device"]

    def _noise_coef_ptr(self) -> int:
        """the coef argument of gct2_noise_image_table / _rng_table"""
        return self._schedule_tables()[0].data_ptr()

    # ---- the training losses besides the plain MSE (train.py:254-280) -------------------------------------------------------------
    def _loss_resources(self, store: dict, B: int, H: int, W: int, Cc: int = 3) -> Tuple[int, torch.Tensor, Optional[torch.Tensor]]:
        """(kind code, scratch, basis or None) of gct2_loss_fwd_bwd for the current training_loss and this shape: allocated on first use
        and kept in `store` (a buffer set's, or the variant engine's).  A shape the kind refuses (pooled MSE off the 16-pixel grid, a
        DCT of a non-square image) raises here, before anything is launched."""
        code = training_loss_code(self.training_loss)
        key = (code, B, H, W, Cc)
        if key not in store:
            need = C.c_size_t(0)
            _lib.check(self.lib.gct2_loss_scratch(code, B, H, W, Cc, C.byref(need)), "gct2_loss_scratch")
            scratch = torch.zeros(need.value, dtype=torch.float32, device=self.device)
            basis = torch.from_numpy(dct_basis(H)).to(self.device) if code == _lib.LOSS_DCT else None
            store[key] = (scratch, basis)
        return (code,) + store[key]

    def _loss_launch(self, store: dict, pred: torch.Tensor, target, dpred: Optional[torch.Tensor], loss: torch.Tensor, stream: int) -> None:
        """gct2_loss_fwd_bwd of the current (non-"mse") training_loss on an fp32 [B,H,W,C] prediction; target: a device address or a Slot
        holding one; dpred = None: the loss only"""
        B, H, W, Cc = pred.shape
        code, scratch, basis = self._loss_resources(store, B, H, W, Cc)
        call("gct2_loss_fwd_bwd", code, pred.data_ptr(), target, dpred.data_ptr() if dpred is not None else None, loss.data_ptr(),
             scratch.data_ptr(), scratch.numel(), B, H, W, Cc, basis.data_ptr() if basis is not None else None, self._ls_ptr(), stream)

    # ---- evaluation: the training loss per held-out image (Keras Model.evaluate / fit(validation_data=...)) ----------------------------
    # what an engine provides: _eval_buffers(B, H, W) -> (t_int int32 [B], eps fp32 [B,H,W,3], store dict), device tensors the engine
    # keeps per shape; _eval_noise(x, t_int, eps, draw) -> the noised network input, stored where its forward pass reads it (draw None:
    # eps holds the noise; else (seed, offset, keep): drawn inside the noising kernel from stream EVAL_STREAM_EPS, written to eps only
    # when keep); _eval_forward(noised, t_int) -> the fp32 [B,H,W,3] prediction, optimizer launches held back flushed first
    def _eval_resources(self, store: dict, B: int, H: int, W: int, Cc: int = 3) -> Tuple[int, torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
        """(kind code, scratch, basis or None, rows [B]) of gct2_eval_loss_rows for the current training_loss and this shape: allocated
        on first use and kept in `store`; a shape the kind refuses raises here, before anything is launched"""
        code = training_loss_code(self.training_loss)
        key = ("eval", code, B, H, W, Cc)
        if key not in store:
            need = C.c_size_t(0)
            _lib.check(self.lib.gct2_eval_loss_scratch(code, B, H, W, Cc, C.byref(need)), "gct2_eval_loss_scratch")
            scratch = torch.zeros(max(4, need.value), dtype=torch.float32, device=self.device)
            basis = torch.from_numpy(dct_basis(H)).to(self.device) if code == _lib.LOSS_DCT else None
            store[key] = (scratch, basis)
        return (code,) + store[key]

    def _metrics_resources(self, store: dict, B: int, H: int, W: int, Cc: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scratch, window) of gct2_image_metrics for this shape: allocated on first use and kept in `store`"""
        key = ("metrics", B, H, W, Cc)
        if key not in store:
            window = ssim_window()
            need = C.c_size_t(0)
            _lib.check(self.lib.gct2_image_metrics_scratch(B, H, W, Cc, len(window), C.byref(need)), "gct2_image_metrics_scratch")
            store[key] = (torch.zeros(max(4, need.value), dtype=torch.float32, device=self.device), torch.from_numpy(window).to(self.device))
        return store[key]

    def _x0_coefficients(self, t_int: torch.Tensor) -> Tuple[int, Optional[torch.Tensor], Optional[torch.Tensor]]:
        """(mode, u, v) of x0_coefficients for the objective switches and the noise schedule as they stand"""
        mode = x0_mode(self.predict_x, self.predict_scaled_epsilon, self.ordinary_differential_equation, predict_v=self.predict_v)
        if mode == _lib.SAMPLE_X:
            return mode, None, None
        if self._x0_tables is None:
            self._x0_tables = {}
        key = (mode, self.noise_schedule, float(self.alpha_dash_offset), int(self.steps))
        if key not in self._x0_tables:
            host = x0_tables(self.steps, mode, self.noise_schedule, self.alpha_dash_offset)
            self._x0_tables[key] = tuple(torch.from_numpy(h).to(self.device) for h in host)
        return (mode,) + x0_coefficients(t_int, self.steps, mode, tables=self._x0_tables[key])

    def _noise_roots(self, t_int: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """per-image float32 (sqrt(alpha_dash(t)), sqrt(1 - alpha_dash(t))): the default schedule's torch formula, or the host tables"""
        if self._default_schedule():
            a = alpha_dash(t_int.to(torch.float32), self.steps)
            return a.sqrt().contiguous(), (1 - a).sqrt().contiguous()
        _, sa, sb = self._schedule_tables()
        idx = t_int.to(torch.int64).clamp(0, self.steps)
        return sa.index_select(0, idx).contiguous(), sb.index_select(0, idx).contiguous()

    def _eval_metrics(self, names: Tuple[str, ...], store: dict, x: torch.Tensor, pred: torch.Tensor, eps_buf: torch.Tensor,
                      t_int: torch.Tensor) -> dict:
        """gct2_image_metrics of the x0 estimate against the clean batch: {name: fp32 [B] device tensor} for `names`.  Under a
        non-default objective the fp32 noised image sqrt(a) x + sqrt(1 - a) eps is formed first (gct2_mix_per_image; eps is kept
        there) and x0 = u noised + v pred inside the metrics kernel; under the default one x0 is the prediction itself."""
        B, H, W, Cc = x.shape
        scratch, window = self._metrics_resources(store, B, H, W, Cc)
        s = self._stream()
        mode, u, v = self._x0_coefficients(t_int)
        noised32 = None
        if u is not None:
            sa, sb = self._noise_roots(t_int)
            key = ("metrics_noised", B, H, W, Cc)
            if key not in store:
                store[key] = torch.empty(B, H, W, Cc, dtype=torch.float32, device=self.device)
            noised32 = store[key]
            call("gct2_mix_per_image", x.data_ptr(), eps_buf.data_ptr(), sa.data_ptr(), sb.data_ptr(), noised32.data_ptr(), B, H * W * Cc, s)
        out = torch.empty(3, B, dtype=torch.float32, device=self.device)
        want_ssim = "ssim" in names
        call("gct2_image_metrics", pred.data_ptr(), None if u is None else noised32.data_ptr(), None if u is None else u.data_ptr(),
             None if u is None else v.data_ptr(), x.data_ptr(), window.data_ptr(), window.numel(), METRICS_MAX_VAL, METRICS_K1, METRICS_K2,
             out[0].data_ptr(), out[1].data_ptr() if "psnr" in names else None, out[2].data_ptr() if want_ssim else None,
             scratch.data_ptr(), scratch.numel(), B, H, W, Cc, s)
        self.last_eval["metrics"] = dict(mode=mode, u=u, v=v, noised=noised32, window=window)
        return {n: out[METRICS.index(n)] for n in names}

    def evaluate_batch(self, x: torch.Tensor, index0: int = 0, t=None, eps: Optional[torch.Tensor] = None,
                       seed: Optional[int] = None, metrics=()):
        """the training loss of every image of a held-out batch on its own: (rows fp32 [B], t_int int32 [B]), device tensors, no host
        synchronisation.  In exact arithmetic rows.mean() is what Trainer.call computes for the same t and eps.

        metrics: names out of METRICS (check_metrics); with any, the return value is (rows, t_int, {name: fp32 [B]}) - the image-space
        metrics of every image's x0 estimate (x0_coefficients) against the clean image, by one gct2_image_metrics launch on what the
        loss launch read.  With none, nothing changes: the same launches, the same return value, the same last_eval keys.

        The draws belong to evaluation alone and depend on the image, not on the batch: with seed (None: rng_seed), the image of
        global index i = index0 + k takes position i of Philox stream EVAL_STREAM_T for its timestep and positions
        [i*H*W*3, (i+1)*H*W*3) of stream EVAL_STREAM_EPS for its noise, however the validation set is cut into batches.  t: an int or B
        ints in 1..steps instead of the draw (check_timesteps); eps: injected noise, fp32 [B,H,W,3].

        A pure function of the weights: the training streams' offsets, iterations, the optimizer slots, the averages, the loss-scale
        state and the recorded step plans are left alone, nothing is scaled in place and the loss is never multiplied by a loss scale.
        Refused inside a plan recording."""
        if _lib._recording is not None:
            raise _lib.Gct2Error("evaluate_batch inside a plan recording: evaluation is not part of a train step")
        metrics = check_metrics(metrics)
        self.check_step_settings()
        if x.dim() != 4 or x.shape[-1] != 3:
            raise ValueError(f"expected an NHWC batch [B,H,W,3], got {tuple(x.shape)}")
        index0 = int(index0)
        if index0 < 0:
            raise ValueError(f"index0 must be >= 0, got {index0}")
        B, H, W, _ = x.shape
        vals = None if t is None else check_timesteps(t, B, self.steps)
        if eps is not None and tuple(eps.shape) != tuple(x.shape):
            raise ValueError(f"eps of shape {tuple(eps.shape)} for a batch of shape {tuple(x.shape)}")
        if x.dtype != torch.float32 or not x.is_contiguous() or x.device != self.device:
            x = x.to(self.device, torch.float32).contiguous()
        seed = int(self.rng_seed if seed is None else seed)
        t_int, eps_buf, store = self._eval_buffers(B, H, W)
        code, scratch, basis = self._eval_resources(store, B, H, W)
        rows = torch.empty(B, dtype=torch.float32, device=self.device)
        s = self._stream()
        if vals is None:
            call("gct2_rng_uniform_int", seed, EVAL_STREAM_T, index0, t_int.data_ptr(), B, 1, self.steps, s)
        else:
            t_int.copy_(torch.tensor(vals, dtype=torch.int32))
        default = self.default_objective()
        if eps is not None:
            eps_buf.copy_(eps.to(self.device, torch.float32))
            noised = self._eval_noise(x, t_int, eps_buf, None)
        else:
            noised = self._eval_noise(x, t_int, eps_buf, (seed, index0 * H * W * 3, not default))
        pred = self._eval_forward(noised, t_int)
        a = c = w = None
        if not default:                                        # train.py:238-252; the target is formed inside the loss kernel
            a, c, w = self.objective_coefficients(t_int)
            if not self.objective_weighted():
                w = None
        call("gct2_eval_loss_rows", code, pred.data_ptr(), x.data_ptr(), None if default else eps_buf.data_ptr(),
             None if a is None else a.data_ptr(), None if c is None else c.data_ptr(), None if w is None else w.data_ptr(), rows.data_ptr(),
             scratch.data_ptr(), scratch.numel(), B, H, W, 3, basis.data_ptr() if basis is not None else None, s)
        # what the launches read stays alive with the engine until the next evaluation (and is what the tests restate the rows from)
        self.last_eval = dict(x=x, pred=pred, eps=None if default and eps is None else eps_buf, t_int=t_int, coef=(a, c, w), noised=noised)
        lam = self._loss_weights(t_int)
        if lam is not None:                                    # the weighted rows: one op on [B]; the caller can divide by loss_weight
            rows = rows * lam
            self.last_eval["loss_weight"] = lam
        if metrics:
            return rows, t_int.clone(), self._eval_metrics(metrics, store, x, pred, eps_buf, t_int)
        return rows, t_int.clone()

    # ---- per-timestep heads (train.py:199, 203, 211-214) ------------------------------------------------------------------------
    def head_shapes(self, cin: int) -> Tuple[Tuple[int, int], Tuple[int]]:
        """(kernel, bias) shapes of the Dense head on `cin` channels: Dense(3), or Dense(3 * steps) with timestep_heads"""
        units = 3 * self.steps if self.timestep_heads else 3
        return (cin, units), (units,)

    def _steps_scratch(self, store: dict, B: int, HW: int, cin: int) -> torch.Tensor:
        """scratch of gct2_dense_steps_bwd for this shape (the partial rows of dw / db), allocated on first use and kept in `store`"""
        key = ("dense_steps", B, HW, cin)
        if key not in store:
            need = C.c_size_t(0)
            _lib.check(self.lib.gct2_dense_steps_scratch(B, HW, cin, 3, C.byref(need)), "gct2_dense_steps_scratch")
            store[key] = torch.zeros(need.value, dtype=torch.float32, device=self.device)
        return store[key]

    def _dense2_scratch(self, store: dict, M: int, cin: int, chid: int) -> torch.Tensor:
        """scratch of gct2_dense2_bwd for this shape (the partial rows of the four head gradients), allocated on first use and kept in `store`"""
        key = ("dense2", M, cin, chid)
        if key not in store:
            need = C.c_size_t(0)
            _lib.check(self.lib.gct2_dense2_scratch(M, cin, chid, 3, C.byref(need)), "gct2_dense2_scratch")
            store[key] = torch.zeros(need.value, dtype=torch.float32, device=self.device)
        return store[key]

    # ---- optimizer (train.py:50-65,75) ---------------------------------------------------------------------------------------
    def learning_rate(self, k: Optional[int] = None) -> float:
        k = self.iterations if k is None else k
        if self.lr_schedule is not None:
            return inverse_time_decay_lr(k, *self.lr_schedule[1:])
        return warmup_lr(k, self.base_lr, self.warm_up)

    def adam_alpha(self, k: Optional[int] = None) -> float:
        k = self.iterations if k is None else k
        return adam_step_size(self.learning_rate(k), k, self.beta_1, self.beta_2)

    def step_size(self, k: Optional[int] = None) -> float:
        """what multiplies the update of step k: Adam folds its bias correction into it, SGD and RMSprop take the learning rate"""
        return self.adam_alpha(k) if self.optimizer_kind == "adam" else self.learning_rate(k)

    def set_optimizer(self, kind: str = "adam", momentum: float = 0.0, nesterov: bool = False, rho: float = 0.9) -> None:
        """the optimizer kind and the hyper-parameters only SGD / RMSprop have (epsilon is the engine's, as for Adam).  Another KIND is
        allowed while no step has been applied: afterwards the slots hold the other optimizer's state (the rule of dropping loss
        scaling).  Optimizer launches the engine holds back are flushed first: they belong to a step made with the old setting."""
        kind, momentum, nesterov, rho = optimizer_hyper(kind, momentum, nesterov, rho)
        if kind != self.optimizer_kind:
            why = getattr(self, "_optimizer_forbidden", None)
            if why and kind != "adam":
                raise ValueError(why)
            if self.iterations != 0:
                raise _lib.Gct2Error(f"the engine has already applied {self.iterations} steps with {self.optimizer_kind}: its slots hold that "
                                     f"optimizer's state, the kind cannot become {kind} now")
        self.flush_deferred()
        self.optimizer_kind, self.momentum, self.nesterov, self.rho = kind, momentum, nesterov, rho

    # ---- dynamic loss scaling (train.py:82-83) -------------------------------------------------------------------------------
    def enable_loss_scaling(self, initial_scale: float = 2.0 ** 15) -> None:
        """tf.keras.mixed_precision.LossScaleOptimizer (train.py:82-83): allocate the device-side state (32-byte
        gct2_loss_scale_state).  Allowed until the first optimizer step, so `trainer(example)` may come before `compile`
        exactly as in train.py:505-514."""
        if self.ls_state is not None:
            return
        if self._iterations != 0:
            raise _lib.Gct2Error("loss scaling cannot be switched on after optimizer steps have been applied")
        self.loss_scaling = True
        self.ls_state = torch.zeros(8, dtype=torch.int32, device=self.device)
        call("gct2_loss_scale_init", self.ls_state.data_ptr(), float(initial_scale), self._stream())

    @property
    def iterations(self) -> int:
        """optimizer.iterations [TF].  Under LossScaleOptimizer a skipped step does not advance it, and whether a step was
        skipped is only known on the device: the counter lives there (gct2_loss_scale_state.applied_steps) and reading it
        synchronises."""
        if self.ls_state is not None:
            return int(self.ls_state[4].item())
        return self._iterations

    @iterations.setter
    def iterations(self, k: int) -> None:
        self._iterations = int(k)
        if self.ls_state is not None:
            self.ls_state[4] = int(k)

    def loss_scale(self) -> Tuple[float, int]:
        """(current scale, finite steps since it last changed)"""
        if self.ls_state is None:
            return 1.0, 0
        raw = self.ls_state.cpu()
        return float(raw[:1].view(torch.float32)[0]), int(raw[2])

    def _ls_ptr(self) -> Optional[int]:
        return self.ls_state.data_ptr() if self.ls_state is not None else None

    def begin_step(self) -> None:
        if self.ls_state is None:
            return
        adam = self.optimizer_kind == "adam"
        if adam and self.lr_schedule is None:              # the default step keeps its call
            call("gct2_loss_scale_begin", self.ls_state.data_ptr(), float(self.base_lr), int(self.warm_up), float(self.beta_1),
                 float(self.beta_2), self._stream())
        elif self.lr_schedule is None:
            call("gct2_loss_scale_begin_schedule", self.ls_state.data_ptr(), _lib.SCHEDULE_WARMUP, float(self.base_lr), float(self.warm_up),
                 0.0, 0, int(adam), float(self.beta_1), float(self.beta_2), self._stream())
        else:
            _, initial, decay_steps, decay_rate, staircase = self.lr_schedule
            call("gct2_loss_scale_begin_schedule", self.ls_state.data_ptr(), _lib.SCHEDULE_INVERSE_TIME_DECAY, initial, decay_steps,
                 decay_rate, int(staircase), int(adam), float(self.beta_1), float(self.beta_2), self._stream())

    def _check_finite(self, grads_ptr: int, n: int, stream: Optional[int] = None) -> None:
        if self.ls_state is not None:
            call("gct2_scale_check_finite", grads_ptr, n, self.ls_state.data_ptr(), self._stream() if stream is None else stream)

    # ---- gradient clipping (tf.keras.optimizers.Adam(clipnorm=..., global_clipnorm=..., clipvalue=...)) [TF] --------------------------
    # what an engine provides: _clip_segments() -> one (begin, count) per parameter tensor inside its gradient arena, in arena order
    # and without the alignment padding; _clip_device() -> where that arena lives
    def set_clipping(self, clipnorm: Optional[float] = None, global_clipnorm: Optional[float] = None, clipvalue: Optional[float] = None) -> None:
        """Keras' rule: at most one of the three, each > 0 and finite (ValueError); all None switches clipping off.  A hyper-parameter
        like beta_1: it holds from the next step on and is not part of a checkpoint.  Optimizer launches the engine holds back are
        flushed first: they belong to a step made with the old setting."""
        mode, value = clipping_mode(clipnorm, global_clipnorm, clipvalue)
        why = getattr(self, "_clip_forbidden", None)
        if why and mode != _lib.CLIP_NONE:
            raise ValueError(why)
        self.flush_deferred()
        self.clip_mode, self.clip = mode, value

    def _clip_by_norm(self) -> bool:
        """the step reduces the gradient arena first (gct2_grad_sumsq, which also sets the loss-scale state's found_inf)"""
        return self.clip_mode in (_lib.CLIP_NORM, _lib.CLIP_GLOBAL_NORM)

    def _clip_reduction(self):
        """(device segment table, nseg, npartials, partials, sumsq, [(begin, count)]) of gct2_grad_sumsq: laid out by
        gct2_sumsq_layout, uploaded and allocated on first use, kept for the engine's lifetime (step plans hold the addresses)"""
        if self._clip_table is None:
            self._clip_table = self._sumsq_tables(self._clip_segments())
        return self._clip_table

    def _sumsq_tables(self, segments):
        segs = [(int(b), int(c)) for b, c in segments]
        n = len(segs)
        begin, count = (C.c_uint64 * n)(*[b for b, _ in segs]), (C.c_uint64 * n)(*[c for _, c in segs])
        out, npartials = (C.c_uint64 * (3 * n))(), C.c_size_t(0)
        _lib.check(_lib.load().gct2_sumsq_layout(begin, count, n, out, C.byref(npartials)), "gct2_sumsq_layout")
        dev = self._clip_device()
        table = torch.tensor(list(out), dtype=torch.int64).to(dev)          # gct2_sumsq_seg[n]: three 64-bit words each
        return (table, n, int(npartials.value), torch.zeros(npartials.value, dtype=torch.float64, device=dev),
                torch.zeros(n + 1, dtype=torch.float64, device=dev), segs)

    # ---- L2 weight regularizer and gradient transformer (train.py:47-48, 71-74, 80) [TF] ------------------------------------------------
    # what an engine provides besides the clipping hooks: _l2_segments() -> the (begin, count) of the tensors that carry the
    # regularizer (default: every tensor; VariantEngine leaves Residual's bias-free projection out, train.py:107)
    def set_regularizer(self, l2: Optional[float] = None) -> None:
        """tf.keras.regularizers.l2(l2) on every kernel, bias and the Dense head [TF]: None or 0 switches it off, a negative or
        non-finite factor is a ValueError.  A setting like set_clipping: it holds from the next step on and is not part of a
        checkpoint.  Optimizer launches the engine holds back are flushed first: they belong to a step made with the old setting."""
        held, _ = l2_coefficients(l2)
        why = getattr(self, "_reg_forbidden", None)
        if why and held > 0.0:
            raise ValueError(why)
        self.flush_deferred()
        self.l2 = held

    def set_gradient_transform(self, name: str = "none") -> None:
        """the optimizer's gradient_transformers: "none", or "sign" (train.py:47-48), applied behind the clipping step as Keras'
        _transform_gradients does [TF].  A setting like set_regularizer."""
        if name not in GRADIENT_TRANSFORMS:
            raise ValueError(f"unknown gradient transform {name!r} (one of {', '.join(GRADIENT_TRANSFORMS)})")
        why = getattr(self, "_reg_forbidden", None)
        if why and name != "none":
            raise ValueError(why)
        self.flush_deferred()
        self.grad_transform = name

    def _regularized(self) -> bool:
        """the step's optimizer launches are gct2_optimizer_apply_reg's (and the step is not fused)"""
        return self.l2 > 0.0 or self.grad_transform != "none"

    def _l2_segments(self):
        return self._clip_segments()

    @property
    def regularization_loss(self) -> Optional[torch.Tensor]:
        """the penalty l2 * sum(w^2) of the last regularized train step, fp32 [1] on the device (None while the regularizer is off)"""
        return self._l2_state[1] if self.l2 > 0.0 and self._l2_state is not None else None

    def _reg_table(self, total: int):
        """(segments, per-tensor coefficients, runs, device copy of the coefficients) for the current l2: built on first use and kept
        for the engine's lifetime (step plans hold the device address)"""
        _, c = l2_coefficients(self.l2)
        if self._reg_tables is None:
            self._reg_tables = {}
        if c not in self._reg_tables:
            segs = [(int(b), int(n)) for b, n in self._clip_segments()]
            carry = {(int(b), int(n)) for b, n in self._l2_segments()} if c > 0.0 else set()
            assert carry <= set(segs), "_l2_segments() must name tensors of _clip_segments()"
            coeffs = [c if seg in carry else 0.0 for seg in segs]
            self._reg_tables[c] = (segs, coeffs, coefficient_runs(segs, coeffs, total),
                                   torch.tensor(coeffs, dtype=torch.float32).to(self._clip_device()))
        return self._reg_tables[c]

    # ---- the launches of a non-fused optimizer step: every kind, clipped or not, regularized or not ---------------------------------------
    def _update_launches(self, p: torch.Tensor, m: torch.Tensor, v: torch.Tensor, g: torch.Tensor, shadow: Optional[torch.Tensor], lo: int,
                         hi: int, grad_mul: float, stream: int) -> None:
        """the optimizer launches of every step that is not the plain fused Adam one, over arenas (tensors; shadow None in fp32 mode).
        The entry point: gct2_optimizer_apply_reg for every kind as soon as a regularizer or a transformer is on (Adam's betas ride in
        the momentum / rho positions), else gct2_adam_keras_clipped for Adam and gct2_optimizer_apply for SGD / RMSprop; only the slots
        the kind uses are handed over.  The sequence: for the two norm modes, which take the whole arena ([lo, hi) = [0, total)), the
        reduction first (gct2_grad_sumsq; gct2_grad_sumsq_l2 over the regularized gradient as soon as a coefficient is non-zero), then
        for clipnorm one update per tensor over exactly its elements, reading its own sum; otherwise one update per run of neighbouring
        tensors with the same coefficient inside [lo, hi) - ONE launch where every tensor carries the regularizer, or none does -
        reading the total under global_clipnorm"""
        ls_ptr = self._ls_ptr()
        lr = 0.0 if self.ls_state is not None else self.step_size()
        kind = OPTIMIZER_KINDS[self.optimizer_kind]
        adam, reg = kind == _lib.OPT_ADAM, self._regularized()
        use_m, use_v = adam or float(self.momentum) > 0.0, kind != _lib.OPT_SGD
        if reg:
            name, transform = "gct2_optimizer_apply_reg", GRADIENT_TRANSFORMS[self.grad_transform]
            _, coeffs, runs, dev_coeffs = self._reg_table(p.numel())         # (per tensor of _clip_segments(), the reduction's segments)
        else:
            name, coeffs, runs = "gct2_adam_keras_clipped" if adam else "gct2_optimizer_apply", None, [(lo, hi, 0.0)]
        if adam and not reg:
            head, hyper = (), (float(self.beta_1), float(self.beta_2))
        else:
            first, second = (self.beta_1, self.beta_2) if adam else (self.momentum, self.rho)
            head, hyper = (kind,), (float(first), int(bool(self.nesterov)), float(second))

        def launch(lo: int, n: int, sumsq_ptr: Optional[int], coeff: float) -> None:
            call(name, *head, p.data_ptr() + 4 * lo, m.data_ptr() + 4 * lo if use_m else None, v.data_ptr() + 4 * lo if use_v else None,
                 g.data_ptr() + 4 * lo, None if shadow is None else shadow.data_ptr() + 2 * lo, self.dtype, n, Slot("alpha", lr), *hyper,
                 float(self.epsilon), grad_mul, ls_ptr, self.clip_mode, float(self.clip), sumsq_ptr, *((coeff, transform) if reg else ()), stream)

        total_ptr = None
        if self._clip_by_norm():
            table, nseg, npartials, partials, sumsq, segs = self._clip_reduction()
            coeffs = coeffs or [0.0] * nseg
            if any(coeffs):
                call("gct2_grad_sumsq_l2", g.data_ptr(), p.data_ptr(), table.data_ptr(), dev_coeffs.data_ptr(), nseg, npartials, grad_mul,
                     ls_ptr, partials.data_ptr(), sumsq.data_ptr(), stream)
            else:
                call("gct2_grad_sumsq", g.data_ptr(), table.data_ptr(), nseg, npartials, grad_mul, ls_ptr, partials.data_ptr(),
                     sumsq.data_ptr(), stream)
            if self.clip_mode == _lib.CLIP_NORM:
                for s, ((begin, n), coeff) in enumerate(zip(segs, coeffs)):
                    launch(begin, n, sumsq.data_ptr() + 8 * s, coeff)
                return
            total_ptr = sumsq.data_ptr() + 8 * nseg
        for begin, end, coeff in runs:
            begin, end = max(begin, lo), min(end, hi)
            if end > begin:
                launch(begin, end - begin, total_ptr, coeff)

    def _fp32_parameters(self) -> torch.Tensor:
        """the raw fp32 parameter arena, laid out like the gradient arena (what the engines also hand to the averages: _ema_source)"""
        return self._ema_source()[0]

    def _penalty_begin(self, stream: int) -> None:
        """head of a regularized step: S = the fp64 sum of squares of the regularized tensors as the forward pass is about to read them
        (gct2_grad_sumsq pointed at the fp32 parameter arena, over a segment table, partials and sums of its own)"""
        if self._l2_state is None:
            dev = self._clip_device()
            self._l2_state = (self._sumsq_tables(self._l2_segments()), torch.zeros(1, dtype=torch.float32, device=dev),
                              torch.zeros(1, dtype=torch.float32, device=dev))
        (table, nseg, npartials, partials, sumsq, _), _, _ = self._l2_state
        p = self._fp32_parameters()
        call("gct2_grad_sumsq", p.data_ptr(), table.data_ptr(), nseg, npartials, 1.0, None, partials.data_ptr(), sumsq.data_ptr(), stream)

    def _penalty_finish(self, loss: torch.Tensor, stream: int) -> torch.Tensor:
        """behind the loss: what Keras' train_step reports, loss + l2 * S (gct2_l2_penalty); the data term stays where it is"""
        (_, nseg, _, _, sumsq, _), penalty, total = self._l2_state
        call("gct2_l2_penalty", loss.data_ptr(), sumsq.data_ptr() + 8 * nseg, float(self.l2), penalty.data_ptr(), total.data_ptr(), stream)
        return total

    # ---- exponential moving average of the parameters (tf.keras.optimizers.Adam(use_ema=True, ema_momentum=...)) [TF] -----------
    # what an engine provides: _ema_source() -> (fp32 parameter arena, compute-dtype copy or None), raw storage;
    # _ema_tensors() -> (averages, their compute-dtype copy or None) and _ema_attach(ema, ema_shadow), which stores them with whoever
    # resolves weight pointers (ParamArena / _Net); _ema_select(on) / _ema_selected(), the switch between the two weight sets
    def flush_deferred(self) -> None:
        """optimizer launches an engine holds back (UNetEngine.defer_adam); nothing to do for an engine that holds none back"""

    def enable_ema(self, momentum: float = 0.99) -> None:
        """switch the parameter averages on (or change their momentum): average = momentum * average + (1 - momentum) * var after
        every APPLIED optimizer step.  The averages start as copies of the current parameters and of their compute-dtype copy, as
        Keras >= 2.11 creates them with initial_value=var; that is [TF] behaviour and parity-unpinned (there is no TensorFlow
        here).  Optimizer launches the engine holds back are flushed first: they belong to a step made with the old setting."""
        m = float(momentum)
        if not (0.0 <= m <= 1.0):
            raise ValueError(f"ema_momentum must lie in [0, 1], got {momentum!r}")
        why = getattr(self, "_ema_forbidden", None)
        if why:
            raise ValueError(why)
        if self._ema_reading:
            raise _lib.Gct2Error("enable_ema inside ema_weights()")
        self.flush_deferred()
        if self._ema is None:
            p, shadow = self._ema_source()
            self._ema_attach(p.clone(), shadow.clone() if shadow is not None else None)
        self.use_ema, self.ema_momentum = True, m

    def disable_ema(self) -> None:
        """drop the averages (their memory goes with them)"""
        if self._ema_reading:
            raise _lib.Gct2Error("disable_ema inside ema_weights()")
        self.flush_deferred()
        self.use_ema = False
        self._ema_attach(None, None)

    def _ema_launch(self, lo: int, hi: int, momentum: float, one_minus: float, ls_ptr: Optional[int], stream: int) -> None:
        p, _ = self._ema_source()
        sh = self._ema_shadow
        call("gct2_ema_update", self._ema.data_ptr() + 4 * lo, p.data_ptr() + 4 * lo, None if sh is None else sh.data_ptr() + 2 * lo,
             self.dtype, hi - lo, momentum, one_minus, ls_ptr, stream)

    def _ema_step_update(self) -> None:
        """every optimizer launch of the step is enqueued when finish_step() runs: one launch over the arena (UNetEngine, which may
        hold some back, splits it)"""
        m, c = ema_coefficients(self.ema_momentum)
        self._ema_launch(0, self._ema.numel(), m, c, self._ls_ptr(), self._stream())

    def ema_overwrite(self) -> None:
        """Keras' finalize_variable_values: the parameters (and their compute-dtype copy) become the averages, as device copies"""
        if not self.use_ema:
            raise ValueError("ema_overwrite: the engine keeps no averages (Adam(use_ema=True) / enable_ema())")
        self.flush_deferred()
        p, shadow = self._ema_source()
        p.copy_(self._ema)
        if shadow is not None:
            shadow.copy_(self._ema_shadow)

    @contextlib.contextmanager
    def ema_weights(self):
        """inside, every forward launch (predict, the sampler) reads the averaged kernels, biases and Dense head instead of the raw
        iterate; train_step refuses.  The raw weights are back on exit, also after an exception."""
        if not self.use_ema:
            raise ValueError("ema_weights: the engine keeps no averages (Adam(use_ema=True) / enable_ema())")
        if self._ema_reading:
            raise _lib.Gct2Error("ema_weights() is already active")
        self.flush_deferred()
        self._ema_select(True)
        try:
            yield self
        finally:
            self._ema_select(False)

    def _refuse_training_on_averages(self) -> None:
        if self._ema_reading:
            raise _lib.Gct2Error("train_step inside ema_weights(): the step would differentiate the averaged weights")

    def finish_step(self) -> None:
        if self.use_ema:                   # after every Adam launch of the step, in front of the loss-scale update (found_inf gates it)
            self._ema_step_update()
        if self.ls_state is not None:      # applied_steps (= optimizer.iterations) advances on the device, only if finite
            call("gct2_loss_scale_update", self.ls_state.data_ptr(), LOSS_SCALE_GROWTH_INTERVAL, self._stream())
        else:
            self._iterations += 1
