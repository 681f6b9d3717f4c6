"""`log_sample` - the reference's sampler (train.py:323-496) with every objective switch it reads (train.py:29-32:
`predict_x`, `predict_scaled_epsilon`, `ordinary_differential_equation`; `prediction_weighting` is a training-only switch,
log_sample never reads it): one-shot denoising at `test_step` (at `steps / 2` in ODE mode, train.py:326-328), `steps` network
evaluations that invert the example image into noise, the four edits of that noise (avg-pool/upsample, roll, per-pixel
codebook), and `steps` evaluations of reverse sampling on a batch of six.

Everything stays on the device: the state (x_theta, epsilon_theta, fake) is fp32 like the reference's, the pointwise steps
are library kernels (gct2_diffusion_mix / _update / gct2_noise_edits, include/gct2.h).  The network evaluations reuse the
planned forward pass of UNetEngine at batch 1 and 6 (captured once into a HIP graph per buffer set), or - for the topology
variants of train.py:20, 26, 27 - VariantEngine.predict, layer by layer.  Returns the tensors the reference hands to tf.summary.

`generate` - what the reference does not have: n new images from noise at a batch size and step count of the caller's choice,
reproducible from a seed, with the two controls of every DDIM / DDPM sampler (eta, clipping of the x0 estimate).  Same network
evaluations; the two pointwise launches of a step are one (gct2_diffusion_step), the state is `fake` alone.  With `init=` it starts
from an image noised to an intermediate timestep (gct2_diffusion_start_image), with `mask=` it regenerates only where the mask says so
(gct2_diffusion_step_masked).  With `solver="dpm2m"` every step is the second-order multistep update instead (DPM-Solver++ 2M:
gct2_diffusion_step_multistep, one more fp32 plane that carries the previous step's estimate); `encode` takes the same switch.

With `clip_denoised="dynamic"` the fixed clip bound gives way to dynamic thresholding (Saharia et al. 2022): per image and per step a
high order statistic of |x0| (gct2_x0_quantile, a radix select) bounds the estimate, and one gct2_diffusion_step_dynamic launch takes
the place of whichever of the three steps the run would have used.

With `guide=` a second denoiser's prediction is taken at every step whose weight is not 1 and the step samples from
p_guide + w (p_main - p_guide) (two-network guidance: autoguidance, class guidance between two denoisers): ONE
gct2_diffusion_step_guided launch combines the two planes on the way in, runs whichever step the run would have used, and also writes
the next input into the guide engine's buffers; gct2_x0_quantile_guided is the select on the combined estimate.

`encode` - the inversion loop of log_sample as an API: a batch of images into latents over the same strided timesteps."""
from __future__ import annotations

import contextlib
import ctypes as C
import gc
import math
import warnings
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import model as M
from ._lib import SAMPLE_EPS, SAMPLE_ODE, SAMPLE_SCALED_EPS, SAMPLE_V, SAMPLE_X, call
from .engine import TORCH_DTYPE, UNetEngine
from .trainer_math import alpha_dash            # train.py:85-93 on python floats, as in the reference
from .trainer_math import check_noise_schedule, check_timesteps, noise_schedule_name
from .trainer_math import GENERATE_STREAM, ddim_sigma2, generate_image_stride, generate_offset, sampling_timesteps
from .trainer_math import check_mask, img2img_steps
from .trainer_math import SOLVERS, multistep_coefficient
from .trainer_math import check_predict_v
from .trainer_math import quantile_rank
from .trainer_math import guidance_launches, guidance_table


def sample_mode(predict_x: bool, predict_scaled_epsilon: bool, ordinary_differential_equation: bool, predict_v: bool = False) -> int:
    """the branch order of train.py:338-355, 382-413, 452-479: ODE first, then predict_x, then the two epsilon forms.  predict_v (the v
    objective, which the reference does not have) comes before all of them: predict_x is ignored, the other two are a ValueError."""
    if check_predict_v(predict_v, predict_scaled_epsilon, False, ordinary_differential_equation):
        return SAMPLE_V
    if ordinary_differential_equation:
        return SAMPLE_ODE
    if predict_x:
        return SAMPLE_X
    return SAMPLE_SCALED_EPS if predict_scaled_epsilon else SAMPLE_EPS


class _Sampler:
    """one network + the pointwise steps around it.  `net(B)` hands out the evaluation of a batch size: (input views for
    gct2_diffusion_mix, a function that runs the network and returns the fp32 prediction tensor)."""

    def __init__(self, eng, steps: int, mode: int, H: int, W: int, use_graph: bool = True, schedule=None, offset: float = 0.0):
        self.eng, self.steps, self.mode, self.H, self.W = eng, steps, mode, H, W
        self.schedule, self.offset = schedule, offset            # alpha_dash's live line (train.py:85-93); None / 0.0 = the reference's
        self.planned = isinstance(eng, UNetEngine)
        # a network evaluation at batch 1 / 6 is ~20 short launches, and log_sample runs 401 of them back to back: launch-bound.
        # The planned forward pass of a buffer set is captured ONCE into a HIP graph (every pointer and shape is fixed per buffer
        # set) and replayed; the pointwise steps around it carry per-step scalars and stay ordinary launches.
        self.use_graph = use_graph and self.planned
        # kept on the engine: the reference calls log_sample once per epoch, the buffer sets and arenas (hence the graphs) live on.
        # A graph bakes in the workspace pointers and the tile choices of the engine's call context at capture time: the cache is
        # keyed on the context's version (bumped by every set_workspace / set_tuning / force_direct) and holds the buffer set
        # itself, so neither a re-tuned context nor a recycled id() can replay a stale graph.  A graph also bakes in the weight
        # pointers: the key carries the weight set (raw / averaged, engine.ema_weights()), so each set replays its own capture.
        if self.planned and not hasattr(eng, "_forward_graphs"):
            eng._forward_graphs = {}
        self._inputs: Dict[int, torch.Tensor] = {}
        # per-timestep heads (train.py:199, 203, 211-214): the network reads t.  The planned engine's head takes it from the buffer
        # set's device-resident t_int, a fixed address the captured graph reads too: set_t fills it with an ordinary launch in front
        # of the evaluation, outside the graph.  Without the switch nothing is launched for t (train.py:207: "t is ignored")
        self.heads = bool(getattr(eng, "timestep_heads", False))
        self._t: Dict[int, int] = {}
        self._dynamic: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}     # per batch size: gct2_x0_quantile's (scratch, rows [B,2])

    # ---- network evaluation ---------------------------------------------------------------------------------------------
    def _graph_for(self, b):
        eng = self.eng
        cache: Dict[Tuple[int, int, bool], Tuple[object, object]] = eng._forward_graphs
        version, averaged = eng.ctx.version, bool(eng._ema_reading)
        for key in [k for k in cache if k[1] != version]:       # the context changed: every captured graph is stale
            del cache[key]
        hit = cache.get((id(b), version, averaged))
        if hit is not None and hit[1] is b:
            return hit[0]
        eng.forward(b)                          # (also the first evaluation: whatever lazy set-up there is happens here)
        # dead engines hold reference cycles (and with them step plans, events, graphs, device tensors): the cyclic collector must not
        # finalise them INSIDE the capture (torch.cuda.graph no longer collects on entry) - collect now, keep it off until the capture ends
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                eng.forward(b)
        except _lib.Gct2Error:                  # a launch was rejected: a real error, not a refused capture
            raise
        except RuntimeError as e:               # capture refused (e.g. a profiler holding the stream): plain launches from now on
            warnings.warn(f"log_sample: HIP graph capture of the forward pass was refused ({e}); using plain launches")
            self.use_graph = False
            return None
        finally:
            if gc_was_on:
                gc.enable()
        cache[(id(b), version, averaged)] = (g, b)
        return None                             # this evaluation has already run (the warm-up call above)

    def set_t(self, B: int, t: int) -> None:
        """the timestep of the next evaluation at batch B (tf.constant([t]), broadcast over the batch): checked on the host against
        1..steps of the engine (ValueError), then written where the head kernels read it"""
        if not self.heads:
            return
        (t,) = check_timesteps(t, 1, self.eng.steps)
        self._t[B] = t
        if self.planned:
            self.eng.buffers(B, self.H, self.W).t_int.fill_(t)

    def set_t_rows(self, B: int, t: torch.Tensor) -> None:
        """set_t's per-image form: t int32 [B] on the device, one timestep per image (a distillation batch), copied where the head
        kernels read it - no host round trip, so nothing is checked here: the caller's values come from a table of valid timesteps"""
        if not self.heads:
            return
        if self.planned:
            self.eng.buffers(B, self.H, self.W).t_int.copy_(t)
        else:
            self._t[B] = t

    def evaluate(self, B: int) -> torch.Tensor:
        """denoiser((fake, t)) on the image gct2_diffusion_mix has just stored: t is ignored (train.py:208-210) unless the engine
        carries the per-timestep heads (set_t).  Returns the fp32 prediction [B,H,W,3] (valid until the next evaluation)."""
        eng = self.eng
        if not self.planned:
            if self.heads and torch.is_tensor(self._t[B]):       # set_t_rows: predict's body with the device-resident timesteps
                eng.flush_deferred()
                eng.net.t_int = self._t[B]
                return eng.top.fwd(self._inputs[B])
            return eng.predict(self._inputs[B], self._t[B]) if self.heads else eng.predict(self._inputs[B])
        b = eng.buffers(B, self.H, self.W)
        eng.flush_deferred()                     # optimizer launches the last train step held back: never inside a captured graph
        if not self.use_graph:
            eng.forward(b)
            return b.pred
        cache = eng._forward_graphs
        hit = cache.get((id(b), eng.ctx.version, bool(eng._ema_reading)))
        if hit is not None and hit[1] is b:
            hit[0].replay()
        else:
            self._graph_for(b)
        return b.pred

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.eng.device).cuda_stream

    def input_views(self, B: int) -> Tuple[int, int, Optional[int], int]:
        """(out, ldout, out2, ldout2) of the pointwise kernels: where the network of batch B reads its input in the compute dtype - the
        planned engine's packed image and the image slice of R_0, or the one tensor VariantEngine.predict is handed"""
        eng = self.eng
        if self.planned:
            b = eng.buffers(B, self.H, self.W)
            return b.img.data_ptr(), 4, eng._slice_ptr(b.R[0], eng.topo.fu(0)), b.ld[0]
        inp = self._inputs.get(B)
        if inp is None:
            inp = self._inputs[B] = torch.empty(B, self.H, self.W, 3, dtype=TORCH_DTYPE[eng.dtype], device=eng.device)
        return inp.data_ptr(), 3, None, 0

    def mix(self, B: int, x: torch.Tensor, e: torch.Tensor, alpha: float, fake: torch.Tensor) -> None:
        """fake = sqrt(alpha) x + sqrt(1 - alpha) e, also written where the network reads its input."""
        call("gct2_diffusion_mix", self.eng.dtype, x.data_ptr(), e.data_ptr(), alpha, fake.data_ptr(), *self.input_views(B),
             B * self.H * self.W, 3, self._stream())

    def start(self, B: int, seed: int, offset: int, image_stride: int, fake: torch.Tensor) -> None:
        """fake = the normals of generation's stream from `offset` on, images image_stride apart (gct2_diffusion_start)."""
        call("gct2_diffusion_start", self.eng.dtype, seed, GENERATE_STREAM, offset, image_stride, fake.data_ptr(), *self.input_views(B),
             B, self.H * self.W * 3, 3, self._stream())

    def fused_step(self, B: int, pred: torch.Tensor, fake: torch.Tensor, a_t: float, a_prev: float, sigma2: float, clip: float, seed: int,
                   offset: int, image_stride: int, x0: Optional[torch.Tensor]) -> None:
        """update + clip + re-noising to a_prev in one launch, in place on fake (gct2_diffusion_step); x0: where the x0 estimate goes"""
        call("gct2_diffusion_step", self.mode, self.eng.dtype, pred.data_ptr(), fake.data_ptr(), a_t, a_prev, sigma2, clip, seed,
             GENERATE_STREAM, offset, image_stride, fake.data_ptr(), x0.data_ptr() if x0 is not None else None, *self.input_views(B),
             B, self.H * self.W * 3, 3, self._stream())

    def start_image(self, B: int, known: torch.Tensor, alpha: float, seed: int, offset: int, image_stride: int, fake: torch.Tensor) -> None:
        """fake = sqrt(alpha) known + sqrt(1 - alpha) (the normals `start` would write): gct2_diffusion_start_image"""
        call("gct2_diffusion_start_image", self.eng.dtype, known.data_ptr(), alpha, seed, GENERATE_STREAM, offset, image_stride,
             fake.data_ptr(), *self.input_views(B), B, self.H * self.W * 3, 3, self._stream())

    def masked_step(self, B: int, pred: torch.Tensor, fake: torch.Tensor, known: torch.Tensor, mask: torch.Tensor, a_t: float, a_prev: float,
                    sigma2: float, clip: float, seed: int, offset: int, offset0: int, image_stride: int, x0: Optional[torch.Tensor]) -> None:
        """fused_step where mask >= 1, the known image re-noised to a_prev with its own starting noise (offset0) where mask <= 0, the
        blend between: gct2_diffusion_step_masked, in place on fake; x0: the estimate composited with the known image the same way"""
        call("gct2_diffusion_step_masked", self.mode, self.eng.dtype, pred.data_ptr(), fake.data_ptr(), known.data_ptr(), mask.data_ptr(),
             a_t, a_prev, sigma2, clip, seed, GENERATE_STREAM, offset, offset0, image_stride, fake.data_ptr(),
             x0.data_ptr() if x0 is not None else None, *self.input_views(B), B, self.H * self.W * 3, 3, self._stream())

    def multistep_step(self, B: int, pred: torch.Tensor, fake: torch.Tensor, hist: torch.Tensor, known: Optional[torch.Tensor],
                       mask: Optional[torch.Tensor], a_t: float, a_prev: float, c1: float, clip: float, seed: int, offset0: int,
                       image_stride: int, x0: Optional[torch.Tensor]) -> None:
        """fused_step at sigma2 = 0 (masked_step with known and mask) re-noising the estimate extrapolated by c1 from the one in hist, which
        then takes this step's: gct2_diffusion_step_multistep, in place on fake and hist"""
        call("gct2_diffusion_step_multistep", self.mode, self.eng.dtype, pred.data_ptr(), fake.data_ptr(), hist.data_ptr(),
             known.data_ptr() if known is not None else None, mask.data_ptr() if mask is not None else None, a_t, a_prev, c1, clip, seed,
             GENERATE_STREAM, offset0, image_stride, fake.data_ptr(), hist.data_ptr(), x0.data_ptr() if x0 is not None else None,
             *self.input_views(B), B, self.H * self.W * 3, 3, self._stream())

    def dynamic_rows(self, B: int, pred: torch.Tensor, fake: torch.Tensor, a_t: float, rank: int, floor: float) -> torch.Tensor:
        """per image, the rank-th smallest |x0| of the step's own estimate against the floor: gct2_x0_quantile into this batch size's
        fp32 [B,2] = {s_b, r_b} (valid until the next call at B); the scratch lives beside it"""
        scratch, rows = self._rows(B)
        call("gct2_x0_quantile", self.mode, pred.data_ptr(), fake.data_ptr(), a_t, rank, floor, rows.data_ptr(), None, scratch.data_ptr(),
             scratch.numel(), B, self.H * self.W * 3, self._stream())
        return rows

    def dynamic_step(self, B: int, pred: torch.Tensor, fake: torch.Tensor, hist: Optional[torch.Tensor], known: Optional[torch.Tensor],
                     mask: Optional[torch.Tensor], rows: torch.Tensor, a_t: float, a_prev: float, sigma2: float, c1: float, seed: int,
                     offset: int, offset0: int, image_stride: int, x0: Optional[torch.Tensor]) -> None:
        """fused_step / masked_step (known and mask) / multistep_step (hist) with rows [B,2] = {s_b, r_b} in the place of the scalar
        clip: gct2_diffusion_step_dynamic, in place on fake (and hist)"""
        ptr = lambda t: t.data_ptr() if t is not None else None
        call("gct2_diffusion_step_dynamic", self.mode, self.eng.dtype, pred.data_ptr(), fake.data_ptr(), ptr(hist), ptr(known), ptr(mask),
             rows.data_ptr(), a_t, a_prev, sigma2, c1, seed, GENERATE_STREAM, offset, offset0, image_stride, fake.data_ptr(), ptr(hist),
             ptr(x0), *self.input_views(B), B, self.H * self.W * 3, 3, self._stream())

    def _rows(self, B: int) -> Tuple[torch.Tensor, torch.Tensor]:
        held = self._dynamic.get(B)
        if held is None:
            need = C.c_size_t(0)
            call("gct2_x0_quantile_scratch", B, self.H * self.W * 3, C.byref(need))
            held = self._dynamic[B] = (torch.empty(need.value, dtype=torch.uint8, device=self.eng.device),
                                       torch.empty(B, 2, dtype=torch.float32, device=self.eng.device))
        return held

    def guided_rows(self, B: int, pred: torch.Tensor, pred_guide: torch.Tensor, w: float, fake: torch.Tensor, a_t: float, rank: int,
                    floor: float) -> torch.Tensor:
        """dynamic_rows on the combined prediction p = pred_guide + w (pred - pred_guide), formed pass by pass and never stored:
        gct2_x0_quantile_guided, into the same [B,2] and scratch"""
        scratch, rows = self._rows(B)
        call("gct2_x0_quantile_guided", self.mode, pred.data_ptr(), pred_guide.data_ptr(), w, fake.data_ptr(), a_t, rank, floor,
             rows.data_ptr(), None, scratch.data_ptr(), scratch.numel(), B, self.H * self.W * 3, self._stream())
        return rows

    def guided_step(self, B: int, pred: torch.Tensor, pred_guide: Optional[torch.Tensor], w: float, fake: torch.Tensor,
                    hist: Optional[torch.Tensor], known: Optional[torch.Tensor], mask: Optional[torch.Tensor], rows: Optional[torch.Tensor],
                    a_t: float, a_prev: float, sigma2: float, c1: float, clip: float, seed: int, offset: int, offset0: int, image_stride: int,
                    x0: Optional[torch.Tensor], guide_views=(None, 0, None, 0)) -> None:
        """whichever of fused_step / masked_step / multistep_step / dynamic_step the arguments select, on pred_guide + w (pred - pred_guide)
        (pred_guide None: on pred), the result also stored to guide_views - the guide engine's input_views: gct2_diffusion_step_guided, in
        place on fake (and hist)"""
        ptr = lambda t: t.data_ptr() if t is not None else None
        call("gct2_diffusion_step_guided", self.mode, self.eng.dtype, pred.data_ptr(), ptr(pred_guide), w, fake.data_ptr(), ptr(hist),
             ptr(known), ptr(mask), ptr(rows), a_t, a_prev, sigma2, c1, clip, seed, GENERATE_STREAM, offset, offset0, image_stride,
             fake.data_ptr(), ptr(hist), ptr(x0), *self.input_views(B), *guide_views, B, self.H * self.W * 3, 3, self._stream())

    def update(self, pred: torch.Tensor, fake: torch.Tensor, alpha: float, alpha_prev: float, x: torch.Tensor, e: Optional[torch.Tensor]) -> None:
        """train.py:382-413 / 452-479 by mode (gct2_diffusion_update)."""
        call("gct2_diffusion_update", self.mode, pred.data_ptr(), fake.data_ptr(), alpha, alpha_prev, x.data_ptr(),
             e.data_ptr() if e is not None else None, pred.numel(), self._stream())

    def step(self, B: int, x, e, fake, t: int) -> None:
        a = alpha_dash(t, self.steps, self.schedule, self.offset)
        self.mix(B, x, e, a, fake)
        self.set_t(B, t)
        pred = self.evaluate(B)
        # ODE mode leaves epsilon_theta alone (train.py:382-392: only x_theta is assigned; `fake = ...` there is dead, the next
        # iteration recomputes it)
        self.update(pred, fake, a, alpha_dash(t - 1, self.steps, self.schedule, self.offset), x, None if self.mode == SAMPLE_ODE else e)


def _resolve_switches(eng, predict_x, predict_scaled_epsilon, ordinary_differential_equation, predict_v=None) -> int:
    """the sampler's objective switches: explicit arguments, else the module-level globals (train.py reads its globals when
    log_sample runs).  A network trained for another objective would sample garbage without any error: refuse a mismatch
    with the engine's own switches."""
    want = dict(predict_x=M.predict_x if predict_x is None else predict_x,
                predict_scaled_epsilon=M.predict_scaled_epsilon if predict_scaled_epsilon is None else predict_scaled_epsilon,
                ordinary_differential_equation=(M.ordinary_differential_equation if ordinary_differential_equation is None
                                                else ordinary_differential_equation))
    if bool(M.predict_v if predict_v is None else predict_v):          # (named only when on: the messages of the reference's switches stay)
        want["predict_v"] = True
    mode = sample_mode(**want)
    if all(hasattr(eng, k) for k in want):
        have = sample_mode(eng.predict_x, eng.predict_scaled_epsilon, eng.ordinary_differential_equation,
                           predict_v=getattr(eng, "predict_v", False))
        if have != mode:
            raise ValueError(f"log_sample: objective switches {want} select sampler mode {mode}, but the engine was set up for "
                             f"mode {have} (predict_x={eng.predict_x}, predict_scaled_epsilon={eng.predict_scaled_epsilon}, "
                             f"ordinary_differential_equation={eng.ordinary_differential_equation}"
                             f"{', predict_v=True' if getattr(eng, 'predict_v', False) else ''}); train.py:29-32 are read by "
                             "Trainer.call and log_sample alike")
    return mode


def _resolve_schedule(eng, noise_schedule, alpha_dash_offset):
    """the sampler's noise schedule: an explicit noise_schedule= / alpha_dash_offset= pair, else the engine's own.  Like
    _resolve_switches: a network trained under another schedule samples garbage without any error, so an explicit pair that
    disagrees with the engine's is refused (callables compare by identity)."""
    have = (getattr(eng, "noise_schedule", "quadratic"), float(getattr(eng, "alpha_dash_offset", 0.0)))
    if noise_schedule is None and alpha_dash_offset is None:
        return have
    want = check_noise_schedule(have[0] if noise_schedule is None else noise_schedule, have[1] if alpha_dash_offset is None else alpha_dash_offset)
    if want != have:
        raise ValueError(f"log_sample: noise schedule {noise_schedule_name(want[0])!r} with offset {want[1]!r} was asked for, but the engine "
                         f"was set up for {noise_schedule_name(have[0])!r} with offset {have[1]!r} (set_noise_schedule / the module globals "
                         "noise_schedule and alpha_dash_offset; train.py:85-93 is read by Trainer.call and log_sample alike)")
    return want


def log_sample(denoiser: "M.Denoiser", example_image: torch.Tensor, example: torch.Tensor, dictionary: torch.Tensor,
               steps: Optional[int] = None, test_step: Optional[int] = None, predict_x: Optional[bool] = None,
               predict_scaled_epsilon: Optional[bool] = None, ordinary_differential_equation: Optional[bool] = None,
               use_graph: bool = True, use_ema: bool = False, noise_schedule=None, alpha_dash_offset: Optional[float] = None,
               predict_v: Optional[bool] = None) -> Dict[str, torch.Tensor]:
    """example_image [1,H,W,3] fp32 in [-1,1) (train.py:305); example [1,2,H,W,3] ~ N(0,1) (train.py:306);
    dictionary [H,W,2**bits_per_pixel,3] ~ N(0,1) (train.py:308-311); all on the HIP device.
    use_ema: every network evaluation reads the engine's parameter averages (Adam(use_ema=True)) instead of the raw iterate.
    noise_schedule / alpha_dash_offset: alpha_dash's live line (train.py:85-93); by default the engine's (set_noise_schedule), an
    explicit pair must agree with it (ValueError)."""
    eng = denoiser.ensure_engine()
    with (eng.ema_weights() if use_ema else contextlib.nullcontext()):
        return _log_sample(eng, example_image, example, dictionary, steps, test_step, predict_x, predict_scaled_epsilon,
                           ordinary_differential_equation, use_graph, noise_schedule, alpha_dash_offset, predict_v)


def _log_sample(eng, example_image, example, dictionary, steps, test_step, predict_x, predict_scaled_epsilon,
                ordinary_differential_equation, use_graph, noise_schedule=None, alpha_dash_offset=None,
                predict_v=None) -> Dict[str, torch.Tensor]:
    steps = M.steps if steps is None else steps
    test_step = M.test_step if test_step is None else test_step
    mode = _resolve_switches(eng, predict_x, predict_scaled_epsilon, ordinary_differential_equation, predict_v)
    schedule, offset = _resolve_schedule(eng, noise_schedule, alpha_dash_offset)
    alpha = lambda t: alpha_dash(t, steps, schedule, offset)
    dev = eng.device
    f32 = lambda t: t.to(dev, torch.float32).contiguous()
    example_image, example, dictionary = f32(example_image), f32(example), f32(dictionary)
    _, H, W, _ = example_image.shape
    if example.shape != (1, 2, H, W, 3) or dictionary.shape[:2] != (H, W) or dictionary.shape[3] != 3:
        raise ValueError("log_sample: example must be [1,2,H,W,3] and dictionary [H,W,K,3] for an example image [1,H,W,3]")
    S = _Sampler(eng, steps, mode, H, W, use_graph, schedule, offset)
    out: Dict[str, torch.Tensor] = {}
    image = example_image[0][None].contiguous()

    # ---- single-shot denoising (train.py:325-361): at test_step; ODE mode mixes with alpha_dash(steps / 2) ** 0.5
    if mode == SAMPLE_ODE:
        factor = alpha(steps / 2) ** 0.5                              # train.py:326-328
        a_t, a_prev = alpha(steps / 2), alpha(steps / 2 - 1)
    else:
        factor = alpha(test_step)
        a_t, a_prev = factor, 0.0
    fake = torch.empty_like(image)
    S.mix(1, image, example[0, :1].contiguous(), factor, fake)
    S.set_t(1, test_step)                       # tf.constant([test_step]) also in ODE mode, which mixes at steps / 2 (train.py:335)
    # (never through the graph: the first evaluation of a buffer set is the capture's warm-up anyway)
    pred = eng.forward(eng.buffers(1, H, W)) if S.planned else S.evaluate(1)
    denoised, scratch = torch.empty_like(image), torch.empty_like(image)
    # denoised of train.py:338-355 is x_theta of the same update the loops use, at alpha = image_factor
    S.update(pred, fake, a_t, a_prev, denoised, scratch)
    out["denoised"] = denoised
    loss, dpred, partials = torch.zeros(1, device=dev), torch.empty_like(denoised), torch.zeros(1024, device=dev)
    call("gct2_mse_fwd_bwd", denoised.data_ptr(), image.data_ptr(), dpred.data_ptr(), loss.data_ptr(), partials.data_ptr(),
         denoised.numel(), None, S._stream())
    out["example_loss"] = loss.sqrt()           # reduce_mean((image - denoised)**2)**0.5   (train.py:357-361)

    # ---- forward diffusion: invert the example image (train.py:364-413)
    x_theta, eps_theta = image.clone(), image.clone()
    for t in range(1, steps + 1):
        S.step(1, x_theta, eps_theta, fake, t)
    out["epsilon_theta"] = eps_theta.clone()

    # ---- the four edits + the two random noises -> batch of six (train.py:415-437)
    edits = torch.empty(4, H, W, 3, device=dev)
    call("gct2_noise_edits", eps_theta.data_ptr(), dictionary.data_ptr(), dictionary.shape[2], edits.data_ptr(), H, W, 3, S._stream())
    start = torch.cat([example[0], edits], 0).contiguous()
    x_theta, eps_theta, fake = start.clone(), start.clone(), torch.empty_like(start)

    # ---- backward diffusion (train.py:439-496)
    marks = ((steps, "step_1"), (steps // 4, "step_0.25"), (2 * steps // 4, "step_0.5"), (3 * steps // 4, "step_0.75"))
    for t in range(steps, 0, -1):
        S.step(6, x_theta, eps_theta, fake, t)
        for tm, name in marks:                  # the reference's four `if`s (train.py:488-495): distinct tags, may share a t
            if t == tm:
                out[name] = x_theta.clone()
    out["fake"] = x_theta.clone()
    return out


def generate(denoiser: "M.Denoiser", n: int, num_steps: Optional[int] = None, eta: float = 0.0, clip_denoised=None, seed: int = 0,
             first_index: int = 0, batch_size: Optional[int] = None, timesteps=None, noise: Optional[torch.Tensor] = None,
             use_ema: bool = False, use_graph: bool = True, return_steps=(), size=None, predict_x: Optional[bool] = None,
             predict_scaled_epsilon: Optional[bool] = None, ordinary_differential_equation: Optional[bool] = None, noise_schedule=None,
             alpha_dash_offset: Optional[float] = None, init: Optional[torch.Tensor] = None, strength: float = 1.0, mask=None,
             solver: str = "ddim", predict_v: Optional[bool] = None, dynamic_percentile: Optional[float] = None,
             dynamic_floor: Optional[float] = None, return_thresholds: bool = False, guide: Optional["M.Denoiser"] = None,
             guidance_scale=None, guidance_interval=None, guide_use_ema: bool = False):
    """n new images from noise: strided DDIM sampling (Song et al. 2021) over K = num_steps of the engine's `steps` timesteps
    (trainer_math.sampling_timesteps; None: all of them; or an explicit strictly increasing `timesteps` list within 1..steps), one
    network evaluation and ONE pointwise launch (gct2_diffusion_step) per step.  Returns fp32 [n,H,W,3] on the device: the x0 estimate
    of the last step, which the reference logs as `fake` (its schedule never reaches alpha = 1, so the estimate is the sample).
    eta: 0 the deterministic DDIM step, 1 the DDPM posterior variance (trainer_math.ddim_sigma2).  clip_denoised: True clips every x0
    estimate to [-1, 1], a float to that bound (eps is re-derived from the clipped estimate); None / False: no clipping.
    seed, first_index: image g = first_index + position draws its starting noise and the noise of every step from Philox stream
    GENERATE_STREAM by g alone (trainer_math.generate_offset): the result does not depend on batch_size (default min(n, 64)), and
    generate(4) is generate(2) followed by generate(2, first_index=2).  noise [n,H,W,3]: the starting noise instead of the drawn one.
    size: H = W (or (H, W)) when no noise is given; None is the module's `size`.  return_steps: timesteps whose x0 estimate is
    returned too - then the result is (images, {t: fp32 [n,H,W,3]}).  use_ema: every evaluation reads the parameter averages.
    The objective switches (predict_v, the v objective, among them: gct2_diffusion_step's mode V, whose estimates divide by nothing) and
    the noise schedule resolve like log_sample's; the ODE objective is refused (its network predicts one
    step back only: striding and eta mean nothing there).  No training state moves: the RNG positions of training and evaluation,
    optimizer slots, averages, loss scale and recorded plans stay as they are.
    init [n,H,W,3] fp32: image-to-image.  The K' = trainer_math.img2img_steps(K, strength) last steps of the schedule run, from the image
    noised to the K'-th timestep with its own starting noise (gct2_diffusion_start_image); the step at a timestep reads the Philox slot the
    full run reads there, so strength only cuts the front of the schedule (strength = 1: all K steps, from the image noised to the
    last timestep).  return_steps must then lie among the K' timesteps visited.
    mask with init ([H,W], [n,H,W] or [n,H,W,1]; trainer_math.check_mask): inpainting.  1 regenerates a pixel, 0 keeps it: every step is
    gct2_diffusion_step_masked, which pins the kept region to init re-noised with the image's starting noise; the result is the last
    estimate composited with init (kept pixels are init's bits).  ValueError: mask or strength != 1 without init, init with noise, an
    init of another shape than [n,H,W,3], strength outside (0, 1].
    solver: "ddim" (the default: the calls and the bits described above) or "dpm2m", the second-order multistep solver of the
    probability-flow ODE (DPM-Solver++ 2M, Lu et al. 2022): every step is ONE gct2_diffusion_step_multistep launch, which re-noises the
    estimate extrapolated from the previous step's, D = x0 + c1 (x0 - x0_prev) with c1 = trainer_math.multistep_coefficient(alpha of the
    timestep evaluated before, a_t, a_prev); the previous estimate lives in one more fp32 plane per batch.  No extra network evaluation.
    c1 = 0 (the DDIM step's bits) at the first step run - of every batch, also after a strength cut - and at the last, whose result is
    its own x0 estimate; so num_steps <= 2 is solver="ddim" bit for bit.  Deterministic: eta != 0 is a ValueError.  return_steps holds
    the network's (clipped, with mask composited) estimates, not the extrapolated ones.  An unknown name is a ValueError.  What the
    solver does to sample quality on a trained network is not measured in this project; its order of accuracy as an integrator is
    (tests/test_multistep_kernels_gpu.py).
    clip_denoised="dynamic": dynamic thresholding (Saharia et al. 2022, "Imagen", section 2.3) in the fixed clip's place.  At every step
    and for every image, s = the trainer_math.quantile_rank(dynamic_percentile, H W 3)-th smallest |x0| of the network's estimate (the
    exact order statistic, one gct2_x0_quantile call); where s > dynamic_floor the estimate is clipped to [-s, s] and multiplied by
    dynamic_floor / s, elsewhere it is clipped to dynamic_floor like clip_denoised=dynamic_floor (a NaN or infinite s too); eps is
    re-derived either way, in ONE gct2_diffusion_step_dynamic launch that stands for the plain, the masked and the multistep step.  It
    composes with every other argument (with mask= the statistic runs over the whole estimate, kept pixels included); a huge floor is
    clip_denoised=floor bit for bit.  return_thresholds=True appends {t: fp32 [n]} to the result: s of every image at every timestep
    run, which shows whether the percentile ever engages.  ValueError: dynamic_percentile outside (0, 1], a dynamic_floor that is not
    finite and > 0, either of them (anything but None, the defaults 0.995 and 1.0 included) or return_thresholds without
    clip_denoised="dynamic", any other string.  dynamic_percentile=None is 0.995, dynamic_floor=None is 1.0.  Not covered: interpolated percentiles, per-channel or mask-aware statistics, encode, log_sample, the data-parallel
    wrappers.  What it does to the sample quality of a trained network is not measured in this project.
    guide: a second Denoiser - two-network guidance.  At every step the prediction the step uses is p = p_guide + w (p_main - p_guide), both
    networks evaluated at the same fake and timestep under the same objective (where x0 is affine in the prediction, so this is the same
    combination of the two x0 estimates): w = 1 the main network alone, w = 0 the guide alone, w > 1 extrapolates away from the guide.  With
    a less-trained or smaller checkpoint of the same model as the guide (clone_denoiser, a checkpoint, the raw weights against the
    averages) this is autoguidance (Karras et al. 2024); with a guide trained on everything and a main model trained on one class it is
    class guidance between two denoisers (Liu et al. 2022).  guidance_scale: a float, a callable f(t) -> float or a sequence of `steps`
    floats indexed by t - 1; guidance_interval=(t_lo, t_hi) keeps the weight for t_lo <= t <= t_hi and sets it to 1 elsewhere
    (Kynkaanniemi et al. 2024); both resolve on the host (trainer_math.guidance_table).  A step whose weight is exactly 1.0 does not
    evaluate the guide, and a run whose weights are all 1 is guide=None launch for launch (trainer_math.guidance_launches).  The combine
    is fp32, d = p_main - p_guide, t = (float)w d, p = p_guide + t, each rounded once, inside ONE gct2_diffusion_step_guided launch per
    step that is otherwise the step the run would have used and also stores the next input into the guide engine's buffers; under
    clip_denoised="dynamic" the select is gct2_x0_quantile_guided on the same p - guidance above 1 is what pushes x0 outside [-1, 1]
    and gives dynamic thresholding its purpose.  guide_use_ema: the guide reads its averages, independently of use_ema.  It composes
    with every other argument; each network replays its own captured forward graph; no training state of either denoiser moves.
    ValueError before any launch: guidance_scale or guidance_interval without guide, guide without guidance_scale, a guide that is the
    main denoiser's own engine (use clone_denoiser), a guide with other steps, noise schedule, offset, objective, compute dtype or
    device, a weight that is not finite, an interval outside 1..steps or with t_lo > t_hi.  What guidance does to the sample quality
    of a trained network is not measured in this project (no data, no Inception network).  Not covered: encode, log_sample, Distiller,
    the data-parallel wrappers."""
    eng = denoiser.ensure_engine()
    steps = int(eng.steps)
    if solver not in SOLVERS:
        raise ValueError(f"generate: solver must be one of {SOLVERS!r}, got {solver!r}")
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"generate: n must be a positive int, got {n!r}")
    mode = _resolve_switches(eng, predict_x, predict_scaled_epsilon, ordinary_differential_equation, predict_v)
    if mode == SAMPLE_ODE:
        raise ValueError("generate: the ordinary_differential_equation objective predicts the image one step back only; strided sampling "
                         "and eta have no meaning there (log_sample runs its sampler)")
    schedule, offset = _resolve_schedule(eng, noise_schedule, alpha_dash_offset)
    geng, weights = None, None
    if guide is None:
        if guidance_scale is not None or guidance_interval is not None or guide_use_ema:
            raise ValueError("generate: guidance_scale, guidance_interval and guide_use_ema belong to guide=, which is None")
    else:
        if guidance_scale is None:
            raise ValueError("generate: guide= needs guidance_scale (1.0 is the main network alone)")
        geng = guide.ensure_engine()
        if geng is eng:
            raise ValueError("generate: the guide is the main denoiser's own engine; guide with a copy (clone_denoiser) or another checkpoint")
        if int(geng.steps) != steps or _resolve_schedule(geng, None, None) != (schedule, offset):
            raise ValueError(f"generate: the guide (steps {geng.steps}, schedule {_resolve_schedule(geng, None, None)!r}) and the main denoiser "
                             f"(steps {steps}, schedule {(schedule, offset)!r}) must share steps, noise schedule and offset")
        try:
            gmode = _resolve_switches(geng, predict_x, predict_scaled_epsilon, ordinary_differential_equation, predict_v)
        except ValueError as e:
            raise ValueError(f"generate: the guide predicts under another objective than the main denoiser ({e})") from None
        if gmode != mode:
            raise ValueError(f"generate: the guide's sampler mode {gmode} differs from the main denoiser's {mode}")
        try:
            weights = guidance_table(guidance_scale, steps, guidance_interval)
        except ValueError as e:
            raise ValueError(f"generate: {e}") from None
        if geng.dtype != eng.dtype or geng.device != eng.device:
            raise ValueError(f"generate: the guide computes in dtype {geng.dtype} on {geng.device}, the main denoiser in {eng.dtype} on "
                             f"{eng.device}: the fused step writes one value into both networks' inputs")
    if not float(eta) >= 0.0:
        raise ValueError(f"generate: eta must be >= 0, got {eta!r}")
    multistep = solver == "dpm2m"
    if multistep and float(eta) != 0.0:
        raise ValueError(f"generate: solver 'dpm2m' is deterministic (it integrates the probability-flow ODE): eta must be 0, got {eta!r}")
    taus = _taus("generate", steps, num_steps, timesteps)
    K = len(taus)
    dynamic = isinstance(clip_denoised, str) and clip_denoised == "dynamic"
    if dynamic:
        clip = 0.0
        try:
            percentile = 0.995 if dynamic_percentile is None else float(dynamic_percentile)
            floor = 1.0 if dynamic_floor is None else float(dynamic_floor)
        except (TypeError, ValueError):
            raise ValueError(f"generate: dynamic_percentile and dynamic_floor must be numbers, got {dynamic_percentile!r}, "
                             f"{dynamic_floor!r}") from None
        if isinstance(dynamic_percentile, bool) or not 0.0 < percentile <= 1.0:
            raise ValueError(f"generate: dynamic_percentile must lie in (0, 1], got {dynamic_percentile!r}")
        with np.errstate(over="ignore"):
            floor32 = float(np.float32(floor))          # the kernel's F
        if isinstance(dynamic_floor, bool) or not (floor > 0.0 and math.isfinite(floor) and math.isfinite(floor32) and floor32 > 0.0):
            raise ValueError(f"generate: dynamic_floor must be a finite bound > 0 (also in fp32), got {dynamic_floor!r}")
    else:
        if dynamic_percentile is not None or dynamic_floor is not None or return_thresholds:
            raise ValueError('generate: dynamic_percentile, dynamic_floor and return_thresholds belong to clip_denoised="dynamic", got '
                             f"clip_denoised={clip_denoised!r}")
        if clip_denoised is None or clip_denoised is False:
            clip = 0.0
        elif clip_denoised is True:
            clip = 1.0
        else:
            try:
                if isinstance(clip_denoised, str):
                    raise ValueError
                clip = float(clip_denoised)
            except (TypeError, ValueError):
                clip = float("nan")
            if not (clip > 0.0 and clip < float("inf")):
                raise ValueError('generate: clip_denoised must be True, False, None, "dynamic" or a finite bound > 0, got '
                                 f"{clip_denoised!r}")
    if init is None and (mask is not None or strength != 1.0):
        raise ValueError("generate: mask and strength condition the run on an image: they need init")
    if init is not None and noise is not None:
        raise ValueError("generate: init starts from an image noised with the drawn noise; noise cannot be given too")
    try:
        K_run = img2img_steps(K, strength)
    except (TypeError, ValueError):
        raise ValueError(f"generate: strength must lie in (0, 1], got {strength!r}") from None
    if init is not None:
        if not isinstance(init, torch.Tensor) or init.dim() != 4 or init.shape[0] != n or init.shape[3] != 3 or \
                (size is not None and tuple(init.shape[1:3]) != _hw(size)):
            raise ValueError(f"generate: init must be [n,H,W,3] = [{n},H,W,3], got {tuple(getattr(init, 'shape', ()))}")
        H, W = int(init.shape[1]), int(init.shape[2])
        if mask is not None:
            try:
                mask = check_mask(mask, n, H, W)
            except ValueError as e:
                raise ValueError(f"generate: {e}") from None
    elif noise is not None:
        if noise.dim() != 4 or noise.shape[0] != n or noise.shape[3] != 3 or (size is not None and tuple(noise.shape[1:3]) != _hw(size)):
            raise ValueError(f"generate: noise must be [n,H,W,3] = [{n},H,W,3], got {tuple(noise.shape)}")
        H, W = int(noise.shape[1]), int(noise.shape[2])
    else:
        H, W = _hw(M.size if size is None else size)
    marks = tuple(return_steps)
    if any(t not in taus[:K_run] for t in marks):
        raise ValueError(f"generate: return_steps {list(marks)!r} must be among the timesteps sampled, {taus[:K_run]!r}")
    bs = min(n, 64) if batch_size is None else batch_size
    if isinstance(bs, bool) or not isinstance(bs, int) or bs < 1:
        raise ValueError(f"generate: batch_size must be a positive int, got {batch_size!r}")
    per_image = H * W * 3
    rank = quantile_rank(percentile, per_image) if dynamic else 0
    seed, first_index = int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_index)
    if first_index < 0 or generate_offset(first_index + n, 0, K, per_image) >= 1 << 64:
        raise ValueError(f"generate: first_index = {first_index!r} leaves the 64-bit stream")
    stride = generate_image_stride(K, per_image)
    alpha = lambda t: float(alpha_dash(t, steps, schedule, offset))
    plan = []                                   # per step in sampling order: (t, a_t, a_prev, sigma2)
    for k in range(K):
        tau = taus[K - 1 - k]
        a_t, a_prev = alpha(tau), alpha(taus[K - 2 - k] if k < K - 1 else 0)
        s2 = ddim_sigma2(a_t, a_prev, eta)
        # the kernel forms sqrt((1 - a_prev) - sigma2) in fp32: a sigma2 clamped at 1 - a_prev in double must not pass it there
        lim = float(np.float32(1.0) - np.float32(a_prev))
        plan.append((tau, a_t, a_prev, lim if float(np.float32(s2)) > lim else s2))
    # solver="dpm2m": c1 per step.  0 at the first step run (no history yet) and at the last (its re-noised state is never read, the
    # result is that step's own estimate); between them the estimate of the step before extrapolates
    c1s = [0.0 if k <= K - K_run or k == K - 1 else multistep_coefficient(plan[k - 1][1], plan[k][1], plan[k][2]) for k in range(K)]

    # guidance: what every step run launches (the same for every batch), from the weights of the timesteps in sampling order
    start_copy, launches = guidance_launches([weights[plan[k][0] - 1] for k in range(K - K_run, K)]) if geng is not None else (False, None)

    dev = eng.device
    with contextlib.ExitStack() as weights_read:
        if use_ema:
            weights_read.enter_context(eng.ema_weights())
        if geng is not None and guide_use_ema:
            weights_read.enter_context(geng.ema_weights())
        eng.flush_deferred()
        S = _Sampler(eng, steps, mode, H, W, use_graph, schedule, offset)
        SG = None
        if geng is not None:
            geng.flush_deferred()
            SG = _Sampler(geng, steps, mode, H, W, use_graph, schedule, offset)
        out = torch.empty(n, H, W, 3, dtype=torch.float32, device=dev)
        kept = {t: torch.empty_like(out) for t in marks}
        bounds = {tau: torch.empty(n, dtype=torch.float32, device=dev) for tau in taus[:K_run]} if dynamic and return_thresholds else None
        fake = gstart = None
        for g0 in range(0, n, bs):
            B = min(bs, n - g0)
            if fake is None or fake.shape[0] != B:
                fake = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
                hist = torch.empty_like(fake) if multistep else None       # the estimate of the step before (first read at c1 != 0)
            off0 = generate_offset(first_index + g0, 0, K, per_image)
            known = keep = None
            if init is not None:                # the image noised to the first timestep visited, with the noise `start` would write
                known = init[g0:g0 + B].to(dev, torch.float32).contiguous()
                keep = None if mask is None else mask[g0:g0 + B].to(dev).contiguous()
                S.start_image(B, known, plan[K - K_run][1], seed, off0, stride, fake)
            elif noise is None:
                S.start(B, seed, off0, stride, fake)
            else:
                z = noise[g0:g0 + B].to(dev, torch.float32).contiguous()
                S.mix(B, z, z, 0.0, fake)       # alpha = 0: fake = 0 z + 1 z
            if start_copy:                      # the first step run reads the guide: its views take the start, once per batch
                if gstart is None or gstart.shape[0] != B:
                    gstart = torch.empty_like(fake)     # (the fp32 output of the copy: the state itself is read only)
                SG.mix(B, fake, fake, 0.0, gstart)
            for k, (tau, a_t, a_prev, s2) in enumerate(plan, 1):
                if k <= K - K_run:              # (init with strength < 1: the front of the schedule is cut, the slots keep their steps)
                    continue
                S.set_t(B, tau)
                pred = S.evaluate(B)
                x0 = out[g0:g0 + B] if k == K else (kept[tau][g0:g0 + B] if tau in kept else None)
                off = generate_offset(first_index + g0, k, K, per_image)
                guided_entry, with_guide, write_views = launches[k - 1 - (K - K_run)] if launches is not None else (False, False, False)
                if guided_entry:
                    w, pg = weights[tau - 1], None
                    if with_guide:
                        SG.set_t(B, tau)
                        pg = SG.evaluate(B)
                    masked = init is not None and mask is not None
                    rows = None
                    if dynamic:
                        rows = S.guided_rows(B, pred, pg, w, fake, a_t, rank, floor) if with_guide else S.dynamic_rows(B, pred, fake, a_t, rank, floor)
                        if bounds is not None:
                            bounds[tau][g0:g0 + B].copy_(rows[:, 0])
                    S.guided_step(B, pred, pg, w if with_guide else 1.0, fake, hist, known if masked else None, keep if masked else None, rows,
                                  a_t, a_prev, 0.0 if multistep else s2, c1s[k - 1] if multistep else 0.0, 0.0 if dynamic else clip, seed, off, off0,
                                  stride, x0, SG.input_views(B) if write_views else (None, 0, None, 0))
                elif dynamic:
                    rows = S.dynamic_rows(B, pred, fake, a_t, rank, floor)
                    if bounds is not None:
                        bounds[tau][g0:g0 + B].copy_(rows[:, 0])
                    masked = init is not None and mask is not None
                    S.dynamic_step(B, pred, fake, hist, known if masked else None, keep if masked else None, rows, a_t, a_prev,
                                   0.0 if multistep else s2, c1s[k - 1] if multistep else 0.0, seed, off, off0, stride, x0)
                elif multistep:
                    S.multistep_step(B, pred, fake, hist, known if keep is not None else None, keep, a_t, a_prev, c1s[k - 1], clip, seed, off0,
                                     stride, x0)
                elif init is not None and mask is not None:
                    S.masked_step(B, pred, fake, known, keep, a_t, a_prev, s2, clip, seed, off, off0, stride, x0)
                else:
                    S.fused_step(B, pred, fake, a_t, a_prev, s2, clip, seed, off, stride, x0)
                if k == K and tau in kept:
                    kept[tau][g0:g0 + B].copy_(x0)
    result = (out, kept) if marks else out
    if bounds is not None:
        result = (*result, bounds) if marks else (out, bounds)
    return result


def encode(denoiser: "M.Denoiser", images: torch.Tensor, num_steps: Optional[int] = None, timesteps=None, batch_size: Optional[int] = None,
           use_ema: bool = False, use_graph: bool = True, start_eps: Optional[torch.Tensor] = None, predict_x: Optional[bool] = None,
           predict_scaled_epsilon: Optional[bool] = None, ordinary_differential_equation: Optional[bool] = None, noise_schedule=None,
           alpha_dash_offset: Optional[float] = None, solver: str = "ddim", predict_v: Optional[bool] = None) -> torch.Tensor:
    """images [n,H,W,3] into latents, fp32 [n,H,W,3] on the device: the forward loop of log_sample (train.py:364-413), strided over the
    K = num_steps timesteps of generate (trainer_math.sampling_timesteps, or an explicit `timesteps` list), ascending.  The state starts
    as x_theta = eps_theta = images like the reference's (train.py:367), or eps_theta = start_eps [n,H,W,3]; every step is one
    network evaluation at its timestep and one gct2_diffusion_step (sigma2 = 0, no clip) that re-mixes the new estimates at the NEXT
    timestep's alpha; the last re-mixes at alpha = 0, which leaves eps_theta: the latent.  At num_steps = steps it is log_sample's
    epsilon_theta.  generate(noise=latent, timesteps=...) decodes it, on this denoiser or on another one (class transfer).  batch_size
    (default min(n, 64)) only cuts the work; the objective switches, the noise schedule and use_ema resolve like generate's, the ODE
    objective is refused, and no training state moves.
    solver: "ddim" (the default: the calls and the bits described above) or "dpm2m": every step is one gct2_diffusion_step_multistep
    launch, the same second-order multistep update as generate's run up the schedule - c1 = trainer_math.multistep_coefficient(alpha of
    the timestep evaluated before, alpha(tau), alpha of the next timestep), 0 at the first step of every batch and, by the helper itself,
    at the last (it goes to alpha 0).  An unknown name is a ValueError."""
    eng = denoiser.ensure_engine()
    steps = int(eng.steps)
    if solver not in SOLVERS:
        raise ValueError(f"encode: solver must be one of {SOLVERS!r}, got {solver!r}")
    mode = _resolve_switches(eng, predict_x, predict_scaled_epsilon, ordinary_differential_equation, predict_v)
    if mode == SAMPLE_ODE:
        raise ValueError("encode: the ordinary_differential_equation objective predicts the image one step back only; a strided "
                         "inversion has no meaning there (log_sample runs its loop)")
    schedule, offset = _resolve_schedule(eng, noise_schedule, alpha_dash_offset)
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[0] < 1 or images.shape[3] != 3:
        raise ValueError(f"encode: images must be [n,H,W,3], got {tuple(getattr(images, 'shape', ()))}")
    n, H, W = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    if start_eps is not None and (not isinstance(start_eps, torch.Tensor) or tuple(start_eps.shape) != tuple(images.shape)):
        raise ValueError(f"encode: start_eps must have the images' shape {tuple(images.shape)}, got {tuple(getattr(start_eps, 'shape', ()))}")
    taus = _taus("encode", steps, num_steps, timesteps)
    K = len(taus)
    bs = min(n, 64) if batch_size is None else batch_size
    if isinstance(bs, bool) or not isinstance(bs, int) or bs < 1:
        raise ValueError(f"encode: batch_size must be a positive int, got {batch_size!r}")
    alpha = lambda t: float(alpha_dash(t, steps, schedule, offset))
    dev = eng.device
    with (eng.ema_weights() if use_ema else contextlib.nullcontext()):
        eng.flush_deferred()
        S = _Sampler(eng, steps, mode, H, W, use_graph, schedule, offset)
        out = torch.empty(n, H, W, 3, dtype=torch.float32, device=dev)
        hist = None
        for g0 in range(0, n, bs):
            B = min(bs, n - g0)
            x = images[g0:g0 + B].to(dev, torch.float32).contiguous()
            e = x if start_eps is None else start_eps[g0:g0 + B].to(dev, torch.float32).contiguous()
            fake = out[g0:g0 + B]               # (the state lives in the result's rows: the last step leaves the latent there)
            S.mix(B, x, e, alpha(taus[0]), fake)
            if solver == "dpm2m" and (hist is None or hist.shape[0] != B):
                hist = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
            for k, tau in enumerate(taus):
                S.set_t(B, tau)
                pred = S.evaluate(B)
                a_t, a_next = alpha(tau), alpha(taus[k + 1]) if k + 1 < K else 0.0
                if solver == "dpm2m":
                    c1 = multistep_coefficient(alpha(taus[k - 1]) if k else None, a_t, a_next)
                    S.multistep_step(B, pred, fake, hist, None, None, a_t, a_next, c1, 0.0, 0, 0, 0, None)
                else:
                    S.fused_step(B, pred, fake, a_t, a_next, 0.0, 0.0, 0, 0, 0, None)
    return out


def _taus(who: str, steps: int, num_steps, timesteps) -> list:
    """the ascending timesteps of a strided run: an explicit list (checked), else sampling_timesteps(steps, num_steps or steps)"""
    if timesteps is not None:
        given = list(timesteps)
        if not given or any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) for t in given) or given[0] < 1 or \
                given[-1] > steps or any(b <= a for a, b in zip(given, given[1:])):
            raise ValueError(f"{who}: timesteps must be strictly increasing integers within 1..{steps}, got {given!r}")
        if num_steps is not None and num_steps != len(given):
            raise ValueError(f"{who}: num_steps = {num_steps!r} disagrees with the {len(given)} timesteps given")
        return [int(t) for t in given]
    try:
        return sampling_timesteps(steps, steps if num_steps is None else num_steps)
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None


def _hw(size) -> Tuple[int, int]:
    """an image size as (H, W): one int is a square"""
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError(f"generate: size must be an int or (H, W), got {size!r}")
        return int(size[0]), int(size[1])
    return int(size), int(size)


def make_log_sample(denoiser: "M.Denoiser", example_image, example, dictionary, sink: Callable[[int, Dict[str, torch.Tensor]], None],
                    use_ema: bool = False):
    """callback with the reference's signature `log_sample(epochs, logs)` (train.py:323, 519-521); `sink(epoch, images)` stands
    for the TensorBoard summary writer.  use_ema: sample from the parameter averages."""
    def cb(epochs, logs):
        sink(epochs, log_sample(denoiser, example_image, example, dictionary, use_ema=use_ema))
    return cb
