"""Progressive distillation (Salimans & Ho 2022, "Progressive Distillation for Fast Sampling of Diffusion Models"): a student learns to
do in ONE DDIM step what its teacher does in two; repeating it takes 2N sampling steps to N, then N / 2, and so on.

Per image of a batch: a pair of teacher steps t -> t' -> t'' is drawn, the image is noised to z_t, the teacher takes its two steps, and
the x~ is solved for that makes ONE DDIM step from z_t land on the teacher's z''.  The student is then handed the pseudo pair
(x~, eps~), eps~ = (z_t - sa_t x~) / sb_t, through the ordinary `train_step(x~, t_int=t, eps=eps~)`: it sees the teacher's z_t up to
rounding, and its target is the distillation target in whatever objective it is configured for - x, eps, scaled eps or v.  No new
training path; the student's loss weighting, optimizer, averages, clipping and head switches work through its own step unchanged.

The pointwise work around the two teacher evaluations is three launches (gct2_distill_start / _step / _target, include/gct2.h):
a batch holds a different timestep per image, which the sampler's scalar-coefficient kernels cannot express."""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, Iterable, Optional

import torch

from . import model as M
from ._lib import SAMPLE_ODE, call
from .sampler import _Sampler, sample_mode
from .trainer_math import DISTILL_STREAM_EPS, DISTILL_STREAM_PAIR, distill_grid, distill_table


def _engine_mode(eng) -> int:
    """the objective an engine was set up for, as a sampler mode (its own switches, not the module globals)"""
    return sample_mode(eng.predict_x, eng.predict_scaled_epsilon, eng.ordinary_differential_equation,
                       predict_v=getattr(eng, "predict_v", False))


def _engine_schedule(eng):
    return getattr(eng, "noise_schedule", "quadratic"), float(getattr(eng, "alpha_dash_offset", 0.0))


def clone_denoiser(denoiser: "M.Denoiser") -> "M.Denoiser":
    """a student for `denoiser`: a new Denoiser of the same configuration (the module switches as they stand, which built the teacher
    too) holding the teacher's weights.  Only the parameters are copied, by name (get_params / set_params: the raw weights, not the
    averages): the optimizer slots, the step counter, the RNG positions and the loss-scale state are the fresh engine's own - the paper
    re-initialises the optimizer every round - so the teacher's optimizer kind and loss scaling need not be the student's."""
    teng = denoiser.ensure_engine()
    student = M.Denoiser(seed=denoiser._seed, device=denoiser._device)
    seng = student.ensure_engine()
    teng.flush_deferred()                       # (optimizer launches the teacher's last step held back)
    have, want = teng.get_params(), seng.get_params()
    if type(seng) is not type(teng) or int(seng.steps) != int(teng.steps) or \
            {k: v.shape for k, v in have.items()} != {k: v.shape for k, v in want.items()}:
        raise ValueError("clone_denoiser: the module switches have changed since the teacher was built (another topology, head or steps)")
    seng.set_params(have)
    return student


class Distiller:
    """one round of progressive distillation: `teacher` (a Denoiser, read only) into the student behind `trainer` (a compiled Trainer),
    which is to sample in N = student_steps steps what the teacher samples in 2N.

    timesteps: the teacher's 2N timesteps (trainer_math.distill_grid; None: sampling_timesteps(steps, 2N), whose odd members are
    sampling_timesteps(steps, N) - the distilled student is sampled with plain generate(num_steps=N)).  clip_denoised: the teacher's clip
    of its x0 estimates, as in generate (True, a bound, None); "dynamic" is refused.  teacher_use_ema: the teacher's evaluations read its
    parameter averages.  use_graph: they replay the captured forward pass, as generate's do.
    Sample k of a run (a running index over every image the Distiller has trained on) draws its pair from position k of Philox stream
    DISTILL_STREAM_PAIR and its noise from positions [k HW3, (k + 1) HW3) of stream DISTILL_STREAM_EPS under `seed`: the targets do not
    depend on the batch size, and a Distiller reloaded from state_dict() continues bit for bit.
    Teacher and student objectives may differ (an eps teacher trains a v student).  ValueError: the ODE objective on either side,
    different steps / noise schedule / offset, clip_denoised="dynamic", a data-parallel wrapper on either side, teacher and student
    being the same object.  Not covered: stochastic (eta > 0), dpm2m and dynamic-threshold teachers, masks and init.  What
    distillation does to the sample quality of a trained network is not measured in this project."""

    def __init__(self, teacher, trainer, student_steps: int, *, timesteps=None, clip_denoised=None, seed: int = 0,
                 teacher_use_ema: bool = False, use_graph: bool = True):
        from .distributed import DataParallelStep, ShardedDataParallelStep
        wrappers = (DataParallelStep, ShardedDataParallelStep)
        if isinstance(teacher, wrappers) or isinstance(trainer, wrappers):
            raise ValueError("Distiller: the data-parallel wrappers are not covered (pass the Denoiser and its Trainer)")
        student = trainer.denoiser
        if student is teacher:
            raise ValueError("Distiller: teacher and student are the same object (clone_denoiser makes the student)")
        self.teacher, self.trainer = teacher, trainer
        teng, seng = teacher.ensure_engine(), self._student_engine()
        if teng is seng:
            raise ValueError("Distiller: teacher and student share one engine (clone_denoiser makes the student)")
        for who, eng in (("teacher", teng), ("student", seng)):
            if getattr(eng, "grad_ready_hook", None) is not None or getattr(eng, "_masters_sharded", False):
                raise ValueError(f"Distiller: the {who}'s engine is driven by a data-parallel wrapper, which is not covered")
            if _engine_mode(eng) == SAMPLE_ODE:
                raise ValueError(f"Distiller: the {who} is set up for the ordinary_differential_equation objective, which predicts one "
                                 "step back only: there is no strided DDIM step to distill")
        if int(teng.steps) != int(seng.steps) or _engine_schedule(teng) != _engine_schedule(seng):
            raise ValueError(f"Distiller: teacher (steps {teng.steps}, schedule {_engine_schedule(teng)!r}) and student (steps {seng.steps}, "
                             f"schedule {_engine_schedule(seng)!r}) must share steps, noise schedule and offset: the student is handed the "
                             "teacher's z_t at the teacher's timestep")
        if isinstance(clip_denoised, str):
            raise ValueError(f'Distiller: clip_denoised must be True, False, None or a finite bound > 0 ("dynamic" is not covered), got '
                             f"{clip_denoised!r}")
        if clip_denoised is None or clip_denoised is False:
            self.clip = 0.0
        elif clip_denoised is True:
            self.clip = 1.0
        else:
            try:
                self.clip = float(clip_denoised)
            except (TypeError, ValueError):
                self.clip = float("nan")
            if not (self.clip > 0.0 and self.clip < float("inf")):
                raise ValueError(f"Distiller: clip_denoised must be True, False, None or a finite bound > 0, got {clip_denoised!r}")
        self.steps = int(teng.steps)
        self.mode = _engine_mode(teng)
        self.schedule, self.offset = _engine_schedule(teng)
        try:
            self.taus = distill_grid(self.steps, student_steps, timesteps)
            table, ttable = distill_table(self.taus, self.steps, self.schedule, self.offset, self.mode)
        except ValueError as e:
            raise ValueError(f"Distiller: {e}") from None
        self.student_steps = len(self.taus) // 2
        self.table = torch.from_numpy(table).to(teng.device)
        self.ttable = torch.from_numpy(ttable).to(teng.device)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.next_sample = 0
        self.teacher_use_ema, self.use_graph = bool(teacher_use_ema), bool(use_graph)
        self._sets: Dict[tuple, dict] = {}

    def _student_engine(self):
        """the student's engine as its Trainer resolves it (the module's objective switches as they stand now, train.py:238-252)"""
        resolve = getattr(self.trainer, "_engine", None)
        return resolve() if resolve is not None else self.trainer.denoiser.ensure_engine()

    def _buffers(self, B: int, H: int, W: int, dev) -> dict:
        held = self._sets.get((B, H, W))
        if held is None:
            plane = lambda: torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
            ints = lambda: torch.empty(B, dtype=torch.int32, device=dev)
            held = self._sets[(B, H, W)] = dict(pair=ints(), t=ints(), t1=ints(), z=plane(), z1=plane(), x=plane(), eps=plane())
        return held

    def targets(self, images: torch.Tensor, first_sample: Optional[int] = None, pair: Optional[torch.Tensor] = None,
                eps: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """the student's pseudo batch for images [B,H,W,3]: dict(x, eps, t, z) = x~ and eps~ (fp32 [B,H,W,3]), the timestep per image
        (int32 [B]) and the teacher's z_t.  Five launches around two teacher evaluations: the pair draw, gct2_distill_start, [teacher],
        gct2_distill_step, [teacher], gct2_distill_target.  The images are samples first_sample, first_sample + 1, ... of the run (None:
        where the Distiller stands; the position is moved by step alone).  pair (int32 [B], 1..N) and eps (fp32 [B,H,W,3]) pin the draws
        instead.  The tensors belong to the Distiller and are valid until its next call at this batch shape.  No training state of
        either network moves."""
        teng = self.teacher.ensure_engine()
        dev = teng.device
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[0] < 1 or images.shape[3] != 3:
            raise ValueError(f"Distiller.targets: images must be [B,H,W,3], got {tuple(getattr(images, 'shape', ()))}")
        x = images.to(dev, torch.float32).contiguous()
        B, H, W, _ = x.shape
        per_image = H * W * 3
        k0 = self.next_sample if first_sample is None else int(first_sample)
        if k0 < 0 or (k0 + B) * per_image >= 1 << 64:
            raise ValueError(f"Distiller.targets: first_sample = {k0!r} leaves the 64-bit stream")
        buf = self._buffers(B, H, W, dev)
        N = self.student_steps
        with (teng.ema_weights() if self.teacher_use_ema else contextlib.nullcontext()):
            teng.flush_deferred()
            S = _Sampler(teng, self.steps, self.mode, H, W, self.use_graph, self.schedule, self.offset)
            s = S._stream()
            if pair is None:
                call("gct2_rng_uniform_int", self.seed, DISTILL_STREAM_PAIR, k0, buf["pair"].data_ptr(), B, 1, N, s)
            else:
                if tuple(pair.shape) != (B,):
                    raise ValueError(f"Distiller.targets: pair must be [B] = [{B}], got {tuple(pair.shape)}")
                buf["pair"].copy_(pair.to(dev, torch.int32))
            if eps is not None:
                if tuple(eps.shape) != tuple(x.shape):
                    raise ValueError(f"Distiller.targets: eps must have the images' shape {tuple(x.shape)}, got {tuple(eps.shape)}")
                eps = eps.to(dev, torch.float32).contiguous()
            tabs = (buf["pair"].data_ptr(), self.table.data_ptr())
            views = (*S.input_views(B), B, per_image, 3, s)
            call("gct2_distill_start", teng.dtype, x.data_ptr(), eps.data_ptr() if eps is not None else None, *tabs, self.ttable.data_ptr(),
                 N, self.seed, DISTILL_STREAM_EPS, k0 * per_image, per_image, buf["z"].data_ptr(), buf["t"].data_ptr(),
                 buf["t1"].data_ptr(), *views)
            S.set_t_rows(B, buf["t"])
            pred = S.evaluate(B)
            call("gct2_distill_step", self.mode, teng.dtype, pred.data_ptr(), buf["z"].data_ptr(), *tabs, N, self.clip,
                 buf["z1"].data_ptr(), *views)
            S.set_t_rows(B, buf["t1"])
            pred = S.evaluate(B)
            call("gct2_distill_target", self.mode, pred.data_ptr(), buf["z1"].data_ptr(), buf["z"].data_ptr(), *tabs, N, self.clip,
                 buf["x"].data_ptr(), buf["eps"].data_ptr(), B, per_image, s)
        return dict(x=buf["x"], eps=buf["eps"], t=buf["t"], z=buf["z"])

    def step(self, images: torch.Tensor) -> torch.Tensor:
        """targets, then the student's train_step(x~, t_int=t, eps=eps~); returns its loss (a 1-element device tensor)"""
        tg = self.targets(images)
        eng = self._student_engine()
        loss = eng.train_step(tg["x"], t_int=tg["t"], eps=tg["eps"])
        inner = getattr(getattr(self.trainer, "optimizer", None), "inner", getattr(self.trainer, "optimizer", None))
        if inner is not None:
            inner._engine = eng
        self.next_sample += int(images.shape[0])
        return loss

    def fit(self, dataset: Iterable, steps_per_epoch: int = 1000, epochs: int = 1, callbacks=(), verbose: int = 1) -> dict:
        """Trainer.fit's loop over step: `dataset` yields images or (image, image) batches; one host synchronisation per epoch"""
        it = iter(dataset)
        history = {"loss": []}
        for epoch in range(epochs):
            logs: Dict[str, float] = {}
            for cb in callbacks:
                if getattr(cb, "on_epoch_begin", None):
                    cb.on_epoch_begin(epoch, logs)
            running = None
            for _ in range(steps_per_epoch):
                data = next(it)
                loss = self.step(data[0] if isinstance(data, (tuple, list)) else data)
                running = loss.clone() if running is None else running + loss
            logs["loss"] = float(running[0]) / steps_per_epoch
            history["loss"].append(logs["loss"])
            if verbose:
                print(f"Distill to {self.student_steps} steps, epoch {epoch + 1}/{epochs} - loss: {logs['loss']:.6f}", flush=True)
            for cb in callbacks:
                if getattr(cb, "on_epoch_end", None):
                    cb.on_epoch_end(epoch, logs)
        return history

    def state_dict(self) -> dict:
        return {"seed": self.seed, "next_sample": self.next_sample, "student_steps": self.student_steps}

    def load_state_dict(self, sd: dict) -> None:
        if int(sd["student_steps"]) != self.student_steps:
            raise ValueError(f"Distiller: the state was written at student_steps = {int(sd['student_steps'])}, this one runs "
                             f"{self.student_steps}")
        self.seed, self.next_sample = int(sd["seed"]) & 0xFFFFFFFFFFFFFFFF, int(sd["next_sample"])


def progressive_distill(denoiser: "M.Denoiser", dataset: Iterable, start_steps: int, end_steps: int, steps_per_round: int,
                        make_optimizer: Callable[[], object], verbose: int = 1, **distiller_kw) -> "M.Denoiser":
    """rounds N = start_steps / 2, start_steps / 4, ..., end_steps: each round's student is a clone of its teacher (clone_denoiser),
    trained for steps_per_round Distiller steps under a fresh make_optimizer(), and becomes the next teacher.  Returns the last
    student, which generate(num_steps=end_steps) samples.  ValueError unless start_steps = end_steps 2^k with k >= 1."""
    start, end = int(start_steps), int(end_steps)
    if end < 1 or start <= end or start % end or (start // end) & (start // end - 1):
        raise ValueError(f"progressive_distill: start_steps must be end_steps times a power of two >= 2, got {start_steps!r}, {end_steps!r}")
    teacher, N = denoiser, start // 2
    while N >= end:
        student = clone_denoiser(teacher)
        trainer = M.Trainer(student)
        trainer.compile(make_optimizer(), M.identity)
        Distiller(teacher, trainer, N, **distiller_kw).fit(dataset, steps_per_round, 1, verbose=verbose)
        teacher, N = student, N // 2
    return teacher
