"""CPU tier of Keras SGD / RMSprop and the InverseTimeDecay schedule [TF]: the schedule's float32 values, the constructors and their
argument checks, the translation into the engines' hyper-parameters (the three optimizer lines the reference keeps commented out,
train.py:69-73), the binding of the two new C entry points and every rejection they make before a launch, the host-side state
(TrainerState) and what is refused - none of which needs a device."""
import ctypes
import types

import numpy as np
import pytest

import clip_cases as K
import optimizer_cases as OC
import gan_class_transfer2_amd as g
from gan_class_transfer2_amd import trainer_math as TM

P = 4096                    # a fake, 16-byte aligned device address: every launching call below is rejected before anything reads it
S = P + 65536               # ... and an 8-byte aligned one for sumsq
EINVAL = 1


# ---- the schedule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staircase", [False, True], ids=["plain", "staircase"])
@pytest.mark.parametrize("initial, decay_steps, decay_rate", OC.REFERENCE_SCHEDULES)
def test_inverse_time_decay_values(initial, decay_steps, decay_rate, staircase):
    sched = g.InverseTimeDecay(initial, decay_steps, decay_rate, staircase)
    for k in OC.SCHEDULE_STEPS:
        want = OC.inverse_time_decay(k, initial, decay_steps, decay_rate, staircase)
        assert want.dtype == np.float32
        got = TM.inverse_time_decay_lr(k, initial, decay_steps, decay_rate, staircase)
        assert isinstance(got, float) and np.float32(got).tobytes() == want.tobytes() and got == float(want), (k, got, want)
        assert sched(k) == got
    # the schedule's landmarks, exactly: the initial rate at step 0, half of it after decay_steps
    assert TM.inverse_time_decay_lr(0, initial, decay_steps, decay_rate, staircase) == float(np.float32(initial))
    assert TM.inverse_time_decay_lr(decay_steps, initial, decay_steps, decay_rate, staircase) == float(np.float32(initial) / np.float32(2))
    if staircase:                                                    # floored: constant inside a period
        assert TM.inverse_time_decay_lr(9_999, initial, decay_steps, decay_rate, True) == float(np.float32(initial))
        assert TM.inverse_time_decay_lr(10_001, initial, decay_steps, decay_rate, True) == TM.inverse_time_decay_lr(10_000, initial, decay_steps, decay_rate, True)
    else:
        assert TM.inverse_time_decay_lr(10_001, initial, decay_steps, decay_rate) < TM.inverse_time_decay_lr(10_000, initial, decay_steps, decay_rate)


# ---- constructors -----------------------------------------------------------------------------------------------------------------
def test_constructor_defaults_are_keras():
    s = g.SGD()
    assert (s.learning_rate, s.momentum, s.nesterov) == (0.01, 0.0, False)
    r = g.RMSprop()
    assert (r.learning_rate, r.rho, r.momentum, r.epsilon, r.centered) == (0.001, 0.9, 0.0, 1e-7, False)
    for opt in (s, r):
        assert (opt.use_ema, opt.ema_momentum, opt.clipnorm, opt.global_clipnorm, opt.clipvalue) == (False, 0.99, None, None, None)
        assert opt.iterations == 0 and opt.loss_scaling is False and opt.lr(5) == opt.learning_rate
        with pytest.raises(RuntimeError, match="not bound"):
            opt.finalize_variable_values()
    d = g.InverseTimeDecay(2.0, 10_000, 1)
    assert (d.initial_learning_rate, d.decay_steps, d.decay_rate, d.staircase) == (2.0, 10_000, 1, False)
    # the reference's lines as written (positional arguments)
    s = g.SGD(0.25, 0.5, True)
    assert (s.learning_rate, s.momentum, s.nesterov) == (0.25, 0.5, True)
    assert g.SGD(d).lr(10_000) == 1.0 and g.RMSprop(g.InverseTimeDecay(1e-5, 10_000, 1)).lr(0) == float(np.float32(1e-5))
    wrapped = g.LossScaleOptimizer(g.SGD(0.25, 0.5, True))
    assert wrapped.inner.loss_scaling and wrapped.momentum == 0.5 and wrapped.nesterov is True
    assert isinstance(g.Adam(), g.model.Optimizer) and isinstance(s, g.model.Optimizer) and isinstance(r, g.model.Optimizer)


def test_constructor_argument_checks():
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            g.SGD(momentum=bad)
        with pytest.raises(ValueError, match="momentum"):
            g.RMSprop(momentum=bad)
        with pytest.raises(ValueError, match="rho"):
            g.RMSprop(rho=bad)
    for bad in (-1e-7, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            g.RMSprop(epsilon=bad)
    for bad in (0, -5, float("nan")):
        with pytest.raises(ValueError, match="decay_steps"):
            g.InverseTimeDecay(1.0, bad, 1.0)
    for ok in (dict(momentum=0.0), dict(momentum=1.0)):
        g.SGD(**ok); g.RMSprop(**ok)
    g.RMSprop(rho=0.0); g.RMSprop(rho=1.0); g.RMSprop(epsilon=0.0)
    with pytest.raises(NotImplementedError, match="centered"):
        g.RMSprop(centered=True)
    for Opt in (g.SGD, g.RMSprop):
        for kw in (dict(clipnorm=1.0, clipvalue=0.5), dict(clipnorm=1.0, global_clipnorm=1.0), dict(global_clipnorm=2.0, clipvalue=0.5)):
            with pytest.raises(ValueError, match="at most one"):
                Opt(**kw)
        for name in K_ARGS:
            assert getattr(Opt(**{name: 0.25}), name) == 0.25
            with pytest.raises(ValueError, match=name):
                Opt(**{name: -1.0})
        with pytest.raises(ValueError, match="ema_momentum"):
            Opt(use_ema=True, ema_momentum=1.5)
        with pytest.raises(NotImplementedError, match="ema_overwrite_frequency"):
            Opt(ema_overwrite_frequency=10)


K_ARGS = ("clipnorm", "global_clipnorm", "clipvalue")


# ---- the translation --------------------------------------------------------------------------------------------------------------
def test_engine_hyper_parameters_of_the_reference_lines():
    hp = g.model.engine_hyper_parameters
    assert hp(g.SGD(0.25, 0.5, True)) == dict(optimizer_kind="sgd", momentum=0.5, nesterov=True, base_lr=0.25, warm_up=0)
    assert hp(g.SGD(g.InverseTimeDecay(2.0, 10_000, 1))) == dict(optimizer_kind="sgd", momentum=0.0, nesterov=False,
                                                                 lr_schedule=("inverse_time_decay", 2.0, 10_000.0, 1.0, False))
    assert hp(g.RMSprop(g.InverseTimeDecay(1e-5, 10_000, 1))) == dict(optimizer_kind="rmsprop", rho=0.9, momentum=0.0, epsilon=1e-7,
                                                                      lr_schedule=("inverse_time_decay", 1e-5, 10_000.0, 1.0, False))
    assert hp(g.LossScaleOptimizer(g.SGD(0.25, 0.5, True))) == hp(g.SGD(0.25, 0.5, True))
    assert hp(g.RMSprop(1e-3, clipvalue=0.5, use_ema=True)) == dict(optimizer_kind="rmsprop", rho=0.9, momentum=0.0, epsilon=1e-7, base_lr=1e-3,
                                                                    warm_up=0, use_ema=True, ema_momentum=0.99, clip_mode=K.CLIP_VALUE, clip=0.5)
    # Adam with the new schedule; and the default optimizer's dictionary is the literal it always was
    assert hp(g.Adam(g.InverseTimeDecay(2.0, 10_000, 1, True))) == dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                                                                       lr_schedule=("inverse_time_decay", 2.0, 10_000.0, 1.0, True))
    assert hp(g.model.default_optimizer()) == dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7, base_lr=2e-5, warm_up=g.model.warm_up)


def test_a_callable_learning_rate_of_another_type_is_still_refused():
    class Cosine:
        def __call__(self, step):
            return 1e-3

    for opt in (g.SGD(Cosine()), g.RMSprop(lambda step: 1e-3), g.Adam(Cosine())):
        hp = g.model.engine_hyper_parameters(opt)
        assert "base_lr" not in hp and "lr_schedule" not in hp
        tr = g.Trainer(types.SimpleNamespace(engine=None))
        tr.compile(opt, g.identity)
        with pytest.raises(NotImplementedError, match="WarmUp, InverseTimeDecay or constant"):
            tr._engine()


# ---- the host-side state ------------------------------------------------------------------------------------------------------------
class Stub(TM.TrainerState):
    """TrainerState without a device: the attributes its optimizer methods read"""

    def __init__(self, iterations=0):
        self.base_lr, self.warm_up, self.beta_1, self.beta_2, self.epsilon = 1e-2, 4, 0.9, 0.999, 1e-7
        self._iterations, self.ls_state, self.loss_scaling = iterations, None, False
        self.flushed = 0

    def flush_deferred(self):
        self.flushed += 1

    def _ema_tensors(self):
        return None, None


def test_trainer_state_defaults_dispatch_and_the_kind_rule():
    e = Stub()
    assert (e.optimizer_kind, e.momentum, e.nesterov, e.rho, e.lr_schedule) == ("adam", 0.0, False, 0.9, None)
    assert "optimizer_kind" not in vars(e) and "lr_schedule" not in vars(e)        # class-level defaults: an Adam engine carries nothing new
    assert e.learning_rate(1) == TM.warmup_lr(1, 1e-2, 4) and e.step_size(1) == e.adam_alpha(1) != e.learning_rate(1)
    e.set_optimizer("sgd", momentum=0.5, nesterov=True)
    assert (e.optimizer_kind, e.momentum, e.nesterov, e.flushed) == ("sgd", 0.5, True, 1)
    assert e.step_size(1) == e.learning_rate(1) == TM.warmup_lr(1, 1e-2, 4)
    e.lr_schedule = TM.inverse_time_decay_schedule(2.0, 10_000, 1, False)
    for k in OC.SCHEDULE_STEPS:
        assert e.learning_rate(k) == e.step_size(k) == float(OC.inverse_time_decay(k, 2.0, 10_000, 1))
    e.set_optimizer("adam")                                          # Adam reads the same schedule through adam_alpha
    assert e.step_size(3) == TM.adam_step_size(float(OC.inverse_time_decay(3, 2.0, 10_000, 1)), 3, 0.9, 0.999)
    for bad in (dict(kind="adagrad"), dict(kind="sgd", momentum=2.0), dict(kind="rmsprop", rho=-1.0)):
        with pytest.raises(ValueError):
            e.set_optimizer(**bad)
    assert e.optimizer_kind == "adam"
    # after applied steps the kind is fixed; its hyper-parameters are not
    e = Stub(iterations=3)
    with pytest.raises(g.Gct2Error, match="already applied 3 steps"):
        e.set_optimizer("sgd")
    assert e.optimizer_kind == "adam" and e.flushed == 0
    e = Stub()
    e.set_optimizer("rmsprop", rho=0.8)
    e._iterations = 2
    e.set_optimizer("rmsprop", rho=0.7, momentum=0.9)
    assert (e.rho, e.momentum) == (0.7, 0.9)
    with pytest.raises(g.Gct2Error, match="rmsprop"):
        e.set_optimizer("adam")
    # an engine driven by a data-parallel wrapper stays with Adam
    e = Stub()
    e._optimizer_forbidden = "driven by a wrapper"
    with pytest.raises(ValueError, match="driven by a wrapper"):
        e.set_optimizer("sgd")
    e.set_optimizer("adam")


def test_compile_applies_kind_and_schedule_to_an_existing_engine():
    eng = Stub()
    tr = g.Trainer(types.SimpleNamespace(engine=eng))
    tr.compile(g.SGD(g.InverseTimeDecay(2.0, 10_000, 1)), g.identity)
    assert eng.optimizer_kind == "sgd" and eng.lr_schedule == ("inverse_time_decay", 2.0, 10_000.0, 1.0, False) and eng.base_lr == 1e-2
    tr.compile(g.RMSprop(1e-3, rho=0.8, momentum=0.5, epsilon=1e-6), g.identity)
    assert (eng.optimizer_kind, eng.rho, eng.momentum, eng.epsilon, eng.lr_schedule, eng.base_lr, eng.warm_up) == ("rmsprop", 0.8, 0.5, 1e-6, None, 1e-3, 0)
    tr.compile(g.model.default_optimizer(), g.identity)
    assert eng.optimizer_kind == "adam" and eng.lr_schedule is None and (eng.base_lr, eng.warm_up) == (2e-5, g.model.warm_up)
    eng._iterations = 1
    before = (eng.base_lr, eng.warm_up, eng.epsilon)
    with pytest.raises(g.Gct2Error, match="already applied"):
        tr.compile(g.SGD(0.25, 0.5, True), g.identity)
    assert eng.optimizer_kind == "adam" and (eng.base_lr, eng.warm_up, eng.epsilon) == before      # refused before anything was written


def test_wrappers_refuse_an_engine_that_is_not_adam():
    from gan_class_transfer2_amd.distributed import _refuse_optimizer
    eng = Stub()
    why = _refuse_optimizer(eng, "DataParallelStep")
    assert "DataParallelStep" in why and not hasattr(eng, "_optimizer_forbidden")
    eng.set_optimizer("sgd", momentum=0.5)
    with pytest.raises(ValueError, match="DataParallelStep.*sgd"):
        _refuse_optimizer(eng, "DataParallelStep")


def test_plan_key_and_checkpoint_code_cover_the_kind():
    import inspect
    src = inspect.getsource(g.UNetEngine._plan_key)
    for name in ("optimizer_kind", "momentum", "nesterov", "rho", "lr_schedule"):
        assert "self." + name in src, name
    assert TM.OPTIMIZER_KINDS == {"adam": 0, "sgd": OC.SGD, "rmsprop": OC.RMSPROP}


# ---- the binding ------------------------------------------------------------------------------------------------------------------
def test_both_entry_points_are_declared_exported_bound_and_plannable():
    L = g._lib
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert hasattr(raw, "gct2_optimizer_apply") and hasattr(raw, "gct2_loss_scale_begin_schedule") and hasattr(raw, "gct2_loss_scale_begin")
    assert L.SIGNATURES["gct2_optimizer_apply"] == [i, vp, vp, vp, vp, vp, i, sz, f, f, i, f, f, f, vp, i, f, vp, vp]
    assert L.SIGNATURES["gct2_loss_scale_begin_schedule"] == [vp, i, f, f, f, i, i, f, f, vp]
    assert {"gct2_optimizer_apply", "gct2_loss_scale_begin_schedule"} <= L.PLANNABLE
    assert lib.gct2_abi_version() == L.ABI_VERSION == 17              # additions change no signature
    assert (L.OPT_ADAM, L.OPT_SGD, L.OPT_RMSPROP) == (0, OC.SGD, OC.RMSPROP) == (0, 1, 2)
    assert (L.SCHEDULE_WARMUP, L.SCHEDULE_INVERSE_TIME_DECAY) == (OC.WARMUP, OC.INVERSE_TIME_DECAY) == (0, 1)
    header = open(L.os.path.join(L._HERE, "..", "include", "gct2.h")).read()
    for text in ("int gct2_optimizer_apply(int kind, float* p, float* m, float* v, float* g, void* shadow, int shadow_dtype, size_t n,",
                 "int gct2_loss_scale_begin_schedule(gct2_loss_scale_state* state, int schedule, float initial, float steps, float decay_rate,",
                 "#define GCT2_OPT_SGD 1", "#define GCT2_OPT_RMSPROP 2", "#define GCT2_SCHEDULE_WARMUP 0", "#define GCT2_SCHEDULE_INVERSE_TIME_DECAY 1",
                 "gct2_optimizer_apply, gct2_loss_scale_begin_schedule (additive)", "PARITY UNPINNED"):
        assert text in header, text
    for name, nargs, text in (("gct2_optimizer_apply", 19, b"optimizer_apply: unknown kind 0"),
                              ("gct2_loss_scale_begin_schedule", 10, b"loss_scale_begin_schedule: null state")):
        plan = L.Plan()
        idx = ctypes.c_int(-1)
        arr = (ctypes.c_uint64 * nargs)()
        assert lib.gct2_plan_add_call(plan.handle, name.encode(), arr, nargs, ctypes.byref(idx)) == 0 and idx.value == 0
        assert lib.gct2_plan_add_call(plan.handle, name.encode(), arr, nargs - 1, None) == EINVAL
        assert b"takes %d arguments" % nargs in lib.gct2_last_error()
        # the recorded call (all-zero arguments) is rejected by its own checks when the plan runs: nothing is launched
        failed = ctypes.c_int(-1)
        assert lib.gct2_plan_run(plan.handle, 0, 1, ctypes.byref(failed)) == EINVAL and failed.value == 0
        assert text in lib.gct2_last_error()


def _opt(**o):
    a = dict(kind=OC.RMSPROP, p=P, m=P + 4096, v=P + 8192, g=P + 12288, shadow=None, dtype=g.F32, n=1024, lr=1e-3, momentum=0.9, nesterov=0,
             rho=0.9, eps=1e-7, grad_mul=1.0, ls=None, mode=K.CLIP_NONE, clip=0.0, sumsq=None, stream=None)
    assert not set(o) - set(a)
    a.update(o)
    return list(a.values())


@pytest.mark.parametrize("args, text", [
    (_opt(kind=0), "unknown kind 0"),                                # Adam stays where it is
    (_opt(kind=3), "unknown kind 3"),
    (_opt(kind=-1), "unknown kind -1"),
    (_opt(momentum=-0.5), "momentum -0.5 outside [0, 1]"),
    (_opt(momentum=1.5), "momentum 1.5 outside [0, 1]"),
    (_opt(momentum=float("nan")), "outside [0, 1]"),
    (_opt(rho=1.5), "rho 1.5 outside [0, 1]"),
    (_opt(rho=float("nan")), "outside [0, 1]"),
    (_opt(eps=-1.0), "epsilon -1 < 0"),
    (_opt(p=None), "null pointer"),
    (_opt(g=None), "null pointer"),
    (_opt(m=None), "null pointer"),                                  # RMSprop with momentum uses both slots
    (_opt(v=None), "null pointer"),
    (_opt(kind=OC.SGD, m=None), "null pointer"),                     # SGD with momentum uses m
    (_opt(n=0), "n == 0"),
    (_opt(p=P + 8), "16-byte aligned"),
    (_opt(g=P + 12288 + 4), "16-byte aligned"),
    (_opt(m=P + 4096 + 4), "16-byte aligned"),
    (_opt(v=P + 8192 + 8), "16-byte aligned"),
    (_opt(shadow=P + 16384 + 4, dtype=g.BF16), "8-byte aligned"),
    (_opt(mode=K.CLIP_GLOBAL_NORM, clip=1.0, sumsq=S + 4), "8-byte aligned"),
    (_opt(shadow=P + 16384, dtype=g.F32), "16-bit dtype"),
    (_opt(shadow=P + 16384, dtype=7), "16-bit dtype"),
    (_opt(mode=4, clip=1.0), "unknown clip_mode 4"),
    (_opt(mode=K.CLIP_VALUE, clip=0.0), "must be finite and > 0"),
    (_opt(mode=K.CLIP_NORM, clip=float("inf"), sumsq=S), "must be finite and > 0"),
    (_opt(mode=K.CLIP_NORM, clip=1.0), "clip_mode 2 needs sumsq"),
    (_opt(mode=K.CLIP_GLOBAL_NORM, clip=1.0), "clip_mode 3 needs sumsq"),
    # two mistakes: the earlier check names the call
    (_opt(kind=7, p=None), "unknown kind 7"),
    (_opt(momentum=2.0, n=0), "momentum 2 outside [0, 1]"),
    (_opt(p=None, n=0), "null pointer"),
])
def test_optimizer_apply_rejects_bad_arguments_without_a_device(args, text):
    lib = g._lib.load()
    assert lib.gct2_optimizer_apply(*args) == EINVAL
    msg = lib.gct2_last_error().decode()
    assert msg.startswith("optimizer_apply: ") and text in msg, msg


def _begin(**o):
    a = dict(state=P, schedule=OC.INVERSE_TIME_DECAY, initial=2.0, steps=10_000.0, decay_rate=1.0, staircase=0, bias_correction=0, beta1=0.9,
             beta2=0.999, stream=None)
    assert not set(o) - set(a)
    a.update(o)
    return list(a.values())


@pytest.mark.parametrize("args, text", [
    (_begin(state=None), "null state"),
    (_begin(schedule=2), "unknown schedule 2"),
    (_begin(schedule=-1), "unknown schedule -1"),
    (_begin(steps=0.0), "decay_steps 0 must be > 0"),
    (_begin(steps=-3.0), "decay_steps -3 must be > 0"),
    (_begin(steps=float("nan")), "must be > 0"),
    (_begin(schedule=OC.WARMUP, steps=-1.0), "warm-up steps -1 must be a whole number"),
    (_begin(schedule=OC.WARMUP, steps=2.5), "warm-up steps 2.5 must be a whole number"),
    (_begin(schedule=OC.WARMUP, steps=float("nan")), "must be a whole number"),
    (_begin(schedule=OC.WARMUP, steps=2.0 ** 25), "must be a whole number in [0, 2^24]"),
    (_begin(state=None, schedule=9), "null state"),
])
def test_loss_scale_begin_schedule_rejects_bad_arguments_without_a_device(args, text):
    lib = g._lib.load()
    assert lib.gct2_loss_scale_begin_schedule(*args) == EINVAL
    msg = lib.gct2_last_error().decode()
    assert msg.startswith("loss_scale_begin_schedule: ") and text in msg, msg


# ---- the call lists ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_scaled", [False, True], ids=["host_counter", "loss_scaled"])
def test_launch_helper_and_begin_step_call_lists(monkeypatch, loss_scaled):
    """_update_launches for SGD / RMSprop in the four clipping modes (gct2_grad_sumsq first for the two norm modes, then the update
    once or per tensor; only the slots in use are handed over) and which begin entry point begin_step calls"""
    calls = []
    monkeypatch.setattr(TM, "call", lambda name, *a: calls.append((name, [x.value if type(x) is TM.Slot else x for x in a])))

    class T:
        def __init__(self, base):
            self.base = base

        def data_ptr(self):
            return self.base

    class E(Stub):
        dtype = 1

        def arm(self):                                               # (the stand-in state holds no counter: set after set_optimizer)
            self.ls_state = T(777) if loss_scaled else None
            self._iterations = 2

        def _stream(self):
            return 5

        def _clip_reduction(self):
            return T(10_000), 2, 3, T(20_000), T(30_000), [(0, 100), (128, 60)]

    p, m, v, gr, sh = T(1 << 20), T(2 << 20), T(3 << 20), T(4 << 20), T(5 << 20)
    ls = 777 if loss_scaled else None
    for kind, hyper, use_m, use_v in (("sgd", dict(), False, False), ("sgd", dict(momentum=0.5, nesterov=True), True, False),
                                      ("rmsprop", dict(rho=0.8), False, True), ("rmsprop", dict(rho=0.8, momentum=0.9), True, True)):
        e = E()
        e.set_optimizer(kind, **hyper)
        e.arm()
        lr = 0.0 if loss_scaled else TM.warmup_lr(2, 1e-2, 4)
        for mode, kw in ((K.CLIP_NONE, {}), (K.CLIP_VALUE, dict(clipvalue=0.5)), (K.CLIP_GLOBAL_NORM, dict(global_clipnorm=0.5)),
                         (K.CLIP_NORM, dict(clipnorm=0.5))):
            e.set_clipping(**kw)
            del calls[:]
            e._update_launches(p, m, v, gr, sh, 64, 256, 0.5, 9)
            thr = 0.5 if kw else 0.0

            def update(lo, n, ss):
                return ("gct2_optimizer_apply", [TM.OPTIMIZER_KINDS[kind], p.base + 4 * lo, m.base + 4 * lo if use_m else None,
                                                 v.base + 4 * lo if use_v else None, gr.base + 4 * lo, sh.base + 2 * lo, 1, n, lr,
                                                 e.momentum, int(e.nesterov), e.rho, 1e-7, 0.5, ls, mode, thr, ss, 9])
            reduce = ("gct2_grad_sumsq", [gr.base, 10_000, 2, 3, 0.5, ls, 20_000, 30_000, 9])
            if mode in (K.CLIP_NONE, K.CLIP_VALUE):
                assert calls == [update(64, 192, None)]
            elif mode == K.CLIP_GLOBAL_NORM:
                assert calls == [reduce, update(64, 192, 30_000 + 16)]
            else:
                assert calls == [reduce, update(0, 100, 30_000), update(128, 60, 30_000 + 8)]
    # begin_step: nothing without a device-side counter; the old entry point for Adam + WarmUp; the new one for everything else
    e = E()
    sched = TM.inverse_time_decay_schedule(2.0, 10_000, 1, True)
    want = {("adam", None): ("gct2_loss_scale_begin", [777, 1e-2, 4, 0.9, 0.999, 5]),
            ("adam", sched): ("gct2_loss_scale_begin_schedule", [777, 1, 2.0, 10_000.0, 1.0, 1, 1, 0.9, 0.999, 5]),
            ("sgd", None): ("gct2_loss_scale_begin_schedule", [777, 0, 1e-2, 4.0, 0.0, 0, 0, 0.9, 0.999, 5]),
            ("rmsprop", sched): ("gct2_loss_scale_begin_schedule", [777, 1, 2.0, 10_000.0, 1.0, 1, 0, 0.9, 0.999, 5])}
    for (kind, schedule), expected in want.items():
        e._iterations, e.ls_state = 0, None
        e.set_optimizer(kind)
        e.lr_schedule = schedule
        e.arm()
        del calls[:]
        e.begin_step()
        assert calls == ([expected] if loss_scaled else []), (kind, schedule)


# ---- the restatement on its own -----------------------------------------------------------------------------------------------------
def test_restatement_by_hand():
    """values small enough to follow by hand, all exact in float32"""
    f = np.float32
    assert (OC.SGD, OC.RMSPROP) == (g._lib.OPT_SGD, g._lib.OPT_RMSPROP)      # the kinds apply() dispatches on are the binding's
    p, m, v, gr = f([1.0, -2.0]), f([0.5, 0.25]), f([4.0, 0.0]), f([2.0, -4.0])
    # plain SGD, lr = 0.25: p - 0.25 g
    got = OC.sgd(p, None, gr, 0.25)
    assert got[0].tolist() == [0.5, -1.0] and got[1] is None
    # momentum 0.5: m = 0.5 m - 0.25 g = [0.25 - 0.5, 0.125 + 1] = [-0.25, 1.125]; p + m
    p2, m2 = OC.sgd(p, m, gr, 0.25, 0.5)
    assert m2.tolist() == [-0.25, 1.125] and p2.tolist() == [0.75, -0.875]
    # Nesterov: p + (0.5 m_new - 0.25 g) = [1 + (-0.125 - 0.5), -2 + (0.5625 + 1)]
    p3, m3 = OC.sgd(p, m, gr, 0.25, 0.5, True)
    assert m3.tolist() == [-0.25, 1.125] and p3.tolist() == [0.375, -0.4375]
    # RMSprop, rho = 0.75, epsilon = 0: v = 0.75 v + 0.25 g^2 = [3 + 1, 0 + 4] = [4, 4]; p - lr g / sqrt(v) = [1 - 0.25, -2 + 0.5]
    p4, m4, v4 = OC.rmsprop(p, None, v, gr, 0.25, 0.75, 0.0, 0.0)
    assert v4.tolist() == [4.0, 4.0] and p4.tolist() == [0.75, -1.5] and m4 is None
    # ... with momentum 0.5: m = 0.5 m + lr g / sqrt(v + 0) = [0.25 + 0.25, 0.125 - 0.5]; p - m
    p5, m5, v5 = OC.rmsprop(p, m, v, gr, 0.25, 0.75, 0.5, 0.0)
    assert m5.tolist() == [0.5, -0.375] and p5.tolist() == [0.5, -1.625] and v5.tolist() == [4.0, 4.0]
    # epsilon outside the root without momentum, inside it with: v = 0, g = 0 divides by epsilon / sqrt(epsilon) - no NaN
    z = f([0.0])
    assert OC.rmsprop(z, None, z, z, 1.0, 0.9, 0.0, 1e-7)[0].tolist() == [0.0] and OC.rmsprop(z, z, z, z, 1.0, 0.9, 0.5, 1e-7)[0].tolist() == [0.0]
    # apply(): scaling and clipping in front, unused slots handed back untouched
    poison = f([np.nan, np.nan])
    out = OC.apply(OC.SGD, p, poison, poison, gr * 4, 0.25, {}, K.CLIP_VALUE, 2.0, grad_mul=0.5, inv_scale=0.5)
    assert out[0].tolist() == [0.5, -1.5] and out[1] is poison and out[2] is poison
    out = OC.apply(OC.RMSPROP, p, poison, v, gr, 0.25, dict(rho=0.75, epsilon=0.0))
    assert out[0].tolist() == [0.75, -1.5] and out[1] is poison and out[2].tolist() == [4.0, 4.0]
    assert all(a.dtype == np.float32 for a in (p2, m2, p4, v4, p5, m5))
