"""CPU tier of the parameter averages (Keras Adam(use_ema=True) [TF]): the C entry point is declared, exported, bound and plannable,
rejects bad arguments before any launch, and the optimizer translation carries the two hyper-parameters."""
import ctypes

import numpy as np
import pytest

import gan_class_transfer2_amd as g

P = 4096                    # a fake, 16-byte aligned device address: every call below is rejected before anything reads it
EINVAL = 1


def test_ema_update_is_exported_bound_and_plannable():
    L = g._lib
    lib = L.load()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "gct2_ema_update")
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert L.SIGNATURES["gct2_ema_update"] == [vp, vp, vp, i, sz, f, f, vp, vp]
    assert "gct2_ema_update" in L.PLANNABLE
    assert lib.gct2_abi_version() == L.ABI_VERSION == 17              # an addition changes no signature
    plan = L.Plan()
    idx = ctypes.c_int(-1)
    arr = (ctypes.c_uint64 * 9)()
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_ema_update", arr, 9, ctypes.byref(idx)) == 0 and idx.value == 0
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_ema_update", arr, 8, None) == EINVAL
    assert b"takes 9 arguments" in lib.gct2_last_error()
    # the recorded call (all-zero arguments) is rejected by its own checks when the plan runs: nothing is launched
    failed = ctypes.c_int(-1)
    assert lib.gct2_plan_run(plan.handle, 0, 1, ctypes.byref(failed)) == EINVAL and failed.value == 0
    assert b"ema_update: null pointer" in lib.gct2_last_error()


def _ema(**o):
    a = dict(ema=P, p=P + 4096, shadow=None, dtype=g.F32, n=1024, momentum=0.99, one_minus=0.01, ls=None, stream=None)
    assert not set(o) - set(a)
    a.update(o)
    return list(a.values())


@pytest.mark.parametrize("args, text", [
    (_ema(ema=None), "null pointer"),
    (_ema(p=None), "null pointer"),
    (_ema(n=0), "n == 0"),
    (_ema(ema=P + 8), "16-byte aligned"),
    (_ema(p=P + 4), "16-byte aligned"),
    (_ema(shadow=P + 8192 + 4, dtype=g.BF16), "8-byte aligned"),
    (_ema(shadow=P + 8192, dtype=g.F32), "16-bit dtype"),
    (_ema(shadow=P + 8192, dtype=7), "16-bit dtype"),
    (_ema(momentum=-0.01), "outside [0, 1]"),
    (_ema(momentum=1.5), "outside [0, 1]"),
    (_ema(momentum=float("nan")), "outside [0, 1]"),
    (_ema(momentum=float("inf")), "outside [0, 1]"),
])
def test_ema_update_rejects_bad_arguments_without_a_device(args, text):
    lib = g._lib.load()
    assert lib.gct2_ema_update(*args) == EINVAL
    msg = lib.gct2_last_error().decode()
    assert msg.startswith("ema_update: ") and text in msg, msg


def test_adam_carries_the_ema_hyper_parameters():
    hp = g.model.engine_hyper_parameters
    base = dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7, base_lr=2e-5, warm_up=2000)
    assert hp(g.Adam(g.WarmUp(2e-5, 2000), use_ema=True, ema_momentum=0.9)) == dict(base, use_ema=True, ema_momentum=0.9)
    assert hp(g.LossScaleOptimizer(g.Adam(g.WarmUp(2e-5, 2000), use_ema=True))) == dict(base, use_ema=True, ema_momentum=0.99)
    # off (the default): the keys are left out - the dictionary is the one from before the averages existed
    opt = g.model.default_optimizer()
    assert (opt.use_ema, opt.ema_momentum, opt.ema_overwrite_frequency) == (False, 0.99, None)
    assert hp(opt) == dict(base, warm_up=g.model.warm_up)
    assert hp(g.Adam(g.WarmUp(2e-5, 2000), use_ema=False, ema_momentum=0.5)) == base
    with pytest.raises(NotImplementedError, match="finalize_variable_values"):
        g.Adam(ema_overwrite_frequency=5)
    with pytest.raises(ValueError, match="ema_momentum"):
        g.Adam(use_ema=True, ema_momentum=1.5)
    assert callable(g.Adam().finalize_variable_values) and callable(g.LossScaleOptimizer(g.Adam()).finalize_variable_values)
    with pytest.raises(RuntimeError, match="not bound"):
        g.Adam(use_ema=True).finalize_variable_values()


def test_compile_switches_the_averages_of_a_live_engine():
    """Trainer.compile on an existing engine: enable_ema(momentum) / disable_ema(), never a plain attribute write"""
    import types
    calls = []
    eng = types.SimpleNamespace(ls_state=None, iterations=0, use_ema=False,
                                enable_ema=lambda m: (calls.append(("on", m)), setattr(eng, "use_ema", True)),
                                disable_ema=lambda: (calls.append(("off",)), setattr(eng, "use_ema", False)))
    tr = g.Trainer(types.SimpleNamespace(engine=eng))
    tr.compile(g.Adam(g.WarmUp(1e-4, 7)), g.identity)
    assert calls == [] and not hasattr(eng, "ema_momentum")
    tr.compile(g.Adam(g.WarmUp(1e-4, 7), use_ema=True, ema_momentum=0.9), g.identity)
    tr.compile(g.Adam(g.WarmUp(1e-4, 7), use_ema=True, ema_momentum=0.95), g.identity)
    tr.compile(g.Adam(g.WarmUp(1e-4, 7)), g.identity)
    assert calls == [("on", 0.9), ("on", 0.95), ("off",)] and eng.base_lr == 1e-4


@pytest.mark.parametrize("momentum", [0.99, 0.999])
def test_one_minus_is_formed_in_double_and_rounded_once(momentum):
    from gan_class_transfer2_amd.trainer_math import ema_coefficients
    m, c = ema_coefficients(momentum)
    assert np.float32(m) == np.float32(momentum) and m == float(np.float32(momentum))
    assert c == float(np.float32(1.0 - momentum))
    # ... which is NOT the float32 subtraction (1 - fl(momentum)): the two differ in the last bits at these momenta
    assert np.float32(c) != np.float32(1.0) - np.float32(momentum)
    # ctypes hands the engine's Python floats to the C ABI as these float32 values, unchanged
    assert ctypes.c_float(m).value == np.float32(momentum) and ctypes.c_float(c).value == np.float32(1.0 - momentum)


class _Calls:
    """stands in for _lib.call in the modules under test: the host logic below runs without a device and nothing is launched"""

    def __init__(self):
        self.log = []

    def __call__(self, name, *args):
        self.log.append((name, args))


def _host_engine(monkeypatch):
    """a UNetEngine with only the attributes the EMA host logic reads, on a CPU arena of the reference topology"""
    import torch
    from gan_class_transfer2_amd import engine as E, trainer_math as TM

    class Stub(E.UNetEngine):
        def __init__(self, **kw):
            self.__dict__.update(kw)

        def flush_deferred(self):                       # (the real one asks torch for the current HIP stream)
            if self._pending:
                self._launch_pending(0)

        def _stream(self):
            return 0

    calls = _Calls()
    monkeypatch.setattr(E, "call", calls)
    monkeypatch.setattr(TM, "call", calls)
    A = E.ParamArena(g.Topology(128, 512, 6), g.BF16, torch.device("cpu"))
    A.glorot_init(3)
    A._shadow.copy_(A._p.to(torch.bfloat16))
    eng = Stub(arena=A, dtype=g.BF16, ls_state=None, _iterations=0, _pending=[], _pending_ema=None, _plans={"stale": None}, _plan_seen={"stale": 2})
    return eng, A, calls


def test_step_end_and_deferred_launches_cover_the_arena_exactly_once(monkeypatch):
    """with deferred Adam the step-end launch covers [end of the deferred prefix, total) and a second launch over the prefix follows
    the held-back gct2_adam_apply launches, with the momentum of the step that deferred them"""
    import torch
    from gan_class_transfer2_amd.trainer_math import ema_coefficients
    eng, A, calls = _host_engine(monkeypatch)
    assert eng.use_ema is False and eng._ema is None and A.ema is None
    eng.finish_step()
    assert calls.log == [] and eng.iterations == 1                     # off: the step's call list is what it was
    eng.enable_ema(0.9)
    assert eng._plans == {} and eng._plan_seen == {}                   # recorded steps bake in the averages' addresses: dropped with them
    assert torch.equal(A.ema, A._p) and torch.equal(A.ema_shadow, A._shadow) and A.ema.data_ptr() != A._p.data_ptr()
    # no deferral: one launch over the whole arena
    eng.finish_step()
    m, c = ema_coefficients(0.9)
    assert calls.log == [("gct2_ema_update", (A._ema.data_ptr(), A._p.data_ptr(), A._ema_shadow.data_ptr(), g.BF16, A.total, m, c, None, 0))]
    del calls.log[:]
    # UpShuffle_0..2 held back (the arena's prefix)
    eng._pending = [("layer", l, g._lib.AdamArgs()) for l in ("U0", "U1", "U2")]
    cut = A.layer_ranges["U2"][1]
    assert A.layer_ranges["U0"][0] == 0 and 0 < cut < A.total
    eng.finish_step()
    assert calls.log == [("gct2_ema_update", (A._ema.data_ptr() + 4 * cut, A._p.data_ptr() + 4 * cut, A._ema_shadow.data_ptr() + 2 * cut, g.BF16,
                                              A.total - cut, m, c, None, 0))]
    assert eng._pending_ema == (((0, cut),), m, c)
    del calls.log[:]
    eng.ema_momentum = 0.5                                              # (a later change must not reach the step already made)
    eng._launch_pending(7)
    assert [n for n, _ in calls.log] == ["gct2_adam_apply"] * 3 + ["gct2_ema_update"]
    assert calls.log[-1][1] == (A._ema.data_ptr(), A._p.data_ptr(), A._ema_shadow.data_ptr(), g.BF16, cut, m, c, None, 7)
    assert eng._pending == [] and eng._pending_ema is None
    # a deferral set that is no prefix: the complement is covered in pieces, adjacent held-back ranges are merged
    del calls.log[:]
    eng._pending = [("layer", l, g._lib.AdamArgs()) for l in ("U1", "U2", "U4")]
    now, held = eng._ema_partition()
    (a0, a1), (b0, b1) = (A.layer_ranges["U1"][0], A.layer_ranges["U2"][1]), A.layer_ranges["U4"]
    assert now == [(0, a0), (a1, b0), (b1, A.total)] and held == [(a0, a1), (b0, b1)] and eng._pending_ema is None
    eng.finish_step()
    assert [a[4] for _, a in calls.log] == [a0, b0 - a1, A.total - b1] and eng._pending_ema == (((a0, a1), (b0, b1)), 0.5, 0.5)


def test_weight_pointers_follow_the_selected_weight_set(monkeypatch):
    eng, A, calls = _host_engine(monkeypatch)
    with pytest.raises(ValueError, match="no averages"):
        with eng.ema_weights():
            pass
    eng.enable_ema(0.99)
    o = A.offsets["D3.w"]
    raw = (A.wptr("D3.w"), A.pptr("D3.b"))
    assert raw == (A._shadow.data_ptr() + 2 * o, A._p.data_ptr() + 4 * A.offsets["D3.b"])
    with eng.ema_weights():
        assert eng._ema_reading and (A.wptr("D3.w"), A.pptr("D3.b")) == (A._ema_shadow.data_ptr() + 2 * o, A._ema.data_ptr() + 4 * A.offsets["D3.b"])
        with pytest.raises(g.Gct2Error, match="already active"):
            with eng.ema_weights():
                pass
        with pytest.raises(g.Gct2Error, match="ema_weights"):
            eng._refuse_training_on_averages()
    assert not eng._ema_reading and (A.wptr("D3.w"), A.pptr("D3.b")) == raw
    with pytest.raises(KeyError):
        with eng.ema_weights():
            A.wptr("no such tensor")
    assert not eng._ema_reading and (A.wptr("D3.w"), A.pptr("D3.b")) == raw      # back after an exception too
    # finalize_variable_values: device copies of the averages into the parameters and their compute-dtype copy
    A._ema.add_(1.0); A._ema_shadow.add_(1.0)
    eng.ema_overwrite()
    import torch
    assert torch.equal(A._p, A._ema) and torch.equal(A._shadow, A._ema_shadow)
    eng._ema_forbidden = "driven by ShardedDataParallelStep"
    with pytest.raises(ValueError, match="ShardedDataParallelStep"):
        eng.enable_ema(0.5)
    eng._plans["recorded with the averages"] = None
    eng.disable_ema()
    assert eng.use_ema is False and A.ema is None and A.ema_shadow is None and eng._ema is None and eng._plans == {}
