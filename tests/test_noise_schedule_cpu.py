"""The noise schedules of train.py:85-93 (the six bodies of alpha_dash and the offset behind the live one), the parts that need no GPU:
the two C entry points, the host arithmetic of trainer_math (alpha_dash, noise_table, alpha_table), its refusals, and the module
globals that model.configure / model.alpha_dash follow."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import denoiser_oracle as O

F32, BF16, F16 = 0, 1, 2
NEW = ("gct2_noise_image_table", "gct2_noise_image_rng_table")


def tm():
    import gan_class_transfer2_amd as g
    return g.trainer_math


def test_symbols_signatures_and_abi():
    import gan_class_transfer2_amd as g
    L = g._lib
    raw = L.load()
    assert raw.gct2_abi_version() == 17                              # additions change no signature
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    assert L.SIGNATURES[NEW[0]] == [i, vp, vp, vp, vp, vp, i, vp, i, i, i, i, i, vp]
    assert L.SIGNATURES[NEW[1]] == [i, vp, vp, u64, u64, u64, vp, vp, vp, i, vp, i, i, i, i, i, vp]
    # the formula forms plus ONE pointer (coef), behind eps / eps_out
    assert len(L.SIGNATURES[NEW[0]]) == len(L.SIGNATURES["gct2_noise_image"]) + 1
    assert len(L.SIGNATURES[NEW[1]]) == len(L.SIGNATURES["gct2_noise_image_rng"]) + 1
    assert all(hasattr(raw, n) for n in NEW) and set(NEW) <= L.PLANNABLE
    assert all(n in open(L.__file__.replace("_lib.py", "csrc/plan.hip")).read() for n in NEW)       # a step plan can hold them
    assert g.NOISE_SCHEDULES == ("quadratic", "exp2", "rational", "exp16", "cosine", "quartic")


CLOSED_FORM_AT_0 = dict(quadratic=0.25, exp2=0.5, rational=254 / 766, exp16=1.0, cosine=1.0, quartic=1.0)


@pytest.mark.parametrize("name", list(CLOSED_FORM_AT_0))
def test_named_formula_at_zero_and_monotone(name):
    T = tm()
    steps = 200
    assert T.alpha_dash(0, steps, name) == pytest.approx(CLOSED_FORM_AT_0[name], rel=1e-15)
    assert T.alpha_dash(0.0, steps, name) == T.alpha_dash(0, steps, name)
    vals = [T.alpha_dash(float(t), steps, name) for t in range(steps + 1)]
    assert all(isinstance(v, float) for v in vals)                   # Python floats in, Python floats out (the sampler's use)
    assert all(a > b for a, b in zip(vals, vals[1:])), name          # strictly decreasing over t = 0 .. steps
    assert all(0.0 <= v <= 1.0 for v in vals)
    # the offset is added behind the formula (train.py:93's tail)
    assert T.alpha_dash(3.0, steps, name, 1e-4) == T.alpha_dash(3.0, steps, name) + 1e-4
    # float32 table of alpha: same values to float32 accuracy, t = 0 .. steps
    A = T.alpha_table(name, 0.0, steps)
    assert A.dtype == np.float32 and A.shape == (steps + 1,)
    assert np.abs(A.astype(np.float64) - np.array(vals)).max() <= 4e-6       # a few float32 roundings of values <= 1 (pow / cos included)


def test_formulas_against_their_text():
    """each body of train.py:88-93 written out again, with Python's right-associative ** spelled as nested powers"""
    T = tm()
    steps, t = 50, 7.0
    u = t / (steps + 1)
    assert T.alpha_dash(t, steps, "exp2") == 1 - 2 ** (u - 1)
    p = 2 ** (8 ** u)
    assert T.alpha_dash(t, steps, "rational") == (2 ** 8 - p) / (256 * p - p + 2 ** 8)
    assert T.alpha_dash(t, steps, "rational") == (2**8 - 2**8**u) / (256 * 2**8**u - 2**8**u + 2**8)
    assert T.alpha_dash(t, steps, "exp16") == (256 * 256) ** (-1 * u)
    assert T.alpha_dash(t, steps, "cosine") == math.cos(math.pi / 2 * u) ** 2
    assert T.alpha_dash(t, steps, "quartic") == (1 - u) ** 4
    assert T.alpha_dash(t, steps, "quadratic", 1e-4) == (1 - u) ** 2 * 0.25 + 1e-4
    assert T.alpha_dash(steps / 2 - 1, steps, lambda v: 0.5 - 0.25 * v) == 0.5 - 0.25 * ((steps / 2 - 1) / (steps + 1))


def test_two_argument_alpha_dash_is_unchanged():
    import gan_class_transfer2_amd as g
    T = tm()
    assert g.sampler.alpha_dash is T.alpha_dash
    for steps in (200, 50, 7):
        for t in (0, 1, 25, steps, steps / 2, steps / 2 - 1):
            want = (1 - t / (steps + 1)) ** 2 * 0.25
            assert T.alpha_dash(t, steps) == want == float(O.alpha_dash(t, steps))
            assert T.alpha_dash(t, steps, "quadratic", 0.0) == want and T.alpha_dash(t, steps, None) == want
    tt = torch.arange(1, 201, dtype=torch.float32)
    assert torch.equal(T.alpha_dash(tt, 200), (1 - tt / 201) ** 2 * 0.25)


def _coefs_from_the_stated_chain(dtype, steps):
    """(sa, sb) per timestep out of the op chains that tests/pointwise_cases.py states for gct2_noise_image (O.noise_image_f32 /
    O.noise_image_f16): x = 1, eps = 0 leaves fl(1 * sa + 0 * sb) = sa, and x = 0, eps = 1 leaves sb"""
    t = np.arange(1, steps + 1, dtype=np.int32)
    one, zero = np.ones((steps, 1, 1, 1), np.float32), np.zeros((steps, 1, 1, 1), np.float32)
    f = O.noise_image_f16 if dtype == F16 else O.noise_image_f32
    return (np.asarray(f(one, t, zero, steps)).reshape(steps).astype(np.float32),
            np.asarray(f(zero, t, one, steps)).reshape(steps).astype(np.float32))


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("steps", [200, 7])
def test_quadratic_table_equals_the_stated_chains(dtype, steps):
    T = tm()
    tab = T.noise_table("quadratic", 0, steps, dtype)
    assert tab.dtype == np.float32 and tab.shape == (steps, 2) and tab.flags["C_CONTIGUOUS"]
    sa, sb = _coefs_from_the_stated_chain(dtype, steps)
    assert np.array_equal(tab[:, 0].view(np.uint32), sa.view(np.uint32))
    assert np.array_equal(tab[:, 1].view(np.uint32), sb.view(np.uint32))
    if dtype == F16:                                                  # fp16-representable: the kernel's conversion is exact
        assert np.array_equal(tab, tab.astype(np.float16).astype(np.float32))


def test_bf16_table_is_the_f32_table_and_a_callable_equals_the_name():
    T = tm()
    for name, offset in (("quadratic", 1e-4), ("cosine", 0.0), ("exp2", 1e-4)):
        assert np.array_equal(T.noise_table(name, offset, 200, BF16), T.noise_table(name, offset, 200, F32))
    body = lambda t: (1 - t) ** 2 * 0.25
    for dtype in (F32, BF16, F16):
        for steps in (200, 7):
            assert np.array_equal(T.noise_table(body, 0.0, steps, dtype), T.noise_table("quadratic", 0.0, steps, dtype))
    assert np.array_equal(T.alpha_table(body, 0.0, 200), T.alpha_table("quadratic", 0.0, 200))
    # a callable is called ONCE, on the whole array of D values, and its result is cast to D
    seen = []
    T.noise_table(lambda t: seen.append((t.dtype, t.shape)) or np.full(t.shape, 0.5, np.float64), 0.0, 9, F16)
    assert seen == [(np.dtype(np.float16), (9,))]
    # sb is formed from a, not from sa: (sqrt(a), sqrt(1 - a)) in D
    tab = T.noise_table("cosine", 0.0, 200, F32)
    a = np.cos(np.float32(math.pi / 2) * (np.arange(1, 201).astype(np.float32) / np.float32(201))) ** 2
    assert a.dtype == np.float32 and np.array_equal(tab[:, 0], np.sqrt(a)) and np.array_equal(tab[:, 1], np.sqrt(np.float32(1) - a))


def test_every_name_at_200_steps_in_both_arithmetics():
    T = tm()
    for name in T.NOISE_SCHEDULES:
        a32 = T.alpha_table(name, 0.0, 200)[1:]
        assert ((a32 > 0) & (a32 < 1)).all(), name
        tab = T.noise_table(name, 0.0, 200, F32)
        assert np.isfinite(tab).all() and ((tab > 0) & (tab <= 1)).all(), name     # sa > 0 is a > 0, sb > 0 is a < 1 (a root may round to 1)
    with pytest.raises(ValueError, match="exp16.*float16"):           # 256*256 overflows float16: refused for F16 by name
        T.noise_table("exp16", 0.0, 200, F16)
    q = T.noise_table("quartic", 0.0, 200, F16)                       # merely underflows to a = 0 at the last two timesteps: legal
    assert np.array_equal(q[-2:], np.array([[0.0, 1.0], [0.0, 1.0]], np.float32)) and (q[:-2, 0] > 0).all()
    for name in ("quadratic", "exp2", "rational"):
        tab = T.noise_table(name, 0.0, 200, F16)
        assert ((tab > 0) & (tab <= 1)).all(), name                   # a inside (0, 1) in float16: sa > 0 and sb > 0
    # "cosine" in float16: cos(pi/2 * t) = 1 - 3.0e-5 at t = 1/201 and 1 - 1.2e-4 at 2/201, and float16's spacing below 1 is 4.9e-4:
    # both round to 1, so a = 1 (sb = 0: no noise) at the first two timesteps whatever the order of the operations.  Inside [0, 1],
    # hence legal like quartic's a = 0; everywhere else strictly inside
    c = T.noise_table("cosine", 0.0, 200, F16)
    assert np.array_equal(c[:2], np.array([[1.0, 0.0], [1.0, 0.0]], np.float32)) and ((c[2:] > 0) & (c[2:] <= 1)).all()


def test_refusals():
    T = tm()
    with pytest.raises(ValueError, match="unknown noise_schedule 'linear'"):
        T.noise_table("linear", 0.0, 200, F32)
    with pytest.raises(ValueError, match="unknown noise_schedule"):
        T.check_noise_schedule("Quadratic")
    with pytest.raises(ValueError, match="callable"):
        T.check_noise_schedule(3)
    for bad in (float("nan"), float("inf"), -float("inf"), "x", None):
        with pytest.raises(ValueError, match="alpha_dash_offset"):
            T.check_noise_schedule("quadratic", bad)
    with pytest.raises(ValueError, match=r"not a finite value in \[0, 1\]"):
        T.noise_table("exp16", 0.5, 200, F32)                         # alpha(1) + 0.5 > 1
    with pytest.raises(ValueError, match=r"not a finite value in \[0, 1\]"):
        T.noise_table("quadratic", -0.01, 200, F32)                   # alpha(200) - 0.01 < 0
    with pytest.raises(ValueError, match=r"not a finite value in \[0, 1\]"):
        T.noise_table(lambda t: t * float("nan"), 0.0, 200, F32)
    with pytest.raises(ValueError, match=r"not a finite value in \[0, 1\]"):
        T.alpha_table(lambda t: 1.5 - t, 0.0, 200)
    with pytest.raises(ValueError, match="cannot be evaluated in float16"):
        T.noise_table(lambda t: (t * t.dtype.type(60000.0)) * t.dtype.type(4.0) * t.dtype.type(0.0), 0.0, 200, F16)   # overflows on the way
    with pytest.raises(ValueError, match="exp16"):
        T.noise_table("exp16", 0.0, 200, F16)
    with pytest.raises(ValueError, match="shape"):
        T.noise_table(lambda t: 0.5, 0.0, 200, F32)


def test_objective_coefficients_gather_from_the_alpha_table():
    """CPU tensors: (a, c, w) under a non-default schedule are numpy's float32 roots of alpha_table at t (t - 1 in ODE mode); the
    default call is what it was"""
    T = tm()
    steps = 7
    t_int = torch.tensor([1, 7, 3, 4], dtype=torch.int32)
    A = T.alpha_table("exp2", 0.0, steps)
    f = np.float32
    a, c, w = T.objective_coefficients(t_int, steps, False, False, True, False, schedule="exp2")
    s = np.sqrt(f(1) - A[t_int.numpy()])
    assert np.array_equal(a.numpy(), np.zeros(4, f)) and np.array_equal(c.numpy(), s) and np.array_equal(w.numpy(), s)
    a, c, w = T.objective_coefficients(t_int, steps, False, True, True, False, schedule="exp2")      # predict_scaled_epsilon: c = s * s
    assert np.array_equal(a.numpy(), np.zeros(4, f)) and np.array_equal(c.numpy(), s * s) and np.array_equal(w.numpy(), s)
    a, c, w = T.objective_coefficients(t_int, steps, True, False, False, True, schedule="exp2")
    a1 = A[t_int.numpy() - 1]
    assert np.array_equal(a.numpy(), np.sqrt(a1)) and np.array_equal(c.numpy(), np.sqrt(f(1) - a1)) and np.array_equal(w.numpy(), np.ones(4, f))
    tt = t_int.to(torch.float32)
    a, c, w = T.objective_coefficients(t_int, steps, False, True, False, False)
    s = (1 - (1 - tt / (steps + 1)) ** 2 * 0.25).sqrt()
    assert torch.equal(c, s) and torch.equal(a, torch.zeros(4)) and torch.equal(w, torch.ones(4))


def test_checkpoint_marker():
    T = tm()
    T.check_schedule_marker({}, "quadratic", 0.0)
    m = T.schedule_marker("cosine", 1e-4)
    assert m.dtype == torch.float64 and m.tolist() == [4.0, 1e-4]
    T.check_schedule_marker({"noise_schedule": m}, "cosine", 1e-4)
    for sched, off in (("quadratic", 0.0), ("cosine", 0.0), ("exp2", 1e-4)):
        with pytest.raises(ValueError, match="nothing is loaded"):
            T.check_schedule_marker({"noise_schedule": m}, sched, off)
    with pytest.raises(ValueError, match="nothing is loaded"):
        T.check_schedule_marker({}, "cosine", 0.0)
    body = lambda t: t
    assert T.schedule_marker(body, 0.0).tolist() == [-1.0, 0.0]       # a callable is stored as "custom" and compares with nothing
    T.check_schedule_marker({"noise_schedule": T.schedule_marker(body, 0.0)}, "cosine", 0.0)
    T.check_schedule_marker({"noise_schedule": m}, body, 0.0)


def test_configure_and_model_alpha_dash_follow_the_setting(monkeypatch):
    import gan_class_transfer2_amd as g
    M, T = g.model, tm()
    assert (M.noise_schedule, M.alpha_dash_offset) == ("quadratic", 0.0)
    for k in ("noise_schedule", "alpha_dash_offset", "steps"):
        monkeypatch.setattr(M, k, getattr(M, k))                      # (restored after the test)
    g.configure(steps=50)
    assert g.alpha_dash(7) == T.alpha_dash(7, 50) == (1 - 7 / 51) ** 2 * 0.25
    g.configure(noise_schedule="cosine", alpha_dash_offset=1e-4)
    assert (M.noise_schedule, M.alpha_dash_offset) == ("cosine", 1e-4)
    assert g.alpha_dash(7) == math.cos(math.pi / 2 * (7 / 51)) ** 2 + 1e-4
    tt = torch.tensor([1.0, 7.0])
    assert torch.equal(g.alpha_dash(tt), torch.cos(math.pi / 2 * (tt / 51)) ** 2 + 1e-4)
    body = lambda t: 0.5 - 0.25 * t
    g.configure(noise_schedule=body, alpha_dash_offset=0)
    assert M.noise_schedule is body and M.alpha_dash_offset == 0.0 and g.alpha_dash(7) == 0.5 - 0.25 * (7 / 51)
    for bad in (dict(noise_schedule="linear"), dict(noise_schedule=5), dict(alpha_dash_offset=float("nan")), dict(alpha_dash_offset="much")):
        with pytest.raises(ValueError):
            g.configure(**bad)
    assert M.noise_schedule is body and M.alpha_dash_offset == 0.0    # a refused value changes nothing
    g.configure(noise_schedule="quadratic")
    assert g.alpha_dash(7) == T.alpha_dash(7, 50)


def test_plan_key_names_the_schedule():
    import inspect
    import gan_class_transfer2_amd as g
    from unittest import mock
    src = inspect.getsource(g.UNetEngine._plan_key)
    assert "self.noise_schedule" in src and "self.alpha_dash_offset" in src
    eng = mock.MagicMock()
    eng.noise_schedule, eng.alpha_dash_offset = "quadratic", 0.0
    key = lambda: g.UNetEngine._plan_key(eng, "buffers", True, False, eng.stream)
    off = key()
    eng.noise_schedule = "cosine"
    cos = key()
    eng.alpha_dash_offset = 1e-4
    assert len({off, cos, key()}) == 3
    body = lambda t: t
    eng.noise_schedule, eng.alpha_dash_offset = body, 0.0
    custom = key()
    eng.noise_schedule = lambda t: t
    assert key() != custom                                            # another callable: another plan
    eng.noise_schedule = "quadratic"
    assert key() == off


def test_trainer_state_setting():
    """set_noise_schedule on a TrainerState without a device: class-level defaults (a default engine carries nothing new), deferred
    work flushed, host tables formed once per (schedule, offset, steps, dtype) and validated before anything changes, the device
    copies made on first use, and objective_coefficients reading them"""
    T = tm()

    class Stub(T.TrainerState):
        def __init__(self, dtype):
            self.dtype, self.steps, self.device, self.flushed = dtype, 7, torch.device("cpu"), 0
            self.predict_x, self.predict_scaled_epsilon, self.prediction_weighting, self.ordinary_differential_equation = False, False, True, False

        def flush_deferred(self):
            self.flushed += 1

    e = Stub(F32)
    assert (e.noise_schedule, e.alpha_dash_offset, e._noise_tables) == ("quadratic", 0.0, None) and e._default_schedule()
    assert not {"noise_schedule", "alpha_dash_offset", "_noise_tables"} & set(vars(e))
    e.set_noise_schedule("quadratic", 0.0)
    assert e.flushed == 1 and e._noise_tables is None and e._default_schedule()          # the default builds no table
    t_int = torch.tensor([1, 7, 3], dtype=torch.int32)
    tt = t_int.to(torch.float32)
    a, c, w = e.objective_coefficients(t_int)
    assert torch.equal(w, (1 - (1 - tt / 8) ** 2 * 0.25).sqrt())                         # the default keeps its torch formula
    e.set_noise_schedule("exp2", 1e-4)
    assert e.flushed == 2 and (e.noise_schedule, e.alpha_dash_offset) == ("exp2", 1e-4) and not e._default_schedule()
    (entry,) = e._noise_tables.values()
    assert "device" not in entry and np.array_equal(entry["host"][0], T.noise_table("exp2", 1e-4, 7, F32))
    coef, sqa, sqb = e._schedule_tables()
    assert e._schedule_tables()[0] is coef and e._noise_coef_ptr() == coef.data_ptr() and coef.data_ptr() % 8 == 0
    A = T.alpha_table("exp2", 1e-4, 7)
    assert np.array_equal(coef.numpy(), T.noise_table("exp2", 1e-4, 7, F32)) and np.array_equal(sqa.numpy(), np.sqrt(A))
    a, c, w = e.objective_coefficients(t_int)
    assert np.array_equal(w.numpy(), np.sqrt(np.float32(1) - A[t_int.numpy()])) and np.array_equal(c.numpy(), w.numpy())
    for bad, why in ((("linear", 0.0), "unknown noise_schedule"), (("exp2", float("inf")), "alpha_dash_offset"), (("cosine", 1e-4), r"\[0, 1\]")):
        with pytest.raises(ValueError, match=why):
            e.set_noise_schedule(*bad)
    assert e.flushed == 2 and (e.noise_schedule, e.alpha_dash_offset) == ("exp2", 1e-4)   # refused before anything was flushed or written
    h = Stub(F16)
    with pytest.raises(ValueError, match="exp16.*float16"):
        h.set_noise_schedule("exp16")
    h.set_noise_schedule("quartic")
    body = lambda t: (1 - t) ** 2 * 0.25
    e.set_noise_schedule(body)
    e.set_noise_schedule("exp2", 1e-4)
    e.set_noise_schedule(body)
    assert len(e._noise_tables) == 2 and e._schedule_tables()[0].data_ptr() != coef.data_ptr()      # kept for the engine's lifetime
    e.set_noise_schedule("exp2", 1e-4)
    assert e._schedule_tables()[0] is coef                                                # (a step plan holds this address)
