"""The v objective and the per-timestep loss weights without a GPU: the new symbols in the header, the binding, the plan table and the
built library; trainer_math.loss_weight_table against the closed forms of min-SNR-gamma; what is refused before anything launches;
the v identities on the host restatements of tests/objective_cases.py; and the restated gradient against central finite differences."""
import inspect
import os
import re

import numpy as np
import pytest

import objective_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gct2_objective_loss_fwd_bwd", "gct2_objective_loss_scratch")


def pkg():
    import gan_class_transfer2_amd as g
    return g


def tm():
    return pkg().trainer_math


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_everywhere():
    g = pkg()
    L = g._lib
    raw = L.load()
    assert L.ABI_VERSION == 17 and raw.gct2_abi_version() == 17       # additions change no signature
    assert L.SAMPLE_V == 5 == OC.SAMPLE_V and (L.SAMPLE_X, L.SAMPLE_EPS, L.SAMPLE_SCALED_EPS, L.SAMPLE_ODE) == (0, 1, 2, 3)
    header = open(os.path.join(ROOT, "include", "gct2.h")).read()
    plan = open(os.path.join(ROOT, "gan-class-transfer2_amd", "csrc", "plan.hip")).read()
    assert "GCT2_SAMPLE_V = 5" in header and "reserved and refused" in header
    for name in NEW:
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto and hasattr(raw, name)
        assert len(proto.group(1).split(",")) == len(L.SIGNATURES[name]) <= 28                 # plan.hip MAX_ARGS
    assert len(L.SIGNATURES[NEW[0]]) == 18 and L.SIGNATURES[NEW[0]][-1] is L._vp and L.SIGNATURES[NEW[0]][11] is L._sz
    assert NEW[0] in L.PLANNABLE and f"GCT2_ENTRY({NEW[0]})" in plan and NEW[1] not in L.PLANNABLE
    assert g.loss_weight_table is g.trainer_math.loss_weight_table


def test_a_plan_records_the_call():
    L = pkg()._lib
    plan = L.Plan()
    plan.begin(execute=False)
    try:
        L.call(NEW[0], 0, 64, 64, 64, 64, 64, None, 64, 64, 64, 64, 1024, 2, 4, 4, 3, None, None)
    finally:
        plan.end()
    assert plan.n == 1


def test_the_host_entry_points_refuse_without_a_gpu():
    """gct2_objective_loss_scratch is host only: kinds other than MSE / L1, bad dims, B > 65535, n >= 2^31"""
    import ctypes
    raw = pkg()._lib.load()
    need = ctypes.c_size_t(0)
    assert raw.gct2_objective_loss_scratch(0, 2, 40, 40, 3, ctypes.byref(need)) == 0
    assert need.value >= 2 * 2 * 2 and need.value % 4 == 0              # two work-groups per image, one fp64 partial sum each
    for bad in ((2, 2, 16, 16, 3), (3, 2, 16, 16, 3), (-1, 2, 16, 16, 3), (0, 0, 16, 16, 3), (0, 2, 16, 16, 5), (0, 2, 16, 16, 0),
                (1, 65536, 1, 1, 1), (0, 2, 32768, 32768, 1)):
        assert raw.gct2_objective_loss_scratch(*bad, ctypes.byref(need)) != 0, bad
    assert raw.gct2_objective_loss_scratch(0, 2, 16, 16, 3, None) != 0


# ---- the weight table --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule,gamma", [("quadratic", 0.1), ("cosine", 5.0)])
@pytest.mark.parametrize("objective", ["x", "eps", "v"])
def test_min_snr_table_equals_the_closed_forms(schedule, gamma, objective):
    M = tm()
    steps = 200
    table = M.loss_weight_table("min_snr", gamma, steps, objective, schedule, 0.0)
    assert table.dtype == np.float32 and table.shape == (steps + 1,) and table[0] == 0
    alpha = M.alpha_table(schedule, 0.0, steps).astype(np.float64)[1:]
    want, snr = OC.min_snr_weights(alpha, gamma, objective)
    assert (snr < gamma).any() and (snr > gamma).any()               # the clip is live on both sides of gamma
    assert np.array_equal(table[1:], want.astype(np.float32))
    # the x0-space weight is min(SNR, gamma) under every objective: eps carries 1 / SNR of it, v carries 1 / (SNR + 1)
    back = {"x": 1.0, "eps": snr, "v": snr + 1.0}[objective]
    ok = snr > 0
    assert np.allclose((want * back)[ok], np.minimum(snr, gamma)[ok], rtol=1e-12)


def test_default_schedule_never_reaches_gamma_5():
    """why the quadratic case runs at gamma = 0.1: alpha <= 0.25 there, SNR <= 1 / 3"""
    M = tm()
    alpha = M.alpha_table("quadratic", 0.0, 200).astype(np.float64)[1:]
    assert (alpha / (1 - alpha)).max() < 0.34
    assert np.array_equal(M.loss_weight_table("min_snr", 5.0, 200, "eps"), np.r_[0.0, np.ones(200)].astype(np.float32))


def test_callables_and_tables():
    M = tm()
    steps = 7
    seen = []
    table = M.loss_weight_table(lambda snr, t: seen.append((snr, t)) or 1.0 / t, 5.0, steps, None)
    assert [t for _, t in seen] == list(range(1, steps + 1)) and all(isinstance(s, float) for s, _ in seen)
    assert np.array_equal(table, np.float32([0.0] + [1.0 / t for t in range(1, steps + 1)]))
    seq = [0.5, 0.0, 2.0, 3.0, 1e-3, 7.0, 1.0]
    for given in (seq, tuple(seq), np.float64(seq)):
        assert np.array_equal(M.loss_weight_table(given, 5.0, steps, None), np.float32([0.0] + seq))
    assert np.array_equal(M.loss_weight_table(seq, 5.0, steps, "x", "cosine", 0.0), np.float32([0.0] + seq))   # under any objective


def test_bad_tables_and_callables_are_value_errors():
    M = tm()
    steps = 5
    good = [1.0] * steps
    for bad in ([1.0] * 4, [1.0] * 6, [], good[:-1] + [-1.0], good[:-1] + [float("nan")], good[:-1] + [float("inf")], good[:-1] + [1e39],
                lambda snr, t: -0.5, lambda snr, t: float("nan"), lambda snr, t: "x", lambda snr, t: None, "snr", "min-snr", 3, object()):
        with pytest.raises(ValueError):
            M.loss_weight_table(bad, 5.0, steps, "x")
    for gamma in (0.0, -1.0, float("nan"), float("inf"), "big", None):
        with pytest.raises(ValueError):
            M.loss_weight_table("min_snr", gamma, steps, "x")
    for objective in (None, "scaled_eps", "ode"):
        with pytest.raises(ValueError):
            M.loss_weight_table("min_snr", 5.0, steps, objective)
    with pytest.raises(ValueError):
        M.loss_weight_table(None, 5.0, steps, "x")
    with pytest.raises(ValueError):
        M.loss_weight_table("min_snr", 5.0, 0, "x")


# ---- the switches --------------------------------------------------------------------------------------------------------------------------------

def test_objective_switches_keep_their_four_names():
    g = pkg()
    four = ("predict_x", "predict_scaled_epsilon", "prediction_weighting", "ordinary_differential_equation")
    assert g.trainer_math.OBJECTIVE_SWITCHES == four and tuple(g.model.objective_switches()) == four
    assert g.model.predict_v is False and g.model.loss_weighting is None and g.model.min_snr_gamma == 5.0
    for fn in (g.generate, g.encode, g.log_sample):
        assert inspect.signature(fn).parameters["predict_v"].default is None
    for cls in (g.UNetEngine, g.engine.TrainerState, __import__("gan_class_transfer2_amd.variants", fromlist=["x"]).VariantEngine):
        assert inspect.signature(cls.__init__).parameters["predict_v"].default is False


def test_modes_and_tables_of_the_v_objective():
    g = pkg()
    M, L = g.trainer_math, g._lib
    for fn in (M.x0_mode, g.sampler.sample_mode):
        assert fn(True, False, False) == L.SAMPLE_X and fn(False, False, False) == L.SAMPLE_EPS       # the existing decisions
        assert fn(False, True, False) == L.SAMPLE_SCALED_EPS and fn(True, True, True) == L.SAMPLE_ODE
        for px in (True, False):
            assert fn(px, False, False, predict_v=True) == L.SAMPLE_V                                # predict_x is ignored
        for clash in ((True, True, False), (True, False, True)):
            with pytest.raises(ValueError, match="predict_v"):
                fn(*clash, predict_v=True)
    for schedule, offset in (("quadratic", 0.0), ("cosine", 0.0), ("quadratic", 1e-4)):
        u, v = M.x0_tables(200, L.SAMPLE_V, schedule, offset)
        assert u.dtype == v.dtype == np.float32 and u[0] == 0 and v[0] == 0
        a = [float(M.alpha_dash(float(t), 200, schedule, offset)) for t in range(1, 201)]
        assert np.array_equal(u[1:], np.float32([x ** 0.5 for x in a]))
        assert np.array_equal(v[1:], np.float32([-((1 - x) ** 0.5) for x in a]))


def test_refused_switch_combinations():
    g = pkg()
    M = g.trainer_math
    for kw in (dict(predict_scaled_epsilon=True), dict(prediction_weighting=True), dict(ordinary_differential_equation=True)):
        with pytest.raises(ValueError, match="predict_v"):
            M.check_predict_v(True, **kw)
        assert M.check_predict_v(False, **kw) is False
        with pytest.raises(ValueError, match="predict_v"):
            M.weighting_objective(predict_v=True, **kw)
    assert M.check_predict_v(True) is True
    assert M.weighting_objective() == "x" and M.weighting_objective(predict_x=False) == "eps"
    assert M.weighting_objective(predict_x=False, predict_v=True) == "v" == M.weighting_objective(predict_v=True)
    for kw in (dict(predict_x=False, predict_scaled_epsilon=True), dict(predict_x=False, prediction_weighting=True),
               dict(ordinary_differential_equation=True)):
        assert M.weighting_objective(**kw) is None
    # an engine's own settings, on a bare TrainerState (no device): validated on the host before anything changes
    eng = M.TrainerState.__new__(M.TrainerState)
    eng.steps, eng.predict_x, eng.predict_scaled_epsilon, eng.prediction_weighting, eng.ordinary_differential_equation = 50, False, False, False, False
    eng.set_loss_weighting("min_snr", 0.1)
    assert (eng.loss_weighting, eng.min_snr_gamma) == ("min_snr", 0.1)
    eng.check_step_settings()
    for name, value in (("predict_scaled_epsilon", True), ("prediction_weighting", True), ("ordinary_differential_equation", True)):
        setattr(eng, name, value)
        with pytest.raises(ValueError, match="loss_weighting"):
            eng.check_step_settings()
        with pytest.raises(ValueError, match="loss_weighting"):
            eng.set_loss_weighting("min_snr", 5.0)
        eng.set_loss_weighting([1.0] * 50)                               # a table is accepted under any objective
        eng.set_loss_weighting(lambda snr, t: 1.0)
        eng.loss_weighting = "min_snr"
        setattr(eng, name, False)
    eng.predict_v = True
    eng.ordinary_differential_equation = True
    with pytest.raises(ValueError, match="predict_v"):
        eng.check_step_settings()
    eng.ordinary_differential_equation = False
    for loss in ("dct", "mse_pooled"):
        eng.training_loss = loss
        with pytest.raises(ValueError, match="training_loss"):
            eng.check_step_settings()
        with pytest.raises(ValueError, match="training_loss"):
            eng.set_loss_weighting("min_snr", 5.0)
    eng.training_loss = "l1"
    eng.check_step_settings()
    before = (eng.loss_weighting, eng.min_snr_gamma)
    for bad in ("nope", [1.0] * 49, [-1.0] * 50):
        with pytest.raises(ValueError):
            eng.set_loss_weighting(bad)
    with pytest.raises(ValueError):
        eng.set_loss_weighting("min_snr", -2.0)
    assert (eng.loss_weighting, eng.min_snr_gamma) == before             # a refused setting changes nothing
    eng.set_loss_weighting(None)
    assert eng.loss_weighting is None
    # configure(): the globals are checked where they are set
    with pytest.raises(ValueError):
        g.model.configure(loss_weighting="nope")
    with pytest.raises(ValueError):
        g.model.configure(min_snr_gamma=0.0)
    assert g.model.loss_weighting is None and g.model.min_snr_gamma == 5.0


def test_data_parallel_wrappers_refuse_loss_weighting_on_the_host():
    import types
    D = __import__("gan_class_transfer2_amd.distributed", fromlist=["x"])
    eng = types.SimpleNamespace(loss_weighting="min_snr")
    for who in ("DataParallelStep", "ShardedDataParallelStep"):
        with pytest.raises(ValueError, match="loss_weighting"):
            D._refuse_loss_weighting(eng, who)
    eng = types.SimpleNamespace(loss_weighting=None)
    D._refuse_loss_weighting(eng, "DataParallelStep")
    assert "loss_weighting" in eng._weighting_forbidden
    src = inspect.getsource(D)
    assert src.count('_refuse_loss_weighting(engine, "DataParallelStep")') == 1
    assert src.count('_refuse_loss_weighting(engine, "ShardedDataParallelStep")') == 1


# ---- the v identities ------------------------------------------------------------------------------------------------------------------------------

def test_v_identities_with_the_exact_target_as_the_prediction():
    """with pred = the target itself, u noised + v pred recovers x and v_update recovers (x, eps), within 1e-6 relative: float32
    chains of three operations at magnitudes <= 4 (sa^2 + sb^2 = 1 up to the rounding of the two roots).  The noised image and the
    target are formed the way the train step forms them, from the float32 roots of objective_coefficients; u, v and v_update's roots
    come from Python floats.  On the default schedule (alpha <= 0.25) the two agree within 2e-7 absolute.  Under "cosine" they do not
    at small t - float32 forms 1 - alpha with alpha = 0.99994 and loses twelve bits, sqrt(1 - alpha) is 0.0078125 against 0.0078148 -
    which is a property of the schedule tables, not of the objective: the figure is printed, the identity is asserted where the roots
    agree"""
    g = pkg()
    M, L = g.trainer_math, g._lib
    import torch
    steps = 200
    rng = np.random.default_rng(5)
    scale = 4.0
    for schedule in ("quadratic", "cosine"):
        u, v = M.x0_tables(steps, L.SAMPLE_V, schedule, 0.0)
        for t in (1, 37, 100, 199, 200):
            x = np.clip(rng.standard_normal((4, 8, 8, 3)), -1, 1).astype(np.float32)
            eps = np.clip(rng.standard_normal(x.shape), -4, 4).astype(np.float32)
            a_t = float(M.alpha_dash(float(t), steps, schedule, 0.0))
            ti = torch.full((4,), t, dtype=torch.int32)
            a, c, w = M.objective_coefficients(ti, steps, schedule=schedule, predict_v=True)
            assert (w.numpy() == 1).all() and a.dtype == c.dtype == torch.float32
            a, c = a.numpy().reshape(4, 1, 1, 1), c.numpy().reshape(4, 1, 1, 1)
            sa, sb = c, -a                                              # (a, c, w) = (-sb, sa, 1)
            noised = sa * x + sb * eps
            target = a * x + c * eps                                    # gct2_mix_per_image's rule
            assert target.dtype == noised.dtype == np.float32
            x0 = u[t] * noised + v[t] * target
            xr, er = OC.v_update(target, noised, a_t)
            errs = [float(np.abs(d).max()) for d in (x0 - x, xr - x, er - eps)]
            print(f"{schedule} t {t}: |x0 - x| {errs[0]:.3g}, v_update |x - x| {errs[1]:.3g}, |e - eps| {errs[2]:.3g}")
            if schedule == "quadratic":
                assert np.allclose(sa, OC.roots(a_t)[0], rtol=0, atol=2e-7) and np.allclose(sb, OC.roots(a_t)[1], rtol=0, atol=2e-7)
                assert max(errs) <= 1e-6 * scale, (schedule, t, errs)
    xr, er = OC.v_update(np.float32([1.5, -2.0]), np.float32([0.25, 3.0]), 0.0)                      # a_t = 0: sa = 0, sb = 1
    assert np.array_equal(xr, np.float32([-1.5, 2.0])) and np.array_equal(er, np.float32([0.25, 3.0]))


# ---- the gradient ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", OC.KINDS, ids=OC.KIND_IDS)
def test_dpred_is_the_gradient_of_the_loss(kind):
    """central finite differences in float64 on the smooth restatement, with w and lam: dpred / s of objective_loss_reference agrees
    within the float32 rounding of its products (1e-6 relative) plus what the float32 rounding of d itself (three operations at
    magnitudes <= 8: 1e-6 absolute) does to the gradient 2 lam w d / n, plus the differences' own error"""
    shape = (3, 5, 7, 3)
    v = OC.loss_inputs(shape, seed=3)
    _, dpred, loss = OC.objective_loss_reference(kind, v["pred"], v["x"], v["eps"], v["a"], v["c"], v["w"], v["lam"], s=1024.0)
    f = lambda p: OC.objective_loss_f64(kind, p, v["x"], v["eps"], v["a"], v["c"], v["w"], v["lam"])
    assert abs(f(v["pred"]) - loss) <= 1e-6 * abs(loss)
    rng = np.random.default_rng(9)
    h = 1e-4
    for _ in range(24):
        i = tuple(int(rng.integers(0, s)) for s in shape)
        up, dn = v["pred"].astype(np.float64), v["pred"].astype(np.float64)
        up[i] += h
        dn[i] -= h
        fd = (f(up) - f(dn)) / (2 * h)
        got = float(dpred[i]) / 1024.0
        slope = 2.0 * abs(float(v["lam"][i[0]]) * float(v["w"][i[0]])) / dpred.size
        assert abs(got - fd) <= 1e-6 * abs(fd) + 1e-6 * slope + 1e-12, (i, got, fd)
    # without weights the product with g_b is absent, with one of them it is that vector
    _, plain, _ = OC.objective_loss_reference(kind, v["pred"], v["x"])
    _, only_lam, _ = OC.objective_loss_reference(kind, v["pred"], v["x"], lam=v["lam"])
    assert np.array_equal(only_lam, plain * v["lam"].reshape(3, 1, 1, 1))
