"""The Trainer host math (gan_class_transfer2_amd.trainer_math): one copy, unchanged bits, no GPU needed."""
import itertools
import os
import types

import numpy as np
import pytest
import torch

import gan_class_transfer2_amd as g
from gan_class_transfer2_amd import trainer_math as TM
from gan_class_transfer2_amd.variants import VariantEngine
from oracle import denoiser_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_math.npz")
SWITCHES = list(itertools.product((False, True), repeat=4))     # order: TM.OBJECTIVE_SWITCHES
HYPER = {"default": dict(base_lr=2e-5, warm_up=2000), "const": dict(base_lr=1e-3, warm_up=0)}


def _key(bits) -> str:
    return "".join("01"[v] for v in bits)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("bits", SWITCHES, ids=_key)
def test_objective_coefficients_equal_the_recorded_ones_bit_for_bit(golden, bits):
    """(a, c, w) for t = 1..200 under every switch combination, against the vectors the engines' own copies of the formula
    produced before they were replaced by the shared function"""
    t_int = torch.from_numpy(golden["t_int"])
    assert t_int.tolist() == list(range(1, 201))
    got = torch.stack(TM.objective_coefficients(t_int, 200, *bits))
    assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(golden["acw_" + _key(bits)]))
    for v in TM.objective_coefficients(t_int, 200, *bits):
        assert v.is_contiguous() and v.shape == (200,)


@pytest.mark.parametrize("tag", sorted(HYPER))
def test_learning_rate_and_adam_step_size_equal_the_recorded_ones_bit_for_bit(golden, tag):
    ks = [int(k) for k in golden["k"]]
    assert ks == [0, 1, 5, 1999, 2000, 2001, 100000]
    for i, k in enumerate(ks):
        lr = TM.warmup_lr(k, **HYPER[tag])
        assert lr == float(golden["lr_" + tag][i]), (tag, k)
        assert TM.adam_step_size(lr, k, 0.9, 0.999) == float(golden["adam_alpha_" + tag][i]), (tag, k)


def test_alpha_dash_and_learning_rate_equal_the_oracle(golden):
    for t in list(range(0, 202)) + [100.0, 99.0, 25, 0.5]:          # (the sampler asks at steps / 2 and steps / 2 - 1 too)
        assert TM.alpha_dash(t, 200) == float(O.alpha_dash(t, 200)), t
    assert TM.alpha_dash(7, 50) == float(O.alpha_dash(7, 50))
    for hp in HYPER.values():
        for k in (int(k) for k in golden["k"]):
            assert TM.warmup_lr(k, **hp) == O.warmup_lr(k, hp["base_lr"], hp["warm_up"]), (hp, k)


@pytest.mark.parametrize("bits", SWITCHES, ids=_key)
def test_target_from_the_shared_coefficients_matches_the_float64_oracle(bits):
    """target = a x + c eps in float32 (what gct2_mix_per_image forms from the coefficient vectors) against
    oracle.denoiser_oracle.objective_terms in float64, t = 1..200, one 4 x 4 image per t (numpy default_rng(0)).
    Measured with the engines' formula before it moved here: max abs error 3.483e-07 over the sixteen combinations (targets up to
    |4.1|; the worst is predict_scaled_epsilon + prediction_weighting, 2.869e-07 for the ODE target, 0 where a, c are 0 / 1),
    and 4.544e-08 on the prediction weight.  Bound: twice the measured error - float32 rounding of the coefficient (three
    operations) and of the two products and the sum is all that separates the two."""
    sw = dict(zip(TM.OBJECTIVE_SWITCHES, bits))
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (200, 4, 4, 3)).astype(np.float32)
    eps = rng.standard_normal((200, 4, 4, 3)).astype(np.float32)
    t_int = torch.arange(1, 201, dtype=torch.int32)
    a, c, w = (v.numpy() for v in TM.objective_coefficients(t_int, 200, **sw))
    target = (a[:, None, None, None] * x + c[:, None, None, None] * eps).astype(np.float32)
    ref, w_ref = O.objective_terms(x.astype(np.float64), t_int.numpy(), eps.astype(np.float64), 200, **sw)
    err = float(np.max(np.abs(target.astype(np.float64) - ref)))
    w_err = float(np.max(np.abs(w.astype(np.float64) - w_ref.reshape(-1))))
    print(f"{_key(bits)}: target max abs err {err:.3e}, weight max abs err {w_err:.3e}")
    assert err <= 2 * 3.483e-07 and w_err <= 2 * 4.544e-08
    # the two questions the engines ask about the switches agree with the oracle's weight and target
    assert TM.objective_weighted(sw["predict_x"], sw["prediction_weighting"], sw["ordinary_differential_equation"]) == bool(np.any(w_ref != 1.0))
    assert TM.default_objective(sw["predict_x"], sw["ordinary_differential_equation"]) == (ref is not None and np.array_equal(ref, x))


def test_model_surface_returns_the_shared_values(monkeypatch):
    for base, warm in ((2e-5, 2000), (1e-3, 0), (3e-4, 10)):
        for k in (0, 1, 9, 10, 11, 1999, 2000, 100000):
            assert g.WarmUp(base, warm)(k) == TM.warmup_lr(k, base, warm)
    for steps in (200, 50):
        monkeypatch.setattr(g.model, "steps", steps)                 # alpha_dash(t) reads the module-level steps when called
        for t in (0, 1, 25, steps / 2, steps):
            assert g.alpha_dash(t) == TM.alpha_dash(t, steps)
        tt = torch.arange(1, steps + 1, dtype=torch.float32)
        assert torch.equal(g.alpha_dash(tt), TM.alpha_dash(tt, steps))
    assert g.sampler.alpha_dash is TM.alpha_dash


def test_both_engines_inherit_one_copy():
    """class attribute identity: neither engine overrides what the shared base owns"""
    for name in ("learning_rate", "adam_alpha", "objective_coefficients", "default_objective", "objective_weighted",
                 "enable_loss_scaling", "iterations", "loss_scale", "begin_step", "finish_step", "_check_finite", "f32_matrix",
                 "_new_ctx"):
        for cls in (g.UNetEngine, VariantEngine):
            assert issubclass(cls, TM.TrainerState)
            assert name not in vars(cls), (cls.__name__, name)
            assert getattr(cls, name) is getattr(TM.TrainerState, name)
    assert TM.LOSS_SCALE_GROWTH_INTERVAL == 2000


@pytest.mark.parametrize("cls", [g.UNetEngine, VariantEngine], ids=lambda c: c.__name__)
def test_engine_methods_return_the_shared_values_on_a_stub(cls):
    """the inherited methods on an object that has only the attributes they read (no device, no library)"""
    class Stub(cls):
        def __init__(self, **kw):
            self.__dict__.update(kw)

    for bits in SWITCHES:
        sw = dict(zip(TM.OBJECTIVE_SWITCHES, bits))
        eng = Stub(steps=200, ls_state=None, _iterations=0, **sw)
        t_int = torch.arange(1, 201, dtype=torch.int32)
        for got, want in zip(eng.objective_coefficients(t_int), TM.objective_coefficients(t_int, 200, **sw)):
            assert torch.equal(got, want)
        assert eng.default_objective() == TM.default_objective(sw["predict_x"], sw["ordinary_differential_equation"])
        assert eng.objective_weighted() == TM.objective_weighted(sw["predict_x"], sw["prediction_weighting"],
                                                                 sw["ordinary_differential_equation"])
    for hp in HYPER.values():
        eng = Stub(beta_1=0.9, beta_2=0.999, ls_state=None, _iterations=0, **hp)
        for k in (0, 1, 5, 1999, 2000, 2001):
            eng.iterations = k                                       # (the setter; without loss scaling the counter is the host's)
            assert eng.iterations == k
            assert eng.learning_rate() == eng.learning_rate(k) == TM.warmup_lr(k, **hp)
            assert eng.adam_alpha() == eng.adam_alpha(k) == TM.adam_step_size(TM.warmup_lr(k, **hp), k, 0.9, 0.999)
            eng.finish_step()
            assert eng.iterations == k + 1
        eng.base_lr, eng.warm_up, eng.beta_1 = 1e-4, 3, 0.8          # Trainer.compile() rewrites them on a live engine
        assert eng.adam_alpha(1) == TM.adam_step_size(TM.warmup_lr(1, 1e-4, 3), 1, 0.8, 0.999)
        assert eng.loss_scale() == (1.0, 0)


def test_glorot_limit_and_the_arena_draw_order():
    import math
    assert TM.glorot_limit((4, 4, 3, 128)) == math.sqrt(6.0 / (16 * 3 + 16 * 128))
    assert TM.glorot_limit((3, 3, 8, 16)) == math.sqrt(6.0 / (9 * 8 + 9 * 16))
    assert TM.glorot_limit((67, 3)) == math.sqrt(6.0 / (67 + 3))
    # UNetEngine's arena: sorted names, draws for kernels only - a seed gives the weights it gave before
    from gan_class_transfer2_amd.engine import ParamArena
    A = ParamArena(g.Topology(8, 16, 2), g.F32, torch.device("cpu"))
    A.glorot_init(5)
    gen = torch.Generator(device="cpu").manual_seed(5)
    for name in sorted(A.shapes):
        shp = A.shapes[name]
        if name.endswith(".b"):
            assert not A.param(name).any()
            continue
        rf = 1 if len(shp) == 2 else shp[0] * shp[1]
        lim = math.sqrt(6.0 / (rf * shp[-2] + rf * shp[-1]))
        assert torch.equal(A.param(name), (torch.rand(shp, generator=gen, dtype=torch.float32) * 2 - 1) * lim)


def test_optimizer_translation_serves_both_paths():
    hp = g.model.engine_hyper_parameters
    assert hp(g.Adam(g.WarmUp(2e-5, 2000))) == dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7, base_lr=2e-5, warm_up=2000)
    assert hp(g.LossScaleOptimizer(g.Adam(1e-3, 0.8, 0.99, 1e-8))) == dict(beta_1=0.8, beta_2=0.99, epsilon=1e-8, base_lr=1e-3, warm_up=0)
    assert "base_lr" not in hp(g.Adam(lambda k: 1e-3))
    # Trainer.compile() on a live engine: plain attribute writes, nothing else needed from the engine
    den = types.SimpleNamespace(engine=types.SimpleNamespace(ls_state=None, iterations=0))
    tr = g.Trainer(den)
    tr.compile(g.Adam(g.WarmUp(1e-4, 7), 0.8, 0.99, 1e-8), g.identity)
    e = den.engine
    assert (e.base_lr, e.warm_up, e.beta_1, e.beta_2, e.epsilon) == (1e-4, 7, 0.8, 0.99, 1e-8)
