"""The v objective and the per-timestep loss weights on the tiny network of tests/test_generate_step_gpu.py (size 16, pixel_size 8,
max_size 16, 2 octaves, steps = 6, fp32): the train step's loss against torch, the weighted step against the unweighted non-fused one,
exact doubling under a table of twos, min-SNR against the rows of evaluation, generate / encode in mode V against a hand loop, the
PSNR of evaluation, what is refused, and that nothing else moves."""
import numpy as np
import pytest
import torch

from test_generate_step_gpu import F32, SIZE, STEPS, _state, den, hand_loop, lib, noise, same_bits, stream, tiny

pytestmark = pytest.mark.gpu
B = 4
T_INT = [1, 2, 5, 6]                                            # SNR(t) = 0.225, 0.146, 0.021, 0.0051: both sides of gamma = 0.1


def batch(gpu, n=B, seed=4):
    return torch.tensor(np.floor(np.random.default_rng(seed).uniform(0, 256, (n, SIZE, SIZE, 3))) / 128 - 1, dtype=torch.float32, device=gpu)


def injected(gpu, n=B):
    return torch.tensor(T_INT[:n], dtype=torch.int32, device=gpu), noise(gpu, n, seed=77)


def roots(t_int):
    """the float32 roots of the default schedule's torch formula (trainer_math.alpha_dash on a float32 tensor)"""
    a = (1 - t_int.to(torch.float32) / (STEPS + 1)) ** 2 * 0.25
    return a.sqrt().reshape(-1, 1, 1, 1), (1 - a).sqrt().reshape(-1, 1, 1, 1)


def fixed_order(gpu, head="hidden_dense", **kw):
    """the same tiny topology on an engine whose reverse pass adds in a fixed order: fp32 on the matrix cores with the hidden Dense
    layer (or the per-timestep heads), whose weight gradients go through partial rows.  The plain fp32 engine's dense_bwd and its
    direct weight-gradient kernels add with float atomics - D0.w, U0.w, dense.w and dense.b then differ in the last bits between two
    identical steps -, so a statement about the BITS of the whole gradient arena needs this engine (both heads are non-fused paths,
    which the weighted step composes with)"""
    import gan_class_transfer2_amd as g
    return g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS, f32_matrix=True, seed=5, **{head: True}, **kw)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def test_predict_v_train_step(gpu):
    """the loss is the MSE between the engine's kept prediction and sa eps - sb x, within 1e-6 relative (both are fp64-accumulated means
    of float32 residuals that differ by one rounding of the target); the first step moves the parameters"""
    eng = tiny(gpu, rng_seed=9, predict_v=True)
    eng.base_lr, eng.warm_up = 1e-2, 0
    assert not eng.default_objective() and not eng.objective_weighted()
    x = batch(gpu)
    t_int, eps = injected(gpu)
    before = eng.arena.p.clone()
    loss = eng.train_step(x, t_int, eps)
    torch.cuda.synchronize()
    pred = eng.buffers(B, SIZE, SIZE).pred
    sa, sb = roots(t_int)
    target = sa * eps - sb * x
    want = float(((pred.double() - target.double()) ** 2).mean())
    got = float(loss[0])
    print(f"predict_v train step: loss {got:.9g}, torch {want:.9g}, relative {abs(got - want) / want:.3g}")
    assert abs(got - want) <= 1e-6 * want
    a, c, w = eng.objective_coefficients(t_int)
    assert torch.equal(a.reshape(-1, 1, 1, 1), -sb) and torch.equal(c.reshape(-1, 1, 1, 1), sa) and bool((w == 1).all())
    assert eng.iterations == 1 and not torch.equal(eng.arena.p, before)
    assert int((eng.arena.p != before).sum()) > 1000
    # predict_x is ignored under predict_v: the same step, bit for bit, on the engine whose sums have a fixed order
    steps = []
    for predict_x in (True, False):
        other = fixed_order(gpu, rng_seed=9, predict_v=True, predict_x=predict_x)
        other.base_lr, other.warm_up = 1e-2, 0
        steps.append((other.train_step(x, t_int, eps).clone(), other.arena.p.clone()))
    assert same_bits(steps[0][0], steps[1][0]) and same_bits(steps[0][1], steps[1][1])


# the loss and the gradient arena of the weighted step under a table of ones against the non-fused unweighted step: 1.5 x measured
# (profiles/objective_parity.json), never above 1e-5 - the two paths differ only in the rounding order of dpred.  Measured on the
# fixed_order engine: on the plain tiny engine the float atomics of the reverse pass alone move the arena by 4e-8 .. 7e-8 from run to
# run, and a bound of 1.5 x one such run would be a bound on that noise.  Measured: the gradient arena bit-identical under all three
# objectives (the product with g = 1 is exact and d is formed like gct2_mse_fwd_bwd's); the loss one float32 place apart (8.17e-8,
# 6.26e-8, 8.2e-8 relative: gct2_mse_fwd_bwd adds float32 partial sums, the new kernel fp64 ones)
ONES_BOUND = {"x": (1.23e-7, 0.0), "eps": (9.4e-8, 0.0), "v": (1.23e-7, 0.0)}          # (loss, gradient arena)
OBJECTIVES = {"x": {}, "eps": dict(predict_x=False), "v": dict(predict_v=True)}


@pytest.mark.parametrize("objective", list(OBJECTIVES))
def test_a_table_of_ones_is_the_unweighted_non_fused_step(gpu, objective, parity_log):
    x = batch(gpu)
    t_int, eps = injected(gpu)
    base = fixed_order(gpu, rng_seed=9, **OBJECTIVES[objective])
    base.use_fused_head = False
    want_loss = base.train_step(x, t_int, eps, apply=False).clone()
    want = base.arena.g.clone()
    eng = fixed_order(gpu, rng_seed=9, **OBJECTIVES[objective])
    eng.set_loss_weighting([1.0] * STEPS)
    got_loss = eng.train_step(x, t_int, eps, apply=False).clone()
    got = eng.arena.g.clone()
    torch.cuda.synchronize()
    e_loss, e_grad = abs(float(got_loss[0]) - float(want_loss[0])) / float(want_loss[0]), rel_l2(got, want)
    print(f"table of ones against the unweighted step, {objective}: loss relative {e_loss:.3g}, gradient arena relative L2 {e_grad:.3g}")
    parity_log(f"objective_ones_{objective}", loss_rel=e_loss, grad_rel_l2=e_grad)
    assert float(want.abs().max()) > 0 and max(ONES_BOUND[objective]) <= 1e-5
    assert e_loss <= ONES_BOUND[objective][0] and e_grad <= ONES_BOUND[objective][1], (objective, e_loss, e_grad)
    assert eng.buffers(B, SIZE, SIZE).target is None               # no target plane was written


@pytest.mark.parametrize("head", ["hidden_dense", "timestep_heads"])
@pytest.mark.parametrize("loss", ["mse", "l1"])
def test_a_table_of_twos_doubles_loss_and_gradients_exactly(gpu, loss, head):
    """the loss and the WHOLE gradient arena, bit for bit: a power of two scales every product and sum of the reverse pass exactly, as
    long as its sums have a fixed order (fixed_order; the weighted step composes with both non-fused heads)"""
    x = batch(gpu)
    t_int, eps = injected(gpu)
    out = []
    for weight in (1.0, 2.0):
        eng = fixed_order(gpu, head, rng_seed=9, predict_x=False)
        eng.training_loss = loss
        eng.set_loss_weighting([weight] * STEPS)
        l = eng.train_step(x, t_int, eps, apply=False).clone()
        out.append((l, eng.arena.g.clone()))
    torch.cuda.synchronize()
    (l1, g1), (l2, g2) = out
    assert float(g1.abs().max()) > 0 and int((g1 != 0).sum()) > 1000
    assert same_bits(l2, 2 * l1) and same_bits(g2, 2 * g1)


@pytest.mark.parametrize("loss", ["mse", "l1"])
def test_a_table_of_twos_on_the_plain_engine(gpu, loss):
    """the plain fp32 engine (float atomics in its weight gradients): the loss and the gradient of the prediction, which the new launch
    writes, still double exactly"""
    x = batch(gpu)
    t_int, eps = injected(gpu)
    out = []
    for weight in (1.0, 2.0):
        eng = tiny(gpu, rng_seed=9, predict_x=False)
        eng.training_loss = loss
        eng.set_loss_weighting([weight] * STEPS)
        l = eng.train_step(x, t_int, eps, apply=False).clone()
        b = eng.buffers(B, SIZE, SIZE)
        out.append((l, b.dpred.clone()))
    torch.cuda.synchronize()
    (l1, d1), (l2, d2) = out
    assert float(d1.abs().max()) > 0 and same_bits(l2, 2 * l1) and same_bits(d2, 2 * d1)


def test_min_snr_loss_is_the_weighted_mean_of_the_evaluation_rows(gpu):
    """gamma = 0.1 under the epsilon objective at t = 1, 2, 5, 6: the step's loss against mean(lambda_b rows_b) of an UNWEIGHTED
    evaluate_batch at the same t and eps, within 1e-6 relative (float32 casts of the loss and of every row: 2^-23 together)"""
    import gan_class_transfer2_amd as g
    x = batch(gpu)
    t_int, eps = injected(gpu)
    plain = tiny(gpu, rng_seed=9, predict_x=False)
    rows, tt = plain.evaluate_batch(x, t=T_INT, eps=eps)
    eng = tiny(gpu, rng_seed=9, predict_x=False)
    eng.set_loss_weighting("min_snr", 0.1)
    loss = eng.train_step(x, t_int, eps, apply=False).clone()
    call_rows, _ = eng.evaluate_batch(x, t=T_INT, eps=eps)       # the weighted rows of evaluation, and their weights
    torch.cuda.synchronize()
    table = g.trainer_math.loss_weight_table("min_snr", 0.1, STEPS, "eps")
    lam = table[T_INT].astype(np.float64)
    assert (lam == 1).any() and (lam < 1).any() and tt.cpu().tolist() == T_INT
    want = float((lam * rows.cpu().numpy().astype(np.float64)).mean())
    got = float(loss[0])
    print(f"min_snr step loss {got:.9g}, weighted mean of the rows {want:.9g}, relative {abs(got - want) / want:.3g}")
    assert abs(got - want) <= 1e-6 * want
    assert np.array_equal(eng.last_eval["loss_weight"].cpu().numpy(), table[T_INT])
    assert same_bits(call_rows, rows * eng.last_eval["loss_weight"]) and "loss_weight" not in plain.last_eval


def test_generate_and_encode_in_mode_v(gpu):
    import gan_class_transfer2_amd as g
    L = lib()
    eng = tiny(gpu, predict_v=True)
    kw = dict(num_steps=3, eta=0, clip_denoised=False, predict_v=True)
    taus = g.sampling_timesteps(STEPS, 3)
    # the drawn start: what gct2_diffusion_start reads for images 0 and 1 of seed 0
    per = SIZE * SIZE * 3
    z = torch.empty(2, SIZE, SIZE, 3, device=gpu)
    for i in range(2):
        L.call("gct2_rng_normal", 0, g.GENERATE_STREAM, g.trainer_math.generate_offset(i, 0, 3, per), z[i].data_ptr(), per, stream())
    want = hand_loop(eng, z, taus, L.SAMPLE_V)
    assert torch.isfinite(want).all() and float(want.std()) > 0
    for more in (dict(size=SIZE), dict(noise=z), dict(size=SIZE, use_graph=False)):
        got = g.generate(den(eng), 2, **kw, **more)
        torch.cuda.synchronize()
        assert same_bits(got, want), (more, float((got - want).abs().max()))
    four = g.generate(den(eng), 4, size=SIZE, **kw)
    hi = g.generate(den(eng), 2, size=SIZE, first_index=2, **kw)
    assert same_bits(four, torch.cat([want, hi]))
    two = dict(kw, num_steps=2)
    assert same_bits(g.generate(den(eng), 2, size=SIZE, solver="dpm2m", **two), g.generate(den(eng), 2, size=SIZE, solver="ddim", **two))
    multi = g.generate(den(eng), 2, size=SIZE, solver="dpm2m", **dict(kw, num_steps=6))
    assert torch.isfinite(multi).all() and not same_bits(multi, g.generate(den(eng), 2, size=SIZE, **dict(kw, num_steps=6)))
    for solver in ("ddim", "dpm2m"):
        latent = g.encode(den(eng), batch(gpu, 2), num_steps=3, predict_v=True, solver=solver)
        assert tuple(latent.shape) == (2, SIZE, SIZE, 3) and torch.isfinite(latent).all() and float(latent.std()) > 0
    # the engine's own objective is the sampler's: a mismatch is refused either way
    with pytest.raises(ValueError, match="mode"):
        g.generate(den(eng), 2, size=SIZE, num_steps=3, predict_v=False)
    with pytest.raises(ValueError, match="mode"):
        g.generate(den(tiny(gpu)), 2, size=SIZE, num_steps=3, predict_v=True)


@pytest.fixture
def tiny_model():
    """the module-level hyper-parameters of the reference script set to the tiny configuration, restored afterwards"""
    import gan_class_transfer2_amd as g
    names = ("size", "pixel_size", "max_size", "octaves", "steps", "compute_dtype", "mixed_precision", "block_depth", "residual", "concat",
             "warm_up", "regularizer", "training_loss", "predict_x", "predict_scaled_epsilon", "prediction_weighting",
             "ordinary_differential_equation", "predict_v", "loss_weighting", "min_snr_gamma", "noise_schedule", "alpha_dash_offset")
    keep = {n: getattr(g.model, n) for n in names}
    g.configure(size=SIZE, pixel_size=8, max_size=16, octaves=2, steps=STEPS, compute_dtype="float32", mixed_precision=False,
                block_depth=0, residual=False, concat=True, regularizer=None, training_loss="mse", predict_x=True,
                predict_scaled_epsilon=False, prediction_weighting=False, ordinary_differential_equation=False, predict_v=False,
                loss_weighting=None, min_snr_gamma=5.0, noise_schedule="quadratic", alpha_dash_offset=0.0)
    yield g
    g.configure(**keep)


def test_trainer_follows_the_new_globals(gpu, tiny_model):
    """configure(predict_v=..., loss_weighting=...) reach the engine before every step; evaluate(metrics=["psnr"]) under predict_v is
    image_metrics(sa noised - sb pred, x) (the PSNR of two estimates that differ by float32 roundings of x0, 1e-7 relative to values of
    size <= 4 against errors of size 1: below 1e-4 dB; bound 1e-3 dB); Trainer.call takes the loss-only form; the weighted evaluation
    reports the weighted mean and loss_weight"""
    g = tiny_model
    g.configure(predict_v=True)
    tr = g.Trainer(g.Denoiser(seed=3, device=gpu))
    tr.compile(g.Adam(1e-3), g.identity)
    x = batch(gpu)
    out = tr.evaluate([x], t=T_INT, metrics=["psnr"], return_dict=True)
    eng = tr.denoiser.engine
    assert eng.predict_v and eng.loss_weighting is None and "loss_weight" not in out
    last = eng.last_eval
    t_int = torch.tensor(T_INT, dtype=torch.int32, device=gpu)
    a = [float(g.trainer_math.alpha_dash(float(t), STEPS)) for t in T_INT]
    sa = torch.tensor([v ** 0.5 for v in a], dtype=torch.float32, device=gpu).reshape(-1, 1, 1, 1)
    sb = torch.tensor([(1 - v) ** 0.5 for v in a], dtype=torch.float32, device=gpu).reshape(-1, 1, 1, 1)
    assert last["metrics"]["mode"] == g._lib.SAMPLE_V
    x0 = sa * last["metrics"]["noised"] - sb * last["pred"]
    want = g.model.image_metrics(x0, x)["psnr"].cpu().numpy()
    print(f"psnr under predict_v: {out['per_image_psnr']}, image_metrics of sa noised - sb pred: {want}")
    assert np.isfinite(want).all() and np.abs(out["per_image_psnr"] - want).max() <= 1e-3
    # the weights: a train step, Trainer.call and evaluate all follow the globals
    g.configure(loss_weighting="min_snr", min_snr_gamma=0.1)
    plain = out["per_image"]
    weighted = tr.evaluate([x], t=T_INT, return_dict=True)
    assert (eng.loss_weighting, eng.min_snr_gamma) == ("min_snr", 0.1)
    lam = g.trainer_math.loss_weight_table("min_snr", 0.1, STEPS, "v")[T_INT]
    assert np.array_equal(weighted["loss_weight"], lam) and np.array_equal(weighted["per_image"], plain * lam)
    assert weighted["loss"] == float(np.mean(weighted["per_image"], dtype=np.float64))
    state = _state(eng)
    loss = tr(x)                                                  # Trainer.call: the loss only, no gradient, no step
    assert torch.isfinite(loss) and eng.iterations == state["iterations"]
    step = tr.train_step((x, x))["loss"]
    assert torch.isfinite(step).all() and eng.iterations == state["iterations"] + 1
    # what the globals refuse, before anything launches
    g.configure(training_loss="dct")
    with pytest.raises(ValueError, match="training_loss"):
        tr.train_step((x, x))
    g.configure(training_loss="mse", loss_weighting=None, ordinary_differential_equation=True)
    with pytest.raises(ValueError, match="predict_v"):
        tr.train_step((x, x))
    g.configure(ordinary_differential_equation=False, predict_v=False, predict_x=False, predict_scaled_epsilon=True, loss_weighting="min_snr")
    with pytest.raises(ValueError, match="loss_weighting"):
        tr.train_step((x, x))
    assert eng.iterations == state["iterations"] + 1


def test_refusals_on_the_engine(gpu):
    from gan_class_transfer2_amd.distributed import DataParallelStep, ShardedDataParallelStep
    import gan_class_transfer2_amd as g
    x = batch(gpu, 2)
    eng = tiny(gpu, predict_x=False)
    eng.set_loss_weighting("min_snr", 0.1)
    for wrapper in (DataParallelStep, ShardedDataParallelStep):
        with pytest.raises(ValueError, match="loss_weighting"):
            wrapper(eng)
    eng.training_loss = "dct"
    with pytest.raises(ValueError, match="training_loss"):
        eng.train_step(x)
    with pytest.raises(ValueError, match="training_loss"):
        eng.evaluate_batch(x)
    eng.training_loss = "mse"
    eng.set_loss_weighting(None)
    eng.training_loss = "dct"
    with pytest.raises(ValueError, match="training_loss"):
        eng.set_loss_weighting("min_snr", 0.1)
    assert eng.loss_weighting is None
    with pytest.raises(ValueError, match="predict_v"):
        tiny(gpu, predict_v=True, ordinary_differential_equation=True)
    with pytest.raises(ValueError, match="predict_v"):
        tiny(gpu, predict_v=True, predict_x=False, prediction_weighting=True)
    bad = tiny(gpu, predict_v=True)
    bad.ordinary_differential_equation = True
    for run in (lambda: bad.train_step(x), lambda: bad.evaluate_batch(x), lambda: g.generate(den(bad), 2, size=SIZE, num_steps=2)):
        with pytest.raises(ValueError, match="predict_v"):
            run()
    assert _state(bad) == dict(rng_t=0, rng_eps=0, iterations=0) and _state(eng) == dict(rng_t=0, rng_eps=0, iterations=0)


def test_evaluate_and_generate_move_no_training_state(gpu):
    """a weighted v-objective train step taken after evaluate_batch, generate and encode is bit-identical to one taken without them; the
    RNG positions, the step counter and the recorded plans do not move"""
    import gan_class_transfer2_amd as g
    x = batch(gpu, 2)
    engines = [fixed_order(gpu, rng_seed=9, predict_v=True), fixed_order(gpu, rng_seed=9, predict_v=True)]
    for eng in engines:
        eng.base_lr, eng.warm_up = 1e-2, 0
        eng.set_loss_weighting("min_snr", 0.1)
        eng.train_step(x)
    busy = engines[0]
    state, plans = _state(busy), len(busy._plans)
    busy.evaluate_batch(x, metrics=("psnr",))
    g.generate(den(busy), 2, size=SIZE, num_steps=3, predict_v=True)
    g.encode(den(busy), x, num_steps=3, solver="dpm2m", predict_v=True)
    assert _state(busy) == state and len(busy._plans) == plans == 0        # (a weighted step is eager: nothing is ever recorded)
    losses = [eng.train_step(x).clone() for eng in engines]
    torch.cuda.synchronize()
    assert same_bits(losses[0], losses[1]) and same_bits(engines[0].arena.p, engines[1].arena.p)
    assert _state(busy)["iterations"] == state["iterations"] + 1


@pytest.mark.parametrize("loss", ["mse", "l1"])
def test_variant_engine_follows(gpu, loss):
    """a variant network (block_depth = 1) under predict_v with min-SNR weights: the step's loss is the weighted mean of the rows of an
    unweighted evaluate_batch at the same t and eps (1e-6 relative, as above), the loss-only call (Trainer.call's) gives the same loss,
    the step moves the parameters, and generate runs in mode V"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.variants import VariantEngine
    x = batch(gpu)
    t_int, eps = injected(gpu)
    make = lambda: VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4, rng_seed=9, predict_v=True)
    plain, eng = make(), make()
    plain.training_loss = eng.training_loss = loss
    rows, _ = plain.evaluate_batch(x, t=T_INT, eps=eps)
    eng.base_lr, eng.warm_up = 1e-2, 0
    eng.set_loss_weighting("min_snr", 0.1)
    only = eng.train_step(x, t_int, eps, backward=False).clone()
    before = eng.net.p.clone()
    got = eng.train_step(x, t_int, eps).clone()
    torch.cuda.synchronize()
    lam = g.trainer_math.loss_weight_table("min_snr", 0.1, STEPS, "v")[T_INT].astype(np.float64)
    want = float((lam * rows.cpu().numpy().astype(np.float64)).mean())
    print(f"variant, {loss}: step loss {float(got[0]):.9g}, weighted mean of the rows {want:.9g}")
    assert abs(float(got[0]) - want) <= 1e-6 * want and same_bits(only, got)
    assert not torch.equal(eng.net.p, before) and eng.iterations == 1
    out = g.generate(den(eng), 2, num_steps=3, size=SIZE, predict_v=True)
    assert torch.isfinite(out).all() and float(out.std()) > 0
