"""The image metrics on the engines and through Trainer (evaluate_batch(metrics=...), Trainer.evaluate(metrics=...), compile(metrics=...),
fit(validation_data=...), image_metrics) on the GPU, on the tiny network of tests/test_eval_step_gpu.py: Topology(8, 16, 2), 16 x 16
images, steps = 6.

The metrics an engine returns are compared with the float64 restatement of tests/metrics_cases.py formed from the engine's OWN stored
tensors (engine.last_eval: prediction, x, and under "metrics" the fp32 noised image, u, v and the window the launch read) at the
tolerance of tests/test_metrics_kernels_gpu.py; those tensors in turn are checked against trainer_math's host arithmetic.  Evaluation
with metrics must not move any training state, and without metrics nothing about evaluation changes."""
import gc

import numpy as np
import pytest
import torch

import eval_cases as E
import metrics_cases as M

pytestmark = pytest.mark.gpu
TOPO, SIZE, STEPS = (8, 16, 2), 16, 6
F32, BF16 = 0, 1
ALL = ("psnr", "ssim", "mse_x0")
OBJECTIVES = {"default": dict(predict_x=True), "ode": dict(ordinary_differential_equation=True), "epsilon": dict(predict_x=False),
              "scaled_epsilon": dict(predict_x=False, predict_scaled_epsilon=True)}
MODE = {"default": 0, "epsilon": 1, "scaled_epsilon": 2, "ode": 3}
SWITCHES = dict(predict_x=True, predict_scaled_epsilon=False, prediction_weighting=False, ordinary_differential_equation=False)
PRED_BOUND = 2e-5          # tests/test_eval_step_gpu.py: what that file holds per_image to when the set is cut differently
f32, f64 = np.float32, np.float64


@pytest.fixture(autouse=True)
def _collect_engines():
    """engines hold reference cycles (and step plans); collect them here, not inside a later test"""
    yield
    gc.collect()
    torch.cuda.synchronize()


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def unet(gpu, dt, **kw):
    import gan_class_transfer2_amd as g
    return g.UNetEngine(g.Topology(*TOPO), dt, gpu, **{**dict(steps=STEPS, base_lr=1e-2, warm_up=0, seed=21, rng_seed=5), **kw})


def variant(gpu, dt, **kw):
    from gan_class_transfer2_amd.variants import VariantEngine
    return VariantEngine(TOPO[0], TOPO[1], TOPO[2], 1, False, True, dt, gpu, **{**dict(steps=STEPS, base_lr=1e-2, warm_up=0, seed=21, rng_seed=5), **kw})


def batches(gpu, n, B=4, seed=11):
    rng = np.random.default_rng(seed)
    return [torch.tensor(np.floor(rng.uniform(0, 256, (B, SIZE, SIZE, 3))) / 128 - 1, dtype=torch.float32, device=gpu) for _ in range(n)]


def restated(eng):
    """dict(mse_x0, psnr, ssim) float64 [B] from what the metrics launch read"""
    le = eng.last_eval
    f = lambda t: None if t is None else t.detach().float().cpu().numpy()
    m = le["metrics"]
    out = M.metrics(f(le["pred"]), f(le["x"]), f(m["window"]), f(m["noised"]), f(m["u"]), f(m["v"]))
    return dict(mse_x0=out["mse"], psnr=out["psnr"], ssim=out["ssim"])


def assert_metrics(eng, got, tag):
    torch.cuda.synchronize()
    want = restated(eng)
    for n, v in got.items():
        v = v.cpu().numpy() if torch.is_tensor(v) else v
        print(tag, n, v, want[n])
        M.assert_close(v, want[n], (tag, n))
    return want


# ---- 1. the metrics against the restatement: both engines, four objectives, a table schedule ------------------------------------------------
@pytest.mark.parametrize("schedule", ["quadratic", "cosine"])
@pytest.mark.parametrize("make", [unet, variant], ids=["unet", "variant"])
def test_metrics_equal_the_restatement_of_the_engines_own_tensors(gpu, make, schedule):
    import gan_class_transfer2_amd as g
    T = g.trainer_math
    eng = make(gpu, F32)
    if schedule != "quadratic":
        eng.set_noise_schedule(schedule)
    x, = batches(gpu, 1)
    seen = {}
    for oname, switches in OBJECTIVES.items():
        for k, v in {**SWITCHES, **switches}.items():
            setattr(eng, k, v)
        rows, t, got = eng.evaluate_batch(x, index0=3, metrics=ALL)
        assert list(got) == list(ALL) and all(v.dtype == torch.float32 and v.shape == (4,) for v in got.values())
        want = assert_metrics(eng, got, (oname, schedule))
        seen[oname] = want["mse_x0"]
        m, le = eng.last_eval["metrics"], eng.last_eval
        assert m["mode"] == MODE[oname] and np.array_equal(m["window"].cpu().numpy(), T.ssim_window())
        tt = t.cpu().numpy()
        if oname == "default":                                  # x0 is the prediction itself: nothing is mixed, nothing is kept
            assert m["u"] is None and m["v"] is None and m["noised"] is None
            # ... and mse_x0 is the MSE row of the loss launch on the same tensors (training_loss "mse", default objective)
            # (another order of the float64 partial sums: one float32 ulp, the tolerance of either kernel)
            assert E.ulps(got["mse_x0"].cpu().numpy(), rows.cpu().numpy()).max() <= 1
            continue
        u, v = T.x0_coefficients(tt, STEPS, MODE[oname], schedule, 0.0)
        assert np.array_equal(m["u"].cpu().numpy(), u) and np.array_equal(m["v"].cpu().numpy(), v)
        # the fp32 noised image: fl(fl(sqrt(a) x) + fl(sqrt(1 - a) eps)) with the roots of each image's timestep
        if schedule == "quadratic":
            a = T.alpha_dash(torch.tensor(tt, dtype=torch.float32), STEPS)
            sa, sb = a.sqrt().numpy(), (1 - a).sqrt().numpy()
        else:
            roots = T.alpha_roots(schedule, 0.0, STEPS)
            sa, sb = roots[0][tt], roots[1][tt]
        noised = E.residual(np.zeros_like(le["x"].cpu().numpy()), le["x"].cpu().numpy(), le["eps"].cpu().numpy(), sa, sb)
        got_noised = m["noised"].cpu().numpy()
        if schedule == "quadratic":
            # the roots are torch's on the device there and on the host here: one float32 ulp each at most, then the two products
            # and the sum round: 3 * 2^-24 (|x| + |eps|), both roots being at most 1
            bound = 3 * 2.0 ** -24 * (np.abs(le["x"].cpu().numpy()) + np.abs(le["eps"].cpu().numpy()))
            assert (np.abs(got_noised - noised) <= bound).all()
        else:
            assert np.array_equal(got_noised.view(np.int32), noised.view(np.int32))
        # the network saw the same image (up to the rounding of its own noising kernel)
        assert np.abs(le["noised"][..., :3].float().cpu().numpy() - got_noised).max() <= 1e-5
    assert len({tuple(np.round(v, 9)) for v in seen.values()}) == len(seen)          # four different estimates
    assert (eng.rng_offset_t, eng.rng_offset_eps, eng.iterations) == (0, 0, 0)


def test_bf16_engines_report_metrics_too(gpu):
    eng = unet(gpu, BF16, predict_x=False)
    x, = batches(gpu, 1)
    _, _, got = eng.evaluate_batch(x, metrics=("ssim", "psnr"))
    assert list(got) == ["ssim", "psnr"]
    assert_metrics(eng, got, "bf16")


# ---- 2. the metrics belong to the image, not to the batch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [unet, variant], ids=["unet", "variant"])
def test_metrics_do_not_depend_on_how_the_set_is_split(gpu, make):
    eng = make(gpu, F32, predict_x=False)                      # the epsilon objective: eps is kept and enters the estimate
    x, = batches(gpu, 1, B=5)
    runs = {}
    for cut in ((5,), (2, 3), (1, 1, 1, 1, 1)):
        first, parts = 0, {n: [] for n in ALL + ("t",)}
        for width in cut:
            _, t, got = eng.evaluate_batch(x[first:first + width], index0=100 + first, metrics=ALL)
            torch.cuda.synchronize()
            for n in ALL:
                parts[n].append(got[n].clone())
            parts["t"].append(t.clone())
            first += width
        runs[cut] = {n: torch.cat(v) for n, v in parts.items()}
    whole = runs[(5,)]
    for cut in ((2, 3), (1, 1, 1, 1, 1)):
        assert torch.equal(runs[cut]["t"], whole["t"]), cut
        for n in ALL:
            dist = float(((runs[cut][n] - whole[n]).abs() / whole[n].abs()).max())
            print(cut, n, dist)
            assert dist <= PRED_BOUND, f"{n} of {cut} against one batch of 5: max relative distance {dist:.3g} (bound {PRED_BOUND})"


# ---- 3. evaluation with metrics moves no training state ------------------------------------------------------------------------------------
def state_of(eng):
    torch.cuda.synchronize()
    A = eng.arena
    return {n: getattr(A, n).clone() for n in ("p", "m", "v") + (("shadow",) if A.shadow is not None else ())}


# (batch 1: tests/test_eval_step_gpu.py says why two free-running engines can be compared bit for bit only there)
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_evaluating_with_metrics_between_steps_changes_nothing(gpu, dt, batch=1):
    xs = batches(gpu, 6, B=batch)
    held_out, = batches(gpu, 1, B=batch, seed=3)
    kw = dict(predict_x=(dt != F32))                           # fp32: the epsilon objective, whose metrics also form the noised image
    A, B = unet(gpu, dt, **kw), unet(gpu, dt, **kw)
    la, lb = [], []
    for k in range(6):
        if k in (2, 3):
            plans = dict(A._plans)
            A.evaluate_batch(held_out, index0=17, metrics=ALL)
            assert A._plans == plans and (A.rng_offset_t, A.rng_offset_eps) == (B.rng_offset_t, B.rng_offset_eps)
        la.append(A.train_step(xs[k]).clone())
        lb.append(B.train_step(xs[k]).clone())
    sa, sb = state_of(A), state_of(B)
    assert [bits(l).item() for l in la] == [bits(l).item() for l in lb], (la, lb)
    for n in sa:
        assert torch.equal(bits(sa[n]), bits(sb[n])), n
    assert (A.iterations, A.rng_offset_t, A.rng_offset_eps) == (B.iterations, B.rng_offset_t, B.rng_offset_eps) == (6, 6 * batch, 6 * batch * SIZE * SIZE * 3)


# ---- 4. without metrics nothing changes -------------------------------------------------------------------------------------------------
def record_calls(monkeypatch):
    """every entry point the engines' host code calls from here on, by name"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import variants
    names, real = [], g._lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    for mod in (g._lib, g.trainer_math, g.engine, variants, g.model):
        if getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", spy)
    return names


@pytest.mark.parametrize("oname", ["default", "epsilon"])
def test_no_metrics_no_launches(gpu, monkeypatch, oname):
    eng = unet(gpu, F32, **OBJECTIVES[oname])
    x, = batches(gpu, 1)
    eng.evaluate_batch(x)                                       # (buffers and tables exist from here on)
    names = record_calls(monkeypatch)
    out = eng.evaluate_batch(x)
    plain = list(names)
    assert isinstance(out, tuple) and len(out) == 2
    assert set(eng.last_eval) == {"x", "pred", "eps", "t_int", "coef", "noised"}
    assert "gct2_image_metrics" not in plain and "gct2_eval_loss_rows" in plain
    del names[:]
    out = eng.evaluate_batch(x, metrics=())
    assert len(out) == 2 and names == plain                     # the empty tuple is no metrics
    del names[:]
    out = eng.evaluate_batch(x, metrics=("ssim",))
    assert len(out) == 3 and set(eng.last_eval) == {"x", "pred", "eps", "t_int", "coef", "noised", "metrics"}
    extra = list(names)
    for n in plain:
        extra.remove(n)
    assert extra == (["gct2_image_metrics"] if oname == "default" else ["gct2_mix_per_image", "gct2_image_metrics"])
    with pytest.raises(ValueError, match="unknown metric"):
        eng.evaluate_batch(x, metrics=("accuracy",))


# ---- 5. Trainer: evaluate, compile, fit, image_metrics ---------------------------------------------------------------------------------------
@pytest.fixture
def tiny_model():
    """the module-level hyper-parameters of the tiny fp32 network, put back afterwards"""
    import gan_class_transfer2_amd as g
    names = ("size", "pixel_size", "max_size", "octaves", "steps", "compute_dtype", "mixed_precision", "block_depth", "residual", "concat",
             "warm_up", "regularizer", "training_loss", "predict_x")
    keep = {n: getattr(g.model, n) for n in names}
    g.configure(size=SIZE, pixel_size=TOPO[0], max_size=TOPO[1], octaves=TOPO[2], steps=STEPS, compute_dtype="float32", mixed_precision=False,
                block_depth=0, residual=False, concat=True, regularizer=None, training_loss="mse", predict_x=True)
    yield g
    g.configure(**keep)


@pytest.mark.parametrize("predict_x", [True, False], ids=["predict_x", "epsilon"])
def test_trainer_evaluate_reports_metrics(gpu, tiny_model, monkeypatch, predict_x):
    g = tiny_model
    g.configure(predict_x=predict_x)
    tr = g.Trainer(g.Denoiser(seed=3, device=gpu))
    tr.compile(g.Adam(1e-3), g.identity)
    x, = batches(gpu, 1, B=10)
    data = [(x[0:4], x[0:4]), x[4:8], (x[8:10], x[8:10])]
    plain = tr.evaluate(data)
    assert isinstance(plain, float)                             # no metrics compiled, none asked: exactly as before
    assert set(tr.evaluate(data, return_dict=True)) == {"loss", "per_image", "t"}
    names = record_calls(monkeypatch)
    assert tr.evaluate(data, metrics=()) == plain
    assert "gct2_image_metrics" not in names and names.count("gct2_mix_per_image") == 0
    out = tr.evaluate(data, metrics=ALL, return_dict=True)
    eng = tr.denoiser.engine
    assert list(out) == ["loss", "per_image", "t", "psnr", "per_image_psnr", "ssim", "per_image_ssim", "mse_x0", "per_image_mse_x0"]
    assert out["loss"] == plain
    per = {n: [] for n in ALL}
    for a, b in ((0, 4), (4, 8), (8, 10)):                      # the same batches, one by one, each against the restatement
        _, _, got = eng.evaluate_batch(x[a:b], index0=a, metrics=ALL)
        assert_metrics(eng, got, (predict_x, a))
        for n in ALL:
            per[n].append(got[n].cpu().numpy())
    for n in ALL:
        assert out["per_image_" + n].dtype == f32 and np.array_equal(out["per_image_" + n], np.concatenate(per[n])), n
        assert isinstance(out[n], float) and out[n] == float(np.mean(out["per_image_" + n], dtype=f64))
    assert 0 < out["mse_x0"] and np.isfinite(out["psnr"]) and -1 <= out["ssim"] < 1
    if predict_x:                                               # the estimate is the prediction: the loss is its mean squared error
        assert E.ulps(out["per_image_mse_x0"], out["per_image"]).max() <= 1
    # the list form, in the order asked
    assert tr.evaluate(data, metrics=("psnr",)) == [plain, out["psnr"]]
    assert tr.evaluate(data, metrics=["ssim", "mse_x0", "psnr"]) == [plain, out["ssim"], out["mse_x0"], out["psnr"]]
    # compiled metrics are the default; () switches them off for one call
    tr.compile(g.Adam(1e-3), g.identity, metrics=["ssim"])
    assert tr.evaluate(data) == [plain, out["ssim"]] and tr.evaluate(data, metrics=()) == plain
    assert tr.evaluate(data, metrics=["psnr"]) == [plain, out["psnr"]]
    # PSNR by timestep: any per-image vector bins like the loss
    counts, means = g.trainer_math.loss_by_timestep(out["per_image_psnr"], out["t"], STEPS)
    assert counts.sum() == 10 and abs(np.nansum(counts * means) / 10 - out["psnr"]) <= 1e-12 * abs(out["psnr"])
    with pytest.raises(ValueError, match="unknown metric"):
        tr.evaluate(data, metrics=["accuracy"])
    assert (eng.iterations, eng.rng_offset_t, eng.rng_offset_eps) == (0, 0, 0)


def test_fit_logs_the_compiled_metrics(gpu, tiny_model, capsys):
    g = tiny_model
    train = [(x, x) for x in batches(gpu, 4, B=1)]
    held_out = [(x, x) for x in batches(gpu, 2, seed=3)]
    tr = g.Trainer(g.Denoiser(seed=3, device=gpu))
    tr.compile(g.Adam(1e-2), g.identity, metrics=["ssim"])
    logs = []
    hist = tr.fit(train, steps_per_epoch=2, epochs=2, callbacks=[g.LambdaCallback(on_epoch_end=lambda e, l: logs.append(dict(l)))],
                  validation_data=held_out)
    printed = capsys.readouterr().out.strip().splitlines()
    assert list(hist) == ["loss", "val_loss", "val_ssim"] and len(hist["val_ssim"]) == 2
    assert [set(l) for l in logs] == [{"loss", "val_loss", "val_ssim"}] * 2
    assert [l["val_ssim"] for l in logs] == hist["val_ssim"] and hist["val_ssim"][0] != hist["val_ssim"][1]
    assert all(-1 <= v <= 1 for v in hist["val_ssim"]) and all(" - val_ssim: " in p for p in printed)
    assert [hist["val_loss"][1], hist["val_ssim"][1]] == tr.evaluate(held_out)


def test_image_metrics_of_two_batches(gpu):
    import gan_class_transfer2_amd as g
    a, = batches(gpu, 1, B=3)
    same = g.image_metrics(a, a)
    torch.cuda.synchronize()
    assert list(same) == ["mse_x0", "psnr", "ssim"]
    assert torch.equal(same["ssim"], torch.ones(3, device=gpu)) and bool((same["mse_x0"] == 0).all()) and bool(torch.isposinf(same["psnr"]).all())
    b = (a + 0.05 * torch.randn(a.shape, generator=torch.Generator().manual_seed(2)).to(gpu)).contiguous()
    got = g.image_metrics(a, b)
    want = M.metrics(a.cpu().numpy(), b.cpu().numpy(), g.trainer_math.ssim_window())
    for n, k in (("mse_x0", "mse"), ("psnr", "psnr"), ("ssim", "ssim")):
        M.assert_close(got[n].cpu().numpy(), want[k], n)
    box = g.image_metrics(a, b, filter_size=8, filter_sigma=100.0, max_val=1.0)
    want = M.metrics(a.cpu().numpy(), b.cpu().numpy(), g.trainer_math.ssim_window(8, 100.0), max_val=1.0)
    M.assert_close(box["ssim"].cpu().numpy(), want["ssim"], "box ssim")
    M.assert_close(box["psnr"].cpu().numpy(), want["psnr"], "box psnr")
    with pytest.raises(ValueError):
        g.image_metrics(a, b[:2])
    with pytest.raises(g.Gct2Error, match="smaller than"):
        g.image_metrics(a[:, :8], b[:, :8])
