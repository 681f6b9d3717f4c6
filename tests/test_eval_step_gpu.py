"""Evaluation on the engines and through Trainer (evaluate_batch, Trainer.evaluate, fit(validation_data=...)) on the GPU, tiny network:
Topology(8, 16, 2), 16 x 16 images, steps = 6.

The rows an engine returns are compared with the float64 restatement of tests/eval_cases.py formed from the engine's OWN stored
prediction, x, eps and coefficients (engine.last_eval), at the tolerances of tests/test_eval_kernels_gpu.py: 1 ulp of
float32(restatement) for MSE, L1 and pooled MSE, the DCT bound of tests/test_losses_gpu.py per image.  Evaluation must not move any
training state: an engine that evaluates between its steps stays bit-identical to one that does not."""
import gc

import numpy as np
import pytest
import torch

import eval_cases as E
import loss_cases as K

pytestmark = pytest.mark.gpu
TOPO, SIZE, STEPS = (8, 16, 2), 16, 6
F32, BF16, F16 = 0, 1, 2
LOSSES = ("mse", "l1", "mse_pooled", "dct")
OBJECTIVES = {"default": dict(predict_x=True), "ode": dict(ordinary_differential_equation=True), "epsilon": dict(predict_x=False),
              "scaled_epsilon": dict(predict_x=False, predict_scaled_epsilon=True), "weighting": dict(predict_x=False, prediction_weighting=True)}
SWITCHES = dict(predict_x=True, predict_scaled_epsilon=False, prediction_weighting=False, ordinary_differential_equation=False)
PRED_BOUND = 2e-5          # tests/test_step_gpu.py: fp32 prediction, rel-L2


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
    return g.UNetEngine(g.Topology(*TOPO), dt, gpu, **{**dict(steps=STEPS, base_lr=1e-2, warm_up=0, seed=21, rng_seed=5, loss_scaling=(dt == F16)), **kw})


def variant(gpu, dt, **kw):
    from gan_class_transfer2_amd.variants import VariantEngine
    return VariantEngine(TOPO[0], TOPO[1], TOPO[2], 1, False, True, dt, gpu, **{**dict(steps=STEPS, base_lr=1e-2, warm_up=0, seed=21, rng_seed=5), **kw})


def batches(gpu, n, B=4, seed=11):
    rng = np.random.default_rng(seed)
    return [torch.tensor(np.floor(rng.uniform(0, 256, (B, SIZE, SIZE, 3))) / 128 - 1, dtype=torch.float32, device=gpu) for _ in range(n)]


def restated(eng, kind_name):
    """(float64 rows, residual) from what the engine's launches read: its stored prediction, x, eps and coefficient vectors"""
    import gan_class_transfer2_amd as g
    le = eng.last_eval
    f = lambda t: None if t is None else t.detach().float().cpu().numpy()
    a, c, w = (f(v) for v in le["coef"])
    eps = f(le["eps"]) if a is not None else None
    G = g.trainer_math.dct_basis(SIZE) if kind_name == "dct" else None
    d = E.residual(f(le["pred"]), f(le["x"]), eps, a, c, w)
    return E.rows_of_residual(K.KINDS[kind_name], d, G), d, G


def assert_rows(eng, rows, kind_name, tag):
    torch.cuda.synchronize()
    want, d, G = restated(eng, kind_name)
    got = rows.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all() and want.min() > 0, tag
    if kind_name != "dct":
        u = E.ulps(got, want.astype(np.float32))
        assert u.max() <= 1, (tag, got, want)
    else:
        e32 = E.fp32_dct_rows_error(d, G, want)
        err = np.abs(got.astype(np.float64) - want) / want
        assert (err <= np.maximum(1e-6, 4 * e32)).all(), (tag, err, e32)
    return want


# ---- 1. rows against the restatement: both engines, two dtypes, five objectives, four losses ---------------------------------------------
@pytest.mark.parametrize("make", [unet, variant], ids=["unet", "variant"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_rows_equal_the_restatement_of_the_engines_own_tensors(gpu, make, dt):
    eng = make(gpu, dt)
    x, = batches(gpu, 1)
    seen = {}
    for oname, switches in OBJECTIVES.items():
        for k, v in {**SWITCHES, **switches}.items():
            setattr(eng, k, v)
        for loss in LOSSES:
            eng.training_loss = loss
            rows, t = eng.evaluate_batch(x, index0=3)
            want = assert_rows(eng, rows, loss, (oname, loss))
            seen[(oname, loss)] = want
            a, c, w = eng.last_eval["coef"]
            assert (a is None) == (c is None) == (oname == "default") and (w is not None) == (oname == "weighting")
            if oname == "weighting":                           # the prediction is read only: what the forward pass stored is still there
                pred = eng.last_eval["pred"].clone()
                noised = eng.last_eval["noised"][..., :3].clone()
                again = eng.predict(noised, t)
                torch.cuda.synchronize()
                assert torch.equal(bits(again), bits(pred)), (oname, loss)
    assert len({tuple(np.round(v, 9)) for v in seen.values()}) == len(seen)          # twenty different figures
    assert (eng.rng_offset_t, eng.rng_offset_eps, eng.iterations) == (0, 0, 0)


# ---- 2. evaluation moves no training state ----------------------------------------------------------------------------------------------
def state_of(eng):
    torch.cuda.synchronize()
    A = eng.arena
    st = {n: getattr(A, n).clone() for n in ("p", "m", "v") + (("shadow",) if A.shadow is not None else ())}
    if eng.ls_state is not None:
        st["ls_state"] = eng.ls_state.clone()
    return st


# Batch 1.  Two free-running engines can be compared bit for bit only where no float atomic decides a bit, and at this topology that is
# batch 1: the plain head's gct2_dense_bwd adds one partial sum per 128 pixels into the zeroed dense.w / dense.b in arrival order
# (tests/test_noise_schedule_step_gpu.py lockstep) - two work-groups at batch 1, where 0 + a + b = 0 + b + a and the order cannot show.
# Measured on an MI355X with NO evaluation anywhere: six steps of two engines with the same seeds agree in every bit at batch 1 (plain,
# hidden-Dense and per-timestep heads) and differ in every tensor at batch 4 (all three heads).  The held-out batch has the training
# shape, so evaluation runs in the buffer set the train steps (and their recorded plans) use
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16_loss_scaled"])
def test_evaluating_between_steps_changes_nothing(gpu, dt, batch=1):
    xs = batches(gpu, 6, B=batch)
    held_out, = batches(gpu, 1, B=batch, seed=3)
    A, B = unet(gpu, dt), unet(gpu, dt)
    assert A.use_plan and B.use_plan
    la, lb = [], []
    for k in range(6):
        if k == 3:
            plans = dict(A._plans)
            for loss in ("mse", "dct"):                        # (the setting is evaluation's alone here: put back before the next step)
                A.training_loss = loss
                A.evaluate_batch(held_out, index0=17)
            A.training_loss = "mse"
            assert A._plans == plans and (A.rng_offset_t, A.rng_offset_eps) == (B.rng_offset_t, B.rng_offset_eps)
        la.append(A.train_step(xs[k]).clone())
        lb.append(B.train_step(xs[k]).clone())
    sa, sb = state_of(A), state_of(B)
    assert [bits(l).item() for l in la] == [bits(l).item() for l in lb], (la, lb)
    for n in sa:
        assert torch.equal(bits(sa[n]), bits(sb[n])), n
    assert (A.iterations, A.rng_offset_t, A.rng_offset_eps) == (B.iterations, B.rng_offset_t, B.rng_offset_eps) == (6, 6 * batch, 6 * batch * SIZE * SIZE * 3)
    if dt == F16:
        assert A.loss_scale() == B.loss_scale()


def test_evaluation_is_refused_inside_a_recording(gpu, monkeypatch):
    import gan_class_transfer2_amd as g
    eng = unet(gpu, F32)
    x, = batches(gpu, 1)
    monkeypatch.setattr(g._lib, "_recording", object())
    with pytest.raises(g._lib.Gct2Error, match="recording"):
        eng.evaluate_batch(x)


# ---- 3. the draws belong to the image, not to the batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [unet, variant], ids=["unet", "variant"])
def test_rows_do_not_depend_on_how_the_set_is_split(gpu, make):
    eng = make(gpu, F32, predict_x=False)                      # the epsilon objective: eps is kept and enters the target
    x, = batches(gpu, 1, B=8)
    runs = {}
    for width in (8, 4, 1):
        rows, ts, noised, eps = [], [], [], []
        for first in range(0, 8, width):
            r, t = eng.evaluate_batch(x[first:first + width], index0=100 + first)
            torch.cuda.synchronize()
            rows.append(r.clone()); ts.append(t.clone())
            noised.append(eng.last_eval["noised"][..., :3].clone()); eps.append(eng.last_eval["eps"].clone())
        runs[width] = tuple(torch.cat(v) for v in (rows, ts, noised, eps))
    r8, t8, n8, e8 = runs[8]
    assert 1 <= int(t8.min()) and int(t8.max()) <= STEPS and len(set(t8.tolist())) > 1
    for width in (4, 1):
        r, t, n, e = runs[width]
        assert torch.equal(t, t8), width
        assert torch.equal(bits(n), bits(n8)) and torch.equal(bits(e), bits(e8)), width
        dist = float(((r - r8).abs() / r8.abs()).max())
        assert dist <= PRED_BOUND, f"rows of {8 // width} x {width} against 1 x 8: max relative distance {dist:.3g} (bound {PRED_BOUND})"
    # another index0 is another draw; another seed too
    other, t_other = eng.evaluate_batch(x, index0=0)
    seeded, t_seeded = eng.evaluate_batch(x, index0=100, seed=99)
    torch.cuda.synchronize()
    assert not torch.equal(other, r8) and not torch.equal(seeded, r8)
    # ... and the training streams (ids 1 and 2) are not the evaluation streams (3 and 4)
    draw = torch.zeros(8, dtype=torch.int32, device=gpu)
    import gan_class_transfer2_amd as g
    g._lib.call("gct2_rng_uniform_int", eng.rng_seed, 3, 100, draw.data_ptr(), 8, 1, STEPS, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(draw, t8)
    g._lib.call("gct2_rng_normal", eng.rng_seed, 4, 100 * SIZE * SIZE * 3, e8.data_ptr(), e8.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(bits(e8), bits(runs[4][3]))


def test_explicit_timesteps_are_honoured_and_checked(gpu):
    eng = unet(gpu, F32)
    x, = batches(gpu, 1)
    rows3, t = eng.evaluate_batch(x, t=3)
    assert t.tolist() == [3, 3, 3, 3] and t.dtype == torch.int32
    assert_rows(eng, rows3, "mse", "t=3")
    rows, t = eng.evaluate_batch(x, t=[1, 6, 3, 2])
    assert t.tolist() == [1, 6, 3, 2]
    assert_rows(eng, rows, "mse", "t list")
    torch.cuda.synchronize()
    assert bits(rows)[2].item() == bits(rows3)[2].item()        # image 2: the same timestep, the same noise (it belongs to the index)
    eps = torch.randn(4, SIZE, SIZE, 3, generator=torch.Generator().manual_seed(1))
    rows, _ = eng.evaluate_batch(x, t=torch.tensor([2, 2, 5, 5]), eps=eps)
    torch.cuda.synchronize()
    assert torch.equal(eng.last_eval["eps"].cpu(), eps)
    assert_rows(eng, rows, "mse", "injected eps")
    for bad in (0, STEPS + 1, [1, 2, 3], 2.0, [1, 2, 3, True]):
        with pytest.raises(ValueError):
            eng.evaluate_batch(x, t=bad)
    for bad in (dict(index0=-1), dict(eps=eps[:2])):
        with pytest.raises(ValueError):
            eng.evaluate_batch(x, **bad)
    with pytest.raises(ValueError):
        eng.evaluate_batch(x[..., :2])


# ---- 4. the head variants and a table schedule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["timestep_heads", "hidden_dense", "cosine_schedule"])
@pytest.mark.parametrize("make", [unet, variant], ids=["unet", "variant"])
def test_head_variants_and_a_table_schedule(gpu, make, case):
    kw = {case: True} if case != "cosine_schedule" else {}
    eng = make(gpu, F32, predict_x=False, prediction_weighting=True, **kw)
    if case == "cosine_schedule":
        eng.set_noise_schedule("cosine")
    plain = make(gpu, F32, predict_x=False, prediction_weighting=True)
    x, = batches(gpu, 1)
    eng.training_loss = plain.training_loss = "l1"
    rows, t = eng.evaluate_batch(x, index0=8)
    assert_rows(eng, rows, "l1", case)
    ref, t_ref = plain.evaluate_batch(x, index0=8)
    torch.cuda.synchronize()
    assert torch.equal(t, t_ref) and not torch.equal(rows, ref)
    if case == "cosine_schedule":                              # the noised input and the coefficients come from the host's tables
        import gan_class_transfer2_amd as g
        roots = g.trainer_math.alpha_roots("cosine", 0.0, STEPS)
        w = eng.last_eval["coef"][2].cpu().numpy()
        assert np.array_equal(w, roots[1][t.cpu().numpy()])
        assert not torch.equal(bits(eng.last_eval["noised"]), bits(plain.last_eval["noised"]))


# ---- 5. the averaged weights ---------------------------------------------------------------------------------------------------------------
def test_evaluation_on_the_averaged_weights(gpu):
    eng = unet(gpu, F32, use_ema=True, ema_momentum=0.5)
    for x in batches(gpu, 3):
        eng.train_step(x)
    held_out, = batches(gpu, 1, seed=3)
    raw, t = eng.evaluate_batch(held_out)
    with eng.ema_weights():
        avg, t_avg = eng.evaluate_batch(held_out)
        assert_rows(eng, avg, "mse", "ema")
        pred = eng.last_eval["pred"].clone()
        noised = eng.last_eval["noised"][..., :3].clone()
    torch.cuda.synchronize()
    assert torch.equal(t, t_avg) and not torch.equal(raw, avg)
    assert torch.equal(bits(eng.predict(noised, use_ema=True)), bits(pred))
    assert not torch.equal(bits(eng.predict(noised)), bits(pred))


# ---- 6. Trainer.evaluate and fit(validation_data=...) ------------------------------------------------------------------------------------------
@pytest.fixture
def tiny_model():
    """the module-level hyper-parameters of the tiny fp32 network, put back afterwards"""
    import gan_class_transfer2_amd as g
    names = ("size", "pixel_size", "max_size", "octaves", "steps", "compute_dtype", "mixed_precision", "block_depth", "residual", "concat",
             "warm_up", "regularizer", "training_loss")
    keep = {n: getattr(g.model, n) for n in names}
    g.configure(size=SIZE, pixel_size=TOPO[0], max_size=TOPO[1], octaves=TOPO[2], steps=STEPS, compute_dtype="float32", mixed_precision=False,
                block_depth=0, residual=False, concat=True, regularizer=None, training_loss="mse")
    yield g
    g.configure(**keep)


def test_trainer_evaluate_weighs_every_image_alike(gpu, tiny_model):
    g = tiny_model
    tr = g.Trainer(g.Denoiser(seed=3, device=gpu))
    tr.compile(g.Adam(1e-3), g.identity)
    x, = batches(gpu, 1, B=10)
    data = [(x[0:4], x[0:4]), x[4:8], (x[8:10], x[8:10])]       # pairs and bare batches, a partial last one
    out = tr.evaluate(data, return_dict=True)
    eng = tr.denoiser.engine
    assert set(out) == {"loss", "per_image", "t"} and out["per_image"].dtype == np.float32 and out["t"].dtype == np.int32
    assert out["per_image"].shape == out["t"].shape == (10,) and isinstance(out["loss"], float)
    direct = [eng.evaluate_batch(x[a:b], index0=a) for a, b in ((0, 4), (4, 8), (8, 10))]
    torch.cuda.synchronize()
    assert np.array_equal(out["per_image"], torch.cat([r for r, _ in direct]).cpu().numpy())
    assert np.array_equal(out["t"], torch.cat([t for _, t in direct]).cpu().numpy())
    assert out["loss"] == float(np.mean(out["per_image"], dtype=np.float64)) == tr.evaluate(data)
    by_batch = np.mean([out["per_image"][a:b].mean(dtype=np.float64) for a, b in ((0, 4), (4, 8), (8, 10))])
    assert abs(out["loss"] - by_batch) > 1e-9 * out["loss"]    # (not the mean of the batch means)
    two = tr.evaluate(data, steps=2, return_dict=True)
    assert np.array_equal(two["per_image"], out["per_image"][:8])
    fixed = tr.evaluate(data, t=2, return_dict=True)
    assert fixed["t"].tolist() == [2] * 10
    counts, means = g.trainer_math.loss_by_timestep(out["per_image"], out["t"], STEPS)
    assert counts.sum() == 10 and abs(np.nansum(counts * means) / 10 - out["loss"]) <= 1e-12 * out["loss"]
    with pytest.raises(ValueError, match="no batch"):
        tr.evaluate([])
    assert (eng.iterations, eng.rng_offset_t, eng.rng_offset_eps) == (0, 0, 0)
    # the L2 penalty joins `loss`, not `per_image`
    g.configure(regularizer=g.regularizers.l2(1e-3))
    reg = tr.evaluate(data, return_dict=True)
    assert eng.l2 == float(np.float32(1e-3)) and np.array_equal(reg["per_image"], out["per_image"])
    penalty = float(np.float32(1e-3)) * sum(float((v.astype(np.float64) ** 2).sum()) for v in eng.get_params().values())
    assert penalty > 1e-3 * out["loss"]
    assert abs((reg["loss"] - out["loss"]) - penalty) <= 1e-5 * penalty, (reg["loss"], out["loss"], penalty)


def test_fit_with_validation_data(gpu, tiny_model, capsys):
    g = tiny_model
    train = [(x, x) for x in batches(gpu, 8, B=1)]              # (batch 1: see ISOLATION - two trainers are compared bit for bit)
    held_out = [(x, x) for x in batches(gpu, 2, seed=3)] + [batches(gpu, 1, B=2, seed=4)[0]]
    def run(**kw):
        tr = g.Trainer(g.Denoiser(seed=3, device=gpu))
        tr.compile(g.Adam(1e-2), g.identity)
        logs = []
        hist = tr.fit(train, steps_per_epoch=2, epochs=4, callbacks=[g.LambdaCallback(on_epoch_end=lambda e, l: logs.append(dict(l)))], **kw)
        return tr, hist, logs

    tr, hist, logs = run(validation_data=held_out, validation_freq=2)
    printed = capsys.readouterr().out.strip().splitlines()
    _, plain, plain_logs = run()
    plain_printed = capsys.readouterr().out.strip().splitlines()
    assert list(hist) == ["loss", "val_loss"] and len(hist["loss"]) == 4 and len(hist["val_loss"]) == 2
    assert ["val_loss" in l for l in logs] == [False, True, False, True]
    assert [l["val_loss"] for l in logs if "val_loss" in l] == hist["val_loss"]
    assert hist["val_loss"][0] != hist["val_loss"][1] and all(np.isfinite(hist["val_loss"]))
    assert hist["val_loss"][1] == tr.evaluate(held_out)         # the weights as the last epoch left them; the draws are the same
    # without validation_data nothing changes - and with it the training is bit for bit the same
    assert list(plain) == ["loss"] and all(set(l) == {"loss"} for l in plain_logs)
    assert plain["loss"] == hist["loss"]
    assert [("val_loss" in p) for p in printed] == [False, True, False, True] and not any("val_loss" in p for p in plain_printed)
    assert [p.split(" - val_loss")[0] for p in printed] == plain_printed
    every = run(validation_data=held_out, validation_steps=1, validation_use_ema=False)[1]
    assert len(every["val_loss"]) == 4 and every["loss"] == hist["loss"]
