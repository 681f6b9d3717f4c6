"""The hidden Dense(pixel_size, relu) layer in front of the head (train.py:195-197) through the engines, the model mirror and the
sampler, on the GPU.

The CPU references are plain torch in float64 on the engine's own stored tensors (R_0, dpred), the method of
tests/test_timestep_heads_step_gpu.py: the two layers are the last ones, so their forward and all of their gradients can be restated from
what the step leaves in its buffers.  h and dh are rounded to the compute dtype where the kernels round them.  fp32 tolerances: that
file's - 8 2^-24 sum |terms| for the prediction (and, here, for dR_0: sums over the 8 hidden units of the tiny network), n 2^-24
sum |x dy| for a gradient summed over n pixels - derived, not tuned; 16-bit steps: its 4e-3 relative bound on the loss.  The tiny network
is tests/test_sampler_gpu.py's (pixel_size 8, max_size 16, 2 octaves, 16 x 16 images, 6 steps): Fu_0 = 4, the hidden layer is 7 -> 8."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
STEPS, SIZE = 6, 16
TINY = (8, 16, 2)


def tiny(gpu, dtype=F32, hidden=True, **kw):
    import gan_class_transfer2_amd as g
    kw = dict(dict(steps=STEPS, seed=3, rng_seed=5, base_lr=1e-3, warm_up=0), **kw)
    if hidden is not None:
        kw["hidden_dense"] = hidden
    return g.UNetEngine(g.Topology(*TINY), dtype, gpu, **kw)


def batch(gpu, B, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randint(0, 256, (B, SIZE, SIZE, 3), generator=gen).float() / 128 - 1).to(gpu)
    eps = torch.randn(B, SIZE, SIZE, 3, generator=gen)
    return x, eps


def bits(t):
    return t.contiguous().view(torch.int32)


def rnd(t, dtype):
    return t.to(TD[dtype]).double()


def head_float64(r0, w1, b1, w2, b2, dtype):
    """(h, prediction) of the two layers in float64 on [.., cin] rows, h rounded once to the compute dtype"""
    h = rnd(torch.clamp(r0 @ w1 + b1, min=0.0), dtype)
    return h, h @ w2 + b2


def engine_head_reference(eng, b):
    """everything the two layers produce, in float64, from the engine's stored R_0 and dpred (and their per-entry fp32 bounds)"""
    cin, fu = eng.topo.fu(0) + 3, eng.topo.fu(0)
    A, dt = eng.arena, eng.dtype
    w1 = (A.param("dense_hidden.w") if dt == F32 else A.shadow[A.offsets["dense_hidden.w"]:][:A.numel("dense_hidden.w")].view(A.shapes["dense_hidden.w"])).double().cpu()
    b1, w2, b2 = (A.param(k).double().cpu() for k in ("dense_hidden.b", "dense.w", "dense.b"))
    r0 = b.R[0][..., :cin].double().cpu().reshape(-1, cin)
    dp = (b.dpred.half() if dt == F16 else b.dpred).double().cpu().reshape(-1, 3)
    n = r0.shape[0]
    h, pred = head_float64(r0, w1, b1, w2, b2, dt)
    dh = rnd((h > 0) * (dp @ w2.T), dt)
    e = 2.0 ** -24
    out = dict(pred=pred, dw2=h.T @ dp, db2=dp.sum(0), dw1=r0.T @ dh, db1=dh.sum(0), dr0=((r0 > 0) * (dh @ w1.T))[:, :fu])
    chid = w1.shape[1]
    bound = dict(pred=chid * e * (h.abs() @ w2.abs() + b2.abs()), dw2=n * e * (h.abs().T @ dp.abs()), db2=n * e * dp.abs().sum(0),
                 dw1=n * e * (r0.abs().T @ dh.abs()), db1=n * e * dh.abs().sum(0), dr0=(chid * e * (dh.abs() @ w1.abs().T))[:, :fu])
    return out, bound, h


def engine_head_results(eng, b):
    g = eng.get_grads()
    fu = eng.topo.fu(0)
    T = lambda a: torch.tensor(a).double()
    return dict(pred=b.pred.double().cpu().reshape(-1, 3), dw2=T(g["dense.w"]), db2=T(g["dense.b"]), dw1=T(g["dense_hidden.w"]),
                db1=T(g["dense_hidden.b"]), dr0=b.dR[0][..., :fu].double().cpu().reshape(-1, fu))


def test_constructor_shapes_and_init(gpu):
    import math
    eng = tiny(gpu)
    A = eng.arena
    assert eng.hidden_dense and not eng.fused_head_ok()
    assert A.shapes["dense_hidden.w"] == (7, 8) and A.shapes["dense_hidden.b"] == (8,) and A.shapes["dense.w"] == (8, 3) and A.shapes["dense.b"] == (3,)
    for name, lim in (("dense_hidden.w", math.sqrt(6.0 / (7 + 8))), ("dense.w", math.sqrt(6.0 / (8 + 3)))):
        w = A.param(name)
        assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.7 * lim, name
    assert bool((A.param("dense_hidden.b") == 0).all()) and bool((A.param("dense.b") == 0).all())
    lo, hi = A.layer_ranges["dense"]
    assert all(lo <= A.offsets[k] < hi for k in ("dense_hidden.w", "dense_hidden.b", "dense.w", "dense.b"))
    # everything that walks the arena by tensor sees the two new tensors: named state, clipping and L2 segments
    nsd = eng.named_state_dict()
    assert tuple(nsd["p/dense_hidden.w"].shape) == (7, 8) and tuple(nsd["m/dense_hidden.b"].shape) == (8,) and "hidden_dense" in nsd
    segs, l2 = dict(eng._clip_segments()), dict(eng._l2_segments())
    for k, n in (("dense_hidden.w", 56), ("dense_hidden.b", 8), ("dense.w", 24)):
        assert segs[A.offsets[k]] == n and l2[A.offsets[k]] == n, k      # both new tensors carry the regularizer, like every other pair
    # the other tensors of the network are what the plain engine draws
    plain = tiny(gpu, hidden=False)
    assert not plain.hidden_dense and plain.arena.shapes["dense.w"] == (7, 3) and "dense_hidden.w" not in plain.arena.shapes
    for k in plain.arena.shapes:
        if not k.startswith("dense"):
            assert torch.equal(plain.arena.param(k), A.param(k)), k


def test_predict_and_one_step_against_float64_fp32(gpu, parity_log):
    eng = tiny(gpu)
    eng.set_params({"dense_hidden.b": np.linspace(-0.3, 0.3, 8).astype(np.float32), "dense.b": np.array([-0.5, 0.1, 0.5], dtype=np.float32)})
    eng.ctx.log_launches(True)
    x, eps = batch(gpu, 2, seed=1)
    loss = eng.train_step(x, torch.tensor([1, STEPS], dtype=torch.int32), eps, apply=False).clone()
    torch.cuda.synchronize()
    log = eng.read_launch_log()
    eng.ctx.log_launches(False)
    assert log.count("dense2:fwd:plain") == 1 and log.count("dense2:bwd:plain") == 1, log
    b = eng.buffers(2, SIZE, SIZE)
    ref, bound, h = engine_head_reference(eng, b)
    assert 0.2 < float((h > 0).double().mean()) < 0.8                     # the ReLU of the hidden layer masks a real share of the units
    got = engine_head_results(eng, b)
    worst = {k: float(((got[k] - ref[k]).abs() / bound[k].clamp_min(1e-300)).max()) for k in ref}
    want_loss = float(((ref["pred"] - x.double().cpu().reshape(-1, 3)) ** 2).mean())
    parity_log("hidden_dense_step_f32", loss=float(loss[0]), loss_float64_head=want_loss, **{k + "_err_over_bound": v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    assert abs(float(loss[0]) - want_loss) <= 1e-5 * want_loss
    assert float(got["dr0"].abs().max()) > 0 and float(np.abs(eng.get_grads()["D0.w"]).max()) > 0       # the input gradient reached the network
    # predict: the same two layers on the R_0 the forward pass leaves
    noised = torch.randn(2, SIZE, SIZE, 3, device=gpu)
    y = eng.predict(noised).clone()
    torch.cuda.synchronize()
    ref, bound, _ = engine_head_reference(eng, b)
    assert bool(((y.double().cpu().reshape(-1, 3) - ref["pred"]).abs() <= bound["pred"]).all())


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("width", ["tiny", "reference"])
def test_sixteen_bit_step_against_float64(gpu, dtype, width, parity_log):
    """F16 with dynamic loss scaling.  Reference width (pixel_size 128, Fu_0 = 64: a plain engine takes the fused head there): the
    matrix-core kernels run inside the step - proved by the launch log; the tiny network (Chid = 8) takes the plain ones."""
    import gan_class_transfer2_amd as g
    topo = g.Topology(128, 256, 2) if width == "reference" else g.Topology(*TINY)
    kw = dict(steps=STEPS, seed=3, rng_seed=5, loss_scaling=(dtype == F16))
    if width == "reference":
        assert g.UNetEngine(topo, dtype, gpu, **kw).fused_head_ok()
    eng = g.UNetEngine(topo, dtype, gpu, hidden_dense=True, **kw)
    assert not eng.fused_head_ok()
    x, _ = batch(gpu, 2, seed=6)
    eng.ctx.log_launches(True); eng.ctx_tail.log_launches(True)
    loss = eng.train_step(x, apply=False).clone()
    torch.cuda.synchronize()
    log = eng.read_launch_log()
    eng.ctx.log_launches(False); eng.ctx_tail.log_launches(False)
    path = "mfma" if width == "reference" else "plain"
    assert log.count(f"dense2:fwd:{path}") == 1 and log.count(f"dense2:bwd:{path}") == 1 and not any(t.startswith("halo:convT:head") for t in log), log
    b = eng.buffers(2, SIZE, SIZE)
    ref, _, h = engine_head_reference(eng, b)
    want = float(((ref["pred"] - x.double().cpu().reshape(-1, 3)) ** 2).mean())
    got = float(loss[0])
    res = engine_head_results(eng, b)
    rel = {k: float((res[k] - ref[k]).norm() / ref[k].norm().clamp_min(1e-300)) for k in ("dw2", "db2", "dw1", "db1", "dr0")}
    parity_log(f"hidden_dense_step_{'bf16' if dtype == BF16 else 'f16'}_{width}", loss=got, loss_float64_head=want, rel=abs(got - want) / want,
               **{k + "_rel_l2": v for k, v in rel.items()})
    assert np.isfinite(got) and abs(got - want) <= 4e-3 * want, (got, want)
    assert all(np.isfinite(v).all() for v in eng.get_grads().values())
    # the gradients of the two layers against float64 on the stored tensors (dpred carries the loss scale in both): the same 4e-3,
    # relative to the tensor's norm (one rounding of h / dh to 8 or 11 significant bits per term, summed over hundreds of terms)
    assert all(v <= 4e-3 for v in rel.values()), rel


def test_planned_steps_equal_eager_steps_and_all_four_tensors_move(gpu):
    """5 steps from one seed, the last ones replayed from a step plan (a step shape is recorded the second time it is seen, and the
    first step - nothing held back yet - is a shape of its own), and run call by call: the same losses and parameters, bit for bit
    (f32_matrix, batch 2: no kernel of this step then adds more than two partial sums with float atomics)."""
    xs = [batch(gpu, 2, seed=k)[0] for k in range(5)]
    out = []
    for use_plan in (False, True):
        eng = tiny(gpu, f32_matrix=True)
        eng.use_plan = use_plan
        p0 = {k: eng.arena.param(k).clone() for k in ("dense_hidden.w", "dense_hidden.b", "dense.w", "dense.b")}
        losses = [eng.train_step(xs[0]).clone()]
        torch.cuda.synchronize()
        for k, v in p0.items():
            assert not torch.equal(eng.arena.param(k), v), k               # one applied step: all four head tensors have moved
        losses += [eng.train_step(xs[k]).clone() for k in (1, 2, 3, 4)]
        torch.cuda.synchronize()
        assert bool(eng._plans) == use_plan and eng.iterations == 5
        out.append((torch.cat(losses), eng.arena.p.clone()))
    assert torch.equal(bits(out[0][0]), bits(out[1][0])), (out[0][0], out[1][0])
    assert torch.equal(bits(out[0][1]), bits(out[1][1]))


def test_planned_bf16_steps_with_deferred_adam_equal_eager_steps(gpu):
    """the reference width in bf16 (the matrix-core head kernels, fused per-layer Adam, defer_adam): planned = eager, bit for bit"""
    import gan_class_transfer2_amd as g
    xs = [batch(gpu, 2, seed=k)[0] for k in range(5)]
    out = []
    for use_plan in (False, True):
        eng = g.UNetEngine(g.Topology(128, 256, 2), BF16, gpu, steps=STEPS, seed=3, rng_seed=5, hidden_dense=True)
        assert eng.defer_adam
        eng.use_plan = use_plan
        losses = [eng.train_step(x).clone() for x in xs]
        torch.cuda.synchronize()
        assert bool(eng._plans) == use_plan
        out.append((torch.cat(losses), eng.arena.p.clone(), eng.arena.shadow.clone()))
    assert torch.equal(bits(out[0][0]), bits(out[1][0])) and torch.equal(bits(out[0][1]), bits(out[1][1]))
    assert torch.equal(out[0][2].view(torch.int16), out[1][2].view(torch.int16))


def test_switch_off_is_the_engine_without_the_argument(gpu):
    import gan_class_transfer2_amd as g
    gen = torch.Generator().manual_seed(4)
    xs = [(torch.randint(0, 256, (4, 16, 16, 3), generator=gen).float() / 128 - 1).to(gpu) for _ in range(3)]
    res = []
    for kw in (dict(hidden_dense=False, head_initializer="glorot_uniform"), dict()):
        eng = g.UNetEngine(g.Topology(128, 256, 2), BF16, gpu, steps=STEPS, seed=3, rng_seed=5, **kw)
        assert eng.fused_head_ok() and not eng.hidden_dense
        losses = [eng.train_step(x).clone() for x in xs]
        torch.cuda.synchronize()
        res.append((torch.cat(losses), {n: getattr(eng.arena, n).clone() for n in ("p", "m", "v", "shadow")}, sorted(eng.state_dict()),
                    dict(eng.arena.offsets)))
    assert torch.equal(bits(res[0][0]), bits(res[1][0])) and res[0][2] == res[1][2] and "hidden_dense" not in res[0][2] and res[0][3] == res[1][3]
    for n in ("p", "m", "v"):
        assert torch.equal(bits(res[0][1][n]), bits(res[1][1][n])), n
    assert torch.equal(res[0][1]["shadow"].view(torch.int16), res[1][1]["shadow"].view(torch.int16))


def test_every_training_loss_runs_one_finite_step(gpu):
    from gan_class_transfer2_amd.trainer_math import TRAINING_LOSSES
    x, _ = batch(gpu, 2, seed=2)
    for kind in TRAINING_LOSSES:
        eng = tiny(gpu)
        eng.training_loss = kind
        w0 = eng.arena.param("dense_hidden.w").clone()
        loss = eng.train_step(x)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss[0])) and float(loss[0]) > 0, kind
        assert not torch.equal(eng.arena.param("dense_hidden.w"), w0) and bool(torch.isfinite(eng.arena.p).all()), kind


@pytest.mark.parametrize("what", ["use_ema", "global_clipnorm", "sgd", "l2", "weighted_objective"])
def test_optimizer_side_options_move_the_hidden_kernel(gpu, what):
    eng = tiny(gpu, use_ema=True) if what == "use_ema" else tiny(gpu, **(dict(predict_x=False, prediction_weighting=True) if what == "weighted_objective" else {}))
    if what == "global_clipnorm":
        eng.set_clipping(global_clipnorm=0.5)
    elif what == "sgd":
        eng.set_optimizer("sgd", momentum=0.9)
    elif what == "l2":
        eng.set_regularizer(1e-3)
    x, _ = batch(gpu, 2, seed=3)
    w0 = eng.arena.param("dense_hidden.w").clone()
    loss = eng.train_step(x)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss[0])) and eng.iterations == 1
    w1 = eng.arena.param("dense_hidden.w")
    assert not torch.equal(w1, w0) and bool(torch.isfinite(eng.arena.p).all())
    if what == "use_ema":
        o, n = eng.arena.offsets["dense_hidden.w"], eng.arena.numel("dense_hidden.w")
        ema = eng.arena.ema[o:o + n].view(7, 8)
        m = eng.ema_momentum
        assert float((ema - (m * w0 + (1 - m) * w1)).abs().max()) <= 1e-6


def _sampler_inputs(gpu):
    gen = torch.Generator().manual_seed(8)
    image = (torch.rand(1, SIZE, SIZE, 3, generator=gen) * 2 - 1).to(gpu)
    example = torch.randn(1, 2, SIZE, SIZE, 3, generator=gen).to(gpu)
    dictionary = torch.randn(SIZE, SIZE, 4, 3, generator=gen).to(gpu)
    return image, example, dictionary


def test_log_sample_with_and_without_the_graph(gpu):
    import gan_class_transfer2_amd as g
    eng = tiny(gpu)
    den = types.SimpleNamespace(ensure_engine=lambda: eng)
    res = [g.log_sample(den, *_sampler_inputs(gpu), steps=STEPS, test_step=2, use_graph=ug) for ug in (True, False)]
    torch.cuda.synchronize()
    assert len(eng._forward_graphs) >= 2
    assert set(res[0]) == set(res[1])
    for k in res[0]:
        assert bool(torch.isfinite(res[0][k]).all()) and torch.equal(res[0][k], res[1][k]), k


def test_variant_engine_step_against_float64(gpu, parity_log):
    """block_depth = 1: the variant engine composes the pair from the launches it is defined by (a 1 x 1 convolution with ReLU, then
    the head).  One step; prediction, loss and the four head gradients against float64 on the stored input of the hidden layer.  The
    gradient bounds add what the prediction's own error (<= its bound) contributes through dpred = 2 (pred - x) / N."""
    from gan_class_transfer2_amd.variants import VariantEngine
    eng = VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4, hidden_dense=True)
    cin = eng.head_cin
    assert cin == 8 and eng.shapes["dense_hidden.w"] == (eng.shapes["blkTopB.0.w"][-1], 8) and eng.shapes["dense.w"] == (8, 3)
    hid = eng.top.nodes[-2]
    keep = {}
    fwd0 = hid.fwd
    hid.fwd = lambda xin: keep.setdefault("x", xin.clone()) is None or fwd0(xin)
    x, eps = batch(gpu, 2, seed=9)
    loss = eng.train_step(x, torch.tensor([1, STEPS], dtype=torch.int32), eps, apply=False).clone()
    torch.cuda.synchronize()
    g = eng.get_grads()
    assert np.isfinite(float(loss[0])) and all(np.isfinite(v).all() for v in g.values())
    P = {k: torch.tensor(v).double() for k, v in eng.get_params().items()}
    xin = keep["x"].double().cpu().reshape(-1, keep["x"].shape[-1])
    n = xin.shape[0]
    h, pred = head_float64(xin, P["dense_hidden.w"], P["dense_hidden.b"], P["dense.w"], P["dense.b"], F32)
    e = 2.0 ** -24
    he = 8 * e * (xin.abs() @ P["dense_hidden.w"].abs() + P["dense_hidden.b"].abs())      # h's own error: an fp32 sum of 8 products
    pb = 8 * e * (h.abs() @ P["dense.w"].abs() + P["dense.b"].abs()) + he @ P["dense.w"].abs()
    got_pred = eng.last["pred"].double().cpu().reshape(-1, 3)
    assert bool(((got_pred - pred).abs() <= pb).all())
    xt = x.double().cpu().reshape(-1, 3)
    want = float(((pred - xt) ** 2).mean())
    assert abs(float(loss[0]) - want) <= 1e-5 * want
    dp = 2 * (pred - xt) / (n * 3)
    dpe = 2 * pb / (n * 3) + dp.abs() * 2 * e                            # dpred's own error: the prediction's, and its fp32 rounding
    dh = (h > 0) * (dp @ P["dense.w"].T)
    dhe = dpe @ P["dense.w"].abs().T + 4 * e * (dp.abs() @ P["dense.w"].abs().T)
    ref = {"dense.w": h.T @ dp, "dense.b": dp.sum(0), "dense_hidden.w": xin.T @ dh, "dense_hidden.b": dh.sum(0)}
    bnd = {"dense.w": n * e * (h.abs().T @ dp.abs()) + h.abs().T @ dpe + he.T @ dp.abs(), "dense.b": n * e * dp.abs().sum(0) + dpe.sum(0),
           "dense_hidden.w": n * e * (xin.abs().T @ dh.abs()) + xin.abs().T @ dhe, "dense_hidden.b": n * e * dh.abs().sum(0) + dhe.sum(0)}
    worst = {k: float(((torch.tensor(g[k]).double() - ref[k]).abs() / bnd[k].clamp_min(1e-300)).max()) for k in ref}
    parity_log("hidden_dense_variant_f32", loss=float(loss[0]), loss_float64_head=want, **{k + "_err_over_bound": v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    assert float(np.abs(g["D0.w"]).max()) > 0                              # the input gradient of the pair reached the network


def test_refusals(gpu):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import distributed as D
    from gan_class_transfer2_amd.variants import VariantEngine
    for wrapper in (D.DataParallelStep, D.ShardedDataParallelStep):
        with pytest.raises(ValueError, match=wrapper.__name__ + ".*hidden_dense"):
            wrapper(tiny(gpu))
    with pytest.raises(ValueError, match="hidden_dense.*timestep_heads"):
        tiny(gpu, timestep_heads=True)
    with pytest.raises(ValueError, match="hidden_dense.*timestep_heads"):
        VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, hidden_dense=True, timestep_heads=True)
    with pytest.raises(ValueError, match="head_initializer"):
        tiny(gpu, head_initializer="ones")


def test_checkpoints_round_trip_and_the_other_shape_is_refused(gpu):
    on, off = tiny(gpu), tiny(gpu, hidden=False)
    x, _ = batch(gpu, 2, seed=5)
    on.train_step(x)
    torch.cuda.synchronize()
    sd = on.state_dict()
    assert int(sd["hidden_dense"][0]) == 8 and "hidden_dense" not in off.state_dict()
    twin = tiny(gpu, seed=9)
    twin.load_state_dict(sd)
    for n in ("p", "m", "v"):
        assert torch.equal(getattr(twin.arena, n), getattr(on.arena, n)), n
    assert twin.iterations == 1
    l_on, l_twin = on.train_step(x).clone(), twin.train_step(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(bits(l_on), bits(l_twin))
    named = tiny(gpu, seed=11)
    named.load_named_state_dict(on.named_state_dict())
    assert torch.equal(named.arena.p, on.arena.p)
    before = on.arena.p.clone()
    with pytest.raises(ValueError, match="hidden Dense"):
        on.load_state_dict(off.state_dict())
    with pytest.raises(ValueError, match="hidden Dense"):
        off.load_state_dict(on.state_dict())
    with pytest.raises(ValueError):
        on.load_named_state_dict(off.named_state_dict())
    assert torch.equal(on.arena.p, before)                                  # nothing was loaded, not even a prefix


def test_zero_head_initializer_predicts_the_bias(gpu):
    from gan_class_transfer2_amd.variants import VariantEngine
    bias = np.array([0.25, -0.5, 0.75], dtype=np.float32)
    noised = torch.randn(2, SIZE, SIZE, 3, device=gpu)
    for hidden in (True, False):
        eng, ref = tiny(gpu, hidden=hidden, head_initializer="zeros"), tiny(gpu, hidden=hidden)
        assert bool((eng.arena.param("dense.w") == 0).all()) and bool((ref.arena.param("dense.w") != 0).any())
        for k in ref.arena.shapes:
            if k != "dense.w":
                assert torch.equal(eng.arena.param(k), ref.arena.param(k)), k        # every other tensor draws what it would have drawn
        eng.set_params({"dense.b": bias})
        y = eng.predict(noised)
        torch.cuda.synchronize()
        assert bool((y == torch.tensor(bias, device=gpu)).all()), hidden
    var = VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4, hidden_dense=True, head_initializer="zeros")
    assert bool((torch.tensor(var.get_params()["dense.w"]) == 0).all())
    var.set_params({"dense.b": bias})
    assert bool((var.predict(noised) == torch.tensor(bias, device=gpu)).all())


def test_model_mirror_call_eager_call_and_trainer(gpu):
    import gan_class_transfer2_amd as g
    M = g.model
    g.configure(size=SIZE, pixel_size=8, max_size=16, octaves=2, steps=STEPS, compute_dtype="float32", hidden_dense=True)
    try:
        den = g.Denoiser(seed=3)
        assert den.hidden is not None and den.hidden.units == 8 and den.hidden.activation == "relu" and den.head.units == 3
        eng = den.ensure_engine()
        assert eng.hidden_dense and den.hidden.kernel.shape == (7, 8) and den.head.kernel.shape == (8, 3)
        x = torch.randn(2, SIZE, SIZE, 3, device=gpu)
        t = torch.tensor([2, 5], dtype=torch.int32, device=gpu).view(2, 1, 1, 1)
        planned, eager = den((x, t)), den.call_eager((x, t))
        torch.cuda.synchronize()
        assert planned.shape == (2, SIZE, SIZE, 3) and float((planned - eager).abs().max()) <= 1e-5 * float(planned.abs().max())
        assert set(den.trainable_variables) >= {"dense_hidden.w", "dense_hidden.b"}
        tr = g.Trainer(den)
        assert float(tr(x)) > 0
        M.configure(hidden_dense=False)
        with pytest.raises(ValueError, match="hidden_dense"):
            tr.train_step((x, x))
        M.configure(hidden_dense=True, timestep_heads=True)
        with pytest.raises(ValueError, match="hidden_dense.*timestep_heads"):
            g.Denoiser(seed=3)
        # a variant network: the nested eager layers run the hidden layer too
        M.configure(timestep_heads=False, block_depth=1)
        den = g.Denoiser(seed=3)
        eng = den.ensure_engine()
        assert eng.hidden_dense and den.hidden.kernel.shape == eng.shapes["dense_hidden.w"]
        planned, eager = den((x, t)), den.call_eager((x, t))
        torch.cuda.synchronize()
        assert float((planned - eager).abs().max()) <= 1e-5 * float(planned.abs().max())
    finally:
        g.configure(size=256, pixel_size=128, max_size=512, octaves=6, steps=200, compute_dtype=None, hidden_dense=False, timestep_heads=False,
                    block_depth=0)
