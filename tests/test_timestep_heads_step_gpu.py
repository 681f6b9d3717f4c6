"""Per-timestep heads (train.py:199, 203, 211-214) through the engines, the model mirror and the sampler, on the GPU.

The CPU references are plain torch / numpy in float64 on the engine's own stored tensors (R_0, dpred): the head is the last layer, so
its forward and its kernel / bias gradients can be restated exactly from what the step leaves in its buffers.  Tolerance of a summed
quantity: the standard fp32 summation bound n 2^-24 sum |x dy| over its n terms - derived, not tuned.  The tiny network is the one
tests/test_sampler_gpu.py uses (pixel_size 8, max_size 16, 2 octaves, 16 x 16 images, 6 steps)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
STEPS, SIZE = 6, 16
TINY = (8, 16, 2)                        # pixel_size, max_size, octaves: Fu_0 = 4, the head reads 7 channels (ld 8)


def tiny(gpu, dtype=F32, heads=True, **kw):
    import gan_class_transfer2_amd as g
    kw = dict(dict(steps=STEPS, seed=3, rng_seed=5, base_lr=1e-3, warm_up=0), **kw)
    if heads is not None:
        kw["timestep_heads"] = heads
    return g.UNetEngine(g.Topology(*TINY), dtype, gpu, **kw)


def batch(gpu, B, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randint(0, 256, (B, SIZE, SIZE, 3), generator=gen).float() / 128 - 1).to(gpu)
    eps = torch.randn(B, SIZE, SIZE, 3, generator=gen)
    return x, eps


def bits(t):
    return t.contiguous().view(torch.int32)


def head_reference(eng, b, t_list):
    """(per-slice float64 R_0^T dpred [cin, steps, 3], its bias row sums [steps, 3], the per-entry bounds of both) from the buffers"""
    cin = eng.topo.fu(0) + 3
    B, hw = b.B, b.H * b.W
    r0 = b.R[0][..., :cin].double().cpu().reshape(B, hw, cin)
    dp = b.dpred.double().cpu().reshape(B, hw, 3)
    if eng.dtype == F16:
        dp = b.dpred.half().double().cpu().reshape(B, hw, 3)          # the gradient entering a mixed_float16 Dense output is fp16
    dw, db = torch.zeros(cin, eng.steps, 3, dtype=torch.float64), torch.zeros(eng.steps, 3, dtype=torch.float64)
    bw, bb = torch.zeros_like(dw), torch.zeros_like(db)
    for s in set(v - 1 for v in t_list):
        imgs = [i for i, v in enumerate(t_list) if v - 1 == s]
        n = len(imgs) * hw
        for i in imgs:
            dw[:, s] += r0[i].T @ dp[i]
            db[s] += dp[i].sum(0)
            bw[:, s] += r0[i].abs().T @ dp[i].abs()
            bb[s] += dp[i].abs().sum(0)
        bw[:, s] *= n * 2.0 ** -24
        bb[s] *= n * 2.0 ** -24
    return dw, db, bw, bb


def test_constructor_shapes_and_init(gpu):
    import math
    eng = tiny(gpu)
    A = eng.arena
    assert eng.timestep_heads and not eng.fused_head_ok()
    assert A.shapes["dense.w"] == (7, 3 * STEPS) and A.shapes["dense.b"] == (3 * STEPS,)
    w, bz = A.param("dense.w"), A.param("dense.b")
    lim = math.sqrt(6.0 / (7 + 3 * STEPS))
    assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.8 * lim and bool((bz == 0).all())
    # everything that walks the arena by tensor sees the larger head: named state, clipping and L2 segments
    nsd = eng.named_state_dict()
    assert tuple(nsd["p/dense.w"].shape) == (7, 3 * STEPS) and tuple(nsd["m/dense.b"].shape) == (3 * STEPS,)
    segs = dict(eng._clip_segments())
    assert segs[A.offsets["dense.w"]] == 7 * 3 * STEPS and segs[A.offsets["dense.b"]] == 3 * STEPS
    plain = tiny(gpu, heads=False)
    assert not plain.timestep_heads and plain.arena.shapes["dense.w"] == (7, 3)


@pytest.mark.parametrize("s", [1, STEPS])
def test_equal_timesteps_reduce_to_the_plain_head(gpu, s):
    """F32, the tiny network, three images at one timestep s: the loss, the prediction, dR_0 and every gradient but the head's equal
    the plain engine's on slice s - 1 BIT FOR BIT.  Both engines run their fp32 convolutions on the matrix cores (f32_matrix): the
    direct fp32 weight-gradient kernel splits its 192 rows over three work-groups here and adds them with float atomics, so two runs
    of ONE engine already differ in the last bit there (three addends, any order); the matrix-core kernels sum in a fixed order.
    The head kernels are the same in both modes."""
    on, off = tiny(gpu, f32_matrix=True), tiny(gpu, heads=False, f32_matrix=True)
    params = on.get_params()
    plain = {k: v for k, v in params.items() if not k.startswith("dense.")}
    plain["dense.w"] = params["dense.w"][:, 3 * (s - 1):3 * s].copy()
    bias = np.linspace(-0.5, 0.5, 3 * STEPS).astype(np.float32)              # (a non-zero bias: the slice of b must be the right one too)
    on.set_params({"dense.b": bias})
    plain["dense.b"] = bias[3 * (s - 1):3 * s].copy()
    off.set_params(plain)
    x, eps = batch(gpu, 3)
    t = torch.tensor([s, s, s], dtype=torch.int32)
    l_on = on.train_step(x, t, eps, apply=False).clone()
    l_off = off.train_step(x, t, eps, apply=False).clone()
    torch.cuda.synchronize()
    b_on, b_off = on.buffers(3, SIZE, SIZE), off.buffers(3, SIZE, SIZE)
    assert torch.equal(bits(l_on), bits(l_off)) and torch.equal(bits(b_on.pred), bits(b_off.pred))
    assert torch.equal(bits(b_on.dR[0]), bits(b_off.dR[0]))
    g_on, g_off = on.get_grads(), off.get_grads()
    for k in g_off:
        if not k.startswith("dense."):
            assert np.array_equal(g_on[k].view(np.int32), g_off[k].view(np.int32)), k
    dw, db, bw, bb = head_reference(on, b_on, [s, s, s])
    gw = torch.tensor(g_on["dense.w"]).double().view(7, STEPS, 3)
    gb = torch.tensor(g_on["dense.b"]).double().view(STEPS, 3)
    assert bool(((gw[:, s - 1] - torch.tensor(g_off["dense.w"]).double()).abs() <= bw[:, s - 1]).all())
    assert bool(((gb[s - 1] - torch.tensor(g_off["dense.b"]).double()).abs() <= bb[s - 1]).all())
    others = [q for q in range(STEPS) if q != s - 1]
    assert bool((gw[:, others] == 0).all()) and bool((gb[others] == 0).all())


def test_mixed_timesteps_head_gradient_against_float64(gpu, parity_log):
    eng = tiny(gpu)
    eng.set_params({"dense.b": np.linspace(-0.5, 0.5, 3 * STEPS).astype(np.float32)})
    x, eps = batch(gpu, 4, seed=1)
    tl = [1, STEPS, 1, min(3, STEPS)]
    eng.train_step(x, torch.tensor(tl, dtype=torch.int32), eps, apply=False)
    torch.cuda.synchronize()
    b = eng.buffers(4, SIZE, SIZE)
    # the forward head on the stored R_0, per image on its own slice
    W, bias = eng.arena.param("dense.w").double().cpu().view(7, STEPS, 3), eng.arena.param("dense.b").double().cpu().view(STEPS, 3)
    r0 = b.R[0][..., :7].double().cpu()
    pred = torch.stack([r0[i] @ W[:, v - 1] + bias[v - 1] for i, v in enumerate(tl)])
    perr = float((b.pred.double().cpu() - pred).abs().max())
    assert perr <= 8 * 2.0 ** -24 * float((r0.abs().reshape(-1, 7) @ W.abs().reshape(7, -1)).max() + bias.abs().max())
    dw, db, bw, bb = head_reference(eng, b, tl)
    g = eng.get_grads()
    gw, gb = torch.tensor(g["dense.w"]).double().view(7, STEPS, 3), torch.tensor(g["dense.b"]).double().view(STEPS, 3)
    ew, eb = (gw - dw).abs(), (gb - db).abs()
    sel = sorted(set(v - 1 for v in tl))
    parity_log("timestep_heads_mixed_f32", pred_max_abs_err=perr, dw_worst_err_over_bound=float((ew[:, sel] / bw[:, sel]).max()),
               db_worst_err_over_bound=float((eb[sel] / bb[sel]).max()), dw_max_abs_err=float(ew.max()))
    assert bool((ew <= bw).all()) and bool((eb <= bb).all())             # (unselected slices: bound 0, the gradient exactly 0)
    unsel = [q for q in range(STEPS) if q not in sel]
    assert bool((bits(torch.tensor(g["dense.w"]).view(7, STEPS, 3)[:, unsel]) == 0).all())


def test_one_applied_step_moves_only_the_selected_slices(gpu):
    eng = tiny(gpu)
    x, eps = batch(gpu, 4, seed=2)
    tl = [1, STEPS, 1, 3]
    w0, b0 = eng.arena.param("dense.w").clone().view(7, STEPS, 3), eng.arena.param("dense.b").clone().view(STEPS, 3)
    eng.train_step(x, torch.tensor(tl, dtype=torch.int32), eps, apply=True)
    torch.cuda.synchronize()
    assert eng.iterations == 1
    w1, b1 = eng.arena.param("dense.w").view(7, STEPS, 3), eng.arena.param("dense.b").view(STEPS, 3)
    for q in range(STEPS):
        if q + 1 in tl:
            assert not torch.equal(w1[:, q], w0[:, q]) and not torch.equal(b1[q], b0[q]), q
        else:
            assert torch.equal(bits(w1[:, q]), bits(w0[:, q])) and torch.equal(bits(b1[q]), bits(b0[q])), q


def test_planned_steps_equal_eager_steps(gpu):
    """4 steps from one seed, replayed from a step plan (recorded at the second step) and run call by call: the same losses and
    parameters, bit for bit.  Batch 2: no sum of this step then has more than two addends that meet in a float atomic (the direct
    fp32 weight-gradient kernel splits 128 rows over two work-groups, the bias column sums fit one), so the bits depend on the inputs
    alone and an unequal bit is the plan's."""
    xs = [batch(gpu, 2, seed=k)[0] for k in range(4)]
    out = []
    for use_plan in (False, True):
        eng = tiny(gpu)
        eng.use_plan = use_plan
        losses = [eng.train_step(xs[k]).clone() for k in range(4)]
        torch.cuda.synchronize()
        assert bool(eng._plans) == use_plan and eng.iterations == 4
        out.append((torch.cat(losses), eng.arena.p.clone()))
    assert torch.equal(bits(out[0][0]), bits(out[1][0])), (out[0][0], out[1][0])
    assert torch.equal(bits(out[0][1]), bits(out[1][1]))


def test_switch_off_is_the_engine_without_the_argument(gpu):
    """timestep_heads=False passed explicitly and an engine built without the argument: the same bits after 4 steps (reference width,
    bf16: the fused matrix-core head - no kernel of this step adds with atomics)"""
    import gan_class_transfer2_amd as g
    gen = torch.Generator().manual_seed(4)
    xs = [(torch.randint(0, 256, (4, 16, 16, 3), generator=gen).float() / 128 - 1).to(gpu) for _ in range(4)]
    res = []
    for kw in (dict(timestep_heads=False), dict()):
        eng = g.UNetEngine(g.Topology(128, 256, 2), BF16, gpu, steps=STEPS, seed=3, rng_seed=5, **kw)
        assert eng.fused_head_ok() and not eng.timestep_heads
        losses = [eng.train_step(x).clone() for x in xs]
        torch.cuda.synchronize()
        res.append((torch.cat(losses), {n: getattr(eng.arena, n).clone() for n in ("p", "m", "v", "shadow")}, sorted(eng.state_dict())))
    assert torch.equal(bits(res[0][0]), bits(res[1][0])) and res[0][2] == res[1][2] and "timestep_heads" not in res[0][2]
    for n in ("p", "m", "v"):
        assert torch.equal(bits(res[0][1][n]), bits(res[1][1][n])), n
    assert torch.equal(res[0][1]["shadow"].view(torch.int16), res[1][1]["shadow"].view(torch.int16))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_sixteen_bit_step_runs_on_the_non_fused_path(gpu, dtype, parity_log):
    """reference width (Fu_0 = 64: a plain engine takes the fused head there), F16 with dynamic loss scaling.  The loss against a
    float64 evaluation of the gathered head on the stored R_0: 4e-3 relative, the kernel tolerance tests/test_step_gpu.py holds the
    16-bit head's stored outputs to (test_config3_full_batch_layer_local_vs_oracle: "U0.fwd+head.pred")."""
    import gan_class_transfer2_amd as g
    topo = g.Topology(128, 256, 2)
    kw = dict(steps=STEPS, seed=3, rng_seed=5, loss_scaling=(dtype == F16))
    assert g.UNetEngine(topo, dtype, gpu, **kw).fused_head_ok()
    eng = g.UNetEngine(topo, dtype, gpu, timestep_heads=True, **kw)
    assert not eng.fused_head_ok()
    x, _ = batch(gpu, 4, seed=6)
    eng.ctx.log_launches(True); eng.ctx_tail.log_launches(True)
    loss = eng.train_step(x, apply=False).clone()               # (t_int from the engine's own RNG; the parameters stay what the pass read)
    torch.cuda.synchronize()
    log = eng.read_launch_log()
    eng.ctx.log_launches(False); eng.ctx_tail.log_launches(False)
    assert log.count("dense_steps:fwd") == 1 and log.count("dense_steps:bwd") == 1 and not any(t.startswith("halo:convT:head") for t in log), log
    b = eng.buffers(4, SIZE, SIZE)
    tl = b.t_int.cpu().tolist()
    assert all(1 <= v <= STEPS for v in tl)
    cin = 67
    W, bias = eng.arena.param("dense.w").double().cpu().view(cin, STEPS, 3), eng.arena.param("dense.b").double().cpu().view(STEPS, 3)
    r0 = b.R[0][..., :cin].double().cpu()
    pred = torch.stack([r0[i] @ W[:, v - 1] + bias[v - 1] for i, v in enumerate(tl)])
    want = float(((pred - x.double().cpu()) ** 2).mean())
    got = float(loss[0])
    parity_log(f"timestep_heads_step_{'bf16' if dtype == BF16 else 'f16'}", loss=got, loss_float64_head=want, rel=abs(got - want) / want)
    assert np.isfinite(got) and abs(got - want) <= 4e-3 * want, (got, want)
    assert np.isfinite(eng.get_grads()["dense.w"]).all()


def _heads_return_t(eng, set_params):
    cin = eng.head_cin if hasattr(eng, "head_cin") else eng.topo.fu(0) + 3
    set_params({"dense.w": np.zeros((cin, 3 * STEPS), dtype=np.float32),
                "dense.b": np.repeat(np.arange(1, STEPS + 1, dtype=np.float32), 3)})


def _sampler_inputs(gpu):
    gen = torch.Generator().manual_seed(8)
    image = (torch.rand(1, SIZE, SIZE, 3, generator=gen) * 2 - 1).to(gpu)
    example = torch.randn(1, 2, SIZE, SIZE, 3, generator=gen).to(gpu)
    dictionary = torch.randn(SIZE, SIZE, 4, 3, generator=gen).to(gpu)
    return image, example, dictionary


def _check_sampler_saw_t(res, test_step):
    want = {"denoised": test_step, "step_1": STEPS, "step_0.25": STEPS // 4, "step_0.5": 2 * STEPS // 4, "step_0.75": 3 * STEPS // 4, "fake": 1}
    for k, v in want.items():
        assert bool((res[k] == float(v)).all()), (k, v, float(res[k].min()), float(res[k].max()))


@pytest.mark.parametrize("use_graph", [True, False])
def test_sampler_passes_the_timestep_of_every_evaluation(gpu, use_graph):
    """dense.w = 0 and dense.b[3 s + c] = s + 1: the network returns t.  predict_x: x_theta is the prediction, so the images
    log_sample keeps are the timesteps at which it kept them"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu)
    _heads_return_t(eng, eng.set_params)
    den = types.SimpleNamespace(ensure_engine=lambda: eng)
    res = g.log_sample(den, *_sampler_inputs(gpu), steps=STEPS, test_step=2, use_graph=use_graph)
    torch.cuda.synchronize()
    _check_sampler_saw_t(res, 2)
    if use_graph:
        assert len(eng._forward_graphs) >= 2                               # batch 1 and batch 6 were replayed from their captures


def test_sampler_passes_the_timestep_on_a_variant_network(gpu):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.variants import VariantEngine
    eng = VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4, timestep_heads=True)
    assert eng.shapes["dense.w"] == (eng.head_cin, 3 * STEPS)
    _heads_return_t(eng, eng.set_params)
    den = types.SimpleNamespace(ensure_engine=lambda: eng)
    res = g.log_sample(den, *_sampler_inputs(gpu), steps=STEPS, test_step=3)
    torch.cuda.synchronize()
    _check_sampler_saw_t(res, 3)


def test_variant_engine_step_against_float64(gpu):
    """block_depth = 1: one step with mixed timesteps; the head's kernel / bias gradients against float64 on the stored head input"""
    from gan_class_transfer2_amd.variants import VariantEngine
    eng = VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4, timestep_heads=True)
    x, eps = batch(gpu, 4, seed=9)
    tl = [1, STEPS, 1, 3]
    loss = eng.train_step(x, torch.tensor(tl, dtype=torch.int32), eps, apply=False)
    torch.cuda.synchronize()
    g = eng.get_grads()
    assert np.isfinite(float(loss[0])) and all(np.isfinite(v).all() for v in g.values())
    gw = torch.tensor(g["dense.w"]).view(eng.head_cin, STEPS, 3)
    for q in range(STEPS):
        assert bool((gw[:, q] != 0).any()) == (q + 1 in tl), q
    assert float(np.abs(g["D0.w"]).max()) > 0                              # the input gradient of the gathered head reached the network


def test_predict_needs_valid_timesteps(gpu):
    eng = tiny(gpu)
    x = torch.randn(2, SIZE, SIZE, 3, device=gpu)
    for bad in (dict(), dict(t=0), dict(t=STEPS + 1), dict(t=[1, 2, 3]), dict(t=1.0)):
        with pytest.raises(ValueError):
            eng.predict(x, **bad)
    _heads_return_t(eng, eng.set_params)
    y = eng.predict(x, t=[2, 5])
    torch.cuda.synchronize()
    assert bool((y[0] == 2).all()) and bool((y[1] == 5).all())
    assert bool((eng.predict(x, 4) == 4).all())
    # without the switch t is accepted and ignored, as ever
    plain = tiny(gpu, heads=False)
    assert torch.equal(plain.predict(x, t=3).clone(), plain.predict(x))


def test_data_parallel_wrappers_refuse_the_switch(gpu):
    from gan_class_transfer2_amd import distributed as D
    for wrapper in (D.DataParallelStep, D.ShardedDataParallelStep):
        with pytest.raises(ValueError, match="per-timestep heads"):
            wrapper(tiny(gpu))


def test_checkpoints_of_the_other_head_shape_are_refused(gpu):
    on, off = tiny(gpu), tiny(gpu, heads=False)
    before = on.arena.p.clone()
    with pytest.raises(ValueError, match="Dense"):
        on.load_state_dict(off.state_dict())
    with pytest.raises(ValueError, match="Dense"):
        off.load_state_dict(on.state_dict())
    with pytest.raises(ValueError):
        on.load_named_state_dict(off.named_state_dict())
    assert torch.equal(on.arena.p, before)                                  # nothing was loaded, not even a prefix
    twin = tiny(gpu, seed=9)
    twin.load_state_dict(on.state_dict())                                   # the same shape loads
    assert torch.equal(twin.arena.p, on.arena.p)


def test_model_mirror_call_and_eager_call_use_t(gpu):
    import gan_class_transfer2_amd as g
    M = g.model
    g.configure(size=SIZE, pixel_size=8, max_size=16, octaves=2, steps=STEPS, compute_dtype="float32", timestep_heads=True)
    try:
        den = g.Denoiser(seed=3)
        assert den.head.units == 3 * STEPS
        eng = den.ensure_engine()
        assert eng.timestep_heads and eng.steps == STEPS
        x = torch.randn(2, SIZE, SIZE, 3, device=gpu)
        t = torch.tensor([2, 5], dtype=torch.int32, device=gpu).view(2, 1, 1, 1)          # Trainer.call's shape
        planned, eager = den((x, t)), den.call_eager((x, t))
        torch.cuda.synchronize()
        assert planned.shape == (2, SIZE, SIZE, 3) and float((planned - eager).abs().max()) <= 1e-5 * float(planned.abs().max())
        one = den((x, torch.tensor([5])))                                                    # log_sample's [1]: broadcast over the batch
        assert torch.equal(one[1], planned[1]) and not torch.equal(one[0], planned[0])
        with pytest.raises(ValueError):
            den((x, torch.tensor([0])))
        tr = g.Trainer(den)
        assert float(tr(x)) > 0                                                              # Trainer.call: t_int from the engine's RNG
        M.configure(timestep_heads=False)
        with pytest.raises(ValueError, match="timestep_heads"):
            tr.train_step((x, x))
    finally:
        g.configure(size=256, pixel_size=128, max_size=512, octaves=6, steps=200, compute_dtype=None, timestep_heads=False)
