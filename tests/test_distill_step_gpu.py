"""Distiller on the tiny network of tests/test_generate_step_gpu.py (size 16, pixel_size 8, max_size 16, 2 octaves, steps = 6, parameters
of tests/golden/tiny_sampler.npz): the targets against a loop written here from the forward pass and tests/distill_cases.py's
restatement, bit for bit; the student's step against train_step called by hand; the batch cut, the reload, mixed objectives, the
averages, the per-timestep heads, a variant network, the refusals; and that nothing of the teacher moves."""
import types

import numpy as np
import pytest
import torch

import distill_cases as D
from test_generate_step_gpu import F32, SIZE, STEPS, den, lib, same_bits, stream, tiny

pytestmark = pytest.mark.gpu
PER = SIZE * SIZE * 3
MODE = {"x": D.SAMPLE_X, "eps": D.SAMPLE_EPS, "v": D.SAMPLE_V}
SWITCH = {"x": {}, "eps": dict(predict_x=False), "v": dict(predict_v=True)}


def images(gpu, n, seed=4):
    return torch.tensor(np.floor(np.random.default_rng(seed).uniform(0, 256, (n, SIZE, SIZE, 3))) / 128 - 1, dtype=torch.float32, device=gpu)


def trainer_of(eng):
    """what Distiller reads of a compiled Trainer, around an engine built here"""
    return types.SimpleNamespace(denoiser=den(eng), _engine=lambda: eng, optimizer=None)


def student(gpu, **kw):
    eng = tiny(gpu, rng_seed=9, **kw)
    eng.base_lr, eng.warm_up = 1e-2, 0                     # a visible update
    return eng


def kept(tg):
    return {k: v.clone() for k, v in tg.items()}


def hand_targets(eng, x, n, seed, k0, mode, clip=0.0, heads=False):
    """the same targets from the launches the three kernels replace: the pair and the noise drawn at the documented stream positions,
    every pointwise step in numpy (distill_cases), the network through gct2_diffusion_mix(alpha = 0) - which stores z itself - and
    eng.forward.  Returns numpy (xt, et, t, z0)"""
    import gan_class_transfer2_amd as g
    L, T = lib(), g.trainer_math
    B = x.shape[0]
    tab, tt = T.distill_table(T.distill_grid(STEPS, n), STEPS, mode=mode)
    pair = torch.empty(B, dtype=torch.int32, device=x.device)
    eps = torch.empty_like(x)
    L.call("gct2_rng_uniform_int", seed, T.DISTILL_STREAM_PAIR, k0, pair.data_ptr(), B, 1, n, stream())
    L.call("gct2_rng_normal", seed, T.DISTILL_STREAM_EPS, k0 * PER, eps.data_ptr(), B * PER, stream())
    torch.cuda.synchronize()
    pair = pair.cpu().numpy()
    assert pair.min() >= 1 and pair.max() <= n
    rows = tt[pair - 1]
    b = eng.buffers(B, SIZE, SIZE)
    views = (b.img.data_ptr(), 4, eng._slice_ptr(b.R[0], eng.topo.fu(0)), b.ld[0], B * SIZE * SIZE, 3, stream())
    fake = torch.empty_like(x)

    def evaluate(z, t):
        zd = torch.tensor(z.reshape(x.shape), device=x.device)
        L.call("gct2_diffusion_mix", eng.dtype, zd.data_ptr(), zd.data_ptr(), 0.0, fake.data_ptr(), *views)
        if heads:
            b.t_int.copy_(torch.tensor(t, dtype=torch.int32))
        pred = eng.forward(b)
        torch.cuda.synchronize()
        return pred.cpu().numpy().reshape(B, PER)

    flat = lambda t: t.cpu().numpy().reshape(B, PER)
    z0 = D.start_f32(tab, pair, flat(x), flat(eps))
    z1 = D.step_f32(mode, tab, pair, evaluate(z0, rows[:, 0]), z0, clip)
    xt, et, _, _ = D.target_f32(mode, tab, pair, evaluate(z1, rows[:, 1]), z1, z0, clip)
    return xt, et, rows[:, 0], z0


def assert_targets(tg, want, what):
    xt, et, t, z0 = want
    shape = tuple(tg["x"].shape)
    for key, w in (("z", z0), ("x", xt), ("eps", et)):
        assert same_bits(tg[key].cpu(), torch.tensor(w.reshape(shape))), (what, key, float((tg[key].cpu() - torch.tensor(w.reshape(shape))).abs().max()))
    assert tg["t"].cpu().tolist() == [int(v) for v in t], what


@pytest.mark.parametrize("n", [3, 1])
@pytest.mark.parametrize("mode", ["x", "eps"])
def test_targets_equal_the_hand_written_loop(gpu, mode, n):
    """fp32, B = 3 from sample 5: bit for bit the loop written above, with plain launches, with a captured graph and with its replay"""
    import gan_class_transfer2_amd as g
    teacher, stu = tiny(gpu, **SWITCH[mode]), student(gpu)
    x = images(gpu, 3)
    for clip_denoised, clip in ((None, 0.0), (True, 1.0)):
        want = hand_targets(teacher, x, n, 21, 5, MODE[mode], clip)
        assert np.isfinite(want[0]).all() and want[0].std() > 0
        for use_graph in (False, True, True):
            d = g.Distiller(den(teacher), trainer_of(stu), n, seed=21, use_graph=use_graph, clip_denoised=clip_denoised)
            tg = d.targets(x, first_sample=5)
            torch.cuda.synchronize()
            assert_targets(tg, want, (mode, n, clip, use_graph))
            assert d.next_sample == 0                       # (targets never moves the position)
    assert len(teacher._forward_graphs) == 1


def test_targets_set_the_timestep_of_every_image(gpu):
    """per-timestep heads: t and t' of every image reach the head kernels - against the loop that sets them by hand"""
    import gan_class_transfer2_amd as g
    teacher = g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS, seed=4, timestep_heads=True)
    stu = g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS, seed=4, timestep_heads=True, rng_seed=9)
    x = images(gpu, 4)
    want = hand_targets(teacher, x, 3, 7, 0, D.SAMPLE_X, heads=True)
    assert len(set(want[2].tolist())) > 1                   # more than one timestep in the batch
    wrong = hand_targets(teacher, x, 3, 7, 0, D.SAMPLE_X, heads=False)      # (whatever t_int held: not the per-image rows)
    assert not np.array_equal(want[0], wrong[0])
    for use_graph in (False, True, True):
        d = g.Distiller(den(teacher), trainer_of(stu), 3, seed=7, use_graph=use_graph)
        tg = d.targets(x)
        torch.cuda.synchronize()
        assert_targets(tg, want, use_graph)
    loss = d.step(x)                                        # the student's own heads read t through its train_step
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()


def _params_equal(a, b):
    pa, pb = a.get_params(), b.get_params()
    return all(np.array_equal(pa[k].view(np.int32), pb[k].view(np.int32)) for k in pa)


@pytest.mark.parametrize("pairing", [("x", "x"), ("eps", "v")], ids=["x_to_x", "eps_to_v"])
def test_step_is_the_students_own_train_step(gpu, pairing):
    """Distiller.step against train_step(x~, t_int=t, eps=eps~) called by hand on a second identical student: the loss bits and every
    parameter; an eps teacher trains a v student through the same path.  The teacher's state dictionary, RNG positions and step counter
    do not move"""
    import gan_class_transfer2_amd as g
    t_mode, s_mode = pairing
    teacher = tiny(gpu, **SWITCH[t_mode])
    A, Bn = student(gpu, **SWITCH[s_mode]), student(gpu, **SWITCH[s_mode])
    x = images(gpu, 4)
    before = teacher.state_dict()
    state = (teacher.rng_offset_t, teacher.rng_offset_eps, teacher.iterations)
    d = g.Distiller(den(teacher), trainer_of(A), 3, seed=3)
    ref = g.Distiller(den(teacher), trainer_of(Bn), 3, seed=3)
    for k in range(3):
        # (batch 1: at this tiny topology gct2_dense_bwd adds its partial sums with float atomics, so two engines are bit-equal in every
        # parameter at batch 1 only - DESIGN.md, noise schedules - whoever calls their train_step)
        loss = d.step(x[k:k + 1]).clone()
        torch.cuda.synchronize()
        tg = kept(ref.targets(x[k:k + 1], first_sample=k))
        by_hand = Bn.train_step(tg["x"], t_int=tg["t"], eps=tg["eps"]).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(by_hand).all() and same_bits(loss, by_hand), (pairing, k)
        assert _params_equal(A, Bn), (pairing, k)
    assert d.next_sample == 3 and ref.next_sample == 0 and A.iterations == Bn.iterations == 3
    assert not _params_equal(A, student(gpu, **SWITCH[s_mode]))             # (the steps did move the student)
    after = teacher.state_dict()
    assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert (teacher.rng_offset_t, teacher.rng_offset_eps, teacher.iterations) == state


def test_targets_do_not_depend_on_the_batch_cut_and_reload(gpu):
    """four samples at B = 4 equal two batches at B = 2; another seed gives other targets; a Distiller reloaded from state_dict()
    continues bit for bit (and so does the student reloaded from its own)"""
    import gan_class_transfer2_amd as g
    teacher = tiny(gpu, predict_x=False)
    A, Bn = student(gpu), student(gpu)
    x = images(gpu, 4)
    d = g.Distiller(den(teacher), trainer_of(A), 3, seed=11, clip_denoised=True)
    whole = kept(d.targets(x))
    lo, hi = kept(d.targets(x[:2])), kept(d.targets(x[2:], first_sample=2))
    other = kept(g.Distiller(den(teacher), trainer_of(A), 3, seed=12, clip_denoised=True).targets(x))
    torch.cuda.synchronize()
    for key in ("x", "eps", "t", "z"):
        assert torch.equal(whole[key], torch.cat([lo[key], hi[key]])), key
    assert not torch.equal(whole["z"], other["z"])
    # the teacher's clip bounds the targets of pair 1, which are its x0 estimates themselves (the other pairs' are solved from clipped ones)
    first = kept(d.targets(x, pair=torch.tensor([1, 1, 2, 3], dtype=torch.int32)))
    assert first["t"].cpu().tolist() == [2, 2, 4, 6] and float(first["x"][:2].abs().max()) <= 1.0
    d.step(x[:1])                                                            # (batch 1: two engines are bit-equal in every parameter there only)
    d.step(x[1:2])
    sd = d.state_dict()
    assert sd == {"seed": 11, "next_sample": 2, "student_steps": 3}
    Bn.load_state_dict(A.state_dict())
    d2 = g.Distiller(den(teacher), trainer_of(Bn), 3, seed=99, clip_denoised=True)
    d2.load_state_dict(sd)
    la = d.step(x[2:3]).clone()
    torch.cuda.synchronize()
    lb = d2.step(x[2:3]).clone()
    torch.cuda.synchronize()
    assert same_bits(la, lb) and _params_equal(A, Bn) and d.state_dict() == d2.state_dict()
    with pytest.raises(ValueError):
        g.Distiller(den(teacher), trainer_of(Bn), 1).load_state_dict(sd)


def test_teacher_reads_its_averages(gpu):
    import gan_class_transfer2_amd as g
    raw, avg, stu = tiny(gpu, use_ema=True, ema_momentum=0.5), tiny(gpu), student(gpu)
    x = images(gpu, 2)
    raw.base_lr, raw.warm_up = 1e-2, 0
    raw.train_step(x)
    avg.set_params({k: raw.arena._view(raw.arena.ema, k).clone() for k in raw.arena.shapes})
    torch.cuda.synchronize()
    kw = dict(seed=5)
    got_raw = kept(g.Distiller(den(raw), trainer_of(stu), 3, **kw).targets(x))
    got_avg = kept(g.Distiller(den(raw), trainer_of(stu), 3, teacher_use_ema=True, **kw).targets(x))
    want_avg = kept(g.Distiller(den(avg), trainer_of(stu), 3, **kw).targets(x))
    torch.cuda.synchronize()
    assert same_bits(got_avg["x"], want_avg["x"]) and same_bits(got_avg["eps"], want_avg["eps"])
    assert same_bits(got_raw["z"], got_avg["z"]) and not torch.equal(got_raw["x"], got_avg["x"])


def test_distills_a_variant_network(gpu):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.variants import VariantEngine
    make = lambda **kw: VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4, predict_x=False, **kw)
    teacher, stu = make(), make(rng_seed=9)
    x = images(gpu, 4)
    d = g.Distiller(den(teacher), trainer_of(stu), 3, seed=2, clip_denoised=True)
    whole = kept(d.targets(x))
    lo, hi = kept(d.targets(x[:2])), kept(d.targets(x[2:], first_sample=2))
    torch.cuda.synchronize()
    assert torch.isfinite(whole["x"]).all() and torch.isfinite(whole["eps"]).all() and float(whole["x"].std()) > 0
    assert all(torch.equal(whole[k], torch.cat([lo[k], hi[k]])) for k in whole)
    loss = d.step(x)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and d.next_sample == 4


def test_variant_with_timestep_heads_reads_the_per_image_timesteps(gpu):
    """a variant network with per-timestep heads: the device-resident t / t' of every image reach its head kernels - against the loop
    that hands VariantEngine.predict the same timesteps as a host list"""
    import gan_class_transfer2_amd as g
    import gan_class_transfer2_amd.trainer_math as T
    from gan_class_transfer2_amd.variants import VariantEngine
    make = lambda **kw: VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4, timestep_heads=True, **kw)
    teacher, stu = make(), make(rng_seed=9)
    x = images(gpu, 4)
    d = g.Distiller(den(teacher), trainer_of(stu), 3, seed=6)
    tg = kept(d.targets(x))
    torch.cuda.synchronize()
    tab, tt = T.distill_table(T.distill_grid(STEPS, 3), STEPS, mode=D.SAMPLE_X)
    pair = torch.empty(4, dtype=torch.int32, device=gpu)
    eps = torch.empty_like(x)
    lib().call("gct2_rng_uniform_int", 6, T.DISTILL_STREAM_PAIR, 0, pair.data_ptr(), 4, 1, 3, stream())
    lib().call("gct2_rng_normal", 6, T.DISTILL_STREAM_EPS, 0, eps.data_ptr(), 4 * PER, stream())
    torch.cuda.synchronize()
    pair = pair.cpu().numpy()
    rows = tt[pair - 1]
    assert len(set(rows[:, 0].tolist())) > 1
    flat = lambda t: t.detach().cpu().numpy().reshape(4, PER)
    evaluate = lambda z, t: flat(teacher.predict(torch.tensor(z.reshape(x.shape), device=gpu), [int(v) for v in t]))
    z0 = D.start_f32(tab, pair, flat(x), flat(eps))
    z1 = D.step_f32(D.SAMPLE_X, tab, pair, evaluate(z0, rows[:, 0]), z0, 0.0)
    xt, et, _, _ = D.target_f32(D.SAMPLE_X, tab, pair, evaluate(z1, rows[:, 1]), z1, z0, 0.0)
    assert_targets(tg, (xt, et, rows[:, 0], z0), "variant with heads")
    swapped = D.target_f32(D.SAMPLE_X, tab, pair, evaluate(z1, rows[:, 0]), z1, z0, 0.0)[0]       # (t in the place of t': other heads)
    assert not np.array_equal(swapped, xt)
    loss = d.step(x)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()


@pytest.fixture
def tiny_model():
    """the module-level hyper-parameters of the reference script set to the tiny configuration, restored afterwards"""
    import gan_class_transfer2_amd as g
    names = ("size", "pixel_size", "max_size", "octaves", "steps", "compute_dtype", "mixed_precision", "block_depth", "residual", "concat",
             "warm_up", "regularizer", "training_loss", "predict_x", "predict_scaled_epsilon", "prediction_weighting",
             "ordinary_differential_equation", "predict_v", "loss_weighting", "min_snr_gamma", "noise_schedule", "alpha_dash_offset",
             "timestep_heads", "hidden_dense")
    keep = {n: getattr(g.model, n) for n in names}
    g.configure(size=SIZE, pixel_size=8, max_size=16, octaves=2, steps=STEPS, compute_dtype="float32", mixed_precision=False,
                block_depth=0, residual=False, concat=True, warm_up=0, regularizer=None, training_loss="mse", predict_x=True,
                predict_scaled_epsilon=False, prediction_weighting=False, ordinary_differential_equation=False, predict_v=False,
                loss_weighting=None, min_snr_gamma=5.0, noise_schedule="quadratic", alpha_dash_offset=0.0, timestep_heads=False,
                hidden_dense=False)
    yield g
    g.configure(**keep)


def _arena_equal(a, b):
    return bool(torch.equal(a.arena.p.view(torch.int32), b.arena.p.view(torch.int32)))


@pytest.mark.parametrize("optimizer", ["sgd", "loss_scaled_adam"])
def test_clone_denoiser_copies_the_weights_alone(gpu, tiny_model, optimizer):
    """a teacher trained under SGD with momentum, or under a loss-scaled Adam (neither is what a fresh Denoiser's engine runs): the
    clone holds its weights bit for bit; optimizer slots, step counter and RNG positions are a fresh engine's; the teacher is untouched"""
    g = tiny_model
    teacher = g.Denoiser(seed=3, device=gpu)
    tr = g.Trainer(teacher)
    opt = g.SGD(1e-2, momentum=0.9) if optimizer == "sgd" else g.LossScaleOptimizer(g.Adam(1e-3))
    tr.compile(opt, g.identity)
    x = images(gpu, 2)
    for _ in range(2):
        tr.train_step((x, x))
    teng = teacher.engine
    assert teng.iterations == 2 and (teng.optimizer_kind == "sgd" or teng.ls_state is not None)
    before = teng.state_dict()
    student = g.clone_denoiser(teacher)
    seng = student.engine
    torch.cuda.synchronize()
    assert student is not teacher and seng is not teng and _arena_equal(seng, teng)
    assert seng.iterations == 0 and (seng.rng_offset_t, seng.rng_offset_eps) == (0, 0)
    assert float(seng.arena.m.abs().max()) == 0.0 and float(seng.arena.v.abs().max()) == 0.0
    after = teng.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    # the clone trains under an optimizer of its own
    st = g.Trainer(student)
    st.compile(g.Adam(1e-3), g.identity)
    d = g.Distiller(teacher, st, 3, seed=1)
    loss = d.step(x)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and seng.iterations == 1 and not _arena_equal(seng, teng)


def test_fit_and_progressive_distill(gpu, tiny_model):
    """Distiller.fit with a callback (two epochs of two steps), then progressive_distill from 4 sampling steps to 1: two rounds, each
    student a clone of its teacher; the first teacher does not move and the result is sampled with generate(num_steps=1)"""
    import itertools
    g = tiny_model
    teacher = g.Denoiser(seed=3, device=gpu)
    teacher.ensure_engine()
    start = teacher.engine.arena.p.clone()
    x = images(gpu, 2)
    data = itertools.cycle([(x, x)])
    student = g.clone_denoiser(teacher)
    tr = g.Trainer(student)
    tr.compile(g.Adam(1e-3), g.identity)
    seen = []
    d = g.Distiller(teacher, tr, 3, seed=2)
    history = d.fit(data, steps_per_epoch=2, epochs=2, verbose=0,
                    callbacks=[g.LambdaCallback(on_epoch_begin=lambda e, logs: seen.append(("begin", e)),
                                                on_epoch_end=lambda e, logs: seen.append(("end", e, logs["loss"])))])
    assert len(history["loss"]) == 2 and np.isfinite(history["loss"]).all() and d.next_sample == 8
    assert [s[:2] for s in seen] == [("begin", 0), ("end", 0), ("begin", 1), ("end", 1)] and [s[2] for s in seen if s[0] == "end"] == history["loss"]
    assert student.engine.iterations == 4
    made = []

    def make_optimizer():
        made.append(g.Adam(1e-3))
        return made[-1]

    last = g.progressive_distill(teacher, data, 4, 1, 3, make_optimizer, seed=5, verbose=0)
    torch.cuda.synchronize()
    assert len(made) == 2 and last is not teacher and last.engine.iterations == 3
    assert torch.equal(teacher.engine.arena.p, start) and not torch.equal(last.engine.arena.p, start)
    out = g.generate(last, 2, num_steps=1, size=SIZE)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, SIZE, SIZE, 3) and torch.isfinite(out).all()
    for bad in ((4, 3), (6, 4), (4, 4), (2, 4), (4, 0)):
        with pytest.raises(ValueError):
            g.progressive_distill(teacher, data, bad[0], bad[1], 1, make_optimizer)


def test_refusals(gpu):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.distributed import DataParallelStep
    teacher, stu = tiny(gpu), student(gpu)
    ok = lambda **kw: g.Distiller(den(teacher), trainer_of(stu), 3, **kw)
    ok()
    bad = [lambda: ok(clip_denoised="dynamic"), lambda: ok(clip_denoised=-1.0), lambda: ok(clip_denoised=float("inf")),
           lambda: g.Distiller(den(teacher), trainer_of(stu), 4),                                   # 2 N > steps
           lambda: g.Distiller(den(teacher), trainer_of(stu), 0),
           lambda: ok(timesteps=[1, 2, 3]), lambda: ok(timesteps=[1, 2, 3, 3, 5, 6]),
           lambda: g.Distiller(den(teacher), trainer_of(teacher), 3),                               # one engine on both sides
           lambda: g.Distiller(den(tiny(gpu, predict_x=False, ordinary_differential_equation=True)), trainer_of(stu), 3),
           lambda: g.Distiller(den(teacher), trainer_of(student(gpu, predict_x=False, ordinary_differential_equation=True)), 3)]
    same = den(teacher)
    bad.append(lambda: g.Distiller(same, types.SimpleNamespace(denoiser=same, _engine=lambda: stu, optimizer=None), 3))
    other_steps = g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=8, seed=4)
    bad.append(lambda: g.Distiller(den(teacher), trainer_of(other_steps), 3))
    cosine = student(gpu)
    cosine.set_noise_schedule("cosine", 0.0)
    bad.append(lambda: g.Distiller(den(teacher), trainer_of(cosine), 3))
    shifted = student(gpu)
    shifted.set_noise_schedule("quadratic", 1e-4)
    bad.append(lambda: g.Distiller(den(teacher), trainer_of(shifted), 3))
    wrapped = student(gpu)
    wrapper = DataParallelStep(wrapped)
    bad.append(lambda: g.Distiller(den(teacher), trainer_of(wrapped), 3))
    bad.append(lambda: g.Distiller(den(teacher), wrapper, 3))
    for k, make in enumerate(bad):
        with pytest.raises(ValueError):
            make()
            pytest.fail(f"refusal {k} did not raise")
    d = ok()
    for args in ((torch.zeros(2, SIZE, SIZE, 4, device=gpu),), (torch.zeros(SIZE, SIZE, 3, device=gpu),)):
        with pytest.raises(ValueError):
            d.targets(*args)
    x = images(gpu, 2)
    with pytest.raises(ValueError):
        d.targets(x, pair=torch.ones(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        d.targets(x, eps=torch.zeros(2, SIZE, SIZE, 1))
    with pytest.raises(ValueError):
        d.targets(x, first_sample=-1)


def test_the_student_learns_a_pinned_batch(gpu):
    """pair= and eps= pin one batch, so the targets are one fixed pseudo batch: the student's distillation loss after 30 of its own
    steps on it is below its first (a condition, not a measured threshold)"""
    import gan_class_transfer2_amd as g
    teacher, stu = tiny(gpu), student(gpu)
    stu.base_lr = 1e-3
    x = images(gpu, 4)
    gen = torch.Generator().manual_seed(13)
    eps = torch.randn(4, SIZE, SIZE, 3, generator=gen).to(gpu)
    pair = torch.tensor([3, 1, 2, 3], dtype=torch.int32, device=gpu)
    d = g.Distiller(den(teacher), trainer_of(stu), 3, seed=1)
    tg = kept(d.targets(x, pair=pair, eps=eps))
    again = kept(d.targets(x, pair=pair, eps=eps))
    drawn = kept(d.targets(x))
    torch.cuda.synchronize()
    assert all(torch.equal(tg[k], again[k]) for k in tg) and not torch.equal(tg["z"], drawn["z"])
    assert tg["t"].cpu().tolist() == [6, 2, 4, 6]
    losses = [float(stu.train_step(tg["x"], t_int=tg["t"], eps=tg["eps"])[0]) for _ in range(30)]
    print(f"pinned batch: loss {losses[0]:.6g} -> {losses[-1]:.6g}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
