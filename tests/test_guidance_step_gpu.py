"""generate(guide=...) on the tiny network of tests/test_generate_step_gpu.py (size 16, steps = 6, parameters of
tests/golden/tiny_sampler.npz) with a guide whose parameters are the golden ones under a fixed-seed perturbation: against a loop written
here from the two forward passes and the float32 restatement of tests/guidance_cases.py, bit for bit; the weights 1 and 0; the interval
and where the guide is evaluated; the split run and the batch cut; dynamic thresholding under guidance; the other networks; that the
default launches none of the new entry points; that no training state of either denoiser moves; and the refusals."""
import numpy as np
import pytest
import torch

import dynamic_cases as D
import guidance_cases as GC
from test_generate_step_gpu import GOLDEN, SIZE, STEPS, F32, _state, den, lib, noise, same_bits, tiny
from test_img2img_step_gpu import alpha, half_plane, images, views
from test_multistep_step_gpu import inject

pytestmark = pytest.mark.gpu
PER = SIZE * SIZE * 3
NEW = ("gct2_x0_quantile_guided", "gct2_diffusion_step_guided")
OLD_STEPS = ("gct2_diffusion_step", "gct2_diffusion_step_masked", "gct2_diffusion_step_multistep", "gct2_diffusion_step_dynamic")
OBJECTIVES = {"x": {}, "eps": dict(predict_x=False), "scaled_eps": dict(predict_x=False, predict_scaled_epsilon=True), "v": dict(predict_v=True)}
MODE_OF = dict(zip(("x", "eps", "scaled_eps", "v"), GC.MODES))
TABLE = [3.0, 1.0, 0.5, 2.0, 1.0, 1.5]                 # w(t) at index t - 1: guided and unguided timesteps, above and below 1


def guide_of(gpu, **kw):
    """a second tiny engine: the golden parameters under guidance_cases.perturbed"""
    import gan_class_transfer2_amd as g
    z = np.load(GOLDEN)
    eng = g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS, **kw)
    eng.set_params(GC.perturbed({k[6:]: z[k] for k in z.files if k.startswith("param/")}))
    return eng


def forward(eng, b, v, state, shape):
    inject(eng, v, state.reshape(shape))
    pred = eng.forward(b)
    torch.cuda.synchronize()
    return pred.cpu().numpy().reshape(shape[0], PER)


def generate_by_hand(eng, geng, z, taus, mode, weights, solver="ddim", dynamic=None, clip=0.0):
    """generate(guide=, noise=z) at eta = 0: per step the main forward pass, the guide's where w != 1, then the restatement of the
    (guided) select and of the guided step on the host.  dynamic: (percentile, floor).  Returns the last estimate, {timestep: estimate},
    {timestep: s [n]} and the timesteps at which the guide ran"""
    import gan_class_transfer2_amd as g
    n, K = z.shape[0], len(taus)
    (b, v), (gb, gv) = views(eng, n), views(geng, n)
    state, hist, estimates, bounds, guided_at = z.cpu().numpy().reshape(n, PER), None, {}, {}, []
    for k in range(K):
        tau = taus[K - 1 - k]
        a_t, a_prev = alpha(tau), alpha(taus[K - 2 - k] if k < K - 1 else 0)
        c1 = None if solver == "ddim" else (0.0 if k in (0, K - 1) else g.multistep_coefficient(alpha(taus[K - k]), a_t, a_prev))
        w = weights[tau - 1]
        pm = forward(eng, b, v, state, z.shape)
        pg = forward(geng, gb, gv, state, z.shape) if w != 1.0 else None
        if pg is not None:
            guided_at.append(tau)
        rows = None
        if dynamic is not None:
            p = pm if pg is None else GC.combine_f32(pm, pg, w)
            rows, _ = D.select_f32(mode, p, state, a_t, D.quantile_rank(dynamic[0], PER), dynamic[1])
            bounds[tau] = torch.tensor(rows[:, 0]).to(z.device)
        state, x0, hist = GC.guided_step_f32(mode, pm, pg, w, state, a_t, a_prev, rows=rows, clip=clip, hist=hist, c1=c1)
        estimates[tau] = torch.tensor(x0.reshape(z.shape)).to(z.device)
    return estimates[taus[0]], estimates, bounds, guided_at


@pytest.mark.parametrize("solver", ["ddim", "dpm2m"])
@pytest.mark.parametrize("objective", list(OBJECTIVES))
def test_generate_equals_the_hand_loop(gpu, objective, solver):
    """fp32, a given starting noise, a table of weights with guided and unguided timesteps: bit for bit the hand-written loop, with plain
    launches and with graph replay (each network replays its own capture), return_steps included; and it is neither network's own run"""
    import gan_class_transfer2_amd as g
    sw = OBJECTIVES[objective]
    eng, geng = tiny(gpu, **sw), guide_of(gpu, **sw)
    z = noise(gpu, 2)
    for num_steps in (6, 3):
        taus = g.sampling_timesteps(STEPS, num_steps)
        want, estimates, _, guided_at = generate_by_hand(eng, geng, z, taus, MODE_OF[objective], TABLE, solver)
        assert torch.isfinite(want).all() and float(want.std()) > 0 and 0 < len(guided_at) < num_steps
        kw = dict(num_steps=num_steps, noise=z, solver=solver, guide=den(geng), guidance_scale=TABLE, **sw)
        for use_graph in (False, True, True):                   # (the second graph run replays the captures of the first)
            got = g.generate(den(eng), 2, use_graph=use_graph, **kw)
            torch.cuda.synchronize()
            assert same_bits(got, want), (objective, solver, num_steps, use_graph, float((got - want).abs().max()))
        got, kept = g.generate(den(eng), 2, return_steps=(taus[-1], taus[0]), **kw)
        torch.cuda.synchronize()
        assert same_bits(got, want) and all(same_bits(kept[t], estimates[t]) for t in kept) and set(kept) == {taus[-1], taus[0]}
        base = dict(num_steps=num_steps, noise=z, solver=solver, **sw)
        assert not torch.equal(want, g.generate(den(eng), 2, **base)) and not torch.equal(want, g.generate(den(geng), 2, **base))
    assert len(eng._forward_graphs) == 1 and len(geng._forward_graphs) == 1


@pytest.mark.parametrize("solver", ["ddim", "dpm2m"])
def test_weights_one_and_zero(gpu, solver):
    """guidance_scale = 1.0 is guide=None bit for bit; a weight of 0 is the guide's own generate bit for bit - from drawn noise with a
    clip, and with init + mask"""
    import gan_class_transfer2_amd as g
    eng, geng = tiny(gpu, predict_x=False), guide_of(gpu, predict_x=False)
    init = images(gpu, 3)
    for kw in (dict(size=SIZE, seed=3, clip_denoised=True), dict(init=init, mask=half_plane(gpu), seed=4)) + \
            ((dict(size=SIZE, seed=5, eta=0.7),) if solver == "ddim" else ()):
        kw = dict(kw, num_steps=4, predict_x=False, solver=solver, batch_size=2)
        main, other = g.generate(den(eng), 3, **kw), g.generate(den(geng), 3, **kw)
        one = g.generate(den(eng), 3, guide=den(geng), guidance_scale=1.0, **kw)
        zero = g.generate(den(eng), 3, guide=den(geng), guidance_scale=0.0, **kw)
        mid = g.generate(den(eng), 3, guide=den(geng), guidance_scale=2.0, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(main).all() and torch.isfinite(other).all() and not torch.equal(main, other)
        assert same_bits(one, main), sorted(kw)
        assert same_bits(zero, other), sorted(kw)
        assert torch.isfinite(mid).all() and not torch.equal(mid, main) and not torch.equal(mid, other)


def test_interval_and_where_the_guide_runs(gpu, monkeypatch):
    """guidance_interval = (3, 4) of 6 timesteps: the run equals the hand loop; the guide's forward pass runs at t = 4 and t = 3 only (its
    context's launch log holds exactly two forward passes, the evaluations come in that order); the step at t = 5 is the guided entry
    point without pred_guide - it writes the guide's views -, the steps at t = 6, 2 and 1 are the existing one; no copy at the start.
    With the interval at the top of the schedule the copy is there, once per batch"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import sampler
    eng, geng = tiny(gpu, predict_x=False), guide_of(gpu, predict_x=False)
    z = noise(gpu, 2)
    taus = g.sampling_timesteps(STEPS, 6)
    weights = g.guidance_table(2.5, STEPS, (3, 4))
    want, _, _, guided_at = generate_by_hand(eng, geng, z, taus, MODE_OF["eps"], weights)
    assert guided_at == [4, 3]
    gb, _ = views(geng, 2)
    geng.ctx.log_launches(True)
    geng.forward(gb)
    one_pass = geng.ctx.read_launch_log()
    assert one_pass
    calls, evaluated = [], []
    real_call, real_eval, real_set_t = sampler.call, sampler._Sampler.evaluate, sampler._Sampler.set_t
    monkeypatch.setattr(sampler, "call", lambda name, *a: (calls.append((name, a)), real_call(name, *a))[1])
    monkeypatch.setattr(sampler._Sampler, "evaluate", lambda self, B: (evaluated.append("guide" if self.eng is geng else "main"), real_eval(self, B))[1])
    kw = dict(num_steps=6, noise=z, predict_x=False, guide=den(geng), guidance_scale=2.5, use_graph=False)
    got = g.generate(den(eng), 2, guidance_interval=(3, 4), **kw)
    torch.cuda.synchronize()
    log = geng.ctx.read_launch_log()
    assert same_bits(got, want)
    assert log == one_pass * 2                                   # two forward passes of the guide, no more
    assert evaluated == ["main", "main", "main", "guide", "main", "guide", "main", "main"]
    steps = [(name, a) for name, a in calls if name in OLD_STEPS + NEW]
    assert [name for name, _ in steps] == [OLD_STEPS[0], NEW[1], NEW[1], NEW[1], OLD_STEPS[0], OLD_STEPS[0]]
    given = [(a[3] is not None, a[27] is not None) for name, a in steps if name == NEW[1]]        # (pred_guide, out3)
    assert given == [(False, True), (True, True), (True, False)]
    assert [name for name, _ in calls].count("gct2_diffusion_mix") == 1          # the given noise; no copy into the guide's views
    # the interval at the top: the first step run is guided, one copy per batch (3 images at batch_size 2: two batches)
    del calls[:], evaluated[:]
    g.generate(den(eng), 3, num_steps=6, size=SIZE, seed=2, batch_size=2, predict_x=False, guide=den(geng), guidance_scale=2.5,
               guidance_interval=(5, 6), use_graph=False)
    names = [name for name, _ in calls]
    assert names.count("gct2_diffusion_mix") == 2 and names.count(NEW[1]) == 2 * 2 and names.count(OLD_STEPS[0]) == 2 * 4
    assert evaluated.count("guide") == 2 * 2 and evaluated.count("main") == 2 * 6
    geng.ctx.log_launches(False)


def test_split_runs_and_the_batch_cut(gpu):
    """generate(4, batch_size=4) is generate(2, batch_size=2) followed by generate(2, first_index=2, batch_size=2), whatever batch_size
    cuts: from drawn noise with eta, under dpm2m, and with init + mask, where kept pixels are init's bits"""
    import gan_class_transfer2_amd as g
    eng, geng = tiny(gpu, predict_x=False), guide_of(gpu, predict_x=False)
    init = images(gpu, 4)
    m = torch.rand(4, SIZE, SIZE, generator=torch.Generator().manual_seed(3)).round().to(gpu)
    base = dict(num_steps=4, predict_x=False, seed=11, guide=den(geng), guidance_scale=2.0, guidance_interval=(2, 6))
    runs = (lambda n, lo=0, **more: g.generate(den(eng), n, size=SIZE, first_index=lo, **dict(base, eta=0.7, **more)),
            lambda n, lo=0, **more: g.generate(den(eng), n, size=SIZE, first_index=lo, **dict(base, solver="dpm2m", **more)),
            lambda n, lo=0, **more: g.generate(den(eng), n, init=init[lo:lo + n], mask=m[lo:lo + n], first_index=lo, **dict(base, **more)))
    for run in runs:
        a, b, odd = run(4, batch_size=4), run(4, batch_size=2), run(4, batch_size=3)
        lo, hi = run(2, batch_size=2), run(2, lo=2, batch_size=2)
        other, unguided = run(4, seed=12), run(4, guidance_scale=1.0)
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and same_bits(a, b) and same_bits(a, odd) and same_bits(a, torch.cat([lo, hi]))
        assert not torch.equal(a, other) and not torch.equal(a, unguided)
    a = runs[2](4)
    torch.cuda.synchronize()
    assert torch.equal(a[m == 0], init[m == 0])                  # kept pixels are init's bits


@pytest.mark.parametrize("solver", ["ddim", "dpm2m"])
def test_dynamic_thresholding_under_guidance(gpu, solver):
    """w = 3 with clip_denoised="dynamic": the run equals the hand loop with the guided select, thresholds included; some s exceeds the
    floor and the images lie within it; graph replay gives the same bits"""
    import gan_class_transfer2_amd as g
    eng, geng = tiny(gpu, predict_x=False), guide_of(gpu, predict_x=False)
    z = noise(gpu, 2)
    taus = g.sampling_timesteps(STEPS, 3)
    want, _, want_bounds, _ = generate_by_hand(eng, geng, z, taus, MODE_OF["eps"], [3.0] * STEPS, solver, dynamic=(0.9, 0.25))
    assert torch.isfinite(want).all() and float(want.abs().max()) <= 0.25
    assert any(bool((s > 0.25).any()) for s in want_bounds.values())
    kw = dict(num_steps=3, noise=z, solver=solver, predict_x=False, guide=den(geng), guidance_scale=3.0, clip_denoised="dynamic",
              dynamic_percentile=0.9, dynamic_floor=0.25, return_thresholds=True)
    for use_graph in (False, True, True):
        got, bounds = g.generate(den(eng), 2, use_graph=use_graph, **kw)
        torch.cuda.synchronize()
        assert same_bits(got, want), (solver, use_graph, float((got - want).abs().max()))
        assert set(bounds) == set(taus) and all(same_bits(bounds[t], want_bounds[t]) for t in taus)
    # from drawn noise at the default floor, with init + mask: s at least the floor, above it somewhere, the images within it
    init = images(gpu, 3)
    for more in (dict(size=SIZE), dict(init=init, mask=half_plane(gpu))):
        out, bounds = g.generate(den(eng), 3, num_steps=6, seed=7, batch_size=2, solver=solver, predict_x=False, guide=den(geng),
                                 guidance_scale=3.0, clip_denoised="dynamic", return_thresholds=True, **more)
        torch.cuda.synchronize()
        assert sorted(bounds) == [1, 2, 3, 4, 5, 6] and all(bool((s >= 1.0).all()) and bool(torch.isfinite(s).all()) for s in bounds.values())
        assert any(bool((s > 1.0).any()) for s in bounds.values()), {t: s.tolist() for t, s in bounds.items()}
        assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0 and float(out.std()) > 0


def test_other_networks(gpu):
    """per-timestep heads on both sides (set_t on both), a variant engine guided by a variant engine, and the averages of the guide:
    shape, finite, the kept half, the batch cut, and the guide matters"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.variants import VariantEngine
    init, m = images(gpu, 3), half_plane(gpu)
    heads = [g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS, seed=s, timestep_heads=True) for s in (4, 5)]
    variants = [VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=s) for s in (4, 5)]
    ema = guide_of(gpu, use_ema=True, ema_momentum=0.5)
    ema.base_lr, ema.warm_up = 1e-2, 0
    ema.train_step(init[:2])
    for eng, geng, more in ((heads[0], heads[1], {}), (variants[0], variants[1], {}), (tiny(gpu), ema, dict(guide_use_ema=True)),
                            (tiny(gpu), ema, {})):
        kw = dict(num_steps=6, strength=4 / 6, seed=5, clip_denoised=True, init=init, mask=m, guide=den(geng), guidance_scale=2.0, **more)
        a, b = (g.generate(den(eng), 3, batch_size=bs, **kw) for bs in (2, 3))
        plain = g.generate(den(eng), 3, **dict(kw, guidance_scale=1.0))
        torch.cuda.synchronize()
        assert tuple(a.shape) == (3, SIZE, SIZE, 3) and torch.isfinite(a).all() and float(a.std()) > 0 and same_bits(a, b)
        assert torch.equal(a[:, :, :SIZE // 2], init[:, :, :SIZE // 2]) and float(a.abs().max()) <= 1.0
        assert not torch.equal(a, plain)
    raw = g.generate(den(tiny(gpu)), 3, num_steps=6, seed=5, size=SIZE, guide=den(ema), guidance_scale=2.0)
    avg = g.generate(den(tiny(gpu)), 3, num_steps=6, seed=5, size=SIZE, guide=den(ema), guidance_scale=2.0, guide_use_ema=True)
    assert not torch.equal(raw, avg)                             # guide_use_ema reads other weights


def test_the_default_launches_none_of_it(gpu, monkeypatch):
    """guide=None: the calls of today - neither new entry point in the binding's calls or in the context's launch log; with a guide at
    a constant weight every step is one gct2_diffusion_step_guided (and one guided select under dynamic thresholding) and none of the
    steps it stands for"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import sampler
    eng, geng = tiny(gpu, predict_x=False), guide_of(gpu, predict_x=False)
    names = []
    real = sampler.call
    monkeypatch.setattr(sampler, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    init = images(gpu, 2)
    eng.ctx.log_launches(True)
    cases = (dict(size=SIZE, eta=0.5), dict(size=SIZE, clip_denoised=0.5, solver="dpm2m"), dict(init=init, mask=half_plane(gpu), clip_denoised=True),
             dict(size=SIZE, clip_denoised="dynamic"))
    for kw in cases:
        assert torch.isfinite(g.generate(den(eng), 2, num_steps=3, predict_x=False, **kw)).all()
    log = eng.ctx.read_launch_log()
    eng.ctx.log_launches(False)
    assert names and not any(n in names for n in NEW) and not any("guided" in t for t in log)
    for kw, old in zip(cases, (OLD_STEPS[0], OLD_STEPS[2], OLD_STEPS[1], OLD_STEPS[3])):
        del names[:]
        g.generate(den(eng), 2, num_steps=3, predict_x=False, guide=den(geng), guidance_scale=1.0, **kw)      # all ones: guide=None's calls
        assert names.count(old) == 3 and not any(n in names for n in NEW)
        del names[:]
        g.generate(den(eng), 2, num_steps=3, predict_x=False, guide=den(geng), guidance_scale=1.5, **kw)
        assert names.count(NEW[1]) == 3 and not any(n in names for n in OLD_STEPS)
        assert names.count(NEW[0]) == (3 if kw.get("clip_denoised") == "dynamic" else 0) and "gct2_x0_quantile" not in names


def test_no_training_state_moves(gpu):
    """after guided runs the state_dict, the RNG offsets, the recorded plans and the averages of BOTH denoisers are what they were, and
    the next train step of each is bit-identical (loss and parameters) to the one taken without the runs"""
    import gan_class_transfer2_amd as g
    x = images(gpu, 2, seed=4)
    init = images(gpu, 3)
    engines = [tiny(gpu, rng_seed=9, use_ema=True, ema_momentum=0.5), guide_of(gpu, rng_seed=10, use_ema=True, ema_momentum=0.5)]
    before = []
    for eng in engines:
        eng.base_lr, eng.warm_up = 1e-2, 0
        eng.train_step(x)                                        # (one step first: a recorded plan, optimizer slots and averages exist)
        sd, state = eng.state_dict(), _state(eng)
        want_loss = eng.train_step(x).clone()                    # the step taken WITHOUT the runs
        torch.cuda.synchronize()
        want, stepped = eng.get_params(), _state(eng)
        assert stepped != state
        eng.load_state_dict(sd)
        assert _state(eng) == state
        before.append((eng.state_dict(), state, want_loss, want, stepped, {k: id(v) for k, v in eng._plans.items()}))
    A, Gd = engines
    g.generate(den(A), 3, num_steps=4, seed=1, batch_size=2, clip_denoised="dynamic", init=init, mask=half_plane(gpu), solver="dpm2m",
               guide=den(Gd), guidance_scale=2.0, guide_use_ema=True)
    g.generate(den(A), 2, num_steps=6, size=SIZE, use_graph=False, eta=1.0, use_ema=True, guide=den(Gd), guidance_scale=lambda t: 1.0 + t / 6,
               guidance_interval=(2, 5))
    torch.cuda.synchronize()
    for eng, (sd, state, want_loss, want, stepped, plans) in zip(engines, before):
        now = eng.state_dict()
        assert set(now) == set(sd) and all(torch.equal(now[k], sd[k]) for k in sd)
        assert _state(eng) == state and {k: id(v) for k, v in eng._plans.items()} == plans
        loss = eng.train_step(x).clone()
        torch.cuda.synchronize()
        assert same_bits(loss, want_loss)
        got = eng.get_params()
        for k in ("D0.w", "dense.w"):
            assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k
        assert _state(eng) == stepped


def test_refusals(gpu):
    """every ValueError of the issue, on real engines, before any launch"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import sampler
    eng, geng = tiny(gpu), guide_of(gpu)
    names = []
    real = sampler.call
    sampler.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        run = lambda d=eng, **kw: g.generate(den(d), 2, size=SIZE, num_steps=3, **kw)
        bad = [dict(guidance_scale=2.0), dict(guidance_interval=(1, 3)), dict(guide=den(geng)), dict(guide=den(eng), guidance_scale=2.0),
               dict(guide=den(guide_of(gpu, predict_x=False)), guidance_scale=2.0),
               dict(guide=den(g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS + 2)), guidance_scale=2.0),
               dict(guide=den(g.UNetEngine(g.Topology(8, 16, 2), 1, gpu, steps=STEPS)), guidance_scale=2.0)]
        bad += [dict(guide=den(geng), guidance_scale=w) for w in (float("nan"), float("inf"), True, [1.0] * 5, lambda t: float("nan"))]
        bad += [dict(guide=den(geng), guidance_scale=2.0, guidance_interval=i) for i in ((0, 3), (1, 7), (4, 3))]
        for kw in bad:
            with pytest.raises(ValueError):
                run(**kw)
        other = guide_of(gpu)
        other.set_noise_schedule("cosine", 0.0)
        with pytest.raises(ValueError, match="noise schedule"):
            run(guide=den(other), guidance_scale=2.0)
        ode = dict(ordinary_differential_equation=True)
        with pytest.raises(ValueError, match="ordinary_differential_equation"):
            run(tiny(gpu, **ode), guide=den(guide_of(gpu, **ode)), guidance_scale=2.0, **ode)
    finally:
        sampler.call = real
    assert not names                                             # nothing was launched
