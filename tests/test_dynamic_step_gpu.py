"""generate(clip_denoised="dynamic") on the tiny network of tests/test_generate_step_gpu.py (size 16, steps = 6, parameters of
tests/golden/tiny_sampler.npz): a floor nothing reaches is the fixed clip bit for bit; against a loop written here from the forward
pass and the float32 restatement of the select and the step; the split run and the batch cut, thresholds included; the thresholds
engage under the epsilon objective and the images stay within the floor; graph replay; the other configurations; that the default
launches none of the new entry points; and that nothing else moves."""
import numpy as np
import pytest
import torch

import dynamic_cases as D
from test_generate_step_gpu import GOLDEN, SIZE, STEPS, SWITCHES, F32, _state, den, lib, noise, same_bits, tiny
from test_img2img_step_gpu import alpha, half_plane, images, mode_of, views
from test_multistep_step_gpu import inject

pytestmark = pytest.mark.gpu
PER = SIZE * SIZE * 3
NEW = ("gct2_x0_quantile", "gct2_diffusion_step_dynamic")
OLD_STEPS = ("gct2_diffusion_step", "gct2_diffusion_step_masked", "gct2_diffusion_step_multistep")


@pytest.mark.parametrize("solver", ["ddim", "dpm2m"])
def test_a_floor_nothing_reaches_is_the_fixed_clip(gpu, solver):
    """dynamic_floor = 1e30: the floor always wins, the bits are clip_denoised=1e30's - plain and masked, and with eta under ddim"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, predict_x=False)
    init = images(gpu, 2)
    for kw in (dict(size=SIZE, seed=3), dict(init=init, mask=half_plane(gpu), seed=4), dict(init=init, strength=4 / 6, seed=5)) + \
            ((dict(size=SIZE, seed=6, eta=0.7),) if solver == "ddim" else ()):
        kw = dict(kw, num_steps=6, predict_x=False, solver=solver)
        a, bounds = g.generate(den(eng), 2, clip_denoised="dynamic", dynamic_floor=1e30, return_thresholds=True, **kw)
        b = g.generate(den(eng), 2, clip_denoised=1e30, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and same_bits(a, b), sorted(kw)
        assert all(torch.equal(s, torch.full_like(s, 1e30)) for s in bounds.values())


def generate_by_hand(eng, z, taus, mode, percentile, floor):
    """generate(clip_denoised="dynamic", noise=z) under ddim at eta = 0: per step the forward pass, then the restatement of the select
    and of the step on the host.  Returns the last estimate, {timestep: estimate} and {timestep: s [n]}"""
    b, v = views(eng, z.shape[0])
    K = len(taus)
    rank = D.quantile_rank(percentile, PER)
    state, estimates, bounds = z.cpu().numpy().reshape(z.shape[0], PER), {}, {}
    for k in range(K):
        tau = taus[K - 1 - k]
        a_t, a_prev = alpha(tau), alpha(taus[K - 2 - k] if k < K - 1 else 0)
        inject(eng, v, state.reshape(z.shape))
        pred = eng.forward(b)
        torch.cuda.synchronize()
        p = pred.cpu().numpy().reshape(z.shape[0], PER)
        rows, _ = D.select_f32(mode, p, state, a_t, rank, floor)
        state, x0, _ = D.dynamic_step_f32(mode, p, state, rows, a_t, a_prev)
        estimates[tau] = torch.tensor(x0.reshape(z.shape)).to(z.device)
        bounds[tau] = torch.tensor(rows[:, 0]).to(z.device)
    return estimates[taus[0]], estimates, bounds


@pytest.mark.parametrize("mode", list(SWITCHES))
def test_generate_equals_the_hand_loop(gpu, mode):
    """fp32, a given starting noise, a floor of 0.25 that the estimates of this network exceed: bit for bit the hand-written loop, with
    plain launches and with graph replay, the thresholds and return_steps included; and it is not the fixed clip at the floor"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, **SWITCHES[mode])
    z = noise(gpu, 2)
    taus = g.sampling_timesteps(STEPS, 3)
    want, estimates, want_bounds = generate_by_hand(eng, z, taus, mode_of(mode), 0.9, 0.25)
    assert torch.isfinite(want).all() and float(want.abs().max()) <= 0.25
    assert any(bool((s > 0.25).any()) for s in want_bounds.values())          # the percentile engages: not the fixed clip
    kw = dict(num_steps=3, noise=z, clip_denoised="dynamic", dynamic_percentile=0.9, dynamic_floor=0.25, **SWITCHES[mode])
    for use_graph in (False, True, True):                       # (the second graph run replays the capture of the first)
        got, bounds = g.generate(den(eng), 2, use_graph=use_graph, return_thresholds=True, **kw)
        torch.cuda.synchronize()
        assert same_bits(got, want), (mode, use_graph, float((got - want).abs().max()))
        assert set(bounds) == set(taus) and all(same_bits(bounds[t], want_bounds[t]) for t in taus)
    got, kept, bounds = g.generate(den(eng), 2, return_steps=(taus[-1], taus[0]), return_thresholds=True, **kw)
    torch.cuda.synchronize()
    assert same_bits(got, want) and all(same_bits(kept[t], estimates[t]) for t in kept) and set(kept) == {taus[-1], taus[0]}
    assert same_bits(g.generate(den(eng), 2, **kw), want)                      # without the thresholds: the images alone
    assert not torch.equal(want, g.generate(den(eng), 2, **dict(kw, clip_denoised=0.25, dynamic_percentile=None, dynamic_floor=None)))


def test_split_runs_and_the_batch_cut(gpu):
    """generate(4, batch_size=4) is generate(2, batch_size=2) followed by generate(2, first_index=2, batch_size=2), thresholds included,
    whatever batch_size cuts: from drawn noise with eta, under dpm2m, and with init + mask"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, predict_x=False)
    init = images(gpu, 4)
    m = torch.rand(4, SIZE, SIZE, generator=torch.Generator().manual_seed(3)).round().to(gpu)
    base = dict(num_steps=4, predict_x=False, clip_denoised="dynamic", dynamic_percentile=0.95, seed=11, return_thresholds=True)
    runs = (lambda n, lo=0, **more: g.generate(den(eng), n, size=SIZE, first_index=lo, **dict(base, eta=0.7, **more)),
            lambda n, lo=0, **more: g.generate(den(eng), n, size=SIZE, first_index=lo, **dict(base, solver="dpm2m", **more)),
            lambda n, lo=0, **more: g.generate(den(eng), n, init=init[lo:lo + n], mask=m[lo:lo + n], first_index=lo, **dict(base, **more)))
    for run in runs:
        (a, sa), (b, sb), (odd, so) = run(4, batch_size=4), run(4, batch_size=2), run(4, batch_size=3)
        (lo, slo), (hi, shi) = run(2, batch_size=2), run(2, lo=2, batch_size=2)
        other, _ = run(4, seed=12)
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and same_bits(a, b) and same_bits(a, odd) and same_bits(a, torch.cat([lo, hi]))
        assert set(sa) == set(sb) == set(so) == set(slo) == set(shi) and len(sa) == 4
        for t in sa:
            assert tuple(sa[t].shape) == (4,) and sa[t].dtype == torch.float32
            assert same_bits(sa[t], sb[t]) and same_bits(sa[t], so[t]) and same_bits(sa[t], torch.cat([slo[t], shi[t]]))
        assert not torch.equal(a, other)
    a, _ = runs[2](4)
    torch.cuda.synchronize()
    assert torch.equal(a[m == 0], init[m == 0])                  # kept pixels are init's bits


def test_thresholds_engage_and_images_stay_within_the_floor(gpu):
    """the epsilon objective divides by sqrt(a_t): some step's s exceeds the floor, every s is at least the floor, and the final images
    (the last thresholded estimate) lie in [-floor, floor] - at the default floor and at another"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, predict_x=False)
    for floor, solver in ((1.0, "ddim"), (0.5, "dpm2m")):
        out, bounds = g.generate(den(eng), 3, num_steps=6, size=SIZE, seed=7, predict_x=False, clip_denoised="dynamic", dynamic_floor=floor,
                                 solver=solver, return_thresholds=True)
        torch.cuda.synchronize()
        assert sorted(bounds) == [1, 2, 3, 4, 5, 6] and all(tuple(s.shape) == (3,) for s in bounds.values())
        assert any(bool((s > floor).any()) for s in bounds.values()), {t: s.tolist() for t, s in bounds.items()}
        assert all(bool((s >= floor).all()) and bool(torch.isfinite(s).all()) for s in bounds.values())
        assert torch.isfinite(out).all() and float(out.abs().max()) <= floor and float(out.std()) > 0
    # a strength cut: only the timesteps run are reported
    init = images(gpu, 2)
    _, bounds = g.generate(den(eng), 2, num_steps=6, strength=2 / 6, init=init, seed=7, predict_x=False, clip_denoised="dynamic",
                           return_thresholds=True)
    assert sorted(bounds) == [1, 2]


def test_other_configurations(gpu):
    """per-timestep heads, the averages and a variant network, each once: shape, finite, the floor, the kept half, the batch cut"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.variants import VariantEngine
    heads = g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS, seed=4, timestep_heads=True)
    init, m = images(gpu, 3), half_plane(gpu)
    ema = tiny(gpu, use_ema=True, ema_momentum=0.5)
    ema.base_lr, ema.warm_up = 1e-2, 0
    ema.train_step(init[:2])
    variant = VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4)
    for eng, more in ((heads, {}), (ema, dict(use_ema=True)), (variant, {})):
        kw = dict(num_steps=6, strength=4 / 6, seed=5, clip_denoised="dynamic", dynamic_percentile=0.9, dynamic_floor=0.5, init=init, mask=m, **more)
        out = [g.generate(den(eng), 3, batch_size=bs, **kw) for bs in (2, 3)]
        torch.cuda.synchronize()
        a, b = out
        assert tuple(a.shape) == (3, SIZE, SIZE, 3) and torch.isfinite(a).all() and float(a.std()) > 0 and same_bits(a, b)
        assert torch.equal(a[:, :, :SIZE // 2], init[:, :, :SIZE // 2]) and float(a[:, :, SIZE // 2:].abs().max()) <= 0.5


def test_the_default_launches_none_of_it(gpu, monkeypatch):
    """clip_denoised left alone, True or a float: the calls of today (none of the new entry points, in the binding's calls and in the
    context's launch log) and the same bits as before the switch existed in the signature; with the switch every step is one select
    and one gct2_diffusion_step_dynamic, and none of the three steps it stands for"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import sampler
    eng = tiny(gpu, predict_x=False)
    names = []
    real = sampler.call
    monkeypatch.setattr(sampler, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    init = images(gpu, 2)
    eng.ctx.log_launches(True)
    for kw in (dict(size=SIZE), dict(size=SIZE, clip_denoised=True, eta=0.5), dict(size=SIZE, clip_denoised=0.5, solver="dpm2m"),
               dict(init=init, mask=half_plane(gpu), clip_denoised=True)):
        out = g.generate(den(eng), 2, num_steps=3, predict_x=False, **kw)
        assert torch.isfinite(out).all()
    log = eng.ctx.read_launch_log()
    eng.ctx.log_launches(False)
    assert names and not any(n in names for n in NEW) and not any("quantile" in t or "dynamic" in t for t in log)
    for kw, old in ((dict(size=SIZE, eta=0.5), OLD_STEPS[0]), (dict(size=SIZE, solver="dpm2m"), OLD_STEPS[2]),
                    (dict(init=init, mask=half_plane(gpu)), OLD_STEPS[1])):
        del names[:]
        g.generate(den(eng), 2, num_steps=3, predict_x=False, clip_denoised=True, **kw)
        assert names.count(old) == 3
        del names[:]
        g.generate(den(eng), 2, num_steps=3, predict_x=False, clip_denoised="dynamic", **kw)
        assert names.count(NEW[0]) == 3 and names.count(NEW[1]) == 3 and not any(n in names for n in OLD_STEPS)
        assert names.count("gct2_x0_quantile_scratch") <= 1


def test_no_training_state_moves(gpu):
    """tests/test_generate_step_gpu.py's check with the switch on: a train step taken after generate(clip_denoised="dynamic") is
    bit-identical (loss and parameter tensors) to the one taken without it, on ONE engine from the same restored state_dict; the RNG
    positions and the step counter do not move; log_sample before and after gives identical outputs"""
    import gan_class_transfer2_amd as g
    z = np.load(GOLDEN)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
    sample_args = (t(z["example_image"]), t(z["example"]), t(z["dictionary"]))
    x = images(gpu, 2, seed=4)
    init = images(gpu, 3)
    A = tiny(gpu, rng_seed=9)
    A.base_lr, A.warm_up = 1e-2, 0
    A.train_step(x)                                              # (one step first: a recorded plan and optimizer slots exist)
    sd = A.state_dict()
    state = _state(A)
    want_loss = A.train_step(x).clone()                          # the step taken WITHOUT it
    torch.cuda.synchronize()
    want, stepped = A.get_params(), _state(A)
    assert stepped != state
    A.load_state_dict(sd)
    assert _state(A) == state
    before = g.log_sample(den(A), *sample_args, steps=STEPS, test_step=2)
    g.generate(den(A), 3, num_steps=4, seed=1, batch_size=2, clip_denoised="dynamic", init=init, mask=half_plane(gpu), solver="dpm2m")
    g.generate(den(A), 2, num_steps=6, size=SIZE, use_graph=False, eta=1.0, clip_denoised="dynamic", dynamic_floor=0.5, return_thresholds=True)
    assert _state(A) == state
    after = g.log_sample(den(A), *sample_args, steps=STEPS, test_step=2)
    torch.cuda.synchronize()
    assert set(before) == set(after) and all(same_bits(before[k].reshape(-1), after[k].reshape(-1)) for k in before)
    loss = A.train_step(x).clone()
    torch.cuda.synchronize()
    assert same_bits(loss, want_loss)
    got = A.get_params()
    for k in ("D0.w", "dense.w"):
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k
    assert _state(A) == stepped
