"""generate(solver="dpm2m") and encode(solver="dpm2m") on the tiny network of tests/test_generate_step_gpu.py (size 16, steps = 6,
parameters of tests/golden/tiny_sampler.npz): against loops written here from the forward pass, the float32 restatement of
gct2_diffusion_step_multistep on the host and gct2_diffusion_mix(alpha = 0) to put the state back, bit for bit; the runs every c1
of which is 0 against solver="ddim"; the split run, the batch cut, the mask, return_steps, the other configurations; that the
default is today's sampler; and that nothing else moves."""
import numpy as np
import pytest
import torch

import multistep_cases as MC
from test_generate_step_gpu import GOLDEN, SIZE, STEPS, SWITCHES, F32, _state, den, lib, noise, same_bits, tiny
from test_img2img_step_gpu import alpha, half_plane, images, mode_of, views

pytestmark = pytest.mark.gpu


def inject(eng, v, state):
    """the state back where generate keeps it and where the network reads it: gct2_diffusion_mix(alpha = 0), fake = 0 s + 1 s"""
    s = torch.tensor(state).to(eng.device).contiguous()
    fake = torch.empty_like(s)
    lib().call("gct2_diffusion_mix", eng.dtype, s.data_ptr(), s.data_ptr(), 0.0, fake.data_ptr(), *v)
    return fake


def generate_by_hand(eng, z, taus, mode, clip=0.0):
    """generate(solver="dpm2m", noise=z): per step the forward pass, then the restatement on the host.  c1 = 0 at the first and at the
    last step, multistep_coefficient(alpha of the timestep evaluated before, a_t, a_prev) between.  Returns the last estimate and
    {timestep: the network's (clipped) estimate there}"""
    import gan_class_transfer2_amd as g
    b, v = views(eng, z.shape[0])
    K = len(taus)
    state, hist, estimates, c1s = z.cpu().numpy(), None, {}, []
    for k in range(K):
        tau = taus[K - 1 - k]
        a_t, a_prev = alpha(tau), alpha(taus[K - 2 - k] if k < K - 1 else 0)
        c1 = 0.0 if k in (0, K - 1) else g.multistep_coefficient(alpha(taus[K - k]), a_t, a_prev)
        inject(eng, v, state)
        pred = eng.forward(b)
        torch.cuda.synchronize()
        state, x0, hist = MC.multistep_step_f32(mode, pred.cpu().numpy(), state, hist, a_t, a_prev, c1, clip)
        estimates[tau] = torch.tensor(x0).to(z.device)
        c1s.append(c1)
    return estimates[taus[0]], estimates, c1s


@pytest.mark.parametrize("num_steps", [6, 3])
@pytest.mark.parametrize("mode", list(SWITCHES))
def test_generate_equals_the_hand_loop(gpu, mode, num_steps):
    """fp32, a given starting noise: bit for bit the hand-written loop, with plain launches and with graph replay; return_steps hands
    out the network's estimates, not the extrapolated ones; and it is not the DDIM sampler"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, **SWITCHES[mode])
    z = noise(gpu, 2)
    taus = g.sampling_timesteps(STEPS, num_steps)
    want, estimates, c1s = generate_by_hand(eng, z, taus, mode_of(mode))
    assert c1s[0] == 0.0 and c1s[-1] == 0.0 and all(c > 0.0 for c in c1s[1:-1]) and len(c1s) == num_steps
    assert torch.isfinite(want).all() and float(want.std()) > 0
    for use_graph in (False, True, True):                       # (the second graph run replays the capture of the first)
        got = g.generate(den(eng), 2, num_steps=num_steps, noise=z, use_graph=use_graph, solver="dpm2m", **SWITCHES[mode])
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, SIZE, SIZE, 3)
        assert same_bits(got, want), (mode, num_steps, use_graph, float((got - want).abs().max()))
    marks = (taus[-1], taus[1], taus[0])
    got, kept = g.generate(den(eng), 2, timesteps=taus, noise=z, return_steps=marks, solver="dpm2m", **SWITCHES[mode])
    torch.cuda.synchronize()
    assert same_bits(got, want) and set(kept) == set(marks)
    for t in marks:
        assert same_bits(kept[t], estimates[t]), t
    ddim = g.generate(den(eng), 2, num_steps=num_steps, noise=z, **SWITCHES[mode])
    assert not torch.equal(ddim, want)
    # the first step has no history: its estimate is the DDIM sampler's; the second estimate is the first the extrapolation reaches
    _, ddim_kept = g.generate(den(eng), 2, num_steps=num_steps, noise=z, return_steps=marks, **SWITCHES[mode])
    assert same_bits(ddim_kept[taus[-1]], kept[taus[-1]])


@pytest.mark.parametrize("num_steps", [1, 2])
def test_short_runs_are_the_ddim_sampler(gpu, num_steps):
    """one and two steps: every c1 is 0 (the first step run and the last), the bits are solver="ddim"'s - from noise, from a seed with the
    clip, and from an image under a mask"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, predict_x=False)
    z, init = noise(gpu, 2), images(gpu, 2)
    for kw in (dict(noise=z), dict(seed=3, size=SIZE, clip_denoised=True), dict(seed=4, init=init, mask=half_plane(gpu)),
               dict(seed=4, init=init)):
        kw = dict(kw, num_steps=num_steps, predict_x=False)
        a, b = g.generate(den(eng), 2, solver="dpm2m", **kw), g.generate(den(eng), 2, solver="ddim", **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and same_bits(a, b), sorted(kw)
    x = images(gpu, 2, seed=9)
    for K in (1, 2):                                             # encode: no history at the first step, alpha 0 after the last
        assert same_bits(g.encode(den(eng), x, num_steps=K, solver="dpm2m", predict_x=False), g.encode(den(eng), x, num_steps=K, predict_x=False))
    # a strength cut to two steps of six: the first step run has no history
    kw = dict(num_steps=6, strength=2 / 6, seed=5, init=init, predict_x=False)
    assert same_bits(g.generate(den(eng), 2, solver="dpm2m", **kw), g.generate(den(eng), 2, **kw))


def test_split_runs_and_the_batch_cut(gpu):
    """generate(4) is generate(2) followed by generate(2, first_index=2), whatever batch_size cuts: with init + mask and from drawn
    noise; every batch starts without history"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, predict_x=False)
    init = images(gpu, 4)
    m = torch.rand(4, SIZE, SIZE, generator=torch.Generator().manual_seed(3)).round().to(gpu)
    kw = dict(num_steps=4, predict_x=False, clip_denoised=True, solver="dpm2m", seed=11)
    masked = lambda n, lo=0, **more: g.generate(den(eng), n, init=init[lo:lo + n], mask=m[lo:lo + n], first_index=lo, **dict(kw, **more))
    drawn = lambda n, lo=0, **more: g.generate(den(eng), n, size=SIZE, first_index=lo, **dict(kw, **more))
    for run in (masked, drawn):
        a, b, odd = run(4, batch_size=2), run(4, batch_size=4), run(4, batch_size=3)
        lo, hi = run(2), run(2, lo=2)
        other = run(4, seed=12)
        first_order = run(4, solver="ddim")
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and float(a.abs().max()) <= 1.0
        assert same_bits(a, b) and same_bits(a, odd) and same_bits(a, torch.cat([lo, hi]))
        assert not torch.equal(a, other) and not torch.equal(a, first_order)
    a = masked(4)
    torch.cuda.synchronize()
    assert torch.equal(a[m == 0], init[m == 0])                  # kept pixels are init's bits
    assert not torch.equal(a[m == 1], init[m == 1])


def test_masked_runs_keep_the_image(gpu):
    """all-ones is the unmasked image-to-image run, all-zeros returns init, the half plane keeps its half - and return_steps holds the
    composited estimates"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu)
    init = images(gpu, 3)
    kw = dict(num_steps=6, strength=4 / 6, seed=6, init=init, solver="dpm2m")
    plain = g.generate(den(eng), 3, **kw)
    ones = g.generate(den(eng), 3, mask=torch.ones(SIZE, SIZE), **kw)
    zeros = g.generate(den(eng), 3, mask=torch.zeros(3, SIZE, SIZE, 1, device=gpu), **kw)
    half, kept = g.generate(den(eng), 3, mask=half_plane(gpu), return_steps=(3, 2), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(plain).all() and same_bits(ones, plain) and torch.equal(zeros, init)
    for v in (half, kept[3], kept[2]):
        assert torch.equal(v[:, :, :SIZE // 2], init[:, :, :SIZE // 2])
    new = half[:, :, SIZE // 2:]
    assert torch.isfinite(new).all() and float((new - init[:, :, SIZE // 2:]).abs().mean()) > 1e-3
    assert not torch.equal(new, plain[:, :, SIZE // 2:])
    assert not torch.equal(half, g.generate(den(eng), 3, mask=half_plane(gpu), **dict(kw, solver="ddim")))


def encode_by_hand(eng, x0, taus, mode):
    """encode(solver="dpm2m"): gct2_diffusion_mix(x, x, alpha(tau_1)), then per timestep the forward pass and the restatement to the NEXT
    timestep's alpha (0 after the last).  Returns the last state: the latent"""
    import gan_class_transfer2_amd as g
    b, v = views(eng, x0.shape[0])
    fake = torch.empty_like(x0)
    lib().call("gct2_diffusion_mix", eng.dtype, x0.data_ptr(), x0.data_ptr(), alpha(taus[0]), fake.data_ptr(), *v)
    torch.cuda.synchronize()
    state, hist, c1s = fake.cpu().numpy(), None, []
    for k, tau in enumerate(taus):
        a_t, a_next = alpha(tau), alpha(taus[k + 1]) if k + 1 < len(taus) else 0.0
        c1 = g.multistep_coefficient(alpha(taus[k - 1]) if k else None, a_t, a_next)
        if k:
            inject(eng, v, state)
        pred = eng.forward(b)
        torch.cuda.synchronize()
        state, _, hist = MC.multistep_step_f32(mode, pred.cpu().numpy(), state, hist, a_t, a_next, c1, 0.0)
        c1s.append(c1)
    return torch.tensor(state).to(x0.device), c1s


@pytest.mark.parametrize("mode", list(SWITCHES))
def test_encode_equals_its_hand_loop(gpu, mode):
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, **SWITCHES[mode])
    x = images(gpu, 2)
    for K in (6, 3):
        taus = g.sampling_timesteps(STEPS, K)
        want, c1s = encode_by_hand(eng, x, taus, mode_of(mode))
        assert c1s[0] == 0.0 and c1s[-1] == 0.0 and all(c > 0.0 for c in c1s[1:-1])
        for use_graph in (False, True):
            got = g.encode(den(eng), x, num_steps=K, use_graph=use_graph, solver="dpm2m", **SWITCHES[mode])
            torch.cuda.synchronize()
            assert torch.isfinite(got).all() and same_bits(got, want), (mode, K, use_graph, float((got - want).abs().max()))
        assert not torch.equal(got, g.encode(den(eng), x, num_steps=K, **SWITCHES[mode]))
    a, b = (g.encode(den(eng), images(gpu, 4), num_steps=3, batch_size=bs, solver="dpm2m", **SWITCHES[mode]) for bs in (3, 4))
    assert same_bits(a, b)
    back = g.generate(den(eng), 2, noise=got, num_steps=3, solver="dpm2m", **SWITCHES[mode])
    assert torch.isfinite(back).all() and float(back.std()) > 0


def test_the_default_is_todays_sampler(gpu):
    """solver left alone, solver="ddim": the same bits, from generate (plain, noisy, masked) and from encode"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu)
    init, z = images(gpu, 2), noise(gpu, 2)
    for kw in (dict(noise=z, num_steps=3), dict(size=SIZE, seed=2, eta=0.7, num_steps=6, clip_denoised=True),
               dict(init=init, mask=half_plane(gpu), seed=3, num_steps=3, return_steps=(2,))):
        a, b = g.generate(den(eng), 2, **kw), g.generate(den(eng), 2, solver="ddim", **kw)
        torch.cuda.synchronize()
        if isinstance(a, tuple):
            assert same_bits(a[1][2], b[1][2])
            a, b = a[0], b[0]
        assert same_bits(a, b)
    assert same_bits(g.encode(den(eng), init, num_steps=3), g.encode(den(eng), init, num_steps=3, solver="ddim"))
    with pytest.raises(ValueError, match="solver"):
        g.generate(den(eng), 2, size=SIZE, solver="euler")
    with pytest.raises(ValueError, match="eta"):
        g.generate(den(eng), 2, size=SIZE, solver="dpm2m", eta=0.5)


def test_other_configurations(gpu):
    """per-timestep heads, the averages and a variant network, each once: shape, finite, the clip, the kept half, the batch cut; the
    heads see the timestep of every evaluation"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.variants import VariantEngine
    heads = g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS, seed=4, timestep_heads=True)
    init, m = images(gpu, 3), half_plane(gpu)
    ema = tiny(gpu, use_ema=True, ema_momentum=0.5)
    ema.base_lr, ema.warm_up = 1e-2, 0
    ema.train_step(init[:2])
    variant = VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4)
    for eng, more in ((heads, {}), (ema, dict(use_ema=True)), (variant, {})):
        lat = [g.encode(den(eng), init, num_steps=4, batch_size=bs, solver="dpm2m", **more) for bs in (2, 3)]
        out = [g.generate(den(eng), 3, num_steps=6, strength=4 / 6, seed=5, clip_denoised=True, init=init, mask=m, batch_size=bs, solver="dpm2m",
                          **more) for bs in (2, 3)]
        torch.cuda.synchronize()
        for a, b in (lat, out):
            assert tuple(a.shape) == (3, SIZE, SIZE, 3) and torch.isfinite(a).all() and float(a.std()) > 0 and same_bits(a, b)
        assert torch.equal(out[0][:, :, :SIZE // 2], init[:, :, :SIZE // 2]) and float(out[0].abs().max()) <= 1.0
        assert not torch.equal(out[0], g.generate(den(eng), 3, num_steps=6, strength=4 / 6, seed=5, clip_denoised=True, init=init, mask=m, **more))
    kw = dict(num_steps=4, seed=5, size=SIZE, solver="dpm2m")
    assert not torch.equal(g.generate(den(ema), 3, **kw), g.generate(den(ema), 3, use_ema=True, **kw))
    # the heads read t: the run at the timesteps 2, 4, 6 is not the run of the same three evaluations at 1, 2, 3
    z = noise(gpu, 2, seed=52)
    a = g.generate(den(heads), 2, timesteps=[2, 4, 6], noise=z, solver="dpm2m")
    b = g.generate(den(heads), 2, timesteps=[1, 2, 3], noise=z, solver="dpm2m")
    assert torch.isfinite(a).all() and not torch.equal(a, b)


def test_no_training_state_moves(gpu):
    """tests/test_img2img_step_gpu.py's check with the new solver: a train step taken after encode and generate with solver="dpm2m" is
    bit-identical (loss and parameter tensors) to the one taken without them, on ONE engine from the same restored state_dict; the RNG
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
    want_loss = A.train_step(x).clone()                          # the step taken WITHOUT them
    torch.cuda.synchronize()
    want, stepped = A.get_params(), _state(A)
    assert stepped != state
    A.load_state_dict(sd)
    assert _state(A) == state
    before = g.log_sample(den(A), *sample_args, steps=STEPS, test_step=2)
    g.encode(den(A), init, num_steps=4, batch_size=2, solver="dpm2m")
    g.generate(den(A), 3, num_steps=4, seed=1, batch_size=2, clip_denoised=True, init=init, mask=half_plane(gpu), solver="dpm2m")
    g.generate(den(A), 2, num_steps=6, size=SIZE, use_graph=False, solver="dpm2m")
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
