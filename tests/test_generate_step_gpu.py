"""generate on the tiny network of tests/test_sampler_gpu.py (size 16, pixel_size 8, max_size 16, 2 octaves, steps = 6, parameters of
tests/golden/tiny_sampler.npz): against a loop written here from the forward pass and the two launches the fused step replaces, bit
for bit; the seed, the batch cut, clipping, the per-timestep heads, the averages, a variant network; and that nothing else moves."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import denoiser_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_sampler.npz")
SIZE, STEPS = 16, 6
F32 = 0
SWITCHES = {"x": {}, "eps": dict(predict_x=False)}


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def tiny(gpu, dtype=F32, **kw):
    import gan_class_transfer2_amd as g
    z = np.load(GOLDEN)
    eng = g.UNetEngine(g.Topology(8, 16, 2), dtype, gpu, steps=STEPS, **kw)
    eng.set_params({k[6:]: z[k] for k in z.files if k.startswith("param/")})
    return eng


def den(eng):
    return types.SimpleNamespace(ensure_engine=lambda: eng)


def noise(gpu, n, seed=51):
    return torch.randn(n, SIZE, SIZE, 3, generator=torch.Generator().manual_seed(seed)).to(gpu)


def hand_loop(eng, z, taus, mode, heads=False):
    """the same schedule from the launches generate replaces: gct2_diffusion_mix(alpha = 0) puts the noise in, then per step the
    forward pass, gct2_diffusion_update and gct2_diffusion_mix(alpha_prev).  Returns the last x_theta."""
    L = lib()
    B = z.shape[0]
    b = eng.buffers(B, SIZE, SIZE)
    views = (b.img.data_ptr(), 4, eng._slice_ptr(b.R[0], eng.topo.fu(0)), b.ld[0], B * SIZE * SIZE, 3, stream())
    fake, x, e = (torch.empty_like(z) for _ in range(3))
    L.call("gct2_diffusion_mix", eng.dtype, z.data_ptr(), z.data_ptr(), 0.0, fake.data_ptr(), *views)
    K = len(taus)
    for k in range(K):
        tau = taus[K - 1 - k]
        a_t, a_prev = float(O.alpha_dash(tau, STEPS)), float(O.alpha_dash(taus[K - 2 - k] if k < K - 1 else 0, STEPS))
        if heads:
            b.t_int.fill_(tau)
        pred = eng.forward(b)
        L.call("gct2_diffusion_update", mode, pred.data_ptr(), fake.data_ptr(), a_t, a_prev, x.data_ptr(), e.data_ptr(), x.numel(), stream())
        L.call("gct2_diffusion_mix", eng.dtype, x.data_ptr(), e.data_ptr(), a_prev, fake.data_ptr(), *views)
    torch.cuda.synchronize()
    return x


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("num_steps", [6, 3])
@pytest.mark.parametrize("mode", list(SWITCHES))
def test_generate_equals_the_two_launch_loop(gpu, mode, num_steps):
    """fp32, eta = 0, a given starting noise: bit for bit the hand-written loop, with graph replay and with plain launches"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, **SWITCHES[mode])
    z = noise(gpu, 2)
    taus = g.sampling_timesteps(STEPS, num_steps)
    assert taus == ([1, 2, 3, 4, 5, 6] if num_steps == 6 else [2, 4, 6])
    want = hand_loop(eng, z, taus, lib().SAMPLE_X if mode == "x" else lib().SAMPLE_EPS)
    assert torch.isfinite(want).all() and float(want.std()) > 0
    for use_graph in (False, True, True):                       # (the second graph run replays the capture of the first)
        got = g.generate(den(eng), 2, num_steps=num_steps, eta=0.0, noise=z, use_graph=use_graph, **SWITCHES[mode])
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, SIZE, SIZE, 3)
        assert same_bits(got, want), (mode, num_steps, use_graph, float((got - want).abs().max()))
    assert len(eng._forward_graphs) == 1
    # an explicit timesteps list is the same schedule; return_steps hands out the estimates on the way
    got, kept = g.generate(den(eng), 2, timesteps=taus, noise=z, return_steps=(taus[-1], taus[0]), **SWITCHES[mode])
    torch.cuda.synchronize()
    assert same_bits(got, want) and same_bits(kept[taus[0]], want) and set(kept) == {taus[0], taus[-1]}
    first = hand_loop(eng, z, taus[-1:], lib().SAMPLE_X if mode == "x" else lib().SAMPLE_EPS)
    # (the one-step loop ends at alpha_dash(0), the K-step one at alpha_dash of the next timestep: x_theta of the first step is the same)
    assert same_bits(kept[taus[-1]], first)


@pytest.mark.parametrize("mode", list(SWITCHES))
def test_generate_against_the_float64_sampler(gpu, mode, parity_log):
    """eta = 0.7 with the clip, 3 of 6 steps, two images from index 4: the whole sampler in float64 (generate_cases.ddim_sample_f64 around
    the float64 network oracle) fed the draws gct2_rng_normal makes at the documented slots of stream 5.  The bound is the one
    tests/test_sampler_gpu.py holds fp32 log_sample to on this network (2e-5 relative L2, measured 1e-7 .. 3e-7 there; fewer steps here)"""
    import gan_class_transfer2_amd as g
    import generate_cases as G
    from oracle import sampler_oracle as S
    z = np.load(GOLDEN)
    cfg = O.OracleConfig(size=SIZE, pixel_size=8, max_size=16, octaves=2, batch_size=1)
    net = S.unet_denoiser({k[6:]: z[k] for k in z.files if k.startswith("param/")}, cfg)
    eng = tiny(gpu, **SWITCHES[mode])
    K, n, first, seed, per = 3, 2, 4, 21, SIZE * SIZE * 3
    taus = g.sampling_timesteps(STEPS, K)
    draws = torch.empty(K + 1, n, SIZE, SIZE, 3, device=gpu)
    for k in range(K + 1):
        for i in range(n):
            lib().call("gct2_rng_normal", seed, g.GENERATE_STREAM, g.trainer_math.generate_offset(first + i, k, K, per), draws[k, i].data_ptr(),
                       per, stream())
    torch.cuda.synchronize()
    d = draws.cpu().numpy().astype(np.float64)
    want = G.ddim_sample_f64(lambda fake, t: net(fake), d[0], taus, STEPS, lib().SAMPLE_X if mode == "x" else lib().SAMPLE_EPS, eta=0.7,
                             clip=1.0, z=d[1:])
    got = g.generate(den(eng), n, num_steps=K, eta=0.7, clip_denoised=True, seed=seed, first_index=first, size=SIZE, **SWITCHES[mode])
    torch.cuda.synchronize()
    got = got.cpu().numpy().astype(np.float64)
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"generate against the float64 sampler, {mode}: relative L2 {err:.3g}")
    parity_log(f"generate_fp32_{mode}", rel_l2=err)
    assert np.abs(want).max() <= 1.0 and err <= 2e-5, (mode, err)


def test_generate_is_reproducible_from_its_seed_and_cut_anywhere(gpu):
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, predict_x=False)
    kw = dict(num_steps=3, eta=0.7, size=SIZE, predict_x=False)
    a = g.generate(den(eng), 4, seed=11, batch_size=2, **kw)
    b = g.generate(den(eng), 4, seed=11, batch_size=4, **kw)
    c = g.generate(den(eng), 4, seed=12, batch_size=4, **kw)
    lo, hi = g.generate(den(eng), 2, seed=11, **kw), g.generate(den(eng), 2, seed=11, first_index=2, **kw)
    odd = g.generate(den(eng), 4, seed=11, batch_size=3, **kw)                      # a partial last chunk
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert same_bits(a, b) and same_bits(a, torch.cat([lo, hi])) and same_bits(a, odd)
    assert not torch.equal(a, c)
    assert all(not torch.equal(a[i], a[j]) for i in range(4) for j in range(i))     # every image has noise of its own
    # eta matters, and eta = 0 draws nothing after the start: only the start depends on the slot layout
    d = g.generate(den(eng), 4, seed=11, **dict(kw, eta=0.0))
    assert not torch.equal(a, d)


def test_generate_start_is_the_documented_stream(gpu):
    """eta = 0 from the drawn start equals eta = 0 from the same noise handed in: image g reads stream 5 at (g (K + 1)) per_image"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu)
    K, per = 3, SIZE * SIZE * 3
    z = torch.empty(2, SIZE, SIZE, 3, device=gpu)
    for i in range(2):
        lib().call("gct2_rng_normal", 77, g.GENERATE_STREAM, g.trainer_math.generate_offset(5 + i, 0, K, per), z[i].data_ptr(), per, stream())
    got = g.generate(den(eng), 2, num_steps=K, seed=77, first_index=5, size=SIZE)
    want = g.generate(den(eng), 2, num_steps=K, noise=z)
    torch.cuda.synchronize()
    assert same_bits(got, want)


def test_generate_clips_the_estimate(gpu):
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, predict_x=False)
    kw = dict(num_steps=6, eta=0.5, seed=3, size=SIZE, predict_x=False)
    free = g.generate(den(eng), 3, **kw)
    unit, kept = g.generate(den(eng), 3, clip_denoised=True, return_steps=(6, 3), **kw)
    half = g.generate(den(eng), 3, clip_denoised=0.5, **kw)
    torch.cuda.synchronize()
    assert float(free.abs().max()) > 1.0                         # the epsilon objective divides by sqrt(alpha): the guard is needed
    assert float(unit.abs().max()) <= 1.0 and float(half.abs().max()) <= 0.5
    assert all(float(v.abs().max()) <= 1.0 for v in kept.values())
    assert same_bits(g.generate(den(eng), 3, clip_denoised=False, **kw), free)


def test_generate_sets_the_timestep_of_every_evaluation(gpu):
    """per-timestep heads: num_steps = 3 against the hand-written loop that sets t = tau_i in front of every forward pass"""
    import gan_class_transfer2_amd as g
    eng = g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS, seed=4, timestep_heads=True)
    z = noise(gpu, 2, seed=52)
    taus = g.sampling_timesteps(STEPS, 3)
    want = hand_loop(eng, z, taus, lib().SAMPLE_X, heads=True)
    wrong = hand_loop(eng, z, [1, 2, 3], lib().SAMPLE_X, heads=True)
    assert not torch.equal(want, wrong)
    for use_graph in (False, True, True):
        got = g.generate(den(eng), 2, num_steps=3, noise=z, use_graph=use_graph)
        torch.cuda.synchronize()
        assert same_bits(got, want), use_graph


def test_generate_reads_the_averages(gpu):
    import gan_class_transfer2_amd as g
    raw, avg = tiny(gpu, use_ema=True, ema_momentum=0.5), tiny(gpu)
    x = torch.tensor(np.floor(np.random.default_rng(3).uniform(0, 256, (2, SIZE, SIZE, 3))) / 128 - 1, dtype=torch.float32, device=gpu)
    raw.base_lr, raw.warm_up = 1e-2, 0                           # a visible update: the averages and the iterate part ways
    raw.train_step(x)
    avg.set_params({k: raw.arena._view(raw.arena.ema, k).clone() for k in raw.arena.shapes})     # a plain engine whose weights ARE the averages
    torch.cuda.synchronize()
    assert torch.equal(avg.arena.p, raw.arena.ema) and not torch.equal(raw.arena.p, raw.arena.ema)
    z = noise(gpu, 2, seed=53)
    kw = dict(num_steps=3, noise=z)
    got_raw, got_avg = g.generate(den(raw), 2, **kw), g.generate(den(raw), 2, use_ema=True, **kw)
    again = g.generate(den(raw), 2, **kw)
    want_avg = g.generate(den(avg), 2, **kw)
    torch.cuda.synchronize()
    assert same_bits(got_avg, want_avg) and same_bits(got_raw, again) and not torch.equal(got_raw, got_avg)
    with pytest.raises(ValueError):
        g.generate(den(avg), 2, use_ema=True, **kw)              # that engine keeps no averages


def test_generate_on_a_variant_network(gpu):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.variants import VariantEngine
    eng = VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4, predict_x=False)
    a = g.generate(den(eng), 3, num_steps=3, eta=1.0, seed=5, size=SIZE, batch_size=2, clip_denoised=True, predict_x=False)
    b = g.generate(den(eng), 3, num_steps=3, eta=1.0, seed=5, size=SIZE, batch_size=3, clip_denoised=True, predict_x=False)
    torch.cuda.synchronize()
    assert tuple(a.shape) == (3, SIZE, SIZE, 3) and torch.isfinite(a).all() and float(a.abs().max()) <= 1.0 and float(a.std()) > 0
    assert same_bits(a, b)


def _state(eng):
    return dict(rng_t=eng.rng_offset_t, rng_eps=eng.rng_offset_eps, iterations=eng.iterations)


def test_generate_moves_no_training_state(gpu):
    """a train step taken after generate is bit-identical to one taken without it (loss and a parameter tensor); the RNG positions and
    the step counter do not move; log_sample before and after gives identical outputs"""
    import gan_class_transfer2_amd as g
    z = np.load(GOLDEN)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
    sample_args = (t(z["example_image"]), t(z["example"]), t(z["dictionary"]))
    x = torch.tensor(np.floor(np.random.default_rng(4).uniform(0, 256, (2, SIZE, SIZE, 3))) / 128 - 1, dtype=torch.float32, device=gpu)
    engines = [tiny(gpu, rng_seed=9), tiny(gpu, rng_seed=9)]
    for eng in engines:
        eng.base_lr, eng.warm_up = 1e-2, 0
        eng.train_step(x)                                        # (one step first: a recorded plan and optimizer slots exist)
    A, Bn = engines
    before = g.log_sample(den(A), *sample_args, steps=STEPS, test_step=2)
    state = _state(A)
    g.generate(den(A), 3, num_steps=3, eta=0.7, seed=1, size=SIZE, batch_size=2, clip_denoised=True)
    g.generate(den(A), 2, num_steps=6, size=SIZE, use_graph=False)
    assert _state(A) == state == _state(Bn)
    after = g.log_sample(den(A), *sample_args, steps=STEPS, test_step=2)
    torch.cuda.synchronize()
    assert set(before) == set(after) and all(same_bits(before[k].reshape(-1), after[k].reshape(-1)) for k in before)
    la, lb = A.train_step(x).clone(), Bn.train_step(x).clone()
    torch.cuda.synchronize()
    assert same_bits(la, lb)
    pa, pb = A.get_params(), Bn.get_params()
    for k in ("D0.w", "dense.w"):
        assert np.array_equal(pa[k].view(np.int32), pb[k].view(np.int32)), k
    assert _state(A) == _state(Bn) and _state(A) != state
