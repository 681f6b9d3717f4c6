"""encode and the image-conditioned generate (init, strength, mask) on the tiny network of tests/test_generate_step_gpu.py (size 16,
steps = 6, parameters of tests/golden/tiny_sampler.npz): against log_sample's own inversion, against loops written here from the forward
pass and the launches the fused ones replace (bit for bit), against the float64 loops of tests/img2img_cases.py around the float64
network oracle; the seed, the batch cut, the other configurations; and that nothing else moves."""
import numpy as np
import pytest
import torch

import img2img_cases as I
from oracle import denoiser_oracle as O
from test_generate_step_gpu import GOLDEN, SIZE, STEPS, SWITCHES, F32, _state, den, lib, noise, same_bits, stream, tiny

pytestmark = pytest.mark.gpu
PER = SIZE * SIZE * 3


def images(gpu, n, seed=7):
    """n images in [-1, 1) on the 1/128 grid, like decoded files"""
    return torch.tensor(np.floor(np.random.default_rng(seed).uniform(0, 256, (n, SIZE, SIZE, 3))) / 128 - 1, dtype=torch.float32, device=gpu)


def half_plane(gpu):
    m = torch.zeros(SIZE, SIZE, device=gpu)
    m[:, SIZE // 2:] = 1.0
    return m


def views(eng, B):
    b = eng.buffers(B, SIZE, SIZE)
    return b, (b.img.data_ptr(), 4, eng._slice_ptr(b.R[0], eng.topo.fu(0)), b.ld[0], B * SIZE * SIZE, 3, stream())


def alpha(t):
    return float(O.alpha_dash(t, STEPS))


def mode_of(name):
    return lib().SAMPLE_X if name == "x" else lib().SAMPLE_EPS


def oracle_net():
    from oracle import sampler_oracle as S
    z = np.load(GOLDEN)
    cfg = O.OracleConfig(size=SIZE, pixel_size=8, max_size=16, octaves=2, batch_size=1)
    return S.unet_denoiser({k[6:]: z[k] for k in z.files if k.startswith("param/")}, cfg)


def slot_draws(gpu, seed, first, n, K, slots):
    """what gct2_rng_normal writes at the documented slots of generation's stream: [len(slots), n, H, W, 3]"""
    import gan_class_transfer2_amd as g
    d = torch.empty(len(slots), n, SIZE, SIZE, 3, device=gpu)
    for j, k in enumerate(slots):
        for i in range(n):
            lib().call("gct2_rng_normal", seed, g.GENERATE_STREAM, g.trainer_math.generate_offset(first + i, k, K, PER), d[j, i].data_ptr(), PER,
                       stream())
    torch.cuda.synchronize()
    return d


# ---- encode -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(SWITCHES))
def test_encode_over_every_timestep_is_log_samples_inversion(gpu, mode):
    import gan_class_transfer2_amd as g
    z = np.load(GOLDEN)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
    eng = tiny(gpu, **SWITCHES[mode])
    want = g.log_sample(den(eng), t(z["example_image"]), t(z["example"]), t(z["dictionary"]), steps=STEPS, test_step=2, **SWITCHES[mode])["epsilon_theta"]
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and float(want.std()) > 0
    for use_graph in (False, True, True):
        got = g.encode(den(eng), t(z["example_image"]), num_steps=STEPS, use_graph=use_graph, **SWITCHES[mode])
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, SIZE, SIZE, 3)
        assert torch.equal(got, want), (mode, use_graph, float((got - want).abs().max()))


def invert_by_hand(eng, x0, taus, mode):
    """x = e = images; per timestep gct2_diffusion_mix, the forward pass, gct2_diffusion_update.  Returns the last eps_theta."""
    L = lib()
    b, v = views(eng, x0.shape[0])
    x, e, fake = x0.clone(), x0.clone(), torch.empty_like(x0)
    for tau in taus:
        L.call("gct2_diffusion_mix", eng.dtype, x.data_ptr(), e.data_ptr(), alpha(tau), fake.data_ptr(), *v)
        pred = eng.forward(b)
        L.call("gct2_diffusion_update", mode, pred.data_ptr(), fake.data_ptr(), alpha(tau), alpha(tau - 1), x.data_ptr(), e.data_ptr(), x.numel(), stream())
    torch.cuda.synchronize()
    return e


@pytest.mark.parametrize("mode", list(SWITCHES))
def test_encode_strided_against_the_hand_loop_and_float64(gpu, mode, parity_log):
    """3 of 6 timesteps, two images: the bits of the loop written from the launches, and the float64 inversion around the float64 network
    oracle within the bound the project holds fp32 log_sample (inversion included) to on this network, 2e-5 relative L2"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, **SWITCHES[mode])
    x = images(gpu, 2)
    taus = g.sampling_timesteps(STEPS, 3)
    want = invert_by_hand(eng, x, taus, mode_of(mode))
    got = g.encode(den(eng), x, num_steps=3, **SWITCHES[mode])
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(g.encode(den(eng), x, timesteps=taus, use_graph=False, **SWITCHES[mode]), want)
    net = oracle_net()
    ref = I.invert_f64(lambda fake, t: net(fake), x.cpu().numpy(), taus, STEPS, mode_of(mode))
    err = float(np.linalg.norm(got.cpu().numpy().astype(np.float64) - ref) / np.linalg.norm(ref))
    print(f"encode against the float64 inversion, {mode}: relative L2 {err:.3g}")
    parity_log(f"encode_fp32_{mode}", rel_l2=err)
    assert err <= 2e-5, (mode, err)
    # start_eps replaces the reference's eps_theta = image
    e0 = noise(gpu, 2, seed=54)
    other = g.encode(den(eng), x, num_steps=3, start_eps=e0, **SWITCHES[mode])
    ref = I.invert_f64(lambda fake, t: net(fake), x.cpu().numpy(), taus, STEPS, mode_of(mode), start_eps=e0.cpu().numpy())
    err = float(np.linalg.norm(other.cpu().numpy().astype(np.float64) - ref) / np.linalg.norm(ref))
    assert not torch.equal(other, got) and err <= 2e-5, err


def test_encode_batch_cut_and_round_trip(gpu):
    import gan_class_transfer2_amd as g
    eng = tiny(gpu)
    x = images(gpu, 4)
    a, b, c = (g.encode(den(eng), x, num_steps=3, batch_size=bs) for bs in (2, 3, 4))
    torch.cuda.synchronize()
    assert same_bits(a, b) and same_bits(a, c) and all(not torch.equal(a[i], a[j]) for i in range(4) for j in range(i))
    taus = g.sampling_timesteps(STEPS, 3)
    back = g.generate(den(eng), 4, noise=a, timesteps=taus)
    torch.cuda.synchronize()
    assert tuple(back.shape) == (4, SIZE, SIZE, 3) and torch.isfinite(back).all() and float(back.std()) > 0


# ---- init, strength ---------------------------------------------------------------------------------------------------------------------------

def img2img_by_hand(eng, init, z0, taus, run, mode):
    """gct2_diffusion_mix(init, z0, alpha(tau_run)), then `run` rounds of forward pass + gct2_diffusion_update + gct2_diffusion_mix(a_prev)"""
    L = lib()
    b, v = views(eng, init.shape[0])
    fake, x, e = (torch.empty_like(init) for _ in range(3))
    L.call("gct2_diffusion_mix", eng.dtype, init.data_ptr(), z0.data_ptr(), alpha(taus[run - 1]), fake.data_ptr(), *v)
    for j in range(run, 0, -1):
        a_t, a_prev = alpha(taus[j - 1]), alpha(taus[j - 2] if j > 1 else 0)
        pred = eng.forward(b)
        L.call("gct2_diffusion_update", mode, pred.data_ptr(), fake.data_ptr(), a_t, a_prev, x.data_ptr(), e.data_ptr(), x.numel(), stream())
        L.call("gct2_diffusion_mix", eng.dtype, x.data_ptr(), e.data_ptr(), a_prev, fake.data_ptr(), *v)
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("mode", list(SWITCHES))
def test_generate_from_an_image_equals_the_hand_loop(gpu, mode):
    """strength = 0.5 of 6 steps at eta = 0: the slot-0 draw mixed into the image at alpha(tau_3), then three steps; strength = 1: all six"""
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, **SWITCHES[mode])
    init = images(gpu, 2)
    seed, first = 31, 3
    taus = g.sampling_timesteps(STEPS, 6)
    z0 = slot_draws(gpu, seed, first, 2, 6, (0,))[0]
    kw = dict(num_steps=6, eta=0.0, seed=seed, first_index=first, init=init, **SWITCHES[mode])
    for strength, run in ((0.5, 3), (1.0, 6), (0.2, 1)):
        want = img2img_by_hand(eng, init, z0, taus, run, mode_of(mode))
        for use_graph in (False, True):
            got, kept = g.generate(den(eng), 2, strength=strength, use_graph=use_graph, return_steps=(taus[run - 1],), **kw)
            torch.cuda.synchronize()
            assert same_bits(got, want), (mode, strength, use_graph, float((got - want).abs().max()))
            assert set(kept) == {taus[run - 1]} and (run > 1 or same_bits(kept[1], want))
    with pytest.raises(ValueError, match="return_steps"):
        g.generate(den(eng), 2, strength=0.5, return_steps=(4,), **kw)
    assert not torch.equal(g.generate(den(eng), 2, strength=0.5, **kw), g.generate(den(eng), 2, strength=1.0, **kw))


# ---- mask ---------------------------------------------------------------------------------------------------------------------------------------

def test_masks_all_ones_all_zeros_half_plane(gpu):
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, predict_x=False)
    init = images(gpu, 3)
    for kw in (dict(num_steps=6, eta=0.7, clip_denoised=True, seed=5, strength=0.5), dict(num_steps=3, eta=0.0, seed=6)):
        kw = dict(kw, init=init, predict_x=False)
        plain = g.generate(den(eng), 3, **kw)
        ones = g.generate(den(eng), 3, mask=torch.ones(SIZE, SIZE), **kw)
        zeros = g.generate(den(eng), 3, mask=torch.zeros(3, SIZE, SIZE, 1, device=gpu), **kw)
        half = g.generate(den(eng), 3, mask=half_plane(gpu), **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(plain).all() and same_bits(ones, plain)
        assert torch.equal(zeros, init)
        assert torch.equal(half[:, :, :SIZE // 2], init[:, :, :SIZE // 2])
        new = half[:, :, SIZE // 2:]
        assert torch.isfinite(new).all() and not torch.equal(new, init[:, :, SIZE // 2:]) and float((new - init[:, :, SIZE // 2:]).abs().mean()) > 1e-3
        # the regenerated half sees the kept half through the network: it is not the unmasked run's
        assert not torch.equal(new, plain[:, :, SIZE // 2:])


@pytest.mark.parametrize("mode", list(SWITCHES))
def test_masked_generate_against_the_float64_sampler(gpu, mode, parity_log):
    """eta = 0.7 with the clip, 3 of 6 steps, two images from index 4, the half-plane mask with a blended column: the float64 masked
    sampler fed the draws of the documented slots.  The bound is the one fp32 log_sample is held to on this network (2e-5 relative L2)"""
    import gan_class_transfer2_amd as g
    net = oracle_net()
    eng = tiny(gpu, **SWITCHES[mode])
    K, n, first, seed = 3, 2, 4, 21
    taus = g.sampling_timesteps(STEPS, K)
    init = images(gpu, n, seed=8)
    m = half_plane(gpu)
    m[:, SIZE // 2 - 1] = 0.5
    d = slot_draws(gpu, seed, first, n, K, range(K + 1)).cpu().numpy().astype(np.float64)
    el = np.broadcast_to(m.cpu().numpy()[None, :, :, None], (n, SIZE, SIZE, 3))
    want = I.masked_sample_f64(lambda fake, t: net(fake), init.cpu().numpy(), el, d[0], taus, STEPS, mode_of(mode), eta=0.7, clip=1.0, z=d[1:])
    got = g.generate(den(eng), n, num_steps=K, eta=0.7, clip_denoised=True, seed=seed, first_index=first, init=init, mask=m, **SWITCHES[mode])
    torch.cuda.synchronize()
    got = got.cpu().numpy().astype(np.float64)
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"masked generate against the float64 sampler, {mode}: relative L2 {err:.3g}")
    parity_log(f"masked_generate_fp32_{mode}", rel_l2=err)
    assert np.abs(want).max() <= 1.0 and err <= 2e-5, (mode, err)


def test_masked_generate_is_reproducible_from_its_seed_and_cut_anywhere(gpu):
    import gan_class_transfer2_amd as g
    eng = tiny(gpu, predict_x=False)
    init = images(gpu, 4)
    m = torch.rand(4, SIZE, SIZE, generator=torch.Generator().manual_seed(3)).round().to(gpu)
    kw = dict(num_steps=3, eta=0.7, predict_x=False, clip_denoised=True)
    run = lambda n, lo=0, **more: g.generate(den(eng), n, init=init[lo:lo + n], mask=m[lo:lo + n], first_index=lo, **dict(kw, **more))
    a, b, odd = run(4, seed=11, batch_size=2), run(4, seed=11, batch_size=4), run(4, seed=11, batch_size=3)
    c = run(4, seed=12)
    lo, hi = run(2, seed=11), run(2, lo=2, seed=11)
    det = [run(4, seed=s, eta=0.0) for s in (11, 11, 12)]
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert same_bits(a, b) and same_bits(a, odd) and same_bits(a, torch.cat([lo, hi]))
    assert not torch.equal(a, c) and not torch.equal(a, det[0])
    assert same_bits(det[0], det[1]) and not torch.equal(det[0], det[2])        # eta = 0: deterministic given the seed of the start
    assert torch.equal(a[m == 0], init[m == 0])


def test_other_configurations(gpu):
    """per-timestep heads, the averages and a variant network, each once: shape, finite, the batch cut"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.variants import VariantEngine
    init, m = images(gpu, 3), half_plane(gpu)
    heads = g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS, seed=4, timestep_heads=True)
    ema = tiny(gpu, use_ema=True, ema_momentum=0.5)
    ema.base_lr, ema.warm_up = 1e-2, 0
    ema.train_step(init[:2])
    variant = VariantEngine(8, 16, 2, 1, False, True, F32, gpu, steps=STEPS, seed=4)
    for eng, more in ((heads, {}), (ema, dict(use_ema=True)), (variant, {})):
        lat = [g.encode(den(eng), init, num_steps=3, batch_size=bs, **more) for bs in (2, 3)]
        out = [g.generate(den(eng), 3, num_steps=6, strength=0.5, eta=1.0, seed=5, clip_denoised=True, init=init, mask=m, batch_size=bs, **more)
               for bs in (2, 3)]
        torch.cuda.synchronize()
        for a, b in (lat, out):
            assert tuple(a.shape) == (3, SIZE, SIZE, 3) and torch.isfinite(a).all() and float(a.std()) > 0 and same_bits(a, b)
        assert torch.equal(out[0][:, :, :SIZE // 2], init[:, :, :SIZE // 2]) and float(out[0].abs().max()) <= 1.0
    raw = g.generate(den(ema), 3, num_steps=3, seed=5, init=init, mask=m)
    avg = g.generate(den(ema), 3, num_steps=3, seed=5, init=init, mask=m, use_ema=True)
    assert not torch.equal(raw, avg) and not torch.equal(g.encode(den(ema), init, num_steps=3), g.encode(den(ema), init, num_steps=3, use_ema=True))


def test_no_training_state_moves(gpu):
    """a train step taken after encode, a masked generate and an image-to-image generate is bit-identical (loss and parameter
    tensors) to the one taken without them; the RNG positions and the step counter do not move; log_sample before and after gives
    identical outputs.  Both steps run on ONE engine, from the same restored state_dict: two engine instances of equal state need not
    round their weight-gradient sums alike (their buffers sit at other addresses), which has nothing to do with sampling"""
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
    # the step taken WITHOUT them
    want_loss = A.train_step(x).clone()
    torch.cuda.synchronize()
    want, stepped = A.get_params(), _state(A)
    assert stepped != state
    A.load_state_dict(sd)
    assert _state(A) == state
    # ... and with them in front
    before = g.log_sample(den(A), *sample_args, steps=STEPS, test_step=2)
    g.encode(den(A), init, num_steps=3, batch_size=2)
    g.generate(den(A), 3, num_steps=3, eta=0.7, seed=1, batch_size=2, clip_denoised=True, init=init, mask=half_plane(gpu))
    g.generate(den(A), 2, num_steps=6, strength=0.5, init=init[:2], use_graph=False)
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


def test_errors(gpu):
    import gan_class_transfer2_amd as g
    eng = tiny(gpu)
    init = images(gpu, 2)
    for kw, what in ((dict(mask=half_plane(gpu), size=SIZE), "init"), (dict(strength=0.5, size=SIZE), "init"),
                     (dict(init=init, noise=noise(gpu, 2)), "noise"), (dict(init=images(gpu, 3)), "init"), (dict(init=init[..., :2]), "init"),
                     (dict(init=init[0]), "init"), (dict(init=init, strength=0.0), "strength"), (dict(init=init, strength=1.01), "strength"),
                     (dict(init=init, mask=torch.ones(2, SIZE, SIZE, 3)), "mask"), (dict(init=init, mask=torch.ones(SIZE)), "mask")):
        with pytest.raises(ValueError, match=what):
            g.generate(den(eng), 2, num_steps=3, **kw)
    for kw, what in ((dict(num_steps=7), "num_steps"), (dict(start_eps=init[:1]), "start_eps"), (dict(batch_size=0), "batch_size")):
        with pytest.raises(ValueError, match=what):
            g.encode(den(eng), init, **kw)
