"""Generation without a GPU: the host math (trainer_math.sampling_timesteps / ddim_sigma2 / generate_offset), what the restatements
of tests/generate_cases.py can tell apart, the two new entry points in the header, the binding, the plan table and the built
library, and the arguments generate refuses before it launches anything."""
import os
import re
import types

import numpy as np
import pytest

import generate_cases as G
import pointwise_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gct2_diffusion_step", "gct2_diffusion_start")


def tm():
    import gan_class_transfer2_amd as g
    return g.trainer_math


# ---- sampling_timesteps ------------------------------------------------------------------------------------------------------------------

def test_sampling_timesteps():
    T = tm().sampling_timesteps
    assert T(200, 1) == [200] and T(6, 1) == [6]
    assert T(200, 200) == list(range(1, 201)) and T(6, 6) == [1, 2, 3, 4, 5, 6]
    for K in (3, 7, 50):
        taus = T(200, K)
        assert len(taus) == K and taus[0] >= 1 and taus[-1] == 200
        assert all(b > a for a, b in zip(taus, taus[1:])), taus
        assert taus == [int(np.ceil(i * 200 / K)) for i in range(1, K + 1)]
    assert T(6, 3) == [2, 4, 6]
    for bad in ((200, 201), (6, 7), (6, 0), (6, -1), (6, 2.0), (6, True)):
        with pytest.raises(ValueError):
            T(*bad)


# ---- ddim_sigma2 --------------------------------------------------------------------------------------------------------------------------

def schedule_pairs(schedule, steps=200, K=7):
    """(a_t, a_prev) of every step of a K-step sampler under a named schedule"""
    M = tm()
    taus = M.sampling_timesteps(steps, K)
    a = lambda t: float(M.alpha_dash(t, steps, schedule, 0.0))
    return [(a(t), a(taus[i - 1] if i else 0)) for i, t in enumerate(taus)]


def test_ddim_sigma2():
    M = tm()
    for schedule in M.NOISE_SCHEDULES:
        for a_t, a_prev in schedule_pairs(schedule):
            assert 0.0 <= a_t < a_prev <= 1.0, (schedule, a_t, a_prev)
            assert M.ddim_sigma2(a_t, a_prev, 0.0) == 0.0
            posterior = (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)           # the DDPM posterior variance (Ho et al. 2020, eq. 7)
            assert M.ddim_sigma2(a_t, a_prev, 1.0) == posterior == G.sigma2(a_t, a_prev, 1.0)
            for eta in (0.0, 0.3, 0.7, 1.0, 5.0):
                s2 = M.ddim_sigma2(a_t, a_prev, eta)
                assert 0.0 <= s2 <= 1.0 - a_prev
                ce2 = (1.0 - a_prev) - s2                                       # what the kernel takes the root of, in float64
                assert ce2 >= 0.0 and abs(ce2 + s2 - (1.0 - a_prev)) <= 2.0 ** -52
            assert M.ddim_sigma2(a_t, a_prev, 1e3) == 1.0 - a_prev or a_prev == 1.0   # clamped from above
    for bad in (-1e-9, -1.0, float("nan")):
        with pytest.raises(ValueError):
            M.ddim_sigma2(0.1, 0.2, bad)


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_step_without_noise_or_clip_is_update_then_mix(mode):
    """sigma^2 = 0, clip = 0: diffusion_update_f32 followed by diffusion_mix_f32(a_prev), bit for bit; and the FMA-contracted form of
    the re-noising differs on these inputs, so the GPU test can tell the two apart"""
    pred, fake = G.step_case(G.B, G.NPIXS[0] * G.C)
    for t in P.DIFFUSION_TS:
        a_t, a_prev = G.alphas(t)
        got, x = G.diffusion_step_f32(mode, pred, fake, a_t, a_prev, 0.0, 0.0)
        xw, ew = P.diffusion_update_f32(mode, pred, fake, a_t, a_prev)
        want = P.diffusion_mix_f32(xw, ew, a_prev)
        assert got.dtype == want.dtype == np.float32
        assert np.array_equal(got.view(np.int32), want.view(np.int32)) and np.array_equal(x.view(np.int32), xw.view(np.int32))
        for clip in (0.0, -1.0):
            same, _ = G.diffusion_step_f32(mode, pred, fake, a_t, a_prev, 0.0, clip)
            assert np.array_equal(same.view(np.int32), got.view(np.int32))
        for term in (0, 1):
            fused, _ = G.diffusion_step_fused(mode, pred, fake, a_t, a_prev, 0.0, 0.0, term=term)
            share = float(np.mean(fused != got))
            if t == 1 and term == 0:                     # a_prev = alpha_dash(0) = 0.25: cx = 0.5, the product cx x is exact
                assert share == 0.0
            else:                                        # (a small cx - t = 199, 200 - rounds away most of the product's low bits:
                assert share > 0.005, (mode, t, term, share)     # one element would do; 45 of 9027 are asked for)
        # and both are the float64 step to float32 accuracy (the epsilon modes divide by sqrt(a_t) ~ 0.0025 at t = 200: relative)
        ref, x64 = G.ddim_step_f64(mode, pred, fake, a_t, a_prev, 0.0, 0.0)
        assert np.abs(got - ref).max() <= 4e-6 * max(1.0, np.abs(ref).max()) and np.abs(x - x64).max() <= 4e-6 * max(1.0, np.abs(x64).max())


@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_step_with_noise_and_clip_against_float64(mode):
    pred, fake = G.clip_case()
    rng = np.random.default_rng(43)
    z = rng.standard_normal(pred.shape).astype(np.float32)
    for t in P.DIFFUSION_TS:
        a_t, a_prev = G.alphas(t)
        s2 = G.sigma2(a_t, a_prev, 0.7)
        assert s2 > 0
        for clip in G.CLIPS:
            got, x = G.diffusion_step_f32(mode, pred, fake, a_t, a_prev, s2, clip, z)
            with np.errstate(all="ignore"):
                ref, x64 = G.ddim_step_f64(mode, pred, fake, a_t, a_prev, s2, clip, z)
            nan = np.isnan(x64)
            assert np.array_equal(np.isnan(x), nan) and np.array_equal(np.isnan(got), nan) and 0 < nan.sum() < 20
            ok = ~nan
            assert np.abs(x[ok]).max() == np.float32(clip) and (np.abs(x[ok]) <= np.float32(clip)).all()
            assert (x[ok] == np.float32(clip)).any() and (x[ok] == -np.float32(clip)).any() and (np.abs(x[ok]) < np.float32(clip)).any()
            assert np.abs(got[ok] - ref[ok]).max() <= 4e-6 * max(1.0, np.abs(ref[ok]).max())
            # the clip changes the result, and so does the noise
            unclipped, _ = G.diffusion_step_f32(mode, pred, fake, a_t, a_prev, s2, 0.0, z)
            silent, _ = G.diffusion_step_f32(mode, pred, fake, a_t, a_prev, 0.0, clip)
            assert (unclipped[ok] != got[ok]).any() and (silent[ok] != got[ok]).mean() > 0.9


# ---- the offset rule -----------------------------------------------------------------------------------------------------------------------

def test_generation_offsets_never_overlap():
    M = tm()
    assert M.GENERATE_STREAM == 5 and M.GENERATE_STREAM not in (1, 2, M.EVAL_STREAM_T, M.EVAL_STREAM_EPS)
    for K, per in ((1, 5), (3, 3009), (6, 768), (50, 49152)):
        starts = [M.generate_offset(g, k, K, per) for g in range(5) for k in range(K + 1)]
        assert starts == sorted(starts) and starts[0] == 0
        assert all(b - a == per for a, b in zip(starts, starts[1:]))           # back to back: [start, start + per) never overlap
        stride = M.generate_image_stride(K, per)
        assert stride == (K + 1) * per
        for k in range(K + 1):                                                  # one launch covers images g, g + 1, ... of a slot
            assert M.generate_offset(3, k, K, per) == M.generate_offset(1, k, K, per) + 2 * stride
    for bad in ((-1, 0), (0, -1), (0, 4)):
        with pytest.raises(ValueError):
            M.generate_offset(bad[0], bad[1], 3, 12)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------

def test_new_entry_points_everywhere():
    import gan_class_transfer2_amd as g
    L = g._lib
    raw = L.load()
    assert L.ABI_VERSION == 17 and raw.gct2_abi_version() == 17
    header = open(os.path.join(ROOT, "include", "gct2.h")).read()
    plan = open(os.path.join(ROOT, "gan-class-transfer2_amd", "csrc", "plan.hip")).read()
    for name in NEW:
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(L.SIGNATURES[name]) <= 28, name       # plan.hip MAX_ARGS
        assert name in L.PLANNABLE and hasattr(raw, name) and f"GCT2_ENTRY({name})" in plan
        assert L.SIGNATURES[name][-1] is L._vp                                              # the stream
    assert len(L.SIGNATURES[NEW[0]]) == 22 and len(L.SIGNATURES[NEW[1]]) == 14
    assert L.SIGNATURES[NEW[0]][4:8] == [L._d] * 4                                          # a_t, a_prev, sigma2, clip are doubles
    assert hasattr(g, "generate") and hasattr(g.Denoiser, "generate") and g.GENERATE_STREAM == 5


def test_a_plan_records_both_calls():
    """the plan's entry table carries both entries with their arity (nothing runs: execute=False)"""
    import gan_class_transfer2_amd as g
    L = g._lib
    plan = L.Plan()
    plan.begin(execute=False)
    try:
        L.call("gct2_diffusion_start", 0, 1, 5, 0, 12, 64, 64, 4, None, 0, 1, 12, 3, None)
        L.call("gct2_diffusion_step", 0, 0, 64, 64, 0.1, 0.2, 0.0, 0.0, 1, 5, 0, 12, 64, None, 64, 4, None, 0, 1, 12, 3, None)
    finally:
        plan.end()
    assert plan.n == 2


# ---- what generate refuses before any launch -------------------------------------------------------------------------------------------------

def fake_denoiser(**switches):
    """an engine that has nothing but what generate reads before it launches: touching anything else is an AttributeError"""
    kw = dict(predict_x=True, predict_scaled_epsilon=False, ordinary_differential_equation=False)
    kw.update(switches)
    eng = types.SimpleNamespace(steps=6, noise_schedule="quadratic", alpha_dash_offset=0.0, **kw)
    return types.SimpleNamespace(ensure_engine=lambda: eng)


def test_generate_refuses_bad_arguments():
    import torch
    import gan_class_transfer2_amd as g
    den = fake_denoiser()
    with pytest.raises(ValueError, match="ordinary_differential_equation"):
        g.generate(fake_denoiser(ordinary_differential_equation=True), 2, ordinary_differential_equation=True, size=16)
    for kw, what in ((dict(eta=-0.1), "eta"), (dict(eta=float("nan")), "eta"), (dict(num_steps=7), "num_steps"), (dict(num_steps=0), "num_steps"),
                     (dict(timesteps=[2, 2, 5]), "timesteps"), (dict(timesteps=[3, 2]), "timesteps"), (dict(timesteps=[0, 2]), "timesteps"),
                     (dict(timesteps=[2, 7]), "timesteps"), (dict(timesteps=[]), "timesteps"), (dict(timesteps=[1.5, 2]), "timesteps"),
                     (dict(timesteps=[2, 4], num_steps=3), "num_steps"), (dict(noise=torch.zeros(3, 16, 16, 3)), "noise"),
                     (dict(noise=torch.zeros(2, 16, 16, 4)), "noise"), (dict(noise=torch.zeros(2, 16, 16)), "noise"),
                     (dict(clip_denoised=-1.0), "clip_denoised"), (dict(return_steps=[5], num_steps=3), "return_steps"),
                     (dict(batch_size=0), "batch_size"), (dict(first_index=-1), "first_index")):
        with pytest.raises(ValueError, match=what):
            g.generate(den, 2, size=16, **kw)
    with pytest.raises(ValueError, match="n must"):
        g.generate(den, 0, size=16)
    with pytest.raises(ValueError):                                    # the engine was set up for another objective
        g.generate(den, 2, size=16, predict_x=False)
