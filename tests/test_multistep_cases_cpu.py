"""The second-order multistep sampler without a GPU: the host math (trainer_math.half_log_snr / multistep_coefficient), what the
restatements of tests/multistep_cases.py compute (the DDIM step's bits at c1 = 0, the paper's DPM-Solver++ 2M step, the order of
accuracy the GPU test asks of the kernel), the new entry point in the header, the binding, the plan table and the built library,
and the arguments generate / encode refuse before they launch anything."""
import math
import os
import re
import types

import numpy as np
import pytest

import generate_cases as G
import img2img_cases as I
import multistep_cases as MC
import pointwise_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "gct2_diffusion_step_multistep"


def tm():
    import gan_class_transfer2_amd as g
    return g.trainer_math


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    """bit equality, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the host math ---------------------------------------------------------------------------------------------------------------------------

def test_half_log_snr():
    M = tm()
    assert M.SOLVERS == ("ddim", "dpm2m")
    assert M.half_log_snr(0.5) == 0.0
    for a in (1e-5, 0.1, 0.3, 0.9, 0.999):
        assert M.half_log_snr(a) == 0.5 * math.log(a / (1.0 - a)) == MC.half_log_snr(a)
        assert math.isclose(M.half_log_snr(a), math.log(math.sqrt(a) / math.sqrt(1.0 - a)), rel_tol=1e-12, abs_tol=1e-12)
    assert M.half_log_snr(0.0) == M.half_log_snr(-0.1) == -math.inf
    assert M.half_log_snr(1.0) == M.half_log_snr(1.5) == math.inf


def alpha_at(lam):
    """the alpha whose half-log-SNR is lam"""
    return 1.0 / (1.0 + math.exp(-2.0 * lam))


def test_multistep_coefficient():
    M = tm()
    c = M.multistep_coefficient
    down = [alpha_at(l) for l in (-2.0, -1.5, -1.0)]                   # uniform spacing in lambda, towards the image (generate)
    assert math.isclose(c(*down), 0.5, rel_tol=1e-9)
    assert math.isclose(c(*down[::-1]), 0.5, rel_tol=1e-9)             # and towards the noise (encode)
    a, b, d = alpha_at(-2.0), alpha_at(-1.0), alpha_at(-0.25)          # h_prev = 1, h = 0.75
    assert math.isclose(c(a, b, d), 0.375, rel_tol=1e-9)
    # no history, or an end of the process among the three: the first-order step
    assert c(None, 0.2, 0.3) == 0.0
    for triple in ((0.0, 0.2, 0.3), (0.1, 0.0, 0.3), (0.1, 0.2, 0.0), (1.0, 0.2, 0.1), (0.3, 1.0, 0.1), (0.3, 0.2, 1.0)):
        assert c(*triple) == 0.0, triple
    assert c(0.2, 0.2, 0.3) == 0.0                                     # h_prev == 0
    # ascending equals descending on mirrored alphas: lambda(1 - a) = -lambda(a)
    for a0, a1, a2 in ((0.05, 0.2, 0.5), (0.3, 0.31, 0.7), (1e-5, 1e-3, 0.1)):
        assert math.isclose(c(a0, a1, a2), c(1.0 - a0, 1.0 - a1, 1.0 - a2), rel_tol=1e-9)
        assert c(a0, a1, a2) > 0.0 and c(a2, a1, a0) > 0.0             # monotone either way: c1 > 0
    # the project's schedules: every step of a strided run in both directions
    for schedule in M.NOISE_SCHEDULES:
        taus = M.sampling_timesteps(200, 7)
        al = [float(M.alpha_dash(t, 200, schedule, 0.0)) for t in taus]
        for k in range(1, len(al) - 1):
            assert c(al[k - 1], al[k], al[k + 1]) > 0.0 and c(al[k + 1], al[k], al[k - 1]) > 0.0
        assert c(al[-2], al[-1], 0.0) == 0.0                           # encode's last step goes to alpha 0: the helper returns 0 by itself


# ---- the restatements --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_restatement_at_c1_zero_is_the_ddim_step(mode):
    """c1 = 0: generate_cases.diffusion_step_f32 at sigma2 = 0 bit for bit, whatever hist holds; hist_out is the clipped estimate;
    with a mask, img2img_cases.step_masked_f32"""
    p, f = G.clip_case()
    nan_hist = np.full_like(p, np.nan)
    kn, el = I.known_case(*p.shape), I.per_element(I.mask_case("pattern", p.shape[0], p.shape[1] // G.C), G.C)
    z0 = G.step_case(p.shape[0], p.shape[1])[1]
    for t in P.DIFFUSION_TS:
        a_t, a_prev = G.alphas(t)
        for clip in MC.CLIPS:
            want, x = G.diffusion_step_f32(mode, p, f, a_t, a_prev, 0.0, clip)
            for hist in (None, nan_hist):
                got, x0, h_out = MC.multistep_step_f32(mode, p, f, hist, a_t, a_prev, 0.0, clip)
                assert same_bits(got, want) and same_bits(x0, x) and same_bits(h_out, x)
            want_m, x_m = I.step_masked_f32(mode, p, f, kn, el, a_t, a_prev, 0.0, clip, z0)
            got, x0, h_out = MC.multistep_step_f32(mode, p, f, nan_hist, a_t, a_prev, 0.0, clip, kn, el, z0)
            assert same_bits(got, want_m) and same_bits(x0, x_m) and same_bits(h_out, x)


def test_restatement_extrapolates_and_tells_a_fused_multiply_add():
    """c1 != 0 changes the state (not the estimate), and d = fma(c, x - hist, x) is not what the restatement computes at c1 = 1.37"""
    p, f = G.step_case(G.B, G.NPIXS[0] * G.C)
    hist = MC.hist_case(*p.shape)
    a_t, a_prev = G.alphas(37)
    base, x, _ = MC.multistep_step_f32(P.SAMPLE_X, p, f, hist, a_t, a_prev, 0.0, 0.0)
    for c1 in MC.C1S[1:]:
        got, x0, h_out = MC.multistep_step_f32(P.SAMPLE_X, p, f, hist, a_t, a_prev, c1, 0.0)
        assert same_bits(x0, x) and same_bits(h_out, x) and not same_bits(got, base)
        # float64 on the same float32 inputs: the extrapolated form
        sa, sb = np.float64(np.float32(np.sqrt(a_t))), np.float64(np.float32(np.sqrt(1 - a_t)))
        d = p.astype(np.float64) * (1 + np.float64(np.float32(c1))) - np.float64(np.float32(c1)) * hist
        ref = np.sqrt(np.float64(np.float32(a_prev))) * d + np.sqrt(1 - np.float64(np.float32(a_prev))) * (f - sa * d) / sb
        assert np.abs(got - ref).max() < 2e-5 * (1 + np.abs(ref).max())
    fused, _, _ = MC.multistep_step_fused(P.SAMPLE_X, p, f, hist, a_t, a_prev, 1.37, 0.0)
    plain, _, _ = MC.multistep_step_f32(P.SAMPLE_X, p, f, hist, a_t, a_prev, 1.37, 0.0)
    assert (bits(fused) != bits(plain)).sum() > 0


def test_extrapolated_form_is_the_papers():
    """cx D + ce (x - sa D) / sb with D = x0 + c1 (x0 - x0_prev), c1 = multistep_coefficient, equals DPM-Solver++ 2M's
    (sigma' / sigma) x - alpha' (exp(-h) - 1) D with D = (1 + 1 / (2 r)) x0 - 1 / (2 r) x0_prev within 1e-12, in both directions"""
    M = tm()
    rng = np.random.default_rng(67)
    x_t, x0, x0_prev = (rng.standard_normal(64) for _ in range(3))
    al = [MC.order_alpha(t) for t in (200, 180, 170, 120, 60, 20, 1)]
    for seq in (al, al[::-1]):
        for a_before, a_t, a_prev in zip(seq, seq[1:], seq[2:]):
            c1 = M.multistep_coefficient(a_before, a_t, a_prev)
            assert c1 > 0
            paper = MC.dpm2m_step_paper_f64(x_t, x0, x0_prev, a_before, a_t, a_prev)
            ours = MC.dpm2m_step_extrapolated_f64(x_t, x0, x0_prev, c1, a_t, a_prev)
            assert np.abs(paper - ours).max() <= 1e-12 * max(1.0, np.abs(paper).max()), (a_before, a_t, a_prev)
        first = MC.dpm2m_step_paper_f64(x_t, x0, None, None, seq[1], seq[2])
        assert np.abs(first - MC.dpm2m_step_extrapolated_f64(x_t, x0, None, 0.0, seq[1], seq[2])).max() <= 1e-12
        # the first-order step of the paper is the DDIM step
        ddim, _ = G.ddim_step_f64(P.SAMPLE_X, x0, x_t, seq[1], seq[2], 0.0, 0.0)
        assert np.abs(first - ddim).max() <= 1e-12


def test_exact_flow_solves_the_ode_of_the_optimal_denoiser():
    """the Gaussian model's closed forms agree: many small first-order steps with the optimal denoiser converge to exact_flow"""
    mu, s, x_T = MC.gaussian_case()
    assert mu.shape == (MC.ORDER_SHAPE[0], MC.ORDER_SHAPE[1] * MC.ORDER_SHAPE[2])
    assert mu.min() >= -0.5 and mu.max() <= 0.5 and s.min() >= 0.2 and s.max() <= 0.8
    ts = list(range(MC.ORDER_HIGH, MC.ORDER_LOW - 1, -1))
    x = x_T.copy()
    for t, t1 in zip(ts, ts[1:]):
        a_t, a_prev = MC.order_alpha(t), MC.order_alpha(t1)
        x0 = mu + MC.denoiser_gain(a_t, s) * (x - math.sqrt(a_t) * mu)
        x = MC.dpm2m_step_paper_f64(x, x0, None, None, a_t, a_prev)
    exact = MC.exact_flow(MC.order_alpha(MC.ORDER_LOW), MC.order_alpha(MC.ORDER_HIGH), x_T, mu, s)
    assert np.abs(x - exact).max() < 1e-3


@pytest.mark.parametrize("ascending", [False, True], ids=["descending", "ascending"])
@pytest.mark.parametrize("mode", MC.ORDER_MODES, ids=["x", "eps"])
def test_restatement_meets_the_order_conditions(mode, ascending):
    """the float32 restatement on the seeded arrays the GPU test uses: first order halves its error with the step, second order
    takes it down by more than 3, and 19 second-order timesteps beat 37 first-order ones"""
    c = tm().multistep_coefficient
    E1 = {len(MC.order_timesteps(d)): MC.order_error_f32(mode, d, ascending, False, c) for d in MC.ORDER_STRIDES}
    E2 = {len(MC.order_timesteps(d)): MC.order_error_f32(mode, d, ascending, True, c) for d in MC.ORDER_STRIDES}
    assert sorted(E1) == [10, 19, 37]
    MC.order_conditions(E1, E2)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------

def test_new_entry_point_everywhere():
    import gan_class_transfer2_amd as g
    L = g._lib
    raw = L.load()
    assert L.ABI_VERSION == 17 and raw.gct2_abi_version() == 17       # an addition changes no signature
    header = open(os.path.join(ROOT, "include", "gct2.h")).read()
    plan = open(os.path.join(ROOT, "gan-class-transfer2_amd", "csrc", "plan.hip")).read()
    proto = re.search(r"\bint " + NEW + r"\(([^;]*)\);", header)
    assert proto
    assert len(proto.group(1).split(",")) == len(L.SIGNATURES[NEW]) == 26 <= 28                # plan.hip MAX_ARGS
    assert NEW in L.PLANNABLE and hasattr(raw, NEW) and f"GCT2_ENTRY({NEW})" in plan
    sig = L.SIGNATURES[NEW]
    assert sig[-1] is L._vp and sig[7:11] == [L._d] * 4 and sig[11:15] == [L._u64] * 4        # a_t, a_prev, c1, clip; seed .. image_stride
    for word in ("hist_out[i] = x", "d = x + c * (x - hist_in[i])", "ed = (fake_in[i] - sa d) / sb", "g = cx d + ce ed"):
        assert word in header, word
    for name in ("SOLVERS", "half_log_snr", "multistep_coefficient"):
        assert getattr(g, name) is getattr(g.trainer_math, name)


def test_a_plan_records_the_call():
    import gan_class_transfer2_amd as g
    L = g._lib
    plan = L.Plan()
    plan.begin(execute=False)
    try:
        L.call(NEW, 0, 0, 64, 64, 64, None, None, 0.1, 0.2, 0.5, 0.0, 1, 5, 0, 12, 64, 64, None, 64, 4, None, 0, 1, 12, 3, None)
    finally:
        plan.end()
    assert plan.n == 1


# ---- what generate and encode refuse before any launch ---------------------------------------------------------------------------------------

def fake_denoiser(**switches):
    """an engine that has nothing but what generate reads before it launches: touching anything else is an AttributeError"""
    kw = dict(predict_x=True, predict_scaled_epsilon=False, ordinary_differential_equation=False)
    kw.update(switches)
    eng = types.SimpleNamespace(steps=6, noise_schedule="quadratic", alpha_dash_offset=0.0, **kw)
    return types.SimpleNamespace(ensure_engine=lambda: eng)


def test_generate_and_encode_refuse_bad_solver_arguments():
    import inspect
    import torch
    import gan_class_transfer2_amd as g
    den = fake_denoiser()
    img = torch.zeros(2, 16, 16, 3)
    assert inspect.signature(g.generate).parameters["solver"].default == "ddim"
    assert inspect.signature(g.encode).parameters["solver"].default == "ddim"
    for bad in ("heun", "DPM2M", "", None, 2):
        with pytest.raises(ValueError, match="solver"):
            g.generate(den, 2, size=16, solver=bad)
        with pytest.raises(ValueError, match="solver"):
            g.encode(den, img, solver=bad)
    for eta in (0.5, 1.0):
        with pytest.raises(ValueError, match="eta"):
            g.generate(den, 2, size=16, solver="dpm2m", eta=eta)
    with pytest.raises(ValueError, match="eta"):
        g.generate(den, 2, size=16, solver="dpm2m", eta=-1.0)
    # the ODE objective stays refused, and every other refusal comes before any launch with the new solver too
    with pytest.raises(ValueError, match="ordinary_differential_equation"):
        g.generate(fake_denoiser(ordinary_differential_equation=True), 2, ordinary_differential_equation=True, size=16, solver="dpm2m")
    with pytest.raises(ValueError, match="ordinary_differential_equation"):
        g.encode(fake_denoiser(ordinary_differential_equation=True), img, ordinary_differential_equation=True, solver="dpm2m")
    for kw, what in ((dict(num_steps=7), "num_steps"), (dict(timesteps=[3, 2]), "timesteps"), (dict(mask=torch.ones(16, 16)), "init"),
                     (dict(strength=0.5), "init"), (dict(return_steps=[5], num_steps=3), "return_steps")):
        with pytest.raises(ValueError, match=what):
            g.generate(den, 2, size=16, solver="dpm2m", **kw)
    with pytest.raises(ValueError, match="num_steps"):
        g.encode(den, img, solver="dpm2m", num_steps=7)
