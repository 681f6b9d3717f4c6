"""Image-conditioned generation without a GPU: trainer_math.img2img_steps / check_mask, what the restatements of
tests/img2img_cases.py state and can tell apart, the two new entry points in the header, the binding, the plan table and the built
library, and the arguments generate / encode refuse before they launch anything."""
import os
import re
import types

import numpy as np
import pytest

import generate_cases as G
import img2img_cases as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gct2_diffusion_step_masked", "gct2_diffusion_start_image")


def tm():
    import gan_class_transfer2_amd as g
    return g.trainer_math


def test_img2img_steps():
    S = tm().img2img_steps
    assert [S(6, s) for s in (1.0, 0.5, 0.4, 0.01, 0.99, 0.75)] == [6, 3, 2, 1, 6, 5]
    assert S(50, 0.5) == 25 and S(50, 0.3) == 15 and S(1, 0.2) == 1 and S(200, 1) == 200 and S(3, 0.5) == 2
    for K in (1, 2, 7, 50):
        got = [S(K, s) for s in np.linspace(0.001, 1.0, 97)]
        assert got == sorted(got) and got[0] == 1 and got[-1] == K
    for bad in (0.0, -0.5, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="strength"):
            S(6, bad)


def test_check_mask():
    import torch
    M = tm().check_mask
    n, H, W = 3, 4, 5
    one = torch.arange(H * W, dtype=torch.float64).reshape(H, W)
    got = M(one, n, H, W)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, H, W) and got.is_contiguous()
    assert all(torch.equal(got[i], one.float()) for i in range(n))
    each = torch.rand(n, H, W)
    assert torch.equal(M(each, n, H, W), each) and torch.equal(M(each[..., None], n, H, W), each)
    assert M(each.permute(0, 2, 1).contiguous().permute(0, 2, 1), n, H, W).is_contiguous()
    assert torch.equal(M(np.ones((H, W), bool), n, H, W), torch.ones(n, H, W))
    for shape in ((W, H), (n + 1, H, W), (n, H, W, 3), (1, H, W), (n, H, W, 1, 1), (H * W,), ()):
        with pytest.raises(ValueError, match="mask"):
            M(torch.zeros(shape), n, H, W)
    # n = 1: [1,H,W] is the per-image form
    assert tuple(M(torch.zeros(1, H, W), 1, H, W).shape) == (1, H, W)


def _case(eta):
    per = G.NPIXS[0] * G.C
    pred, fake = G.step_case(G.B, per)
    known = I.known_case(G.B, per)
    rng = np.random.default_rng(59)
    z0, z = (rng.standard_normal(pred.shape).astype(np.float32) for _ in range(2))
    a_t, a_prev = G.alphas(37)
    return pred, fake, known, z0, z, a_t, a_prev, G.sigma2(a_t, a_prev, eta)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_all_ones_is_the_plain_step_and_all_zeros_keeps_the_image(mode, eta):
    pred, fake, known, z0, z, a_t, a_prev, s2 = _case(eta)
    want, x = G.diffusion_step_f32(mode, pred, fake, a_t, a_prev, s2, 1.0, z)
    ones = I.per_element(I.mask_case("ones", G.B, G.NPIXS[0]), G.C)
    got, x0 = I.step_masked_f32(mode, pred, fake, known, ones, a_t, a_prev, s2, 1.0, z0, z)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(x0), bits(x))
    zeros = I.per_element(I.mask_case("zeros", G.B, G.NPIXS[0]), G.C)
    p = pred.copy()
    p[:, :8] = np.float32([np.nan, np.inf, -np.inf, 1e38, -1e38, 0, 1, -1])        # nothing of the prediction reaches a kept pixel
    got, x0 = I.step_masked_f32(mode, p, fake, known, zeros, a_t, a_prev, s2, 0.0, z0, z)
    assert np.array_equal(bits(x0), bits(known)) and np.array_equal(bits(got), bits(I.kept_f32(known, a_prev, z0)))
    assert np.array_equal(bits(I.kept_f32(known, a_prev, z0)), bits(I.start_image_f32(known, a_prev, z0)))


def test_start_image_is_mix_of_the_draw():
    import pointwise_cases as P
    _, _, known, z0, _, a_t, _, _ = _case(0.0)
    for a in (a_t, 0.0, 1.0, 0.25, 1e-3):
        assert np.array_equal(bits(I.start_image_f32(known, a, z0)), bits(P.diffusion_mix_f32(known, z0, a)))


@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_pattern_mask_per_pixel_and_against_float64(mode):
    pred, fake, known, z0, z, a_t, a_prev, s2 = _case(0.7)
    m = I.mask_case("pattern", G.B, G.NPIXS[0])
    assert all(np.array_equal(m[b, :8], np.float32(I.PATTERN), equal_nan=True) and np.array_equal(m[b, -8:], np.float32(I.PATTERN), equal_nan=True)
               for b in range(G.B))
    el = I.per_element(m, G.C)
    assert el.shape == pred.shape and np.array_equal(el[0, :6], np.float32([0, 0, 0, 1, 1, 1]))
    got, x0 = I.step_masked_f32(mode, pred, fake, known, el, a_t, a_prev, s2, 1.0, z0, z)
    g, x = G.diffusion_step_f32(mode, pred, fake, a_t, a_prev, s2, 1.0, z)
    h = I.kept_f32(known, a_prev, z0)
    full, kept, nan = el >= 1, el <= 0, np.isnan(el)
    assert full.sum() and kept.sum() and nan.sum() and (el == np.float32(1e-30)).sum()
    assert np.array_equal(bits(got[full]), bits(g[full])) and np.array_equal(bits(x0[full]), bits(x[full]))          # 1 and 1.5
    assert np.array_equal(bits(got[kept]), bits(h[kept])) and np.array_equal(bits(x0[kept]), bits(known[kept]))      # 0 and -0.5
    assert np.isnan(got[nan]).all() and np.isnan(x0[nan]).all()
    tiny = el == np.float32(1e-30)                      # 1 - m rounds to 1: h + m g, within half an ulp of h
    assert np.abs(got[tiny] - h[tiny]).max() <= 1e-29 * np.abs(g[tiny]).max() + np.spacing(np.abs(h[tiny])).max()
    # float32 rounding of the float64 blended step on the finite masks: the step's own error (generate_cases' bound style: a few ulp
    # of the largest term) plus three roundings of the blend
    ok = ~nan
    w, wx = I.step_masked_f64(mode, pred, fake, known, np.where(nan, 0, el), a_t, a_prev, s2, 1.0, z0, z)
    scale = np.abs(g.astype(np.float64)) + np.abs(h.astype(np.float64)) + 1.0
    assert (np.abs(got.astype(np.float64) - w)[ok] <= 16 * 2.0 ** -24 * scale[ok] * (1 + 1 / np.sqrt(a_t))).all()
    assert (np.abs(x0.astype(np.float64) - wx)[ok] <= 16 * 2.0 ** -24 * (1 + 1 / np.sqrt(a_t))).all()
    # the contracted blends differ on blended pixels and nowhere else, so the GPU test can tell them apart.  m g is exact for m = 0.5 and
    # 0.25 (and 0.5 h too): fma(m, g, fl((1 - m) h)) IS the unfused blend there and shows only at 0.3 / 0.7; fma(1 - m, h, fl(m g))
    # shows at 0.25 (0.75 h is inexact) as well
    quarter, other = el == 0.25, (el == np.float32(0.3)) | (el == np.float32(0.7))
    part = quarter | other | (el == 0.5)
    for term in (0, 1):
        f, _ = I.step_masked_f32(mode, pred, fake, known, el, a_t, a_prev, s2, 1.0, z0, z, blend=lambda m_, g_, h_: I.blend_fused(m_, g_, h_, term))
        differ = bits(f) != bits(got)
        assert differ[other].sum() > 0 and not differ[~part & ok].any() and not differ[el == 0.5].any()
        assert differ[quarter].sum() > 0 if term == 1 else not differ[quarter].any()


def test_float64_loops_agree_with_the_plain_sampler():
    """all-ones in float64 is ddim_sample_f64 from the noised image; all-zeros returns the image; invert_f64 of a perfect eps predictor
    returns eps"""
    rng = np.random.default_rng(61)
    shape = (2, 4, 4, 3)
    known, z0 = rng.uniform(-1, 1, shape), rng.standard_normal(shape)
    z = rng.standard_normal((3,) + shape)
    net = lambda fake, t: np.tanh(fake * 0.5 + t * 0.01)
    taus, steps = [2, 4, 6], 6
    for run in (3, 2, 1):
        a0 = float(I.O.alpha_dash(taus[run - 1], steps))
        start = np.sqrt(a0) * known + np.sqrt(1 - a0) * z0
        want = G.ddim_sample_f64(net, start, taus[:run], steps, G.SAMPLE_X, eta=0.7, clip=1.0, z=z[3 - run:])
        got = I.masked_sample_f64(net, known, np.ones(shape), z0, taus, steps, G.SAMPLE_X, run=run, eta=0.7, clip=1.0, z=z)
        assert np.allclose(got, want, rtol=0, atol=1e-14)
        assert np.array_equal(I.masked_sample_f64(net, known, np.zeros(shape), z0, taus, steps, G.SAMPLE_X, run=run, eta=0.7, z=z), known)
    eps = rng.standard_normal(shape)
    assert np.allclose(I.invert_f64(lambda fake, t: eps, known, taus, steps, G.SAMPLE_EPS), eps, rtol=0, atol=1e-12)
    # a perfect x predictor: x stays the image, e stays start_eps (fake = sa x + sb e, e' = (fake - sa x) / sb)
    assert np.allclose(I.invert_f64(lambda fake, t: known, known, taus, steps, G.SAMPLE_X, start_eps=eps), eps, rtol=0, atol=1e-12)
    assert np.allclose(I.invert_f64(lambda fake, t: known, known, taus, steps, G.SAMPLE_X), known, rtol=0, atol=1e-12)


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
    step, masked = L.SIGNATURES["gct2_diffusion_step"], L.SIGNATURES[NEW[0]]
    # the step's arguments plus known, mask (behind fake_in) and offset0 (behind offset)
    assert masked == step[:4] + [L._vp, L._vp] + step[4:11] + [L._u64] + step[11:]
    assert L.SIGNATURES[NEW[1]] == [L._i, L._vp, L._d] + L.SIGNATURES["gct2_diffusion_start"][1:]
    for name in ("encode", "generate", "img2img_steps", "check_mask"):
        assert hasattr(g, name), name
    assert hasattr(g.Denoiser, "encode") and hasattr(g.Denoiser, "generate")


def fake_denoiser(**switches):
    kw = dict(predict_x=True, predict_scaled_epsilon=False, ordinary_differential_equation=False)
    kw.update(switches)
    eng = types.SimpleNamespace(steps=6, noise_schedule="quadratic", alpha_dash_offset=0.0, **kw)
    return types.SimpleNamespace(ensure_engine=lambda: eng)


def test_generate_and_encode_refuse_bad_arguments():
    import torch
    import gan_class_transfer2_amd as g
    den = fake_denoiser()
    img = torch.zeros(2, 16, 16, 3)
    for kw, what in ((dict(mask=torch.ones(16, 16)), "init"), (dict(strength=0.5), "init"),
                     (dict(init=img, noise=torch.zeros(2, 16, 16, 3)), "noise"),
                     (dict(init=torch.zeros(3, 16, 16, 3)), "init"), (dict(init=torch.zeros(2, 16, 16, 4)), "init"),
                     (dict(init=torch.zeros(2, 16, 16)), "init"), (dict(init=img, size=8), "init"),
                     (dict(init=img, strength=0.0), "strength"), (dict(init=img, strength=1.5), "strength"),
                     (dict(init=img, strength=-1.0), "strength"), (dict(init=img, strength=float("nan")), "strength"),
                     (dict(init=img, mask=torch.ones(8, 16)), "mask"), (dict(init=img, mask=torch.ones(2, 16, 16, 3)), "mask"),
                     (dict(init=img, strength=0.5, num_steps=6, return_steps=[4]), "return_steps")):
        with pytest.raises(ValueError, match=what):
            g.generate(den, 2, **kw)
    with pytest.raises(ValueError, match="ordinary_differential_equation"):
        g.encode(fake_denoiser(ordinary_differential_equation=True), img, ordinary_differential_equation=True)
    for kw, what in ((dict(num_steps=7), "num_steps"), (dict(timesteps=[3, 2]), "timesteps"), (dict(batch_size=0), "batch_size"),
                     (dict(start_eps=torch.zeros(2, 16, 16)), "start_eps")):
        with pytest.raises(ValueError, match=what):
            g.encode(den, img, **kw)
    with pytest.raises(ValueError, match="images"):
        g.encode(den, torch.zeros(2, 16, 16))
