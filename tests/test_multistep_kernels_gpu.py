"""gct2_diffusion_step_multistep, ELEMENT BY ELEMENT and bit for bit (+0 == -0, NaN == NaN) against tests/multistep_cases.py's
restatement (the masked form fed the draws gct2_rng_normal makes at the documented stream elements) and against the GPU's own
gct2_diffusion_step / gct2_diffusion_step_masked where nothing is extrapolated; every output is a view with pixel stride ld inside a
sentinel-filled buffer (tests/test_generate_kernels_gpu.py's View / Outputs) that must be unchanged around the view after each call.
Then the kernel as an integrator: its order of accuracy on a Gaussian data model whose probability-flow ODE has a closed-form solution."""
import numpy as np
import pytest
import torch

import exact_cases as E
import generate_cases as G
import img2img_cases as I
import multistep_cases as MC
import pointwise_cases as P
import test_generate_kernels_gpu as TG
import test_img2img_kernels_gpu as TI
from exact_cases import BF16, F16, F32, SENTINEL
from test_generate_kernels_gpu import DTS, DT_IDS, Outputs, View, dev, draws, lib, stream

pytestmark = pytest.mark.gpu
NEW = "gct2_diffusion_step_multistep"
FORMS = ("plain", "masked")


class MOutputs(Outputs):
    """Outputs and the history plane"""

    def __init__(self, shape, dt, gpu, x0=True, out2=True, fake=None, hist=None, hist_out=True):
        super().__init__(shape, dt, gpu, x0=x0, out2=out2, fake=fake)
        self.hist = View(shape, torch.float32, gpu, values=hist) if hist_out else None

    def check(self, dt, fake_want, x0_want, hist_want, what):
        super().check(dt, fake_want, x0_want, what)
        if self.hist is not None:
            self.hist.check(hist_want, what + ": hist_out")


def multistep(mode, dt, pred, fake_in_ptr, hist_in_ptr, known, mask, a_t, a_prev, c1, clip, off0, stride, o, shape, seed=G.SEED, sid=G.SID):
    B, npix, C = shape
    lib().call(NEW, mode, dt, pred.data_ptr(), fake_in_ptr, hist_in_ptr, known.data_ptr() if known is not None else None,
               mask.data_ptr() if mask is not None else None, a_t, a_prev, c1, clip, seed, sid, off0, stride, o.fake.ptr,
               o.hist.ptr if o.hist else None, o.x0.ptr if o.x0 else None, *o.views(), B, npix * C, C, stream())


def inputs(gpu, shape, form, kind="pattern"):
    """host (pred, fake, hist, known, mask per element), device (pred, fake, hist, known, mask per pixel); known / mask None: plain"""
    B, npix, C = shape
    p, f = MC.step_inputs(shape)
    h = MC.hist_case(B, npix * C)
    if form == "plain":
        return (p, f, h, None, None), (dev(p, gpu), dev(f, gpu), dev(h, gpu), None, None)
    kn, m = I.known_case(B, npix * C), I.mask_case(kind, B, npix)
    return (p, f, h, kn, I.per_element(m, C)), tuple(dev(a, gpu) for a in (p, f, h, kn, m))


COMBOS = [(clip, c1) for clip in MC.CLIPS for c1 in MC.C1S]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_multistep_per_element(gpu, dt, mode, shape, form):
    """clip off / 1.0 / 0.5 on generate_cases.CLIP_SPECIALS (beyond, on and just past the bounds, a NaN, both infinities) times
    c1 = 0 / 0.5 / 1.37, over the timesteps 1, 37, 199, 200; views with ldout 4 and 67 in f32 / bf16 / f16; the masked form with the
    pattern mask and the starting noise at offset0 = 0, 1, 2, 3, 5 and across the wrap of the low counter word, images an
    image_stride apart that is no multiple of 4.  The long shape takes the second trip of the grid-stride loop"""
    B, npix, C = shape
    per = npix * C
    (p, f, h, kn, el), (pred, fake, hist, known, mask) = inputs(gpu, shape, form)
    stride = G.image_stride(per)
    extrapolated = 0
    for k, (clip, c1) in enumerate(COMBOS):
        t = P.DIFFUSION_TS[k % len(P.DIFFUSION_TS)]
        off0 = G.OFFSETS[k % len(G.OFFSETS)]
        a_t, a_prev = G.alphas(t)
        z0 = draws(gpu, shape, off0, stride) if form == "masked" else None
        o = MOutputs(shape, dt, gpu, out2=per < 1000000 or k == 0)
        multistep(mode, dt, pred, fake.data_ptr(), hist.data_ptr(), known, mask, a_t, a_prev, c1, clip, off0, stride, o, shape)
        want, x0, hx = MC.multistep_step_f32(mode, p, f, h, a_t, a_prev, c1, clip, kn, el, z0)
        if c1:
            base, _, _ = MC.multistep_step_f32(mode, p, f, h, a_t, a_prev, 0.0, clip, kn, el, z0)
            extrapolated += int((base.view(np.int32) != want.view(np.int32)).sum())
        o.check(dt, torch.tensor(want), torch.tensor(x0), torch.tensor(hx),
                f"{NEW} {form} {E.DTYPE_NAMES[dt]} mode {mode} t {t} clip {clip} c1 {c1} offset0 {off0} shape {shape}")
    assert extrapolated > per                                      # (the cases with c1 != 0 are not the DDIM step)


def test_extrapolation_is_not_contracted(gpu):
    """d = x + c (x - hist) with the product rounded on its own: fma(c, x - hist, x) differs from what the kernel stored at c1 = 1.37"""
    shape = (G.B, G.NPIXS[0], G.C)
    p, f = G.step_case(G.B, shape[1] * G.C)
    h = MC.hist_case(G.B, shape[1] * G.C)
    a_t, a_prev = G.alphas(37)
    o = MOutputs(shape, F32, gpu)
    pred, fake, hist = dev(p, gpu), dev(f, gpu), dev(h, gpu)
    multistep(P.SAMPLE_X, F32, pred, fake.data_ptr(), hist.data_ptr(), None, None, a_t, a_prev, 1.37, 0.0, 0, 0, o, shape)
    got = o.fake.got().numpy().reshape(p.shape)
    fused, _, _ = MC.multistep_step_fused(P.SAMPLE_X, p, f, h, a_t, a_prev, 1.37, 0.0)
    plain, _, _ = MC.multistep_step_f32(P.SAMPLE_X, p, f, h, a_t, a_prev, 1.37, 0.0)
    assert (fused.view(np.int32) != got.view(np.int32)).sum() > 0
    assert (plain.view(np.int32) == got.view(np.int32)).all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_in_place_and_null_outputs(gpu, mode, form):
    """fake_out == fake_in and hist_out == hist_in: the bits of the out-of-place run (a thread reads its element of both planes before
    it writes it); hist_out, x0_out and out2 may be NULL"""
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    _, (pred, fake, hist, known, mask) = inputs(gpu, shape, form, "half")
    stride, off0 = G.image_stride(per), 3 + 5 * per
    a_t, a_prev = G.alphas(199)
    for c1 in (0.0, 1.37):
        apart = MOutputs(shape, F16, gpu)
        multistep(mode, F16, pred, fake.data_ptr(), hist.data_ptr(), known, mask, a_t, a_prev, c1, 1.0, off0, stride, apart, shape)
        want, x, hx = apart.fake.got(), apart.x0.got(), apart.hist.got()
        finite = torch.isfinite(want)
        assert finite.sum() > want.numel() - 100 and float(want[finite].abs().max()) > 0
        assert float(hx[torch.isfinite(hx)].abs().max()) <= 1.0            # the clipped estimate
        in_place = MOutputs(shape, F16, gpu, fake=fake, hist=hist)
        multistep(mode, F16, pred, in_place.fake.ptr, in_place.hist.ptr, known, mask, a_t, a_prev, c1, 1.0, off0, stride, in_place, shape)
        in_place.check(F16, want, x, hx, f"in place, {form} mode {mode} c1 {c1}")
        bare = MOutputs(shape, F16, gpu, x0=False, out2=False, hist_out=False)
        multistep(mode, F16, pred, fake.data_ptr(), hist.data_ptr(), known, mask, a_t, a_prev, c1, 1.0, off0, stride, bare, shape)
        bare.check(F16, want, None, None, f"null hist_out, x0_out and out2, {form} mode {mode} c1 {c1}")


@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_c1_zero_is_the_existing_step(gpu, mode):
    """c1 = 0 with hist_in NULL and with a NaN-filled hist_in: fake', x0_out and both views are the bits of gct2_diffusion_step at
    sigma2 = 0 and of gct2_diffusion_step_masked, calls made here on the same inputs (CLIP_SPECIALS in pred, with and without the clip);
    hist_out is the plain step's x0_out"""
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    stride, off0 = G.image_stride(per), 2 + 7 * per
    a_t, a_prev = G.alphas(199)
    nan_hist = torch.full((G.B, per), float("nan"), device=gpu)
    _, (pred, fake, _, known, mask) = inputs(gpu, shape, "masked")
    for clip in (0.0, 1.0):
        plain = Outputs(shape, BF16, gpu)
        TG.step(mode, BF16, pred, fake.data_ptr(), a_t, a_prev, 0.0, clip, 0, 0, plain, shape)
        want, x = plain.fake.got(), plain.x0.got()
        assert torch.isnan(want).any()
        kept = Outputs(shape, BF16, gpu)
        TI.masked(mode, BF16, pred, fake.data_ptr(), known, mask, a_t, a_prev, 0.0, clip, 0, off0, stride, kept, shape)
        want_m, x_m = kept.fake.got(), kept.x0.got()
        for hist_ptr, name in ((None, "NULL"), (nan_hist.data_ptr(), "NaN")):
            o = MOutputs(shape, BF16, gpu)
            multistep(mode, BF16, pred, fake.data_ptr(), hist_ptr, None, None, a_t, a_prev, 0.0, clip, 0, 0, o, shape)
            o.check(BF16, want, x, x, f"c1 = 0 against diffusion_step, hist_in {name}, mode {mode} clip {clip}")
            o = MOutputs(shape, BF16, gpu)
            multistep(mode, BF16, pred, fake.data_ptr(), hist_ptr, known, mask, a_t, a_prev, 0.0, clip, off0, stride, o, shape)
            o.check(BF16, want_m, x_m, x, f"c1 = 0 against diffusion_step_masked, hist_in {name}, mode {mode} clip {clip}")


def test_kept_pixels_never_see_the_extrapolation(gpu):
    """an all-zeros mask at c1 = 1.37 with NaN / infinities in pred and a NaN-filled history: fake' is h and x0_out is known, exactly"""
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    stride, off0 = G.image_stride(per), 5
    a_t, a_prev = G.alphas(37)
    (p, f, h, kn, _), (pred, fake, _, known, _) = inputs(gpu, shape, "masked")
    zeros = dev(I.mask_case("zeros", G.B, shape[1]), gpu)
    nan_hist = torch.full((G.B, per), float("nan"), device=gpu)
    z0 = draws(gpu, shape, off0, stride)
    o = MOutputs(shape, BF16, gpu)
    multistep(P.SAMPLE_EPS, BF16, pred, fake.data_ptr(), nan_hist.data_ptr(), known, zeros, a_t, a_prev, 1.37, 1.0, off0, stride, o, shape)
    kept = I.kept_f32(kn, a_prev, z0)
    assert np.isfinite(kept).all()
    _, x = G.diffusion_step_f32(P.SAMPLE_EPS, p, f, a_t, a_prev, 0.0, 1.0)
    o.check(BF16, torch.tensor(kept), torch.tensor(kn), torch.tensor(x), "all-zeros mask at c1 = 1.37")


def test_refuses_bad_arguments_and_launches_nothing(gpu):
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    _, (pred, fake, hist, known, mask) = inputs(gpu, shape, "masked")
    o = MOutputs(shape, F32, gpu)
    L = lib()
    good = dict(mode=P.SAMPLE_EPS, dt=F32, pred=pred.data_ptr(), fake=fake.data_ptr(), hist=hist.data_ptr(), known=known.data_ptr(),
                mask=mask.data_ptr(), a_t=0.1, a_prev=0.2, c1=0.5, clip=0.0, B=G.B, per=per, C=G.C, ldout=G.LDOUT, ldout2=G.LDOUT2,
                fake_out=o.fake.ptr, out=o.out.ptr)
    bad = [dict(mode=P.SAMPLE_ODE), dict(mode=4), dict(mode=-1), dict(dt=3), dict(pred=None), dict(fake=None),
           dict(known=None), dict(mask=None),                                                   # one of the pair alone
           dict(c1=float("nan")), dict(c1=float("inf")), dict(c1=-float("inf")), dict(c1=1e39),  # not finite (1e39: not in fp32)
           dict(hist=None), dict(hist=None, c1=-0.25), dict(hist=None, known=None, mask=None),   # c1 != 0 without a history
           dict(fake_out=None), dict(out=None), dict(a_t=1.0), dict(a_t=0.0), dict(a_t=-0.1), dict(a_t=float("nan")), dict(a_prev=1.5),
           dict(a_prev=-0.1), dict(a_prev=float("nan")), dict(B=0), dict(per=0), dict(per=per - 1), dict(C=0), dict(ldout=2), dict(ldout2=2),
           dict(B=1 << 20)]

    def run(a):
        L.call(NEW, a["mode"], a["dt"], a["pred"], a["fake"], a["hist"], a["known"], a["mask"], a["a_t"], a["a_prev"], a["c1"], a["clip"],
               1, 2, 4 * per, per, a["fake_out"], o.hist.ptr, o.x0.ptr, a["out"], a["ldout"], o.out2.ptr, a["ldout2"], a["B"], a["per"], a["C"],
               stream())

    for change in bad:
        with pytest.raises(L.Gct2Error):
            run(dict(good, **change))
    untouched = torch.full(shape, SENTINEL)
    o.check(F32, untouched, untouched, untouched, "refused calls")      # every view still holds the sentinel: nothing was launched
    # legal: no history at c1 = 0 (also a c1 that is 0 once cast to fp32), a_t = 0 where nothing divides by sqrt(a_t)
    for change in (dict(hist=None, c1=0.0), dict(hist=None, c1=1e-60), dict(hist=None, c1=0.0, known=None, mask=None), dict(mode=P.SAMPLE_X, a_t=0.0)):
        run(dict(good, **change))
    torch.cuda.synchronize()


# ---- the kernel as an integrator ---------------------------------------------------------------------------------------------------------------

def order_error_gpu(gpu, mode, d, ascending, second):
    """one run of the kernel, in place on fake and hist, driven by the analytic denoiser evaluated in torch on the device: the
    max-abs error of the last state against the exact flow"""
    import gan_class_transfer2_amd as g
    B, npix, C = MC.ORDER_SHAPE
    mu64, s64, _ = MC.gaussian_case()
    start, end = MC.order_ends(ascending)
    t32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)).to(gpu).contiguous()
    mu, fake = t32(mu64), t32(start)
    hist = torch.full_like(fake, float("nan"))                     # never read at the first step (c1 = 0)
    out = torch.empty(B * npix, C, device=gpu)
    for _, a_t, a_prev, c1 in MC.order_schedule(d, ascending, second, g.multistep_coefficient):
        pred = MC.order_prediction(mode, fake, a_t, mu, t32(MC.denoiser_gain(a_t, s64))).contiguous()
        assert pred.dtype == torch.float32
        lib().call(NEW, mode, F32, pred.data_ptr(), fake.data_ptr(), hist.data_ptr(), None, None, a_t, a_prev, c1, 0.0, 0, 0, 0, 0,
                   fake.data_ptr(), hist.data_ptr(), None, out.data_ptr(), C, None, 0, B, npix * C, C, stream())
    torch.cuda.synchronize()
    assert torch.equal(out.reshape(-1), fake.reshape(-1))
    return float(np.abs(fake.cpu().numpy().astype(np.float64) - end).max())


@pytest.mark.parametrize("ascending", [False, True], ids=["descending", "ascending"])
@pytest.mark.parametrize("mode", MC.ORDER_MODES, ids=["x", "eps"])
def test_order_of_accuracy(gpu, mode, ascending):
    """steps = 200, quadratic schedule, timesteps range(20, 201, d) for d = 20, 10, 5 (10, 19, 37 points) between the exact states at
    t = 200 and t = 20: E1 (every c1 = 0) halves with the step, E1(19) / E1(37) <= 2.3; E2 (multistep_coefficient) falls by
    E2(19) / E2(37) >= 3.0; and E2(19) < E1(37) - the second-order solver at 19 timesteps beats the first-order one at 37.  Both modes
    start at t = 200 (the epsilon mode's division by sqrt(a_t) = 0.0025 there does not spoil fp32: the float32 restatement meets the
    conditions on these arrays, tests/test_multistep_cases_cpu.py: ratios 2.0 and 3.5 descending, 2.0 and 4.1 ascending)"""
    E1 = {len(MC.order_timesteps(d)): order_error_gpu(gpu, mode, d, ascending, False) for d in MC.ORDER_STRIDES}
    E2 = {len(MC.order_timesteps(d)): order_error_gpu(gpu, mode, d, ascending, True) for d in MC.ORDER_STRIDES}
    print(f"order of accuracy, mode {mode}, {'ascending' if ascending else 'descending'}: E1 {E1} E2 {E2}")
    r1, r2 = MC.order_conditions(E1, E2)
    print(f"  E1(19) / E1(37) = {r1:.3f}, E2(19) / E2(37) = {r2:.3f}, E2(19) = {E2[19]:.3g} < E1(37) = {E1[37]:.3g}")
