"""gct2_diffusion_step_masked and gct2_diffusion_start_image, ELEMENT BY ELEMENT and bit for bit (+0 == -0, NaN == NaN) against
tests/img2img_cases.py's restatements fed the draws gct2_rng_normal makes at the documented stream elements, and against the GPU's own
gct2_diffusion_step / gct2_rng_normal + gct2_diffusion_mix.  Every output is a view with pixel stride ld inside a sentinel-filled
buffer (tests/test_generate_kernels_gpu.py's View / Outputs) that must be unchanged around the view after each call."""
import numpy as np
import pytest
import torch

import exact_cases as E
import generate_cases as G
import img2img_cases as I
import pointwise_cases as P
import test_generate_kernels_gpu as TG
from exact_cases import BF16, F16, F32, SENTINEL
from test_generate_kernels_gpu import DTS, DT_IDS, Outputs, dev, draws, lib, stream

pytestmark = pytest.mark.gpu


def masked(mode, dt, pred, fake_in_ptr, known, mask, a_t, a_prev, s2, clip, off, off0, stride, o, shape, seed=G.SEED, sid=G.SID):
    B, npix, C = shape
    lib().call("gct2_diffusion_step_masked", mode, dt, pred.data_ptr(), fake_in_ptr, known.data_ptr(), mask.data_ptr(), a_t, a_prev, s2, clip,
               seed, sid, off, off0, stride, o.fake.ptr, o.x0.ptr if o.x0 else None, *o.views(), B, npix * C, C, stream())


def inputs(gpu, shape, kind="pattern", case=G.step_case):
    """(host pred, fake, known, mask per element), (device pred, fake, known, mask per pixel)"""
    B, npix, C = shape
    p, f = case(B, npix * C) if case is G.step_case else case()
    kn, m = I.known_case(B, npix * C), I.mask_case(kind, B, npix)
    return (p, f, kn, I.per_element(m, C)), tuple(dev(a, gpu) for a in (p, f, kn, m))


def other_lane(off, k):
    """the starting noise's offset for a step's offset: far away, at another lane of its Philox counter"""
    return off + 4 * 1000 + 1 + k % 3


def fused_differs(host, got, a_t, a_prev, s2, clip, z0, z, mode):
    """the contracted blends (img2img_cases.blend_fused) are NOT what the kernel computed: they differ from it on blended pixels"""
    p, f, kn, el = host
    got = got.numpy().reshape(el.shape)
    for term in (0, 1):
        w, _ = I.step_masked_f32(mode, p, f, kn, el, a_t, a_prev, s2, clip, z0, z, blend=lambda m_, g_, h_: I.blend_fused(m_, g_, h_, term))
        differ = w.view(np.int32) != got.view(np.int32)
        where = (el == np.float32(0.3)) | (el == np.float32(0.7)) | ((el == 0.25) if term == 1 else False)
        assert differ[where].sum() > 0, term
        assert not differ[(el >= 1) | (el <= 0)].any()


@pytest.mark.parametrize("npix", G.NPIXS)
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_masked_step_per_element(gpu, dt, mode, npix):
    """the pattern mask (kept, regenerated, blends, out-of-range values, 1e-30 and a NaN at the start and the end of every image); the
    step's noise at offset + b image_stride + i, the starting noise at offset0 + b image_stride + i at ANOTHER lane of its counter, an
    image_stride that is no multiple of 4; sigma2 = 0 and eta 0.7 / 1, with and without the clip"""
    shape = (G.B, npix, G.C)
    per = npix * G.C
    host, (pred, fake, known, mask) = inputs(gpu, shape)
    p, f, kn, el = host
    stride = G.image_stride(per)
    for k, off in enumerate(G.OFFSETS):
        t, eta, clip = P.DIFFUSION_TS[k % len(P.DIFFUSION_TS)], (0.0, 0.7, 1.0)[k % 3], (0.0, 1.0)[k % 2]
        off0 = other_lane(off, k)
        assert (off - off0) % 4 != 0
        a_t, a_prev = G.alphas(t)
        s2 = G.sigma2(a_t, a_prev, eta)
        z0 = draws(gpu, shape, off0, stride)
        z = draws(gpu, shape, off, stride) if eta else None
        o = Outputs(shape, dt, gpu)
        masked(mode, dt, pred, fake.data_ptr(), known, mask, a_t, a_prev, s2, clip, off, off0, stride, o, shape)
        want, x0 = I.step_masked_f32(mode, p, f, kn, el, a_t, a_prev, s2, clip, z0, z)
        got = o.fake.got()
        what = f"diffusion_step_masked {E.DTYPE_NAMES[dt]} mode {mode} t {t} eta {eta} clip {clip} offset {off} offset0 {off0} npix {npix}"
        o.check(dt, torch.tensor(want), torch.tensor(x0), what)
        fused_differs(host, got, a_t, a_prev, s2, clip, z0, z, mode)


@pytest.mark.parametrize("off", G.ALIGNED_OFFSETS)
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_masked_step_four_element_form(gpu, dt, mode, off):
    """what generate passes: offset, offset0, image_stride and per_image multiples of 4 and 16-byte aligned planes (16-byte accesses,
    both draws at the same lanes) - the restatement's bits; the same call with one plane 4 bytes off the alignment takes the general
    form and gives the same bits (a group of four elements spans up to three pixels of the mask at C = 3)"""
    shape = (G.B, G.NPIXS[1], G.C)
    per = shape[1] * shape[2]
    host, (pred, fake, known, mask) = inputs(gpu, shape)
    p, f, kn, el = host
    off0 = G.ALIGNED_OFFSETS[0] + 8 * per if off else G.ALIGNED_OFFSETS[1]
    a_t, a_prev = G.alphas(37)
    z0 = draws(gpu, shape, off0, per)
    shifted = torch.empty(pred.numel() + 1, device=gpu)[1:]
    shifted.copy_(pred.reshape(-1))
    assert shifted.data_ptr() % 16 == 4
    for eta in (1.0, 0.0):
        s2 = G.sigma2(a_t, a_prev, eta)
        z = draws(gpu, shape, off, per) if eta else None
        want, x0 = I.step_masked_f32(mode, p, f, kn, el, a_t, a_prev, s2, 0.5, z0, z)
        for pr, form in ((pred, "four-element"), (shifted, "general")):
            o = Outputs(shape, dt, gpu)
            assert per % 4 == 0 and all(ptr % 16 == 0 for ptr in (pred.data_ptr(), fake.data_ptr(), known.data_ptr(), o.fake.ptr, o.x0.ptr))
            masked(mode, dt, pr, fake.data_ptr(), known, mask, a_t, a_prev, s2, 0.5, off, off0, per, o, shape)
            o.check(dt, torch.tensor(want), torch.tensor(x0), f"diffusion_step_masked {E.DTYPE_NAMES[dt]} mode {mode} eta {eta}, {form} form, "
                    f"images back to back from {off} / {off0}")


@pytest.mark.parametrize("shape", [G.LONG_SHAPE, G.MANY_IMAGES_SHAPE, G.LONG_RNG_SHAPE, G.LONG_VEC_SHAPE],
                         ids=["1x525319x1", "2051x1x3", "1x2098183x1", "1x2098180x1"])
def test_masked_step_second_trips(gpu, shape):
    """sigma2 = 0 on one length past the grid cap of the one-element-per-thread kernel (and on 2051 images: every image's own z0
    range); at eta = 1 more images than work-groups (the image loop), one image of more than 2048 x 256 Philox counters (the counter
    loop) in the general and in the four-element form.  bf16, epsilon mode; the 67-wide copy only where it is small"""
    B, npix, C = shape
    per = npix * C
    host, (pred, fake, known, mask) = inputs(gpu, shape)
    p, f, kn, el = host
    vec = shape == G.LONG_VEC_SHAPE
    stride, off, off0 = (per, 4, 8 + 4 * per) if vec else (G.image_stride(per), 3, 6 + B * G.image_stride(per))
    a_t, a_prev = G.alphas(37)
    etas = (0.0,) if shape == G.LONG_SHAPE else (0.0, 1.0) if shape == G.MANY_IMAGES_SHAPE else (1.0,)

    def all_draws(first):
        if B == 1:
            return draws(gpu, shape, first, stride)
        whole = torch.empty((B - 1) * stride + per, device=gpu)      # 2051 images: one draw over the whole range, cut into the images
        lib().call("gct2_rng_normal", G.SEED, G.SID, first, whole.data_ptr(), whole.numel(), stream())
        torch.cuda.synchronize()
        whole = whole.cpu().numpy()
        return np.stack([whole[b * stride:b * stride + per] for b in range(B)])

    z0 = all_draws(off0)
    for eta in etas:
        s2 = G.sigma2(a_t, a_prev, eta)
        z = all_draws(off) if eta else None
        o = Outputs(shape, BF16, gpu, out2=per < 1000000)
        masked(P.SAMPLE_EPS, BF16, pred, fake.data_ptr(), known, mask, a_t, a_prev, s2, 0.0, off, off0, stride, o, shape)
        want, x0 = I.step_masked_f32(P.SAMPLE_EPS, p, f, kn, el, a_t, a_prev, s2, 0.0, z0, z)
        o.check(BF16, torch.tensor(want), torch.tensor(x0), f"diffusion_step_masked, shape {shape}, eta {eta}")


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_all_ones_is_diffusion_step_and_all_zeros_keeps_the_image(gpu, mode, eta):
    """all-ones: fake', x0_out and both views are a gct2_diffusion_step call's, made here.  All-zeros with NaN, infinities and estimates
    far beyond the clip planted in pred (generate_cases.clip_case): fake' is h and x0_out is known, exactly - nothing of g gets through"""
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    stride, off, off0 = G.image_stride(per), 5, 2 + 7 * per
    a_t, a_prev = G.alphas(199)
    s2 = G.sigma2(a_t, a_prev, eta)
    z0 = draws(gpu, shape, off0, stride)
    for clip in (0.0, 1.0):
        (p, f, kn, el), (pred, fake, known, mask) = inputs(gpu, shape, "ones", G.clip_case)
        plain = Outputs(shape, BF16, gpu)
        TG.step(mode, BF16, pred, fake.data_ptr(), a_t, a_prev, s2, clip, off, stride, plain, shape)
        want, x = plain.fake.got(), plain.x0.got()
        assert torch.isnan(want).any()
        o = Outputs(shape, BF16, gpu)
        masked(mode, BF16, pred, fake.data_ptr(), known, mask, a_t, a_prev, s2, clip, off, off0, stride, o, shape)
        o.check(BF16, want, x, f"all-ones against diffusion_step, mode {mode} eta {eta} clip {clip}")
        _, (_, _, _, zeros) = inputs(gpu, shape, "zeros", G.clip_case)
        o = Outputs(shape, BF16, gpu)
        masked(mode, BF16, pred, fake.data_ptr(), known, zeros, a_t, a_prev, s2, clip, off, off0, stride, o, shape)
        h = I.kept_f32(kn, a_prev, z0)
        assert np.isfinite(h).all()
        o.check(BF16, torch.tensor(h), torch.tensor(kn), f"all-zeros, mode {mode} eta {eta} clip {clip}")


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_masked_step_in_place_and_null_outputs(gpu, mode, eta):
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    _, (pred, fake, known, mask) = inputs(gpu, shape, "half")
    stride, off, off0 = G.image_stride(per), 2, 3 + 5 * per
    a_t, a_prev = G.alphas(199)
    s2 = G.sigma2(a_t, a_prev, eta)
    apart = Outputs(shape, F16, gpu)
    masked(mode, F16, pred, fake.data_ptr(), known, mask, a_t, a_prev, s2, 1.0, off, off0, stride, apart, shape)
    want, x = apart.fake.got(), apart.x0.got()
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(x.reshape(G.B, shape[1], G.C)[:, :shape[1] // 2], known.cpu().reshape(G.B, shape[1], G.C)[:, :shape[1] // 2])
    in_place = Outputs(shape, F16, gpu, fake=fake)                      # fake_out == fake_in
    masked(mode, F16, pred, in_place.fake.ptr, known, mask, a_t, a_prev, s2, 1.0, off, off0, stride, in_place, shape)
    in_place.check(F16, want, x, f"in place, mode {mode} eta {eta}")
    bare = Outputs(shape, F16, gpu, x0=False, out2=False)               # x0_out and out2 NULL
    masked(mode, F16, pred, fake.data_ptr(), known, mask, a_t, a_prev, s2, 1.0, off, off0, stride, bare, shape)
    bare.check(F16, want, None, f"null x0_out and out2, mode {mode} eta {eta}")


# ---- gct2_diffusion_start_image ------------------------------------------------------------------------------------------------------------

def start_image(dt, known, a, off, stride, o, shape, seed=G.SEED, sid=G.SID):
    B, npix, C = shape
    lib().call("gct2_diffusion_start_image", dt, known.data_ptr(), a, seed, sid, off, stride, o.fake.ptr, *o.views(), B, npix * C, C, stream())


@pytest.mark.parametrize("npix", G.NPIXS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_start_image_equals_rng_normal_then_mix(gpu, dt, npix):
    """the two launches it replaces, made here: gct2_rng_normal per image, then gct2_diffusion_mix(x = known, e = z0, alpha = a) - fake,
    and the copies in the compute dtype; and both are the host restatement"""
    shape = (G.B, npix, G.C)
    per = npix * G.C
    kn = I.known_case(G.B, per)
    known = dev(kn, gpu)
    cases = [(off, G.image_stride(per)) for off in G.OFFSETS]
    if per % 4 == 0:                                    # images back to back from a counter's start: the four-element form
        cases += [(off, per) for off in G.ALIGNED_OFFSETS]
    for k, (off, stride) in enumerate(cases):
        a = (G.alphas(37)[0], G.alphas(200)[0], 0.0, 1.0)[k % 4]
        z0 = draws(gpu, shape, off, stride)
        zd = dev(z0, gpu)
        f2 = torch.empty(G.B * per, device=gpu)
        out = torch.empty(G.B * npix, G.C, dtype=E.TDT[dt], device=gpu)
        lib().call("gct2_diffusion_mix", dt, known.data_ptr(), zd.data_ptr(), a, f2.data_ptr(), out.data_ptr(), G.C, None, 0, G.B * npix, G.C, stream())
        torch.cuda.synchronize()
        what = f"diffusion_start_image {E.DTYPE_NAMES[dt]} a {a} offset {off} npix {npix}"
        E.assert_elementwise_equal(f2.cpu().reshape(G.B, -1), torch.tensor(I.start_image_f32(kn, a, z0)), ("b", "i"), what + ": the pair against the host")
        o = Outputs(shape, dt, gpu, x0=False)
        start_image(dt, known, a, off, stride, o, shape)
        E.assert_elementwise_equal(o.out.got().reshape(-1), out.cpu().reshape(-1), ("i",), what + ": the pair's copy")
        o.check(dt, f2.cpu(), None, what)


# ---- refused arguments ------------------------------------------------------------------------------------------------------------------------

def test_refuses_bad_arguments_and_launches_nothing(gpu):
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    _, (pred, fake, known, mask) = inputs(gpu, shape)
    o = Outputs(shape, F32, gpu)
    L = lib()
    good = dict(mode=P.SAMPLE_EPS, dt=F32, pred=pred.data_ptr(), fake=fake.data_ptr(), known=known.data_ptr(), mask=mask.data_ptr(), a_t=0.1,
                a_prev=0.2, s2=0.05, clip=0.0, B=G.B, per=per, C=G.C, ldout=G.LDOUT, ldout2=G.LDOUT2, fake_out=o.fake.ptr, out=o.out.ptr)
    bad = [dict(mode=P.SAMPLE_ODE), dict(mode=4), dict(mode=-1), dict(dt=3), dict(pred=None), dict(fake=None), dict(known=None), dict(mask=None),
           dict(fake_out=None), dict(out=None), dict(a_t=1.0), dict(a_t=0.0), dict(a_t=-0.1), dict(a_t=float("nan")), dict(a_prev=1.5),
           dict(a_prev=-0.1), dict(s2=-0.01), dict(s2=0.81), dict(s2=float("nan")), dict(B=0), dict(per=0), dict(per=per - 1), dict(C=0),
           dict(ldout=2), dict(ldout2=2), dict(B=1 << 20)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(L.Gct2Error):
            L.call("gct2_diffusion_step_masked", a["mode"], a["dt"], a["pred"], a["fake"], a["known"], a["mask"], a["a_t"], a["a_prev"], a["s2"],
                   a["clip"], 1, 2, 0, 4 * per, per, a["fake_out"], o.x0.ptr, a["out"], a["ldout"], o.out2.ptr, a["ldout2"], a["B"], a["per"],
                   a["C"], stream())
    good = dict(dt=F32, known=known.data_ptr(), a=0.3, fake_out=o.fake.ptr, out=o.out.ptr, ldout=G.LDOUT, ldout2=G.LDOUT2, B=G.B, per=per, C=G.C)
    bad = [dict(dt=3), dict(known=None), dict(fake_out=None), dict(out=None), dict(a=-0.1), dict(a=1.1), dict(a=float("nan")), dict(B=0), dict(per=0),
           dict(per=per - 1), dict(C=0), dict(ldout=2), dict(ldout2=2), dict(B=1 << 20)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(L.Gct2Error):
            L.call("gct2_diffusion_start_image", a["dt"], a["known"], a["a"], 1, 2, 0, per, a["fake_out"], a["out"], a["ldout"], o.out2.ptr,
                   a["ldout2"], a["B"], a["per"], a["C"], stream())
    untouched = torch.full(shape, SENTINEL)
    o.check(F32, untouched, untouched, "refused calls")                 # every view still holds the sentinel: nothing was launched
    # a_t = 0 is legal where nothing divides by sqrt(a_t)
    L.call("gct2_diffusion_step_masked", P.SAMPLE_X, F32, pred.data_ptr(), fake.data_ptr(), known.data_ptr(), mask.data_ptr(), 0.0, 0.2, 0.0, 0.0,
           1, 2, 0, 4 * per, per, o.fake.ptr, None, o.out.ptr, G.LDOUT, None, 0, G.B, per, G.C, stream())
    torch.cuda.synchronize()
