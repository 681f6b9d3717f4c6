"""gct2_diffusion_step and gct2_diffusion_start, ELEMENT BY ELEMENT and bit for bit (+0 == -0, NaN == NaN): without noise against the
GPU's own gct2_diffusion_update + gct2_diffusion_mix, with noise against tests/generate_cases.diffusion_step_f32 fed the draws
gct2_rng_normal makes at the same stream elements.  Every output is a view with pixel stride ld inside a sentinel-filled buffer
(guard pixels in front and behind, pad columns up to ld) that must be unchanged around the view after each call."""
import numpy as np
import pytest
import torch

import exact_cases as E
import generate_cases as G
import pointwise_cases as P
from exact_cases import BF16, F16, F32, SENTINEL

pytestmark = pytest.mark.gpu

DTS = [F32, BF16, F16]
DT_IDS = ["f32", "bf16", "f16"]


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, gpu):
    return torch.tensor(np.ascontiguousarray(a)).to(gpu).contiguous()


class View:
    """an output view [B, npix, C] with pixel stride ld inside a flat sentinel-filled buffer (exact_cases.wide_view, 64 guard pixels)"""

    def __init__(self, shape, tdt, gpu, ld=None, values=None):
        init = torch.full(shape, SENTINEL, dtype=tdt, device=gpu) if values is None else values.reshape(shape).to(tdt)
        self.shape = tuple(shape)
        self.buf, self.view, self.ptr = E.wide_view(init, shape[-1] if ld is None else ld, fill=SENTINEL, guard_pixels=64)

    def got(self):
        torch.cuda.synchronize()
        return self.view.cpu().contiguous()

    def check(self, want, what):
        """bit equality per element, then nothing outside the view changed (that check overwrites the view: it comes last)"""
        E.assert_elementwise_equal(self.got(), want.reshape(self.shape), ("b", "p", "c"), what)
        E.assert_outside_untouched_device(self.buf, self.view, SENTINEL, what)


class Outputs:
    """the four (five) outputs of one call"""

    def __init__(self, shape, dt, gpu, x0=True, out2=True, fake=None):
        self.fake = View(shape, torch.float32, gpu, values=fake)
        self.x0 = View(shape, torch.float32, gpu) if x0 else None
        self.out = View(shape, E.TDT[dt], gpu, ld=G.LDOUT)
        self.out2 = View(shape, E.TDT[dt], gpu, ld=G.LDOUT2) if out2 else None

    def views(self):
        return (self.out.ptr, G.LDOUT, self.out2.ptr if self.out2 else None, G.LDOUT2 if self.out2 else 0)

    def check(self, dt, fake_want, x0_want, what):
        """fake_want / x0_want: float32 CPU tensors; the compute-dtype copies are one rounding of fake_want"""
        copy = fake_want.to(E.TDT[dt])
        self.fake.check(fake_want, what + ": fake_out")
        if self.x0 is not None:
            self.x0.check(x0_want, what + ": x0_out")
        self.out.check(copy, what + ": out")
        if self.out2 is not None:
            self.out2.check(copy, what + ": out2")


def step(mode, dt, pred, fake_in_ptr, a_t, a_prev, s2, clip, off, stride, o, shape, seed=G.SEED, sid=G.SID):
    B, npix, C = shape
    lib().call("gct2_diffusion_step", mode, dt, pred.data_ptr(), fake_in_ptr, a_t, a_prev, s2, clip, seed, sid, off, stride, o.fake.ptr,
               o.x0.ptr if o.x0 else None, *o.views(), B, npix * C, C, stream())


def draws(gpu, shape, off, stride, seed=G.SEED, sid=G.SID):
    """what gct2_rng_normal writes for the elements of every image: one call per image"""
    B, npix, C = shape
    z = torch.empty(B, npix * C, device=gpu)
    for b in range(B):
        lib().call("gct2_rng_normal", seed, sid, off + b * stride, z[b].data_ptr(), npix * C, stream())
    torch.cuda.synchronize()
    return z.cpu().numpy()


# ---- sigma^2 = 0: the two launches it replaces ------------------------------------------------------------------------------------------

def pair(gpu, mode, dt, pred, fake, a_t, a_prev, shape):
    """gct2_diffusion_update then gct2_diffusion_mix(a_prev) on the same inputs, into plain tensors: (fake', x, out)"""
    B, npix, C = shape
    n = B * npix * C
    x, e, f2 = (torch.empty(n, device=gpu) for _ in range(3))
    out = torch.empty(B * npix, C, dtype=E.TDT[dt], device=gpu)
    lib().call("gct2_diffusion_update", mode, pred.data_ptr(), fake.data_ptr(), a_t, a_prev, x.data_ptr(), e.data_ptr(), n, stream())
    lib().call("gct2_diffusion_mix", dt, x.data_ptr(), e.data_ptr(), a_prev, f2.data_ptr(), out.data_ptr(), C, None, 0, B * npix, C, stream())
    torch.cuda.synchronize()
    return f2.cpu(), x.cpu(), out.cpu()


@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_step_without_noise_equals_update_then_mix(gpu, dt, mode, shape):
    """eta = 0, no clip: fake_out, out, out2 are the GPU's own gct2_diffusion_update + gct2_diffusion_mix on the same inputs, x0_out
    the update's x_theta, and both are the host restatement (which a fused multiply-add would miss, tests/test_generate_cases_cpu.py).
    The long shape has a second trip of the grid-stride loop"""
    B, npix, C = shape
    p, f = G.step_case(B, npix * C)
    pred, fake = dev(p, gpu), dev(f, gpu)
    for t in (P.DIFFUSION_TS if npix < 10000 else (37,)):
        a_t, a_prev = G.alphas(t)
        o = Outputs(shape, dt, gpu)
        step(mode, dt, pred, fake.data_ptr(), a_t, a_prev, 0.0, 0.0, 0, 0, o, shape)
        f2, x, out = pair(gpu, mode, dt, pred, fake, a_t, a_prev, shape)
        what = f"diffusion_step {E.DTYPE_NAMES[dt]} mode {mode} t {t} shape {shape}"
        host, hx = G.diffusion_step_f32(mode, p, f, a_t, a_prev, 0.0, 0.0)
        E.assert_elementwise_equal(f2.reshape(B, -1), torch.tensor(host), ("b", "i"), what + ": the pair against the host")
        E.assert_elementwise_equal(out.reshape(-1), f2.to(E.TDT[dt]), ("i",), what + ": the pair's copy")
        o.check(dt, f2, x, what)


# ---- sigma^2 > 0 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("npix", G.NPIXS)
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_step_with_noise_per_element(gpu, dt, mode, npix):
    """z = gct2_rng_normal's draws at elements offset + b image_stride + i (an image_stride that is no multiple of 4: every image
    starts at another lane of its Philox counter; offsets inside the first counters and across the wrap of the low counter word);
    the output is diffusion_step_f32 on those draws"""
    shape = (G.B, npix, G.C)
    per = npix * G.C
    p, f = G.step_case(G.B, per)
    pred, fake = dev(p, gpu), dev(f, gpu)
    stride = G.image_stride(per)
    for k, off in enumerate(G.OFFSETS):
        t, eta = P.DIFFUSION_TS[k % len(P.DIFFUSION_TS)], G.ETAS[k % len(G.ETAS)]
        a_t, a_prev = G.alphas(t)
        s2 = G.sigma2(a_t, a_prev, eta)
        assert np.float32(s2) > 0
        z = draws(gpu, shape, off, stride)
        o = Outputs(shape, dt, gpu)
        step(mode, dt, pred, fake.data_ptr(), a_t, a_prev, s2, 0.0, off, stride, o, shape)
        want, x = G.diffusion_step_f32(mode, p, f, a_t, a_prev, s2, 0.0, z)
        o.check(dt, torch.tensor(want), torch.tensor(x), f"diffusion_step {E.DTYPE_NAMES[dt]} mode {mode} t {t} eta {eta} offset {off} npix {npix}")


@pytest.mark.parametrize("off", G.ALIGNED_OFFSETS)
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_step_with_noise_four_element_form(gpu, dt, mode, off):
    """what generate passes: offset, image_stride and per_image multiples of 4 and 16-byte aligned planes, so a thread owns a whole
    Philox counter and moves the fp32 planes as 16-byte accesses - the same bits; the second offset crosses the wrap of the low counter word"""
    shape = (G.B, G.NPIXS[1], G.C)
    per = shape[1] * shape[2]
    p, f = G.step_case(G.B, per)
    pred, fake = dev(p, gpu), dev(f, gpu)
    a_t, a_prev = G.alphas(37)
    s2 = G.sigma2(a_t, a_prev, 1.0)
    z = draws(gpu, shape, off, per)
    o = Outputs(shape, dt, gpu)
    assert per % 4 == 0 and all(ptr % 16 == 0 for ptr in (pred.data_ptr(), fake.data_ptr(), o.fake.ptr, o.x0.ptr))
    step(mode, dt, pred, fake.data_ptr(), a_t, a_prev, s2, 0.5, off, per, o, shape)
    want, x = G.diffusion_step_f32(mode, p, f, a_t, a_prev, s2, 0.5, z)
    o.check(dt, torch.tensor(want), torch.tensor(x), f"diffusion_step {E.DTYPE_NAMES[dt]} mode {mode}, images back to back from {off}")
    # one element off the alignment takes the general form: the same draws one element later
    o = Outputs(shape, dt, gpu)
    step(mode, dt, pred, fake.data_ptr(), a_t, a_prev, s2, 0.5, off + 1, per, o, shape)
    want, x = G.diffusion_step_f32(mode, p, f, a_t, a_prev, s2, 0.5, draws(gpu, shape, off + 1, per))
    o.check(dt, torch.tensor(want), torch.tensor(x), f"diffusion_step {E.DTYPE_NAMES[dt]} mode {mode}, images back to back from {off + 1}")


SECOND_TRIPS = [G.LONG_SHAPE, G.MANY_IMAGES_SHAPE, G.LONG_RNG_SHAPE, G.LONG_VEC_SHAPE]


@pytest.mark.parametrize("shape", SECOND_TRIPS, ids=["1x525319x1", "2051x1x3", "1x2098183x1", "1x2098180x1"])
def test_step_with_noise_second_trips(gpu, shape):
    """the with-noise kernel's loops: the issue's long length; more images than work-groups (the image loop); one image of more than
    2048 x 256 Philox counters (the counter loop), from inside a counter and - the length a multiple of 4 - from a counter's start (the
    four-element form).  The no-noise kernel's second trip is test_step_without_noise_equals_update_then_mix's long shape.  bf16,
    epsilon mode; the 67-wide copy only where it is small"""
    B, npix, C = shape
    per = npix * C
    p, f = G.step_case(B, per)
    pred, fake = dev(p, gpu), dev(f, gpu)
    stride, off = (per, 4) if shape == G.LONG_VEC_SHAPE else (G.image_stride(per), 3)
    a_t, a_prev = G.alphas(37)
    s2 = G.sigma2(a_t, a_prev, 1.0)
    if B == 1:
        z = draws(gpu, shape, off, stride)
    else:                                               # 2051 images: one draw over the whole range, cut into the images
        whole = torch.empty((B - 1) * stride + per, device=gpu)
        lib().call("gct2_rng_normal", G.SEED, G.SID, off, whole.data_ptr(), whole.numel(), stream())
        torch.cuda.synchronize()
        whole = whole.cpu().numpy()
        z = np.stack([whole[b * stride:b * stride + per] for b in range(B)])
    o = Outputs(shape, BF16, gpu, out2=per < 1000000)
    step(P.SAMPLE_EPS, BF16, pred, fake.data_ptr(), a_t, a_prev, s2, 0.0, off, stride, o, shape)
    want, x = G.diffusion_step_f32(P.SAMPLE_EPS, p, f, a_t, a_prev, s2, 0.0, z)
    o.check(BF16, torch.tensor(want), torch.tensor(x), f"diffusion_step with noise, shape {shape}")


# ---- clip ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
@pytest.mark.parametrize("dt", [F32, F16], ids=["f32", "f16"])
def test_step_clips_the_estimate_and_rederives_eps(gpu, dt, mode, eta):
    """estimates beyond the bound, on it, just past it, a NaN and both infinities (generate_cases.clip_case): x0_out is the clipped
    estimate (the NaN stays), fake' is built from it and from eps = (f - sa x) / sb; clip = 0 and clip < 0 leave the bits of the
    unclipped call"""
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    p, f = G.clip_case()
    pred, fake = dev(p, gpu), dev(f, gpu)
    stride, off = G.image_stride(per), 5
    z = draws(gpu, shape, off, stride) if eta else None
    for t in (37, 200):
        a_t, a_prev = G.alphas(t)
        s2 = G.sigma2(a_t, a_prev, eta)
        results = {}
        for clip in G.CLIPS + (0.0, -1.0):
            o = Outputs(shape, dt, gpu)
            step(mode, dt, pred, fake.data_ptr(), a_t, a_prev, s2, clip, off, stride, o, shape)
            want, x = G.diffusion_step_f32(mode, p, f, a_t, a_prev, s2, clip, z)
            if clip > 0:
                ok = ~np.isnan(x)
                assert (~ok).sum() > 0 and np.abs(x[ok]).max() == np.float32(clip)
            results[clip] = o.fake.got()
            o.check(dt, torch.tensor(want), torch.tensor(x), f"diffusion_step {E.DTYPE_NAMES[dt]} mode {mode} t {t} eta {eta} clip {clip}")
        E.assert_elementwise_equal(results[-1.0], results[0.0], ("b", "p", "c"), "clip < 0 against clip = 0")
        assert not torch.equal(torch.nan_to_num(results[1.0]), torch.nan_to_num(results[0.0]))


# ---- aliasing, null outputs, refused arguments -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_step_in_place_and_null_outputs(gpu, mode, eta):
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    p, f = G.step_case(G.B, per)
    pred, fake = dev(p, gpu), dev(f, gpu)
    stride, off = G.image_stride(per), 2
    a_t, a_prev = G.alphas(199)
    s2 = G.sigma2(a_t, a_prev, eta)
    apart = Outputs(shape, F16, gpu)
    step(mode, F16, pred, fake.data_ptr(), a_t, a_prev, s2, 1.0, off, stride, apart, shape)
    want, x = apart.fake.got(), apart.x0.got()
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    in_place = Outputs(shape, F16, gpu, fake=fake)                      # fake_out == fake_in
    step(mode, F16, pred, in_place.fake.ptr, a_t, a_prev, s2, 1.0, off, stride, in_place, shape)
    in_place.check(F16, want, x, f"in place, mode {mode} eta {eta}")
    bare = Outputs(shape, F16, gpu, x0=False, out2=False)               # x0_out and out2 NULL
    step(mode, F16, pred, fake.data_ptr(), a_t, a_prev, s2, 1.0, off, stride, bare, shape)
    bare.check(F16, want, None, f"null x0_out and out2, mode {mode} eta {eta}")


def test_step_refuses_bad_arguments_and_launches_nothing(gpu):
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    p, f = G.step_case(G.B, per)
    pred, fake = dev(p, gpu), dev(f, gpu)
    o = Outputs(shape, F32, gpu)
    L = lib()
    good = dict(mode=P.SAMPLE_EPS, dt=F32, pred=pred.data_ptr(), fake=fake.data_ptr(), a_t=0.1, a_prev=0.2, s2=0.05, clip=0.0, B=G.B, per=per,
                C=G.C, ldout=G.LDOUT, ldout2=G.LDOUT2, fake_out=o.fake.ptr, out=o.out.ptr)
    bad = [dict(mode=P.SAMPLE_ODE), dict(mode=4), dict(mode=-1), dict(dt=3), dict(pred=None), dict(fake=None), dict(fake_out=None), dict(out=None),
           dict(a_t=1.0), dict(a_t=0.0), dict(a_t=-0.1), dict(a_t=float("nan")), dict(a_prev=1.5), dict(a_prev=-0.1), dict(s2=-0.01),
           dict(s2=0.81), dict(s2=float("nan")), dict(B=0), dict(per=0), dict(per=per - 1), dict(C=0), dict(ldout=2), dict(ldout2=2),
           dict(B=1 << 20)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(L.Gct2Error):
            L.call("gct2_diffusion_step", a["mode"], a["dt"], a["pred"], a["fake"], a["a_t"], a["a_prev"], a["s2"], a["clip"], 1, 2, 0, per,
                   a["fake_out"], o.x0.ptr, a["out"], a["ldout"], o.out2.ptr, a["ldout2"], a["B"], a["per"], a["C"], stream())
    with pytest.raises(L.Gct2Error):
        L.call("gct2_diffusion_start", 3, 1, 2, 0, per, o.fake.ptr, o.out.ptr, G.LDOUT, None, 0, G.B, per, G.C, stream())
    with pytest.raises(L.Gct2Error):
        L.call("gct2_diffusion_start", F32, 1, 2, 0, per, None, o.out.ptr, G.LDOUT, None, 0, G.B, per, G.C, stream())
    untouched = torch.full(shape, SENTINEL)
    o.check(F32, untouched, untouched, "refused calls")                 # every view still holds the sentinel: nothing was launched
    # a_t = 0 is legal where nothing divides by sqrt(a_t)
    L.call("gct2_diffusion_step", P.SAMPLE_X, F32, pred.data_ptr(), fake.data_ptr(), 0.0, 0.2, 0.0, 0.0, 1, 2, 0, per, o.fake.ptr, None, o.out.ptr,
           G.LDOUT, None, 0, G.B, per, G.C, stream())
    torch.cuda.synchronize()


# ---- gct2_diffusion_start --------------------------------------------------------------------------------------------------------------------

def start(dt, off, stride, o, shape, B=None, first=0):
    """images first .. first + B - 1 of the views"""
    _, npix, C = shape
    per = npix * C
    size = {F32: 4, BF16: 2, F16: 2}[dt]
    lib().call("gct2_diffusion_start", dt, G.SEED, G.SID, off, stride, o.fake.ptr + 4 * first * per, o.out.ptr + size * first * npix * G.LDOUT,
               G.LDOUT, o.out2.ptr + size * first * npix * G.LDOUT2 if o.out2 else None, G.LDOUT2 if o.out2 else 0,
               shape[0] if B is None else B, per, C, stream())


@pytest.mark.parametrize("npix", G.NPIXS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_start_equals_rng_normal_per_image(gpu, dt, npix):
    shape = (G.B, npix, G.C)
    per = npix * G.C
    cases = [(off, G.image_stride(per)) for off in G.OFFSETS]
    if per % 4 == 0:                                    # images back to back from a counter's start: the four-element form
        cases += [(off, per) for off in G.ALIGNED_OFFSETS]
    for off, stride in cases:
        z = torch.tensor(draws(gpu, shape, off, stride))
        o = Outputs(shape, dt, gpu, x0=False)
        start(dt, off, stride, o, shape)
        o.check(dt, z, None, f"diffusion_start {E.DTYPE_NAMES[dt]} offset {off} npix {npix}")
    assert float(z.std()) > 0.9 and abs(float(z.mean())) < 0.05


def test_start_in_two_calls_equals_one(gpu):
    """B = 4 in one call against two calls of B = 2, the second with the offset advanced by 2 image_stride"""
    shape = (4, G.NPIXS[0], G.C)
    stride, off = G.image_stride(shape[1] * shape[2]), P.CARRY
    one, two = Outputs(shape, BF16, gpu, x0=False), Outputs(shape, BF16, gpu, x0=False)
    start(BF16, off, stride, one, shape)
    start(BF16, off, stride, two, shape, B=2)
    start(BF16, off + 2 * stride, stride, two, shape, B=2, first=2)
    want = one.fake.got()
    assert not torch.equal(want[:2], want[2:])
    two.check(BF16, want, None, "two calls of two images")
    one.check(BF16, want, None, "one call of four images")
