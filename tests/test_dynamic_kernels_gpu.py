"""gct2_x0_quantile and gct2_diffusion_step_dynamic, ELEMENT BY ELEMENT and bit for bit (+0 == -0, NaN == NaN) against
tests/dynamic_cases.py's restatement (the order statistic by numpy's sort of the keys; the step fed the draws gct2_rng_normal makes
at the documented stream elements) and against the GPU's own gct2_diffusion_step / _step_masked / _step_multistep where every image's
bound is the floor.  Every output - q_out, rows, and the step's planes - is a view inside a sentinel-filled buffer
(tests/test_generate_kernels_gpu.py's View / Outputs) that must be unchanged around the view after each call; the select's scratch is
poisoned with 0xFF before each call, and each call is issued twice."""
import numpy as np
import pytest
import torch

import dynamic_cases as D
import exact_cases as E
import generate_cases as G
import img2img_cases as I
import multistep_cases as MC
import pointwise_cases as P
import test_generate_kernels_gpu as TG
import test_img2img_kernels_gpu as TI
import test_multistep_kernels_gpu as TM
from exact_cases import BF16, F16, F32, SENTINEL
from test_generate_kernels_gpu import DTS, DT_IDS, Outputs, View, dev, draws, lib, stream
from test_multistep_kernels_gpu import MOutputs

pytestmark = pytest.mark.gpu
SELECT, STEP = "gct2_x0_quantile", "gct2_diffusion_step_dynamic"
FORMS = ("plain", "masked")


def scratch_for(gpu, B, per):
    import ctypes
    need = ctypes.c_size_t(0)
    lib().call("gct2_x0_quantile_scratch", B, per, ctypes.byref(need))
    assert need.value > 0
    return torch.empty(need.value, dtype=torch.uint8, device=gpu)


def select(gpu, mode, pred, fake, a_t, rank, floor, B, per, want_rows, want_q, what):
    """the call, twice, each time on a scratch poisoned with 0xFF and into fresh sentinel-filled views; returns rows [B, 2] on the device"""
    scratch = scratch_for(gpu, B, per)
    rows = None
    for turn in range(2):
        scratch.fill_(0xFF)
        r, q = View((B, 1, 2), torch.float32, gpu), View((1, B, 1), torch.float32, gpu)
        lib().call(SELECT, mode, pred.data_ptr(), fake.data_ptr() if fake is not None else None, a_t, rank, floor, r.ptr, q.ptr,
                   scratch.data_ptr(), scratch.numel(), B, per, stream())
        rows = r.got().reshape(B, 2).to(gpu)
        q.check(torch.tensor(want_q).reshape(1, B, 1), f"{what}: q_out, call {turn}")
        r.check(torch.tensor(want_rows).reshape(B, 1, 2), f"{what}: rows, call {turn}")
    return rows


# ---- the select ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(D.crafted_cases())), ids=[c[0] for c in D.crafted_cases()])
def test_select_on_crafted_planes(gpu, case):
    """mode X with fake NULL on the planes where a digit pass can go wrong: an all-equal image, two values with the rank on either
    side of the boundary and on it, runs of ties, neighbours that differ in one key bit (the lowest, and the top and bottom bit of each
    digit), denormals and both zeros, infinities and NaNs below and above the rank (the fallback rows {F, 1}), rank 1 and per_image;
    three images with different distributions per call"""
    name, plane, ranks = D.crafted_cases()[case]
    B, per = plane.shape
    pred = dev(plane, gpu)
    fallback = 0
    for rank in ranks:
        for floor in (1.0, 0.37):
            rows, q = D.select_f32(P.SAMPLE_X, plane, None, 0.3, rank, floor)
            fallback += int((~np.isfinite(q)).sum())
            select(gpu, P.SAMPLE_X, pred, None, 0.3, rank, floor, B, per, rows, q, f"{SELECT} {name} rank {rank} floor {floor}")
    assert fallback > 0 or name != "many_specials"


@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
def test_select_per_mode(gpu, mode, shape):
    """every objective at t = 1, 37, 199, 200 (sa = 0.0025 at t = 200 under the epsilon objectives) on dynamic_cases.step_inputs; per_image
    3009 (no multiple of 4, one work-group per image), 3072, and one image of 525319 elements (many work-groups per image, the
    grid-stride loop's second trip)"""
    B, npix, C = shape
    per = npix * C
    rank = D.quantile_rank(D.PERCENTILE, per)
    for t in P.DIFFUSION_TS:
        a_t, _ = G.alphas(t)
        p, f = D.step_inputs(shape, mode, t)
        rows, q = D.select_f32(mode, p, f, a_t, rank, D.FLOOR)
        select(gpu, mode, dev(p, gpu), dev(f, gpu), a_t, rank, D.FLOOR, B, per, rows, q, f"{SELECT} mode {mode} t {t} shape {shape}")


# ---- the step ------------------------------------------------------------------------------------------------------------------------------

def dynamic(mode, dt, pred, fake_in_ptr, hist_in_ptr, known, mask, rows, a_t, a_prev, s2, c1, off, off0, stride, o, shape, seed=G.SEED,
            sid=G.SID):
    B, npix, C = shape
    hist = getattr(o, "hist", None)
    lib().call(STEP, mode, dt, pred.data_ptr(), fake_in_ptr, hist_in_ptr, known.data_ptr() if known is not None else None,
               mask.data_ptr() if mask is not None else None, rows.data_ptr() if rows is not None else None, a_t, a_prev, s2, c1, seed, sid,
               off, off0, stride, o.fake.ptr, hist.ptr if hist else None, o.x0.ptr if o.x0 else None, *o.views(), B, npix * C, C, stream())


def masked_inputs(gpu, shape, form, kind="pattern"):
    """host (known, mask per element), device (known, mask per pixel); None: plain"""
    B, npix, C = shape
    if form == "plain":
        return (None, None), (None, None)
    kn, m = I.known_case(B, npix * C), I.mask_case(kind, B, npix)
    return (kn, I.per_element(m, C)), (dev(kn, gpu), dev(m, gpu))


# (multistep, eta or c1, offset of the step's noise): the DDIM step without noise, with noise at EVERY offset of G.OFFSETS (0, 1, 2, 3, 5
# and across the wrap of the low counter word), the multistep form without and with an extrapolation
COMBOS = ((False, 0.0, 0),) + tuple((False, 1.0, off) for off in G.OFFSETS) + ((True, 0.0, 0), (True, D.C1, 0))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_dynamic_step_per_element(gpu, dt, mode, shape, form):
    """rows from the GPU's own select (one image under the floor, two above it: tests/test_dynamic_cases_cpu.py), then the step:
    plain and masked; sigma2 = 0, eta = 1 at each of the offsets 0, 1, 2, 3, 5 and across the wrap of the low counter word (images an
    image_stride apart that is no multiple of 4: the general form of the noise kernel; the masked form's starting noise at the next
    offset of that list), multistep at c1 = 0 and 1.37; the timesteps 1, 37, 199, 200 in turn; views with ldout 4 and 67 in
    f32 / bf16 / f16"""
    B, npix, C = shape
    per = npix * C
    rank = D.quantile_rank(D.PERCENTILE, per)
    stride = G.image_stride(per)
    (kn, el), (known, mask) = masked_inputs(gpu, shape, form)
    h = MC.hist_case(B, per)
    hist = dev(h, gpu)
    for k, (multi, v, off) in enumerate(COMBOS):
        t = P.DIFFUSION_TS[k % len(P.DIFFUSION_TS)]
        off0 = G.OFFSETS[(G.OFFSETS.index(off) + 1) % len(G.OFFSETS)]
        a_t, a_prev = G.alphas(t)
        p, f = D.step_inputs(shape, mode, t)
        pred, fake = dev(p, gpu), dev(f, gpu)
        want_rows, q = D.select_f32(mode, p, f, a_t, rank, D.FLOOR)
        what = f"{E.DTYPE_NAMES[dt]} mode {mode} t {t} {form} {'multistep c1' if multi else 'eta'} {v} offsets {off}, {off0} shape {shape}"
        rows = select(gpu, mode, pred, fake, a_t, rank, D.FLOOR, B, per, want_rows, q, SELECT + " " + what)
        s2 = 0.0 if multi else G.sigma2(a_t, a_prev, v)
        z = draws(gpu, shape, off, stride) if s2 else None
        z0 = draws(gpu, shape, off0, stride) if form == "masked" else None
        o = MOutputs(shape, dt, gpu, out2=per < 1000000 or k == 0, hist_out=multi)
        dynamic(mode, dt, pred, fake.data_ptr(), hist.data_ptr() if multi else None, known, mask, rows, a_t, a_prev, s2, v if multi else 0.0,
                off, off0, stride, o, shape)
        want, x0, hx = D.dynamic_step_f32(mode, p, f, want_rows, a_t, a_prev, s2, z, h, v if multi else None, kn, el, z0)
        o.check(dt, torch.tensor(want), torch.tensor(x0), torch.tensor(hx) if multi else None, STEP + " " + what)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("off", G.ALIGNED_OFFSETS)
@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_dynamic_step_with_noise_four_element_form(gpu, dt, mode, off, form):
    """what generate(clip_denoised="dynamic", eta > 0) passes at every step: offset, offset0, image_stride and per_image multiples of 4
    and 16-byte aligned planes, so a thread owns a whole Philox counter and the fp32 planes move as 16-byte accesses - with the bound
    engaged (rows from the select: one image under the floor, two rescaled), against the restatement; the second offset crosses the
    wrap of the low counter word.  Then one element off the alignment: the general form, the same rows"""
    shape = (G.B, G.NPIXS[1], G.C)
    per = shape[1] * shape[2]
    rank = D.quantile_rank(D.PERCENTILE, per)
    t = 37
    a_t, a_prev = G.alphas(t)
    s2 = G.sigma2(a_t, a_prev, 1.0)
    assert np.float32(s2) > 0
    p, f = D.step_inputs(shape, mode, t)
    pred, fake = dev(p, gpu), dev(f, gpu)
    (kn, el), (known, mask) = masked_inputs(gpu, shape, form)
    want_rows, q = D.select_f32(mode, p, f, a_t, rank, D.FLOOR)
    assert (want_rows[:, 1] == 1).any() and (want_rows[:, 1] < 1).sum() >= 2
    rows = select(gpu, mode, pred, fake, a_t, rank, D.FLOOR, G.B, per, want_rows, q, f"{SELECT} mode {mode}, four-element form")
    off0 = off + 4 * per                                           # (the starting noise of the masked form: aligned too)
    for shift in (0, 1):
        z = draws(gpu, shape, off + shift, per)
        z0 = draws(gpu, shape, off0, per) if form == "masked" else None
        o = MOutputs(shape, dt, gpu, hist_out=False)
        if shift == 0:
            ptrs = [pred.data_ptr(), fake.data_ptr(), o.fake.ptr, o.x0.ptr] + ([known.data_ptr()] if known is not None else [])
            assert per % 4 == 0 and off % 4 == 0 and off0 % 4 == 0 and all(ptr % 16 == 0 for ptr in ptrs)
        dynamic(mode, dt, pred, fake.data_ptr(), None, known, mask, rows, a_t, a_prev, s2, 0.0, off + shift, off0, per, o, shape)
        want, x0, _ = D.dynamic_step_f32(mode, p, f, want_rows, a_t, a_prev, s2, z, None, None, kn, el, z0)
        o.check(dt, torch.tensor(want), torch.tensor(x0), None,
                f"{STEP} {E.DTYPE_NAMES[dt]} mode {mode} {form}, images back to back from {off} + {shift}")


# more images than the select's grid has rows for (the image loop's second trip, in the digit passes and in the finish), and three
# images so long that one grid row is all there is: (B, per_image)
MANY_IMAGES = (G.MANY_IMAGES_SHAPE[0], G.MANY_IMAGES_SHAPE[1] * G.MANY_IMAGES_SHAPE[2])
LONG_IMAGES = (3, 1025 * 4096 + 5)


@pytest.mark.parametrize("shape", [MANY_IMAGES, LONG_IMAGES], ids=["2051x3", "3x4198405"])
def test_select_image_loop(gpu, shape):
    """B = 2051 images of 3 elements: the grid has 2048 rows of images, the last three images take the second trip of the image loop
    of every digit pass and of the finish.  B = 3 images of 1025 x 4096 + 5 elements: 1026 work-groups per image leave one grid row,
    every work-group walks all three images and reuses its histograms.  Epsilon objective, every image its own scale"""
    B, per = shape
    rng = np.random.default_rng([B, per, 73])
    a_t, _ = G.alphas(37)
    scale = (np.exp(rng.uniform(-3, 3, (B, 1))) * np.sqrt(a_t)).astype(np.float32)
    p, f = (rng.standard_normal((B, per)).astype(np.float32) * scale for _ in range(2))
    rank = D.quantile_rank(D.PERCENTILE, per) if per > 3 else 2
    rows, q = D.select_f32(P.SAMPLE_EPS, p, f, a_t, rank, D.FLOOR)
    assert (rows[:, 1] == 1).any() and (rows[:, 1] < 1).any() and len(set(q.tolist())) == B
    select(gpu, P.SAMPLE_EPS, dev(p, gpu), dev(f, gpu), a_t, rank, D.FLOOR, B, per, rows, q, f"{SELECT} B {B} per_image {per}")


@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
def test_floor_rows_are_the_fixed_clip(gpu, mode):
    """rows {F, 1} for every image: the bits of gct2_diffusion_step, _step_masked and _step_multistep at clip = F, launches made here
    on the same inputs (CLIP_SPECIALS in pred: beyond, on and just past the bounds, a NaN, both infinities)"""
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    stride, off, off0 = G.image_stride(per), 3, 2 + 7 * per
    a_t, a_prev = G.alphas(199)
    s2 = G.sigma2(a_t, a_prev, 1.0)
    _, (pred, fake, hist, known, mask) = TM.inputs(gpu, shape, "masked")
    for F in G.CLIPS:
        rows = torch.tensor([[F, 1.0]] * G.B, dtype=torch.float32, device=gpu)
        for s in (0.0, s2):
            want = Outputs(shape, BF16, gpu)
            TG.step(mode, BF16, pred, fake.data_ptr(), a_t, a_prev, s, F, off, stride, want, shape)
            o = MOutputs(shape, BF16, gpu, hist_out=False)
            dynamic(mode, BF16, pred, fake.data_ptr(), None, None, None, rows, a_t, a_prev, s, 0.0, off, off0, stride, o, shape)
            o.check(BF16, want.fake.got(), want.x0.got(), None, f"rows {{F, 1}} against diffusion_step, mode {mode} F {F} sigma2 {s}")
            want = Outputs(shape, BF16, gpu)
            TI.masked(mode, BF16, pred, fake.data_ptr(), known, mask, a_t, a_prev, s, F, off, off0, stride, want, shape)
            o = MOutputs(shape, BF16, gpu, hist_out=False)
            dynamic(mode, BF16, pred, fake.data_ptr(), None, known, mask, rows, a_t, a_prev, s, 0.0, off, off0, stride, o, shape)
            o.check(BF16, want.fake.got(), want.x0.got(), None, f"rows {{F, 1}} against diffusion_step_masked, mode {mode} F {F} sigma2 {s}")
        for c1 in (0.0, D.C1):
            for kn, m in ((None, None), (known, mask)):
                want = MOutputs(shape, BF16, gpu)
                TM.multistep(mode, BF16, pred, fake.data_ptr(), hist.data_ptr(), kn, m, a_t, a_prev, c1, F, off0, stride, want, shape)
                o = MOutputs(shape, BF16, gpu)
                dynamic(mode, BF16, pred, fake.data_ptr(), hist.data_ptr(), kn, m, rows, a_t, a_prev, 0.0, c1, off, off0, stride, o, shape)
                o.check(BF16, want.fake.got(), want.x0.got(), want.hist.got(),
                        f"rows {{F, 1}} against diffusion_step_multistep, mode {mode} F {F} c1 {c1} {'masked' if kn is not None else 'plain'}")


def test_rescale_is_not_contracted(gpu):
    """x = x * r is rounded on its own: neither fma(x, r, c (x r - hist)) in the extrapolation (c1 = 1.37) nor the eps line's
    fma(-sa, x, f) (c1 = 0) is what the kernel stored"""
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    p, f = D.step_inputs(shape, P.SAMPLE_X, 37)
    h = MC.hist_case(G.B, per)
    a_t, a_prev = G.alphas(37)
    rows, _ = D.select_f32(P.SAMPLE_X, p, f, a_t, D.quantile_rank(D.PERCENTILE, per), D.FLOOR)
    assert (rows[:, 1] != 1).sum() >= 2
    pred, fake, hist, drows = dev(p, gpu), dev(f, gpu), dev(h, gpu), dev(rows, gpu)
    for c1, term in ((D.C1, 0), (0.0, 1)):
        o = MOutputs(shape, F32, gpu)
        dynamic(P.SAMPLE_X, F32, pred, fake.data_ptr(), hist.data_ptr(), None, None, drows, a_t, a_prev, 0.0, c1, 0, 0, 0, o, shape)
        got = o.fake.got().numpy().reshape(p.shape)
        fused = D.dynamic_step_fused(P.SAMPLE_X, p, f, rows, a_t, a_prev, h, c1, term)
        plain, _, _ = D.dynamic_step_f32(P.SAMPLE_X, p, f, rows, a_t, a_prev, 0.0, None, h, c1)
        assert (fused.view(np.int32) != got.view(np.int32)).sum() > 0, (c1, term)
        assert (plain.view(np.int32) == got.view(np.int32)).all(), (c1, term)


def test_refuses_bad_arguments_and_launches_nothing(gpu):
    shape = (G.B, G.NPIXS[0], G.C)
    per = shape[1] * shape[2]
    _, (pred, fake, hist, known, mask) = TM.inputs(gpu, shape, "masked")
    L = lib()
    # ---- the select
    scratch = scratch_for(gpu, G.B, per)
    r, q = View((G.B, 1, 2), torch.float32, gpu), View((1, G.B, 1), torch.float32, gpu)
    good = dict(mode=P.SAMPLE_EPS, pred=pred.data_ptr(), fake=fake.data_ptr(), a_t=0.1, rank=7, floor=1.0, rows=r.ptr, q=q.ptr,
                scratch=scratch.data_ptr(), bytes=scratch.numel(), B=G.B, per=per)
    bad = [dict(mode=P.SAMPLE_ODE), dict(mode=4), dict(mode=-1), dict(mode=6), dict(pred=None), dict(fake=None), dict(rows=None),
           dict(scratch=None), dict(a_t=1.0), dict(a_t=0.0), dict(a_t=-0.1), dict(a_t=float("nan")), dict(rank=0), dict(rank=per + 1),
           dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(floor=1e39), dict(floor=1e-60),
           dict(bytes=scratch.numel() - 1), dict(bytes=0), dict(B=0), dict(B=-1), dict(per=0), dict(B=1 << 20, rank=1)]

    def run_select(a):
        L.call(SELECT, a["mode"], a["pred"], a["fake"], a["a_t"], a["rank"], a["floor"], a["rows"], a["q"], a["scratch"], a["bytes"], a["B"],
               a["per"], stream())

    for change in bad:
        with pytest.raises(L.Gct2Error):
            run_select(dict(good, **change))
    import ctypes
    need = ctypes.c_size_t(0)
    for B, n, ptr in ((0, per, ctypes.byref(need)), (G.B, 0, ctypes.byref(need)), (G.B, per, None), (1 << 20, per, ctypes.byref(need))):
        with pytest.raises(L.Gct2Error):
            L.call("gct2_x0_quantile_scratch", B, n, ptr)
    r.check(torch.full((G.B, 1, 2), SENTINEL), "refused selects: rows")
    q.check(torch.full((1, G.B, 1), SENTINEL), "refused selects: q_out")
    # legal: mode X without fake and at a_t = 0, q_out NULL, rank at both ends
    for change in (dict(mode=P.SAMPLE_X, fake=None, a_t=0.0), dict(q=None), dict(rank=1), dict(rank=per), dict(mode=D.SAMPLE_V, a_t=0.0)):
        run_select(dict(good, **change))
    torch.cuda.synchronize()
    # ---- the step
    o = MOutputs(shape, F32, gpu)
    rows = torch.tensor([[1.0, 1.0]] * G.B, dtype=torch.float32, device=gpu)
    good = dict(mode=P.SAMPLE_EPS, dt=F32, pred=pred.data_ptr(), fake=fake.data_ptr(), hist=hist.data_ptr(), known=known.data_ptr(),
                mask=mask.data_ptr(), rows=rows.data_ptr(), a_t=0.1, a_prev=0.2, s2=0.0, c1=0.5, B=G.B, per=per, C=G.C, ldout=G.LDOUT,
                ldout2=G.LDOUT2, fake_out=o.fake.ptr, hist_out=o.hist.ptr, out=o.out.ptr)
    bad = [dict(mode=P.SAMPLE_ODE), dict(mode=4), dict(mode=-1), dict(dt=3), dict(pred=None), dict(fake=None), dict(rows=None),
           dict(known=None), dict(mask=None),                                                   # one of the pair alone
           dict(c1=float("nan")), dict(c1=float("inf")), dict(c1=1e39), dict(hist=None), dict(hist=None, hist_out=None),
           dict(s2=0.1), dict(s2=0.1, c1=0.0), dict(s2=0.1, c1=0.0, hist=None),                  # multistep (a history plane) with noise
           dict(s2=-0.1, c1=0.0, hist=None, hist_out=None), dict(s2=0.9, c1=0.0, hist=None, hist_out=None), dict(fake_out=None),
           dict(out=None), dict(a_t=1.0), dict(a_t=0.0), dict(a_t=float("nan")), dict(a_prev=1.5), dict(a_prev=-0.1), dict(B=0), dict(per=0),
           dict(per=per - 1), dict(C=0), dict(ldout=2), dict(ldout2=2), dict(B=1 << 20)]

    def run_step(a):
        L.call(STEP, a["mode"], a["dt"], a["pred"], a["fake"], a["hist"], a["known"], a["mask"], a["rows"], a["a_t"], a["a_prev"], a["s2"],
               a["c1"], 1, 2, 8 * per, 4 * per, per, a["fake_out"], a["hist_out"], o.x0.ptr, a["out"], a["ldout"], o.out2.ptr, a["ldout2"],
               a["B"], a["per"], a["C"], stream())

    for change in bad:
        with pytest.raises(L.Gct2Error):
            run_step(dict(good, **change))
    untouched = torch.full(shape, SENTINEL)
    o.check(F32, untouched, untouched, untouched, "refused steps")
    for change in (dict(hist=None, c1=0.0), dict(hist=None, hist_out=None, c1=0.0, s2=0.1), dict(known=None, mask=None),
                   dict(mode=P.SAMPLE_X, a_t=0.0)):
        run_step(dict(good, **change))
    torch.cuda.synchronize()
