"""gct2_diffusion_step_guided and gct2_x0_quantile_guided, ELEMENT BY ELEMENT and bit for bit (+0 == -0, NaN == NaN) against the
compositions they replace, launched here on the same inputs: the existing step entry points (gct2_diffusion_step, _step_masked,
_step_multistep, _step_dynamic) and gct2_x0_quantile on the plane pg + w (pm - pg) that torch forms as three separate fp32 operations.
Every output - the step's planes, both pairs of views, rows and q_out - is a view inside a sentinel-filled buffer
(tests/test_generate_kernels_gpu.py's View / Outputs) that must be unchanged around the view after each call.  That the inputs make
these comparisons meaningful is asserted without a GPU (tests/test_guidance_cases_cpu.py)."""
import numpy as np
import pytest
import torch

import dynamic_cases as D
import exact_cases as E
import generate_cases as G
import guidance_cases as GC
import pointwise_cases as P
import test_generate_kernels_gpu as TG
import test_img2img_kernels_gpu as TI
import test_multistep_kernels_gpu as TM
from exact_cases import BF16, F16, F32, SENTINEL
from test_dynamic_kernels_gpu import dynamic, scratch_for
from test_generate_kernels_gpu import DTS, DT_IDS, View, dev, lib, stream
from test_multistep_kernels_gpu import MOutputs

pytestmark = pytest.mark.gpu
SELECT, STEP = "gct2_x0_quantile_guided", "gct2_diffusion_step_guided"
LD3, LD4 = 7, 19                                       # the guide's views: leading dimensions that are neither C nor out / out2's
# (name, multistep, eta or c1, masked): plain at sigma2 = 0, with noise, masked (a fractional mask) without and with noise, multistep at
# c1 = 0 and c1 != 0, plain and masked
FORMS = (("plain", False, 0.0, False), ("noise", False, 1.0, False), ("masked", False, 0.0, True), ("masked_noise", False, 1.0, True),
         ("multistep_c0", True, 0.0, False), ("multistep_c1", True, GC.C1, False), ("multistep_masked_c1", True, GC.C1, True))


def ptr(t):
    return t.data_ptr() if t is not None else None


class GuideViews:
    """out3 / out4: two more compute-dtype views, poisoned around"""

    def __init__(self, shape, dt, gpu, second=True):
        self.out3 = View(shape, E.TDT[dt], gpu, ld=LD3)
        self.out4 = View(shape, E.TDT[dt], gpu, ld=LD4) if second else None

    def args(self):
        return (self.out3.ptr, LD3, self.out4.ptr if self.out4 else None, LD4 if self.out4 else 0)

    def check(self, copy, what):
        self.out3.check(copy, what + ": out3")
        if self.out4 is not None:
            self.out4.check(copy, what + ": out4")


def guided(mode, dt, pred, pred_guide, w, fake_in_ptr, hist_in_ptr, known, mask, rows, a_t, a_prev, s2, c1, clip, off, off0, stride, o, shape,
           gv=None, seed=G.SEED, sid=G.SID):
    B, per = shape[0], shape[1] * shape[2]
    hist = getattr(o, "hist", None)
    lib().call(STEP, mode, dt, pred.data_ptr(), ptr(pred_guide), w, fake_in_ptr, hist_in_ptr, ptr(known), ptr(mask), ptr(rows), a_t, a_prev, s2,
               c1, clip, seed, sid, off, off0, stride, o.fake.ptr, hist.ptr if hist else None, o.x0.ptr if o.x0 else None, *o.views(),
               *(gv.args() if gv else (None, 0, None, 0)), B, per, shape[2], stream())


def existing(mode, dt, pred, fake, hist, known, mask, rows, a_t, a_prev, s2, c1, clip, off, off0, stride, shape, multi, gpu):
    """the existing entry point of the form on ONE prediction plane: its outputs"""
    want = MOutputs(shape, dt, gpu, hist_out=multi)
    if rows is not None:
        dynamic(mode, dt, pred, fake.data_ptr(), hist.data_ptr() if multi else None, known, mask, rows, a_t, a_prev, s2, c1, off, off0, stride,
                want, shape)
    elif multi:
        TM.multistep(mode, dt, pred, fake.data_ptr(), hist.data_ptr(), known, mask, a_t, a_prev, c1, clip, off0, stride, want, shape)
    elif known is not None:
        TI.masked(mode, dt, pred, fake.data_ptr(), known, mask, a_t, a_prev, s2, clip, off, off0, stride, want, shape)
    else:
        TG.step(mode, dt, pred, fake.data_ptr(), a_t, a_prev, s2, clip, off, stride, want, shape)
    return want


def combined(pm, pg, w):
    """pg + w (pm - pg) in torch: three separate fp32 operations, the weight as the fp32 the kernel receives"""
    d = pm - pg
    t = torch.tensor(w, dtype=torch.float32, device=pm.device) * d
    return (pg + t).contiguous()


def plain_select(gpu, mode, pred, fake, a_t, rank, B, per):
    scratch = scratch_for(gpu, B, per)
    rows = torch.empty(B, 2, device=gpu)
    lib().call("gct2_x0_quantile", mode, pred.data_ptr(), fake.data_ptr(), a_t, rank, GC.FLOOR, rows.data_ptr(), None, scratch.data_ptr(),
               scratch.numel(), B, per, stream())
    return rows


def device_planes(gpu, per, mode):
    return tuple(dev(a, gpu) for a in GC.planes(per, mode))


def compare(o, want, dt, multi, what, gv=None):
    copy = want.out.got()
    o.check(dt, want.fake.got(), want.x0.got(), want.hist.got() if multi else None, what)
    assert torch.equal(want.out2.got().view(torch.uint8), copy.view(torch.uint8))
    if gv is not None:
        gv.check(copy, what)


@pytest.mark.parametrize("name", list(GC.STEP_SHAPES))
@pytest.mark.parametrize("mode", GC.MODES, ids=GC.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_plain_form_is_the_existing_entry_point(gpu, dt, mode, name):
    """pred_guide, out3 and out4 NULL: every output of every form - fake_out, hist_out, x0_out, out, out2 - has the bits of the existing
    entry point for that form, without a clip, with the scalar clip and with rows"""
    per, off, off0, stride = GC.STEP_SHAPES[name]
    shape = (GC.B, per // GC.C, GC.C)
    pm, _, fake, hist, known, mask = device_planes(gpu, per, mode)
    a_t, a_prev = G.alphas(GC.T)
    rows_d = plain_select(gpu, mode, pm, fake, a_t, D.quantile_rank(GC.PERCENTILE, per), GC.B, per)
    for form, multi, v, masked in FORMS:
        s2, c1 = (0.0, v) if multi else (G.sigma2(a_t, a_prev, v), 0.0)
        kn, m = (known, mask) if masked else (None, None)
        for clip, rows in ((0.0, None), (0.5, None), (0.0, rows_d)):
            want = existing(mode, dt, pm, fake, hist, kn, m, rows, a_t, a_prev, s2, c1, clip, off, off0, stride, shape, multi, gpu)
            o = MOutputs(shape, dt, gpu, hist_out=multi)
            guided(mode, dt, pm, None, 1.0, fake.data_ptr(), hist.data_ptr() if multi else None, kn, m, rows, a_t, a_prev, s2, c1, clip, off, off0,
                   stride, o, shape)
            compare(o, want, dt, multi, f"{STEP} plain form, {E.DTYPE_NAMES[dt]} mode {mode} {name} {form} clip {clip} rows {rows is not None}")


@pytest.mark.parametrize("name", list(GC.STEP_SHAPES))
@pytest.mark.parametrize("mode", GC.MODES, ids=GC.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_guided_form_is_the_entry_point_on_the_combined_plane(gpu, dt, mode, name):
    """pred_guide given, w = 0, 0.5 and 3: every form equals the existing entry point run on pg + w (pm - pg) formed in torch - with the
    scalar clip and with rows (gct2_x0_quantile's on that plane; at w = 3 the bound engages) - and out3 / out4, views with their own
    leading dimensions, carry exactly the bits of out / out2; nothing around any destination changes"""
    per, off, off0, stride = GC.STEP_SHAPES[name]
    shape = (GC.B, per // GC.C, GC.C)
    pm, pg, fake, hist, known, mask = device_planes(gpu, per, mode)
    a_t, a_prev = G.alphas(GC.T)
    rank = D.quantile_rank(GC.PERCENTILE, per)
    if name == "192_aligned":
        assert per % 4 == 0 and off % 4 == 0 and off0 % 4 == 0 and stride % 4 == 0
        assert all(t.data_ptr() % 16 == 0 for t in (pm, pg, fake, known))
    for w in GC.WEIGHTS:
        p = combined(pm, pg, w)
        rows_d = plain_select(gpu, mode, p, fake, a_t, rank, GC.B, per)
        if w == GC.W_THRESHOLD:
            assert bool((rows_d[:, 1] < 1).any())
        for k, (form, multi, v, masked) in enumerate(FORMS):
            s2, c1 = (0.0, v) if multi else (G.sigma2(a_t, a_prev, v), 0.0)
            kn, m = (known, mask) if masked else (None, None)
            for clip, rows in ((GC.FLOOR, None), (0.0, rows_d)) + (((0.0, None),) if k == 0 else ()):
                want = existing(mode, dt, p, fake, hist, kn, m, rows, a_t, a_prev, s2, c1, clip, off, off0, stride, shape, multi, gpu)
                o, gv = MOutputs(shape, dt, gpu, hist_out=multi), GuideViews(shape, dt, gpu, second=k % 2 == 0)
                if name == "192_aligned":
                    assert o.fake.ptr % 16 == 0 and o.x0.ptr % 16 == 0
                guided(mode, dt, pm, pg, w, fake.data_ptr(), hist.data_ptr() if multi else None, kn, m, rows, a_t, a_prev, s2, c1, clip, off, off0,
                       stride, o, shape, gv)
                compare(o, want, dt, multi, f"{STEP} {E.DTYPE_NAMES[dt]} mode {mode} {name} {form} w {w} clip {clip} rows {rows is not None}", gv)


@pytest.mark.parametrize("mode", GC.MODES, ids=GC.MODE_IDS)
def test_guided_select_is_the_select_on_the_combined_plane(gpu, mode):
    """per_image = 4800, more than one work-group per image: rows and q_out equal gct2_x0_quantile's on the torch-combined plane, on a
    scratch poisoned with 0xFF, and a second run gives the same bits"""
    B, per = GC.B, GC.SELECT_PER_IMAGE
    pm, pg, fake, *_ = device_planes(gpu, per, mode)
    a_t, _ = G.alphas(GC.T)
    rank = D.quantile_rank(GC.PERCENTILE, per)
    scratch = scratch_for(gpu, B, per)
    for w in GC.WEIGHTS:
        p = combined(pm, pg, w)
        want_r, want_q = View((B, 1, 2), torch.float32, gpu), View((1, B, 1), torch.float32, gpu)
        scratch.fill_(0xFF)
        lib().call("gct2_x0_quantile", mode, p.data_ptr(), fake.data_ptr(), a_t, rank, GC.FLOOR, want_r.ptr, want_q.ptr, scratch.data_ptr(),
                   scratch.numel(), B, per, stream())
        rows, q = want_r.got(), want_q.got()
        assert w != GC.W_THRESHOLD or bool((rows[:, 0, 1] < 1).any())
        for turn in range(2):
            scratch.fill_(0xFF)
            r, qq = View((B, 1, 2), torch.float32, gpu), View((1, B, 1), torch.float32, gpu)
            lib().call(SELECT, mode, pm.data_ptr(), pg.data_ptr(), w, fake.data_ptr(), a_t, rank, GC.FLOOR, r.ptr, qq.ptr, scratch.data_ptr(),
                       scratch.numel(), B, per, stream())
            qq.check(q, f"{SELECT} mode {mode} w {w}: q_out, call {turn}")
            r.check(rows, f"{SELECT} mode {mode} w {w}: rows, call {turn}")


@pytest.mark.parametrize("name", list(GC.STEP_SHAPES))
def test_a_nan_of_the_guide_never_reaches_a_kept_pixel(gpu, name):
    """pred_guide is NaN wherever mask = 0: kept pixels of fake_out are the known image re-noised (the bits of the existing masked step on
    the main plane there), kept pixels of x0_out the known image's bits - without noise, with noise and in the multistep form"""
    per, off, off0, stride = GC.STEP_SHAPES[name]
    shape = (GC.B, per // GC.C, GC.C)
    pm, pg, fake, hist, known, _ = device_planes(gpu, per, P.SAMPLE_EPS)
    keep = (torch.arange(GC.B * shape[1], device=gpu).reshape(GC.B, shape[1]) % 3 == 0)
    mask = (~keep).to(torch.float32).contiguous()
    el = keep[:, :, None].expand(GC.B, shape[1], GC.C).reshape(GC.B, per)
    pg = torch.where(el, torch.full_like(pg, float("nan")), pg).contiguous()
    a_t, a_prev = G.alphas(GC.T)
    kept = el.reshape(shape).cpu()
    for multi, v in ((False, 0.0), (False, 1.0), (True, GC.C1)):
        s2, c1 = (0.0, v) if multi else (G.sigma2(a_t, a_prev, v), 0.0)
        want = existing(P.SAMPLE_EPS, F32, pm, fake, hist, known, mask, None, a_t, a_prev, s2, c1, 1.0, off, off0, stride, shape, multi, gpu)
        o = MOutputs(shape, F32, gpu, hist_out=multi)
        guided(P.SAMPLE_EPS, F32, pm, pg, 3.0, fake.data_ptr(), hist.data_ptr() if multi else None, known, mask, None, a_t, a_prev, s2, c1, 1.0, off,
               off0, stride, o, shape)
        got_f, got_x = o.fake.got(), o.x0.got()
        assert torch.isfinite(got_f[kept]).all() and torch.isfinite(got_x[kept]).all()
        assert torch.equal(got_f[kept].view(torch.int32), want.fake.got()[kept].view(torch.int32))
        assert torch.equal(got_x[kept].view(torch.int32), known.cpu().reshape(shape)[kept].view(torch.int32))
        assert torch.isfinite(got_f[~kept]).all()                        # (regenerated pixels read a finite guide)


def test_refuses_bad_arguments_and_launches_nothing(gpu):
    per, off, off0, stride = GC.STEP_SHAPES["75"]
    shape = (GC.B, per // GC.C, GC.C)
    pm, pg, fake, hist, known, mask = device_planes(gpu, per, None)
    L = lib()
    o, gv = MOutputs(shape, F32, gpu), GuideViews(shape, F32, gpu)
    rows = torch.tensor([[1.0, 1.0]] * GC.B, dtype=torch.float32, device=gpu)
    good = dict(mode=P.SAMPLE_EPS, dt=F32, pred=pm.data_ptr(), pg=pg.data_ptr(), w=3.0, fake=fake.data_ptr(), hist=hist.data_ptr(),
                known=known.data_ptr(), mask=mask.data_ptr(), rows=None, a_t=0.1, a_prev=0.2, s2=0.0, c1=0.5, clip=1.0, out3=gv.out3.ptr,
                ld3=LD3, out4=gv.out4.ptr, ld4=LD4, B=GC.B, per=per, C=GC.C, hist_out=o.hist.ptr)
    bad = [dict(pg=None), dict(pg=None, w=0.0), dict(pg=None, w=1.0000001),                # p = pred: w must be 1
           dict(rows=rows.data_ptr()), dict(rows=rows.data_ptr(), clip=0.5), dict(rows=rows.data_ptr(), clip=float("nan")),   # rows with a clip
           dict(out3=None), dict(ld3=2), dict(ld4=2),                                      # out4 without out3; leading dimensions under C
           dict(s2=0.1), dict(s2=0.1, c1=0.0), dict(s2=0.1, c1=0.0, hist=None),            # the multistep form with noise
           dict(mode=P.SAMPLE_ODE), dict(mode=4), dict(mode=-1), dict(mode=6),             # the ODE objective, the reserved code
           dict(w=float("nan")), dict(w=float("inf")), dict(w=1e39), dict(pred=None), dict(fake=None), dict(known=None), dict(mask=None),
           dict(c1=float("nan")), dict(hist=None), dict(a_t=1.0), dict(a_t=0.0), dict(a_prev=1.5), dict(B=0), dict(per=per - 1), dict(C=0),
           dict(dt=3), dict(B=1 << 25)]

    def run(a):
        L.call(STEP, a["mode"], a["dt"], a["pred"], a["pg"], a["w"], a["fake"], a["hist"], a["known"], a["mask"], a["rows"], a["a_t"], a["a_prev"],
               a["s2"], a["c1"], a["clip"], 1, 2, off, off0, stride, o.fake.ptr, a["hist_out"], o.x0.ptr, *o.views(), a["out3"], a["ld3"],
               a["out4"], a["ld4"], a["B"], a["per"], a["C"], stream())

    for change in bad:
        with pytest.raises(L.Gct2Error):
            run(dict(good, **change))
    untouched = torch.full(shape, SENTINEL)
    o.check(F32, untouched, untouched, untouched, "refused steps")
    gv.check(untouched, "refused steps")
    # legal: p = pred at w = 1 exactly, rows without a clip, out3 alone, no guide views, the plain step with noise, mode X at a_t = 0
    for change in (dict(pg=None, w=1.0), dict(rows=rows.data_ptr(), clip=0.0), dict(out4=None, ld4=0), dict(out3=None, out4=None),
                   dict(s2=0.1, c1=0.0, hist=None, hist_out=None), dict(mode=P.SAMPLE_X, a_t=0.0), dict(known=None, mask=None)):
        run(dict(good, **change))
    torch.cuda.synchronize()
    # ---- the select
    scratch = scratch_for(gpu, GC.B, per)
    r = View((GC.B, 1, 2), torch.float32, gpu)
    good = dict(mode=P.SAMPLE_EPS, pred=pm.data_ptr(), pg=pg.data_ptr(), w=3.0, fake=fake.data_ptr(), a_t=0.1, rank=7, floor=1.0, rows=r.ptr,
                scratch=scratch.data_ptr(), bytes=scratch.numel(), B=GC.B, per=per)
    bad = [dict(mode=P.SAMPLE_ODE), dict(mode=4), dict(pred=None), dict(pg=None), dict(fake=None), dict(rows=None), dict(scratch=None),
           dict(w=float("nan")), dict(w=float("inf")), dict(w=1e39), dict(a_t=1.0), dict(a_t=0.0), dict(rank=0), dict(rank=per + 1),
           dict(floor=0.0), dict(floor=float("nan")), dict(bytes=scratch.numel() - 1), dict(B=0), dict(per=0), dict(B=1 << 25, rank=1)]

    def run_select(a):
        L.call(SELECT, a["mode"], a["pred"], a["pg"], a["w"], a["fake"], a["a_t"], a["rank"], a["floor"], a["rows"], None, a["scratch"], a["bytes"],
               a["B"], a["per"], stream())

    for change in bad:
        with pytest.raises(L.Gct2Error):
            run_select(dict(good, **change))
    r.check(torch.full((GC.B, 1, 2), SENTINEL), "refused selects: rows")
    for change in (dict(mode=P.SAMPLE_X, fake=None, a_t=0.0), dict(w=0.0), dict(rank=per)):
        run_select(dict(good, **change))
    torch.cuda.synchronize()
