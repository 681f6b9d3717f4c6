"""gct2_objective_loss_fwd_bwd and the sampler kernels' mode V through the C ABI on the GPU, ELEMENT BY ELEMENT and bit for bit against
the float32 restatements of tests/objective_cases.py.

The loss kernel: both kinds, every legal presence combination of a, c, eps, w and lam, loss scales 1 and 1024, on shapes that put an
image off the 16-byte grid (n_img = 105), hold one element, fill a work-group partly and span two work-groups per image (the kernel's
tile is objective_cases.TILE = 4096 elements of one image).  dpred must equal the restatement bit for bit; the loss is float32 of the
fp64 restatement or its float32 neighbour (fp64 sums differ only in order: the final cast can move one place at the most).  Every
buffer carries guards (tests/test_eval_kernels_gpu.Guarded): NaN around what is read - and the inputs must be unchanged afterwards -,
sentinels around what is written, a scratch of exactly the reported size whose inside starts as NaN.

Mode V: gct2_diffusion_update against v_update (a_t = 0 included), gct2_diffusion_step against update + mix and against the
restatement with a clip, the masked step at m >= 1 against the plain step, the multistep step at c1 = 0 against the plain step and at
c1 != 0 against the restatement; the shapes and views of tests/generate_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import exact_cases as E
import generate_cases as G
import multistep_cases as MC
import objective_cases as OC
import pointwise_cases as P
import test_generate_kernels_gpu as TG
from exact_cases import BF16, F16, F32
from test_eval_kernels_gpu import Guarded, SENTINEL as SENT
from test_generate_kernels_gpu import DTS, DT_IDS, Outputs, dev, lib, stream
from test_multistep_kernels_gpu import MOutputs, multistep

pytestmark = pytest.mark.gpu
NEW = "gct2_objective_loss_fwd_bwd"
V = OC.SAMPLE_V
SHAPE_IDS = ["x".join(map(str, s)) for s in OC.LOSS_SHAPES]
NAMES = ("a", "c", "eps", "w", "lam")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((bits(a) == bits(b)) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))).all())


def adjacent(got, want64):
    """got is float32(want64) or the float32 value next to it"""
    w = np.float32(want64)
    return got == w or got == np.nextafter(w, np.float32(np.inf)) or got == np.nextafter(w, np.float32(-np.inf))


class Case:
    """one shape on the device; run(kind, present, s) launches with the arguments of that presence combination, checks every guard
    and returns (dpred or None, loss)"""

    def __init__(self, gpu, v, shift=0):
        self.gpu, self.v, self.shape = gpu, v, v["pred"].shape
        B, n = self.shape[0], v["pred"].size
        self.n = n
        self.pred, self.x, self.eps = (Guarded(gpu, n, np.nan, v[k], shift) for k in ("pred", "x", "eps"))
        self.a, self.c, self.w, self.lam = (Guarded(gpu, B, np.nan, v[k]) for k in ("a", "c", "w", "lam"))
        self.scale = Guarded(gpu, 4, np.nan, np.float32([1.0, 0, 0, 0]))
        need = ctypes.c_size_t(0)
        lib().check(lib().load().gct2_objective_loss_scratch(0, *self.shape, ctypes.byref(need)), "gct2_objective_loss_scratch")
        self.need = need.value
        self.dpred, self.loss, self.scratch = Guarded(gpu, n, SENT, shift=shift), Guarded(gpu, 4, SENT), Guarded(gpu, self.need, SENT)
        self.inputs = [self.pred, self.x, self.eps, self.a, self.c, self.w, self.lam]

    def arguments(self, code, present, s=1.0, grad=True, **over):
        on = dict(zip(NAMES, present))
        B, H, W, C = self.shape
        if s != 1.0:
            self.scale.inner[0] = s
        ptr = lambda name, g: g.ptr() if on[name] else None
        args = dict(kind=code, pred=self.pred.ptr(), x=self.x.ptr(), eps=ptr("eps", self.eps), a=ptr("a", self.a), c=ptr("c", self.c),
                    w=ptr("w", self.w), lam=ptr("lam", self.lam), dpred=self.dpred.ptr() if grad else None, loss=self.loss.ptr(),
                    scratch=self.scratch.ptr(), scratch_floats=self.need, B=B, H=H, W=W, C=C,
                    ls=self.scale.ptr() if s != 1.0 else None, stream=stream())
        assert not set(over) - set(args)
        args.update(over)
        return list(args.values())

    def prepare(self):
        self.dpred.full.fill_(SENT)
        self.loss.full.fill_(SENT)
        self.scratch.inner.fill_(float("nan"))
        torch.cuda.synchronize()

    def untouched(self):
        """nothing was launched: every output still holds what prepare() left"""
        torch.cuda.synchronize()
        return (bool((self.dpred.full == SENT).all()) and bool((self.loss.full == SENT).all()) and bool(torch.isnan(self.scratch.inner).all())
                and self.scratch.guards_intact())

    def run(self, kind, present, s=1.0, grad=True):
        self.prepare()
        lib().call(NEW, *self.arguments(kind, present, s, grad))
        torch.cuda.synchronize()
        assert all(t.unchanged() for t in self.inputs)                      # pred, x, eps (and the vectors) are read only, bit for bit
        assert self.dpred.guards_intact() and self.loss.guards_intact() and self.scratch.guards_intact()
        loss = self.loss.inner.cpu().numpy()
        assert (loss[1:] == SENT).all()                                     # one float is written
        if not grad:
            assert bool((self.dpred.full == SENT).all())                    # dpred = NULL writes only loss (and scratch)
            return None, loss[0]
        return self.dpred.inner.cpu().numpy().reshape(self.shape), loss[0]

    def want(self, kind, present, s=1.0):
        on = dict(zip(NAMES, present))
        v = self.v
        pick = lambda k: v[k] if on[k] else None
        # (c without a, and eps without a, are legal and ignored: the target is x)
        return OC.objective_loss_reference(kind, v["pred"], v["x"], pick("eps") if on["a"] else None, pick("a"),
                                           pick("c") if on["a"] else None, pick("w"), pick("lam"), s)


@pytest.mark.parametrize("shape", OC.LOSS_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", OC.KINDS, ids=OC.KIND_IDS)
def test_loss_and_gradient_every_presence_combination(gpu, kind, shape):
    v = OC.loss_inputs(shape, seed=1)
    run = Case(gpu, v)
    checked = 0
    for present in OC.presence_combinations():
        for s in OC.LOSS_SCALES:
            d, dpred, loss = run.want(kind, present, s)
            got, got_loss = run.run(kind, present, s)
            what = f"{OC.KIND_IDS[kind]} {shape} {dict(zip(NAMES, present))} s {s}"
            E.assert_elementwise_equal(torch.tensor(got), torch.tensor(dpred), ("b", "h", "w", "c"), what)
            assert adjacent(got_loss, loss), (what, got_loss, loss)
            checked += 1
    assert checked == 2 * len(OC.presence_combinations()) == 40


@pytest.mark.parametrize("shape", OC.LOSS_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", OC.KINDS, ids=OC.KIND_IDS)
def test_exact_sums_bit_for_bit(gpu, kind, shape):
    """integer-valued planes, power-of-two vectors: every product and sum is exact, the loss is exactly the restatement's"""
    v = OC.loss_inputs(shape, seed=2, integers=True)
    run = Case(gpu, v)
    for present in ((True, True, True, True, True), (False, False, False, False, False), (True, True, True, False, True)):
        d, dpred, loss = run.want(kind, present)
        on = dict(zip(NAMES, present))
        col = lambda k: v[k].astype(np.float64).reshape(-1, 1, 1, 1) if on[k] else 1.0
        d64 = col("a") * v["x"] + (col("c") * v["eps"] if on["a"] else 0.0) - col("w") * v["pred"]
        assert np.array_equal(d.astype(np.float64), d64) and float(np.abs(d).max()) < 64      # no float32 operation rounded
        got, got_loss = run.run(kind, present)
        assert bits(got_loss) == bits(np.float32(loss)), (present, got_loss, loss)
        assert same_bits(got, dpred)


@pytest.mark.parametrize("kind", OC.KINDS, ids=OC.KIND_IDS)
def test_operands_off_the_16_byte_grid_give_the_same_bits(gpu, kind):
    shape = OC.LOSS_SHAPES[0]
    v = OC.loss_inputs(shape, seed=1)
    present = (True, True, True, True, True)
    base, base_loss = Case(gpu, v).run(kind, present, 1024.0)
    for shift in (1, 2, 3):
        got, loss = Case(gpu, v, shift=shift).run(kind, present, 1024.0)
        assert same_bits(got, base) and bits(loss) == bits(base_loss)


@pytest.mark.parametrize("shape", [OC.LOSS_SHAPES[0], OC.LOSS_SHAPES[3]], ids=[SHAPE_IDS[0], SHAPE_IDS[3]])
@pytest.mark.parametrize("kind", OC.KINDS, ids=OC.KIND_IDS)
def test_properties_of_the_weights(gpu, kind, shape):
    """two runs give identical bits; lam scaled by 2 doubles loss and dpred exactly; lam[b] = 0 leaves that image's dpred all zeros;
    dpred = NULL writes only the loss, the same one; with lam and w NULL, loss * B agrees with the sum of gct2_eval_loss_rows"""
    v = OC.loss_inputs(shape, seed=4)
    B = shape[0]
    full = (True, True, True, True, True)
    run = Case(gpu, v)
    one, one_loss = run.run(kind, full, 1024.0)
    again, again_loss = run.run(kind, full, 1024.0)
    assert same_bits(one, again) and bits(one_loss) == bits(again_loss)
    _, only_loss = run.run(kind, full, 1024.0, grad=False)
    assert bits(only_loss) == bits(one_loss)
    _, unscaled = run.run(kind, full, 1.0)
    assert bits(unscaled) == bits(one_loss)                                 # the loss is never multiplied by s
    v2 = dict(v, lam=v["lam"] * np.float32(2))
    two, two_loss = Case(gpu, v2).run(kind, full, 1024.0)
    assert same_bits(two, one * np.float32(2)) and bits(two_loss) == bits(np.float32(2) * one_loss)
    lam0 = v["lam"].copy()
    lam0[B - 1] = 0
    zero, zero_loss = Case(gpu, dict(v, lam=lam0)).run(kind, full, 1024.0)
    assert (zero[B - 1] == 0).all() and (B == 1 or (zero[0] != 0).any()) and same_bits(zero[:B - 1], one[:B - 1])
    # against gct2_eval_loss_rows on the same inputs (lam NULL, w NULL): loss * B and the sum of the rows, one place apart at the most
    present = (True, True, True, False, False)
    _, loss = run.run(kind, present)
    need = ctypes.c_size_t(0)
    lib().check(lib().load().gct2_eval_loss_scratch(kind, *shape, ctypes.byref(need)), "gct2_eval_loss_scratch")
    rows = torch.empty(B, device=gpu)
    scratch = torch.zeros(max(4, need.value), device=gpu)
    lib().call("gct2_eval_loss_rows", kind, run.pred.ptr(), run.x.ptr(), run.eps.ptr(), run.a.ptr(), run.c.ptr(), None, rows.data_ptr(),
               scratch.data_ptr(), scratch.numel(), *shape, None, stream())
    torch.cuda.synchronize()
    total = float(rows.cpu().numpy().astype(np.float64).sum())            # (each row is itself one float32 rounding of its fp64 mean)
    # (two float32 casts of relative error <= 2^-24 each stand between the two figures: the loss's and, at the worst, every row's)
    assert abs(float(loss) * B - total) <= 2.0 * 2.0 ** -24 * total * (1 + 1e-6), (float(loss) * B, total)


def test_refusals_launch_nothing(gpu):
    shape = (2, 16, 16, 3)
    run = Case(gpu, OC.loss_inputs(shape, seed=1))
    full = (True, True, True, True, True)
    L = lib()
    bad = [dict(kind=2), dict(kind=3), dict(kind=-1), dict(kind=7), dict(pred=None), dict(x=None), dict(loss=None), dict(scratch=None),
           dict(eps=None), dict(c=None), dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=5), dict(pred=run.pred.ptr() + 2),
           dict(x=run.x.ptr() + 1), dict(dpred=run.dpred.ptr() + 2), dict(lam=run.lam.ptr() + 2), dict(scratch=run.scratch.ptr() + 4),
           dict(scratch_floats=run.need - 1), dict(scratch_floats=0), dict(B=65536, H=1, W=1, C=1), dict(B=2, H=32768, W=32768, C=1),
           dict(dpred=run.pred.ptr())]
    for over in bad:
        run.prepare()
        with pytest.raises(L.Gct2Error):
            L.call(NEW, *run.arguments(0, full, **over))
        assert run.untouched(), over
    run.prepare()
    with pytest.raises(L.Gct2Error):                                        # a without c, eps given
        L.call(NEW, *run.arguments(1, (True, False, True, True, True)))
    assert run.untouched()
    got, _ = run.run(0, full)                                               # and the same arguments, unbroken, run
    assert np.isfinite(got).all()


# ---- mode V of the sampler kernels ---------------------------------------------------------------------------------------------------------

SHAPE = (G.B, G.NPIXS[0], G.C)


@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
def test_update_mode_v_per_element(gpu, shape):
    B, npix, C = shape
    n = B * npix * C
    p, f = G.step_case(B, npix * C)
    pred, fake = dev(p, gpu), dev(f, gpu)
    for a_t in [G.alphas(t)[0] for t in P.DIFFUSION_TS] + [0.0, 0.9999]:
        x, e = (torch.full((n,), float("nan"), device=gpu) for _ in range(2))
        lib().call("gct2_diffusion_update", V, pred.data_ptr(), fake.data_ptr(), a_t, 0.0, x.data_ptr(), e.data_ptr(), n, stream())
        wx, we = OC.v_update(p, f, a_t)
        E.assert_elementwise_equal(x.cpu().reshape(B, -1), torch.tensor(wx), ("b", "i"), f"update V x a_t {a_t}")
        E.assert_elementwise_equal(e.cpu().reshape(B, -1), torch.tensor(we), ("b", "i"), f"update V e a_t {a_t}")


def test_mode_4_stays_refused_and_eps_modes_still_need_a_positive_alpha(gpu):
    L = lib()
    n = 64
    t = torch.zeros(n, device=gpu)
    o = Outputs((1, 16, 4), F32, gpu)
    for mode in (4, 6, -1):
        with pytest.raises(L.Gct2Error):
            L.call("gct2_diffusion_update", mode, t.data_ptr(), t.data_ptr(), 0.1, 0.0, t.data_ptr(), t.data_ptr(), n, stream())
        with pytest.raises(L.Gct2Error):
            TG.step(mode, F32, t, t.data_ptr(), 0.1, 0.2, 0.0, 0.0, 0, 0, o, (1, 16, 4))
    for mode in (P.SAMPLE_EPS, P.SAMPLE_SCALED_EPS):
        with pytest.raises(L.Gct2Error):
            L.call("gct2_diffusion_update", mode, t.data_ptr(), t.data_ptr(), 0.0, 0.0, t.data_ptr(), t.data_ptr(), n, stream())
    with pytest.raises(L.Gct2Error):                                        # a_t = 1 divides by sb in the clip's re-derivation
        TG.step(V, F32, t, t.data_ptr(), 1.0, 0.2, 0.0, 0.0, 0, 0, o, (1, 16, 4))


@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_step_mode_v_equals_update_then_mix(gpu, dt, shape):
    B, npix, C = shape
    p, f = G.step_case(B, npix * C)
    pred, fake = dev(p, gpu), dev(f, gpu)
    for a_t, a_prev in [G.alphas(t) for t in (P.DIFFUSION_TS if npix < 10000 else (37,))] + [(0.0, 0.5)]:
        o = Outputs(shape, dt, gpu)
        TG.step(V, dt, pred, fake.data_ptr(), a_t, a_prev, 0.0, 0.0, 0, 0, o, shape)
        f2, x, out = TG.pair(gpu, V, dt, pred, fake, a_t, a_prev, shape)
        what = f"diffusion_step V {E.DTYPE_NAMES[dt]} a_t {a_t} shape {shape}"
        host, hx = OC.v_step_f32(p, f, a_t, a_prev, 0.0)
        E.assert_elementwise_equal(f2.reshape(B, -1), torch.tensor(host), ("b", "i"), what + ": the pair against the host")
        o.check(dt, f2, x, what)


@pytest.mark.parametrize("clip", G.CLIPS)
def test_step_mode_v_clips_and_rederives_eps(gpu, clip):
    p, f = G.clip_case()
    pred, fake = dev(p, gpu), dev(f, gpu)
    for t in (1, 199):
        a_t, a_prev = G.alphas(t)
        o = Outputs(SHAPE, F32, gpu)
        TG.step(V, F32, pred, fake.data_ptr(), a_t, a_prev, 0.0, clip, 0, 0, o, SHAPE)
        want, x = OC.v_step_f32(p, f, a_t, a_prev, clip)
        assert float(np.nanmax(np.abs(x[np.isfinite(x)]))) <= clip
        o.check(F32, torch.tensor(want), torch.tensor(x), f"diffusion_step V clip {clip} t {t}")


def test_step_mode_v_with_noise_adds_the_draws(gpu):
    """sigma2 > 0: fake' = (cx x + ce e) + cz z with the draws of the documented stream elements (the existing with-noise forms)"""
    a_t, a_prev = G.alphas(37)
    s2 = G.sigma2(a_t, a_prev, 1.0)
    # the general form (an image starts inside a Philox counter) and the four-element form (everything a multiple of 4)
    for npix, off, stride in ((G.NPIXS[0], 5, G.image_stride(G.NPIXS[0] * G.C)), (G.NPIXS[1], 8, G.NPIXS[1] * G.C)):
        shape = (G.B, npix, G.C)
        p, f = G.step_case(G.B, npix * G.C)
        pred, fake = dev(p, gpu), dev(f, gpu)
        z = TG.draws(gpu, shape, off, stride)
        o = Outputs(shape, F32, gpu)
        TG.step(V, F32, pred, fake.data_ptr(), a_t, a_prev, s2, 0.0, off, stride, o, shape)
        x, e = OC.v_estimate(p, f, a_t, 0.0)
        _, _, cx, ce, cz = G.step_coefficients(a_t, a_prev, s2)
        want = (cx * x + ce * e) + cz * z
        o.check(F32, torch.tensor(want), torch.tensor(x), f"diffusion_step V with noise, npix {npix} offset {off}")


def test_masked_step_mode_v_at_full_mask_is_the_plain_step(gpu):
    p, f = G.clip_case()
    pred, fake = dev(p, gpu), dev(f, gpu)
    B, npix, C = SHAPE
    known = torch.full((B, npix * C), 0.25, device=gpu)
    mask = torch.full((B, npix), 1.5, device=gpu)                           # m >= 1: selects, not a blend
    a_t, a_prev = G.alphas(37)
    for clip in (0.0, 1.0):
        plain, masked = Outputs(SHAPE, F16, gpu), Outputs(SHAPE, F16, gpu)
        TG.step(V, F16, pred, fake.data_ptr(), a_t, a_prev, 0.0, clip, 0, 0, plain, SHAPE)
        lib().call("gct2_diffusion_step_masked", V, F16, pred.data_ptr(), fake.data_ptr(), known.data_ptr(), mask.data_ptr(), a_t, a_prev, 0.0,
                   clip, G.SEED, G.SID, 0, 0, npix * C, masked.fake.ptr, masked.x0.ptr, *masked.views(), B, npix * C, C, stream())
        masked.check(F16, plain.fake.got(), plain.x0.got(), f"masked V clip {clip}")


@pytest.mark.parametrize("clip", (0.0, 1.0))
def test_multistep_mode_v(gpu, clip):
    """c1 = 0: the plain step's bits (hist_in NULL); c1 != 0: the restatement"""
    p, f = G.clip_case()
    h = MC.hist_case(G.B, SHAPE[1] * G.C)
    pred, fake, hist = dev(p, gpu), dev(f, gpu), dev(h, gpu)
    a_t, a_prev = G.alphas(199)
    plain = Outputs(SHAPE, BF16, gpu)
    TG.step(V, BF16, pred, fake.data_ptr(), a_t, a_prev, 0.0, clip, 0, 0, plain, SHAPE)
    o = MOutputs(SHAPE, BF16, gpu)
    multistep(V, BF16, pred, fake.data_ptr(), None, None, None, a_t, a_prev, 0.0, clip, 0, 0, o, SHAPE)
    o.check(BF16, plain.fake.got(), plain.x0.got(), plain.x0.got(), f"multistep V c1 0 clip {clip}")
    differs = 0
    for c1 in (0.5, 1.37):
        o = MOutputs(SHAPE, BF16, gpu)
        multistep(V, BF16, pred, fake.data_ptr(), hist.data_ptr(), None, None, a_t, a_prev, c1, clip, 0, 0, o, SHAPE)
        want, x = OC.v_multistep_f32(p, f, h, a_t, a_prev, c1, clip)
        base, _ = OC.v_multistep_f32(p, f, h, a_t, a_prev, 0.0, clip)
        differs += int((bits(want) != bits(base)).sum())
        o.check(BF16, torch.tensor(want), torch.tensor(x), torch.tensor(x), f"multistep V c1 {c1} clip {clip}")
    assert differs > p.size
