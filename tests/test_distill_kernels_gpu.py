"""gct2_distill_start / _step / _target, ELEMENT BY ELEMENT and bit for bit (+0 == -0, NaN == NaN) against tests/distill_cases.py's
restatement, and image by image against the GPU's own gct2_diffusion_start_image / gct2_diffusion_step called with that image's scalars.
One batch holds the last row of the table, the first (no t'': the x0 end point) and a middle one.  Every output is a view inside a
sentinel-filled buffer that must be unchanged around the view after each call."""
import numpy as np
import pytest
import torch

import distill_cases as D
import exact_cases as E
from exact_cases import BF16, F16, F32, SENTINEL
from test_generate_kernels_gpu import DTS, DT_IDS, View, dev, lib, stream

pytestmark = pytest.mark.gpu
START, STEP, TARGET = "gct2_distill_start", "gct2_distill_step", "gct2_distill_target"
SHAPES = [(D.B, npix, D.C) for npix in D.NPIXS]
SHAPE_IDS = ["3x35x3", "3x256x3"]
OFFSET = 5                                             # the draws start inside a Philox counter


def tables(gpu):
    """(float32 table, int32 table, their device copies, alpha) of the teacher's 50 timesteps of 200"""
    import gan_class_transfer2_amd as g
    T = g.trainer_math
    taus = T.distill_grid(D.STEPS, D.N)
    tab, tt = T.distill_table(taus, D.STEPS)
    return tab, tt, dev(tab, gpu), dev(tt, gpu), lambda t: float(T.alpha_dash(t, D.STEPS))


def stride_of(per):
    s = per + 5                                        # every image starts at another lane of its counter
    return s + 1 if s % 4 == 0 else s


def draws(gpu, shape, off, stride):
    B, npix, C = shape
    z = torch.empty(B, npix * C, device=gpu)
    for b in range(B):
        lib().call("gct2_rng_normal", D.SEED, D.SID, off + b * stride, z[b].data_ptr(), npix * C, stream())
    torch.cuda.synchronize()
    return z.cpu().numpy()


class Plane:
    """a flat fp32 output of n elements inside a sentinel-filled buffer, 64 guard elements on either side; shift: the data starts
    that many elements later - off the 16-byte alignment of the buffer"""

    def __init__(self, shape, gpu, shift=0):
        self.shape, self.n, self.lo = tuple(shape), int(np.prod(shape)), 64 + shift
        self.buf = torch.full((self.lo + self.n + 64,), SENTINEL, dtype=torch.float32, device=gpu)
        self.ptr = self.buf.data_ptr() + 4 * self.lo
        assert self.buf.data_ptr() % 16 == 0

    def got(self):
        torch.cuda.synchronize()
        return self.buf[self.lo:self.lo + self.n].cpu().reshape(self.shape)

    def check(self, want, what):
        E.assert_elementwise_equal(self.got(), torch.as_tensor(want).reshape(self.shape), ("b", "p", "c"), what)
        outside = torch.cat([self.buf[:self.lo], self.buf[self.lo + self.n:]]).cpu()
        assert bool((outside == SENTINEL).all()), f"{what}: the guard band changed"


def shifted(view, shift):
    """a View whose pointer (and the torch view that reads it back) is moved `shift` elements on: an `out` pointer off its alignment"""
    if shift:
        assert shift + view.shape[-1] <= view.view.stride(-2)       # the pixel stays inside its row of ld elements
        view.view = view.buf.as_strided(tuple(view.view.shape), view.view.stride(), view.view.storage_offset() + shift)
        view.ptr += shift * view.buf.element_size()
    return view


def off_alignment(t):
    """a copy of a device tensor whose data starts 4 bytes off a 16-byte boundary"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert flat.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4
    return out


class Outputs:
    """the fp32 plane and the two network-input views of gct2_distill_start / _step: packed (ld 4) and strided (ld 67)"""

    def __init__(self, shape, dt, gpu, shift=0, out2=True):
        """shift: the fp32 plane AND both views start that many elements later (the packed view's pixel then ends at its row's end)"""
        self.z = Plane(shape, gpu, shift)
        self.out = shifted(View(shape, E.TDT[dt], gpu, ld=D.LDOUT), shift)
        self.out2 = shifted(View(shape, E.TDT[dt], gpu, ld=D.LDOUT2), shift) if out2 else None

    def views(self):
        return (self.out.ptr, D.LDOUT, self.out2.ptr if self.out2 else None, D.LDOUT2 if self.out2 else 0)

    def check(self, dt, want, what):
        want = torch.as_tensor(want).reshape(self.z.shape)
        self.z.check(want, what + ": fp32 plane")
        self.out.check(want.to(E.TDT[dt]), what + ": out")
        if self.out2 is not None:
            self.out2.check(want.to(E.TDT[dt]), what + ": out2")


def start(dt, x, eps, pair, dtab, dtt, off, stride, o, t_out, t1_out, shape, n=D.N):
    B, npix, C = shape
    lib().call(START, dt, x.data_ptr(), eps.data_ptr() if eps is not None else None, pair.data_ptr(), dtab.data_ptr(), dtt.data_ptr(), n,
               D.SEED, D.SID, off, stride, o.z.ptr, t_out.ptr if t_out else None, t1_out.ptr if t1_out else None, *o.views(), B, npix * C, C,
               stream())


def step(mode, dt, pred, z0, pair, dtab, clip, o, shape, n=D.N):
    B, npix, C = shape
    lib().call(STEP, mode, dt, pred.data_ptr(), z0.data_ptr(), pair.data_ptr(), dtab.data_ptr(), n, clip, o.z.ptr, *o.views(), B, npix * C, C,
               stream())


def target(mode, pred2, z1, z0, pair, dtab, clip, xo, eo, shape, n=D.N):
    B, npix, C = shape
    lib().call(TARGET, mode, pred2.data_ptr(), z1.data_ptr(), z0.data_ptr(), pair.data_ptr(), dtab.data_ptr(), n, clip, xo.ptr, eo.ptr, B,
               npix * C, stream())


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_start_per_element_and_per_image(gpu, dt, shape):
    """z0 = cx0 x + ck0 e on gct2_rng_normal's draws at offset + b image_stride + i, t and t' of every image's row; the same bits with
    the draws handed in as eps; an fp32 plane one element off its alignment; then image by image gct2_diffusion_start_image at
    a = alpha(t) of that image"""
    tab, tt, dtab, dtt, alpha = tables(gpu)
    B, npix, C = shape
    per, stride = npix * C, stride_of(npix * C)
    x = D.planes(B, per)[1]
    dx, pair = dev(x, gpu), dev(np.int32(D.PAIRS), gpu)
    z = draws(gpu, shape, OFFSET, stride)
    want = D.start_f32(tab, D.PAIRS, x, z)
    rows = tt[np.array(D.PAIRS) - 1]
    what = f"{START} {E.DTYPE_NAMES[dt]} shape {shape}"
    for shift, pinned in ((0, False), (1, False), (0, True)):
        o = Outputs(shape, dt, gpu, shift)
        t_out, t1_out = View((B, 1, 1), torch.int32, gpu), View((B, 1, 1), torch.int32, gpu)
        start(dt, dx, dev(z, gpu) if pinned else None, pair, dtab, dtt, OFFSET, stride, o, t_out, t1_out, shape)
        o.check(dt, want, f"{what} shift {shift} pinned {pinned}")
        t_out.check(torch.tensor(rows[:, 0].reshape(B, 1, 1)), what + ": t_out")
        t1_out.check(torch.tensor(rows[:, 1].reshape(B, 1, 1)), what + ": t1_out")
    o = Outputs(shape, dt, gpu, out2=False)                  # t_out, t1_out and out2 may be NULL
    start(dt, dx, None, pair, dtab, dtt, OFFSET, stride, o, None, None, shape)
    o.check(dt, want, what + " without t_out, t1_out, out2")
    for b in range(B):
        one = (1, npix, C)
        o = Outputs(one, dt, gpu)
        lib().call("gct2_diffusion_start_image", dt, dx[b].data_ptr(), alpha(int(rows[b, 0])), D.SEED, D.SID, OFFSET + b * stride, stride,
                   o.z.ptr, *o.views(), 1, per, C, stream())
        o.check(dt, want[b], f"{what}: image {b} against gct2_diffusion_start_image")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_step_per_element_and_per_image(gpu, dt, mode, shape):
    """the teacher's first step with and without the clip (beyond, on and just past the bound, a NaN and both infinities in pred)
    against the restatement, then image by image gct2_diffusion_step(sigma2 = 0) at that image's (alpha(t), alpha(t'))"""
    tab, tt, dtab, _, alpha = tables(gpu)
    B, npix, C = shape
    per = npix * C
    p, _, z0, _ = D.planes(B, per)
    pred, dz0, pair = dev(p, gpu), dev(z0, gpu), dev(np.int32(D.PAIRS), gpu)
    rows = tt[np.array(D.PAIRS) - 1]
    for clip in D.CLIPS:
        want = D.step_f32(mode, tab, D.PAIRS, p, z0, clip)
        what = f"{STEP} {E.DTYPE_NAMES[dt]} mode {mode} clip {clip} shape {shape}"
        for shift in (0, 1):
            o = Outputs(shape, dt, gpu, shift)
            step(mode, dt, pred, dz0, pair, dtab, clip, o, shape)
            o.check(dt, want, f"{what} shift {shift}")
        for b in range(B):
            o = Outputs((1, npix, C), dt, gpu)
            lib().call("gct2_diffusion_step", mode, dt, pred[b].data_ptr(), dz0[b].data_ptr(), alpha(int(rows[b, 0])), alpha(int(rows[b, 1])),
                       0.0, clip, 0, 0, 0, 0, o.z.ptr, None, *o.views(), 1, per, C, stream())
            o.check(dt, want[b], f"{what}: image {b} against gct2_diffusion_step")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
def test_target_per_element(gpu, mode, shape):
    """the second step fused with the solve, with and without the clip; planes 16-byte aligned (per_image 768: four elements per
    thread) and x_out / eps_out one element off the alignment (one element per thread); pair 1 returns the estimate's own bits"""
    tab, _, dtab, _, _ = tables(gpu)
    B, npix, C = shape
    per = npix * C
    p2, z1, z0, _ = D.planes(B, per)
    dp, dz1, dz0, pair = dev(p2, gpu), dev(z1, gpu), dev(z0, gpu), dev(np.int32(D.PAIRS), gpu)
    for clip in D.CLIPS:
        xt, et, x2, _ = D.target_f32(mode, tab, D.PAIRS, p2, z1, z0, clip)
        first = D.PAIRS.index(1)
        assert ((xt[first].view(np.int32) == x2[first].view(np.int32)) | np.isnan(xt[first])).all()
        for shift in (0, 1):
            xo, eo = Plane(shape, gpu, shift), Plane(shape, gpu, shift)
            if shift == 0:
                assert all(ptr % 16 == 0 for ptr in (dp.data_ptr(), dz1.data_ptr(), dz0.data_ptr(), xo.ptr, eo.ptr))
            target(mode, dp, dz1, dz0, pair, dtab, clip, xo, eo, shape)
            what = f"{TARGET} mode {mode} clip {clip} shape {shape} shift {shift}"
            xo.check(xt, what + ": x_out")
            eo.check(et, what + ": eps_out")
        # ONE input plane 4 bytes off its alignment, everything else aligned: the one-element form must take over, for each of the three
        for k, name in enumerate(("pred2", "z1", "z0")):
            ins = [dp, dz1, dz0]
            ins[k] = off_alignment(ins[k])
            xo, eo = Plane(shape, gpu), Plane(shape, gpu)
            target(mode, *ins, pair, dtab, clip, xo, eo, shape)
            xo.check(xt, f"{TARGET} mode {mode} clip {clip} shape {shape}, {name} off its alignment: x_out")
            eo.check(et, f"{TARGET} mode {mode} clip {clip} shape {shape}, {name} off its alignment: eps_out")


def test_pair_values_are_clamped(gpu):
    """a pair of 0 and of N + 5 behaves as 1 and N in all three kernels (the contract clamps; nothing reads outside the tables)"""
    tab, tt, dtab, dtt, _ = tables(gpu)
    shape = SHAPES[0]
    B, npix, C = shape
    per = npix * C
    p, z1, z0, x = D.planes(B, per)
    dp, dz1, dz0, dx = (dev(a, gpu) for a in (p, z1, z0, x))
    wild, tame = (0, D.N + 5, -2147483648), (1, D.N, 1)
    z = draws(gpu, shape, 0, per)
    for pairs in (wild, tame):
        pair = dev(np.int32(pairs), gpu)
        o = Outputs(shape, F32, gpu)
        t_out, t1_out = View((B, 1, 1), torch.int32, gpu), View((B, 1, 1), torch.int32, gpu)
        start(F32, dx, None, pair, dtab, dtt, 0, per, o, t_out, t1_out, shape)
        o.check(F32, D.start_f32(tab, tame, x, z), f"{START} pairs {pairs}")
        t_out.check(torch.tensor(tt[np.array(tame) - 1][:, 0].reshape(B, 1, 1)), f"{START} pairs {pairs}: t_out")
        o = Outputs(shape, F32, gpu)
        step(D.SAMPLE_EPS, F32, dp, dz0, pair, dtab, 1.0, o, shape)
        o.check(F32, D.step_f32(D.SAMPLE_EPS, tab, tame, p, z0, 1.0), f"{STEP} pairs {pairs}")
        xo, eo = Plane(shape, gpu), Plane(shape, gpu)
        target(D.SAMPLE_V, dp, dz1, dz0, pair, dtab, 0.0, xo, eo, shape)
        xt, et, _, _ = D.target_f32(D.SAMPLE_V, tab, tame, p, z1, z0, 0.0)
        xo.check(xt, f"{TARGET} pairs {pairs}: x_out")
        eo.check(et, f"{TARGET} pairs {pairs}: eps_out")


def test_refuses_bad_arguments_and_launches_nothing(gpu):
    tab, tt, dtab, dtt, _ = tables(gpu)
    shape = SHAPES[0]
    B, npix, C = shape
    per = npix * C
    p, z1, z0, x = (dev(a, gpu) for a in D.planes(B, per))
    pair = dev(np.int32(D.PAIRS), gpu)
    L = lib()
    o, xo, eo = Outputs(shape, F32, gpu), Plane(shape, gpu), Plane(shape, gpu)
    good = dict(mode=D.SAMPLE_EPS, dt=F32, a=p.data_ptr(), b=z0.data_ptr(), c=z1.data_ptr(), pair=pair.data_ptr(), tab=dtab.data_ptr(),
                tt=dtt.data_ptr(), n=D.N, z=o.z.ptr, out=o.out.ptr, ldout=D.LDOUT, ldout2=D.LDOUT2, B=B, per=per, C=C, xo=xo.ptr, eo=eo.ptr)

    def run_start(a):
        L.call(START, a["dt"], a["a"], None, a["pair"], a["tab"], a["tt"], a["n"], 1, 9, 0, a["per"], a["z"], None, None, a["out"], a["ldout"],
               o.out2.ptr, a["ldout2"], a["B"], a["per"], a["C"], stream())

    def run_step(a):
        L.call(STEP, a["mode"], a["dt"], a["a"], a["b"], a["pair"], a["tab"], a["n"], 0.0, a["z"], a["out"], a["ldout"], o.out2.ptr, a["ldout2"],
               a["B"], a["per"], a["C"], stream())

    def run_target(a):
        L.call(TARGET, a["mode"], a["a"], a["c"], a["b"], a["pair"], a["tab"], a["n"], 0.0, a["xo"], a["eo"], a["B"], a["per"], stream())

    views = [dict(dt=3), dict(z=None), dict(out=None), dict(per=per - 1), dict(per=0), dict(C=0), dict(ldout=2), dict(ldout2=2), dict(B=0),
             dict(B=1 << 25)]
    common = [dict(a=None), dict(pair=None), dict(tab=None), dict(n=0), dict(n=-3)]
    modes = [dict(mode=3), dict(mode=4), dict(mode=-1), dict(mode=6)]
    for run, bad in ((run_start, common + views + [dict(tt=None)]), (run_step, common + views + modes + [dict(b=None)]),
                     (run_target, common + modes + [dict(b=None), dict(c=None), dict(xo=None), dict(eo=None), dict(B=0), dict(per=0),
                                                    dict(B=1 << 25)])):
        for change in bad:
            with pytest.raises(L.Gct2Error):
                run(dict(good, **change))
    untouched = torch.full(shape, SENTINEL)
    o.check(F32, untouched, "refused calls")
    xo.check(untouched, "refused calls: x_out")
    eo.check(untouched, "refused calls: eps_out")
    for run in (run_start, run_step, run_target):        # and the good arguments are accepted
        run(good)
    torch.cuda.synchronize()
