"""The fused pieces of the default train step against fp64, ELEMENT BY ELEMENT, on exact-sum inputs (tests/exact_cases.py):

  A. the optimizer step fused behind a weight-gradient call (gct2_adam_args: run at once, or deferred and run by gct2_adam_apply),
     which reads the kernel gradient from the launch's split slabs and everything behind the kernel from the gradient arena;
  B. gct2_dense_head_train: the LDS-tile kernel (no workspace) and the matrix-core kernel plus its ordered finish (with one);
  C. gct2_convT4s2_fwd_head_train: UpShuffle_0's forward with the whole head in its epilogue.

As in tests/test_kernels_exact_gpu.py every sum is exact in an fp32 accumulator whatever its order, so every output must EQUAL the
reference rounded once - no tolerance - and every buffer sits between NaN (inputs) or sentinels (outputs).  The two exceptions are
stated where they are made: the loss (the rounding of 1 / n and of the result: 2 fp32 ulp) and the "wide" head case, whose operands
exceed what the two-term backward pass of the matrix-core kernel carries (a bound derived from the operand widths).
"""
import ctypes

import numpy as np
import pytest
import torch

import clip_cases as K
import exact_cases as E
from exact_cases import BF16, F16, F32, GUARD, SENTINEL
from test_kernels_exact_gpu import FN, MODE_DT, Out, check_log, dev, lib, make_ctx, nan_like, stream, wgrad_family, wgrad_views

pytestmark = pytest.mark.gpu

NAN = float("nan")
MODE_OF = {BF16: "bf16", F16: "f16", F32: "f32"}


def f32(a, gpu):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=gpu)


def whole_buffer_unchanged(o, what):
    torch.cuda.synchronize()
    E.assert_elementwise_equal(o.buf, o.before, ("i",), what + ": changed")


# ---- A. weight gradient + gct2_adam_args, gct2_adam_apply ---------------------------------------------------------------------------

ALPHA, BETA1, BETA2, EPSILON = 1e-3, 0.9, 0.999, 1e-7
TAIL = 7
# (elements behind the kernel in the range, shadow dtype, grad_mul): kernel only / whole-vector padding / padding ending in the scalar
# tail, every shadow type, both multipliers
ALL_COMBOS = [(extra, sdt, gm) for extra in (0, 4, 7) for sdt in (None, BF16, F16, F32) for gm in (1.0, 0.25)]
FEW_COMBOS = [(0, None, 1.0), (4, F16, 1.0), (7, BF16, 0.25), (7, F32, 0.25)]


def adam_state(nw):
    """p, m, v (>= 0) over the longest range and the gradients behind the kernel: seeded fp32 draws"""
    rng = np.random.default_rng([nw, 5])
    n = nw + TAIL
    return (rng.standard_normal(n).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32),
            (0.01 * rng.standard_normal(n) ** 2).astype(np.float32), rng.standard_normal(TAIL).astype(np.float32))


def slabs_in_log(log):
    """number of slabs the launch left for the optimizer step: rsplit=N:slabs -> N, every other launch (one owner, atomics, the direct
    and the 3-channel kernels) hands over the gradient in dw -> 0"""
    assert len(log) == 1, log
    t = log[0]
    return int(t.split("rsplit=")[1].split(":")[0]) if t.endswith(":slabs") else 0


class AdamRun:
    """the arenas of one call: p, m, v and the shadow inside sentinel guards, the gradient arena (dw = its first nw elements, pre-filled
    with the sentinel, then the known gradients behind the kernel) inside NaN guards, db"""

    def __init__(self, gpu, nw, n, sdt, Cout):
        p0, m0, v0, tail = adam_state(nw)
        self.nw, self.n, self.sdt = nw, n, sdt
        self.p, self.m, self.v = (Out(f32(a[:n], gpu), 0, 0, guard=True) for a in (p0, m0, v0))
        self.shadow = None if sdt is None else Out(torch.full((n,), SENTINEL, dtype=E.TDT[sdt], device=gpu), 0, 0, guard=True)
        arena = torch.cat([torch.full((nw,), SENTINEL, dtype=torch.float32, device=gpu), f32(tail[:n - nw], gpu)])
        self.gbuf, self.gptr = E.guarded(arena)
        self.gbefore = self.gbuf.clone()
        self.db = Out(nan_like((Cout,), F32, gpu), 0, 0, guard=True)

    def args(self, grad_mul, defer):
        return lib().AdamArgs(p=self.p.ptr, m=self.m.ptr, v=self.v.ptr, shadow=self.shadow.ptr if self.shadow else None,
                              shadow_dtype=self.sdt or 0, n=self.n, alpha=ALPHA, beta1=BETA1, beta2=BETA2, eps=EPSILON, grad_mul=grad_mul,
                              defer=defer, slab_base=None, nslab=-1, slab_stride=0)

    def state_unchanged(self, what):
        for o, name in ((self.p, "p"), (self.m, "m"), (self.v, "v")) + (((self.shadow, "shadow"),) if self.shadow else ()):
            whole_buffer_unchanged(o, f"{what} {name}")

    def check(self, want, gk, nslab, what):
        """p, m, v, shadow over [0, n) and nothing around them; dw keeps its sentinel where slabs were consumed (else it holds the
        gradient); the gradients behind the kernel and the guards of the arena are as they were"""
        p, m, v = (torch.tensor(a) for a in want)
        self.p.check(p, what + " p", ("i",)); self.m.check(m, what + " m", ("i",)); self.v.check(v, what + " v", ("i",))
        if self.shadow:
            self.shadow.check(p.to(E.TDT[self.sdt]), what + " shadow", ("i",))
        dw = self.gbuf[GUARD:GUARD + self.nw]
        E.assert_elementwise_equal(dw, torch.full_like(dw, SENTINEL).cpu() if nslab else torch.tensor(gk), ("i",), what + " dw")
        E.assert_outside_untouched(self.gbuf, self.gbefore, (slice(GUARD, GUARD + self.nw),), what + " gradient arena")

    def bits(self):
        torch.cuda.synchronize()
        return [o.got().clone() for o in (self.p, self.m, self.v) + ((self.shadow,) if self.shadow else ())]


def run_fused_adam(gpu, entry, shape, mode, ws, tuning=0, family=None, contains=(), nslab=None, combos=ALL_COMBOS):
    dt = MODE_DT[mode]
    cs = E.make_case(entry, shape, dt)
    B, Cin, Cout = shape[0], shape[3], shape[4]
    h, w_ = E.wgrad_hw(entry, shape)
    nw = 16 * Cin * Cout
    gk = E.expected(cs.dw, F32).reshape(-1).numpy()           # the kernel gradient the optimizer must see, whatever the slab count
    db_want = E.expected(cs.db, F32)
    c = make_ctx(gpu, mode, ws, tuning)
    xb, xp, dzb, dzp = wgrad_views(gpu, cs, mode)
    family = family or wgrad_family(entry, shape, mode)
    p0, m0, v0, tail = adam_state(nw)

    def wgrad(run, adam):
        lib().call(FN[entry], c.handle, dt, xp, xb.shape[-1], dzp, dzb.shape[-1], run.gptr, run.db.ptr, B, h, w_, Cin, Cout, 0,
                   ctypes.addressof(adam) if adam is not None else None, stream())
        got = slabs_in_log(check_log(c, family, contains))
        return got

    for extra, sdt, grad_mul in combos:
        n = nw + extra
        what = f"{entry} {shape} {mode} ws={ws} n=nw+{extra} shadow={sdt} grad_mul={grad_mul}"
        g = np.concatenate([gk, tail[:extra]])
        want = K.adam(p0[:n], m0[:n], v0[:n], K.scaled(g, grad_mul), ALPHA, BETA1, BETA2, EPSILON)
        # immediate
        run = AdamRun(gpu, nw, n, sdt, Cout)
        left = wgrad(run, run.args(grad_mul, 0))
        if nslab is not None:
            assert left == nslab, (left, nslab)
        run.check(want, gk, left, what + " immediate")
        run.db.check(db_want, what + " db", ("c",))
        fused = run.bits()
        # deferred: nothing moves before gct2_adam_apply, the struct says what the log says, then the same bits
        run = AdamRun(gpu, nw, n, sdt, Cout)
        a = run.args(grad_mul, 1)
        assert wgrad(run, a) == left
        run.state_unchanged(what + " deferred, before the apply")
        run.db.check(db_want, what + " db", ("c",))
        assert a.nslab == left, (a.nslab, left)
        if left:
            lo, hi = c._ws.data_ptr(), c._ws.data_ptr() + c._ws.numel() * 4
            assert a.slab_stride >= nw and lo <= a.slab_base and a.slab_base + ((left - 1) * a.slab_stride + nw) * 4 <= hi
            # NaN right behind the last slab: a read one slab too far shows in p
            assert bool(torch.isnan(c._ws[(a.slab_base - lo) // 4 + left * a.slab_stride:][:nw]).all())
        lib().call("gct2_adam_apply", ctypes.addressof(a), run.gptr, nw, stream())
        run.check(want, gk, left, what + " deferred")
        for x_, y_ in zip(run.bits(), fused):
            E.assert_elementwise_equal(x_, y_, ("i",), what + " deferred vs immediate")
        # the unfused sequence on the same inputs: the gradient into dw, then gct2_adam_keras_multi
        run = AdamRun(gpu, nw, n, sdt, Cout)
        wgrad(run, None)
        lib().call("gct2_adam_keras_multi", run.p.ptr, run.m.ptr, run.v.ptr, run.gptr, run.shadow.ptr if run.shadow else None, sdt or 0, n,
                   ALPHA, BETA1, BETA2, EPSILON, grad_mul, None, 0, stream())
        run.check(want, gk, 0, what + " unfused")
        for x_, y_ in zip(run.bits(), fused):
            E.assert_elementwise_equal(x_, y_, ("i",), what + " unfused vs fused")
    return c


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("B", E.ADAM_SLAB_BS)
@pytest.mark.parametrize("entry", E.WGRAD_ENTRIES)
def test_fused_adam_slab_counts_exact(gpu, entry, B, mode):
    """nslab in {0 (one owner), 2, 8, 9, 10, 17}: the remainder loop alone, one batch of eight loads, a batch plus one, two batches,
    and the dw path; the count is asserted from the launch log and from the struct"""
    run_fused_adam(gpu, entry, E.adam_slab_shape(B), mode, True, family="wgrad:128:", contains=(f"rsplit={B}:" + ("slabs" if B > 1 else "owner"),),
                   nslab=B if B > 1 else 0)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("entry", E.WGRAD_ENTRIES)
def test_fused_adam_production_tile_exact(gpu, entry, mode):
    c = run_fused_adam(gpu, entry, E.WGRAD_TUNING_SHAPE, mode, True, tuning=2 << 16, family="wgrad:256q:", contains=("rsplit=4:slabs",), nslab=4,
                       combos=FEW_COMBOS)
    assert c.read_launch_log() == []


@pytest.mark.parametrize("entry", E.WGRAD_ENTRIES)
def test_fused_adam_f32_matrix_slabs_exact(gpu, entry):
    run_fused_adam(gpu, entry, E.WGRAD_TUNING_SHAPE, "f32m", True, tuning=3 << 28, family="f32mfma:wgrad:", contains=("rsplit=4:slabs",), nslab=4,
                   combos=FEW_COMBOS)


@pytest.mark.parametrize("entry,shape,mode,ws,token", [
    ("conv_wgrad", E.adam_slab_shape(2), "f32", False, "direct:wgrad"), ("convT_wgrad", E.adam_slab_shape(2), "f32", False, "direct:wgrad"),
    ("conv_wgrad", (2, 16, 16, 3, 8), "bf16", True, "rgb:wgrad"), ("conv_wgrad", (2, 16, 16, 3, 8), "f16", True, "rgb:wgrad"),
    ("convT_wgrad", (2, 16, 16, 3, 8), "bf16", True, "direct:wgrad"),
    ("conv_wgrad", E.adam_slab_shape(8), "bf16", False, "rsplit=8:atomics"), ("convT_wgrad", E.adam_slab_shape(8), "f16", False, "rsplit=8:atomics")])
def test_fused_adam_gradient_in_dw_exact(gpu, entry, shape, mode, ws, token):
    """the launches that must hand over nslab = 0: the fp32 direct kernels, the 3-channel layer (it reduces its own slabs), and a
    16-bit split launch without a workspace (atomics into dw)"""
    run_fused_adam(gpu, entry, shape, mode, ws, contains=(token,), nslab=0, combos=FEW_COMBOS)


# ---- B. gct2_dense_head_train ---------------------------------------------------------------------------------------------------------

PAD = 5.0                                     # what the LDS kernel finds in the pad channels [Cin, ld) of x: finite (it multiplies them by zero)
HEAD_ROW = 288


class HeadCall:
    """buffers of one gct2_dense_head_train call on the inputs `cs` (an exact head case): x and dx poisoned views, w / b / target
    inside NaN guards, every output inside sentinels"""

    def __init__(self, gpu, cs, dt, variant, with_pred, accumulate, xin=None):
        Cin, Cout, ld, Cmask = E.HEAD_SHAPE
        x = cs.x if xin is None else xin
        M = x.shape[0]
        self.M, self.dt, self.variant = M, dt, variant
        split = variant == "ws_x2"
        self.xb, self.xp = E.poisoned_view(dev(x[:, :Cmask if split else Cin], dt, gpu), ld, 0)
        if variant == "lds":
            self.xb[1:-1, Cin:] = PAD
        self.x2b, self.x2p = E.poisoned_view(dev(x[:, Cmask:], dt, gpu), 4, 0) if split else (None, None)      # slot 3: NaN
        self.wb, self.wp = E.guarded(dev(cs.w, F32, gpu))
        self.bb, self.bp = E.guarded(dev(cs.bias, F32, gpu))
        self.tb, self.tp = E.guarded(dev(cs.target, F32, gpu))
        self.sb, self.sp = E.guarded(f32([cs.loss_scale], gpu))
        self.pred = Out(nan_like((M, Cout), F32, gpu), 0, 0, guard=True) if with_pred else None
        self.dx = Out(nan_like((M, Cmask), dt, gpu), ld, 0)
        init = lambda prev, shape: dev(prev, F32, gpu) if accumulate else nan_like(shape, F32, gpu)
        self.dw = Out(init(getattr(cs, "prev_dw", None), (Cin, Cout)), 0, 0, guard=True)
        self.db = Out(init(getattr(cs, "prev_db", None), (Cout,)), 0, 0, guard=True)
        self.db_dx = Out(init(getattr(cs, "prev_db_dx", None), (Cmask,)), 0, 0, guard=True)
        self.loss = Out(nan_like((1,), F32, gpu), 0, 0, guard=True)
        self.partials = torch.full((1024,), NAN, dtype=torch.float32, device=gpu)
        self.accumulate = accumulate

    def run(self, c):
        Cin, Cout, ld, Cmask = E.HEAD_SHAPE
        lib().call("gct2_dense_head_train", c.handle, self.dt, self.xp, ld, self.wp, self.bp, self.tp, self.pred.ptr if self.pred else None,
                   self.dx.ptr, ld, self.dw.ptr, self.db.ptr, self.loss.ptr, self.partials.data_ptr(), self.M, Cin, Cout, Cmask, self.sp,
                   self.db_dx.ptr, self.x2p, 4 if self.x2p else 0, self.accumulate, stream())
        torch.cuda.synchronize()

    def kernel_that_ran(self, c):
        """the entry point logs nothing; the two kernels leave their partial sums in different places: the LDS kernel one float per
        work-group in `partials`, the matrix-core kernel one row per work-group at the start of the workspace"""
        assert c.read_launch_log() == []
        if self.variant == "lds":
            tiles = min((self.M + 255) // 256, 1024)
            assert bool(torch.isfinite(self.partials[:tiles]).all()) and bool(torch.isnan(self.partials[tiles:]).all())
        else:
            rows = min(512, ((self.M + 15) // 16 + 3) // 4)
            assert bool(torch.isfinite(c._ws[:rows * HEAD_ROW]).all()) and bool(torch.isnan(c._ws[rows * HEAD_ROW:rows * HEAD_ROW + 4096]).all())
            assert bool(torch.isnan(self.partials).all())


def assert_loss(got, want, what):
    """sum d^2 is exact; the rounding of 1 / n to fp32 and of the result remain: 2 fp32 ulp of sum d^2 / n evaluated in fp64"""
    got = float(got.got()[0])
    ulp = float(np.spacing(np.float32(want)))
    print(f"{what}: loss {got!r} want {want!r} ({abs(got - want) / ulp:.3f} ulp)")
    assert abs(got - want) <= 2 * ulp, (what, got, want)


def check_head_outputs(h, cs, stored_sums, what):
    k = h.accumulate
    if h.pred:
        h.pred.check(E.expected(cs.pred_r, F32), what + " pred", ("m", "o"))
    h.dx.check(E.expected(cs.dx, h.dt), what + " dx", ("m", "c"))           # channels [Cmask, ld) and the guard rows keep their sentinel
    h.dw.check(E.expected(cs.dw + k * cs.prev_dw, F32), what + " dw", ("c", "o"))
    h.db.check(E.expected(cs.db + k * cs.prev_db, F32), what + " db", ("o",))
    h.db_dx.check(E.expected((cs.db_dx_stored if stored_sums else cs.db_dx) + k * cs.prev_db_dx, F32), what + " db_dx", ("c",))
    assert_loss(h.loss, cs.loss, what)
    E.assert_outside_untouched(h.loss.buf, h.loss.before, h.loss.inside, what + " loss")


@pytest.mark.parametrize("variant", ["lds", "ws", "ws_x2"])
@pytest.mark.parametrize("M", E.HEAD_MS)
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_dense_head_train_exact(gpu, dt, M, variant):
    """less than one 16-pixel group, exactly one, a ragged 256-pixel tile and group, more than one trip per wave; both kernels and the
    split input; accumulate 0 (over NaN) and 1 (onto addends on the grid); pred given and NULL.  The matrix-core kernel masks the pad
    channels (NaN there, and in x's own image slice when x2 carries it); the LDS kernel multiplies them by zero weights, so it gets a
    finite value there, which must not leak anywhere.
    M = 32775 does not reach the low term of dpred in the matrix-core backward pass: the budget of db_dx leaves |delta| <= 15 there,
    four bits.  M = 16 and 1000 in bf16 do (tests/test_exact_cases_cpu.py asserts it)."""
    cs = E.make_case("head_train", (M, 67, 3), dt)
    for accumulate, with_pred in ((0, True), (1, False), (1, True)):
        c = make_ctx(gpu, MODE_OF[dt], ws=variant != "lds")          # a NaN workspace of its own: where the partial rows land is fresh evidence
        h = HeadCall(gpu, cs, dt, variant, with_pred, accumulate)
        h.run(c)
        h.kernel_that_ran(c)
        check_head_outputs(h, cs, variant == "lds", f"head_train {MODE_OF[dt]} M={M} {variant} accumulate={accumulate} pred={with_pred}")


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_dense_head_train_wide_operands(gpu, dt):
    """The one case whose dx reference depends on an output of the code under test: dx is compared with fp64 evaluated on the kernel's
    OWN prediction; the prediction itself carries the independence and is bounded against fp64 alone.

    M = 64, weights with 24 significant bits, |pred - target| up to 2^12 steps.  A dense 67-term sum with 24-bit weights cannot be an
    exact fp32 sum, and d = pred - target cancels, so dx is sensitive to the last bit of pred: hence the reference above.  The
    matrix-core kernel carries w as three terms of the storage type in the forward pass (fp32 accuracy) and w and d as TWO terms each
    in the backward pass, without the product of the two low terms.  With s significand bits, round to nearest, and P(a) the power of
    two at or below |a| (half an ulp of a is 2^-s P(a), between 2^-(s+1) |a| and 2^-s |a|):
        |a - hi| <= 2^-s P(a);   the rest r either equals that bound (a power of two: lo is exact) or P(r) <= 2^-(s+1) P(a), so
        |a - hi - lo| <= 2^-(2s+1) P(a)   and   |lo| <= 2^-s P(a)
    (fp16: a low term below 2^-14 is a subnormal with steps of 2^-24: at most max(., 2^-25); dpred IS an fp16 value there: no rest).
    Per product: |d| res(w) + res(d) |w| + res(d) res(w) + |lo_d| |lo_w|, about 2^-16 |w d| in bf16 as the kernel's comment says; plus
    the fp32 sums of the 9 products of the two matrix-core instructions (9 * 2^-24 of the magnitudes); plus half an ulp of the store,
    2^-s P(value) (fp16 subnormals: 2^-25).  Nothing here is measured: the bound follows from the widths alone."""
    cs = E.make_case("head_train", (E.HEAD_WIDE_M, 67, 3), dt, "wide")
    Cin, Cout, ld, Cmask = E.HEAD_SHAPE
    s = E.SIG_BITS[dt]
    c = make_ctx(gpu, MODE_OF[dt], ws=True)
    h = HeadCall(gpu, cs, dt, "ws", True, 0)
    h.run(c)
    h.kernel_that_ran(c)
    pred = h.pred.got().double().cpu().numpy()
    # forward: nine fp32 matrix-core accumulations of three-term operands (2^-24 |w| each) and the bias: 16 * 2^-24 of the magnitudes;
    # GCT2_F16 rounds the result to fp16, where a flip is one fp16 ulp (2^-10 |pred|)
    mag = cs.x @ np.abs(cs.w) + np.abs(cs.bias)
    want_pred = cs.pred if dt == BF16 else E._round_to(cs.pred, F16)
    perr = np.abs(pred - want_pred) / (16 * 2.0 ** -24 * mag + (2.0 ** -10 * np.abs(cs.pred) if dt == F16 else 0))
    print(f"wide pred: worst error / bound {perr.max():.3f}")
    assert perr.max() <= 1
    d = (pred.astype(np.float32) - cs.target.astype(np.float32)).astype(np.float64)          # the kernel's own fp32 subtraction
    dp = d * cs.gscale
    if dt == F16:
        dp = E._round_to(dp, F16)
    floor = 2.0 ** -25 if dt == F16 else 0.0
    P = lambda a: np.where(a != 0, np.ldexp(1.0, np.frexp(np.abs(a))[1] - 1), 0.0)            # the power of two at or below |a|
    res = lambda a: np.where(a != 0, np.maximum(2.0 ** (-2 * s - 1) * P(a), floor), 0.0)       # what two terms leave of an operand
    low = lambda a: 2.0 ** -s * P(a)                                                           # the size of its low term
    w = cs.w[:Cmask]
    aw, ad = np.abs(w), np.abs(dp)
    rw, lo_w = res(w), low(w)
    rd, lo_d = (res(dp), low(dp)) if dt == BF16 else (np.zeros_like(dp), np.zeros_like(dp))    # (powers of two: d and dpred split alike)
    split_err = ad @ rw.T + rd @ aw.T + rd @ rw.T + lo_d @ lo_w.T
    ref = dp @ w.T
    bound = split_err + 9 * 2.0 ** -24 * (ad @ aw.T)
    bound = bound + np.maximum(2.0 ** -s * P(np.abs(ref) + bound), floor)
    mask = cs.x[:, :Cmask] > 0
    got = h.dx.got().double().cpu().numpy()
    ratio = np.abs(got - np.where(mask, ref, 0.0)) / np.maximum(bound, 1e-300)
    print(f"wide dx: worst error / bound {ratio.max():.3f}, median {np.median(ratio[mask]):.3f}")
    assert (got[~mask] == 0).all() and ratio.max() <= 1
    E.assert_outside_untouched(h.dx.buf, h.dx.before, h.dx.inside, "wide dx")


# ---- C. gct2_convT4s2_fwd_head_train --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", E.CONVT_HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_convT_fwd_head_train_exact(gpu, dt, shape):
    """the smallest shape the entry accepts and one with a ragged K and several patches.  y = relu(convT(x) + bias) is an exact sum of
    which a share is really rounded by the 16-bit conversion; the head reads the rounded y.  pred, dy (the masked head gradient,
    rounded once), db (its column sums), head_dw, head_db bit for bit, the loss within 2 ulp; accumulate 0 and 1; the workspace is
    exactly the documented B (H/16) (W/16) 288 floats with NaN behind it.  Then the same inputs through gct2_convT4s2_fwd into a
    stored y followed by gct2_dense_head_train: identical bits, because every sum is exact."""
    cs = E.make_case("convT_head", shape, dt)
    B, H, W, Cin = shape
    Cout, hCin, hCout, ld = 64, 67, 3, 72
    M = B * 4 * H * W
    mode = MODE_OF[dt]
    rows = B * (H // 16) * (W // 16)
    c = make_ctx(gpu, mode)
    wsbuf = torch.full((rows * HEAD_ROW + 4096,), NAN, dtype=torch.float32, device=gpu)
    c.set_workspace(wsbuf[:rows * HEAD_ROW])
    xb, xp = E.poisoned_view(dev(cs.xc, dt, gpu), Cin + 16, 8)
    wb, wp = E.guarded(dev(cs.wc, dt, gpu))
    bb, bp = E.guarded(dev(cs.bc, F32, gpu))
    hwb, hwp = E.guarded(dev(cs.w, F32, gpu))
    hbb, hbp = E.guarded(dev(cs.bias, F32, gpu))
    tb, tp = E.guarded(dev(cs.target, F32, gpu))
    sb, sp = E.guarded(f32([cs.loss_scale], gpu))
    x2b, x2p = E.poisoned_view(dev(cs.img, dt, gpu), 4, 0)                                   # packed image: NaN in slot 3
    want = dict(pred=E.expected(cs.pred_r, F32), dy=E.expected(cs.dx.reshape(B, 2 * H, 2 * W, Cout), dt))
    fused = {}
    for accumulate in (0, 1):
        what = f"convT_fwd_head_train {shape} {mode} accumulate={accumulate}"
        init = lambda prev, shp: dev(prev, F32, gpu) if accumulate else nan_like(shp, F32, gpu)
        pred = Out(nan_like((M, hCout), F32, gpu), 0, 0, guard=True)
        dy = Out(nan_like((B, 2 * H, 2 * W, Cout), dt, gpu), ld, 0)
        hdw, hdb = Out(init(cs.prev_dw, (hCin, hCout)), 0, 0, guard=True), Out(init(cs.prev_db, (hCout,)), 0, 0, guard=True)
        db = Out(init(cs.prev_db_dx, (Cout,)), 0, 0, guard=True)
        loss = Out(nan_like((1,), F32, gpu), 0, 0, guard=True)
        lib().call("gct2_convT4s2_fwd_head_train", c.handle, dt, xp, xb.shape[-1], wp, bp, hwp, hbp, tp, pred.ptr, dy.ptr, ld, hdw.ptr, hdb.ptr,
                   loss.ptr, B, H, W, Cin, Cout, hCin, hCout, sp, db.ptr, x2p, 4, accumulate, stream())
        torch.cuda.synchronize()
        assert check_log(c, "halo:convT:head") == ["halo:convT:head"]
        assert bool(torch.isnan(wsbuf[rows * HEAD_ROW:]).all()), "the kernel wrote behind the documented workspace"
        pred.check(want["pred"], what + " pred", ("m", "o"))
        dy.check(want["dy"], what + " dy")
        db.check(E.expected(cs.db_dx + accumulate * cs.prev_db_dx, F32), what + " db", ("c",))
        hdw.check(E.expected(cs.dw + accumulate * cs.prev_dw, F32), what + " head_dw", ("c", "o"))
        hdb.check(E.expected(cs.db + accumulate * cs.prev_db, F32), what + " head_db", ("o",))
        assert_loss(loss, cs.loss, what)
        fused[accumulate] = [o.got().clone() for o in (pred, dy, hdw, hdb, db, loss)]
    # the unfused pair on the same inputs: y stored (poisoned view, ld 72: the head's input), then the matrix-core head with x2
    c2 = make_ctx(gpu, mode)
    y = Out(nan_like((B, 2 * H, 2 * W, Cout), dt, gpu), ld, 0)
    lib().call("gct2_convT4s2_fwd", c2.handle, dt, xp, xb.shape[-1], wp, bp, y.ptr, ld, B, H, W, Cin, Cout, 1, stream())
    y.check(E.expected(cs.y, dt), f"convT_fwd {shape} {mode} y")
    c2.read_launch_log()
    for accumulate in (0, 1):
        h = HeadCall(gpu, cs, dt, "ws_x2", True, accumulate)
        h.xb[1:-1, :Cout] = y.got().reshape(M, Cout)                                         # the stored activations, bit for bit
        c3 = make_ctx(gpu, mode, ws=True)
        h.run(c3)
        h.kernel_that_ran(c3)
        got = [o.got() for o in (h.pred, h.dx, h.dw, h.db, h.db_dx, h.loss)]
        for a, b_, name in zip(got[:5], fused[accumulate][:5], ("pred", "dy", "head_dw", "head_db", "db")):
            E.assert_elementwise_equal(a.reshape(b_.shape), b_, what=f"unfused vs fused {shape} {mode} accumulate={accumulate} {name}")
