"""The L2 weight regularizer and the sign transformer (train.py:47-48, 71-74, 80) on the GPU: gct2_optimizer_apply_reg per element and
bit for bit (every kind, every shadow type, l2 / sign / both, every clipping mode, plain / loss-scaled / skipped, one launch over the
arena and one per segment, a range the grid-stride loop walks twice), its identity with the unregularized siblings,
gct2_grad_sumsq_l2 on exact-sum inputs, gct2_l2_penalty, train steps of both engines against numpy - eager and planned, through the
public interface, with loss scaling - the variant engine's unregularized projection, the untouched default step, and what is refused.

The reference of every comparison is the arithmetic of include/gct2.h restated in tests/reg_cases.py (tests/clip_cases.py and
tests/optimizer_cases.py for the clipping and the kinds' updates); every comparison is bit for bit, nothing is measured - but for one
bound: a float64 sum of squares over real values is compared with numpy's within the bound of any summation order, count * 2^-53
relative, the one tests/test_clip_gpu.py derives for gct2_grad_sumsq.  Buffers carry NaN in every gap and guard of what a kernel
reads, sentinels around every range it may write, and NaN poison in the slots a kind must not touch.
PARITY UNPINNED w.r.t. TensorFlow (there is none here)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import clip_cases as K
import reg_cases as RC

pytestmark = pytest.mark.gpu
TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
NEW = ("gct2_optimizer_apply_reg", "gct2_grad_sumsq_l2", "gct2_l2_penalty")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_step.npz")
TOPO, SIZE, BATCH = (8, 16, 2), 16, 2                 # the tiny network of tests/golden/tiny_step.npz


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def cast(dt, src):
    """what gct2_cast_from_f32 writes from an fp32 device tensor: the project's one round-to-nearest-even conversion"""
    src = src.contiguous()
    out = torch.empty(src.numel(), dtype=TDT[dt], device=src.device)
    lib().call("gct2_cast_from_f32", dt, src.data_ptr(), out.data_ptr(), src.numel(), stream())
    return out


def bits(a):
    """int32 view of a float32 numpy array or device tensor (as numpy)"""
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same(dev, want):
    """float32 device tensor == numpy array: NaN where NaN, the same bits (so also the sign of zero) everywhere else
    (tests/test_optimizers_gpu.py's comparison)"""
    got = dev.detach().cpu().numpy()
    want = np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))


def ls_state(gpu, scale=2.0 ** 15, found_inf=0, alpha=0.0, applied_steps=0, good_steps=0):
    """a gct2_loss_scale_state on the device: {scale, inv_scale, good_steps, found_inf, applied_steps, alpha, reserved[2]}"""
    st = torch.zeros(8, dtype=torch.int32, device=gpu)
    lib().call("gct2_loss_scale_init", st.data_ptr(), float(scale), stream())
    st[2], st[3], st[4] = good_steps, found_inf, applied_steps
    st.view(torch.float32)[5] = alpha
    return st


@pytest.fixture
def recorded(monkeypatch):
    """names(plan) -> the entry-point names a step plan recorded, in order (Plan.add_call is watched while the test runs)"""
    P = lib().Plan
    orig, log = P.add_call, {}

    def add_call(self, name, args):
        orig(self, name, args)
        if name in lib().PLANNABLE:
            log.setdefault(id(self), []).append(name)
    monkeypatch.setattr(P, "add_call", add_call)
    return lambda plan: log.get(id(plan), [])


# ---- 1. gct2_optimizer_apply_reg, per element and bit for bit ---------------------------------------------------------------------
ADAM_HYPER = dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7)
KINDS = {"adam": (RC.ADAM, ADAM_HYPER), "sgd": (RC.SGD, {}), "sgd_momentum": (RC.SGD, dict(momentum=0.5)),
         "sgd_nesterov": (RC.SGD, dict(momentum=0.5, nesterov=True)), "rmsprop": (RC.RMSPROP, dict(rho=0.9, epsilon=1e-7)),
         "rmsprop_momentum": (RC.RMSPROP, dict(rho=0.9, momentum=0.9, epsilon=1e-7))}
L2 = 0.3                                             # c = fl(0.6): c * p rounds, so a contracted multiply-add would show
C = RC.coefficient(L2)
SETTINGS = {"l2": (C, RC.GRAD_NONE), "sign": (np.float32(0.0), RC.GRAD_SIGN), "l2_sign": (C, RC.GRAD_SIGN)}
MODES = {"none": K.CLIP_NONE, "value": K.CLIP_VALUE, "norm": K.CLIP_NORM, "global": K.CLIP_GLOBAL_NORM}
LR, LS_LR, LS_SCALE, GRAD_MUL = 1.5e-3, 2.5e-3, 2.0 ** 7, 0.5
FACTORS = (GRAD_MUL, GRAD_MUL / LS_SCALE)            # the two factors g is scaled by: plain, loss-scaled
P_FILL, M_FILL, V_FILL, SH_FILL = 12345.0, -12345.0, 24690.0, 77.0
POISON = {"m": 0x7FC00A0A, "v": 0x7FC00B0B}          # quiet NaNs with a payload of their own: an untouched slot keeps these very bits


def build_arena(segs, total, seed):
    """g: NaN in every gap and in both guards; p, m, v: values over the whole range a launch may cover (the gaps included), sentinels
    in the guards.  The first elements of every segment long enough hold +-0 and the exact cancellations of reg_cases"""
    lo, hi = K.GUARD, total - K.GUARD
    assert segs[0][0] == lo and segs[-1][0] + segs[-1][1] <= hi and all(b % 4 == 0 for b, _ in segs)
    rng = np.random.default_rng(seed)
    g = K.poisoned(lambda s, n: rng.standard_normal(n).astype(np.float32), segs, total)
    inner = lambda fill, vals: np.concatenate([np.full(lo, fill, np.float32), vals.astype(np.float32), np.full(total - hi, fill, np.float32)])
    p = inner(P_FILL, rng.standard_normal(hi - lo))
    m = inner(M_FILL, rng.standard_normal(hi - lo) * 1e-2)
    v = inner(V_FILL, rng.random(hi - lo) * 1e-4)
    cancel = RC.plant_zeros_and_cancellations(g, p, segs, C, FACTORS)
    return types.SimpleNamespace(segs=segs, total=total, lo=lo, hi=hi, g=g, p=p, m=m, v=v, cancel=cancel)


@pytest.fixture(scope="module")
def arena(gpu):
    """clip_cases.layout(): ten segments of 1 .. 3 CHUNK + 7 elements at 64-element alignment between two guards"""
    segs, total = K.layout()
    assert [c for _, c in segs] == list(K.SEGMENT_LENGTHS)
    A = build_arena(segs, total, 78)
    assert len(A.cancel) == 2 * sum(c >= 5 for _, c in segs) >= 12
    gp = K.scaled(A.g, GRAD_MUL)
    plain = A.cancel[0::2]
    assert all(RC.regularized(gp, A.p, C)[i] == 0 for i in plain) and all(gp[i] != 0 for i in plain)
    return A


class Run:
    """device copies of the arena for one case: the slots the kind does not use hold NaN poison instead of values"""

    def __init__(self, gpu, A, kind, hyper, dt, host=None):
        self.A, self.kind, self.hyper, self.dt = A, kind, hyper, dt
        self.use_m, self.use_v = kind == RC.ADAM or hyper.get("momentum", 0.0) > 0, kind != RC.SGD
        self.host = host or dict(p=A.p, g=A.g, m=A.m if self.use_m else np.full(A.total, POISON["m"], np.int32).view(np.float32),
                                 v=A.v if self.use_v else np.full(A.total, POISON["v"], np.int32).view(np.float32))
        self.dev = {k: torch.from_numpy(a.copy()).to(gpu) for k, a in self.host.items()}
        self.sh = torch.full((A.total,), SH_FILL, dtype=TDT[dt], device=gpu) if dt else None
        self.sh0 = self.sh.clone() if dt else None

    def args(self, lo, n, lr, grad_mul, ls, mode, clip, sumsq_ptr, pass_unused=True):
        """the arguments gct2_optimizer_apply takes (Adam's betas in the momentum / rho positions)"""
        d, h = self.dev, self.hyper
        ptr = lambda k, used: d[k].data_ptr() + 4 * lo if (used or pass_unused) else None
        first, second = (h["beta_1"], h["beta_2"]) if self.kind == RC.ADAM else (h.get("momentum", 0.0), h.get("rho", 0.9))
        return [self.kind, ptr("p", True), ptr("m", self.use_m), ptr("v", self.use_v), ptr("g", True),
                self.sh.data_ptr() + 2 * lo if self.dt else None, self.dt, n, float(lr), float(first), int(h.get("nesterov", False)), float(second),
                float(h.get("epsilon", 1e-7)), float(grad_mul), None if ls is None else ls.data_ptr(), mode, float(clip), sumsq_ptr]

    def launch(self, lo, n, lr, c, transform, grad_mul=1.0, ls=None, mode=K.CLIP_NONE, clip=0.0, sumsq_ptr=None, pass_unused=True):
        lib().call("gct2_optimizer_apply_reg", *self.args(lo, n, lr, grad_mul, ls, mode, clip, sumsq_ptr, pass_unused), float(c), transform, stream())

    def expect(self, ranges, lr, c, transform, grad_mul=1.0, inv_scale=1.0, mode=K.CLIP_NONE, clip=0.0, ss=None):
        """the arenas after launches over `ranges` ((lo, n) pairs; ss: one float64 per range): numpy over exactly those elements"""
        out = {k: self.host[k].copy() for k in ("p", "m", "v")}
        for r, (lo, n) in enumerate(ranges):
            sl = slice(lo, lo + n)
            p, m, v = RC.apply(self.kind, out["p"][sl], out["m"][sl], out["v"][sl], self.host["g"][sl], lr, self.hyper, c, transform, mode, clip,
                               None if ss is None else ss[r], grad_mul, inv_scale)
            out["p"][sl] = p
            if self.use_m:
                out["m"][sl] = m
            if self.use_v:
                out["v"][sl] = v
        return out

    def check(self, want, ranges, tag):
        torch.cuda.synchronize()
        d = self.dev
        assert np.array_equal(bits(d["g"]), bits(self.host["g"])), tag                  # g is read only: it keeps the data-term gradient
        for k in ("p", "m", "v"):
            used = k == "p" or (k == "m" and self.use_m) or (k == "v" and self.use_v)
            if used:                                             # values inside the ranges, the initial bits (sentinels too) outside
                assert same(d[k], want[k]), (tag, k)
            else:                                                # never touched: the poison's very bits
                assert np.array_equal(bits(d[k]), np.full(self.A.total, POISON[k], np.int32)), (tag, k)
        if self.dt:
            mask = torch.zeros(self.A.total, dtype=torch.bool, device=self.sh.device)
            for lo, n in ranges:
                mask[lo:lo + n] = True
            new = cast(self.dt, d["p"])
            nan = torch.isnan(new) & mask
            assert torch.equal(torch.isnan(self.sh) & mask, nan), tag
            ok = mask & ~nan
            assert torch.equal(self.sh[ok].view(torch.int16), new[ok].view(torch.int16)), tag      # the shadow is the cast of the new p
            assert torch.equal(self.sh[~mask].view(torch.int16), self.sh0[~mask].view(torch.int16)), tag


def sums_for(A, ranges, c, grad_mul, inv_scale, mode):
    """the ONE float64 each launch of a norm mode reads: the regularized gradient's sum of squares over the launch's own elements
    inside segments (clipnorm) or over all segments (global_clipnorm) - numpy's, uploaded; any finite value would do for the kernel"""
    if mode not in (K.CLIP_NORM, K.CLIP_GLOBAL_NORM):
        return None
    per = RC.regularized_sumsq(A.g, A.p, A.segs, [c] * len(A.segs), grad_mul, inv_scale)
    if mode == K.CLIP_GLOBAL_NORM or len(ranges) == 1:
        return [per[-1]] * len(ranges)
    return list(per[:-1])


@pytest.mark.parametrize("dt", [0, 1, 2], ids=["noshadow", "bf16", "f16"])
@pytest.mark.parametrize("name", list(KINDS))
def test_optimizer_apply_reg_per_element(gpu, arena, name, dt):
    kind, hyper = KINDS[name]
    whole = [(arena.lo, arena.hi - arena.lo)]
    moved = 0
    for shape, ranges in (("whole", whole), ("per_segment", list(arena.segs))):
        for sname, (c, transform) in SETTINGS.items():
            for mname, mode in MODES.items():
                clip = {"none": 0.0, "value": 0.5, "norm": 1.0, "global": 150.0}[mname]      # (norm: tensors on either side of it)
                for scaling in ("plain", "loss_scaled", "found_inf"):
                    tag = (name, dt, shape, sname, mname, scaling)
                    inv_scale = 1.0 if scaling == "plain" else 1.0 / LS_SCALE
                    ss = sums_for(arena, ranges, c, GRAD_MUL, inv_scale, mode)
                    dev_ss = torch.tensor(ss, dtype=torch.float64, device=gpu) if ss is not None else None
                    ls = None if scaling == "plain" else ls_state(gpu, LS_SCALE, found_inf=int(scaling == "found_inf"), alpha=LS_LR)
                    R = Run(gpu, arena, kind, hyper, dt)
                    for r, (lo, n) in enumerate(ranges):
                        R.launch(lo, n, LR if ls is None else 123.0, c, transform, GRAD_MUL, ls, mode, clip,
                                 None if ss is None else dev_ss.data_ptr() + 8 * r, pass_unused=(shape == "whole"))
                    if scaling == "found_inf":                   # nothing at all is written
                        R.check(R.expect([], LR, c, transform), [], tag)
                        assert int(ls[3]) == 1
                        continue
                    want = R.expect(ranges, LR if ls is None else LS_LR, c, transform, GRAD_MUL, inv_scale, mode, clip, ss)
                    R.check(want, ranges, tag)
                    moved += not np.array_equal(bits(want["p"]), bits(arena.p))
                    if ls is not None:
                        assert int(ls[3]) == 0                   # nothing here sets the flag
    assert moved == 2 * len(SETTINGS) * len(MODES) * 2           # (every applied step moved something)


def test_the_settings_are_visible_in_the_result(gpu, arena):
    """the three settings give three different results, each different from the unregularized one - in the restatement the per-element
    test compares with, so that an implementation ignoring a setting cannot pass it"""
    R = Run(gpu, arena, RC.ADAM, ADAM_HYPER, 0)
    whole = [(arena.lo, arena.hi - arena.lo)]
    outs = [bits(R.expect(whole, LR, c, t, GRAD_MUL)["p"]).tobytes() for c, t in [(0.0, RC.GRAD_NONE)] + list(SETTINGS.values())]
    assert len(set(outs)) == 4
    # the planted elements: a zero sum, of either sign, has the sign +0 - m of a sign-SGD-like step shows the transformed gradient
    g2 = RC.gradient(arena.g, arena.p, C, RC.GRAD_SIGN, grad_mul=GRAD_MUL)
    for b, n in arena.segs:
        if n >= 5:
            assert [g2[b], g2[b + 1], g2[b + 2], g2[b + 3]] == [0, 0, 1, 0] and not np.signbit(g2[[b, b + 1, b + 3]]).any()
    gr = RC.regularized(K.scaled(arena.g, GRAD_MUL), arena.p, C)
    b = next(b for b, n in arena.segs if n >= 5)
    assert np.signbit(gr[b + 1]) and not np.signbit(gr[b]) and not np.signbit(gr[b + 3])


def test_grid_stride_loop_runs_twice(gpu):
    """n = 2048 * 256 * 4 + 1027: more float4 groups than the largest grid has threads, so the loop's second trip is taken, and a
    3-element tail"""
    n = 2048 * 256 * 4 + 1027
    assert n % 4 == 3 and n // 4 > 2048 * 256
    A = build_arena([(K.GUARD, n)], (K.GUARD + n + 63) // 64 * 64 + K.GUARD, 5)
    R = Run(gpu, A, RC.ADAM, ADAM_HYPER, 1)
    ranges = [(K.GUARD, n)]
    R.launch(K.GUARD, n, LR, C, RC.GRAD_SIGN, GRAD_MUL, None, K.CLIP_VALUE, 0.5)
    want = R.expect(ranges, LR, C, RC.GRAD_SIGN, GRAD_MUL, 1.0, K.CLIP_VALUE, 0.5)
    R.check(want, ranges, "grid_stride")
    last = K.GUARD + n - 1
    assert bits(want["p"])[last] != bits(A.p)[last] and bits(want["p"])[K.GUARD + 2048 * 256 * 4] != bits(A.p)[K.GUARD + 2048 * 256 * 4]


# ---- 2. identity with the siblings ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", ["none", "value", "global"])
@pytest.mark.parametrize("name", list(KINDS))
def test_off_is_the_sibling_bit_for_bit(gpu, arena, name, mname):
    """l2_coeff = 0 and no transformer: gct2_adam_keras_clipped / gct2_optimizer_apply on the same inputs, bit for bit - also where p
    holds inf and -0 (0 * inf would be NaN, -0 + 0 would lose the sign: the add is skipped, not computed)"""
    kind, hyper = KINDS[name]
    mode = MODES[mname]
    p = arena.p.copy()
    inside = np.concatenate([np.arange(b, b + c) for b, c in arena.segs])
    rng = np.random.default_rng(3)
    for value in (np.inf, -np.inf, -0.0):
        p[rng.choice(inside, 40, replace=False)] = value
    g = arena.g.copy()
    g[p == 0] = 0.0                                              # (g' = +0 beside p = -0)
    base = Run(gpu, arena, kind, hyper, 1)
    host = dict(base.host, p=p, g=g)
    lo, n = arena.lo, arena.hi - arena.lo
    ss = torch.tensor([1234.5], dtype=torch.float64, device=gpu)
    clip, sumsq_ptr = {"none": (0.0, None), "value": (0.5, None), "global": (20.0, ss.data_ptr())}[mname]
    for ls in (None, ls_state(gpu, LS_SCALE, alpha=LS_LR)):
        A, B = Run(gpu, arena, kind, hyper, 1, host), Run(gpu, arena, kind, hyper, 1, host)
        a = A.args(lo, n, LR, GRAD_MUL, ls, mode, clip, sumsq_ptr)
        if kind == RC.ADAM:
            lib().call("gct2_adam_keras_clipped", *a[1:8], a[8], a[9], a[11], a[12], *a[13:], stream())
        else:
            lib().call("gct2_optimizer_apply", *a, stream())
        B.launch(lo, n, LR, 0.0, RC.GRAD_NONE, GRAD_MUL, ls, mode, clip, sumsq_ptr)
        torch.cuda.synchronize()
        for k in ("p", "m", "v", "g"):
            assert torch.equal(A.dev[k].view(torch.int32), B.dev[k].view(torch.int32)), (name, mname, k)
        assert torch.equal(A.sh.view(torch.int16), B.sh.view(torch.int16))
        assert not torch.equal(A.dev["p"].view(torch.int32), torch.from_numpy(p).to(gpu).view(torch.int32))      # (a step was made)


# ---- 3. gct2_grad_sumsq_l2 -----------------------------------------------------------------------------------------------------------
class Reduction:
    """a segment table of gct2_sumsq_layout on the device with the partials and sums of one reduction"""

    def __init__(self, gpu, segs):
        n = len(segs)
        begin, count = (ctypes.c_uint64 * n)(*[b for b, _ in segs]), (ctypes.c_uint64 * n)(*[c for _, c in segs])
        out, npart = (ctypes.c_uint64 * (3 * n))(), ctypes.c_size_t(0)
        lib().check(lib().load().gct2_sumsq_layout(begin, count, n, out, ctypes.byref(npart)), "gct2_sumsq_layout")
        self.segs, self.nseg, self.npart = segs, n, npart.value
        self.table = torch.tensor(list(out), dtype=torch.int64).to(gpu)
        self.partials = torch.zeros(self.npart, dtype=torch.float64, device=gpu)
        self.sumsq = torch.zeros(n + 1, dtype=torch.float64, device=gpu)

    def run_l2(self, g, p, coeffs, grad_mul=1.0, ls=None):
        self.coeffs = torch.tensor(coeffs, dtype=torch.float32, device=g.device)
        self.sumsq.fill_(-1.0)
        lib().call("gct2_grad_sumsq_l2", g.data_ptr(), p.data_ptr(), self.table.data_ptr(), self.coeffs.data_ptr(), self.nseg, self.npart,
                   float(grad_mul), None if ls is None else ls.data_ptr(), self.partials.data_ptr(), self.sumsq.data_ptr(), stream())
        torch.cuda.synchronize()
        return self.sumsq.cpu().numpy()

    def run(self, g, grad_mul=1.0, ls=None):
        self.sumsq.fill_(-1.0)
        lib().call("gct2_grad_sumsq", g.data_ptr(), self.table.data_ptr(), self.nseg, self.npart, float(grad_mul),
                   None if ls is None else ls.data_ptr(), self.partials.data_ptr(), self.sumsq.data_ptr(), stream())
        torch.cuda.synchronize()
        return self.sumsq.cpu().numpy()


@pytest.fixture(scope="module")
def exact(gpu):
    """g from clip_cases.exact_values, p the same kind of values, NaN in every gap and guard of BOTH"""
    segs, total = K.layout()
    rng = np.random.default_rng(6)
    g = K.poisoned(lambda s, n: K.exact_values(rng, n), segs, total)
    p = K.poisoned(lambda s, n: RC.exact_parameters(rng, n), segs, total)
    return types.SimpleNamespace(R=Reduction(gpu, segs), segs=segs, g=g, p=p, dg=torch.from_numpy(g).to(gpu), dp=torch.from_numpy(p).to(gpu))


def test_grad_sumsq_l2_equals_numpy_on_exact_inputs(gpu, exact):
    """l2 = 2^-3, so c = 2^-2: every x = g + p / 4 is a multiple of 2^-6, every square a multiple of 2^-12, and any summation order
    is exact in float64 below 2^53 units - per segment and in total, bit for bit.  The NaN gaps of g and p are never read"""
    units = RC.assert_exact_bound_l2(exact.segs)
    assert 2.0 ** 50 < units < 2.0 ** 53
    c = RC.coefficient(2.0 ** -3)
    assert c == 0.25
    coeffs = [c] * len(exact.segs)
    got = exact.R.run_l2(exact.dg, exact.dp, coeffs)
    want = RC.regularized_sumsq(exact.g, exact.p, exact.segs, coeffs)
    assert np.isfinite(want).all() and want[-1] > 0 and np.array_equal(got, want), (got, want)
    plain = K.segment_sumsq(exact.g, exact.segs)
    assert all(got[s] != plain[s] for s in range(len(exact.segs)))      # (the penalty gradient is in every sum)
    # with a loss-scale state: its inv_scale is a factor of g only (k = 1/2: x = g / 2 + p / 4 stays on the 2^-6 grid, below 1280)
    ls = ls_state(gpu, 2.0)
    got = exact.R.run_l2(exact.dg, exact.dp, coeffs, 1.0, ls)
    assert np.array_equal(got, RC.regularized_sumsq(exact.g, exact.p, exact.segs, coeffs, 1.0, 0.5)) and int(ls[3]) == 0
    assert not np.array_equal(got, want)


def test_grad_sumsq_l2_zero_coefficient_is_the_sibling_there(gpu, exact):
    c = np.float32(0.25)
    coeffs = [c if s % 3 else np.float32(0.0) for s in range(len(exact.segs))]        # segments 0, 3, 6, 9 carry no regularizer
    # where the coefficient is 0, p is not even read: poison those segments of p entirely
    p = exact.p.copy()
    for (b, n), cf in zip(exact.segs, coeffs):
        if cf == 0:
            p[b:b + n] = np.nan
    got = exact.R.run_l2(exact.dg, torch.from_numpy(p).to(gpu), coeffs)
    sibling = exact.R.run(exact.dg)
    want = RC.regularized_sumsq(exact.g, exact.p, exact.segs, coeffs)
    assert np.array_equal(got, want)
    for s, cf in enumerate(coeffs):
        assert (got[s] == sibling[s]) == (cf == 0), s
    assert np.array_equal(exact.R.run_l2(exact.dg, exact.dp, [0.0] * len(exact.segs)), sibling)      # all zero: the sibling's bits, total included


def test_grad_sumsq_l2_within_the_bound_of_any_summation_order(gpu, arena):
    """real values: count_s * 2^-53 relative against numpy's float64 sum, the bound tests/test_clip_gpu.py derives for gct2_grad_sumsq
    (non-negative float64 terms, any order); the total is the sequential float64 sum of the segment sums"""
    R = Reduction(gpu, arena.segs)
    coeffs = [C] * len(arena.segs)
    got = R.run_l2(torch.from_numpy(arena.g).to(gpu), torch.from_numpy(arena.p).to(gpu), coeffs, GRAD_MUL)
    want = RC.regularized_sumsq(arena.g, arena.p, arena.segs, coeffs, GRAD_MUL)
    for s, (_, n) in enumerate(arena.segs):
        assert abs(got[s] - want[s]) <= n * 2.0 ** -53 * want[s], (s, n, got[s], want[s])
    total = np.float64(0.0)
    for v in got[:-1]:
        total = total + v
    assert got[-1] == total


def test_grad_sumsq_l2_found_inf_comes_from_the_raw_gradient_alone(gpu, exact):
    coeffs = [np.float32(0.25)] * len(exact.segs)
    b, n = exact.segs[4]
    p = exact.p.copy()
    p[b + 1], p[b + 2] = np.inf, 3e38                              # a large and a non-finite parameter: the sums suffer, the flag does not
    ls = ls_state(gpu, 2.0 ** 7)
    got = exact.R.run_l2(exact.dg, torch.from_numpy(p).to(gpu), coeffs, 1.0, ls)
    assert int(ls[3]) == 0 and np.isinf(got[4]) and np.isfinite(np.delete(got[:-1], 4)).all()
    g = exact.g.copy()
    g[exact.segs[-1][0] + exact.segs[-1][1] - 1] = np.inf          # the last element of the last segment
    ls = ls_state(gpu, 2.0 ** 7)
    exact.R.run_l2(torch.from_numpy(g).to(gpu), exact.dp, coeffs, 1.0, ls)
    assert int(ls[3]) == 1
    # ... and without a state nothing is flagged anywhere
    watch = torch.zeros(8, dtype=torch.int32, device=gpu)
    exact.R.run_l2(torch.from_numpy(g).to(gpu), exact.dp, coeffs)
    assert int(watch.abs().sum()) == 0


# ---- 4. gct2_l2_penalty ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss, S, l2", [(0.5, 1e6, 1e-6), (1.0, 3.0, 2.0 ** -25), (0.0371, 48213.7711, 1e-6), (0.25, 123.0, 0.0),
                                         (7.25, 0.0, 0.01), (1e-3, 1e30, 1e-6)])
def test_l2_penalty(gpu, loss, S, l2):
    buf = torch.tensor([-7.0, loss, -7.0, -7.0, -7.0, -7.0], dtype=torch.float32, device=gpu)      # sentinels around the three scalars
    s = torch.tensor([S], dtype=torch.float64, device=gpu)
    lib().call("gct2_l2_penalty", buf.data_ptr() + 4, s.data_ptr(), float(l2), buf.data_ptr() + 12, buf.data_ptr() + 16, stream())
    torch.cuda.synchronize()
    pen, total = RC.penalty(np.float32(loss), np.float64(S), l2)
    want = np.array([-7.0, np.float32(loss), -7.0, pen, total, -7.0], dtype=np.float32)
    assert same(buf, want), (buf.cpu().numpy(), want)              # loss itself is untouched
    assert float(s[0]) == S


# ---- 5. train steps against the restatement ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    z = np.load(GOLDEN)
    params = {k[len("param/"):]: z[k] for k in z.files if k.startswith("param/")}
    return types.SimpleNamespace(params=params, x=z["x"], t_int=z["t_int"], eps=z["eps"])


def make_engine(gpu, dt, optimizer=None, params=None, **kw):
    """the tiny network; `optimizer` goes through Trainer.compile, as a user's would"""
    import gan_class_transfer2_amd as g
    eng = g.UNetEngine(g.Topology(*TOPO), dt, gpu, **{**dict(base_lr=1e-2, warm_up=0, seed=21, rng_seed=5), **kw})
    if params is not None:
        eng.set_params(params)
    if optimizer is not None:
        g.Trainer(types.SimpleNamespace(engine=eng)).compile(optimizer, g.identity)
    return eng


def arenas_of(eng):
    A = eng.arena
    torch.cuda.synchronize()
    return {n: getattr(A, n).clone() for n in ("p", "m", "v") + (("shadow",) if A.shadow is not None else ())}


def batches(gpu, n=4, seed=11):
    rng = np.random.default_rng(seed)
    return [torch.tensor(rng.uniform(-1, 1, (BATCH, SIZE, SIZE, 3)), dtype=torch.float32, device=gpu) for _ in range(n)]


def kind_of(eng):
    kind = {"adam": RC.ADAM, "sgd": RC.SGD, "rmsprop": RC.RMSPROP}[eng.optimizer_kind]
    hyper = dict(beta_1=eng.beta_1, beta_2=eng.beta_2) if kind == RC.ADAM else dict(momentum=eng.momentum, nesterov=eng.nesterov, rho=eng.rho)
    return kind, dict(hyper, epsilon=eng.epsilon)


def expected_arenas(eng, old, grads, segs, l2_segs, lr, inv_scale=1.0):
    """numpy's p / m / v after the engine's regularized step: the restatement per tensor with the tensor's own coefficient (the
    padding between tensors keeps what it held, except where ONE launch covers it: there g, p, m, v are zero and stay zero for
    every kind, so the two agree).  The sums of squares of a norm mode are the ones the launches read on the device, each checked
    against numpy's within the summation-order bound"""
    kind, hyper = kind_of(eng)
    c = RC.coefficient(eng.l2) if eng.l2 > 0 else np.float32(0.0)
    coeffs = [c if seg in l2_segs else np.float32(0.0) for seg in segs]
    transform = RC.GRAD_SIGN if eng.grad_transform == "sign" else RC.GRAD_NONE
    ss = None
    if eng.clip_mode in (K.CLIP_NORM, K.CLIP_GLOBAL_NORM):
        ss = eng._clip_reduction()[4].cpu().numpy()
        want = RC.regularized_sumsq(grads, old["p"], segs, coeffs, 1.0, inv_scale)
        for s, (_, n) in enumerate(segs):
            assert abs(ss[s] - want[s]) <= n * 2.0 ** -53 * want[s], (s, ss[s], want[s])
        total = np.float64(0.0)
        for v in ss[:-1]:
            total = total + v
        assert ss[-1] == total
    out = {k: old[k].copy() for k in ("p", "m", "v")}
    for s, ((b, n), cf) in enumerate(zip(segs, coeffs)):
        sl = slice(b, b + n)
        one = None if ss is None else (ss[s] if eng.clip_mode == K.CLIP_NORM else ss[-1])
        p, m, v = RC.apply(kind, old["p"][sl], old["m"][sl], old["v"][sl], grads[sl], lr, hyper, cf, transform, eng.clip_mode, eng.clip, one,
                           1.0, inv_scale)
        out["p"][sl] = p
        if m is not None and (kind == RC.ADAM or hyper.get("momentum", 0) > 0):
            out["m"][sl] = m
        if kind != RC.SGD:
            out["v"][sl] = v
    return out


def check_step(eng, before, loss, lr, dt, inv_scale=1.0, data_loss=None):
    """one applied regularized step of a UNetEngine against numpy, on the gradients its optimizer launches read (the engine's own
    arena: at this topology the Dense gradient is summed with float atomics, so a twin engine's would reproduce them only up to the
    order of those additions - tests/test_optimizers_gpu.py own_gradients) and the arenas as they stood before the step"""
    assert eng._grads_in_arena                                   # the non-fused path
    torch.cuda.synchronize()
    grads = eng.arena.g.cpu().numpy()
    assert np.isfinite(grads).all() and float(np.abs(grads).max()) > 0
    old = {n: t.cpu().numpy() for n, t in before.items() if n != "shadow"}
    segs = [(int(b), int(n)) for b, n in eng._clip_segments()]
    pad = np.ones(eng.arena.total, dtype=bool)
    for b, n in segs:
        pad[b:b + n] = False
    assert not grads[pad].any() and not old["p"][pad].any() and not old["m"][pad].any() and not old["v"][pad].any()
    want = expected_arenas(eng, old, grads, segs, set(segs), lr, inv_scale)
    after = arenas_of(eng)
    assert same(after["p"], want["p"]) and same(after["m"], want["m"]) and same(after["v"], want["v"])
    assert not torch.equal(after["p"], before["p"])
    if dt:
        assert torch.equal(after["shadow"].view(torch.int16), cast(dt, after["p"]).view(torch.int16))
    check_reported_loss(eng, old["p"], segs, loss, data_loss)
    return grads, after


def check_reported_loss(eng, p_before, l2_segs, loss, data_loss):
    """the step returned data loss + penalty as gct2_l2_penalty defines them on S, the float64 sum of squares of the regularized
    tensors BEFORE the update (read from the device, checked against numpy's within the summation-order bound)"""
    if not eng.l2 > 0:
        assert eng.regularization_loss is None and data_loss is None
        return
    (_, nseg, _, _, sumsq, _), pen_t, total_t = eng._l2_state
    S = sumsq.cpu().numpy()
    want = K.segment_sumsq(p_before, l2_segs)
    assert nseg == len(l2_segs)
    for s, (_, n) in enumerate(l2_segs):
        assert abs(S[s] - want[s]) <= n * 2.0 ** -53 * want[s], (s, S[s], want[s])
    pen, total = RC.penalty(data_loss.cpu().numpy()[0], S[-1], eng.l2)
    assert same(eng.regularization_loss, [pen]) and same(loss, [total]) and loss.data_ptr() == total_t.data_ptr()
    assert pen > 0 and float(total) >= float(data_loss[0])


def data_loss_of(eng):
    """where the data term of the last step is: the loss scalar of the engine's buffer set (the regularized step leaves it there)"""
    return eng.buffers(BATCH, SIZE, SIZE).loss


STEP_CASES = {
    "adam_l2": (lambda g: g.Adam(g.WarmUp(1e-2, 3)), 1e-3),
    "rmsprop_l2_sign": (lambda g: g.RMSprop(1e-3, momentum=0.9, gradient_transformers=[g.sign_gradient]), 1e-3),
    "adam_l2_clipvalue": (lambda g: g.Adam(1e-2, clipvalue=1e-3), 1e-3),
    "adam_l2_global_clipnorm": (lambda g: g.Adam(1e-2, global_clipnorm=1e-2), 1e-3),
    "adam_l2_clipnorm": (lambda g: g.Adam(1e-2, clipnorm=1e-3), 1e-3),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_regularized_steps_equal_numpy(gpu, tiny, recorded, case):
    """E steps eagerly, P - its arenas overwritten with E's before each step - under step plans (recorded at the second step, replayed
    from the third); after two steps the factor changes, so another plan key is exercised.  Every step of both is the restatement's
    bits; where P's gradients equal E's bit for bit, so do its arenas"""
    import gan_class_transfer2_amd as g
    make, l2 = STEP_CASES[case]
    E, P = make_engine(gpu, 1, make(g), tiny.params), make_engine(gpu, 1, make(g), tiny.params)
    E.use_plan, P.use_plan = False, True
    xs = batches(gpu, 5)
    keys = {False: set(), True: set()}                           # the plan keys seen before / after the factor changes
    for k in range(5):
        factor = l2 if k < 3 else 4 * l2
        for e in (E, P):
            e.set_regularizer(factor)
        before = arenas_of(E)
        for n, t in before.items():
            getattr(P.arena, n).copy_(t)
        lr = E.step_size()
        assert lr == P.step_size()
        b, cur = P.buffers(BATCH, SIZE, SIZE), torch.cuda.current_stream(P.device)
        keys[k >= 3].add(P._plan_key(b, True, False, cur))
        le, lp = E.train_step(xs[k]), P.train_step(xs[k])
        de = data_loss_of(E).clone()
        ge, ae = check_step(E, before, le, lr, 1, data_loss=de)
        gp, ap = check_step(P, before, lp, lr, 1, data_loss=data_loss_of(P).clone())
        assert float(le[0]) == float(lp[0]), k                       # (the forward pass has no atomics: the same loss)
        if np.array_equal(bits(ge), bits(gp)):
            for n in ae:
                assert torch.equal(ae[n], ap[n]), (k, n)
    assert E.iterations == P.iterations == 5 and not E._plans
    assert set(P.state_dict()) - {"optimizer"} == {"arena.p", "arena.m", "arena.v", "counters", "topology"}      # settings, not state
    assert keys[False] and keys[True] and not keys[False] & keys[True] and len(P._plans) >= 2      # the factor is part of the key
    nseg = len(E._clip_segments())
    for sp in P._plans.values():
        names = recorded(sp.plan)
        norm = case in ("adam_l2_global_clipnorm", "adam_l2_clipnorm")
        assert names.count("gct2_optimizer_apply_reg") == (nseg if case == "adam_l2_clipnorm" else 1)      # every tensor alike: ONE launch
        assert names.count("gct2_grad_sumsq_l2") == int(norm) and names.count("gct2_l2_penalty") == 1
        assert names.count("gct2_grad_sumsq") == 1                   # the penalty's reduction, at the head of the step
        assert not any(n in names for n in ("gct2_adam_keras_multi", "gct2_adam_keras_clipped", "gct2_optimizer_apply", "gct2_adam_apply"))
        assert names.index("gct2_grad_sumsq") < names.index("gct2_l2_penalty") < names.index("gct2_optimizer_apply_reg")


@pytest.fixture
def tiny_model():
    """the module-level hyper-parameters of the tiny bf16 network, put back afterwards"""
    import gan_class_transfer2_amd as g
    names = ("size", "pixel_size", "max_size", "octaves", "compute_dtype", "mixed_precision", "block_depth", "residual", "concat", "warm_up",
             "regularizer")
    keep = {n: getattr(g.model, n) for n in names}
    g.configure(size=SIZE, pixel_size=TOPO[0], max_size=TOPO[1], octaves=TOPO[2], compute_dtype="bfloat16", mixed_precision=False, block_depth=0,
                residual=False, concat=True, regularizer=None)
    yield g
    g.configure(**keep)


def test_the_reference_lines_through_the_public_interface(gpu, tiny_model):
    """train.py:71-74 and train.py:80 as written: SGD(0.0001, gradient_transformers=[sign_gradient]) through Trainer.compile /
    train_step - every parameter with a non-zero gradient moves by exactly fl(lr) - then regularizer = l2(1e-6) on top"""
    g = tiny_model
    tr = g.Trainer(g.Denoiser(seed=3, device=gpu))
    opt = g.SGD(0.0001, gradient_transformers=[g.sign_gradient])
    tr.compile(opt, g.identity)
    xs = batches(gpu, 3, seed=2)
    out = tr.train_step((xs[0], xs[0]))
    eng = tr.denoiser.engine
    assert (eng.optimizer_kind, eng.grad_transform, eng.l2, eng.regularization_loss) == ("sgd", "sign", 0.0, None) and eng.use_plan
    before = arenas_of(eng)
    out = tr.train_step((xs[1], xs[1]))
    grads, after = check_step(eng, before, out["loss"], eng.learning_rate(1), 1)
    step = (after["p"].double() - before["p"].double()).cpu().numpy()
    assert (grads != 0).sum() > 1000 and np.allclose(step[grads != 0], -1e-4 * np.sign(grads[grads != 0]), rtol=2e-3, atol=0)
    assert not step[grads == 0].any() and torch.equal(after["m"], before["m"]) and torch.equal(after["v"], before["v"])
    assert out["loss"].data_ptr() == data_loss_of(eng).data_ptr()  # no regularizer: the loss is the data term's own tensor
    g.configure(regularizer=g.regularizers.l2(1e-6))
    before = arenas_of(eng)
    out = tr.train_step((xs[2], xs[2]))
    assert eng.l2 == float(np.float32(1e-6)) and opt.iterations == 3
    check_step(eng, before, out["loss"], eng.learning_rate(2), 1, data_loss=data_loss_of(eng).clone())
    # Trainer.call (no gradients) keeps returning the data term, as calling the Keras model does
    torch.cuda.synchronize()
    pen = float(eng.regularization_loss[0])
    assert pen > 0 and tr(xs[2]).shape == () and float(eng.regularization_loss[0]) == pen
    g.configure(regularizer=None)
    out = tr.train_step((xs[2], xs[2]))
    assert eng.l2 == 0.0 and eng.regularization_loss is None and out["loss"].data_ptr() == data_loss_of(eng).data_ptr()


def test_fp16_loss_scaled_regularized_step_and_a_skipped_one(gpu, tiny):
    """LossScaleOptimizer(Adam) + l2 in fp16: an applied step against numpy at the step size read back from the device state, with the
    penalty gradient added to the UNSCALED gradient; then a step whose gradient arena holds one written inf: skipped - p, m, v, the
    shadow and iterations unchanged, the scale halved"""
    import gan_class_transfer2_amd as g
    A = make_engine(gpu, 2, g.LossScaleOptimizer(g.Adam(g.WarmUp(1e-2, 3))), tiny.params)
    A.set_regularizer(1e-3)
    A.use_plan = False
    assert A.ls_state is not None and A.loss_scale() == (2.0 ** 15, 0)
    X = torch.tensor(tiny.x, dtype=torch.float32, device=gpu)
    before = arenas_of(A)
    loss = A.train_step(X)
    torch.cuda.synchronize()
    alpha = float(A.ls_state.view(torch.float32)[5].item())
    assert alpha > 0 and A.iterations == 1 and A.loss_scale() == (2.0 ** 15, 1)
    _, st1 = check_step(A, before, loss, alpha, 2, inv_scale=2.0 ** -15, data_loss=data_loss_of(A).clone())
    A.train_step(X, apply=False)
    A.arena.g[5] = float("inf")
    A.check_finite(); A.apply_adam(); A.finish_step()
    torch.cuda.synchronize()
    st2 = arenas_of(A)
    assert all(torch.equal(st2[n], st1[n]) for n in st1)
    assert A.iterations == 1 and A.loss_scale() == (2.0 ** 14, 0)


# ---- 6. the variant engine: Residual's projection carries no regularizer ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "global"])
def test_variant_engine_leaves_the_projection_unregularized(gpu, mode):
    """residual=True at the smallest widths: one Adam + l2 step against numpy on the engine's own gradients.  The projection tensors'
    updates are the unregularized formula's, every other tensor's the regularized one's - and the two differ on every tensor, so a
    build that regularizes everything, or nothing, fails"""
    from gan_class_transfer2_amd.variants import VariantEngine
    rng = np.random.default_rng(9)
    eng = VariantEngine(8, 16, 2, 0, True, True, 1, gpu, base_lr=1e-3, warm_up=0, seed=4)
    eng.set_regularizer(0.05)
    if mode == "global":
        eng.set_clipping(global_clipnorm=1e-2)
    N = eng.net
    segs = [(int(b), int(n)) for b, n in eng._clip_segments()]
    l2_segs = [(int(b), int(n)) for b, n in eng._l2_segments()]
    proj = [(N.offsets[name], int(np.prod(shp))) for name, shp in N.specs if name.endswith(".dense.w")]
    assert len(proj) == 2 and set(segs) - set(l2_segs) == set(proj) and (N.offsets["dense.w"], N.shapes["dense.w"][0] * 3) in l2_segs
    x = torch.tensor(rng.uniform(-1, 1, (2, 16, 16, 3)), dtype=torch.float32, device=gpu)
    torch.cuda.synchronize()
    old = {k: t.cpu().numpy() for k, t in (("p", N.p), ("m", N.m), ("v", N.v))}
    lr = eng.step_size()
    loss = eng.train_step(x)
    torch.cuda.synchronize()
    assert eng.iterations == 1
    grads = N.g.cpu().numpy()
    assert np.isfinite(grads).all() and float(np.abs(grads).max()) > 0
    want = expected_arenas(eng, old, grads, segs, set(l2_segs), lr)
    assert same(N.p, want["p"]) and same(N.m, want["m"]) and same(N.v, want["v"])
    assert torch.equal(N.op.view(torch.int16), cast(1, N.p).view(torch.int16))
    if mode == "none":                                           # (the global norm's sums would be others, too)
        everything, nothing = expected_arenas(eng, old, grads, segs, set(segs), lr), expected_arenas(eng, old, grads, segs, set(), lr)
        got = N.m.cpu().numpy()
        for b, n in proj:                                        # regularizing the projection would have given other bits
            assert not np.array_equal(bits(everything["m"][b:b + n]), bits(got[b:b + n])), (b, n)
        kernels = [(b, n) for b, n in l2_segs if old["p"][b:b + n].any()]      # (the biases start at zero: no penalty gradient yet)
        assert len(kernels) >= 5
        for b, n in kernels:                                     # ... and so would regularizing nothing, on every other kernel
            assert not np.array_equal(bits(nothing["m"][b:b + n]), bits(got[b:b + n])), (b, n)
    check_reported_loss(eng, old["p"], l2_segs, loss, eng.loss.clone())
    # Trainer.call's form (no reverse pass) reports the data term and leaves the penalty alone
    pen = float(eng.regularization_loss[0])
    assert eng.train_step(x, backward=False).data_ptr() == eng.loss.data_ptr() and float(eng.regularization_loss[0]) == pen


# ---- 7. off means off ------------------------------------------------------------------------------------------------------------------
WIDE, WIDE_SIZE, WIDE_BATCH = (128, 256, 3), 32, 4    # reference widths: the matrix-core head, so no kernel of the step adds with atomics


def three_steps(gpu, recorded, optimizer, touch):
    """a fresh engine at the reference widths, three planned steps on fixed batches: (engine, arenas after each step, losses, the
    entry-point names of its plans).  touch: both setters are used first, and switched off again"""
    import gan_class_transfer2_amd as g
    eng = g.UNetEngine(g.Topology(*WIDE), 1, gpu, base_lr=1e-2, warm_up=0, seed=21, rng_seed=5)
    g.Trainer(types.SimpleNamespace(engine=eng)).compile(optimizer(g), g.identity)
    if touch:
        eng.set_regularizer(1e-3); eng.set_gradient_transform("sign")
        eng.set_regularizer(None); eng.set_gradient_transform("none")
    rng = np.random.default_rng(11)
    states, losses = [], []
    for _ in range(3):
        x = torch.tensor(rng.uniform(-1, 1, (WIDE_BATCH, WIDE_SIZE, WIDE_SIZE, 3)), dtype=torch.float32, device=gpu)
        losses.append(float(eng.train_step(x)[0]))
        states.append(arenas_of(eng))                            # (reading the arenas flushes what the step held back)
    assert len(eng._plans) >= 1
    return eng, states, losses, [recorded(sp.plan) for sp in eng._plans.values()]


@pytest.mark.parametrize("line", ["default", "sgd"])
def test_off_means_off(gpu, recorded, line):
    """with both settings off the recorded entry points of a step are what they were: none of the three new names, the fused Adam step /
    one gct2_optimizer_apply as before; nothing new is allocated; and three steps are bit-identical to the same steps of an engine on
    which both setters were used and switched off again"""
    optimizer = {"default": lambda g: g.Adam(g.WarmUp(1e-2, 3)), "sgd": lambda g: g.SGD(0.25, 0.5, True)}[line]
    a, sa, la, na = three_steps(gpu, recorded, optimizer, touch=False)
    b, sb, lb, nb = three_steps(gpu, recorded, optimizer, touch=True)
    assert na == nb and la == lb
    stage = ("gct2_adam_", "gct2_optimizer_", "gct2_grad_sumsq", "gct2_loss_scale", "gct2_scale_check", "gct2_ema", "gct2_l2")
    for names in na:
        # recorded on the parent commit with this very sequence of calls: 21 entry points per plan, one optimizer-stage call among them
        # (the default step's other updates ride behind the weight gradients, inside their calls)
        assert not any(n in names for n in NEW), names
        assert len(names) == 21 and [n for n in names if n.startswith(stage)] == [{"default": "gct2_adam_keras_multi", "sgd": "gct2_optimizer_apply"}[line]], names
    assert a._grads_in_arena == b._grads_in_arena == (line != "default")
    for e in (a, b):
        assert e._l2_state is None and e._reg_tables is None and e._clip_table is None and e.regularization_loss is None
    assert not {"l2", "grad_transform", "_l2_state", "_reg_tables"} & set(vars(a))     # never used: nothing new is carried
    for k, (x, y) in enumerate(zip(sa, sb)):
        for n in x:
            assert torch.equal(x[n].view(torch.int32) if x[n].dtype == torch.float32 else x[n].view(torch.int16),
                               y[n].view(torch.int32) if y[n].dtype == torch.float32 else y[n].view(torch.int16)), (k, n)


# ---- 8. what is refused ----------------------------------------------------------------------------------------------------------------
def test_refusals(gpu, tiny, tiny_model):
    g = tiny_model
    from gan_class_transfer2_amd.distributed import DataParallelStep, ShardedDataParallelStep
    for Wrapper in (DataParallelStep, ShardedDataParallelStep):
        for setting in (lambda e: e.set_regularizer(1e-6), lambda e: e.set_gradient_transform("sign")):
            fresh = make_engine(gpu, 1)
            setting(fresh)
            hooks = (fresh.grad_ready_hook, fresh.post_backward)
            with pytest.raises(ValueError, match=Wrapper.__name__):
                Wrapper(fresh)
            assert (fresh.grad_ready_hook, fresh.post_backward) == hooks                  # refused before it touched the engine
            assert not any(hasattr(fresh, n) for n in ("_optimizer_forbidden", "_clip_forbidden", "_reg_forbidden"))
        plain = make_engine(gpu, 1)
        Wrapper(plain)
        for setting in (lambda e: e.set_regularizer(1e-6), lambda e: e.set_gradient_transform("sign")):
            with pytest.raises(ValueError, match=Wrapper.__name__):
                setting(plain)
        plain.set_regularizer(None); plain.set_gradient_transform("none")
        assert not plain._regularized()
    # a sub-range update in a norm mode: the norm needs the whole arena
    eng = make_engine(gpu, 1, g.Adam(1e-2, global_clipnorm=1.0), tiny.params)
    eng.set_regularizer(1e-3)
    eng.train_step(torch.tensor(tiny.x, dtype=torch.float32, device=gpu), apply=False)
    before = arenas_of(eng)
    with pytest.raises(ValueError, match="clipnorm / global_clipnorm"):
        eng.apply_adam(0, 64)
    assert all(torch.equal(t, before[n]) for n, t in arenas_of(eng).items())
    # an unknown transformer, a regularizer that is not l2
    with pytest.raises(NotImplementedError, match="gradient_transformers"):
        g.SGD(0.0001, gradient_transformers=[lambda pairs: pairs])
    with pytest.raises(ValueError, match="unknown gradient transform"):
        eng.set_gradient_transform("abs")
    tr = g.Trainer(g.Denoiser(seed=3, device=gpu))
    tr.compile(g.Adam(1e-3), g.identity)
    g.configure(regularizer=lambda w: 1e-6 * (w * w).sum())
    with pytest.raises(NotImplementedError, match="regularizer"):
        tr.train_step((batches(gpu, 1)[0],) * 2)
    assert tr.denoiser.engine is None                            # refused before anything was built
