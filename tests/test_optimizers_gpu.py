"""Keras SGD / RMSprop and the InverseTimeDecay schedule [TF] on the GPU: gct2_optimizer_apply per element and bit for bit (every
kind, every shadow type, plain / loss-scaled / skipped, one launch over the arena and one per sub-range, clipped), the device-side
schedule of gct2_loss_scale_begin_schedule, train steps of both engines against numpy - eager and planned, with loss scaling, Adam
under the new schedule - the public interface, checkpoints, the untouched default step, and what is refused.

The reference of every comparison is the arithmetic of include/gct2.h restated in tests/optimizer_cases.py (and tests/clip_cases.py
for the gradient's scaling and clipping); every comparison is bit for bit, nothing is measured.  Buffers carry NaN in every gap and
guard of what a kernel reads, sentinels around every range it may write, and NaN poison in the slots a kind must not touch.
PARITY UNPINNED w.r.t. TensorFlow (there is none here)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import clip_cases as K
import optimizer_cases as OC

pytestmark = pytest.mark.gpu
TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
NEW = ("gct2_optimizer_apply", "gct2_loss_scale_begin_schedule")
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
    """float32 device tensor == numpy array: NaN where NaN, the same bits (so also the sign of zero) everywhere else"""
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


# ---- 1. gct2_optimizer_apply, per element and bit for bit ---------------------------------------------------------------------------
KINDS = {"sgd": (OC.SGD, {}), "sgd_momentum": (OC.SGD, dict(momentum=0.5)), "sgd_nesterov": (OC.SGD, dict(momentum=0.5, nesterov=True)),
         "rmsprop": (OC.RMSPROP, dict(rho=0.9, epsilon=1e-7)), "rmsprop_momentum": (OC.RMSPROP, dict(rho=0.9, momentum=0.9, epsilon=1e-7))}
LR, LS_LR, LS_SCALE = 1.5e-3, 2.5e-3, 2.0 ** 7
P_FILL, M_FILL, V_FILL, SH_FILL = 12345.0, -12345.0, 24690.0, 77.0
POISON = {"m": 0x7FC00A0A, "v": 0x7FC00B0B}          # quiet NaNs with a payload of their own: an untouched slot keeps these very bits


@pytest.fixture(scope="module")
def arena(gpu):
    """clip_cases.layout(): ten segments of 1 .. 3 CHUNK + 7 elements at 64-element alignment between two guards.  g: NaN in every gap
    and in both guards; p, m, v: values over the whole range a launch may cover (the gaps included), sentinels in the guards."""
    segs, total = K.layout()
    assert [c for _, c in segs] == list(K.SEGMENT_LENGTHS) and all(b % 64 == 0 for b, _ in segs)
    lo, hi = K.GUARD, total - K.GUARD
    assert segs[0][0] == lo and segs[-1][0] + segs[-1][1] <= hi
    rng = np.random.default_rng(77)
    g = K.poisoned(lambda s, n: rng.standard_normal(n).astype(np.float32), segs, total)
    inner = lambda fill, vals: np.concatenate([np.full(lo, fill, np.float32), vals.astype(np.float32), np.full(total - hi, fill, np.float32)])
    p = inner(P_FILL, rng.standard_normal(hi - lo))
    m = inner(M_FILL, rng.standard_normal(hi - lo) * 1e-2)
    v = inner(V_FILL, rng.random(hi - lo) * 1e-4)
    return types.SimpleNamespace(segs=segs, total=total, lo=lo, hi=hi, g=g, p=p, m=m, v=v)


class Run:
    """device copies of the arena for one case: the slots the kind does not use hold NaN poison instead of values"""

    def __init__(self, gpu, A, kind, hyper, dt):
        self.A, self.kind, self.hyper, self.dt = A, kind, hyper, dt
        self.use_m, self.use_v = hyper.get("momentum", 0.0) > 0, kind == OC.RMSPROP
        host = dict(p=A.p, g=A.g, m=A.m if self.use_m else np.full(A.total, POISON["m"], np.int32).view(np.float32),
                    v=A.v if self.use_v else np.full(A.total, POISON["v"], np.int32).view(np.float32))
        self.host = host
        self.dev = {k: torch.from_numpy(a.copy()).to(gpu) for k, a in host.items()}
        self.sh = torch.full((A.total,), SH_FILL, dtype=TDT[dt], device=gpu) if dt else None
        self.sh0 = self.sh.clone() if dt else None

    def launch(self, lo, n, lr, grad_mul=1.0, ls=None, mode=K.CLIP_NONE, clip=0.0, sumsq_ptr=None, pass_unused=True):
        d = self.dev
        ptr = lambda k, used: d[k].data_ptr() + 4 * lo if (used or pass_unused) else None
        lib().call("gct2_optimizer_apply", self.kind, ptr("p", True), ptr("m", self.use_m), ptr("v", self.use_v), ptr("g", True),
                   self.sh.data_ptr() + 2 * lo if self.dt else None, self.dt, n, float(lr), float(self.hyper.get("momentum", 0.0)),
                   int(self.hyper.get("nesterov", False)), float(self.hyper.get("rho", 0.9)), float(self.hyper.get("epsilon", 1e-7)),
                   float(grad_mul), None if ls is None else ls.data_ptr(), mode, float(clip), sumsq_ptr, stream())

    def expect(self, ranges, lr, grad_mul=1.0, inv_scale=1.0, mode=K.CLIP_NONE, clip=0.0, ss=None):
        """the arenas after launches over `ranges` ((lo, n) pairs; ss: one float64 per range): numpy over exactly those elements"""
        out = {k: self.host[k].copy() for k in ("p", "m", "v")}
        for r, (lo, n) in enumerate(ranges):
            sl = slice(lo, lo + n)
            p, m, v = OC.apply(self.kind, out["p"][sl], out["m"][sl], out["v"][sl], self.host["g"][sl], lr, self.hyper, mode, clip,
                               None if ss is None else ss[r], grad_mul, inv_scale)
            out["p"][sl], out["m"][sl], out["v"][sl] = p, m, v
        return out

    def check(self, want, ranges, tag):
        torch.cuda.synchronize()
        d = self.dev
        assert np.array_equal(bits(d["g"]), bits(self.host["g"])), tag                  # g is read only (never zeroed)
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


def sub_ranges(segs):
    """one launch per segment over an odd-offset sub-range: from its second 16-byte group on (pointers stay 16-byte aligned), the
    whole segment where it has no second group"""
    return [(b + 4, c - 4) if c > 4 else (b, c) for b, c in segs]


@pytest.mark.parametrize("dt", [0, 1, 2], ids=["noshadow", "bf16", "f16"])
@pytest.mark.parametrize("name", list(KINDS))
def test_optimizer_apply_per_element(gpu, arena, name, dt):
    kind, hyper = KINDS[name]
    whole = [(arena.lo, arena.hi - arena.lo)]
    for shape, ranges in (("whole", whole), ("per_segment", sub_ranges(arena.segs))):
        # plain: the host's lr, grad_mul = 0.5
        R = Run(gpu, arena, kind, hyper, dt)
        for lo, n in ranges:
            R.launch(lo, n, LR, grad_mul=0.5, pass_unused=(shape == "whole"))        # (unused slots: garbage pointers or NULL, never read)
        want = R.expect(ranges, LR, grad_mul=0.5)
        R.check(want, ranges, (name, dt, shape, "plain"))
        assert not np.array_equal(bits(want["p"]), bits(arena.p))                   # (the step moved something)
        # with a loss-scale state: its inv_scale times grad_mul as ONE factor, ITS alpha (the lr argument is ignored)
        R = Run(gpu, arena, kind, hyper, dt)
        ls = ls_state(gpu, LS_SCALE, alpha=LS_LR)
        for lo, n in ranges:
            R.launch(lo, n, 123.0, grad_mul=0.5, ls=ls)
        R.check(R.expect(ranges, LS_LR, grad_mul=0.5, inv_scale=1.0 / LS_SCALE), ranges, (name, dt, shape, "loss_scaled"))
        assert int(ls[3]) == 0
        # found_inf = 1: nothing at all is written
        R = Run(gpu, arena, kind, hyper, dt)
        ls = ls_state(gpu, LS_SCALE, found_inf=1, alpha=LS_LR)
        for lo, n in ranges:
            R.launch(lo, n, LR, ls=ls)
        R.check(R.expect([], LR), [], (name, dt, shape, "found_inf"))
        assert int(ls[3]) == 1


class Reduction:
    """gct2_grad_sumsq over the arena's segments: the device table and the sums the clipped launches read"""

    def __init__(self, gpu, segs):
        n = len(segs)
        begin, count = (ctypes.c_uint64 * n)(*[b for b, _ in segs]), (ctypes.c_uint64 * n)(*[c for _, c in segs])
        out, npart = (ctypes.c_uint64 * (3 * n))(), ctypes.c_size_t(0)
        lib().check(lib().load().gct2_sumsq_layout(begin, count, n, out, ctypes.byref(npart)), "gct2_sumsq_layout")
        self.nseg, self.npart = n, npart.value
        self.table = torch.tensor(list(out), dtype=torch.int64).to(gpu)
        self.partials = torch.zeros(self.npart, dtype=torch.float64, device=gpu)
        self.sumsq = torch.zeros(n + 1, dtype=torch.float64, device=gpu)

    def run(self, g, grad_mul=1.0):
        lib().call("gct2_grad_sumsq", g.data_ptr(), self.table.data_ptr(), self.nseg, self.npart, float(grad_mul), None,
                   self.partials.data_ptr(), self.sumsq.data_ptr(), stream())
        torch.cuda.synchronize()
        return self.sumsq.cpu().numpy()


@pytest.mark.parametrize("name", ["sgd_nesterov", "rmsprop"])
@pytest.mark.parametrize("mode", [K.CLIP_VALUE, K.CLIP_GLOBAL_NORM], ids=["clipvalue", "global_clipnorm"])
def test_optimizer_apply_clips(gpu, arena, mode, name):
    """the clipping step of gct2_adam_keras_clipped in front of the update: clipvalue at a threshold inside the gradients' range, the
    global norm at half the gradients' norm - its sum of squares comes from gct2_grad_sumsq on the same arena"""
    kind, hyper = KINDS[name]
    R = Run(gpu, arena, kind, hyper, 1)
    whole = [(arena.lo, arena.hi - arena.lo)]
    if mode == K.CLIP_VALUE:
        clip, ss, ptr = 0.5, None, None
        inside = np.concatenate([arena.g[b:b + c] for b, c in arena.segs])
        assert (np.abs(inside) > clip).any() and (np.abs(inside) < clip).any()
    else:
        red = Reduction(gpu, arena.segs)
        sums = red.run(R.dev["g"], grad_mul=0.5)
        want_sums = K.segment_sumsq(K.scaled(arena.g, 0.5), arena.segs)
        count = sum(c for _, c in arena.segs)
        assert abs(sums[-1] - want_sums[-1]) <= count * 2.0 ** -53 * want_sums[-1]      # (any summation order of non-negative terms)
        clip = 0.5 * float(np.sqrt(sums[-1]))                       # half the norm: the scale is about 0.5
        ss, ptr = [sums[-1]], red.sumsq.data_ptr() + 8 * red.nseg
    R.launch(*whole[0], LR, grad_mul=0.5, mode=mode, clip=clip, sumsq_ptr=ptr)
    want = R.expect(whole, LR, grad_mul=0.5, mode=mode, clip=clip, ss=ss)
    R.check(want, whole, (name, mode))
    plain = R.expect(whole, LR, grad_mul=0.5)
    assert not np.array_equal(bits(want["p"]), bits(plain["p"]))                        # the clipping is visible in the result


# ---- 2. the device-side schedule ------------------------------------------------------------------------------------------------------
def begin_schedule(st, schedule, initial, steps, decay_rate=0.0, staircase=False, bias_correction=False, beta1=0.9, beta2=0.999):
    lib().call("gct2_loss_scale_begin_schedule", st.data_ptr(), schedule, float(initial), float(steps), float(decay_rate), int(staircase),
               int(bias_correction), float(beta1), float(beta2), stream())
    torch.cuda.synchronize()
    return st.cpu()


def untouched(raw, k):
    """every field but found_inf and alpha as ls_state(scale 2^9, good_steps 7, applied_steps k) left it"""
    f = raw.view(torch.float32)
    return (float(f[0]), float(f[1]), int(raw[2]), int(raw[4]), int(raw[6]), int(raw[7])) == (2.0 ** 9, 2.0 ** -9, 7, k, 0, 0)


@pytest.mark.parametrize("staircase", [False, True], ids=["plain", "staircase"])
@pytest.mark.parametrize("initial, decay_steps, decay_rate", OC.REFERENCE_SCHEDULES)
def test_device_inverse_time_decay(gpu, initial, decay_steps, decay_rate, staircase):
    from gan_class_transfer2_amd import trainer_math as TM
    for k in OC.SCHEDULE_STEPS:
        st = ls_state(gpu, 2.0 ** 9, found_inf=1, alpha=-1.0, applied_steps=k, good_steps=7)
        raw = begin_schedule(st, OC.INVERSE_TIME_DECAY, initial, decay_steps, decay_rate, staircase)
        want = OC.inverse_time_decay(k, initial, decay_steps, decay_rate, staircase)
        assert raw.view(torch.float32)[5].numpy().tobytes() == want.tobytes(), (k, float(raw.view(torch.float32)[5]), want)
        assert float(want) == TM.inverse_time_decay_lr(k, initial, decay_steps, decay_rate, staircase)      # ... which is the host's value
        assert int(raw[3]) == 0 and untouched(raw, k), k


def test_device_warmup_and_the_bias_correction(gpu):
    from gan_class_transfer2_amd import trainer_math as TM
    base, warm = 2e-5, 10_000
    for k in OC.SCHEDULE_STEPS:
        st = ls_state(gpu, 2.0 ** 9, found_inf=1, alpha=-1.0, applied_steps=k, good_steps=7)
        raw = begin_schedule(st, OC.WARMUP, base, warm)
        want = np.float32(TM.warmup_lr(k, base, warm))
        assert raw.view(torch.float32)[5].numpy().tobytes() == want.tobytes(), (k, want)
        assert int(raw[3]) == 0 and untouched(raw, k), k
        # with the bias correction the entry point is gct2_loss_scale_begin: WarmUp as it is, InverseTimeDecay as a constant of its value
        old = ls_state(gpu, 2.0 ** 9, found_inf=1, applied_steps=k, good_steps=7)
        lib().call("gct2_loss_scale_begin", old.data_ptr(), base, warm, 0.9, 0.999, stream())
        new = begin_schedule(ls_state(gpu, 2.0 ** 9, found_inf=1, applied_steps=k, good_steps=7), OC.WARMUP, base, warm, bias_correction=True)
        assert torch.equal(old.cpu(), new), k
        lr = float(OC.inverse_time_decay(k, 2.0, 10_000, 1, True))
        lib().call("gct2_loss_scale_begin", old.data_ptr(), lr, 0, 0.9, 0.999, stream())
        new = begin_schedule(ls_state(gpu, 2.0 ** 9, found_inf=1, applied_steps=k, good_steps=7), OC.INVERSE_TIME_DECAY, 2.0, 10_000, 1, True, True)
        assert torch.equal(old.cpu(), new), k
        if k < 2:
            assert float(new.view(torch.float32)[5]) != lr           # (the correction does something while beta^t is not yet 0)


# ---- 3. train steps against the restatement ---------------------------------------------------------------------------------------------
def reference_lines():
    import gan_class_transfer2_amd as g
    return {"sgd_nesterov": lambda: g.SGD(0.25, 0.5, True), "sgd_decay": lambda: g.SGD(g.InverseTimeDecay(2.0, 10_000, 1)),
            "rmsprop_decay": lambda: g.RMSprop(g.InverseTimeDecay(1e-5, 10_000, 1))}


LINES = ("sgd_nesterov", "sgd_decay", "rmsprop_decay")


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


def hyper_of(eng):
    return dict(momentum=eng.momentum, nesterov=eng.nesterov, rho=eng.rho, epsilon=eng.epsilon)


def arenas_of(eng):
    A = eng.arena
    torch.cuda.synchronize()
    return {n: getattr(A, n).clone() for n in ("p", "m", "v") + (("shadow",) if A.shadow is not None else ())}


def put(eng, arenas):
    for n, t in arenas.items():
        getattr(eng.arena, n).copy_(t)


def inputs(gpu, tiny):
    return (torch.tensor(tiny.x, dtype=torch.float32, device=gpu), torch.tensor(tiny.t_int), torch.tensor(tiny.eps, dtype=torch.float32))


def own_gradients(eng):
    """the gradients the optimizer launches of the last step read: the engine's own arena, which the non-fused path fills and no
    optimizer launch writes.  NOT a twin engine's: at this topology (Fu_0 = 4) the head runs gct2_dense_bwd, whose Dense gradient is a
    sum of float atomics - two runs of ONE engine on the same inputs differ in dense.w or dense.b (measured on an MI355X in bf16, f16
    and fp32: eight of nine pairs of runs did, no other tensor ever differed) - so a twin's gradients reproduce the engine's only up to the order of those additions, and
    a reference built on them would test that order, not the optimizer (tests/test_clip_gpu.py reads its gradients the same way)."""
    assert eng._grads_in_arena
    torch.cuda.synchronize()
    return eng.arena.g.cpu().numpy()


def check_against_restatement(eng, before, grads, lr, dt, inv_scale=1.0):
    """p / m / v after the step are the restatement's bits on the arenas as they stood and the step's gradients; the shadow is the cast"""
    old = {n: t.cpu().numpy() for n, t in before.items() if n != "shadow"}
    p, m, v = OC.apply(lib().OPT_SGD if eng.optimizer_kind == "sgd" else lib().OPT_RMSPROP, old["p"], old["m"], old["v"], grads, lr,
                       hyper_of(eng), inv_scale=inv_scale)
    after = arenas_of(eng)
    assert same(after["p"], p) and same(after["m"], m) and same(after["v"], v)
    assert not torch.equal(after["p"], before["p"])
    if dt:
        assert torch.equal(after["shadow"].view(torch.int16), cast(dt, after["p"]).view(torch.int16))
    return after


@pytest.mark.parametrize("line", LINES)
def test_reference_lines_step_by_step(gpu, tiny, line):
    """three bf16 steps per optimizer line of the reference with fixed t_int / eps; numpy applies the restatement to the arenas as they
    stood, on the step's gradients (own_gradients: a twin engine cannot supply them bit for bit here) at the step size the host
    reports."""
    A = make_engine(gpu, 1, reference_lines()[line](), tiny.params)
    A.use_plan = False
    X, Tn, Ep = inputs(gpu, tiny)
    kind = A.optimizer_kind
    assert kind == ("rmsprop" if line == "rmsprop_decay" else "sgd") and (A.lr_schedule is None) == (line == "sgd_nesterov")
    for k in range(3):
        before = arenas_of(A)
        lr = A.step_size()
        assert lr == A.learning_rate(k) and np.float32(lr) == (np.float32(0.25) if line == "sgd_nesterov" else
                                                               OC.inverse_time_decay(k, *(OC.REFERENCE_SCHEDULES[line == "rmsprop_decay"])))
        A.train_step(X, Tn, Ep)
        after = check_against_restatement(A, before, own_gradients(A), lr, 1)
        assert A.iterations == k + 1 and A._grads_in_arena            # the non-fused path
        # the slots the kind does not use are never written
        if kind == "sgd":
            assert torch.equal(after["v"], before["v"])
        if A.momentum == 0:
            assert torch.equal(after["m"], before["m"])


@pytest.mark.parametrize("line", LINES)
def test_planned_steps_equal_eager_steps(gpu, line, recorded):
    """same seeds, the engines' own RNG streams: E runs eagerly, P - its arenas overwritten with E's before each step - under step plans
    (recorded at the second step, replayed from the third).  Every step of both is the restatement's bits on the engine's own
    gradients; where P's gradients equal E's bit for bit (own_gradients: the Dense gradient's float atomics may differ), P's arenas
    equal E's bit for bit: the planned step IS the eager step.  The plans hold gct2_optimizer_apply and no Adam call."""
    E, P = make_engine(gpu, 1, reference_lines()[line]()), make_engine(gpu, 1, reference_lines()[line]())
    E.use_plan, P.use_plan = False, True
    rng = np.random.default_rng(11)
    xs = [torch.tensor(rng.uniform(-1, 1, (BATCH, SIZE, SIZE, 3)), dtype=torch.float32, device=gpu) for _ in range(4)]
    for k in range(4):
        before = arenas_of(E)
        put(P, before)
        lr = E.step_size()
        assert lr == P.step_size()
        le, lp = E.train_step(xs[k]), P.train_step(xs[k])
        ge, gp = own_gradients(E), own_gradients(P)
        a, b = check_against_restatement(E, before, ge, lr, 1), check_against_restatement(P, before, gp, lr, 1)
        assert float(le[0]) == float(lp[0]), k                       # (the forward pass has no atomics: the same loss)
        if np.array_equal(bits(ge), bits(gp)):
            for n in a:
                assert torch.equal(a[n], b[n]), (k, n)
    assert E.iterations == P.iterations == 4 and not E._plans and len(P._plans) >= 1
    for sp in P._plans.values():
        names = recorded(sp.plan)
        assert len(names) > 10 and names.count("gct2_optimizer_apply") == 1 and not any(n.startswith("gct2_adam_") for n in names), names


def test_variant_engine_rmsprop_step(gpu):
    """block_depth = 1 at the smallest widths: one RMSprop step against numpy on the engine's own gradients"""
    from gan_class_transfer2_amd.variants import VariantEngine
    rng = np.random.default_rng(9)
    eng = VariantEngine(8, 16, 2, 1, False, True, 1, gpu, base_lr=1e-3, warm_up=0, seed=4)
    eng.set_optimizer("rmsprop", rho=0.9, momentum=0.9)
    x = torch.tensor(rng.uniform(-1, 1, (2, 16, 16, 3)), dtype=torch.float32, device=gpu)
    N = eng.net
    eng.train_step(x, apply=False)
    torch.cuda.synchronize()
    grads = N.g.cpu().numpy()
    assert np.isfinite(grads).all() and float(np.abs(grads).max()) > 0
    before = [t.cpu().numpy() for t in (N.p, N.m, N.v)]
    lr = eng.step_size()
    assert lr == float(np.float32(1e-3))
    eng.apply_adam()
    torch.cuda.synchronize()
    assert eng.iterations == 1
    want = OC.apply(OC.RMSPROP, *before, grads, lr, hyper_of(eng))
    assert same(N.p, want[0]) and same(N.m, want[1]) and same(N.v, want[2]) and not same(N.p, before[0])
    assert torch.equal(N.op.view(torch.int16), cast(1, N.p).view(torch.int16))


def test_fp16_loss_scaled_sgd_and_a_skipped_step(gpu, tiny):
    """LossScaleOptimizer(SGD(0.25, 0.5, True)) in fp16: an applied step against numpy at the step size read back from the device
    state (gct2_loss_scale_begin_schedule wrote it), then a step whose gradient arena holds one written inf: skipped - p, m, the
    shadow and iterations unchanged, the scale halved"""
    import gan_class_transfer2_amd as g
    A = make_engine(gpu, 2, g.LossScaleOptimizer(g.SGD(0.25, 0.5, True)), tiny.params)
    assert A.ls_state is not None and A.optimizer_kind == "sgd" and A.loss_scale() == (2.0 ** 15, 0)
    A.use_plan = False
    X, Tn, Ep = inputs(gpu, tiny)
    before = arenas_of(A)
    A.train_step(X, Tn, Ep)
    grads = own_gradients(A)                                     # scaled by 2^15
    assert np.isfinite(grads).all()
    lr = float(A.ls_state.view(torch.float32)[5].item())
    assert lr == 0.25 and A.iterations == 1 and A.loss_scale() == (2.0 ** 15, 1)
    st1 = check_against_restatement(A, before, grads, lr, 2, inv_scale=2.0 ** -15)
    A.train_step(X, Tn, Ep, apply=False)
    A.arena.g[5] = float("inf")
    A.check_finite(); A.apply_adam(); A.finish_step()
    torch.cuda.synchronize()
    st2 = arenas_of(A)
    assert all(torch.equal(st2[n], st1[n]) for n in st1)
    assert A.iterations == 1 and A.loss_scale() == (2.0 ** 14, 0)


def test_adam_under_inverse_time_decay(gpu, tiny):
    """an Adam engine with the new schedule: on the host path only adam_alpha reads another learning_rate.  Two steps against
    clip_cases.adam at adam_step_size(inverse_time_decay_lr(k, ...), k, ...)"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import trainer_math as TM
    A = make_engine(gpu, 1, g.Adam(g.InverseTimeDecay(1e-3, 1, 0.5)), tiny.params)
    A.use_plan, A.fuse_adam = False, False
    assert A.optimizer_kind == "adam" and A.lr_schedule == ("inverse_time_decay", 1e-3, 1.0, 0.5, False)
    X, Tn, Ep = inputs(gpu, tiny)
    for k in range(2):
        before = arenas_of(A)
        alpha = TM.adam_step_size(TM.inverse_time_decay_lr(k, 1e-3, 1, 0.5), k, A.beta_1, A.beta_2)
        assert A.step_size() == A.adam_alpha() == alpha
        A.train_step(X, Tn, Ep)
        grads = own_gradients(A)
        old = {n: t.cpu().numpy() for n, t in before.items() if n != "shadow"}
        p, m, v = K.adam(old["p"], old["m"], old["v"], grads, alpha, A.beta_1, A.beta_2, A.epsilon)
        after = arenas_of(A)
        assert same(after["p"], p) and same(after["m"], m) and same(after["v"], v), k
        assert torch.equal(after["shadow"].view(torch.int16), cast(1, after["p"]).view(torch.int16))
    assert TM.inverse_time_decay_lr(1, 1e-3, 1, 0.5) < TM.inverse_time_decay_lr(0, 1e-3, 1, 0.5) and A.iterations == 2


# ---- 4. through the public interface ----------------------------------------------------------------------------------------------------
@pytest.fixture
def tiny_model():
    """the module-level hyper-parameters of the tiny bf16 network, put back afterwards"""
    import gan_class_transfer2_amd as g
    names = ("size", "pixel_size", "max_size", "octaves", "compute_dtype", "mixed_precision", "block_depth", "residual", "concat", "warm_up")
    keep = {n: getattr(g.model, n) for n in names}
    g.configure(size=SIZE, pixel_size=TOPO[0], max_size=TOPO[1], octaves=TOPO[2], compute_dtype="bfloat16", mixed_precision=False, block_depth=0,
                residual=False, concat=True)
    yield g
    g.configure(**keep)


def test_trainer_compile_and_train_step(gpu, tiny_model):
    g = tiny_model
    opt = g.SGD(g.InverseTimeDecay(2.0, 10_000, 1))
    tr = g.Trainer(g.Denoiser(seed=3, device=gpu))
    tr.compile(opt, g.identity)
    rng = np.random.default_rng(2)
    for k in range(2):
        x = torch.tensor(rng.uniform(-1, 1, (BATCH, SIZE, SIZE, 3)), dtype=torch.float32, device=gpu)
        out = tr.train_step((x, x))
        assert out["loss"].shape == (1,)
    eng = tr.denoiser.engine
    torch.cuda.synchronize()
    assert opt.iterations == 2 == eng.iterations and isinstance(eng, g.UNetEngine)
    assert (eng.optimizer_kind, eng.momentum, eng.lr_schedule) == ("sgd", 0.0, ("inverse_time_decay", 2.0, 10_000.0, 1.0, False))
    for k in (0, 1, 2, 10_000):
        assert eng.learning_rate(k) == float(OC.inverse_time_decay(k, 2.0, 10_000, 1)) == opt.lr(k)
    assert eng.learning_rate() == eng.learning_rate(2)
    # another optimizer line on the engine that has stepped: same kind, new hyper-parameters - allowed; another kind - refused
    tr.compile(g.SGD(0.25, 0.5, True), g.identity)
    assert (eng.momentum, eng.nesterov, eng.lr_schedule, eng.base_lr) == (0.5, True, None, 0.25)
    with pytest.raises(g.Gct2Error, match="already applied 2 steps"):
        tr.compile(g.RMSprop(g.InverseTimeDecay(1e-5, 10_000, 1)), g.identity)
    assert eng.optimizer_kind == "sgd"


def test_rmsprop_with_use_ema(gpu, tiny):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import trainer_math as TM
    eng = make_engine(gpu, 1, g.RMSprop(1e-3, use_ema=True, ema_momentum=0.9), tiny.params)
    assert eng.use_ema and eng.optimizer_kind == "rmsprop"
    p0 = eng.arena.p.clone()
    assert torch.equal(eng.arena.ema, p0)
    eng.train_step(inputs(gpu, tiny)[0])
    p1, ema = eng.arena.p.clone(), eng.arena.ema.clone()
    m, c = TM.ema_coefficients(0.9)
    want = np.float32(m) * p0.cpu().numpy() + np.float32(c) * p1.cpu().numpy()
    assert not torch.equal(p1, p0) and same(ema, want) and torch.equal(eng.arena.ema_shadow.view(torch.int16), cast(1, ema).view(torch.int16))


def test_state_dict_round_trip(gpu, tiny):
    import gan_class_transfer2_amd as g
    X = inputs(gpu, tiny)[0]
    new = lambda seed: make_engine(gpu, 1, g.RMSprop(1e-3, momentum=0.9), rng_seed=seed)
    a = new(5)
    a.set_params(tiny.params)
    for _ in range(2):
        a.train_step(X)
    sd = a.state_dict()
    assert set(sd) == {"arena.p", "arena.m", "arena.v", "counters", "topology", "optimizer"}
    assert sd["optimizer"].tolist() == [float(OC.RMSPROP), 0.9, 0.0, 0.9]
    adam = make_engine(gpu, 1)
    assert set(adam.state_dict()) == {"arena.p", "arena.m", "arena.v", "counters", "topology"}         # Adam: the dictionary of before
    b = new(99)
    b.load_state_dict(sd)
    assert b.iterations == 2 and (b.rng_seed, b.rng_offset_t, b.rng_offset_eps) == (a.rng_seed, a.rng_offset_t, a.rng_offset_eps)
    state = arenas_of(a)
    assert all(torch.equal(t, state[n]) for n, t in arenas_of(b).items())
    # both continue: the same loss, each the restatement's bits on its own gradients - and the same bits where those are the same
    lr = a.step_size()
    assert lr == b.step_size()
    la, lb = a.train_step(X), b.train_step(X)
    ga, gb = own_gradients(a), own_gradients(b)
    assert float(la[0]) == float(lb[0])
    sa, sb = check_against_restatement(a, state, ga, lr, 1), check_against_restatement(b, state, gb, lr, 1)
    if np.array_equal(bits(ga), bits(gb)):
        assert all(torch.equal(sa[n], sb[n]) for n in sa)
    c = new(7)
    c.load_named_state_dict(a.named_state_dict())                  # the exchange format by parameter name carries the kind too
    assert torch.equal(c.arena.m, a.arena.m) and c.iterations == 3
    before = arenas_of(adam)
    with pytest.raises(ValueError, match="rmsprop"):
        adam.load_state_dict(sd)
    with pytest.raises(ValueError, match="adam"):
        new(1).load_state_dict(adam.state_dict())
    after = arenas_of(adam)
    assert all(torch.equal(after[n], before[n]) for n in before)   # refused before anything was copied


# ---- 5. the default is untouched ----------------------------------------------------------------------------------------------------------
def test_default_step_records_neither_new_entry_point(gpu, recorded):
    import gan_class_transfer2_amd as g
    eng = make_engine(gpu, 1, g.Adam(g.WarmUp(1e-2, 3)))
    rng = np.random.default_rng(11)
    xs = [torch.tensor(rng.uniform(-1, 1, (BATCH, SIZE, SIZE, 3)), dtype=torch.float32, device=gpu) for _ in range(4)]
    keys = []
    for x in xs:
        b, cur = eng.buffers(BATCH, SIZE, SIZE), torch.cuda.current_stream(eng.device)
        eng.train_step(x)
        keys.append(eng._plan_key(b, True, True, cur))
    torch.cuda.synchronize()
    assert eng.optimizer_kind == "adam" and eng.lr_schedule is None and not eng._grads_in_arena      # the fused path
    assert keys[2] == keys[3] and keys[3] in eng._plans            # unchanged settings: one key, its plan replayed
    assert len(eng._plans) >= 1
    for sp in eng._plans.values():
        names = recorded(sp.plan)
        assert len(names) > 10 and not any(n in names for n in NEW), names
    # ... and with loss scaling the Adam + WarmUp step goes on calling gct2_loss_scale_begin
    ls = make_engine(gpu, 2, g.LossScaleOptimizer(g.Adam(g.WarmUp(1e-2, 3))))
    for x in xs:
        ls.train_step(x)
    torch.cuda.synchronize()
    assert len(ls._plans) >= 1
    for sp in ls._plans.values():
        names = recorded(sp.plan)
        assert "gct2_loss_scale_begin" in names and not any(n in names for n in NEW), names


# ---- 6. what is refused -------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu, tiny):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.distributed import DataParallelStep, ShardedDataParallelStep
    eng = make_engine(gpu, 1, g.SGD(0.25, 0.5, True), tiny.params)
    eng.train_step(inputs(gpu, tiny)[0])
    assert eng.iterations == 1
    before = arenas_of(eng)
    for change in (lambda: eng.set_optimizer("adam"), lambda: eng.set_optimizer("rmsprop"),
                   lambda: g.Trainer(types.SimpleNamespace(engine=eng)).compile(g.Adam(g.WarmUp(1e-2, 0)), g.identity)):
        with pytest.raises(g.Gct2Error, match="already applied 1 steps with sgd"):
            change()
    assert eng.optimizer_kind == "sgd" and all(torch.equal(t, before[n]) for n, t in arenas_of(eng).items())
    eng.set_optimizer("sgd", momentum=0.9)                         # the kind's own hyper-parameters may change
    for Wrapper in (DataParallelStep, ShardedDataParallelStep):
        for kind in ("sgd", "rmsprop"):
            fresh = make_engine(gpu, 1)
            fresh.set_optimizer(kind)
            hooks = (fresh.grad_ready_hook, fresh.post_backward)
            with pytest.raises(ValueError, match=Wrapper.__name__):
                Wrapper(fresh)
            assert (fresh.grad_ready_hook, fresh.post_backward) == hooks                  # refused before it touched the engine
            assert not hasattr(fresh, "_optimizer_forbidden") and not hasattr(fresh, "_clip_forbidden")
        plain = make_engine(gpu, 1)
        Wrapper(plain)
        for kind in ("sgd", "rmsprop"):
            with pytest.raises(ValueError, match=Wrapper.__name__):
                plain.set_optimizer(kind)
        plain.set_optimizer("adam")
        assert plain.optimizer_kind == "adam"
    with pytest.raises(NotImplementedError, match="centered"):
        g.RMSprop(centered=True)
