"""Gradient clipping (Keras Adam(clipnorm / global_clipnorm / clipvalue) [TF]) on the GPU: gct2_grad_sumsq against float64 numpy
(equal on exact-sum inputs, within the bound of any summation order on random ones, identical bits on two streams, the found_inf
flag), gct2_adam_keras_clipped per element and bit for bit, and clipped train steps of both engines against numpy - eager and
planned, with loss scaling, through Trainer.compile - plus what is refused.

The reference of every bit-exact check is the arithmetic of include/gct2.h restated in tests/clip_cases.py.  Buffers carry NaN in
every gap, in the alignment padding and in guard elements on both sides of what a kernel may read, and sentinels behind every range
a kernel may write.  PARITY UNPINNED w.r.t. TensorFlow (there is none here)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import clip_cases as K

pytestmark = pytest.mark.gpu
TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
NONE, VALUE, NORM, GLOBAL = K.CLIP_NONE, K.CLIP_VALUE, K.CLIP_NORM, K.CLIP_GLOBAL_NORM
NEW = ("gct2_grad_sumsq", "gct2_adam_keras_clipped")
SENTINEL = 12345.0


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def cast(dt, src):
    """what gct2_cast_from_f32 writes from an fp32 device tensor: the project's one round-to-nearest-even conversion"""
    out = torch.empty(src.numel(), dtype=TDT[dt], device=src.device)
    lib().call("gct2_cast_from_f32", dt, src.data_ptr(), out.data_ptr(), src.numel(), stream())
    return out


def same(dev, want):
    """float32 device tensor == numpy array: NaN where NaN, the same bits (so also the sign of zero) everywhere else"""
    got = dev.detach().cpu().numpy()
    want = np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))


def same16(a, b):
    """two 16-bit device tensors: NaN where NaN, the same bits everywhere else"""
    nan = torch.isnan(a)
    return a.shape == b.shape and torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan].view(torch.int16), b[~nan].view(torch.int16))


def ls_state(gpu, scale=2.0 ** 15, found_inf=0, alpha=0.0):
    """a gct2_loss_scale_state on the device: {scale, inv_scale, good_steps, found_inf, applied_steps, alpha, reserved[2]}"""
    st = torch.zeros(8, dtype=torch.int32, device=gpu)
    lib().call("gct2_loss_scale_init", st.data_ptr(), float(scale), stream())
    st[3] = found_inf
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


# ---- 1. gct2_grad_sumsq ---------------------------------------------------------------------------------------------------------------
class Reduction:
    """the device side of one segment layout: table, partials and sumsq with sentinels behind them"""

    def __init__(self, gpu, segs):
        n = len(segs)
        begin, count = (ctypes.c_uint64 * n)(*[b for b, _ in segs]), (ctypes.c_uint64 * n)(*[c for _, c in segs])
        out, npart = (ctypes.c_uint64 * (3 * n))(), ctypes.c_size_t(0)
        lib().check(lib().load().gct2_sumsq_layout(begin, count, n, out, ctypes.byref(npart)), "gct2_sumsq_layout")
        self.segs, self.nseg, self.npart = segs, n, npart.value
        assert self.npart == sum(K.partial_counts(segs))
        self.table = torch.tensor(list(out), dtype=torch.int64).to(gpu)
        self.partials = torch.full((self.npart + 8,), SENTINEL, dtype=torch.float64, device=gpu)
        self.sumsq = torch.full((n + 1 + 8,), SENTINEL, dtype=torch.float64, device=gpu)

    def run(self, g, grad_mul=1.0, ls=None, s=None):
        before = g.clone()
        self.partials.fill_(SENTINEL); self.sumsq.fill_(SENTINEL)
        lib().call("gct2_grad_sumsq", g.data_ptr(), self.table.data_ptr(), self.nseg, self.npart, float(grad_mul),
                   None if ls is None else ls.data_ptr(), self.partials.data_ptr(), self.sumsq.data_ptr(), stream() if s is None else s)
        torch.cuda.synchronize()
        assert torch.equal(g.view(torch.int32), before.view(torch.int32))                       # g is read only
        assert bool((self.partials[self.npart:] == SENTINEL).all()) and bool((self.sumsq[self.nseg + 1:] == SENTINEL).all())
        return self.sumsq[:self.nseg + 1].cpu().numpy(), self.partials[:self.npart].cpu().numpy()


@pytest.fixture(scope="module")
def reduction(gpu):
    segs, total = K.layout()
    assert len(segs) == 10 and all(b % 64 == 0 for b, _ in segs)
    K.assert_exact_bound(segs)
    rng = np.random.default_rng(5)
    exact = K.poisoned(lambda s, n: K.exact_values(rng, n), segs, total)
    normal = K.poisoned(lambda s, n: rng.standard_normal(n).astype(np.float32), segs, total)
    return Reduction(gpu, segs), exact, normal, total


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "grad_mul_and_loss_scale"])
def test_grad_sumsq_equals_numpy_on_exact_inputs(gpu, reduction, scaled):
    R, exact, _, _ = reduction
    g = torch.from_numpy(exact).to(gpu)
    ls = ls_state(gpu, 2.0 ** 7) if scaled else None
    got, partials = R.run(g, 0.5 if scaled else 1.0, ls)
    want = K.segment_sumsq(K.scaled(exact, 0.5, 2.0 ** -7) if scaled else exact, R.segs)
    assert np.isfinite(want).all() and want[-1] > 0
    assert np.array_equal(got, want), (got, want)
    # one partial per chunk, a chunk never straddles a segment: partial c of segment s is the sum over its own CHUNK elements
    at = 0
    for (b, c), np_s in zip(R.segs, K.partial_counts(R.segs)):
        for k in range(np_s):
            piece = exact[b + k * K.CHUNK:b + min(c, (k + 1) * K.CHUNK)]
            assert partials[at + k] == K.sumsq(K.scaled(piece, 0.5, 2.0 ** -7) if scaled else piece), (b, k)
        at += np_s
    if scaled:
        assert int(ls[3]) == 0                                       # finite gradients: the flag stays clear


def test_grad_sumsq_within_the_bound_of_any_summation_order(gpu, reduction):
    """non-negative float64 terms: any order of n - 1 additions is within (n - 1) * 2^-53 relative of the exact sum (first order), so
    count_s * 2^-53 relative against numpy's float64 sum is derived, not measured.  The total is the sequential float64 sum of the
    segment sums, which the host repeats exactly."""
    R, _, normal, _ = reduction
    got, _ = R.run(torch.from_numpy(normal).to(gpu))
    want = K.segment_sumsq(normal, R.segs)
    for s, (_, c) in enumerate(R.segs):
        assert abs(got[s] - want[s]) <= c * 2.0 ** -53 * want[s], (s, c, got[s], want[s])
    total = np.float64(0.0)
    for v in got[:-1]:
        total = total + v
    assert got[-1] == total


def test_grad_sumsq_same_bits_on_two_streams(gpu, reduction):
    R, _, normal, _ = reduction
    g = torch.from_numpy(normal).to(gpu)
    out = []
    for _ in range(2):
        s = torch.cuda.Stream(device=gpu)
        torch.cuda.synchronize()
        sums, partials = R.run(g, s=s.cuda_stream)
        out.append((sums.tobytes(), partials.tobytes()))
    assert out[0] == out[1]


@pytest.mark.parametrize("where", ["inf_first_of_first", "nan_last_of_last", "poison_only", "ls_null"])
def test_grad_sumsq_sets_found_inf_for_raw_elements_inside_segments_only(gpu, reduction, where):
    R, _, normal, total = reduction
    buf = normal.copy()
    (b0, _), (b9, c9) = R.segs[0], R.segs[-1]
    if where in ("inf_first_of_first", "ls_null"):
        buf[b0] = np.inf
    elif where == "nan_last_of_last":
        buf[b9 + c9 - 1] = np.nan
    assert np.isnan(buf[:K.GUARD]).all() and np.isnan(buf[b9 + c9:]).all()      # the poison outside the segments is always there
    if where == "ls_null":
        watch = torch.zeros(8, dtype=torch.int32, device=gpu)          # nobody was told about this state: it must stay as it is
        R.run(torch.from_numpy(buf).to(gpu), ls=None)
        assert int(watch.abs().sum()) == 0
        return
    # a scale at which the SCALED values are harmless either way: the flag looks at the raw element
    ls = ls_state(gpu, 2.0 ** 7)
    got, _ = R.run(torch.from_numpy(buf).to(gpu), ls=ls)
    assert int(ls[3]) == (0 if where == "poison_only" else 1)
    assert ls.view(torch.float32)[0].item() == 2.0 ** 7 and ls.view(torch.float32)[1].item() == 2.0 ** -7 and int(ls[4]) == 0
    if where == "poison_only":
        assert np.isfinite(got).all()                                  # elements outside every segment were never read


# ---- 2. gct2_adam_keras_clipped, per element and bit for bit --------------------------------------------------------------------------
HYPER = dict(alpha=1.5e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
SIZES = (1, 3, 4, 5, 1023, 1024, 1029)
PAD = 64


class Arenas:
    """p, m, v, g (and a 16-bit shadow) over [off, off + n) of buffers that hold sentinels (NaN in g) everywhere else"""

    def __init__(self, gpu, dt, n, off, p, m, v, g):
        self.dt, self.n, self.off = dt, n, off
        total = off + n + PAD
        mk = lambda fill, vals: self._fill(torch.full((total,), fill, dtype=torch.float32, device=gpu), vals)
        self.p, self.m, self.v = mk(SENTINEL, p), mk(-SENTINEL, m), mk(2 * SENTINEL, v)
        self.g = mk(float("nan"), g)
        self.sh = torch.full((total,), 77.0, dtype=TDT[dt], device=gpu) if dt else None
        self.g_before = self.g.clone()

    def _fill(self, buf, vals):
        buf[self.off:self.off + self.n] = torch.from_numpy(np.asarray(vals, dtype=np.float32)).to(buf.device)
        return buf

    def ptrs(self):
        o = self.off
        return (self.p.data_ptr() + 4 * o, self.m.data_ptr() + 4 * o, self.v.data_ptr() + 4 * o, self.g.data_ptr() + 4 * o,
                self.sh.data_ptr() + 2 * o if self.dt else None, self.dt, self.n)

    def clipped(self, mode, clip, sumsq_ptr, ls=None, grad_mul=1.0, alpha=HYPER["alpha"]):
        lib().call("gct2_adam_keras_clipped", *self.ptrs(), alpha, HYPER["beta_1"], HYPER["beta_2"], HYPER["epsilon"], float(grad_mul),
                   None if ls is None else ls.data_ptr(), mode, float(clip), sumsq_ptr, stream())
        torch.cuda.synchronize()

    def inside(self, t):
        return t[self.off:self.off + self.n]

    def check_outside(self):
        o, e = self.off, self.off + self.n
        for t, fill in ((self.p, SENTINEL), (self.m, -SENTINEL), (self.v, 2 * SENTINEL)):
            assert bool((t[:o] == fill).all()) and bool((t[e:] == fill).all())
        if self.sh is not None:
            assert bool((self.sh[:o].float() == 77.0).all()) and bool((self.sh[e:].float() == 77.0).all())
        assert torch.equal(self.g.view(torch.int32), self.g_before.view(torch.int32))          # g is read only (never zeroed)


def _inputs(rng, n):
    return (rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 1e-2).astype(np.float32),
            (rng.random(n) * 1e-4).astype(np.float32), rng.standard_normal(n).astype(np.float32))


# (mode, clip, *sumsq, NaN gradient): every mode on both sides of its threshold - values inside and outside +-clip (standard-normal
# gradients against 0.5), a *sumsq below and above clip^2 - plus *sumsq = 0 and inf, and one NaN gradient under VALUE
CLIP_CASES = [(NONE, 0.0, None, False), (VALUE, 0.5, None, False), (VALUE, 0.5, None, True), (VALUE, 1e3, None, False)] + \
             [(mode, 1.5, ss, False) for mode in (NORM, GLOBAL) for ss in (0.25, 2.0, 2.25, 9.0, 0.0, float("inf"))]


@pytest.mark.parametrize("dt", [0, 1, 2], ids=["noshadow", "bf16", "f16"])
def test_adam_keras_clipped_per_element(gpu, dt):
    rng = np.random.default_rng(40 + dt)
    ss_dev = torch.full((3,), float("nan"), dtype=torch.float64, device=gpu)             # the ONE value sits between two NaN
    for n in SIZES:
        for off in (0, 64):
            for mode, clip, ss, with_nan in CLIP_CASES:
                p, m, v, g = _inputs(rng, n)
                if with_nan:
                    g[n // 2] = np.nan
                if mode == VALUE and n >= 1023 and clip == 0.5:
                    assert (np.abs(g[~np.isnan(g)]) > clip).any() and (np.abs(g[~np.isnan(g)]) < clip).any()
                A = Arenas(gpu, dt, n, off, p, m, v, g)
                if ss is not None:
                    ss_dev[1] = ss
                A.clipped(mode, clip, ss_dev.data_ptr() + 8 if ss is not None else None)
                want = K.clipped_adam(p, m, v, g, mode=mode, threshold=clip, ss=ss, **HYPER)
                tag = (n, off, mode, clip, ss, with_nan)
                for got, w in zip((A.p, A.m, A.v), want):
                    assert same(A.inside(got), w), tag
                if with_nan:
                    assert np.isnan(want[0][n // 2]) and np.isnan(want[0]).sum() == 1       # a NaN stays NaN - and stays alone
                if mode == GLOBAL and ss == float("inf"):
                    assert np.isnan(want[0]).all()
                if dt:
                    assert same16(A.inside(A.sh), cast(dt, A.inside(A.p).contiguous())), tag
                A.check_outside()


@pytest.mark.parametrize("dt", [0, 1, 2], ids=["noshadow", "bf16", "f16"])
def test_clip_none_is_adam_keras_multi_bit_for_bit(gpu, dt):
    rng = np.random.default_rng(50 + dt)
    for n in SIZES:
        for off in (0, 64):
            for scaled in (False, True):
                p, m, v, g = _inputs(rng, n)
                ls = ls_state(gpu, 2.0 ** 9, alpha=2.5e-3) if scaled else None
                A, B = Arenas(gpu, dt, n, off, p, m, v, g), Arenas(gpu, dt, n, off, p, m, v, g)
                A.clipped(NONE, 0.0, None, ls=ls, grad_mul=0.25 if scaled else 1.0)
                lib().call("gct2_adam_keras_multi", *B.ptrs(), HYPER["alpha"], HYPER["beta_1"], HYPER["beta_2"], HYPER["epsilon"],
                           0.25 if scaled else 1.0, None if ls is None else ls.data_ptr(), 0, stream())
                torch.cuda.synchronize()
                for a, b in ((A.p, B.p), (A.m, B.m), (A.v, B.v)) + (((A.sh, B.sh),) if dt else ()):
                    assert torch.equal(a, b), (n, off, scaled)
                # ... and both are the restatement: with a loss-scale state, its inv_scale and ITS alpha
                kw = dict(HYPER, alpha=2.5e-3) if scaled else HYPER
                want = K.clipped_adam(p, m, v, g, mode=NONE, threshold=0.0, grad_mul=0.25 if scaled else 1.0,
                                      inv_scale=2.0 ** -9 if scaled else 1.0, **kw)
                assert same(A.inside(A.p), want[0]) and same(A.inside(A.m), want[1]) and same(A.inside(A.v), want[2])
                A.check_outside()


@pytest.mark.parametrize("mode, clip, ss", [(NONE, 0.0, None), (VALUE, 0.5, None), (NORM, 1.5, 9.0), (GLOBAL, 1.5, 9.0)])
def test_adam_keras_clipped_is_gated_by_found_inf(gpu, mode, clip, ss):
    rng = np.random.default_rng(60 + mode)
    ss_dev = torch.tensor([9.0], dtype=torch.float64, device=gpu)
    for found_inf in (1, 0):
        for n in (5, 1029):
            p, m, v, g = _inputs(rng, n)
            ls = ls_state(gpu, 2.0 ** 9, found_inf=found_inf, alpha=2.5e-3)
            A = Arenas(gpu, 1, n, 64, p, m, v, g)
            A.clipped(mode, clip, ss_dev.data_ptr() if ss is not None else None, ls=ls)
            if found_inf:                                            # the skipped step writes nothing
                assert same(A.inside(A.p), p) and same(A.inside(A.m), m) and same(A.inside(A.v), v)
                assert bool((A.inside(A.sh).float() == 77.0).all())
            else:                                                    # ... and an applied one unscales and takes the state's alpha
                want = K.clipped_adam(p, m, v, g, mode=mode, threshold=clip, ss=ss, inv_scale=2.0 ** -9, **dict(HYPER, alpha=2.5e-3))
                assert same(A.inside(A.p), want[0]) and same(A.inside(A.m), want[1]) and same(A.inside(A.v), want[2])
                assert not same(A.inside(A.p), p)
            A.check_outside()
            assert int(ls[3]) == found_inf


# ---- 3. clipped train steps against numpy ------------------------------------------------------------------------------------------
TOPO, SIZE, BATCH = (8, 16, 2), 16, 2                 # the smallest topology the step tests use
MODE_KW = {VALUE: "clipvalue", NORM: "clipnorm", GLOBAL: "global_clipnorm"}


def make_engine(gpu, dt, **kw):
    import gan_class_transfer2_amd as g
    return g.UNetEngine(g.Topology(*TOPO), dt, gpu, base_lr=1e-2, warm_up=0, seed=21, rng_seed=5, **kw)


def batches(gpu, n=4, seed=11):
    rng = np.random.default_rng(seed)
    return [torch.tensor(rng.uniform(-1, 1, (BATCH, SIZE, SIZE, 3)), dtype=torch.float32, device=gpu) for _ in range(n)]


def arenas_of(eng):
    A = eng.arena
    torch.cuda.synchronize()
    return {n: getattr(A, n).clone() for n in ("p", "m", "v") + (("shadow",) if A.shadow is not None else ())}


def thresholds(g, segs):
    """from first-step gradients: half the global norm, half the largest per-tensor norm, the median absolute value"""
    inside = np.concatenate([g[b:b + c] for b, c in segs]).astype(np.float64)
    per_tensor = [float(np.sqrt(np.sum(g[b:b + c].astype(np.float64) ** 2))) for b, c in segs]
    return {GLOBAL: 0.5 * float(np.sqrt(np.sum(inside ** 2))), NORM: 0.5 * max(per_tensor), VALUE: float(np.median(np.abs(inside)))}


def clipped_fraction(g, segs, mode, thr):
    """how much of the arena the threshold touches: elements beyond +-clip / tensors whose norm exceeds it / 1 if the global norm does"""
    if mode == VALUE:
        inside = np.concatenate([g[b:b + c] for b, c in segs])
        return float((np.abs(inside) > np.float32(thr)).mean())
    ss = K.segment_sumsq(g, segs)
    if mode == NORM:
        return float(np.mean([np.float32(np.sqrt(v)) > np.float32(thr) for v in ss[:-1]]))
    return float(np.float32(np.sqrt(ss[-1])) > np.float32(thr))


@pytest.fixture(scope="module")
def first_step(gpu):
    """first-step gradients of the twin engine per dtype (computed once): the thresholds of every step test come from them"""
    out = {}
    for dt in (0, 1):
        B = make_engine(gpu, dt)
        B.fuse_adam = False
        B.train_step(batches(gpu)[0], apply=False)
        torch.cuda.synchronize()
        g = B.arena.g.cpu().numpy()
        assert np.isfinite(g).all() and float(np.abs(g).max()) > 0
        out[dt] = thresholds(g, B._clip_segments())
    return out


def check_step(eng, before, k, segs, mask, mode, thr, dt):
    """one applied clipped step of `eng` against numpy: the gradients are the ones its optimizer launches read - the engine's own
    arena, which the clipped launches never write - clipped by tests/clip_cases.py and applied by Keras Adam in float32 to the
    arenas as they stood before the step; p, m, v and the shadow must be these bits.  Returns (gradients, arenas after)."""
    g = eng.arena.g.cpu().numpy()
    assert np.isfinite(g).all()
    g2 = K.clip_arena(g, segs, mode, thr)
    old = {n: t.cpu().numpy() for n, t in before.items() if n != "shadow"}
    p, m, v = K.adam(old["p"], old["m"], old["v"], g2, eng.adam_alpha(k), eng.beta_1, eng.beta_2, eng.epsilon)
    if mode == NORM:                                             # one launch per tensor: the padding between tensors is not touched
        p, m, v = (np.where(mask, new, old[n]) for new, n in ((p, "p"), (m, "m"), (v, "v")))
    after = arenas_of(eng)
    assert same(after["p"], p) and same(after["m"], m) and same(after["v"], v), k
    assert not torch.equal(after["p"], before["p"])
    if dt:
        assert torch.equal(after["shadow"].view(torch.int16), cast(dt, after["p"]).view(torch.int16))
    return g, after


@pytest.mark.parametrize("factor", [1.0, 10.0], ids=["active", "tenfold"])
@pytest.mark.parametrize("mode", [VALUE, NORM, GLOBAL], ids=["clipvalue", "clipnorm", "global_clipnorm"])
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_clipped_steps_equal_numpy(gpu, first_step, recorded, dt, mode, factor):
    """engine A clips, eagerly; engine P - same seeds, its arenas overwritten with A's before each step - makes the same steps under
    step plans (recorded at the second, replayed from the third).  After every step numpy clips the gradients the engine's optimizer
    launches consumed, applies Keras Adam in float32 and must reproduce p, m, v and the shadow bit for bit - for A and for P.  The
    gradients are read from the engine's OWN arena (a clipped step leaves them there untouched): at this topology the fp32
    weight-gradient kernels add their row splits with float atomics, so a twin engine's gradients equal A's only up to the order of
    those additions, and a reference built on a twin's gradients would test that order, not the clipping.  Where P's gradients do
    equal A's bit for bit, P's arenas must equal A's bit for bit.  The thresholds come from a twin's first-step gradients (fixture).
    factor 1: the threshold bites (asserted); factor 10: the norm modes no longer clip (asserted; the kernels still run, with a scale
    of clip * (1 / clip)), clipvalue clips fewer elements."""
    thr = factor * first_step[dt][mode]
    xs = batches(gpu)
    A, P = make_engine(gpu, dt), make_engine(gpu, dt)
    A.use_plan, P.use_plan = False, True
    for e in (A, P):
        e.set_clipping(**{MODE_KW[mode]: thr})
    segs = A._clip_segments()
    mask = np.zeros(A.arena.total, dtype=bool)
    for b, c in segs:
        mask[b:b + c] = True
    for k in range(4):
        before = arenas_of(A)
        for n, t in before.items():
            getattr(P.arena, n).copy_(t)
        assert A._clip_table is None or mode != VALUE                # clipvalue never allocates the reduction's buffers
        A.train_step(xs[k])
        P.train_step(xs[k])
        torch.cuda.synchronize()
        assert A.iterations == P.iterations == k + 1
        g, after = check_step(A, before, k, segs, mask, mode, thr, dt)
        gP, afterP = check_step(P, before, k, segs, mask, mode, thr, dt)
        if np.array_equal(g.view(np.int32), gP.view(np.int32)):      # the same gradients: the planned step IS the eager step
            for n in after:
                assert torch.equal(after[n], afterP[n]), (k, n)
        frac = clipped_fraction(g, segs, mode, thr)
        if k == 0:
            assert frac > 0 if factor == 1.0 else (frac == 0 if mode != VALUE else frac < clipped_fraction(g, segs, mode, thr / factor))
            if factor == 1.0:                                        # the clipping is visible in the result, not only in the reference
                plain = K.adam(before["p"].cpu().numpy(), before["m"].cpu().numpy(), before["v"].cpu().numpy(), g, A.adam_alpha(k),
                               A.beta_1, A.beta_2, A.epsilon)
                assert not same(after["m"], plain[1])
    assert A._grads_in_arena and not A._plans                        # the non-fused path, eagerly
    assert (A._clip_table is None) == (mode == VALUE)
    assert len(P._plans) >= 1
    for sp in P._plans.values():
        names = recorded(sp.plan)
        assert names.count("gct2_adam_keras_clipped") == (len(segs) if mode == NORM else 1)
        assert names.count("gct2_grad_sumsq") == (0 if mode == VALUE else 1) and "gct2_adam_keras_multi" not in names
        if mode != VALUE:
            assert names.index("gct2_grad_sumsq") < names.index("gct2_adam_keras_clipped")


def test_recompiled_threshold_reaches_replayed_steps_and_off_returns_to_inline(gpu, first_step, recorded):
    """Trainer.compile() with another threshold after the plan was recorded: the threshold is baked into recorded arguments, so it is
    part of the plan's key.  Every step of the planned engine - recorded and replayed ones, before and after the change - is checked
    against numpy with the threshold that holds at that step, on the engine's own gradients.  An optimizer without clipping switches
    it off: plans without the new entry points, fused (inline) optimizer steps again."""
    import gan_class_transfer2_amd as g
    thr = first_step[1][GLOBAL]
    xs = batches(gpu)
    eng = make_engine(gpu, 1)
    eng.use_plan = True
    segs = eng._clip_segments()
    tr = g.Trainer(types.SimpleNamespace(engine=eng))
    opt = lambda **kw: g.Adam(g.WarmUp(1e-2, 0), **kw)
    step, fractions = 0, []
    for phase, kw in enumerate((dict(global_clipnorm=thr), dict(global_clipnorm=0.25 * thr), dict())):
        tr.compile(opt(**kw), g.identity)
        assert (eng.clip_mode, eng.clip) == ((GLOBAL, kw["global_clipnorm"]) if kw else (NONE, 0.0))
        known = set(eng._plans)
        for k in range(4):
            before = arenas_of(eng)
            eng.train_step(xs[k])
            torch.cuda.synchronize()
            if kw:
                gr, _ = check_step(eng, before, step, segs, None, GLOBAL, kw["global_clipnorm"], 1)
                fractions.append(clipped_fraction(gr, segs, GLOBAL, kw["global_clipnorm"]))
            step += 1
            assert eng.iterations == step
        assert eng._grads_in_arena == bool(kw)                         # clipped: the arena path; off: inline (fused) steps again
        fresh = [sp for key, sp in eng._plans.items() if key not in known]
        assert fresh, phase                                            # every setting records its own plan
        for sp in fresh:
            names = recorded(sp.plan)
            assert len(names) > 10 and all((n in names) == bool(kw) for n in NEW), (phase, [n for n in names if n in NEW])
    assert fractions[0] == 1.0 and fractions[4] == 1.0                 # both thresholds bit when they took over



def test_clipping_off_records_none_of_the_new_symbols(gpu, recorded):
    eng = make_engine(gpu, 1)
    for x in batches(gpu):
        eng.train_step(x)
    torch.cuda.synchronize()
    assert eng.clip_mode == NONE and eng._clip_table is None and len(eng._plans) >= 1
    for sp in eng._plans.values():
        assert len(recorded(sp.plan)) > 10 and not any(n in recorded(sp.plan) for n in NEW)


# ---- 4. fp16 + loss scaling + global_clipnorm ------------------------------------------------------------------------------------------
def test_loss_scaled_overflow_is_skipped_and_the_next_step_is_clipped(gpu, monkeypatch):
    """the recipe of test_fp16_overflow_inside_the_reverse_pass_skips_the_step (tests/test_step_gpu.py): fp16, one applied step, then
    the scale re-initialised to 2^28, at which the scaled fp16 gradients overflow inside the reverse pass.  With global_clipnorm the
    reduction is what sets found_inf: the step is skipped (parameters and moments untouched, iterations not advanced, scale halved)
    and the step's launches hold no gct2_scale_check_finite.  The following finite step is applied and clipped (against numpy)."""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import engine as E, trainer_math as TM
    from oracle import denoiser_oracle as O
    cfg = O.OracleConfig(size=32, pixel_size=64, max_size=128, octaves=3, batch_size=4, warm_up=3)
    params = O.init_params(cfg, seed=5)
    x, t_int, eps = O.synthetic_batch(cfg, seed=3)
    eng = g.UNetEngine(g.Topology(cfg.pixel_size, cfg.max_size, cfg.octaves), 2, gpu, steps=cfg.steps, base_lr=cfg.base_lr,
                       warm_up=cfg.warm_up, loss_scaling=True)
    eng.use_plan = False
    eng.set_params(params)
    launches = []
    real = lib().call

    def watched(name, *args):
        launches.append(name)
        real(name, *args)
    monkeypatch.setattr(E, "call", watched)
    monkeypatch.setattr(TM, "call", watched)
    X, T, Ep = torch.tensor(x, dtype=torch.float32, device=gpu), torch.tensor(t_int), torch.tensor(eps, dtype=torch.float32)
    eng.train_step(X, T, Ep, apply=False)                        # first-step gradients (scaled by 2^15) give the threshold
    torch.cuda.synchronize()
    segs = eng._clip_segments()
    thr = thresholds(K.scaled(eng.arena.g.cpu().numpy(), 1.0, 2.0 ** -15), segs)[GLOBAL]
    eng.set_clipping(global_clipnorm=thr)
    eng.apply_adam(); eng.finish_step()                          # (no check_finite: the reduction sets the flag)
    torch.cuda.synchronize()
    assert eng.iterations == 1 and eng.loss_scale() == (2.0 ** 15, 1)
    st1 = arenas_of(eng)
    lib().call("gct2_loss_scale_init", eng.ls_state.data_ptr(), 2.0 ** 28, stream())
    eng.iterations = 1
    del launches[:]
    eng.train_step(X, T, Ep)                                     # the whole step, as Trainer runs it
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(eng.arena.g).all())           # the overflow reached the gradient arena by itself
    assert "gct2_grad_sumsq" in launches and "gct2_adam_keras_clipped" in launches and "gct2_scale_check_finite" not in launches
    st2 = arenas_of(eng)
    assert all(torch.equal(st2[n], st1[n]) for n in st1)
    assert eng.iterations == 1 and eng.loss_scale() == (2.0 ** 27, 0)
    # the next step at a scale that fits: applied, and clipped
    lib().call("gct2_loss_scale_init", eng.ls_state.data_ptr(), 2.0 ** 15, stream())
    eng.iterations = 1
    del launches[:]
    eng.train_step(X, T, Ep)
    torch.cuda.synchronize()
    assert "gct2_scale_check_finite" not in launches and launches.count("gct2_grad_sumsq") == 1
    assert eng.iterations == 2 and eng.loss_scale() == (2.0 ** 15, 1)
    gr = eng.arena.g.cpu().numpy()
    assert np.isfinite(gr).all() and clipped_fraction(K.scaled(gr, 1.0, 2.0 ** -15), segs, GLOBAL, thr) == 1.0
    alpha = float(eng.ls_state.view(torch.float32)[5].item())    # the device's alpha of that step (gct2_loss_scale_begin)
    g2 = K.clip_arena(gr, segs, GLOBAL, thr, inv_scale=2.0 ** -15)
    p, m, v = K.adam(st1["p"].cpu().numpy(), st1["m"].cpu().numpy(), st1["v"].cpu().numpy(), g2, alpha, eng.beta_1, eng.beta_2, eng.epsilon)
    st3 = arenas_of(eng)
    assert same(st3["p"], p) and same(st3["m"], m) and same(st3["v"], v)
    assert torch.equal(st3["shadow"].view(torch.int16), cast(2, st3["p"]).view(torch.int16))


# ---- 5. the variant engine ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [GLOBAL, NORM], ids=["global_clipnorm", "clipnorm"])
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_variant_engine_clips(gpu, dt, mode):
    """block_depth = 1 at the smallest widths: one step against numpy on the engine's own gradients"""
    from gan_class_transfer2_amd.variants import VariantEngine
    rng = np.random.default_rng(9)
    eng = VariantEngine(8, 16, 2, 1, False, True, dt, gpu, base_lr=1e-2, warm_up=0, seed=4)
    x = torch.tensor(rng.uniform(-1, 1, (2, 16, 16, 3)), dtype=torch.float32, device=gpu)
    N = eng.net
    eng.train_step(x, apply=False)
    torch.cuda.synchronize()
    segs = eng._clip_segments()
    assert len(segs) == len(N.specs) and [b for b, _ in segs] == sorted(N.offsets.values())
    g = N.g.cpu().numpy()
    thr = thresholds(g, segs)[mode]
    assert clipped_fraction(g, segs, mode, thr) > 0
    before = [t.cpu().numpy() for t in (N.p, N.m, N.v)]
    assert eng._clip_table is None
    eng.set_clipping(**{MODE_KW[mode]: thr})
    eng.apply_adam()
    torch.cuda.synchronize()
    assert eng.iterations == 1 and eng._clip_table is not None and eng._clip_table[1] == len(segs)
    want = K.adam(*before, K.clip_arena(g, segs, mode, thr), eng.adam_alpha(0), eng.beta_1, eng.beta_2, eng.epsilon)
    if mode == NORM:
        mask = np.zeros(g.size, dtype=bool)
        for b, c in segs:
            mask[b:b + c] = True
        want = [np.where(mask, new, old) for new, old in zip(want, before)]
    assert same(N.p, want[0]) and same(N.m, want[1]) and same(N.v, want[2])
    assert not same(N.m, K.adam(*before, g, eng.adam_alpha(0), eng.beta_1, eng.beta_2, eng.epsilon)[1])     # clipping is visible
    if dt:
        assert torch.equal(N.op.view(torch.int16), cast(dt, N.p).view(torch.int16))
    with pytest.raises(ValueError, match="at most one"):
        eng.set_clipping(clipnorm=1.0, clipvalue=1.0)


# ---- 6. what is refused ----------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from gan_class_transfer2_amd.distributed import DataParallelStep, ShardedDataParallelStep
    for Wrapper in (DataParallelStep, ShardedDataParallelStep):
        for kw in (dict(clipnorm=1.0), dict(global_clipnorm=1.0), dict(clipvalue=1.0)):
            eng = make_engine(gpu, 1)
            eng.set_clipping(**kw)
            hooks = (eng.grad_ready_hook, eng.post_backward)
            with pytest.raises(ValueError, match=Wrapper.__name__):
                Wrapper(eng)
            assert (eng.grad_ready_hook, eng.post_backward) == hooks and not hasattr(eng, "_clip_forbidden")    # refused before it touched the engine
        plain = make_engine(gpu, 1)
        Wrapper(plain)
        for kw in (dict(clipnorm=1.0), dict(global_clipnorm=1.0), dict(clipvalue=1.0)):
            with pytest.raises(ValueError, match=Wrapper.__name__):
                plain.set_clipping(**kw)
        plain.set_clipping()
        assert plain.clip_mode == NONE
    eng = make_engine(gpu, 1)
    lo, hi = eng.arena.layer_ranges["U1"]
    for kw in (dict(clipnorm=1.0), dict(global_clipnorm=1.0)):
        eng.set_clipping(**kw)
        before = arenas_of(eng)
        with pytest.raises(ValueError, match="norm"):
            eng.apply_adam(lo, hi)
        after = arenas_of(eng)
        assert all(torch.equal(after[n], before[n]) for n in before) and eng._clip_table is None
