"""The training losses of Trainer.call besides the plain MSE (train.py:254-280) on the GPU: gct2_loss_fwd_bwd per element and bit for
bit on exact-sum inputs, against the float64 restatement of tests/loss_cases.py on real values, its MSE kind against
gct2_mse_fwd_bwd, the loss-only call, the loss scale, two streams, and both engines with the `training_loss` switch - eager, planned
and changed between steps.

Every buffer of the kernel-level tests carries guard zones: NaN in front of and behind what a kernel may read (pred, target, basis),
sentinels around what it may write (dpred, loss, and a scratch of exactly the size gct2_loss_scratch reports, whose inside starts as
NaN: a kernel that read scratch it had not written would leak it).  PARITY UNPINNED w.r.t. TensorFlow (there is none here)."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import loss_cases as K

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, 12345.0
NEW = ("gct2_loss_fwd_bwd", "gct2_loss_scratch")
EXACT = [("dct", (2, 4, 4, 3)), ("dct", (2, 20, 20, 3)), ("dct", (2, 48, 48, 3)), ("dct", (2, 144, 144, 3)),
         ("mse_pooled", (2, 16, 32, 3)), ("mse_pooled", (3, 48, 16, 3)), ("l1", (3, 5, 7, 3)), ("l1", (1, 1, 100003, 1)),
         ("mse", (3, 5, 7, 3)), ("mse", (1, 1, 100003, 1))]
REAL = [("l1", (2, 20, 20, 3)), ("l1", (2, 256, 256, 3)), ("mse_pooled", (2, 16, 32, 3)), ("mse_pooled", (3, 48, 16, 3)),
        ("dct", (2, 20, 20, 3)), ("dct", (2, 48, 48, 3)), ("dct", (2, 128, 128, 3)), ("dct", (2, 256, 256, 3))]
SMALL = [("mse", (1, 1, 100003, 1)), ("l1", (3, 5, 7, 3)), ("mse_pooled", (2, 16, 32, 3)), ("dct", (2, 20, 20, 3)), ("dct", (2, 144, 144, 3))]
ident = lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}"


@pytest.fixture(autouse=True)
def _collect_engines():
    """engines hold reference cycles (and step plans); collect them here, not inside a later test's graph capture"""
    yield
    gc.collect()
    torch.cuda.synchronize()


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """a flat float32 device buffer [GUARD + shift | n | GUARD]: `inner` is what the kernel gets (shift: floats by which it misses a
    16-byte boundary), the guards must keep their fill"""

    def __init__(self, gpu, n, fill, values=None, shift=0):
        self.n, self.fill, self.lo = n, fill, GUARD + shift
        self.full = torch.full((n + 2 * GUARD + shift,), fill, dtype=torch.float32, device=gpu)
        self.inner = self.full[self.lo:self.lo + n]
        if values is not None:
            self.inner.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32).ravel()))
        self.before = self.full.clone()

    def ptr(self):
        return self.inner.data_ptr()

    def guards_intact(self):
        g = torch.cat([self.full[:self.lo], self.full[self.lo + self.n:]])
        return bool(torch.isnan(g).all()) if np.isnan(self.fill) else bool((g == self.fill).all())

    def unchanged(self):
        return torch.equal(self.full.view(torch.int32), self.before.view(torch.int32))


class Case:
    """one kind and shape on the device: guarded inputs, outputs and scratch; run() launches, checks every guard and returns
    (loss float32, dpred float32 array or None).  shift: pred, target and dpred start that many floats behind a 16-byte boundary (basis
    and scratch have to keep theirs: include/gct2.h)"""

    def __init__(self, gpu, kind, pred, target, G=None, shift=0):
        self.gpu, self.kind, self.shape = gpu, K.KINDS[kind], pred.shape
        n = pred.size
        self.pred, self.target = Guarded(gpu, n, np.nan, pred, shift), Guarded(gpu, n, np.nan, target, shift)
        self.basis = Guarded(gpu, G.size, np.nan, G) if G is not None else None
        need = ctypes.c_size_t(0)
        lib().check(lib().load().gct2_loss_scratch(self.kind, *self.shape, ctypes.byref(need)), "gct2_loss_scratch")
        self.need = need.value
        self.dpred, self.loss, self.scratch = Guarded(gpu, n, SENTINEL, shift=shift), Guarded(gpu, 1, SENTINEL), Guarded(gpu, self.need, SENTINEL)

    def run(self, scale=None, grad=True, s=None, entry="gct2_loss_fwd_bwd"):
        self.dpred.full.fill_(SENTINEL); self.loss.full.fill_(SENTINEL)
        self.scratch.inner.fill_(float("nan"))
        ls = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=self.gpu)
        s = stream() if s is None else s
        torch.cuda.synchronize()                                            # (the fills above ran on the current stream)
        if entry == "gct2_mse_fwd_bwd":
            lib().call(entry, self.pred.ptr(), self.target.ptr(), self.dpred.ptr(), self.loss.ptr(), self.scratch.ptr(), self.pred.n,
                       None if ls is None else ls.data_ptr(), s)
        else:
            lib().call(entry, self.kind, self.pred.ptr(), self.target.ptr(), self.dpred.ptr() if grad else None, self.loss.ptr(),
                       self.scratch.ptr(), self.need, *self.shape, self.basis.ptr() if self.basis else None,
                       None if ls is None else ls.data_ptr(), s)
        torch.cuda.synchronize()
        assert self.pred.unchanged() and self.target.unchanged() and (self.basis is None or self.basis.unchanged())
        assert self.dpred.guards_intact() and self.loss.guards_intact() and self.scratch.guards_intact()
        loss = self.loss.inner.cpu().numpy()[0]
        if not grad:
            assert bool((self.dpred.inner == SENTINEL).all())               # dpred = NULL: nothing but loss and scratch is written
            return loss, None
        dpred = self.dpred.inner.cpu().numpy().reshape(self.shape)
        assert not np.isnan(loss) and not np.isnan(dpred).any()             # no NaN leaked from a guard or from unwritten scratch
        return loss, dpred


def bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def exact_inputs(kind, shape, seed=7):
    rng = np.random.default_rng(seed)
    pred, target = K.exact_pair(rng, shape)
    G = None
    if kind == "dct":
        G = K.signed_permutation_basis(rng, shape[1])
        K.assert_exact_bound(G)                                             # |E| <= 64, |V| <= 4096: every partial sum is exact
    return pred, target, G


def real_inputs(kind, shape, seed=11):
    import gan_class_transfer2_amd as g
    rng = np.random.default_rng(seed)
    pred, target = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    return pred, target, (g.trainer_math.dct_basis(shape[1]) if kind == "dct" else None)


@pytest.fixture(scope="module")
def small_cases(gpu):
    """exact-sum cases shared by tests 3-6: (Case, restatement) by id; built once, inputs never change"""
    out = {}
    for c in SMALL:
        pred, target, G = exact_inputs(*c)
        out[ident(c)] = (Case(gpu, c[0], pred, target, G), K.restate(K.KINDS[c[0]], pred, target, G))
    return out


# ---- 1. per element, exact sums --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=ident)
def test_exact_inputs_bit_for_bit(gpu, case):
    kind, shape = case
    pred, target, G = exact_inputs(kind, shape)
    want = K.restate(K.KINDS[kind], pred, target, G)
    if kind == "dct":
        E, V = K.dct_planes(K.residual(pred, target), G)
        assert np.abs(E).max() <= 64 and np.abs(V).max() <= 4096
    loss, dpred = Case(gpu, kind, pred, target, G).run()
    assert np.array_equal(dpred, want["dpred_bits"]), np.abs(dpred - want["dpred_bits"]).max()      # (+0 == -0)
    assert np.abs(want["dpred_bits"]).max() > 0
    if kind != "dct" or shape[1] <= 20:                                     # the sum is below 2^24
        assert want["loss"] * pred.size < 2 ** 24
        assert bits(loss) == bits(want["loss_bits"]), (loss, want["loss_bits"])
    else:
        assert abs(float(loss) - want["loss"]) <= 1e-6 * want["loss"], (loss, want["loss"])


@pytest.mark.parametrize("case", [("l1", (3, 5, 7, 3)), ("mse_pooled", (2, 16, 32, 3)), ("dct", (2, 20, 20, 3))], ids=ident)
def test_operands_off_the_16_byte_grid_give_the_same_bits(gpu, case):
    """pred, target and dpred 4, 8 and 12 bytes behind a 16-byte boundary (the header asks 4 bytes of them): the kernels read and
    write them element by element instead of in 16-byte groups (loss_kernels.hip: `vec`, the DCT's `xvec`) - the restatement's bits
    like the aligned call, with a loss scale as well"""
    kind, shape = case
    pred, target, G = exact_inputs(kind, shape)
    want = K.restate(K.KINDS[kind], pred, target, G)
    aligned = Case(gpu, kind, pred, target, G)
    assert aligned.pred.ptr() % 16 == 0 and aligned.target.ptr() % 16 == 0 and aligned.dpred.ptr() % 16 == 0
    base_loss, base = aligned.run(1024.0)
    for shift in (1, 2, 3):
        c = Case(gpu, kind, pred, target, G, shift=shift)
        assert c.pred.ptr() % 16 == 4 * shift and c.dpred.ptr() % 16 == 4 * shift and c.scratch.ptr() % 16 == 0
        loss, dpred = c.run()
        assert np.array_equal(dpred, want["dpred_bits"]) and bits(loss) == bits(want["loss_bits"]), shift
        loss, dpred = c.run(1024.0)
        assert np.array_equal(bits(dpred), bits(base)) and bits(loss) == bits(base_loss), shift


# ---- 2. real values --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REAL, ids=ident)
def test_real_values_against_float64(gpu, case, parity_log):
    kind, shape = case
    pred, target, G = real_inputs(kind, shape)
    want = K.restate(K.KINDS[kind], pred, target, G)
    loss, dpred = Case(gpu, kind, pred, target, G).run()
    loss_err = abs(float(loss) - want["loss"]) / want["loss"]
    if kind != "dct":
        err = K.rel_l2(dpred, want["dpred"])
        print(f"{ident(case)}: loss {loss_err:.3g} rel_l2(dpred) {err:.3g}")
        parity_log("losses_" + ident(case), loss_rel=loss_err, dpred_rel_l2=err)
        assert loss_err <= 1e-6 and err <= 1e-6, (loss_err, err)
        return
    # the DCT bound is measured: the same four products in numpy float32 from the fp32 basis, against float64
    e32_dpred, e32_loss = K.fp32_dct_error(pred, target, G, want)
    err = K.max_rel(dpred, want["dpred"])
    print(f"{ident(case)}: dpred {err:.3g} (e32 {e32_dpred:.3g}) loss {loss_err:.3g} (e32 {e32_loss:.3g})")
    parity_log("losses_" + ident(case), dpred_max_rel=err, e32_dpred=e32_dpred, loss_rel=loss_err, e32_loss=e32_loss)
    assert err <= max(1e-6, 4 * e32_dpred), (err, e32_dpred)
    assert loss_err <= max(1e-6, 4 * e32_loss), (loss_err, e32_loss)


# ---- 3. the MSE kind is gct2_mse_fwd_bwd -----------------------------------------------------------------------------------------------
def test_mse_kind_equals_mse_fwd_bwd(gpu, small_cases):
    c, want = small_cases["mse-1x1x100003x1"]
    for scale in (None, 2.0 ** 15):
        la, da = c.run(scale)
        lb, db = c.run(scale, entry="gct2_mse_fwd_bwd")
        assert bits(la) == bits(lb) and np.array_equal(bits(da), bits(db))
    assert bits(la) == bits(want["loss_bits"])


# ---- 4. dpred = NULL -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [ident(c) for c in SMALL])
def test_loss_only_call(gpu, small_cases, name):
    c, _ = small_cases[name]
    loss, _ = c.run()
    only, none = c.run(grad=False)
    assert none is None and bits(only) == bits(loss)


# ---- 5. loss scale ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [ident(c) for c in SMALL])
def test_loss_scale_multiplies_the_gradient_only(gpu, small_cases, name):
    c, want = small_cases[name]
    loss, dpred = c.run()
    loss_s, dpred_s = c.run(2.0 ** 15)
    assert bits(loss_s) == bits(loss)
    assert np.array_equal(dpred_s, dpred * np.float32(2.0 ** 15)) and np.abs(dpred).max() > 0


# ---- 6. two streams --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [ident(c) for c in SMALL])
def test_two_streams_same_bits(gpu, small_cases, name):
    c, _ = small_cases[name]
    loss, dpred = c.run()
    other = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    loss2, dpred2 = c.run(s=other.cuda_stream)
    assert bits(loss) == bits(loss2) and np.array_equal(bits(dpred), bits(dpred2))


def test_real_values_same_bits_run_to_run(gpu):
    """no floating-point atomics: the bits depend on the inputs alone (real values, more than one work-group per sum)"""
    for kind, shape in (("l1", (2, 48, 48, 3)), ("mse_pooled", (3, 48, 16, 3)), ("dct", (2, 144, 144, 3))):
        c = Case(gpu, kind, *real_inputs(kind, shape))
        a, b = c.run(), c.run()
        assert bits(a[0]) == bits(b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


# ---- 7. the engines --------------------------------------------------------------------------------------------------------------------
B, SIZE = 2, 32
TOPO = dict(pixel_size=8, max_size=16, octaves=2)
KINDS = ("mse", "l1", "mse_pooled", "dct")


def make_engine(gpu, dtype, **kw):
    import gan_class_transfer2_amd as g
    return g.UNetEngine(g.Topology(TOPO["pixel_size"], TOPO["max_size"], TOPO["octaves"]), dtype, gpu, steps=50, seed=4, rng_seed=5, **kw)


def batch(gpu, seed=0):
    rng = np.random.default_rng(seed)
    x = torch.tensor(rng.uniform(-1, 1, (B, SIZE, SIZE, 3)).astype(np.float32), device=gpu)
    t_int = torch.tensor(rng.integers(1, 51, B).astype(np.int32))
    eps = torch.tensor(rng.standard_normal((B, SIZE, SIZE, 3)).astype(np.float32))
    return x, t_int, eps


def check_against_restatement(kind, pred, target, loss, dpred, weights=None, tag=None, parity_log=None):
    """the bounds of test 2, on the engine's own prediction"""
    import gan_class_transfer2_amd as g
    G = g.trainer_math.dct_basis(SIZE) if kind == "dct" else None
    want = K.restate(K.KINDS[kind], pred, target, G)
    wd = want["dpred"] if weights is None else want["dpred"] * weights[:, None, None, None]
    loss_err = abs(float(loss) - want["loss"]) / want["loss"]
    if kind == "dct":
        e32_dpred, e32_loss = K.fp32_dct_error(pred, target, G, want)
        err = K.max_rel(dpred, wd)
        assert err <= max(1e-6, 4 * e32_dpred) and loss_err <= max(1e-6, 4 * e32_loss), (kind, err, e32_dpred, loss_err, e32_loss)
    else:
        err = K.rel_l2(dpred, wd)
        assert err <= 1e-6 and loss_err <= 1e-6, (kind, err, loss_err)
    if parity_log is not None:
        parity_log(tag, loss_rel=loss_err, dpred_err=err)


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
def test_engine_loss_and_gradient_by_kind(gpu, dtype, parity_log):
    """b.loss and b.dpred against the restatement applied to the engine's own b.pred and the target, one engine, the kind changed
    between steps"""
    eng = make_engine(gpu, dtype)
    x, t_int, eps = batch(gpu)
    b = eng.buffers(B, SIZE, SIZE)
    seen = {}
    for kind in KINDS + ("mse",):
        eng.training_loss = kind
        loss = eng.train_step(x, t_int, eps, apply=False)
        torch.cuda.synchronize()
        pred = b.pred.cpu().numpy()
        check_against_restatement(kind, pred, x.cpu().numpy(), loss[0], b.dpred.cpu().numpy(), tag=f"losses_engine_{kind}_{('fp32', 'bf16')[dtype]}",
                                  parity_log=parity_log)
        seen.setdefault(kind, []).append((float(loss[0]), b.dpred.cpu().numpy()))
    assert len({v[0][0] for v in seen.values()}) == 4                       # four different losses ...
    assert seen["mse"][0][0] == seen["mse"][1][0] and np.array_equal(seen["mse"][0][1], seen["mse"][1][1])     # ... and back
    assert len(b.loss_store) == 3                                            # scratch per non-default kind, allocated once


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


def arenas_of(eng):
    A = eng.arena
    torch.cuda.synchronize()
    return {n: getattr(A, n).clone() for n in ("p", "m", "v") + (("shadow",) if A.shadow is not None else ())}


def as_bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def lockstep(E, P, x, step_e, step_p, tag):
    """one step of two engines from the SAME arenas (P's are overwritten with E's first): what must be equal bit for bit, is.
    At this topology and size the weight and bias gradients of the narrow layers and of Dense(3) are sums of float atomics (direct
    kernels, gct2_dense_bwd): two runs of ONE engine on the same inputs differ in their last bits (tests/test_optimizers_gpu.py
    own_gradients), whoever steps - so the gradients are read from each engine's own arena (fuse_adam = False) and the optimizer
    state is compared element by element: the forward pass and the loss kernels have no atomics, hence EQUAL losses; equal RNG
    positions and counters; and wherever the two gradients are equal - Adam is elementwise - p, m, v and the shadow are EQUAL.
    Returns the share of elements with equal gradients."""
    for n, t in arenas_of(E).items():
        getattr(P.arena, n).copy_(t)
    le, lp = step_e(x).clone(), step_p(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(as_bits(le), as_bits(lp)) and bool(torch.isfinite(le).all()), (tag, le, lp)
    assert (E.iterations, E.rng_offset_t, E.rng_offset_eps) == (P.iterations, P.rng_offset_t, P.rng_offset_eps), tag
    assert E._grads_in_arena and P._grads_in_arena
    same = as_bits(E.arena.g) == as_bits(P.arena.g)
    a, b = arenas_of(E), arenas_of(P)
    for n in a:
        assert torch.equal(as_bits(a[n])[same], as_bits(b[n])[same]), (tag, n)
    return float(same.float().mean())


def plan_names(eng, recorded):
    """{kind: [entry-point names]} of the step plans an engine holds"""
    out = {}
    for key, sp in eng._plans.items():
        kind = [k for k in key if isinstance(k, str) and k in KINDS][-1]
        out.setdefault(kind, []).append(recorded(sp.plan))
    return out


@pytest.mark.parametrize("mode", ["bf16", "fp32", "f16_loss_scaled"])
def test_planned_step_equals_eager_step_bit_for_bit(gpu, mode, recorded):
    """a train step replayed from its recorded call list against the same step run call by call, with the kind changed between steps
    (every kind gets a plan of its own: the kind is part of the key).  The method of test_step_gpu's test of this name with the
    provision tests/test_optimizers_gpu.py::test_planned_steps_equal_eager_steps makes for the tiny network (lockstep): E steps
    eagerly, P under step plans, from the same arenas."""
    dtype = dict(bf16=1, fp32=0, f16_loss_scaled=2)[mode]
    xs = [batch(gpu, seed=k)[0] for k in range(3)]
    sequence = ["mse"] * 3 + ["dct"] * 3 + ["l1"] * 3 + ["mse_pooled"] * 3 + ["mse"] * 2 + ["dct"] * 2
    E, P = (make_engine(gpu, dtype, loss_scaling=(mode == "f16_loss_scaled")) for _ in range(2))
    E.use_plan, P.use_plan, E.fuse_adam, P.fuse_adam = False, True, False, False
    shares = []
    for k, kind in enumerate(sequence):
        E.training_loss = P.training_loss = kind
        shares.append(lockstep(E, P, xs[k % 3], E.train_step, P.train_step, (k, kind)))
    print(f"{mode}: share of elements with equal gradients per step: {' '.join('%.3f' % u for u in shares)}")
    assert min(shares) > 0.5                                                 # (the comparison covers most of every arena)
    assert not E._plans
    names = plan_names(P, recorded)
    assert set(names) == set(KINDS)                                          # a new kind is a new plan key
    for kind, plans in names.items():
        for calls in plans:
            assert len(calls) > 10
            if kind == "mse":                                                # the default call list names no new symbol
                assert not set(calls) & set(NEW) and calls.count("gct2_mse_fwd_bwd") == 1
            else:
                assert calls.count("gct2_loss_fwd_bwd") == 1 and "gct2_mse_fwd_bwd" not in calls


def test_default_kind_is_what_an_engine_built_before_the_global_was_touched_computes(gpu, recorded):
    """with training_loss = "mse" an engine driven through Trainer - the module global set to another kind and back in between - and an
    engine that never heard of the switch: the same recorded call lists, and (lockstep) the same bits for three steps"""
    import gan_class_transfer2_amd as g
    M = g.model
    xs = [batch(gpu, seed=k)[0] for k in range(3)]
    ref, eng = make_engine(gpu, 1), make_engine(gpu, 1)
    assert "training_loss" not in ref.__dict__                               # the class default: nothing was written
    ref.fuse_adam = eng.fuse_adam = False
    tr = M.Trainer(type("Den", (), dict(engine=eng, ensure_engine=lambda self, **kw: eng, variant=lambda self: False))())
    try:
        M.configure(training_loss="dct")
        assert tr._engine().training_loss == "dct"
        M.configure(training_loss="mse")
        for k, x in enumerate(xs):
            assert lockstep(ref, eng, x, ref.train_step, lambda x: tr.train_step((x, x))["loss"], k) > 0.5
    finally:
        M.configure(training_loss="mse")
    a, b = plan_names(ref, recorded), plan_names(eng, recorded)
    assert set(a) == set(b) == {"mse"} and a == b and not set(sum(b["mse"], [])) & set(NEW)
    assert all(not bufs.loss_store for bufs in eng._bufs.values())           # a default engine allocates nothing new


def test_trainer_call_passes_no_gradient_buffer(gpu, monkeypatch):
    """Trainer.call (no gradients) with a non-default kind: dpred = NULL, and the loss is the restatement's"""
    import gan_class_transfer2_amd as g
    M = g.model
    eng = make_engine(gpu, 0)
    tr = M.Trainer(type("Den", (), dict(engine=eng, ensure_engine=lambda self, **kw: eng, variant=lambda self: False))())
    x = batch(gpu)[0]
    seen = []
    orig = g._lib.call
    spy = lambda name, *a: (seen.append((name, a)), orig(name, *a))[1]
    monkeypatch.setattr(g.trainer_math, "call", spy)
    try:
        M.configure(training_loss="dct")
        b = eng.buffers(B, SIZE, SIZE)
        b.dpred.fill_(SENTINEL)
        loss = tr.call(x)
        torch.cuda.synchronize()
    finally:
        M.configure(training_loss="mse")
    (name, a), = [s for s in seen if s[0] == "gct2_loss_fwd_bwd"]
    assert a[3] is None and bool((b.dpred == SENTINEL).all())
    want = K.dct(b.pred.cpu().numpy(), x.cpu().numpy(), g.trainer_math.dct_basis(SIZE))
    assert abs(float(loss) - want["loss"]) <= 1e-5 * want["loss"]


def test_prediction_weighting_composes_with_the_dct_loss(gpu):
    eng = make_engine(gpu, 0, predict_x=False, prediction_weighting=True)
    eng.training_loss = "dct"
    x, t_int, eps = batch(gpu)
    loss = eng.train_step(x, t_int, eps, apply=False)
    torch.cuda.synchronize()
    b = eng.buffers(B, SIZE, SIZE)
    w = eng.objective_coefficients(t_int.to(gpu))[2].cpu().numpy().astype(np.float64)
    assert w.min() > 0 and w.max() < 1 and b.target is not None
    # the engine keeps the WEIGHTED prediction (train.py:252 reassigns `prediction`); dpred = w_b * dloss/d(w_b pred)
    check_against_restatement("dct", b.pred.cpu().numpy(), b.target.cpu().numpy(), loss[0], b.dpred.cpu().numpy(), weights=w)


def test_variant_engine_takes_the_same_switch(gpu):
    """block_depth = 1 (train.py:20): VariantEngine.train_step dispatches on the kind as UNetEngine does"""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.variants import VariantEngine
    eng = VariantEngine(TOPO["pixel_size"], TOPO["max_size"], TOPO["octaves"], 1, False, True, 0, gpu, steps=50, seed=4)
    x, t_int, eps = batch(gpu)
    losses = {}
    for kind in ("mse", "dct", "mse_pooled"):
        eng.training_loss = kind
        loss = eng.train_step(x, t_int, eps, apply=False)
        torch.cuda.synchronize()
        want = K.restate(K.KINDS[kind], eng.last["pred"].cpu().numpy(), x.cpu().numpy(), g.trainer_math.dct_basis(SIZE) if kind == "dct" else None)
        assert abs(float(loss[0]) - want["loss"]) <= 1e-5 * want["loss"], kind
        # Dense(3)'s bias gradient is the column sum of dpred
        db = eng.get_grads()["dense.b"].astype(np.float64)
        ref = want["dpred"].sum(axis=(0, 1, 2))
        assert np.abs(db - ref).max() <= 1e-5 * np.abs(want["dpred"]).sum(axis=(0, 1, 2)).max(), kind
        losses[kind] = float(loss[0])
    assert len(set(losses.values())) == 3 and len(eng._loss_store) == 2
    eng.training_loss = "l1"
    only = eng.train_step(x, t_int, eps, backward=False)                     # Trainer.call: the loss-only form
    torch.cuda.synchronize()
    want = K.l1(eng.last["pred"].cpu().numpy(), x.cpu().numpy())
    assert abs(float(only[0]) - want["loss"]) <= 1e-6 * want["loss"]
