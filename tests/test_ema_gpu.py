"""The exponential moving average of the parameters (Keras Adam(use_ema=True, ema_momentum=...) [TF]) on the GPU: gct2_ema_update per
element and bit for bit, the recurrence through real train steps (deferred optimizer launches, step plans, loss scaling, the
data-parallel wrapper, the variant engine), and everything that reads through the averages (predict, the sampler, checkpoints,
finalize_variable_values).

The reference of every bit-exact check is the recurrence itself in float32 numpy - two products and one sum, each rounded once:
    ema_k = fl(fl(fl32(m) * ema_{k-1}) + fl(fl32(1 - m) * p_k)),   ema_0 = p_0
PARITY UNPINNED w.r.t. TensorFlow (there is none here): the formula and the initial value are Keras' documented ones.
"""
import socket
import types

import numpy as np
import pytest
import torch

from oracle import denoiser_oracle as O

pytestmark = pytest.mark.gpu
TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def coef(momentum):
    """the two float32 factors the host hands to the kernel: 1 - momentum formed in double, rounded once"""
    return np.float32(momentum), np.float32(1.0 - momentum)


def ema_ref(ema, p, momentum):
    """the recurrence, three numpy lines: float32 arrays in, float32 array out, every operation rounded to float32"""
    m, c = coef(momentum)
    a, b = m * ema, c * p
    return a + b


def host_recurrence(ps, momenta):
    """ema over the parameter iterates p_0 .. p_K (device tensors), ema_0 = p_0; momenta[k - 1] is the momentum of step k"""
    ema = ps[0].cpu().numpy()
    for p, m in zip(ps[1:], momenta):
        ema = ema_ref(ema, p.cpu().numpy(), m)
    return torch.from_numpy(ema)


def cast(dt, src):
    """what gct2_cast_from_f32 writes from an fp32 device tensor: the project's one round-to-nearest-even conversion"""
    out = torch.empty(src.numel(), dtype=TDT[dt], device=src.device)
    lib().call("gct2_cast_from_f32", dt, src.data_ptr(), out.data_ptr(), src.numel(), stream())
    return out


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


def make_engine(cfg, dtype, gpu, **kw):
    import gan_class_transfer2_amd as g
    return g.UNetEngine(g.Topology(cfg.pixel_size, cfg.max_size, cfg.octaves), dtype, gpu, steps=cfg.steps, base_lr=cfg.base_lr,
                        warm_up=cfg.warm_up, **kw)


# ---- 1. the kernel, per element and bit for bit ------------------------------------------------------------------------------
SENTINEL = 12345.0
SIZES = (1, 3, 4, 5, 1022, 65543)       # scalar tail only, one vector, vector + tail, more than one block
PAD = 64


def _run_ema(gpu, dt, n, off, ema, p, momentum, ls=None):
    """one gct2_ema_update over [off, off + n) of buffers with PAD sentinel elements behind the range; returns the buffers"""
    total = off + n + PAD
    eb = torch.full((total,), SENTINEL, dtype=torch.float32, device=gpu)
    pb = torch.full((total,), -SENTINEL, dtype=torch.float32, device=gpu)
    eb[off:off + n] = torch.from_numpy(ema).to(gpu)
    pb[off:off + n] = torch.from_numpy(p).to(gpu)
    sb = torch.full((total,), 77.0, dtype=TDT[dt], device=gpu) if dt else None
    p_before = pb.clone()
    m, c = coef(momentum)
    lib().call("gct2_ema_update", eb.data_ptr() + 4 * off, pb.data_ptr() + 4 * off, sb.data_ptr() + 2 * off if dt else None, dt, n,
               float(m), float(c), ls, stream())
    torch.cuda.synchronize()
    assert torch.equal(pb, p_before)                                   # p is read only
    return eb, sb


def _check_outside(eb, sb, off, n):
    assert bool((eb[:off] == SENTINEL).all()) and bool((eb[off + n:] == SENTINEL).all())
    if sb is not None:
        assert bool((sb[:off].float() == 77.0).all()) and bool((sb[off + n:].float() == 77.0).all())


@pytest.mark.parametrize("momentum", [0.0, 0.99, 1.0])
@pytest.mark.parametrize("dt", [0, 1, 2], ids=["noshadow", "bf16", "f16"])
def test_ema_update_per_element(gpu, dt, momentum):
    rng = np.random.default_rng(100 * dt + int(momentum * 100))
    for n in SIZES:
        for off in (0, 64):
            for k in (-8, 0, 8):
                ema = (rng.standard_normal(n) * 2.0 ** k).astype(np.float32)
                p = (rng.standard_normal(n) * 2.0 ** k).astype(np.float32)
                eb, sb = _run_ema(gpu, dt, n, off, ema, p, momentum)
                want = torch.from_numpy(ema_ref(ema, p, momentum)).to(gpu)
                assert torch.equal(eb[off:off + n], want), (n, off, k)
                if dt:
                    assert torch.equal(sb[off:off + n], cast(dt, eb[off:off + n].contiguous())), (n, off, k)
                _check_outside(eb, sb, off, n)


def test_ema_update_fp16_shadow_overflows_to_inf(gpu):
    n = 1022
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    ema = (1e5 * sign).astype(np.float32)
    eb, sb = _run_ema(gpu, 2, n, 64, ema, ema.copy(), 0.99)
    assert torch.equal(eb[64:64 + n], torch.from_numpy(ema_ref(ema, ema, 0.99)).to(gpu))
    assert bool(torch.isinf(sb[64:64 + n]).all()) and torch.equal(torch.sign(sb[64:64 + n].float()), torch.from_numpy(sign).to(gpu))
    assert torch.equal(sb[64:64 + n], cast(2, eb[64:64 + n].contiguous()))
    _check_outside(eb, sb, 64, n)


# ---- 2. the loss-scale gate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("found_inf", [1, 0])
def test_ema_update_is_gated_by_found_inf(gpu, found_inf):
    state = torch.zeros(8, dtype=torch.int32, device=gpu)
    lib().call("gct2_loss_scale_init", state.data_ptr(), 2.0 ** 15, stream())
    state[3] = found_inf                                               # gct2_loss_scale_state.found_inf
    rng = np.random.default_rng(7)
    for n in (5, 65543):
        ema, p = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        eb, sb = _run_ema(gpu, 1, n, 64, ema, p, 0.99, ls=state.data_ptr())
        if found_inf:
            assert torch.equal(eb[64:64 + n], torch.from_numpy(ema).to(gpu)) and bool((sb[64:64 + n].float() == 77.0).all())
        else:
            assert torch.equal(eb[64:64 + n], torch.from_numpy(ema_ref(ema, p, 0.99)).to(gpu))
            assert torch.equal(sb[64:64 + n], cast(1, eb[64:64 + n].contiguous()))
        _check_outside(eb, sb, 64, n)


# ---- 3. the recurrence through real steps ----------------------------------------------------------------------------------------
STEP_CFG = dict(size=64, pixel_size=128, max_size=512, octaves=4, batch_size=4)      # the deferral window and slab-fed Adam in use


def _step(eng, x, mode):
    if mode == "apply_false":
        loss = eng.train_step(x, apply=False)
        eng.check_finite(); eng.apply_adam(); eng.finish_step()
        return loss
    return eng.train_step(x)


@pytest.mark.parametrize("use_plan", [False, True], ids=["eager", "plan"])
@pytest.mark.parametrize("mode", ["fused", "apply_false", "serial"])
def test_recurrence_through_real_steps(gpu, mode, use_plan, recorded):
    """engine A averages and is never read between its six steps (its deferred optimizer launches stay deferred: the averages of the
    arena's prefix follow them inside the next forward pass); twin B, same seeds, no averages, hands out p after every step.
    apply_false runs finish_step() - hence the EMA launch - from the caller, outside the recorded step body: its plans hold no
    EMA record; the other two modes' plans must."""
    cfg = O.OracleConfig(**STEP_CFG)
    params = O.init_params(cfg, seed=3)
    xs = [torch.tensor(O.synthetic_batch(cfg, seed=k)[0], dtype=torch.float32, device=gpu) for k in range(3)]
    A, B = make_engine(cfg, 1, gpu, rng_seed=5), make_engine(cfg, 1, gpu, rng_seed=5)
    for e in (A, B):
        e.use_plan, e.overlap = use_plan, mode != "serial"
        e.set_params(params)
    A.enable_ema(0.9)                                                  # ema_0 = p_0: the parameters as they stand now
    assert B._ema is None and B.arena.ema is None                      # nothing allocated while off
    ps = [B.arena.p.clone()]
    for k in range(6):
        _step(A, xs[k % 3], mode)
        _step(B, xs[k % 3], mode)
        ps.append(B.arena.p.clone())
    if mode == "fused":
        assert A._pending and A._pending_ema is not None               # still held back: the read below flushes them
    ema = A.arena.ema
    torch.cuda.synchronize()
    assert torch.equal(ema.cpu(), host_recurrence(ps, [0.9] * 6))
    assert not torch.equal(ema, ps[6])                                 # (the average lags the iterate: the check above is not vacuous)
    assert torch.equal(A.arena.ema_shadow, cast(1, ema))
    for name in ("p", "m", "v", "shadow"):                             # averaging does not disturb training
        assert torch.equal(getattr(A.arena, name), getattr(B.arena, name)), name
    assert A.iterations == B.iterations == 6
    if use_plan:
        assert len(A._plans) >= 1 and len(B._plans) >= 1
        counts = [recorded(sp.plan).count("gct2_ema_update") for sp in A._plans.values()]
        # fused: the step-end launch over [end of the deferred prefix, total) + the prefix behind the held-back Adam launches
        assert all(c == {"fused": 2, "serial": 1, "apply_false": 0}[mode] for c in counts), counts
        assert all(len(recorded(sp.plan)) > 20 and "gct2_ema_update" not in recorded(sp.plan) for sp in B._plans.values())
    else:
        assert not A._plans


# ---- 4. loss scaling: a skipped step leaves the averages alone ------------------------------------------------------------------
def test_skipped_step_leaves_the_averages_alone(gpu):
    """the recipe of test_fp16_overflow_inside_the_reverse_pass_skips_the_step: fp16, one applied step, then the scale re-initialised to
    2^28, at which the scaled fp16 gradients overflow inside the reverse pass"""
    cfg = O.OracleConfig(size=32, pixel_size=64, max_size=128, octaves=3, batch_size=4, warm_up=3)
    params = O.init_params(cfg, seed=5)
    x, t_int, eps = O.synthetic_batch(cfg, seed=3)
    eng = make_engine(cfg, 2, gpu, loss_scaling=True)
    eng.set_params(params)
    eng.enable_ema(0.9)
    p0 = eng.arena.p.clone()
    X, T, Ep = torch.tensor(x, dtype=torch.float32, device=gpu), torch.tensor(t_int), torch.tensor(eps, dtype=torch.float32)
    eng.train_step(X, T, Ep, apply=False)
    eng.check_finite(); eng.apply_adam(); eng.finish_step()
    torch.cuda.synchronize()
    assert eng.iterations == 1
    p1, ema1, sh1 = eng.arena.p.clone(), eng.arena.ema.clone(), eng.arena.ema_shadow.clone()
    assert not torch.equal(p1, p0)
    assert torch.equal(ema1.cpu(), host_recurrence([p0, p1], [0.9])) and torch.equal(sh1, cast(2, ema1))
    lib().call("gct2_loss_scale_init", eng.ls_state.data_ptr(), 2.0 ** 28, stream())
    eng.iterations = 1
    eng.train_step(X, T, Ep, apply=False)
    eng.check_finite(); eng.apply_adam(); eng.finish_step()
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(eng.arena.g).all())                 # the overflow reached the gradient arena by itself
    assert eng.iterations == 1 and eng.loss_scale() == (2.0 ** 27, 0)
    assert torch.equal(eng.arena.p, p1) and torch.equal(eng.arena.ema, ema1) and torch.equal(eng.arena.ema_shadow, sh1)


# ---- 5. a momentum change reaches replayed steps ---------------------------------------------------------------------------------
def test_recompiled_momentum_reaches_replayed_steps(gpu, recorded):
    """Trainer.compile() with another ema_momentum after the plan was recorded: the momentum is baked into recorded arguments, so it
    is part of the plan's key.  The planned engine must equal its eager twin, and both the host recurrence over a reader's iterates
    with the momentum switched at the same step."""
    import gan_class_transfer2_amd as g
    cfg = O.OracleConfig(**STEP_CFG)
    params = O.init_params(cfg, seed=3)
    xs = [torch.tensor(O.synthetic_batch(cfg, seed=k)[0], dtype=torch.float32, device=gpu) for k in range(3)]
    out = []
    for kind in ("reader", "eager", "plan"):
        eng = make_engine(cfg, 1, gpu, rng_seed=5)
        eng.use_plan = kind == "plan"
        eng.set_params(params)
        tr = g.Trainer(types.SimpleNamespace(engine=eng))
        opt = lambda m: g.Adam(g.WarmUp(cfg.base_lr, cfg.warm_up), use_ema=True, ema_momentum=m)
        if kind != "reader":
            tr.compile(opt(0.9), g.identity)
        ps = [eng.arena.p.clone()]
        for k in range(8):
            if k == 4 and kind != "reader":
                tr.compile(opt(0.5), g.identity)
                assert eng.use_ema and eng.ema_momentum == 0.5
            eng.train_step(xs[k % 3])
            if kind == "reader":
                ps.append(eng.arena.p.clone())
        torch.cuda.synchronize()
        if kind == "plan":
            assert len(eng._plans) >= 2                                # one plan per momentum
            assert all("gct2_ema_update" in recorded(sp.plan) for sp in eng._plans.values())
        out.append(ps if kind == "reader" else {n: getattr(eng.arena, n).clone() for n in ("p", "m", "v", "shadow", "ema", "ema_shadow")})
    ps, eager, plan = out
    for n in eager:
        assert torch.equal(eager[n], plan[n]), n
    assert torch.equal(plan["p"], ps[8])
    assert torch.equal(plan["ema"].cpu(), host_recurrence(ps, [0.9] * 4 + [0.5] * 4))


# ---- 6. / 7. reading through the averages ------------------------------------------------------------------------------------------
READ_CASES = {"f32": (0, (8, 16, 2), 16), "bf16": (1, (64, 128, 3), 32)}


@pytest.fixture(scope="module", params=list(READ_CASES))
def averaged(request, gpu):
    """A: three visible steps (lr 1e-2, no warm-up) with averages; C: a fresh engine whose parameters ARE A's averages (set_params
    refreshes its compute-dtype copy with the same cast).  Shared by the read-only tests below."""
    import gan_class_transfer2_amd as g
    dt, topo, size = READ_CASES[request.param]
    rng = np.random.default_rng(11)
    mk = lambda **kw: g.UNetEngine(g.Topology(*topo), dt, gpu, base_lr=1e-2, warm_up=0, seed=21, **kw)
    A = mk(use_ema=True, ema_momentum=0.9)
    assert A.use_ema and A.ema_momentum == 0.9 and torch.equal(A.arena.ema, A.arena.p)
    for k in range(3):
        A.train_step(torch.tensor(rng.uniform(-1, 1, (2, size, size, 3)), dtype=torch.float32, device=gpu))
    C = mk()
    C.set_params({k: A.arena._view(A.arena.ema, k).clone() for k in A.arena.shapes})
    torch.cuda.synchronize()
    assert torch.equal(C.arena.p, A.arena.ema) and not torch.equal(A.arena.p, A.arena.ema)
    if dt:
        assert torch.equal(C.arena.shadow, A.arena.ema_shadow)
    x = torch.tensor(rng.uniform(-1, 1, (2, size, size, 3)), dtype=torch.float32, device=gpu)
    return A, C, x, size


def test_predict_reads_the_averages(averaged, gpu):
    import gan_class_transfer2_amd as g
    A, C, x, size = averaged
    raw = A.predict(x).clone()
    want = C.predict(x).clone()
    assert not torch.equal(raw, want)
    assert torch.equal(A.predict(x, use_ema=True), want)
    assert torch.equal(A.predict(x), raw)                              # no swap leaked
    with pytest.raises(RuntimeError, match="inside"):
        with A.ema_weights():
            assert A._ema_reading and torch.equal(A.predict(x), want)
            raise RuntimeError("raised inside ema_weights()")
    assert not A._ema_reading and torch.equal(A.predict(x), raw)       # ... nor after an exception
    p_before, its = A.arena.p.clone(), A.iterations
    with A.ema_weights():
        with pytest.raises(g.Gct2Error, match="ema_weights"):
            A.train_step(x)
    assert torch.equal(A.arena.p, p_before) and A.iterations == its and torch.equal(A.predict(x), raw)
    with pytest.raises(ValueError, match="no averages"):
        C.predict(x, use_ema=True)
    with pytest.raises(ValueError, match="no averages"):
        with C.ema_weights():
            pass


def test_log_sample_reads_the_averages(averaged, gpu):
    import gan_class_transfer2_amd as g
    A, C, _, size = averaged
    rng = np.random.default_rng(5)
    t = lambda *shape: torch.tensor(rng.standard_normal(shape), dtype=torch.float32, device=gpu)
    args = (torch.tensor(rng.uniform(-1, 1, (1, size, size, 3)), dtype=torch.float32, device=gpu), t(1, 2, size, size, 3), t(size, size, 4, 3))
    denA, denC = types.SimpleNamespace(ensure_engine=lambda: A), types.SimpleNamespace(ensure_engine=lambda: C)
    kw = dict(steps=3, test_step=1)
    want_ema = g.log_sample(denC, *args, use_graph=False, **kw)
    want_raw = g.log_sample(denA, *args, use_graph=False, **kw)
    assert not torch.equal(want_ema["fake"], want_raw["fake"])
    for use_graph in (True, False):
        # interleaved on one engine: a graph captured on one weight set must never be replayed for the other
        for use_ema, want in ((False, want_raw), (True, want_ema), (False, want_raw), (True, want_ema)):
            got = g.log_sample(denA, *args, use_graph=use_graph, use_ema=use_ema, **kw)
            torch.cuda.synchronize()
            assert set(got) == set(want)
            for k in want:
                assert torch.equal(got[k], want[k]), (use_graph, use_ema, k)
    assert {k[2] for k in A._forward_graphs} == {False, True} and not A._ema_reading
    # the callback form forwards use_ema (it reads steps / test_step from the module globals, like the reference's log_sample)
    seen = []
    keep = (g.model.steps, g.model.test_step)
    g.configure(steps=3, test_step=1)
    try:
        g.make_log_sample(denA, *args, sink=lambda epoch, images: seen.append((epoch, images)), use_ema=True)(7, {})
        g.make_log_sample(denA, *args, sink=lambda epoch, images: seen.append((epoch, images)))(8, {})
    finally:
        g.configure(steps=keep[0], test_step=keep[1])
    assert [e for e, _ in seen] == [7, 8]
    for (_, got), want in zip(seen, (want_ema, want_raw)):
        for k in want:
            assert torch.equal(got[k], want[k]), k
    with pytest.raises(ValueError, match="no averages"):
        g.log_sample(denC, *args, use_ema=True, **kw)


# ---- 8. finalize_variable_values -----------------------------------------------------------------------------------------------
def test_finalize_variable_values_overwrites_the_parameters(gpu):
    import gan_class_transfer2_amd as g
    dt, topo, size = READ_CASES["bf16"]
    eng = g.UNetEngine(g.Topology(*topo), dt, gpu, base_lr=1e-2, warm_up=0, seed=21, use_ema=True, ema_momentum=0.9)
    rng = np.random.default_rng(3)
    xs = [torch.tensor(rng.uniform(-1, 1, (2, size, size, 3)), dtype=torch.float32, device=gpu) for _ in range(4)]
    for x in xs[:3]:
        eng.train_step(x)
    opt = g.LossScaleOptimizer(g.Adam(g.WarmUp(1e-2, 0), use_ema=True, ema_momentum=0.9))
    opt.inner.loss_scaling = False
    opt.inner._engine = eng
    ema, sh = eng.arena.ema.clone(), eng.arena.ema_shadow.clone()
    assert not torch.equal(eng.arena.p, ema)
    opt.finalize_variable_values()
    assert torch.equal(eng.arena.p, ema) and torch.equal(eng.arena.shadow, sh)
    assert torch.equal(eng.arena.ema, ema) and torch.equal(eng.arena.ema_shadow, sh)
    loss = eng.train_step(xs[3])
    torch.cuda.synchronize()
    assert np.isfinite(float(loss[0])) and eng.iterations == 4 and not torch.equal(eng.arena.p, ema)
    plain = g.UNetEngine(g.Topology(8, 16, 2), 0, gpu)
    with pytest.raises(ValueError, match="no averages"):
        plain.ema_overwrite()


# ---- 9. checkpoints ----------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_averages(gpu, tmp_path):
    cfg = O.OracleConfig(size=32, pixel_size=128, max_size=256, octaves=3, batch_size=4)
    params = O.init_params(cfg, seed=5)
    x = torch.tensor(O.synthetic_batch(cfg, seed=0)[0], dtype=torch.float32, device=gpu)
    a = make_engine(cfg, 1, gpu, rng_seed=11)
    a.set_params(params)
    parent_keys = set(a.state_dict())
    assert parent_keys == {"arena.p", "arena.m", "arena.v", "counters", "topology"}      # off: the dictionary of before
    assert not any(k.startswith("ema") for k in a.named_state_dict())
    off_path = str(tmp_path / "off.safetensors")
    a.save_checkpoint(off_path)
    a.enable_ema(0.9)
    for _ in range(2):
        a.train_step(x)
    assert set(a.state_dict()) == parent_keys | {"arena.ema", "ema_momentum"}
    path = str(tmp_path / "ema.safetensors")
    a.save_checkpoint(path)
    b = make_engine(cfg, 1, gpu, rng_seed=99, use_ema=True, ema_momentum=0.5)
    b.load_checkpoint(path)
    assert b.ema_momentum == 0.9                                       # the averages continue as they were kept
    assert torch.equal(a.arena.ema, b.arena.ema) and torch.equal(a.arena.ema_shadow, b.arena.ema_shadow)
    la, lb = a.train_step(x), b.train_step(x)
    torch.cuda.synchronize()
    assert float(la[0]) == float(lb[0])
    for name in ("p", "m", "v", "ema", "ema_shadow"):
        assert torch.equal(getattr(a.arena, name), getattr(b.arena, name)), name
    # the exchange format by parameter name carries them too
    named = a.named_state_dict()
    assert tuple(named["ema/U0.w"].shape) == tuple(named["p/U0.w"].shape) and float(named["ema_momentum"][0]) == 0.9
    c = make_engine(cfg, 1, gpu, rng_seed=7, use_ema=True)
    c.load_named_state_dict(named)
    assert c.ema_momentum == 0.9
    assert torch.equal(c.arena.ema, a.arena.ema) and torch.equal(c.arena.p, a.arena.p)
    # written without averages -> an averaging engine starts them from the loaded parameters
    d = make_engine(cfg, 1, gpu, use_ema=True)
    d.load_checkpoint(off_path)
    assert torch.equal(d.arena.ema, d.arena.p) and torch.equal(d.arena.ema_shadow, d.arena.shadow)
    assert torch.equal(d.arena._view(d.arena.p, "U1.w").cpu(), torch.tensor(params["U1.w"], dtype=torch.float32))
    # written with averages -> an engine without them refuses instead of dropping state
    e = make_engine(cfg, 1, gpu)
    with pytest.raises(ValueError, match="averages"):
        e.load_checkpoint(path)


# ---- 10. the variant engine --------------------------------------------------------------------------------------------------------
def test_variant_engine_averages(gpu):
    """VariantEngine holds no optimizer launch back, so its own iterates can be read between steps: the recurrence is checked on
    them bit for bit.  Averaging must not disturb training: p, m, v against a twin without averages, within the bound the
    data-parallel tests set for two runs of one step sequence (1e-6 relative: the small reductions of these kernels add with fp32
    atomics, whose order may differ between two runs; nothing else may)."""
    from gan_class_transfer2_amd.variants import VariantEngine
    rng = np.random.default_rng(9)
    mk = lambda **kw: VariantEngine(8, 16, 2, 1, False, True, 0, gpu, base_lr=1e-2, warm_up=0, seed=4, **kw)
    A = mk()
    assert A._ema is None and A.net.ema is None
    A.enable_ema(0.9)
    ps = [A.net.p.clone()]
    for k in range(3):
        A.train_step(torch.tensor(rng.uniform(-1, 1, (2, 16, 16, 3)), dtype=torch.float32, device=gpu))
        ps.append(A.net.p.clone())
    torch.cuda.synchronize()
    assert A.iterations == 3 and not torch.equal(ps[3], ps[0])
    assert torch.equal(A.net.ema.cpu(), host_recurrence(ps, [0.9] * 3)) and not torch.equal(A.net.ema, ps[3])
    B = mk()
    rng_b = np.random.default_rng(9)
    for k in range(3):
        B.train_step(torch.tensor(rng_b.uniform(-1, 1, (2, 16, 16, 3)), dtype=torch.float32, device=gpu))
    torch.cuda.synchronize()
    assert B._ema is None and B.iterations == 3
    for name in ("p", "m", "v"):
        a, b = getattr(A.net, name).double(), getattr(B.net, name).double()
        assert float((a - b).norm() / b.norm()) <= 1e-6, name
    C = mk()
    C.set_params({k: A.net.view(A.net.ema, k).clone().cpu().numpy() for k in A.net.shapes})
    x = torch.tensor(rng.uniform(-1, 1, (2, 16, 16, 3)), dtype=torch.float32, device=gpu)
    raw, want = A.predict(x).clone(), C.predict(x).clone()
    assert not torch.equal(raw, want)
    assert torch.equal(A.predict(x, use_ema=True), want) and torch.equal(A.predict(x), raw)
    with A.ema_weights():
        with pytest.raises(lib().Gct2Error, match="ema_weights"):
            A.train_step(x)
    with pytest.raises(ValueError, match="no averages"):
        C.predict(x, use_ema=True)
    A.ema_overwrite()
    assert torch.equal(A.net.p, A.net.ema) and torch.equal(A.predict(x), want)


# ---- 11. data parallel ---------------------------------------------------------------------------------------------------------------
def test_data_parallel_wrappers_and_the_averages(gpu):
    """DataParallelStep on a 1-rank group with the exchange forced (bucketed all-reduces and per-bucket Adam on the communication
    stream, finish_step - hence the EMA launch - in its tail, recorded with the step): the averages follow the recurrence over the
    engine's own iterates bit for bit, and equal the plain engine's within the bound that test_data_parallel_exchange_streams_single_rank
    sets for the parameters themselves (1e-6 relative: at these widths only the order of fp32 atomic additions may differ between two
    runs, and an average is a convex combination of iterates, so it inherits their bound).  ShardedDataParallelStep refuses."""
    import torch.distributed as dist
    from gan_class_transfer2_amd.distributed import DataParallelStep, ShardedDataParallelStep
    cfg = O.OracleConfig(size=32, pixel_size=64, max_size=128, octaves=3, batch_size=4)
    params = O.init_params(cfg, seed=5)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=gpu)
    try:
        emas = []
        for wrapped in (False, True):
            eng = make_engine(cfg, 1, gpu)
            eng.set_params(params)
            eng.enable_ema(0.9)
            stepper = DataParallelStep(eng, bucket_elems=100_000, force_exchange=True) if wrapped else eng
            ps = [eng.arena.p.clone()]
            for step in range(4):
                x, t_int, eps = O.synthetic_batch(cfg, seed=step)
                stepper.train_step(torch.tensor(x, dtype=torch.float32, device=gpu), torch.tensor(t_int), torch.tensor(eps, dtype=torch.float32))
                ps.append(eng.arena.p.clone())
            torch.cuda.synchronize()
            if wrapped:
                assert stepper.reducer.exchange and stepper.reducer.launched == len(stepper.reducer.buckets) >= 3
            assert eng.iterations == 4
            assert torch.equal(eng.arena.ema.cpu(), host_recurrence(ps, [0.9] * 4))
            assert torch.equal(eng.arena.ema_shadow, cast(1, eng.arena.ema))
            emas.append(eng.arena.ema.double().cpu())
        assert float((emas[1] - emas[0]).norm() / emas[0].norm()) <= 1e-6
        with pytest.raises(ValueError, match="ShardedDataParallelStep"):
            ShardedDataParallelStep(eng, force_exchange=True)
        plain = make_engine(cfg, 1, gpu)
        ShardedDataParallelStep(plain, force_exchange=True)
        with pytest.raises(ValueError, match="ShardedDataParallelStep"):
            plain.enable_ema(0.9)
    finally:
        dist.destroy_process_group()


# ---- 12. averages switched off and on again under step plans ---------------------------------------------------------------------
def test_averages_switched_off_and_on_again_under_plans(gpu, recorded):
    """a recorded step bakes in the addresses of the averages; disable_ema() frees them and a later enable_ema() with the SAME
    momentum allocates new ones (what Trainer.compile does when the optimizer goes plain and back): the old plans must not be
    replayed.  enable, planned steps, disable, allocations that take the freed blocks, enable, planned steps - the new averages must
    follow the recurrence from the parameters at the second enable, and the tensors allocated in between must stay untouched."""
    cfg = O.OracleConfig(**STEP_CFG)
    params = O.init_params(cfg, seed=3)
    xs = [torch.tensor(O.synthetic_batch(cfg, seed=k)[0], dtype=torch.float32, device=gpu) for k in range(3)]
    A, B = make_engine(cfg, 1, gpu, rng_seed=5), make_engine(cfg, 1, gpu, rng_seed=5)
    for e in (A, B):
        e.set_params(params)
    A.enable_ema(0.9)
    ps = [B.arena.p.clone()]
    for k in range(4):
        A.train_step(xs[k % 3])
        B.train_step(xs[k % 3])
        ps.append(B.arena.p.clone())
    assert len(A._plans) >= 1
    assert torch.equal(A.arena.ema.cpu(), host_recurrence(ps, [0.9] * 4))
    A.disable_ema()
    assert not A._plans and not A._plan_seen and A.arena.ema is None
    torch.cuda.synchronize()
    n = A.arena.total
    guards = [torch.full((n,), 3.0, dtype=torch.float32, device=gpu) for _ in range(2)] + \
             [torch.full((n,), 3.0, dtype=torch.bfloat16, device=gpu) for _ in range(2)]
    A.enable_ema(0.9)
    ps = [ps[-1]]
    for k in range(4, 9):
        A.train_step(xs[k % 3])
        B.train_step(xs[k % 3])
        ps.append(B.arena.p.clone())
    ema = A.arena.ema
    torch.cuda.synchronize()
    assert len(A._plans) >= 1 and all("gct2_ema_update" in recorded(sp.plan) for sp in A._plans.values())
    assert torch.equal(ema.cpu(), host_recurrence(ps, [0.9] * 5))
    assert torch.equal(A.arena.ema_shadow, cast(1, ema)) and torch.equal(A.arena.p, B.arena.p)
    assert all(bool((t.float() == 3.0).all()) for t in guards)
