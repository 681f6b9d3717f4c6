"""The noise schedule as a setting of the engines (set_noise_schedule, train.py:85-93): train steps, the noised image, step plans, the
objective's coefficients, checkpoints and the sampler, on the GPU.

The topology is that of the sampler fixture (size 16, pixel_size 8, max_size 16, 2 octaves), batch 2, steps = 7: steps + 1 is a power
of two, so t / (steps + 1) and t * fl(1 / (steps + 1)) agree in float32 at every timestep and the quadratic TABLE (a division, like
train.py:87) holds the very pairs the bf16 formula kernel (a product) computes - the table path can be compared with the formula
path bit for bit in every dtype."""
import math
import os
import types

import numpy as np
import pytest
import torch

from noise_schedule_cases import BF16, F16, F32, mix_ref
from oracle import denoiser_oracle as O
from oracle import sampler_oracle as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_sampler.npz")
TOPO, SIZE, BATCH, STEPS = (8, 16, 2), 16, 2, 7
DTS = [F32, BF16, F16]
DT_IDS = ["f32", "bf16", "f16_loss_scaled"]
QUADRATIC_BODY = lambda t: (1 - t) ** 2 * 0.25          # train.py:93 as a user's own body: forces the table path
DEFAULT_KEYS = {"arena.p", "arena.m", "arena.v", "counters", "topology"}


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def make_engine(gpu, dt, schedule=None, offset=0.0, **kw):
    import gan_class_transfer2_amd as g
    eng = g.UNetEngine(g.Topology(*TOPO), dt, gpu, **{**dict(steps=STEPS, base_lr=1e-2, warm_up=0, seed=21, rng_seed=5,
                                                          loss_scaling=(dt == F16)), **kw})
    if schedule is not None:
        eng.set_noise_schedule(schedule, offset)
    return eng


def batches(gpu, n, seed=11):
    rng = np.random.default_rng(seed)
    return [torch.tensor(np.floor(rng.uniform(0, 256, (BATCH, SIZE, SIZE, 3))) / 128 - 1, dtype=torch.float32, device=gpu) for _ in range(n)]


def arenas_of(eng):
    A = eng.arena
    torch.cuda.synchronize()
    return {n: getattr(A, n).clone() for n in ("p", "m", "v") + (("shadow",) if A.shadow is not None else ())}


HEAD = ("dense.w", "dense.b")


def head_mask(offsets, numel, total, device):
    m = torch.zeros(total, dtype=torch.bool, device=device)
    for k in HEAD:
        m[offsets[k]:offsets[k] + numel(k)] = True
    return m


def assert_same_state(a, b, what):
    """two engines: every parameter, optimizer slot and counter bit for bit; a failure names the tensors that differ"""
    sa, sb = arenas_of(a), arenas_of(b)
    for n in sa:
        if not torch.equal(bits(sa[n]), bits(sb[n])):
            bad = (bits(sa[n]) != bits(sb[n])).cpu().numpy()
            names = [k for k, o in a.arena.offsets.items() if bad[o:o + a.arena.numel(k)].any()]
            raise AssertionError(f"{what}: arena {n} differs in {int(bad.sum())} elements, in {names}")
    assert (a.iterations, a.rng_offset_t, a.rng_offset_eps) == (b.iterations, b.rng_offset_t, b.rng_offset_eps), what


def lockstep(T, D, x, what):
    """one train step of two engines from the SAME arenas (T's are overwritten with D's first), compared bit for bit.

    Why not two free-running engines: at this topology the head runs gct2_dense_bwd, which adds the partial sums of its four
    work-groups (512 pixels, 128 per work-group) into dense.w / dense.b with float atomics, in the order they arrive.  Two runs of ONE
    default engine on the same inputs already differ there in the last bit (tests/test_optimizers_gpu.py own_gradients,
    tests/test_losses_gpu.py lockstep: the provision every step test of this topology makes).  Measured on an MI355X with two
    free-running engines, table against formula, two steps: 1 to 8 elements of dense.w / dense.b differed in p, m or v in each of the
    six cases (three dtypes, eager and planned), and never an element of any other tensor.

    So: the losses, the noised image, the counters, and every element of p, m, v and the 16-bit copy OUTSIDE dense.w / dense.b must
    be equal unconditionally; inside those two tensors, wherever the two engines' gradients came out equal (Adam is elementwise) -
    when the step left its gradients in the arena (a step with the fused per-layer Adam does not; the two tensors are then left out).
    Returns the share of arena elements compared."""
    for n, t in arenas_of(D).items():
        getattr(T.arena, n).copy_(t)
    lt, ld = T.train_step(x).clone(), D.train_step(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(bits(lt), bits(ld)) and bool(torch.isfinite(lt).all()), (what, lt, ld)
    assert (T.iterations, T.rng_offset_t, T.rng_offset_eps) == (D.iterations, D.rng_offset_t, D.rng_offset_eps), what
    bt, bd = T.buffers(*x.shape[:3]), D.buffers(*x.shape[:3])
    assert torch.equal(bits(bt.img), bits(bd.img)) and torch.equal(bt.t_int, bd.t_int), what          # the noised image itself
    assert T._grads_in_arena == D._grads_in_arena, what
    A = D.arena
    head = head_mask(A.offsets, A.numel, A.total, A.g.device)
    if D._grads_in_arena:
        same = bits(T.arena.g) == bits(D.arena.g)
        if not bool(same[~head].all()):
            bad = (~same).cpu().numpy()
            raise AssertionError(f"{what}: gradients differ in {[k for k, o in A.offsets.items() if bad[o:o + A.numel(k)].any()]}")
    else:
        same = ~head
    a, b = arenas_of(T), arenas_of(D)
    for n in a:
        if not torch.equal(bits(a[n])[same], bits(b[n])[same]):
            bad = ((bits(a[n]) != bits(b[n])) & same).cpu().numpy()
            raise AssertionError(f"{what}: arena {n} differs in {int(bad.sum())} compared elements, in "
                                 f"{[k for k, o in A.offsets.items() if bad[o:o + A.numel(k)].any()]}")
    return float(same.float().mean())


@pytest.fixture
def recorded(monkeypatch):
    """names(plan) -> the entry-point names a step plan recorded, in order"""
    P = lib().Plan
    orig, log = P.add_call, {}

    def add_call(self, name, args):
        orig(self, name, args)
        if name in lib().PLANNABLE:
            log.setdefault(id(self), []).append(name)
    monkeypatch.setattr(P, "add_call", add_call)
    return lambda plan: log.get(id(plan), [])


# ---- 1. the plumbing is bit-identical --------------------------------------------------------------------------------------------------
# (dtype, planned, fuse_adam).  fuse_adam off: the gradients stay in the arena, so dense.w / dense.b are compared too; the loss-scaled
# F16 step never fuses, so it needs no such twin
PLUMBING = [(dt, planned, fuse) for dt in DTS for planned in (False, True) for fuse in (True, False) if fuse or dt != F16]
PLUMBING_IDS = [f"{DT_IDS[dt]}-{'planned' if planned else 'eager'}{'' if fuse else '-fuse_adam_off'}" for dt, planned, fuse in PLUMBING]


@pytest.mark.parametrize("dt,planned,fuse_adam", PLUMBING, ids=PLUMBING_IDS)
def test_quadratic_table_steps_equal_default_steps(gpu, dt, planned, fuse_adam, recorded):
    """one engine under the callable (1 - t)**2 * 0.25 (the table entry points), one default engine (the formula entry points): two
    train steps from the same seeds - the losses, the noised image and the parameters, bit for bit (lockstep says where the parent's
    float atomics allow no comparison of two engines at all)."""
    xs = batches(gpu, 2)
    T, D = make_engine(gpu, dt, QUADRATIC_BODY), make_engine(gpu, dt)
    assert not T._default_schedule() and D._default_schedule() and "noise_schedule" not in vars(D)
    for e in (T, D):
        e.use_plan, e.plan_after, e.fuse_adam = planned, 1, fuse_adam      # (planned: the first step already records and replays)
    shares = [lockstep(T, D, x, f"step {k}") for k, x in enumerate(xs)]
    print(f"share of arena elements compared per step: {' '.join('%.4f' % u for u in shares)}")
    assert min(shares) > 0.99                                        # dense.w / dense.b are 24 of ~9e4 elements
    assert D._grads_in_arena == (not fuse_adam or dt == F16)
    assert bool(T._plans) == bool(D._plans) == planned
    if planned:
        nt = [recorded(sp.plan) for sp in T._plans.values()]
        nd = [recorded(sp.plan) for sp in D._plans.values()]
        assert all(n.count("gct2_noise_image_rng_table") == 1 and "gct2_noise_image_rng" not in n for n in nt), nt
        assert all(n.count("gct2_noise_image_rng") == 1 and "gct2_noise_image_rng_table" not in n for n in nd), nd
        assert [len(n) for n in nt] == [len(n) for n in nd]          # the same call list otherwise
    assert D._noise_tables is None                                   # the default engine never built a table


# ---- 2. the noised image -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_noised_image_under_cosine(gpu, dt):
    """after sample_and_noise_into_r0(keep_eps=True): the packed image (and R_0's image slice) = numpy's mix of x, the kept eps and
    noise_table("cosine")[t_int - 1], bit for bit"""
    import gan_class_transfer2_amd as g
    eng = make_engine(gpu, dt, "cosine")
    x = batches(gpu, 1, seed=3)[0]
    b = eng.buffers(BATCH, SIZE, SIZE)
    eng.sample_and_noise_into_r0(b, x, keep_eps=True)
    torch.cuda.synchronize()
    t = b.t_int.cpu().numpy()
    assert ((t >= 1) & (t <= STEPS)).all()
    table = g.trainer_math.noise_table("cosine", 0.0, STEPS, dt)
    want = mix_ref(dt, x.cpu().numpy().reshape(BATCH, -1, 3), b.eps.cpu().numpy().reshape(BATCH, -1, 3), table[t - 1]).reshape(BATCH, SIZE, SIZE, 3)
    fu0 = eng.topo.fu(0)
    for name, got in (("packed image", b.img[..., :3]), ("R_0 image slice", b.R[0][..., fu0:fu0 + 3])):
        assert torch.equal(bits(got.cpu().contiguous()), bits(want)), name
    # ... and it is not the quadratic schedule's image
    quad = mix_ref(dt, x.cpu().numpy().reshape(BATCH, -1, 3), b.eps.cpu().numpy().reshape(BATCH, -1, 3),
                   g.trainer_math.noise_table("quadratic", 0.0, STEPS, dt)[t - 1]).reshape(BATCH, SIZE, SIZE, 3)
    assert not torch.equal(bits(quad), bits(want))


# ---- 3. stale plans ----------------------------------------------------------------------------------------------------------------------
def test_a_changed_schedule_is_another_plan(gpu, recorded):
    """one planned engine stepped under quadratic, cosine, quadratic again, against an eager engine given the same sequence: bit for
    bit (lockstep) - a plan recorded under one schedule is never replayed under another"""
    xs = batches(gpu, 6, seed=5)
    P, E = make_engine(gpu, BF16), make_engine(gpu, BF16)
    P.use_plan, P.plan_after, E.use_plan = True, 1, False
    for k, name in enumerate(["quadratic"] * 2 + ["cosine"] * 2 + ["quadratic"] * 2):
        for e in (P, E):
            e.set_noise_schedule(name)
        lockstep(P, E, xs[k], f"step {k} under {name}")
    assert not E._plans
    names = [recorded(sp.plan) for sp in P._plans.values()]
    assert any("gct2_noise_image_rng_table" in n for n in names) and any("gct2_noise_image_rng" in n for n in names)
    assert not any("gct2_noise_image_rng_table" in n and "gct2_noise_image_rng" in n for n in names)
    # the two schedules do give different images (the comparison above is not vacuous)
    P.set_noise_schedule("cosine")
    E.set_noise_schedule("quadratic")
    for e in (P, E):
        e.rng_offset_t = e.rng_offset_eps = 0
        e.sample_and_noise_into_r0(e.buffers(BATCH, SIZE, SIZE), xs[0])
    torch.cuda.synchronize()
    assert not torch.equal(bits(P.buffers(BATCH, SIZE, SIZE).img), bits(E.buffers(BATCH, SIZE, SIZE).img))


# ---- 4. the objective's coefficients -----------------------------------------------------------------------------------------------------
def test_objective_coefficients_under_exp2(gpu):
    """predict_x=False, prediction_weighting=True under "exp2": (a, c, w) of the step = numpy's gather from alpha_table"""
    import gan_class_transfer2_amd as g
    eng = make_engine(gpu, F32, "exp2", predict_x=False, prediction_weighting=True)
    x = batches(gpu, 1, seed=7)[0]
    loss = eng.train_step(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())
    b = eng.buffers(BATCH, SIZE, SIZE)
    t = b.t_int.cpu().numpy()
    A = g.trainer_math.alpha_table("exp2", 0.0, STEPS)
    assert A.dtype == np.float32 and A.shape == (STEPS + 1,)
    s = np.sqrt(np.float32(1) - A[t])
    a, c, w = (v.cpu().numpy() for v in b._coef)
    assert np.array_equal(a, np.zeros(BATCH, np.float32)) and np.array_equal(c, s) and np.array_equal(w, s)
    # ODE mode gathers at t - 1
    ode = make_engine(gpu, F32, "exp2", ordinary_differential_equation=True)
    ode.train_step(x)
    torch.cuda.synchronize()
    t = ode.buffers(BATCH, SIZE, SIZE).t_int.cpu().numpy()
    a, c, w = (v.cpu().numpy() for v in ode.buffers(BATCH, SIZE, SIZE)._coef)
    assert np.array_equal(a, np.sqrt(A[t - 1])) and np.array_equal(c, np.sqrt(np.float32(1) - A[t - 1])) and np.array_equal(w, np.ones(BATCH, np.float32))


# ---- 5. VariantEngine --------------------------------------------------------------------------------------------------------------------
def test_variant_engine_quadratic_table_steps_equal_default_steps(gpu):
    """block_depth = 1 on VariantEngine, F32: the table engine against the default engine in lockstep - losses and noised images bit
    for bit; p, m, v wherever the two engines' gradients are equal.  Here the same provision reaches further than on UNetEngine:
    besides the head (gct2_dense_bwd), the full-resolution 3 x 3 convolutions of Block sum their weight gradients with float atomics
    (measured on an MI355X: blkTopA.0.w, blkTopB.0.w, dense.w and dense.b differed between the two engines, no other tensor)"""
    from gan_class_transfer2_amd.variants import VariantEngine
    xs = batches(gpu, 2, seed=9)
    make = lambda: VariantEngine(TOPO[0], TOPO[1], TOPO[2], 1, False, True, F32, gpu, steps=STEPS, base_lr=1e-2, warm_up=0, seed=21, rng_seed=5)
    T, D = make(), make()
    T.set_noise_schedule(QUADRATIC_BODY)
    assert not T._default_schedule() and D._default_schedule()
    N = D.net
    numel = lambda k: int(np.prod(N.shapes[k]))
    for k, x in enumerate(xs):
        for n in ("p", "m", "v"):
            getattr(T.net, n).copy_(getattr(D.net, n))
        T.refresh_operands()
        lt, ld = T.train_step(x).clone(), D.train_step(x).clone()
        torch.cuda.synchronize()
        assert torch.equal(bits(lt), bits(ld)) and bool(torch.isfinite(lt).all()), (k, lt, ld)
        assert torch.equal(bits(T.last["noised"]), bits(D.last["noised"])), k
        same = bits(T.net.g) == bits(D.net.g)
        bad = (~same).cpu().numpy()
        print(f"step {k}: share of equal gradients {float(same.float().mean()):.4f}; unequal in {[n for n, o in N.offsets.items() if bad[o:o + numel(n)].any()]}")
        for n in ("p", "m", "v"):
            assert torch.equal(bits(getattr(T.net, n))[same], bits(getattr(D.net, n))[same]), (k, n)
        assert float(same.float().mean()) > 0.9                      # (the comparison covers most of the arena)
    with pytest.raises(ValueError, match="unknown noise_schedule"):
        T.set_noise_schedule("linear")


# ---- 6. checkpoints ----------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_mismatch(gpu):
    xs = batches(gpu, 2, seed=13)
    A = make_engine(gpu, BF16, "cosine", 0.0)
    A.train_step(xs[0])
    sd = A.state_dict()
    assert set(sd) == DEFAULT_KEYS | {"noise_schedule"} and sd["noise_schedule"].tolist() == [4.0, 0.0]
    B = make_engine(gpu, BF16, "cosine", 0.0, seed=99)
    B.load_state_dict(sd)
    assert_same_state(A, B, "after loading")
    la, lb = A.train_step(xs[1]).clone(), B.train_step(xs[1]).clone()
    torch.cuda.synchronize()
    assert torch.equal(bits(la), bits(lb))                           # (the forward pass has no atomics: the same loss from the same state)
    # a named schedule that disagrees: refused, nothing is loaded
    for other in (make_engine(gpu, BF16, seed=99), make_engine(gpu, BF16, "exp2", seed=99), make_engine(gpu, BF16, "cosine", -1e-4, seed=99)):
        before = arenas_of(other)
        with pytest.raises(ValueError, match="nothing is loaded"):
            other.load_state_dict(sd)
        after = arenas_of(other)
        assert all(torch.equal(bits(before[n]), bits(after[n])) for n in before) and other.iterations == 0
    # a default engine's dictionary is what it was; a cosine engine refuses it; a callable is stored as "custom" and loads anywhere
    D = make_engine(gpu, BF16)
    assert set(D.state_dict()) == DEFAULT_KEYS
    with pytest.raises(ValueError, match="nothing is loaded"):
        make_engine(gpu, BF16, "cosine").load_state_dict(D.state_dict())
    Cu = make_engine(gpu, BF16, QUADRATIC_BODY)
    assert Cu.state_dict()["noise_schedule"].tolist() == [-1.0, 0.0]
    D.load_state_dict(Cu.state_dict())
    named = A.named_state_dict()
    assert "noise_schedule" in named
    with pytest.raises(ValueError, match="nothing is loaded"):
        D.load_named_state_dict(named)


# ---- 7. the sampler ----------------------------------------------------------------------------------------------------------------------
def sampler_engine(gpu, z, schedule=None, **switches):
    eng = make_engine(gpu, F32, schedule, **switches)
    eng.set_params({k[6:]: z[k] for k in z.files if k.startswith("param/")})
    return eng


def run_log_sample(gpu, eng, z, **kw):
    import gan_class_transfer2_amd as g
    den = types.SimpleNamespace(ensure_engine=lambda: eng)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
    res = g.log_sample(den, t(z["example_image"]), t(z["example"]), t(z["dictionary"]), steps=STEPS, test_step=2, **kw)
    torch.cuda.synchronize()
    return res


def test_log_sample_with_the_quadratic_callable_equals_the_default(gpu):
    z = np.load(GOLDEN)
    a = run_log_sample(gpu, sampler_engine(gpu, z, QUADRATIC_BODY), z)
    b = run_log_sample(gpu, sampler_engine(gpu, z), z)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def test_log_sample_refuses_a_schedule_that_is_not_the_engines(gpu):
    z = np.load(GOLDEN)
    eng = sampler_engine(gpu, z, "cosine")
    for kw in (dict(noise_schedule="exp2"), dict(noise_schedule="quadratic"), dict(alpha_dash_offset=1e-4), dict(noise_schedule="cosine", alpha_dash_offset=-1e-4)):
        with pytest.raises(ValueError, match="log_sample: noise schedule"):
            run_log_sample(gpu, eng, z, **kw)
    with pytest.raises(ValueError, match="log_sample: noise schedule"):
        run_log_sample(gpu, sampler_engine(gpu, z), z, noise_schedule="cosine")
    run_log_sample(gpu, eng, z, noise_schedule="cosine", alpha_dash_offset=0.0)      # an explicit pair that agrees


ORACLE_BODIES = {     # train.py:91 and :88 in float64, written out here (not taken from the code under test)
    "cosine": lambda t, steps=200: np.cos(math.pi / 2 * (np.asarray(t, dtype=np.float64) / (steps + 1))) ** 2,
    "exp2": lambda t, steps=200: 1 - 2 ** (np.asarray(t, dtype=np.float64) / (steps + 1) - 1),
}


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("mode", ["default", "ode"])
@pytest.mark.parametrize("name", ["cosine", "exp2"])
def test_log_sample_fp32_against_the_oracle(gpu, name, mode, monkeypatch, parity_log):
    """fp32 log_sample under another schedule against oracle.sampler_oracle.log_sample run live in float64 on the fixture's network,
    with the oracle's alpha_dash replaced for the duration of the test (the oracle reads it at call time).  The bound is the project's
    own for this comparison: 2e-5 relative L2 (tests/test_sampler_gpu.py)."""
    z = np.load(GOLDEN)
    switches = dict(ordinary_differential_equation=True) if mode == "ode" else {}
    cfg = O.OracleConfig(size=SIZE, pixel_size=TOPO[0], max_size=TOPO[1], octaves=TOPO[2], batch_size=1)
    params = {k[6:]: z[k] for k in z.files if k.startswith("param/")}
    monkeypatch.setattr(O, "alpha_dash", ORACLE_BODIES[name])
    want = S.log_sample(S.unet_denoiser(params, cfg), z["example_image"], z["example"], z["dictionary"], STEPS, 2, **switches)
    res = run_log_sample(gpu, sampler_engine(gpu, z, name, **switches), z, **switches)
    assert set(res) == set(want)
    errs = {}
    for k, v in res.items():
        ref = np.asarray(want[k])
        errs[k] = rel_l2(v.cpu().numpy().reshape(ref.shape), ref)
    print(f"log_sample fp32 {name} {mode}: " + " ".join(f"{k}={e:.3g}" for k, e in errs.items()))
    parity_log(f"log_sample_fp32_{name}_{mode}", **errs)
    for k, e in errs.items():
        assert e <= 2e-5, (name, mode, k, e)


# ---- 8. the public interface ---------------------------------------------------------------------------------------------------------------
def test_trainer_follows_the_module_globals(gpu):
    """Trainer reads noise_schedule / alpha_dash_offset before every step, like training_loss"""
    import gan_class_transfer2_amd as g
    names = ("size", "pixel_size", "max_size", "octaves", "compute_dtype", "mixed_precision", "block_depth", "residual", "concat", "steps",
             "noise_schedule", "alpha_dash_offset")
    keep = {n: getattr(g.model, n) for n in names}
    try:
        g.configure(size=SIZE, pixel_size=TOPO[0], max_size=TOPO[1], octaves=TOPO[2], compute_dtype="bfloat16", mixed_precision=False,
                    block_depth=0, residual=False, concat=True, steps=STEPS)
        tr = g.Trainer(g.Denoiser(seed=3, device=gpu))
        tr.compile(g.Adam(1e-3), g.identity)
        x = batches(gpu, 1, seed=15)[0]
        tr.train_step((x, x))
        eng = tr.denoiser.engine
        assert eng._default_schedule() and eng._noise_tables is None
        g.configure(noise_schedule="cosine")
        tr.train_step((x, x))
        assert (eng.noise_schedule, eng.alpha_dash_offset) == ("cosine", 0.0)
        assert tr(x).shape == ()                                      # Trainer.call: sample_noise + the table form of the noising
        g.configure(noise_schedule="quadratic", alpha_dash_offset=1e-4)
        tr.train_step((x, x))
        assert (eng.noise_schedule, eng.alpha_dash_offset) == ("quadratic", 1e-4) and not eng._default_schedule()
        g.model.noise_schedule = "linear"                             # written past configure: refused before the step
        with pytest.raises(ValueError, match="unknown noise_schedule"):
            tr.train_step((x, x))
        g.configure(noise_schedule="quadratic", alpha_dash_offset=0.0)
        tr.train_step((x, x))
        torch.cuda.synchronize()
        assert eng._default_schedule() and eng.iterations == 4
        # an engine built by anything else (denoiser(...), the sampler callback) starts under the globals as they stand, like the
        # objective switches
        g.configure(noise_schedule="exp2", alpha_dash_offset=1e-4)
        fresh = g.Denoiser(seed=3, device=gpu).ensure_engine()
        assert (fresh.noise_schedule, fresh.alpha_dash_offset) == ("exp2", 1e-4)
        g.configure(noise_schedule="quadratic", alpha_dash_offset=0.0)
        assert g.Denoiser(seed=3, device=gpu).ensure_engine()._noise_tables is None
    finally:
        g.model.noise_schedule = "quadratic"
        g.configure(**keep)
