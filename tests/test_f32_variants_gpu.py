"""fp32 on the matrix cores beyond the default topology: the stride-1 convolutions gct2_conv2d_s1_{fwd,dgrad,wgrad} through a
context in F32_MATH_MFMA mode (FORM_S1 / FORM_S1T of f32_mfma.hip and the stride-1 mode of its weight gradient),
VariantEngine(f32_matrix=True), model.f32_matrix_cores with a topology switch, and the sampler of a variant network.

Tolerances: those of test_f32_matrix_gpu.py for the kernels (rel-L2 <= 2e-6 against the fp64 oracle; unsplit forward / input-
gradient launches EQUAL to the direct kernels; split launches equal run to run and within 1e-6 of the unsplit result) and those of
test_variants_gpu.py's fp32 case for the train steps (loss 1e-5, every gradient 5e-5, parameters after two Adam steps 2e-6).
"""
import gc
import types

import numpy as np
import pytest
import torch

from oracle import denoiser_oracle as O
from oracle import variants_oracle as V

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
TOL = 2e-6

# (B, H, W, Cin, Cout, ks): every odd ks, the 3-channel Block input in front of level 0, ragged channel counts, odd grids, several
# m- / n-tiles, and a deep level whose 32 output pixels cannot fill the chip (the reduction is split when there is a workspace)
S1_SHAPES = [
    (2, 8, 8, 16, 24, 3),
    (1, 5, 7, 3, 8, 3),
    (2, 5, 7, 3, 128, 3),
    (2, 9, 11, 13, 7, 5),
    (1, 9, 11, 5, 136, 7),
    (2, 6, 4, 136, 13, 1),
    (3, 12, 20, 72, 136, 3),
    (2, 4, 4, 512, 512, 3),
]
SLAB_SHAPE = (4, 32, 32, 64, 128, 3)     # 4096 pixels, 576 x 128 weight gradient: ordered pixel-split slabs


@pytest.fixture(autouse=True)
def _collect_engines():
    yield
    gc.collect()
    torch.cuda.synchronize()


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def f32(a, device):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=device)


def rnd(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def make_ctx(gpu, ws=True, direct=False, tuning=0):
    """a call context on the fp32 matrix cores (or forced direct), with or without a 64 MiB workspace (which the weight gradients
    also use as their scratch: no separate one is registered), launch log on"""
    c = lib().Context()
    c.set_f32_math(lib().F32_MATH_MFMA)
    if direct:
        c.force_direct(True)
    if tuning:
        c.set_tuning(tuning)
    if ws:
        c._ws = torch.empty(16 << 20, dtype=torch.float32, device=gpu)
        c.set_workspace(c._ws)
    c.log_launches(True)
    return c


def check_log(c, kind, calls):
    """one f32mfma token of `kind` per call, nothing else (the direct kernels would log nothing or a direct: token)"""
    log = c.read_launch_log()
    assert len(log) == calls and all(t.startswith(f"f32mfma:{kind}:") for t in log), log
    return log


def splits(log):
    return [int(t.split("=")[1].split(":")[0]) for t in log]


def call_fwd(c, x, ldx, w, b, y, ldy, shape, relu):
    B, H, W, Cin, Cout, ks = shape
    lib().call("gct2_conv2d_s1_fwd", c.handle, F32, x, ldx, w.data_ptr(), b.data_ptr() if b is not None else None, y, ldy,
               B, H, W, Cin, Cout, ks, relu, stream())


def call_dgrad(c, dz, lddz, w, act, ldact, dx, lddx, shape, accumulate):
    B, H, W, Cin, Cout, ks = shape
    lib().call("gct2_conv2d_s1_dgrad", c.handle, F32, dz, lddz, w.data_ptr(), act, ldact, dx, lddx, B, H, W, Cin, Cout, ks, accumulate,
               stream())


def call_wgrad(c, x, ldx, dz, lddz, dw, db, shape, accumulate):
    B, H, W, Cin, Cout, ks = shape
    lib().call("gct2_conv2d_s1_wgrad", c.handle, F32, x.data_ptr(), ldx, dz.data_ptr(), lddz, dw.data_ptr(),
               db.data_ptr() if db is not None else None, B, H, W, Cin, Cout, ks, accumulate, stream())


# ---- 1. every stride-1 entry point against the fp64 oracle, through views (ld > C, pointer offsets) -------------------------------

@pytest.mark.parametrize("ws", [True, False])
@pytest.mark.parametrize("relu,bias", [(0, False), (1, True)])
@pytest.mark.parametrize("shape", S1_SHAPES)
def test_s1_fwd_f32_matrix(gpu, shape, relu, bias, ws):
    B, H, W, Cin, Cout, ks = shape
    rng = np.random.default_rng(1)
    x, w = rnd(rng.standard_normal((B, H, W, Cin))), rnd(rng.standard_normal((ks, ks, Cin, Cout)) * 0.1)
    b = rnd(rng.standard_normal(Cout)) if bias else None
    ref = V.conv_s1_fwd(x, w, b)
    ref = np.maximum(ref, 0) if relu else ref
    ldx, ldy, offx, offy = Cin + 5, Cout + 3, 3, 2
    xb = torch.zeros(B, H, W, ldx, dtype=torch.float32, device=gpu)
    xb[..., offx:offx + Cin] = f32(x, gpu)
    yb = torch.full((B, H, W, ldy), 7.0, dtype=torch.float32, device=gpu)
    c = make_ctx(gpu, ws)
    call_fwd(c, xb.data_ptr() + 4 * offx, ldx, f32(w, gpu), f32(b, gpu) if bias else None, yb.data_ptr() + 4 * offy, ldy, shape, relu)
    torch.cuda.synchronize()
    assert rel_l2(yb[..., offy:offy + Cout].cpu().numpy(), ref) <= TOL
    assert float((yb[..., :offy] - 7).abs().max()) == 0 and float((yb[..., offy + Cout:] - 7).abs().max()) == 0
    check_log(c, "s1", 1)


@pytest.mark.parametrize("ws", [True, False])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", S1_SHAPES)
def test_s1_dgrad_f32_matrix(gpu, shape, masked, accumulate, ws):
    B, H, W, Cin, Cout, ks = shape
    rng = np.random.default_rng(3)
    x = rnd(np.maximum(rng.standard_normal((B, H, W, Cin)), 0))
    w = rnd(rng.standard_normal((ks, ks, Cin, Cout)) * 0.1)
    dz = rnd(rng.standard_normal((B, H, W, Cout)))
    prev = rnd(rng.standard_normal((B, H, W, Cin)))
    dx_ref, _, _ = V.conv_s1_bwd(x, w, dz)
    ref = (dx_ref * (x > 0) if masked else dx_ref) + (prev if accumulate else 0)
    lddz, lddx, ldact = Cout + 2, Cin + 3, Cin + 1
    dzb = torch.zeros(B, H, W, lddz, dtype=torch.float32, device=gpu); dzb[..., 1:1 + Cout] = f32(dz, gpu)
    dxb = torch.full((B, H, W, lddx), 5.0, dtype=torch.float32, device=gpu); dxb[..., 2:2 + Cin] = f32(prev, gpu)
    actb = torch.zeros(B, H, W, ldact, dtype=torch.float32, device=gpu); actb[..., :Cin] = f32(x, gpu)
    c = make_ctx(gpu, ws)
    call_dgrad(c, dzb.data_ptr() + 4, lddz, f32(w, gpu), actb.data_ptr() if masked else None, ldact, dxb.data_ptr() + 8, lddx, shape,
               accumulate)
    torch.cuda.synchronize()
    assert rel_l2(dxb[..., 2:2 + Cin].cpu().numpy(), ref) <= TOL
    assert float((dxb[..., :2] - 5).abs().max()) == 0 and float((dxb[..., 2 + Cin:] - 5).abs().max()) == 0
    check_log(c, "s1t", 1)


def _wgrad_inputs(gpu, shape, seed):
    B, H, W, Cin, Cout, ks = shape
    rng = np.random.default_rng(seed)
    x = rnd(rng.standard_normal((B, H, W, Cin)))
    dz = rnd(rng.standard_normal((B, H, W, Cout)))
    _, dw_ref, db_ref = V.conv_s1_bwd(x, np.zeros((ks, ks, Cin, Cout)), dz)
    ldx, lddz = Cin + 1, Cout + 4
    xb = torch.zeros(B, H, W, ldx, dtype=torch.float32, device=gpu); xb[..., :Cin] = f32(x, gpu)
    dzb = torch.zeros(B, H, W, lddz, dtype=torch.float32, device=gpu); dzb[..., :Cout] = f32(dz, gpu)
    return xb, ldx, dzb, lddz, dw_ref, db_ref


@pytest.mark.parametrize("ws", [True, False])
@pytest.mark.parametrize("shape", S1_SHAPES + [SLAB_SHAPE])
def test_s1_wgrad_f32_matrix(gpu, shape, ws):
    B, H, W, Cin, Cout, ks = shape
    xb, ldx, dzb, lddz, dw_ref, db_ref = _wgrad_inputs(gpu, shape, 5)
    dw = torch.full((ks, ks, Cin, Cout), 9.0, dtype=torch.float32, device=gpu)      # overwritten (accumulate = 0)
    db = torch.full((Cout,), 9.0, dtype=torch.float32, device=gpu)
    c = make_ctx(gpu, ws)
    call_wgrad(c, xb, ldx, dzb, lddz, dw, db, shape, 0)
    torch.cuda.synchronize()
    assert rel_l2(dw.cpu().numpy(), dw_ref) <= TOL
    assert rel_l2(db.cpu().numpy(), db_ref) <= TOL
    call_wgrad(c, xb, ldx, dzb, lddz, dw, db, shape, 1)                              # accumulates
    torch.cuda.synchronize()
    assert rel_l2(dw.cpu().numpy(), 2 * dw_ref) <= TOL
    assert rel_l2(db.cpu().numpy(), 2 * db_ref) <= TOL
    log = check_log(c, "wgrad_s1", 2)
    if not ws:
        assert not any(t.endswith(":slabs") for t in log), log


# ---- 2. unsplit launches: bit for bit the direct kernels; force_direct still wins ------------------------------------------------

@pytest.mark.parametrize("shape", S1_SHAPES)
def test_s1_unsplit_equals_direct_bit_for_bit(gpu, shape):
    """no workspace -> ksplit = 1: every output is direct_conv_s1_kernel's fmaf chain, forward (bias + ReLU) and input gradient
    (masked + accumulated, and plain).  The same calls on a force_direct context log no f32mfma token."""
    B, H, W, Cin, Cout, ks = shape
    rng = np.random.default_rng(7)
    x = f32(rng.standard_normal((B, H, W, Cin)), gpu)
    xr = torch.relu(x)
    w = f32(rng.standard_normal((ks, ks, Cin, Cout)) * 0.1, gpu)
    b = f32(rng.standard_normal(Cout), gpu)
    dz = f32(rng.standard_normal((B, H, W, Cout)), gpu)
    prev = f32(rng.standard_normal((B, H, W, Cin)), gpu)
    outs = []
    for direct in (False, True):
        c = make_ctx(gpu, ws=False, direct=direct)
        y = torch.empty(B, H, W, Cout, device=gpu)
        call_fwd(c, x.data_ptr(), Cin, w, b, y.data_ptr(), Cout, shape, 1)
        d1 = prev.clone()
        call_dgrad(c, dz.data_ptr(), Cout, w, xr.data_ptr(), Cin, d1.data_ptr(), Cin, shape, 1)
        d2 = torch.empty_like(prev)
        call_dgrad(c, dz.data_ptr(), Cout, w, None, 0, d2.data_ptr(), Cin, shape, 0)
        dw = torch.empty(ks, ks, Cin, Cout, device=gpu)
        call_wgrad(c, x, Cin, dz, Cout, dw, None, shape, 0)
        torch.cuda.synchronize()
        log = c.read_launch_log()
        if direct:
            assert not any(t.startswith("f32mfma:") for t in log), log
        else:
            assert log[:3] == ["f32mfma:s1:ksplit=1", "f32mfma:s1t:ksplit=1", "f32mfma:s1t:ksplit=1"], log
            assert len(log) == 4 and log[3].startswith("f32mfma:wgrad_s1:"), log
        outs.append((y, d1, d2, dw))
    for name, a, r in zip(("fwd", "dgrad masked + accumulate", "dgrad"), outs[0][:3], outs[1][:3]):
        if not torch.equal(a, r):
            ulp = (a.view(torch.int32).long() - r.view(torch.int32).long()).abs().max().item()
            pytest.fail(f"{name}: MFMA != direct, max {ulp} ulp")
    assert rel_l2(outs[0][3].cpu().numpy(), outs[1][3].cpu().numpy()) <= TOL


# ---- 3. split launches: deterministic, and no farther from fp64 than the unsplit chain ---------------------------------------------
# An unsplit launch sums each output as ONE fmaf chain (here up to 4608 products for the forward / input gradient, 4096 pixels for the
# weight gradient); that chain's own rounding is ~1e-6 rel-L2 of the fp64 result, and it is what a split launch differs from it by
# (measured: split-K 1.02e-6, weight-gradient slabs 1.15e-6 rel-L2; test_f32_matrix_gpu.py's 1e-6 holds there because its split-K
# shape sums ~1000 products).  So the ordered slabs are held to the fp64 oracle: within TOL, no farther than the unsplit launch, and
# within TOL of it.

def check_split(split, unsplit, ref):
    e_split, e_unsplit = rel_l2(split, ref), rel_l2(unsplit, ref)
    assert e_split <= TOL and e_unsplit <= TOL and e_split <= e_unsplit, (e_split, e_unsplit)
    assert rel_l2(split, unsplit) <= TOL


def test_s1_splitk_is_deterministic_and_close_to_unsplit(gpu):
    shape = (2, 4, 4, 512, 512, 3)
    B, H, W, Cin, Cout, ks = shape
    rng = np.random.default_rng(8)
    x, w = f32(rng.standard_normal((B, H, W, Cin)), gpu), f32(rng.standard_normal((ks, ks, Cin, Cout)) * 0.05, gpu)
    b, dz = f32(rng.standard_normal(Cout), gpu), f32(rng.standard_normal((B, H, W, Cout)), gpu)
    x64, w64, b64, dz64 = (t.double().cpu().numpy() for t in (x, w, b, dz))
    refs = (V.conv_s1_fwd(x64, w64, b64), V.conv_s1_bwd(x64, w64, dz64)[0])

    def run(c):
        y, d = torch.empty(B, H, W, Cout, device=gpu), torch.empty(B, H, W, Cin, device=gpu)
        call_fwd(c, x.data_ptr(), Cin, w, b, y.data_ptr(), Cout, shape, 0)
        call_dgrad(c, dz.data_ptr(), Cout, w, None, 0, d.data_ptr(), Cin, shape, 0)
        return y, d

    c = make_ctx(gpu, ws=True)
    runs = [run(c) for _ in range(2)]
    torch.cuda.synchronize()
    ks_ = splits(c.read_launch_log())
    assert len(ks_) == 4 and min(ks_) > 1, ks_
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    c1 = make_ctx(gpu, ws=False)
    unsplit = run(c1)
    torch.cuda.synchronize()
    assert c1.read_launch_log() == ["f32mfma:s1:ksplit=1", "f32mfma:s1t:ksplit=1"]
    for a, u, r in zip(runs[0], unsplit, refs):
        check_split(a.cpu().numpy(), u.cpu().numpy(), r)


def test_s1_wgrad_slabs_are_deterministic_and_close_to_unsplit(gpu):
    shape = SLAB_SHAPE
    B, H, W, Cin, Cout, ks = shape
    xb, ldx, dzb, lddz, dw_ref, _ = _wgrad_inputs(gpu, shape, 9)
    c = make_ctx(gpu, ws=True)
    runs = []
    for _ in range(2):
        dw = torch.zeros(ks, ks, Cin, Cout, device=gpu)
        call_wgrad(c, xb, ldx, dzb, lddz, dw, None, shape, 0)
        runs.append(dw)
    torch.cuda.synchronize()
    log = c.read_launch_log()
    assert len(log) == 2 and all(t.endswith(":slabs") for t in log) and min(splits(log)) > 1, log
    assert torch.equal(runs[0], runs[1])
    c1 = make_ctx(gpu, ws=True, tuning=1 << 28)          # forced pixel split 2^0 = 1: one owner per tile
    dw1 = torch.zeros(ks, ks, Cin, Cout, device=gpu)
    call_wgrad(c1, xb, ldx, dzb, lddz, dw1, None, shape, 0)
    torch.cuda.synchronize()
    assert c1.read_launch_log() == ["f32mfma:wgrad_s1:rsplit=1:owner"]
    check_split(runs[0].cpu().numpy(), dw1.cpu().numpy(), dw_ref)


# ---- 4. the variant networks on VariantEngine(f32_matrix=True) ----------------------------------------------------------------------

CASES = [dict(block_depth=1, residual=False, concat=True, objective=None),
         dict(block_depth=0, residual=True, concat=True, objective=dict(predict_x=False)),
         dict(block_depth=2, residual=False, concat=False, objective=dict(ordinary_differential_equation=True)),
         dict(block_depth=1, residual=True, concat=False, objective=dict(predict_x=False, predict_scaled_epsilon=True, prediction_weighting=True))]
REF_WIDTH = dict(size=32, pixel_size=128, max_size=512, octaves=3, batch_size=2)


def variant_engine(cfg, gpu, case, dtype=F32, f32_matrix=True):
    from gan_class_transfer2_amd.variants import VariantEngine
    return VariantEngine(cfg.pixel_size, cfg.max_size, cfg.octaves, case["block_depth"], case["residual"], case["concat"], dtype, gpu,
                         steps=cfg.steps, f32_matrix=f32_matrix, **(case["objective"] or {}))


def conv_nodes(eng):
    """convolutions of the network (every kernel but the Dense(3) head's): each is one forward, one weight-gradient and one
    input-gradient call of a step; the head adds one 1 x 1 input-gradient call"""
    return sum(1 for name, _ in eng.net.specs if name.endswith(".w") and name != "dense.w")


def step_inputs(x, t_int, eps, gpu):
    return torch.tensor(x, dtype=torch.float32, device=gpu), torch.tensor(t_int), torch.tensor(eps, dtype=torch.float32)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_variant_engine_step_f32_matrix_vs_oracle(gpu, case, parity_log):
    c = CASES[case]
    bd, res, cat, obj = c["block_depth"], c["residual"], c["concat"], (c["objective"] or {})
    cfg = O.OracleConfig(size=16, pixel_size=8, max_size=16, octaves=2, batch_size=2)
    params = V.init_variant_params(cfg, bd, res, cat, seed=3)
    x, t_int, eps = O.synthetic_batch(cfg, seed=1)
    loss_ref, _, grads_ref = V.variant_trainer_step(params, x, t_int, eps, cfg, bd, res, cat, obj)
    eng = variant_engine(cfg, gpu, c)
    assert eng.f32_matrix and eng.net.ctx.f32_math == lib().F32_MATH_MFMA
    eng.set_params(params)
    eng.net.ctx.log_launches(True)
    loss = eng.train_step(*step_inputs(x, t_int, eps, gpu), apply=False)
    torch.cuda.synchronize()
    log = eng.net.ctx.read_launch_log()
    assert len(log) == 3 * conv_nodes(eng) + 1 and all(t.startswith("f32mfma:") for t in log), log
    grads = eng.get_grads()
    errs = {k: rel_l2(grads[k], grads_ref[k]) for k in grads}
    lrel = abs(float(loss[0]) - loss_ref) / loss_ref
    parity_log(f"variant_case{case}_f32_matrix", loss_rel=lrel, worst_grad_rel_l2=max(errs.values()), worst_grad=max(errs, key=errs.get))
    assert lrel <= 1e-5 and max(errs.values()) <= 5e-5, errs
    # two optimizer steps against Keras Adam on the oracle's gradients
    p = {k: params[k].astype(np.float32) for k in params}
    m = {k: np.zeros_like(params[k], dtype=np.float32) for k in params}
    v = {k: np.zeros_like(params[k], dtype=np.float32) for k in params}
    eng.set_params(params)
    for step in range(2):
        xs, ts, es = O.synthetic_batch(cfg, seed=10 + step)
        _, _, gr = V.variant_trainer_step({k: p[k].astype(np.float64) for k in p}, xs, ts, es, cfg, bd, res, cat, obj)
        for k in p:
            p[k], m[k], v[k] = O.keras_adam_step(p[k], gr[k], m[k], v[k], step, cfg)
        eng.train_step(*step_inputs(xs, ts, es, gpu))
    torch.cuda.synchronize()
    got = eng.get_params()
    assert eng.iterations == 2
    for k in p:
        assert rel_l2(got[k], p[k]) <= 2e-6, k


def test_variant_step_at_reference_widths_f32_matrix(gpu, parity_log):
    """block_depth = 1 at the reference's channel widths in fp32, matrix cores and direct kernels on the same parameters and batch:
    per tensor (loss, prediction, every gradient) the matrix-core step is at most twice as far from fp64 as the direct step (floor
    1e-5).  The split reductions of the deep 512-channel levels change the order of the sums, nothing else."""
    case = dict(block_depth=1, residual=False, concat=True, objective=None)
    cfg = O.OracleConfig(**REF_WIDTH)
    params = V.init_variant_params(cfg, 1, False, True, seed=5)
    x, t_int, eps = O.synthetic_batch(cfg, seed=2)
    loss_ref, pred_ref, grads_ref = V.variant_trainer_step(params, x, t_int, eps, cfg, 1, False, True, None)
    errs = {}
    for f32m in (True, False):
        eng = variant_engine(cfg, gpu, case, f32_matrix=f32m)
        eng.set_params(params)
        eng.net.ctx.log_launches(True)
        loss = eng.train_step(*step_inputs(x, t_int, eps, gpu), apply=False)
        torch.cuda.synchronize()
        log = eng.net.ctx.read_launch_log()
        if f32m:
            assert len(log) == 3 * conv_nodes(eng) + 1 and all(t.startswith("f32mfma:") for t in log), log
        else:
            assert not any(t.startswith("f32mfma:") for t in log), log
        grads = eng.get_grads()
        errs[f32m] = {"loss": abs(float(loss[0]) - loss_ref) / loss_ref, "pred": rel_l2(eng.last["pred"].cpu().numpy(), pred_ref),
                      **{"grad/" + k: rel_l2(grads[k], grads_ref[k]) for k in grads}}
        del eng
    parity_log("variant_reference_width_f32_matrix", **{"matrix/" + k: e for k, e in errs[True].items()},
               **{"direct/" + k: e for k, e in errs[False].items()})
    for k, e in errs[True].items():
        assert e <= max(2 * errs[False][k], 1e-5), (k, e, errs[False][k])


def test_variant_engine_f32_matrix_needs_f32_and_is_read_only(gpu):
    cfg = O.OracleConfig(size=16, pixel_size=8, max_size=16, octaves=2, batch_size=2)
    with pytest.raises(ValueError):
        variant_engine(cfg, gpu, CASES[0], dtype=BF16)
    eng = variant_engine(cfg, gpu, CASES[0], f32_matrix=False)
    assert eng.f32_matrix is False and eng.net.ctx.f32_math == lib().F32_MATH_DIRECT
    with pytest.raises(AttributeError):
        eng.f32_matrix = True


def test_model_knob_builds_f32_matrix_variant_engine(gpu, monkeypatch):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import model as M
    from gan_class_transfer2_amd.variants import VariantEngine
    g.configure(size=32, pixel_size=16, max_size=32, octaves=3, block_depth=1, compute_dtype=None)
    try:
        monkeypatch.setattr(M, "f32_matrix_cores", True)
        den = g.Denoiser(seed=3)
        eng = den.ensure_engine()
        assert isinstance(eng, VariantEngine) and eng.f32_matrix and eng.net.ctx.f32_math == g._lib.F32_MATH_MFMA
        eng.net.ctx.log_launches(True)
        x = torch.randn(2, 32, 32, 3, device=gpu)
        t = torch.ones(2, 1, 1, 1, dtype=torch.int32, device=gpu)
        y = den((x, t))
        torch.cuda.synchronize()
        assert y.shape == (2, 32, 32, 3)
        log = eng.net.ctx.read_launch_log()
        assert len(log) == conv_nodes(eng) and all(t.startswith("f32mfma:") for t in log), log
    finally:
        g.configure(size=256, pixel_size=128, max_size=512, octaves=6, block_depth=0, compute_dtype=None)


def test_log_sample_on_a_variant_network_follows_the_switch(gpu, parity_log):
    """the sampler runs VariantEngine.predict on the engine's context: with the switch every convolution it launches is an f32mfma
    one, without it none is.  Both samplings start from the same parameters and inputs: measured rel-L2 between the two paths'
    outputs 1.7e-7 at most (fake, step_0.25); the deep levels' forward launches split their reduction, nothing else differs"""
    import gan_class_transfer2_amd as g
    cfg = O.OracleConfig(size=16, pixel_size=8, max_size=16, octaves=2, batch_size=2)
    params = V.init_variant_params(cfg, 1, False, True, seed=4)
    gen = torch.Generator().manual_seed(0)
    image = (torch.rand(1, 16, 16, 3, generator=gen) * 2 - 1).to(gpu)
    example = torch.randn(1, 2, 16, 16, 3, generator=gen).to(gpu)
    dictionary = torch.randn(16, 16, 8, 3, generator=gen).to(gpu)
    res = {}
    for f32m in (True, False):
        eng = variant_engine(cfg, gpu, CASES[0], f32_matrix=f32m)
        eng.set_params(params)
        eng.net.ctx.log_launches(True)
        den = types.SimpleNamespace(ensure_engine=lambda: eng)
        out = g.log_sample(den, image, example, dictionary, steps=6, test_step=2)
        torch.cuda.synchronize()
        res[f32m] = {k: v.cpu().numpy() for k, v in out.items()}
        log = eng.net.ctx.read_launch_log()
        if f32m:
            assert log and all(t.startswith("f32mfma:") for t in log), log
        else:
            assert not any(t.startswith("f32mfma:") for t in log), log
        del eng, den
    assert set(res[True]) == set(res[False])
    errs = {k: rel_l2(res[True][k], res[False][k]) for k in res[False]}
    parity_log("log_sample_variant_f32_matrix_vs_direct", **errs)
    for k, e in errs.items():
        assert e <= 1e-6, (k, e)
