"""fp32 on the matrix cores (gct2_ctx_set_f32_math / UNetEngine(f32_matrix=True) / model.f32_matrix_cores).

Tolerances: the existing fp32 ones (rel-L2 <= 2e-6 per kernel against the fp64 oracle; the train-step bounds of
test_golden_tiny_step_fp32 and test_log_sample_fp32_against_golden).  Unsplit forward / input-gradient launches sum in the direct
kernel's order, so they are compared with the direct kernels for EQUALITY; split launches are compared for run-to-run equality and
against the unsplit result (rel-L2 <= 1e-6).
"""
import gc
import os
import types

import numpy as np
import pytest
import torch

from oracle import denoiser_oracle as O

pytestmark = pytest.mark.gpu

F32 = 0
TOL = 2e-6
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_STEP = os.path.join(HERE, "golden", "tiny_step.npz")
GOLDEN_SAMPLER = os.path.join(HERE, "golden", "tiny_sampler.npz")

# test_kernels_gpu.py's shape set: (B, H, W, Cin, Cout), H / W the big grid
CONV_SHAPES = [
    (2, 8, 8, 64, 128),
    (1, 4, 12, 72, 136),
    (3, 2, 2, 256, 64),
    (2, 16, 16, 3, 8),
    (3, 32, 32, 3, 128),
    (1, 8, 8, 4, 136),
    (1, 6, 10, 5, 7),
]
WGRAD_SHAPES = CONV_SHAPES + [(4, 32, 32, 64, 128)]


@pytest.fixture(autouse=True)
def _collect_engines():
    """engines hold reference cycles (and step plans); collect them here, not inside a later test's graph capture"""
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
    """a call context on the fp32 matrix cores (or forced direct), with or without a 64 MiB workspace, launch log on"""
    c = lib().Context()
    c.set_f32_math(lib().F32_MATH_MFMA)
    if direct:
        c.force_direct(True)
    if tuning:
        c.set_tuning(tuning)
    if ws:
        c._ws = torch.empty(16 << 20, dtype=torch.float32, device=gpu)
        c.set_workspace(c._ws)
        c.set_wgrad_workspace(c._ws)
    c.log_launches(True)
    return c


def assert_mfma_log(c):
    log = c.read_launch_log()
    assert any(t.startswith("f32mfma:") for t in log), log
    assert not any(t.startswith("direct:") for t in log), log
    return log


def ksplit_of(log, form):
    return [int(t.split("=")[1]) for t in log if t.startswith(f"f32mfma:{form}:ksplit=")]


# ---- 1. every 4x4 / stride-2 entry point against the fp64 oracle ---------------------------------------------------------

def conv_fwd(c, x, w, b, shape, relu=1):
    """conv4s2_fwd through views inside wider buffers (ld != C, pointer offsets); returns (output view, whole buffer)"""
    B, H, W, Cin, Cout = shape
    dv = x.device if isinstance(x, torch.Tensor) else None
    ldx, ldy, offx, offy = Cin + 5, Cout + 3, 3, 2
    xb = torch.zeros(B, H, W, ldx, dtype=torch.float32, device=dv)
    xb[..., offx:offx + Cin] = x
    yb = torch.full((B, H // 2, W // 2, ldy), 7.0, dtype=torch.float32, device=dv)
    lib().call("gct2_conv4s2_fwd", c.handle, F32, xb.data_ptr() + 4 * offx, ldx, w.data_ptr(), b.data_ptr(), yb.data_ptr() + 4 * offy, ldy,
               B, H, W, Cin, Cout, relu, stream())
    return yb[..., offy:offy + Cout], yb, offy


@pytest.mark.parametrize("ws", [True, False])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv4s2_fwd_f32_matrix(gpu, shape, relu, ws):
    B, H, W, Cin, Cout = shape
    rng = np.random.default_rng(1)
    x, w = rnd(rng.standard_normal((B, H, W, Cin))), rnd(rng.standard_normal((4, 4, Cin, Cout)) * 0.1)
    b = rnd(rng.standard_normal(Cout))
    ref = O.conv4s2_fwd(x, w, b)
    ref = np.maximum(ref, 0) if relu else ref
    c = make_ctx(gpu, ws)
    out, yb, offy = conv_fwd(c, f32(x, gpu), f32(w, gpu), f32(b, gpu), shape, relu)
    torch.cuda.synchronize()
    assert rel_l2(out.cpu().numpy(), ref) <= TOL
    assert float((yb[..., :offy] - 7).abs().max()) == 0 and float((yb[..., offy + Cout:] - 7).abs().max()) == 0
    assert_mfma_log(c)


@pytest.mark.parametrize("ws", [True, False])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_convT4s2_fwd_f32_matrix(gpu, shape, ws):
    B, H, W, Cin, Cout = shape
    rng = np.random.default_rng(2)
    x, w = rnd(rng.standard_normal((B, H, W, Cin))), rnd(rng.standard_normal((4, 4, Cout, Cin)) * 0.1)
    b = rnd(rng.standard_normal(Cout))
    ref = np.maximum(O.convT4s2_fwd(x, w, b), 0)
    ldx, ldy = Cin + 3, Cout + 5
    xb = torch.zeros(B, H, W, ldx, dtype=torch.float32, device=gpu)
    xb[..., 1:1 + Cin] = f32(x, gpu)
    yb = torch.full((B, 2 * H, 2 * W, ldy), 7.0, dtype=torch.float32, device=gpu)
    wd, bd = f32(w, gpu), f32(b, gpu)
    c = make_ctx(gpu, ws)
    lib().call("gct2_convT4s2_fwd", c.handle, F32, xb.data_ptr() + 4, ldx, wd.data_ptr(), bd.data_ptr(), yb.data_ptr() + 4 * 2, ldy,
               B, H, W, Cin, Cout, 1, stream())
    torch.cuda.synchronize()
    assert rel_l2(yb[..., 2:2 + Cout].cpu().numpy(), ref) <= TOL
    assert float((yb[..., :2] - 7).abs().max()) == 0 and float((yb[..., 2 + Cout:] - 7).abs().max()) == 0
    assert_mfma_log(c)


def _dgrad_case(gpu, entry, shape, accumulate, ws, masked, seed):
    """input gradient through views (ld != C), the act mask (own ld), accumulate, and the fused bias gradient split over db / db2
    (db overwritten, db2 added to)"""
    B, H, W, Cin, Cout = shape
    rng = np.random.default_rng(seed)
    conv = entry == "gct2_conv4s2_dgrad"
    x = rnd(np.maximum(rng.standard_normal((B, H, W, Cin)), 0))
    if conv:
        w = rnd(rng.standard_normal((4, 4, Cin, Cout)) * 0.1)
        dz = rnd(rng.standard_normal((B, H // 2, W // 2, Cout)))
        dx_ref, _, _ = O.conv4s2_bwd(x, w, dz)
    else:
        w = rnd(rng.standard_normal((4, 4, Cout, Cin)) * 0.1)
        dz = rnd(rng.standard_normal((B, 2 * H, 2 * W, Cout)))
        dx_ref, _, _ = O.convT4s2_bwd(x, w, dz)
    prev = rnd(rng.standard_normal(x.shape))
    g = dx_ref * (x > 0) if masked else dx_ref
    ref = g + (prev if accumulate else 0)
    split = Cin // 2
    colsum = g.reshape(-1, Cin).sum(0)
    scale = np.abs(g).reshape(-1, Cin).sum(0).max()       # the column sums cancel: bounded against the sum of magnitudes (as
                                                          # test_dgrad_fused_bias_gradients does, same 2e-5 for fp32)
    lddz, lddx, ldact = Cout + 2, Cin + 3, Cin + 1
    dzb = torch.zeros(*dz.shape[:3], lddz, dtype=torch.float32, device=gpu); dzb[..., 1:1 + Cout] = f32(dz, gpu)
    dxb = torch.full((*x.shape[:3], lddx), 5.0, dtype=torch.float32, device=gpu); dxb[..., 2:2 + Cin] = f32(prev, gpu)
    actb = torch.zeros(*x.shape[:3], ldact, dtype=torch.float32, device=gpu); actb[..., :Cin] = f32(x, gpu)
    wd = f32(w, gpu)
    db = torch.full((max(split, 1),), 3.0, dtype=torch.float32, device=gpu)
    db2 = torch.ones(Cin - split, dtype=torch.float32, device=gpu)
    c = make_ctx(gpu, ws)
    lib().call(entry, c.handle, F32, dzb.data_ptr() + 4, lddz, wd.data_ptr(), actb.data_ptr() if masked else None, ldact,
               dxb.data_ptr() + 8, lddx, B, H, W, Cin, Cout, accumulate, db.data_ptr() if split else None, split, db2.data_ptr(), 2,
               stream())
    torch.cuda.synchronize()
    assert rel_l2(dxb[..., 2:2 + Cin].cpu().numpy(), ref) <= TOL
    assert float((dxb[..., :2] - 5).abs().max()) == 0 and float((dxb[..., 2 + Cin:] - 5).abs().max()) == 0
    if split:
        assert np.abs(db.cpu().numpy() - colsum[:split]).max() <= 2e-5 * scale
    assert np.abs(db2.cpu().numpy() - 1 - colsum[split:]).max() <= 2e-5 * scale
    return assert_mfma_log(c)


@pytest.mark.parametrize("ws", [True, False])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv4s2_dgrad_f32_matrix(gpu, shape, accumulate, ws):
    _dgrad_case(gpu, "gct2_conv4s2_dgrad", shape, accumulate, ws, True, 3)


@pytest.mark.parametrize("ws", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_convT4s2_dgrad_f32_matrix(gpu, shape, masked, ws):
    _dgrad_case(gpu, "gct2_convT4s2_dgrad", shape, 1, ws, masked, 4)


def _wgrad_call(c, entry, x, ldx, dz, lddz, dw, db, shape, accumulate):
    B, H, W, Cin, Cout = shape
    lib().call(entry, c.handle, F32, x.data_ptr(), ldx, dz.data_ptr(), lddz, dw.data_ptr(), db.data_ptr() if db is not None else None,
               B, H, W, Cin, Cout, accumulate, None, stream())


def _wgrad_inputs(gpu, entry, shape, seed):
    B, H, W, Cin, Cout = shape
    rng = np.random.default_rng(seed)
    x = rnd(rng.standard_normal((B, H, W, Cin)))
    if entry == "gct2_conv4s2_wgrad":
        dz = rnd(rng.standard_normal((B, H // 2, W // 2, Cout)))
        _, dw_ref, db_ref = O.conv4s2_bwd(x, np.zeros((4, 4, Cin, Cout)), dz)
    else:
        dz = rnd(rng.standard_normal((B, 2 * H, 2 * W, Cout)))
        _, dw_ref, db_ref = O.convT4s2_bwd(x, np.zeros((4, 4, Cout, Cin)), dz)
    ldx, lddz = Cin + 1, Cout + 4
    xb = torch.zeros(*x.shape[:3], ldx, dtype=torch.float32, device=gpu); xb[..., :Cin] = f32(x, gpu)
    dzb = torch.zeros(*dz.shape[:3], lddz, dtype=torch.float32, device=gpu); dzb[..., :Cout] = f32(dz, gpu)
    return xb, ldx, dzb, lddz, dw_ref, db_ref


@pytest.mark.parametrize("ws", [True, False])
@pytest.mark.parametrize("entry", ["gct2_conv4s2_wgrad", "gct2_convT4s2_wgrad"])
@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad_f32_matrix(gpu, shape, entry, ws):
    B, H, W, Cin, Cout = shape
    xb, ldx, dzb, lddz, dw_ref, db_ref = _wgrad_inputs(gpu, entry, shape, 5)
    wshape = (4, 4, Cin, Cout) if entry == "gct2_conv4s2_wgrad" else (4, 4, Cout, Cin)
    dw = torch.full(wshape, 9.0, dtype=torch.float32, device=gpu)      # overwritten (accumulate = 0)
    db = torch.full((Cout,), 9.0, dtype=torch.float32, device=gpu)
    c = make_ctx(gpu, ws)
    _wgrad_call(c, entry, xb, ldx, dzb, lddz, dw, db, shape, 0)
    torch.cuda.synchronize()
    assert rel_l2(dw.cpu().numpy(), dw_ref) <= TOL
    assert rel_l2(db.cpu().numpy(), db_ref) <= TOL
    _wgrad_call(c, entry, xb, ldx, dzb, lddz, dw, db, shape, 1)          # accumulates
    torch.cuda.synchronize()
    assert rel_l2(dw.cpu().numpy(), 2 * dw_ref) <= TOL
    assert rel_l2(db.cpu().numpy(), 2 * db_ref) <= TOL
    log = assert_mfma_log(c)
    assert all(t.startswith("f32mfma:wgrad:rsplit=") for t in log), log
    if not ws:
        assert not any(t.endswith(":slabs") for t in log), log


def test_wgrad_tall_skinny_levels_f32_matrix(gpu):
    """the image layer (Cb = 3: big = the image, small = its 128-channel gradient) and UpShuffle_0's shape (Cb = 64, Cs = 192) over
    many pixels: both split the pixel range into ordered slabs"""
    for entry, shape in (("gct2_conv4s2_wgrad", (8, 64, 64, 3, 128)), ("gct2_convT4s2_wgrad", (4, 32, 32, 192, 64))):
        xb, ldx, dzb, lddz, dw_ref, _ = _wgrad_inputs(gpu, entry, shape, 6)
        dw = torch.zeros(dw_ref.shape, dtype=torch.float32, device=gpu)
        c = make_ctx(gpu, True)
        _wgrad_call(c, entry, xb, ldx, dzb, lddz, dw, None, shape, 0)
        torch.cuda.synchronize()
        assert rel_l2(dw.cpu().numpy(), dw_ref) <= TOL, entry
        log = assert_mfma_log(c)
        assert any(t.endswith(":slabs") and int(t.split("=")[1].split(":")[0]) > 1 for t in log), log


# ---- 2. unsplit tap GEMMs: bit for bit the direct kernels -------------------------------------------------------------------

@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_unsplit_tapgemm_equals_direct_bit_for_bit(gpu, shape):
    """no workspace -> ksplit = 1: every output is the direct kernel's fmaf chain (v_mfma_f32_16x16x4_f32 = k-ordered fmaf), for
    both forms and both epilogues, ragged K / N included"""
    B, H, W, Cin, Cout = shape
    rng = np.random.default_rng(7)
    x = f32(rng.standard_normal((B, H, W, Cin)), gpu)
    xr = torch.relu(x)
    wc = f32(rng.standard_normal((4, 4, Cin, Cout)) * 0.1, gpu)
    wt = f32(rng.standard_normal((4, 4, Cout, Cin)) * 0.1, gpu)
    b = f32(rng.standard_normal(Cout), gpu)
    dz_s = f32(rng.standard_normal((B, H // 2, W // 2, Cout)), gpu)
    dz_b = f32(rng.standard_normal((B, 2 * H, 2 * W, Cout)), gpu)
    prev = f32(rng.standard_normal((B, H, W, Cin)), gpu)
    outs = []
    for direct in (False, True):
        c = make_ctx(gpu, ws=False, direct=direct)
        y1 = torch.empty(B, H // 2, W // 2, Cout, device=gpu)
        lib().call("gct2_conv4s2_fwd", c.handle, F32, x.data_ptr(), Cin, wc.data_ptr(), b.data_ptr(), y1.data_ptr(), Cout, B, H, W, Cin, Cout,
                   1, stream())
        y2 = torch.empty(B, 2 * H, 2 * W, Cout, device=gpu)
        lib().call("gct2_convT4s2_fwd", c.handle, F32, x.data_ptr(), Cin, wt.data_ptr(), b.data_ptr(), y2.data_ptr(), Cout, B, H, W, Cin, Cout,
                   0, stream())
        d1 = prev.clone()
        lib().call("gct2_conv4s2_dgrad", c.handle, F32, dz_s.data_ptr(), Cout, wc.data_ptr(), xr.data_ptr(), Cin, d1.data_ptr(), Cin,
                   B, H, W, Cin, Cout, 1, None, 0, None, 0, stream())
        d2 = torch.empty_like(prev)
        lib().call("gct2_convT4s2_dgrad", c.handle, F32, dz_b.data_ptr(), Cout, wt.data_ptr(), xr.data_ptr(), Cin, d2.data_ptr(), Cin,
                   B, H, W, Cin, Cout, 0, None, 0, None, 0, stream())
        torch.cuda.synchronize()
        log = c.read_launch_log()
        if direct:
            assert log.count("direct:tap") == 4, log
        else:
            assert ksplit_of(log, "conv") == [1, 1] and ksplit_of(log, "convT") == [1, 1], log
        outs.append((y1, y2, d1, d2))
    for name, a, r in zip(("conv fwd", "convT fwd", "conv dgrad", "convT dgrad"), outs[0], outs[1]):
        if not torch.equal(a, r):
            ulp = (a.view(torch.int32).long() - r.view(torch.int32).long()).abs().max().item()
            pytest.fail(f"{name}: MFMA != direct, max {ulp} ulp")


# ---- 3. split launches: deterministic, close to unsplit --------------------------------------------------------------------

def test_splitk_is_deterministic_and_close_to_unsplit(gpu):
    shape = (3, 2, 2, 256, 64)          # 12 output pixels: the reduction is split
    B, H, W, Cin, Cout = shape
    rng = np.random.default_rng(8)
    x, w, b = f32(rng.standard_normal((B, H, W, Cin)), gpu), f32(rng.standard_normal((4, 4, Cin, Cout)) * 0.1, gpu), f32(rng.standard_normal(Cout), gpu)
    c = make_ctx(gpu, ws=True)
    runs = [conv_fwd(c, x, w, b, shape, 0)[0].clone() for _ in range(2)]
    torch.cuda.synchronize()
    ks = ksplit_of(c.read_launch_log(), "conv")
    assert len(ks) == 2 and ks[0] > 1, ks
    assert torch.equal(runs[0], runs[1])
    c1 = make_ctx(gpu, ws=False)
    unsplit = conv_fwd(c1, x, w, b, shape, 0)[0]
    torch.cuda.synchronize()
    assert ksplit_of(c1.read_launch_log(), "conv") == [1]
    assert rel_l2(runs[0].cpu().numpy(), unsplit.cpu().numpy()) <= 1e-6


def test_wgrad_slabs_are_deterministic_and_close_to_unsplit(gpu):
    shape, entry = (4, 32, 32, 64, 128), "gct2_conv4s2_wgrad"
    xb, ldx, dzb, lddz, _, _ = _wgrad_inputs(gpu, entry, shape, 9)
    c = make_ctx(gpu, ws=True)
    runs = []
    for _ in range(2):
        dw = torch.zeros(4, 4, 64, 128, device=gpu)
        _wgrad_call(c, entry, xb, ldx, dzb, lddz, dw, None, shape, 0)
        runs.append(dw)
    torch.cuda.synchronize()
    log = c.read_launch_log()
    assert len(log) == 2 and log[0].endswith(":slabs") and not log[0].startswith("f32mfma:wgrad:rsplit=1:"), log
    assert torch.equal(runs[0], runs[1])
    c1 = make_ctx(gpu, ws=True, tuning=1 << 28)          # forced pixel split 2^0 = 1: one owner per tile
    dw1 = torch.zeros(4, 4, 64, 128, device=gpu)
    _wgrad_call(c1, entry, xb, ldx, dzb, lddz, dw1, None, shape, 0)
    torch.cuda.synchronize()
    assert c1.read_launch_log() == ["f32mfma:wgrad:rsplit=1:owner"]
    assert rel_l2(runs[0].cpu().numpy(), dw1.cpu().numpy()) <= 1e-6


# ---- 4 - 6. train steps -------------------------------------------------------------------------------------------------

def make_engine(cfg, gpu, f32_matrix=True, **kw):
    import gan_class_transfer2_amd as g
    topo = g.Topology(cfg.pixel_size, cfg.max_size, cfg.octaves)
    eng = g.UNetEngine(topo, F32, gpu, steps=cfg.steps, base_lr=cfg.base_lr, warm_up=cfg.warm_up, f32_matrix=f32_matrix, **kw)
    eng.keep_pred = True
    return eng


def test_golden_tiny_step_f32_matrix(gpu):
    """test_golden_tiny_step_fp32's assertions with the fp32 matrix-core kernels"""
    z = np.load(GOLDEN_STEP)
    cfg = O.OracleConfig(size=16, pixel_size=8, max_size=16, octaves=2, batch_size=2)
    eng = make_engine(cfg, gpu)
    assert eng.f32_matrix
    eng.ctx.log_launches(True)
    eng.ctx_tail.log_launches(True)
    names = list(eng.arena.shapes)
    eng.set_params({k: z["param/" + k] for k in names})
    x = torch.tensor(z["x"], dtype=torch.float32, device=gpu)
    loss = eng.train_step(x, torch.tensor(z["t_int"]), torch.tensor(z["eps"], dtype=torch.float32), apply=False)
    torch.cuda.synchronize()
    log = eng.read_launch_log()
    for kind in ("f32mfma:conv:", "f32mfma:convT:", "f32mfma:wgrad:"):
        assert any(t.startswith(kind) for t in log), (kind, log)
    assert not any(t.startswith("direct:") for t in log), log
    b = eng.buffers(2, 16, 16)
    assert abs(float(loss[0]) - float(z["loss"])) <= 1e-5 * float(z["loss"])
    assert rel_l2(b.pred.cpu().numpy(), z["pred"]) <= 2e-5
    fu0 = eng.topo.fu(0)
    assert rel_l2(b.R[0][..., fu0:fu0 + 3].cpu().numpy(), z["noised"]) <= 1e-6
    grads = eng.get_grads()
    for k in names:
        assert rel_l2(grads[k], z["grad/" + k]) <= 2e-5, k
    eng.arena.g.fill_(float("nan"))
    eng.set_params({k: z["param/" + k] for k in names})
    losses = []
    for step in range(2):
        xs, ts, es = O.synthetic_batch(cfg, seed=step)
        losses.append(eng.train_step(torch.tensor(xs, dtype=torch.float32, device=gpu), torch.tensor(ts),
                                     torch.tensor(es, dtype=torch.float32)).clone())
    torch.cuda.synchronize()
    assert eng.iterations == 2
    assert np.allclose([float(l[0]) for l in losses], z["losses2"], rtol=1e-5)
    for k in names:
        assert rel_l2(eng.arena.param(k).cpu().numpy(), z["param2/" + k]) <= 1e-6, k
        upd, upd_ref = eng.arena.param(k).cpu().numpy().astype(np.float64) - z["param/" + k], z["param2/" + k] - z["param/" + k]
        assert rel_l2(upd, upd_ref) <= 2e-3, k
        assert rel_l2(eng.arena.slot_m(k).cpu().numpy(), z["m2/" + k]) <= 5e-5, k
        assert rel_l2(eng.arena.slot_v(k).cpu().numpy(), z["v2/" + k]) <= 5e-5, k
    assert not any(t.startswith("direct:") for t in eng.read_launch_log())


def test_config2_f32_matrix_vs_direct(gpu, parity_log):
    """config 2 at size (3x64x64, bs 32): one step on the matrix cores against one on the direct kernels, same params and batch, and
    both against the fp64 oracle.  The forward pass is the direct kernels' fmaf chain (loss: measured equal); the gradients differ
    by the split reductions' order: measured matrix vs direct <= 2.7e-4 rel-L2 per tensor (deep levels), where EACH path lies
    3.6e-4 .. 8.6e-4 from fp64 (fp32 through 12 layers), the matrix path at most 1.14x the direct path's distance.  Bounds: loss
    1e-6 rel; per gradient 5e-4 from the direct path and at most 1.25x the direct path's distance from fp64 (+1e-6)."""
    cfg = O.OracleConfig(size=64, batch_size=32, octaves=6)
    params = O.init_params(cfg, seed=1234, dtype=np.float32)
    x, t_int, eps = O.synthetic_batch(cfg, seed=0, dtype=np.float32)
    out = []
    for f32m in (True, False):
        eng = make_engine(cfg, gpu, f32_matrix=f32m)
        eng.set_params(params)
        eng.ctx.log_launches(True)
        loss = eng.train_step(torch.tensor(x, dtype=torch.float32, device=gpu), torch.tensor(t_int),
                              torch.tensor(eps, dtype=torch.float32), apply=False)
        torch.cuda.synchronize()
        log = eng.read_launch_log()
        assert any(t.startswith("f32mfma:") for t in log) == f32m and any(t.startswith("direct:") for t in log) != f32m
        out.append((float(loss[0]), eng.get_grads()))
        del eng
    (l_m, g_m), (l_d, g_d) = out
    errs = {k: rel_l2(g_m[k], g_d[k]) for k in g_d}
    _, _, g_ref, _ = O.trainer_step({k: v.astype(np.float64) for k, v in params.items()}, x.astype(np.float64), t_int,
                                    eps.astype(np.float64), cfg)
    err_m = {k: rel_l2(g_m[k], g_ref[k]) for k in g_ref}
    err_d = {k: rel_l2(g_d[k], g_ref[k]) for k in g_ref}
    parity_log("config2_f32_matrix_vs_direct", loss_rel=abs(l_m - l_d) / l_d, **{"vs_direct/" + k: e for k, e in errs.items()},
               **{"matrix_vs_fp64/" + k: e for k, e in err_m.items()}, **{"direct_vs_fp64/" + k: e for k, e in err_d.items()})
    assert abs(l_m - l_d) <= 1e-6 * l_d, (l_m, l_d)
    for k, e in errs.items():
        assert e <= 5e-4 and err_m[k] <= 1.25 * err_d[k] + 1e-6, (k, e, err_m[k], err_d[k])


def test_planned_step_equals_eager_step_f32_matrix(gpu, parity_log):
    """a replayed step plan against the same steps run call by call: losses, counters and RNG positions EQUAL.  The fp32 bias
    gradients are column sums with fp32 atomics (pw_colsum, the direct path's too), so the arenas after six Adam steps are compared
    to rel-L2 1e-6 (recorded in the parity log)"""
    cfg = O.OracleConfig(size=64, pixel_size=128, max_size=512, octaves=4, batch_size=4)
    params = O.init_params(cfg, seed=3)
    xs = [torch.tensor(O.synthetic_batch(cfg, seed=k)[0], dtype=torch.float32, device=gpu) for k in range(3)]
    out = []
    for use_plan in (False, True):
        eng = make_engine(cfg, gpu, rng_seed=5)
        eng.use_plan = use_plan
        eng.set_params(params)
        losses = [eng.train_step(xs[k % 3]).clone() for k in range(6)]
        torch.cuda.synchronize()
        if use_plan:
            assert len(eng._plans) >= 1
        else:
            assert not eng._plans
        out.append((torch.cat(losses), {n: getattr(eng.arena, n).clone() for n in ("p", "m", "v")},
                    (eng.iterations, eng.rng_offset_t, eng.rng_offset_eps)))
    assert torch.equal(out[0][0], out[1][0]), (out[0][0], out[1][0])
    assert out[0][2] == out[1][2]
    diffs = {n: rel_l2(out[1][1][n].cpu().numpy(), out[0][1][n].cpu().numpy()) for n in ("p", "m", "v")}   # (fp32: no 16-bit shadow)
    parity_log("planned_vs_eager_f32_matrix", **diffs)
    for n, e in diffs.items():
        assert e <= 1e-6, (n, e)


# ---- 7. sampler ----------------------------------------------------------------------------------------------------------

SWITCHES = {"default": {}, "eps": dict(predict_x=False), "scaled_eps": dict(predict_x=False, predict_scaled_epsilon=True),
            "ode": dict(ordinary_differential_equation=True)}


@pytest.mark.parametrize("mode", list(SWITCHES))
def test_log_sample_f32_matrix_against_golden(gpu, mode, parity_log):
    import gan_class_transfer2_amd as g
    z = np.load(GOLDEN_SAMPLER)
    eng = g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=6, f32_matrix=True, **SWITCHES[mode])
    eng.set_params({k[6:]: z[k] for k in z.files if k.startswith("param/")})
    eng.ctx.log_launches(True)
    den = types.SimpleNamespace(ensure_engine=lambda: eng)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
    res = g.log_sample(den, t(z["example_image"]), t(z["example"]), t(z["dictionary"]), steps=6, test_step=2, **SWITCHES[mode])
    torch.cuda.synchronize()
    prefix = "out/" if mode == "default" else f"mode/{mode}/"
    want = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}
    assert set(res) == set(want)
    errs = {}
    for k, v in res.items():
        ref = want[k]
        errs[k] = rel_l2(v.cpu().numpy().reshape(ref.shape), ref)
    parity_log(f"log_sample_f32_matrix_{mode}", **errs)
    for k, e in errs.items():
        assert e <= 2e-5, (mode, k, e)
    log = eng.read_launch_log()
    assert any(t.startswith("f32mfma:") for t in log) and not any(t.startswith("direct:") for t in log), log


# ---- 8. the model knob -----------------------------------------------------------------------------------------------------

def test_model_knob_builds_f32_matrix_engine(gpu, monkeypatch):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import model as M
    g.configure(size=32, pixel_size=16, max_size=32, octaves=3, compute_dtype="float32")
    try:
        monkeypatch.setattr(M, "f32_matrix_cores", True)
        den = g.Denoiser(seed=3)
        eng = den.ensure_engine()
        assert eng.f32_matrix and eng.ctx.f32_math == g._lib.F32_MATH_MFMA and eng.ctx_tail.f32_math == g._lib.F32_MATH_MFMA
        eng.ctx.log_launches(True)
        x = torch.randn(2, 32, 32, 3, device=gpu)
        t = torch.ones(2, 1, 1, 1, dtype=torch.int32, device=gpu)
        y = den((x, t))
        torch.cuda.synchronize()
        assert y.shape == (2, 32, 32, 3)
        log = eng.read_launch_log()
        assert any(t.startswith("f32mfma:") for t in log) and not any(t.startswith("direct:") for t in log), log
        with pytest.raises(AttributeError):
            eng.f32_matrix = False
    finally:
        g.configure(size=256, pixel_size=128, max_size=512, octaves=6, compute_dtype=None)
    with pytest.raises(ValueError):
        g.UNetEngine(g.Topology(8, 16, 2), g.BF16, gpu, f32_matrix=True)
