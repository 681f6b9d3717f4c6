"""Every view-taking kernel on ONE operand whose byte offsets reach 2^31, 2^32 or 2^33 (tests/large_view_cases.py), per element.

The library bounds pixel counts, not strides: a [4, 16, 16, 8] view with ld = 2^20 is a valid operand that spans 2 GiB.  Each case
gives one view of a call such a stride and compares the result bit by bit with the COMPACT case's fp64 reference rounded once
(tests/exact_cases.py: `ld` is not part of a case) - a dropped (size_t) cast, a 32-bit buffer offset taken past its range or a
predicate that admits too much gives values that depend on the image index.  As in tests/test_kernels_exact_gpu.py, whose runners
these are: inputs sit in NaN, outputs in a sentinel (one guard row in front of and behind a wide view), everything outside an output
view is proven untouched (on the device: only the gathered view comes to the host), and the launch log must show the family the
case is meant for - at T0 the matrix-core kernel, at T0+ and beyond the direct one.  A case holds at most 10 GiB and frees it before
it returns.  What each case ran, spanned, held and took is printed, and merged into the JSON file that the environment variable
GCT2_LARGE_VIEWS_LOG names when it is set (profiles/large_views.json is a copy of such a file).

Refusals asserted instead of runs: gct2_convT4s2_fwd_head_train with a source at or beyond its bound (GCT2_EINVAL, dy untouched);
gct2_dense_head_train bounds ldx by its LDS tile, and a 2-GiB x at that stride has 4.5 million pixels - beyond the exact inputs; its dx
and x2, which it does not bound, are run wide.
"""
import ctypes
import gc
import json
import os
import time

import numpy as np
import pytest
import torch

import exact_cases as E
import large_view_cases as L
import noise_schedule_cases as N
import pointwise_cases as P
from exact_cases import BF16, F16, F32, SENTINEL
from oracle import denoiser_oracle as O
from test_kernels_exact_gpu import FN, MODE_DT, Out, Place, check_log, dev, lib, make_ctx, nan_like, run_dgrad, run_fwd, run_s1, run_wgrad, stream

pytestmark = pytest.mark.gpu

NAN = float("nan")
HEAD_ROW = 288
EINVAL = 1


# ---- placement of the one wide view ---------------------------------------------------------------------------------------------------

class WideOut:
    """an output view with a stride of millions of elements inside a sentinel-filled flat buffer (exact_cases.wide_view)"""

    def __init__(self, init, ld):
        self.buf, self.view, self.ptr = E.wide_view(init, ld, SENTINEL)

    def got(self):
        return self.view.contiguous()

    def check(self, want, what, names=("b", "h", "w", "c")):
        """the gathered view bit by bit, then - the view masked - nothing else of the buffer changed; consumes the buffer's contents"""
        torch.cuda.synchronize()
        E.assert_elementwise_equal(self.got(), want, names, what)
        E.assert_outside_untouched_device(self.buf, self.view, SENTINEL, what)


class Wide(Place):
    """tests/test_kernels_exact_gpu.py's placement with ONE role at the case's stride"""

    def __init__(self, c):
        self.role, self.ld = c.role, c.ld

    def inp(self, role, t, mode, kind):
        if role != self.role:
            if kind == "x2":                               # the packed image of the fused head: rows of 4 elements, NaN in slot 3
                buf, ptr = E.poisoned_view(t, 4, 0)
                return buf, ptr, 4
            return super().inp(role, t, mode, kind)
        buf, view, ptr = E.wide_view(t, self.ld)
        return buf, ptr, self.ld

    def out(self, role, init, mode):
        if role != self.role:
            return super().out(role, init, mode)
        return WideOut(init, self.ld), self.ld


@pytest.fixture
def view_log(request):
    """record(case, log): family, span, device bytes held (the allocator's peak during the test) and wall time of one case: printed,
    and merged into the JSON file named by GCT2_LARGE_VIEWS_LOG when that is set.  No test asserts a bound on the time."""
    path = os.environ.get("GCT2_LARGE_VIEWS_LOG")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()

    done = []

    def record(c, log):
        done.append(c.id)
        torch.cuda.synchronize()
        held = torch.cuda.max_memory_allocated() - base
        assert held <= L.MAX_DEVICE_BYTES, f"{c.id} held {held / 2 ** 30:.2f} GiB"
        entry = dict(family=";".join(sorted(set(log))) if log else "", span_bytes=c.span, ld=c.ld, device_bytes_held=held,
                     wall_seconds=float("%.3g" % (time.perf_counter() - t0)))
        print(f"{c.id}: {entry}")
        if not path:
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        try:
            with open(path) as f:
                data = json.load(f)
        except (OSError, ValueError):
            data = {}
        data[c.id] = entry
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)

    yield record
    gc.collect()
    torch.cuda.empty_cache()
    if done:                                  # (a failed case's traceback keeps its tensors alive: only a case that reached its end is asked)
        assert torch.cuda.memory_allocated() <= base + (1 << 20), "a case kept device memory"


def params(cases):
    return [pytest.param(c, id=c.id) for c in cases]


# ---- layer entry points ----------------------------------------------------------------------------------------------------------------

def run_layer(gpu, c):
    """one layer case through the runner of its entry point; returns the launch log"""
    place = Wide(c)
    if c.kind == "s1":
        kw = dict(variants=c.variants) if c.entry != "s1_wgrad" else {}
        return run_s1(gpu, c.entry, c.shape, c.mode, c.ws, place=place, prefix=c.family, **kw)
    if c.entry.endswith("_wgrad"):
        ctx = run_wgrad(gpu, c.entry, c.shape, c.mode, c.ws, c.tuning, place=place)
        return check_log(ctx, c.family, c.contains)
    run = run_fwd if c.entry.endswith("_fwd") else run_dgrad
    kw = dict(variants=c.variants) if c.variants else {}
    return run(gpu, c.entry, c.shape, c.mode, ws=c.ws, tuning=c.tuning, contains=c.contains, split=c.split, place=place, family=c.family, **kw)


@pytest.mark.parametrize("c", params(L.layer_cases()))
def test_layer_entry_points_with_one_wide_view(gpu, c, view_log):
    """conv4s2, convT4s2 and conv2d_s1 (KS = 3), forward, input gradient and weight gradient: source / output (also accumulating) /
    act / both operands of a weight gradient, 16-bit at T0 .. T3, fp32 (direct and matrix cores) at T2 and T3"""
    log = run_layer(gpu, c)
    if c.tier == "T0":
        assert log and all(t.startswith(("tap:", "halo:", "wgrad:")) for t in log), log
    if c.tier == "T0+":
        assert not any(t.startswith(("tap:", "halo:", "wgrad:")) for t in log), log
    view_log(c, log)


@pytest.mark.parametrize("c", params(L.many_pixel_cases()))
def test_many_pixels_modest_ld(gpu, c, view_log):
    """5 x 512 x 512 source pixels: the source of conv_fwd and conv_wgrad at ld = 1024 (the direct kernels: the matrix-core predicates
    refuse a source of that size), the 5 x 1024 x 1024 output of the halo kernel at ld = 256 - image 4 of the wide view starts
    exactly at 2^31 bytes.  The fp64 reference is computed in full on the CPU (exact_cases.make_case at this shape)."""
    log = run_layer(gpu, c)
    view_log(c, log)


# ---- ReLU bit planes and the fused bias gradients of a direct input gradient -----------------------------------------------------------------

def packbits(a):
    """bit k of byte c <-> channel 8c + k (include/gct2.h, gct2_ctx_set_relu_bits)"""
    C = a.shape[-1]
    return torch.tensor(np.packbits((a > 0).reshape(-1, C), axis=1, bitorder="little").reshape(*a.shape[:-1], C // 8))


@pytest.mark.parametrize("c", params(L.plane_cases()))
def test_relu_bit_plane_spanning_more_than_4_gib(gpu, c, view_log):
    """the plane [pixels][ld_bytes] is the wide operand: written by the 16-byte epilogues (tap GEMM, halo kernel), derived from the
    stored y by the extra launch (fp32 direct kernels), and read as the ReLU mask of an input gradient (the halo kernel, handed an
    all-positive act with the real mask in the plane)"""
    dt = c.dt
    cs = E.make_case(c.entry, c.shape, dt)
    B, H, W, Cin, Cout = c.shape
    ctx = make_ctx(gpu, c.mode, False, c.tuning)
    place = Place()
    wb, wp = E.guarded(dev(cs.w, dt, gpu))
    if c.entry.endswith("_fwd"):
        want_y = E.expected(np.maximum(cs.ref, 0), dt)
        pb, pview, pptr = E.wide_view(torch.full((*cs.ref.shape[:-1], Cout // 8), 0xA5, dtype=torch.uint8, device=gpu), c.ld, 0xA5)
        xb, xp, ldx = place.inp("x", dev(cs.x, dt, gpu), c.mode, "in")
        bb, bp = E.guarded(dev(cs.bias, F32, gpu))
        y, ldy = place.out("y", nan_like(cs.ref.shape, dt, gpu), c.mode)
        lib().call("gct2_ctx_set_relu_bits", ctx.handle, pptr, c.ld)
        lib().call(FN[c.entry], ctx.handle, dt, xp, ldx, wp, bp, y.ptr, ldy, B, H, W, Cin, Cout, 1, stream())
        y.check(want_y, c.id + " y")
        E.assert_elementwise_equal(pview.contiguous().cpu().to(torch.int32), packbits(want_y.float().numpy()).to(torch.int32), what=c.id + " plane")
        assert 0.2 < float((want_y > 0).float().mean()) < 0.8                # a real mask
        pview.fill_(0xA5)                                                    # the plane masked: every other byte is as it was
        assert all(bool((piece == 0xA5).all()) for piece in pb.split(1 << 28)), "bytes outside the plane changed"
        del pb, pview
        log = ctx.read_launch_log()
        assert ("relu_bits:derived" in log) == (c.tag == "derived"), log
        assert [t for t in log if not t.startswith("relu_bits:")][0].startswith(c.family), log
        if c.tag == "written":
            assert any(t.endswith(":bits") for t in log), log
    else:
        want = E.expected(E.dgrad_ref(cs, 1, 0), dt)
        bits = packbits(cs.act).to(gpu)
        pb, pview, pptr = E.wide_view(bits, c.ld, 0xFF)                   # (around the plane: all ones - a read beside it unmasks)
        dzb, dzp, lddz = place.inp("dz", dev(cs.dz, dt, gpu), c.mode, "in")
        ones, op, ldact = place.inp("act", torch.ones(cs.act.shape, dtype=E.TDT[dt], device=gpu), c.mode, "act")
        dx, lddx = place.out("dx", nan_like(cs.prev.shape, dt, gpu), c.mode)
        lib().call("gct2_ctx_set_relu_bits", ctx.handle, pptr, c.ld)
        lib().call(FN[c.entry], ctx.handle, dt, dzp, lddz, wp, op, ldact, dx.ptr, lddx, B, H, W, Cin, Cout, 0, None, 0, None, 0, stream())
        dx.check(want, c.id + " dx")
        assert 0.2 < float((cs.act > 0).mean()) < 0.8
        log = check_log(ctx, c.family)
        del pb, pview
    view_log(c, log)


@pytest.mark.parametrize("c", params(L.colsum_cases()))
def test_fused_bias_gradients_over_a_wide_dx(gpu, c, view_log):
    """a direct input gradient sums its bias gradients from the stored view (pw_colsum): db / db2 over a dx with a stride of millions
    of elements, first call overwriting (over NaN), second accumulating into dx and adding.  Operands from {-1, 0, 1}: every stored
    value is exact, the column sums exact in any order."""
    dt = c.dt
    cs = E.make_case(c.entry, c.shape, dt, "pm1")
    B, H, W, Cin, Cout = c.shape
    split = 8 if Cin > 8 else 4
    g = E.dgrad_ref(cs, 1, 0)
    assert np.abs(2 * g).max() <= 256
    sums = g.reshape(-1, Cin).sum(0)
    ctx = make_ctx(gpu, c.mode)
    place = Wide(c)
    dzb, dzp, lddz = place.inp("dz", dev(cs.dz, dt, gpu), c.mode, "in")
    wb, wp = E.guarded(dev(cs.w, dt, gpu))
    ab, ap, ldact = place.inp("act", dev(cs.act, dt, gpu), c.mode, "act")
    db = Out(nan_like((split,), F32, gpu), 0, 0, guard=True)
    db2 = Out(nan_like((Cin - split,), F32, gpu), 0, 0, guard=True)
    dx, lddx = place.out("dx", nan_like(g.shape, dt, gpu), c.mode)
    for k, (accumulate, db_acc) in enumerate([(0, 0), (1, 3)], 1):
        lib().call(FN[c.entry], ctx.handle, dt, dzp, lddz, wp, ap, ldact, dx.ptr, lddx, B, H, W, Cin, Cout, accumulate, db.ptr, split, db2.ptr,
                   db_acc, stream())
        db.check(E.expected(k * sums[:split], F32), f"{c.id} call {k} db", ("c",))
        db2.check(E.expected(k * sums[split:], F32), f"{c.id} call {k} db2", ("c",))
    dx.check(E.expected(2 * g, dt), c.id + " dx")
    log = check_log(ctx, c.family)
    del dx
    view_log(c, log)


# ---- the fused head ------------------------------------------------------------------------------------------------------------------------

def assert_loss(got, want, what):
    """tests/test_fused_exact_gpu.py: sum d^2 is exact; the rounding of 1 / n and of the result remain: 2 fp32 ulp"""
    ulp = float(np.spacing(np.float32(want)))
    print(f"{what}: loss {got!r} want {want!r} ({abs(got - want) / ulp:.3f} ulp)")
    assert abs(got - want) <= 2 * ulp, (what, got, want)


@pytest.mark.parametrize("c", params(L.head_cases()))
def test_convT_fwd_head_train_with_one_wide_view(gpu, c, view_log):
    """gct2_convT4s2_fwd_head_train: the source at the largest stride its bound admits, dy at T1 .. T3, the packed image at T1 and T2
    - pred, dy, db, head_dw, head_db bit for bit, the loss within 2 ulp - and the source at the first refused stride and beyond 2 and
    4 GiB: GCT2_EINVAL with the full message, nothing launched, dy still the sentinel.  (Before the bound existed the kernel read
    every source pixel past 2^31 bytes as zeros and returned GCT2_OK.)"""
    dt = c.dt
    B, H, W, Cin = c.shape[:4]
    cs = E.make_case("convT_head", (B, H, W, Cin), dt)
    Cout, hCin, hCout = 64, 67, 3
    M = B * 4 * H * W
    rows = B * (H // 16) * (W // 16)
    ctx = make_ctx(gpu, c.mode)
    wsbuf = torch.full((rows * HEAD_ROW + 4096,), NAN, dtype=torch.float32, device=gpu)
    ctx.set_workspace(wsbuf[:rows * HEAD_ROW])
    place = Wide(c)
    f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=gpu)
    xb, xp, ldx = place.inp("x", dev(cs.xc, dt, gpu), c.mode, "in")
    wb, wp = E.guarded(dev(cs.wc, dt, gpu))
    bb, bp = E.guarded(dev(cs.bc, F32, gpu))
    hwb, hwp = E.guarded(dev(cs.w, F32, gpu))
    hbb, hbp = E.guarded(dev(cs.bias, F32, gpu))
    tb, tp = E.guarded(dev(cs.target, F32, gpu))
    sb, sp = E.guarded(f32([cs.loss_scale]))
    x2b, x2p, ldx2 = place.inp("x2", dev(cs.img.reshape(B, 2 * H, 2 * W, 3), dt, gpu), c.mode, "x2")
    pred = Out(nan_like((M, hCout), F32, gpu), 0, 0, guard=True)
    dy, lddy = place.out("dy", nan_like((B, 2 * H, 2 * W, Cout), dt, gpu), c.mode)
    hdw, hdb = Out(nan_like((hCin, hCout), F32, gpu), 0, 0, guard=True), Out(nan_like((hCout,), F32, gpu), 0, 0, guard=True)
    db = Out(nan_like((Cout,), F32, gpu), 0, 0, guard=True)
    loss = Out(nan_like((1,), F32, gpu), 0, 0, guard=True)
    args = (ctx.handle, dt, xp, ldx, wp, bp, hwp, hbp, tp, pred.ptr, dy.ptr, lddy, hdw.ptr, hdb.ptr, loss.ptr, B, H, W, Cin, Cout, hCin, hCout,
            sp, db.ptr, x2p, ldx2, 0, stream())
    if c.family is None:                                        # refused: the code, the full text, nothing written
        rc = lib().load().gct2_convT4s2_fwd_head_train(*args)
        text = lib().load().gct2_last_error().decode()
        torch.cuda.synchronize()
        assert (rc, text) == (EINVAL, L.HEAD_REFUSAL), (rc, text)
        assert ctx.read_launch_log() == []
        for o, name in ((dy, "dy"), (pred, "pred"), (hdw, "head_dw"), (hdb, "head_db"), (db, "db"), (loss, "loss")):
            E.assert_elementwise_equal(o.buf, o.before, ("i",), f"{c.id}: {name} changed")
        assert bool(torch.isnan(wsbuf).all())
        log = []
    else:
        lib().call("gct2_convT4s2_fwd_head_train", *args)
        torch.cuda.synchronize()
        log = check_log(ctx, "halo:convT:head")
        assert log == ["halo:convT:head"]
        assert bool(torch.isnan(wsbuf[rows * HEAD_ROW:]).all()), "the kernel wrote behind the documented workspace"
        pred.check(E.expected(cs.pred_r, F32), c.id + " pred", ("m", "o"))
        dy.check(E.expected(cs.dx.reshape(B, 2 * H, 2 * W, Cout), dt), c.id + " dy")
        db.check(E.expected(cs.db_dx, F32), c.id + " db", ("c",))
        hdw.check(E.expected(cs.dw, F32), c.id + " head_dw", ("c", "o"))
        hdb.check(E.expected(cs.db, F32), c.id + " head_db", ("o",))
        assert_loss(float(loss.got()[0]), cs.loss, c.id)
    del dy, xb, x2b
    view_log(c, log)


def test_engine_takes_the_unfused_pair_when_the_u0_source_exceeds_the_bound(gpu, monkeypatch):
    """UNetEngine.fused_u0_head_ok mirrors the bound: an engine whose UpShuffle_0 source would not fit runs gct2_convT4s2_fwd +
    gct2_dense_head_train instead of surfacing GCT2_EINVAL from a train step.  The bound is lowered to the source's own size (the
    predicate's input) instead of allocating a 2-GiB network; the two paths compute the same head on the same activations."""
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import engine as eng_mod
    size, B = 32, 2
    gen = torch.Generator().manual_seed(4)
    x = (torch.randint(0, 256, (B, size, size, 3), generator=gen).float() / 128 - 1).to(gpu)
    losses, logs = {}, {}
    for name in ("fused", "bound"):
        eng = g.UNetEngine(g.Topology(128, 256, 2), BF16, gpu, seed=3, rng_seed=5)
        b = eng.buffers(B, size, size)
        Hs, Ws = b.hw[1]
        ldx = eng.u0_source(b)[1]
        assert eng.fused_u0_head_ok(b)
        if name == "bound":
            # the bound at which this source is the first one refused (tests/test_large_view_cases_cpu.py ties u0_head_sizes_ok to
            # the restated predicate at the real bound)
            monkeypatch.setattr(eng_mod, "U0_HEAD_MAX_BYTES", B * Hs * Ws * ldx * 2 + 2 * eng.topo.up_in(0) + 128)
            assert not eng.fused_u0_head_ok(b) and eng.fused_head_ok()
        eng.ctx.log_launches(True); eng.ctx_tail.log_launches(True)
        losses[name] = float(eng.train_step(x, apply=False)[0])
        torch.cuda.synchronize()
        logs[name] = eng.read_launch_log()
        eng.ctx.log_launches(False); eng.ctx_tail.log_launches(False)
        monkeypatch.undo()
    assert logs["fused"].count("halo:convT:head") == 1, logs["fused"]
    assert not any(t.startswith("halo:convT:head") for t in logs["bound"]), logs["bound"]
    fwdT = lambda log: [t for t in log if t.startswith(("tap:convT:", "halo:convT:")) and ":bias_act" in t]      # Conv2DTranspose forwards
    assert len(fwdT(logs["bound"])) == len(fwdT(logs["fused"])) + 1, (logs["fused"], logs["bound"])
    print("losses:", losses)
    # the same head on the same rounded activations; only the order of the fp32 sum of 2 * 32 * 32 * 3 squares differs
    assert np.isfinite(losses["bound"]) and abs(losses["bound"] - losses["fused"]) <= 1e-5 * abs(losses["fused"]), losses


def test_dense_head_train_refuses_a_stride_beyond_its_lds_tile(gpu):
    """the size contract of gct2_dense_head_train (tests/large_view_cases.py): ldx = 240 is the last stride it accepts at Cmask = 64;
    the next one is refused with its message before anything is launched"""
    ctx = make_ctx(gpu, "bf16", ws=True)
    M, Cin, Cout, Cmask = 16, 67, 3, 64
    ld = L.DENSE_HEAD_LDX_MAX + 8
    x = torch.zeros(M, ld, dtype=torch.bfloat16, device=gpu)
    dx = torch.full((M, ld), SENTINEL, dtype=torch.bfloat16, device=gpu)
    small = torch.zeros(4096, dtype=torch.float32, device=gpu)
    rc = lib().load().gct2_dense_head_train(ctx.handle, BF16, x.data_ptr(), ld, small.data_ptr(), small.data_ptr(), small.data_ptr(), None,
                                            dx.data_ptr(), ld, small.data_ptr(), small.data_ptr(), small.data_ptr(), small.data_ptr(), M, Cin,
                                            Cout, Cmask, None, None, None, 0, 0, stream())
    text = lib().load().gct2_last_error().decode()
    torch.cuda.synchronize()
    assert (rc, text) == (EINVAL, L.DENSE_HEAD_REFUSAL % ld), (rc, text)
    assert bool((dx == SENTINEL).all()) and ctx.read_launch_log() == []


# ---- pointwise entry points ------------------------------------------------------------------------------------------------------------------

def pw_views(c, tensors, fills, gpu):
    """role -> (buffer, torch view or None, pointer, ld): the case's role wide, the others compact in a poisoned buffer"""
    out = {}
    for role, t in tensors.items():
        if role == c.role:
            buf, view, ptr = E.wide_view(t, c.ld, fills[role])
            out[role] = (buf, view, ptr, c.ld)
        else:
            C = t.shape[-1]
            buf, ptr = E.poisoned_view(t, C + 5, 2, fills[role])
            out[role] = (buf, E.view_of(buf, 2, C), ptr, C + 5)
    return out


def check_pw_output(c, role, v, want, fill, what):
    buf, view, ptr, ld = v
    torch.cuda.synchronize()
    E.assert_elementwise_equal(view.contiguous(), want, what=what)
    if role == c.role:
        E.assert_outside_untouched_device(buf, view, fill, what)
    else:
        C = want.shape[-1]
        before = torch.full_like(buf, fill)
        E.assert_outside_untouched(buf, before, (slice(1, -1), Ellipsis, slice(2, 2 + C)), what)


@pytest.mark.parametrize("c", params([c for c in L.pointwise_cases() if c.entry in ("relu_mask", "add")]))
def test_relu_mask_and_add_with_one_wide_view(gpu, c, view_log):
    """d = act > 0 ? d : 0 and dst += src on [B, 8, 8, 8] views, each operand in turn at T1 .. T3; integers / 4: every sum is exact
    in every dtype"""
    B, h, w, C = c.view
    rng = np.random.default_rng([B, c.dt, 17])
    a = rng.integers(-8, 9, (B, h, w, C)).astype(np.float64) / 4
    d = rng.integers(-8, 9, (B, h, w, C)).astype(np.float64) / 4
    if c.entry == "relu_mask":
        v = pw_views(c, {"act": dev(a, c.dt, gpu), "d": dev(d, c.dt, gpu)}, {"act": NAN, "d": SENTINEL}, gpu)
        lib().call("gct2_relu_mask", c.dt, v["act"][2], v["act"][3], v["d"][2], v["d"][3], B * h * w, C, stream())
        check_pw_output(c, "d", v["d"], E.expected(np.where(a > 0, d, 0.0), c.dt), SENTINEL, c.id)
    else:
        v = pw_views(c, {"dst": dev(d, c.dt, gpu), "src": dev(a, c.dt, gpu)}, {"dst": SENTINEL, "src": NAN}, gpu)
        lib().call("gct2_add", c.dt, v["dst"][2], v["dst"][3], v["src"][2], v["src"][3], B * h * w, C, stream())
        check_pw_output(c, "dst", v["dst"], E.expected(a + d, c.dt), SENTINEL, c.id)
    del v
    view_log(c, [])


@pytest.mark.parametrize("c", params([c for c in L.pointwise_cases() if c.entry == "noise_image"]))
def test_noise_image_with_a_wide_output(gpu, c, view_log):
    """gct2_noise_image into out / out2 at T1 .. T3, one timestep per image (tests/pointwise_cases.py noise_case(6), its first B
    images), against oracle.noise_image_f32 as in tests/test_pointwise_exact_gpu.py"""
    B, HW, _, C = c.view
    steps = 6
    case = P.noise_case(steps)
    x, eps, t = case["x"][:B], case["eps"][:B], case["t"][:B]
    want = torch.tensor(O.noise_image_f32(x, t, eps, steps, E.DTYPE_NAMES[c.dt])).to(E.TDT[c.dt]).reshape(B, HW, 1, C)
    init = torch.full((B, HW, 1, C), NAN, dtype=E.TDT[c.dt], device=gpu)
    v = pw_views(c, {"out": init, "out2": init.clone()}, {"out": SENTINEL, "out2": SENTINEL}, gpu)
    xd, ed, td = (torch.tensor(np.ascontiguousarray(a), device=gpu) for a in (x, eps, t))
    lib().call("gct2_noise_image", c.dt, xd.data_ptr(), td.data_ptr(), ed.data_ptr(), v["out"][2], v["out"][3], v["out2"][2], v["out2"][3],
               B, HW, C, steps, stream())
    for role in ("out", "out2"):
        check_pw_output(c, role, v[role], want, SENTINEL, f"{c.id} {role}")
    del v
    view_log(c, [])


@pytest.mark.parametrize("c", params([c for c in L.pointwise_cases() if c.entry in ("dense_fwd", "dense_bwd")]))
def test_dense_fwd_bwd_with_one_wide_view(gpu, c, view_log):
    """gct2_dense_fwd reads x, gct2_dense_bwd reads x and writes dx at T1 .. T3 (M = B * 250 rows); inputs and references of
    exact_cases.make_case("dense_fwd", (M, 67, 3))"""
    B, h, w, _ = c.view
    M, Cin, Cout, Cmask = B * h * w, 67, 3, 64
    cs = E.make_case("dense_fwd", (M, Cin, Cout), c.dt)
    xs = dev(cs.x, c.dt, gpu).reshape(B, h, w, Cin)
    wb, wp = E.guarded(dev(cs.w, F32, gpu))
    bb, bp = E.guarded(dev(cs.bias, F32, gpu))
    if c.entry == "dense_fwd":
        v = pw_views(c, {"x": xs}, {"x": NAN}, gpu)
        y = Out(nan_like((M, Cout), F32, gpu), 0, 0, guard=True)
        lib().call("gct2_dense_fwd", c.dt, v["x"][2], v["x"][3], wp, bp, y.ptr, M, Cin, Cout, stream())
        y.check(E.expected(cs.pred, F16).float() if c.dt == F16 else E.expected(cs.pred, F32), c.id, ("m", "o"))
    else:
        init = torch.full((B, h, w, Cmask), NAN, dtype=E.TDT[c.dt], device=gpu)
        v = pw_views(c, {"x": xs, "dx": init}, {"x": NAN, "dx": SENTINEL}, gpu)
        dyb, dyp = E.guarded(dev(cs.dy, F32, gpu))
        dw = Out(nan_like((Cin, Cout), F32, gpu), 0, 0, guard=True)
        db = Out(nan_like((Cout,), F32, gpu), 0, 0, guard=True)
        lib().call("gct2_dense_bwd", c.dt, v["x"][2], v["x"][3], wp, dyp, v["dx"][2], v["dx"][3], dw.ptr, db.ptr, M, Cin, Cout, Cmask, 0, stream())
        dw.check(E.expected(cs.dw, F32), c.id + " dw", ("c", "o"))
        db.check(E.expected(cs.db, F32), c.id + " db", ("o",))
        check_pw_output(c, "dx", v["dx"], E.expected(cs.dx[:, :Cmask], c.dt).reshape(B, h, w, Cmask), SENTINEL, c.id + " dx")
    del v
    view_log(c, [])


NOISE_SEED, NOISE_SID, NOISE_OFF = 0x123456789ABCDEF, 2, 7


@pytest.mark.parametrize("c", params([c for c in L.pointwise_cases() if c.entry in ("noise_image_rng", "noise_image_table", "noise_image_rng_table")]))
def test_noise_image_other_forms_with_a_wide_output(gpu, c, view_log):
    """the rng, table and rng + table forms write out / out2 through the same pixel * ld: the table forms against
    noise_schedule_cases.mix_ref, the formula form against oracle.noise_image_f32; the rng forms on their own draws (eps_out, which
    must be gct2_rng_normal's stream at that offset), as in tests/test_noise_schedule_kernels_gpu.py"""
    B, HW, _, C = c.view
    steps = 4 if "table" in c.entry else 6
    x = P.noise_case(6)["x"][:B]
    eps = P.noise_case(6)["eps"][:B]
    t = np.array([4, 1, 3, 2, 4][:B], np.int32)
    n = B * HW * C
    xd, td = (torch.tensor(np.ascontiguousarray(a), device=gpu) for a in (x, t))
    init = torch.full((B, HW, 1, C), NAN, dtype=E.TDT[c.dt], device=gpu)
    v = pw_views(c, {"out": init, "out2": init.clone()}, {"out": SENTINEL, "out2": SENTINEL}, gpu)
    o = (v["out"][2], v["out"][3], v["out2"][2], v["out2"][3])
    tb, coef = E.guarded(torch.tensor(N.TABLE4, device=gpu))
    if "rng" in c.entry:
        draws = torch.full((n,), NAN, device=gpu)
        eps_out = Out(nan_like((n,), F32, gpu), 0, 0, guard=True)
        lib().call("gct2_rng_normal", NOISE_SEED, NOISE_SID, NOISE_OFF, draws.data_ptr(), n, stream())
        if c.entry == "noise_image_rng":
            lib().call("gct2_noise_image_rng", c.dt, xd.data_ptr(), td.data_ptr(), NOISE_SEED, NOISE_SID, NOISE_OFF, eps_out.ptr, *o, B, HW, C, steps, stream())
        else:
            lib().call("gct2_noise_image_rng_table", c.dt, xd.data_ptr(), td.data_ptr(), NOISE_SEED, NOISE_SID, NOISE_OFF, eps_out.ptr, coef, *o,
                       B, HW, C, steps, stream())
        torch.cuda.synchronize()
        eps_out.check(draws.cpu(), c.id + " eps_out against gct2_rng_normal", ("i",))
        eps = draws.cpu().numpy().reshape(B, HW, C)
    else:
        ed = torch.tensor(np.ascontiguousarray(eps), device=gpu)
        lib().call("gct2_noise_image_table", c.dt, xd.data_ptr(), td.data_ptr(), ed.data_ptr(), coef, *o, B, HW, C, steps, stream())
    if "table" in c.entry:
        want = N.mix_ref(c.dt, x, eps, N.TABLE4[t - 1])
    else:
        want = torch.tensor(O.noise_image_f32(x, t, eps, steps, E.DTYPE_NAMES[c.dt])).to(E.TDT[c.dt])
    want = want.reshape(B, HW, 1, C)
    assert not bool(torch.isnan(want.float()).any())
    for role in ("out", "out2"):
        check_pw_output(c, role, v[role], want, SENTINEL, f"{c.id} {role}")
    del v
    view_log(c, [])


STEPS_T = [1, 3, 2, 3, 1]                     # the weight slice of each image (t_int)


def steps_head(cs):
    """three weight slices from one exact Dense case: the kernel, its negative, its columns reversed (the budget counts magnitudes)"""
    return (np.concatenate([cs.w, -cs.w, cs.w[:, ::-1]], 1), np.concatenate([cs.bias, -cs.bias, cs.bias[::-1]]),
            [(cs.w, cs.bias), (-cs.w, -cs.bias), (cs.w[:, ::-1], cs.bias[::-1])])


@pytest.mark.parametrize("c", params([c for c in L.pointwise_cases() if c.entry.startswith("dense_steps")]))
def test_dense_steps_with_one_wide_view(gpu, c, view_log):
    """gct2_dense_steps_fwd / _bwd (a weight slice per image) with x or dx at T1 .. T3, against fp64 on exact-sum inputs: y, dx, and
    dw / db written in full (the slices no image uses hold zeros)"""
    B, h, w, _ = c.view
    HW, Cin, Cout, Cmask, steps = h * w, 67, 3, 64, 3
    M = B * HW
    cs = E.make_case("dense_fwd", (M, Cin, Cout), c.dt)
    W, bias, slices = steps_head(cs)
    tl = STEPS_T[:B]
    img = lambda a, i: a[i * HW:(i + 1) * HW]
    xs = dev(cs.x, c.dt, gpu).reshape(B, h, w, Cin)
    wb, wp = E.guarded(dev(W, F32, gpu))
    bb, bp = E.guarded(dev(bias, F32, gpu))
    td = torch.tensor(tl, dtype=torch.int32, device=gpu)
    ctx = make_ctx(gpu, c.mode)
    if c.entry == "dense_steps_fwd":
        v = pw_views(c, {"x": xs}, {"x": NAN}, gpu)
        y = Out(nan_like((M, Cout), F32, gpu), 0, 0, guard=True)
        lib().call("gct2_dense_steps_fwd", ctx.handle, c.dt, v["x"][2], v["x"][3], wp, bp, td.data_ptr(), y.ptr, B, HW, Cin, Cout, steps, stream())
        pred = np.concatenate([img(cs.x, i) @ slices[s - 1][0] + slices[s - 1][1] for i, s in enumerate(tl)])
        y.check(E.expected(pred, F16).float() if c.dt == F16 else E.expected(pred, F32), c.id, ("m", "o"))
    else:
        init = torch.full((B, h, w, Cmask), NAN, dtype=E.TDT[c.dt], device=gpu)
        v = pw_views(c, {"x": xs, "dx": init}, {"x": NAN, "dx": SENTINEL}, gpu)
        dyb, dyp = E.guarded(dev(cs.dy, F32, gpu))
        dw = Out(nan_like((Cin, steps * Cout), F32, gpu), 0, 0, guard=True)
        db = Out(nan_like((steps * Cout,), F32, gpu), 0, 0, guard=True)
        need = ctypes.c_size_t(0)
        lib().check(lib().load().gct2_dense_steps_scratch(B, HW, Cin, Cout, ctypes.byref(need)), "gct2_dense_steps_scratch")
        sc = torch.full((need.value + 64,), NAN, device=gpu)
        lib().call("gct2_dense_steps_bwd", ctx.handle, c.dt, v["x"][2], v["x"][3], wp, td.data_ptr(), dyp, v["dx"][2], v["dx"][3], dw.ptr, db.ptr,
                   sc.data_ptr(), need.value, B, HW, Cin, Cout, steps, Cmask, 0, stream())
        dx = np.concatenate([np.where(img(cs.x, i) > 0, img(cs.dy, i) @ slices[s - 1][0].T, 0.0) for i, s in enumerate(tl)])[:, :Cmask]
        want_dw, want_db = np.zeros((Cin, steps * Cout)), np.zeros(steps * Cout)
        for i, s in enumerate(tl):
            want_dw[:, (s - 1) * Cout:s * Cout] += img(cs.x, i).T @ img(cs.dy, i)
            want_db[(s - 1) * Cout:s * Cout] += img(cs.dy, i).sum(0)
        dw.check(E.expected(want_dw, F32), c.id + " dw", ("c", "o"))
        db.check(E.expected(want_db, F32), c.id + " db", ("o",))
        check_pw_output(c, "dx", v["dx"], E.expected(dx, c.dt).reshape(B, h, w, Cmask), SENTINEL, c.id + " dx")
        assert bool(torch.isnan(sc[need.value:]).all())
    log = ctx.read_launch_log()
    assert log == ["dense_steps:fwd" if c.entry == "dense_steps_fwd" else "dense_steps:bwd"], log
    del v
    view_log(c, log)


@pytest.mark.parametrize("c", params([c for c in L.pointwise_cases() if c.entry.startswith("dense2")]))
def test_dense2_with_one_wide_view(gpu, c, view_log):
    """gct2_dense2_fwd / _bwd (hidden Dense(128, relu) + Dense(3), the hidden activation never stored) with x or dx at T1 .. T3, on
    the exact-sum inputs and fp64 reference of tests/test_hidden_dense_kernels_gpu.py's Case: equality.  16-bit runs the matrix-core
    kernels, fp32 the plain ones."""
    import test_hidden_dense_kernels_gpu as H
    B, h, w, _ = c.view
    M, Cin, Chid, Cout, Cmask = B * h * w, 67, 128, 3, 64
    k = H.Case(gpu, c.dt, M, Cin, 72, Chid, Cout, seed=500 + M + c.dt, exact=True)
    assert np.abs(k.pre).max() <= 256 and np.abs(k.dh_raw).max() <= 256
    ctx = make_ctx(gpu, c.mode)
    xs = dev(k.x, c.dt, gpu).reshape(B, h, w, Cin)
    path = "plain" if c.dt == F32 else "mfma"
    nsc = k.scratch_floats()
    sc = torch.full((nsc + 64,), NAN, device=gpu)
    xbuf, xview, xp = E.wide_view(xs, c.ld) if c.role == "x" else (None, None, k.d_x.data_ptr())
    ldx = c.ld if c.role == "x" else k.ldx
    if c.entry == "dense2_fwd":
        y = Out(nan_like((M, Cout), F32, gpu), 0, 0, guard=True)
        lib().call("gct2_dense2_fwd", ctx.handle, c.dt, xp, ldx, k.d_w1.data_ptr(), k.d_b1.data_ptr(), k.d_w2.data_ptr(), k.d_b2.data_ptr(), y.ptr,
                   M, Cin, Chid, Cout, stream())
        y.check(E.expected(k.y, F32), c.id + " y", ("m", "o"))
    else:
        init = torch.full((B, h, w, Cmask), NAN, dtype=E.TDT[c.dt], device=gpu)
        if c.role == "dx":
            out, lddx = WideOut(init, c.ld), c.ld
        else:
            out, lddx = Out(init, Cmask + 8, 0), Cmask + 8
        grads = [Out(nan_like(shape, F32, gpu), 0, 0, guard=True) for shape in ((Cin, Chid), (Chid,), (Chid, Cout), (Cout,))]
        lib().call("gct2_dense2_bwd", ctx.handle, c.dt, xp, ldx, k.d_w1.data_ptr(), k.d_b1.data_ptr(), k.d_w2.data_ptr(),
                   k.d_dy.data_ptr(), out.ptr, lddx, *(g.ptr for g in grads), sc.data_ptr(), nsc, M, Cin, Chid, Cout, Cmask, 0, stream())
        for g, want, name in zip(grads, (k.dw1, k.db1, k.dw2, k.db2), ("dw1", "db1", "dw2", "db2")):
            g.check(E.expected(want, F32), f"{c.id} {name}", ("i", "j"))
        out.check(E.expected(k.dx[:, :Cmask], c.dt).reshape(B, h, w, Cmask), c.id + " dx")
        assert bool(torch.isnan(sc[nsc:]).all())
        del out
    if xbuf is not None:                                     # the NaN around the wide input is as it was
        torch.cuda.synchronize()
        E.assert_outside_untouched_device(xbuf, xview, NAN, c.id + " x")
        del xbuf, xview
    log = ctx.read_launch_log()
    assert log == [f"dense2:{'fwd' if c.entry == 'dense2_fwd' else 'bwd'}:{path}"], log
    view_log(c, log)


@pytest.mark.parametrize("c", params(L.dense_head_cases()))
def test_dense_head_train_with_a_wide_dx_or_x2(gpu, c, view_log):
    """gct2_dense_head_train bounds ldx only: dx (through lddx) and the packed image x2 (through ldx2) at T1 .. T3, at the sizes of
    the exact head inputs (M = B * 250), through the LDS-tile kernel (no workspace) and the matrix-core kernel with x2 - pred, dx, dw,
    db, db_dx bit for bit, the loss within 2 ulp, as in tests/test_fused_exact_gpu.py"""
    B, h, w, _ = c.view
    Cin, Cout, ld, Cmask = E.HEAD_SHAPE
    M = B * h * w
    cs = E.make_case("head_train", (M, Cin, Cout), c.dt)
    split = c.variant == "ws_x2"
    ctx = make_ctx(gpu, c.mode, ws=split)
    place = Wide(c)
    f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=gpu)
    xb, xp = E.poisoned_view(dev(cs.x[:, :Cmask if split else Cin], c.dt, gpu), ld, 0)
    if not split:
        xb[1:-1, Cin:] = 5.0                               # the LDS kernel multiplies the pad channels by zero weights: finite there
    x2p, ldx2 = None, 0
    if split:
        x2b, x2p, ldx2 = place.inp("x2", dev(cs.x[:, Cmask:], c.dt, gpu).reshape(B, h, w, Cin - Cmask), c.mode, "x2")
    wb, wp = E.guarded(dev(cs.w, F32, gpu))
    bb, bp = E.guarded(dev(cs.bias, F32, gpu))
    tb, tp = E.guarded(dev(cs.target, F32, gpu))
    sb, sp = E.guarded(f32([cs.loss_scale]))
    pred = Out(nan_like((M, Cout), F32, gpu), 0, 0, guard=True)
    dx, lddx = place.out("dx", nan_like((B, h, w, Cmask), c.dt, gpu), c.mode)
    dw, db = Out(nan_like((Cin, Cout), F32, gpu), 0, 0, guard=True), Out(nan_like((Cout,), F32, gpu), 0, 0, guard=True)
    db_dx = Out(nan_like((Cmask,), F32, gpu), 0, 0, guard=True)
    loss = Out(nan_like((1,), F32, gpu), 0, 0, guard=True)
    partials = torch.full((1024,), NAN, dtype=torch.float32, device=gpu)
    lib().call("gct2_dense_head_train", ctx.handle, c.dt, xp, ld, wp, bp, tp, pred.ptr, dx.ptr, lddx, dw.ptr, db.ptr, loss.ptr, partials.data_ptr(),
               M, Cin, Cout, Cmask, sp, db_dx.ptr, x2p, ldx2, 0, stream())
    torch.cuda.synchronize()
    assert ctx.read_launch_log() == []
    if split:                                                # the matrix-core kernel leaves its partial rows in the workspace
        assert bool(torch.isnan(partials).all()) and bool(torch.isfinite(ctx._ws[:HEAD_ROW]).all())
    else:                                                    # the LDS-tile kernel one float per work-group in `partials`
        tiles = min((M + 255) // 256, 1024)
        assert bool(torch.isfinite(partials[:tiles]).all()) and bool(torch.isnan(partials[tiles:]).all())
    pred.check(E.expected(cs.pred_r, F32), c.id + " pred", ("m", "o"))
    dx.check(E.expected(cs.dx, c.dt).reshape(B, h, w, Cmask), c.id + " dx")
    dw.check(E.expected(cs.dw, F32), c.id + " dw", ("c", "o"))
    db.check(E.expected(cs.db, F32), c.id + " db", ("o",))
    db_dx.check(E.expected(cs.db_dx if split else cs.db_dx_stored, F32), c.id + " db_dx", ("c",))
    assert_loss(float(loss.got()[0]), cs.loss, c.id)
    del dx
    view_log(c, [])
