"""Every convolution / head kernel against the fp64 oracle ELEMENT BY ELEMENT, on exact-sum inputs (tests/exact_cases.py).

On those inputs an fp32 accumulator holds the exact sum whatever the order, tile, split-K slabs or atomics, so the only rounding
left is the documented one at the store and the output must EQUAL the oracle rounded once (round to nearest even): no tolerance.
Every input and output is a view inside a poisoned buffer - neighbour channels, two guard images, 64 guard elements around weights
and biases hold NaN (inputs) or a sentinel (outputs): an over-read shows up as NaN in the output, an over-write as a changed
sentinel.  Every case asserts through the launch log that the kernel family it is meant to reach is the one that ran.

Rejected by contract, hence not run: nothing in the lists below (the direct kernels take every shape the matrix-core paths refuse).
"""
import numpy as np
import pytest
import torch

import exact_cases as E
from exact_cases import BF16, F16, F32, SENTINEL
from oracle import denoiser_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
MODES = ["bf16", "f16", "f32", "f32m_ws", "f32m"]          # f32m: fp32 on the matrix cores (gct2_ctx_set_f32_math), with / without workspace
MODE_DT = {"bf16": BF16, "f16": F16, "f32": F32, "f32m_ws": F32, "f32m": F32}
FORM = {"conv_fwd": "conv", "convT_fwd": "convT", "conv_dgrad": "convT", "convT_dgrad": "conv"}      # tap-GEMM form of each entry
FN = {"conv_fwd": "gct2_conv4s2_fwd", "convT_fwd": "gct2_convT4s2_fwd", "conv_dgrad": "gct2_conv4s2_dgrad",
      "convT_dgrad": "gct2_convT4s2_dgrad", "conv_wgrad": "gct2_conv4s2_wgrad", "convT_wgrad": "gct2_convT4s2_wgrad",
      "s1_fwd": "gct2_conv2d_s1_fwd", "s1_dgrad": "gct2_conv2d_s1_dgrad", "s1_wgrad": "gct2_conv2d_s1_wgrad"}


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_ctx(gpu, mode, ws=False, tuning=0):
    """a call context of its own per test: fp32 math mode, a NaN-filled 64 MiB scratch for both workspaces or none, tuning, log on"""
    c = lib().Context()
    if mode.startswith("f32m"):
        c.set_f32_math(lib().F32_MATH_MFMA)
    if ws:
        c._ws = torch.full((16 << 20,), NAN, dtype=torch.float32, device=gpu)
        c.set_workspace(c._ws)
        c.set_wgrad_workspace(c._ws)
    if tuning:
        c.set_tuning(tuning)
    c.log_launches(True)
    return c


def dev(a, dt, gpu):
    return torch.tensor(np.asarray(a), dtype=torch.float64).to(E.TDT[dt]).to(gpu).contiguous()


def lay(mode, C, role):
    """(ld, channel offset) of a view: 16-bit views keep the 16 bytes the matrix-core paths need (8 channels); fp32 views use the
    unaligned offsets of tests/test_f32_matrix_gpu.py, and whole 16-byte steps in the f32m_ws mode (its vector loads)"""
    if mode in ("bf16", "f16"):
        return (C + 19) // 4 * 4, 8        # (a multiple of 4: the image layer's 8-byte pixel loads, with a poisoned 4th slot at Cin = 3)
    if mode == "f32m_ws":
        return C + 8, 4
    return {"in": (C + 5, 3), "out": (C + 3, 2), "act": (C + 1, 0)}[role]


class Out:
    """an output view inside a sentinel-filled buffer; check() compares it bit by bit and proves that nothing around it changed"""

    def __init__(self, init, ld, off, guard=False, goff=0):
        self.shape = tuple(init.shape)
        if guard:                                           # goff: E.guarded's element offset (a misaligned fp32 array)
            self.buf, self.ptr = E.guarded(init, SENTINEL, goff)
            self.inside = (slice(E.GUARD + goff, E.GUARD + goff + init.numel()),)
        else:
            self.buf, self.ptr = E.poisoned_view(init, ld, off, SENTINEL)
            self.inside = (slice(1, -1), Ellipsis, slice(off, off + init.shape[-1]))
        self.before = self.buf.clone()

    def got(self):
        return self.buf[self.inside].reshape(self.shape)

    def check(self, want, what, names=("b", "h", "w", "c")):
        torch.cuda.synchronize()
        E.assert_elementwise_equal(self.got(), want, names, what)
        E.assert_outside_untouched(self.buf, self.before, self.inside, what)
        self.before = self.buf.clone()


def nan_like(shape, dt, gpu):
    return torch.full(shape, NAN, dtype=E.TDT[dt], device=gpu)


class Place:
    """where the runners below put the views of a case.  This one: every view in a poisoned buffer of its own at lay()'s stride and
    channel offset, every weight, bias and fp32 gradient array between guards.  tests/test_large_views_gpu.py overrides it per role
    ("x", "dz", "act", "y", "dx") to give one view a stride of millions of elements, tests/alignment_cases.py to choose the alignment
    of every role ("w", "bias", "dw", "db" included)."""

    def inp(self, role, t, mode, kind):
        """an input view (kind: "in" or "act", lay()'s roles) -> (buffer, device pointer, ld)"""
        buf, ptr = E.poisoned_view(t, *lay(mode, t.shape[-1], kind))
        return buf, ptr, buf.shape[-1]

    def out(self, role, init, mode):
        """an output view holding `init` -> (an object with .ptr and .check(want, what, names), ld)"""
        ld, off = lay(mode, init.shape[-1], "out")
        return Out(init, ld, off), ld

    def param(self, role, t):
        """a weight or bias array ("w", "bias") -> (buffer, device pointer)"""
        return E.guarded(t)

    def grad(self, role, init):
        """an fp32 gradient array ("dw", "db", "db2") holding `init` -> an object with .ptr and .check(want, what, names)"""
        return Out(init, 0, 0, guard=True)


PLACE = Place()


def tap_family(entry, shape, mode, halo=False):
    """the launch-log prefix the case must show"""
    Cin, Cout = shape[3], shape[4]
    if mode == "f32":
        return "direct:tap"
    if mode.startswith("f32m"):
        return f"f32mfma:{FORM[entry]}:"
    if entry == "conv_fwd" and Cin <= 4 and Cout % 8 == 0:
        return "rgb:fwd"
    if Cin % 8 or Cout % 8:
        return "direct:tap"
    return "halo:convT:" if halo else f"tap:{FORM[entry]}:"


def check_log(c, prefix, contains=(), split=None):
    """every layer call since the last read logged the expected family (and nothing of another one)"""
    log = [t for t in c.read_launch_log() if not t.startswith(("relu_bits:", "bias_queue:"))]
    assert log and all(t.startswith(prefix) for t in log), (prefix, log)
    for part in contains:
        assert all(part in t for t in log), (part, log)
    if split is not None:
        ks = [int(t.split("ksplit=")[1].split(":")[0]) for t in log if "ksplit=" in t]
        assert ks and all((k > 1) == split for k in ks), (split, log)
    return log


# ---- a. forward and input-gradient calls of the 4x4 / stride-2 layers --------------------------------------------------------------------

def run_fwd(gpu, entry, shape, mode, ws=False, tuning=0, halo=False, contains=(), split=None, place=PLACE, variants=(0, 1), family=None):
    """bias, relu 0 and 1 (variants); family: the launch-log prefix when it is not tap_family()'s"""
    dt = MODE_DT[mode]
    cs = E.make_case(entry, shape, dt)
    B, H, W, Cin, Cout = shape
    c = make_ctx(gpu, mode, ws, tuning)
    xb, xp, ldx = place.inp("x", dev(cs.x, dt, gpu), mode, "in")
    wb, wp = place.param("w", dev(cs.w, dt, gpu))
    bb, bp = place.param("bias", dev(cs.bias, F32, gpu))
    for relu in variants:
        y, ldy = place.out("y", nan_like(cs.ref.shape, dt, gpu), mode)
        lib().call(FN[entry], c.handle, dt, xp, ldx, wp, bp, y.ptr, ldy, B, H, W, Cin, Cout, relu, stream())
        y.check(E.expected(np.maximum(cs.ref, 0) if relu else cs.ref, dt), f"{entry} {shape} {mode} relu={relu}")
        del y                                               # (a view of several GiB leaves before the next one is made)
    return check_log(c, family or tap_family(entry, shape, mode, halo), contains, split)


def run_dgrad(gpu, entry, shape, mode, ws=False, tuning=0, halo=False, contains=(), split=None, place=PLACE,
              variants=((1, 0), (1, 1), (0, 0), (0, 1)), family=None):
    """mask on and off, accumulate 0 and 1 (variants: (masked, accumulate) pairs)"""
    dt = MODE_DT[mode]
    cs = E.make_case(entry, shape, dt)
    B, H, W, Cin, Cout = shape
    c = make_ctx(gpu, mode, ws, tuning)
    dzb, dzp, lddz = place.inp("dz", dev(cs.dz, dt, gpu), mode, "in")
    wb, wp = place.param("w", dev(cs.w, dt, gpu))
    ab, ap, ldact = place.inp("act", dev(cs.act, dt, gpu), mode, "act")
    for masked, accumulate in variants:
        dx, lddx = place.out("dx", dev(cs.prev, dt, gpu) if accumulate else nan_like(cs.prev.shape, dt, gpu), mode)
        lib().call(FN[entry], c.handle, dt, dzp, lddz, wp, ap if masked else None, ldact, dx.ptr, lddx,
                   B, H, W, Cin, Cout, accumulate, None, 0, None, 0, stream())
        dx.check(E.expected(E.dgrad_ref(cs, masked, accumulate), dt), f"{entry} {shape} {mode} mask={masked} accumulate={accumulate}")
        del dx
    return check_log(c, family or tap_family(entry, shape, mode, halo), contains, split)


def run_tap(gpu, entry, *a, **kw):
    (run_fwd if entry.endswith("_fwd") else run_dgrad)(gpu, entry, *a, **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", E.TAP_SHAPES)
@pytest.mark.parametrize("entry", E.TAP_ENTRIES)
def test_tap_entries_exact(gpu, entry, shape, mode):
    """ragged M / K / N, the tiny grid (the fp32 matrix path splits K there when it has a workspace), 16-bit split-K plus finalize at
    K = 8192 (with a workspace), the image-layer kernels, Cin = 4, and a shape only the direct kernels take"""
    sixteen = mode in ("bf16", "f16")
    ws = mode == "f32m_ws" or (sixteen and shape == E.SPLITK_SHAPE)
    split = None
    if sixteen and shape == E.SPLITK_SHAPE:
        split = True
    elif mode.startswith("f32m") and shape == (3, 2, 2, 256, 64):
        split = ws
    run_tap(gpu, entry, shape, mode, ws=ws, split=split)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("tile", [2, 5])
@pytest.mark.parametrize("shape", E.TILE_SHAPES)
@pytest.mark.parametrize("entry", E.TAP_ENTRIES)
def test_tap_tile_variants_exact(gpu, entry, shape, tile, mode):
    run_tap(gpu, entry, shape, mode, tuning=tile, contains=("128x128:" if tile == 2 else "256x128:",))


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("entry,shape", E.HALO_CASES)
def test_halo_kernel_exact(gpu, entry, shape, mode):
    run_tap(gpu, entry, shape, mode, tuning=2 << 24, halo=True)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("entry", E.TAP_ENTRIES)
def test_splitk_xcd_orders_exact(gpu, entry, order, mode):
    run_tap(gpu, entry, E.SPLITK_SHAPE, mode, ws=True, tuning=order << 26, split=True)


# ---- weight gradients ---------------------------------------------------------------------------------------------------------------

def wgrad_family(entry, shape, mode):
    Cin, Cout = shape[3], shape[4]
    if mode == "f32":
        return "direct:wgrad"
    if mode.startswith("f32m"):
        return "f32mfma:wgrad:"
    if entry == "conv_wgrad" and Cin <= 4 and Cout % 8 == 0:
        return "rgb:wgrad"
    return "direct:wgrad" if Cin % 8 or Cout % 8 else "wgrad:"


def wgrad_views(gpu, cs, mode, x=None, dz=None):
    dt = MODE_DT[mode]
    x, dz = cs.x if x is None else x, cs.dz if dz is None else dz
    xb, xp = E.poisoned_view(dev(x, dt, gpu), *lay(mode, x.shape[-1], "in"))
    dzb, dzp = E.poisoned_view(dev(dz, dt, gpu), *lay(mode, dz.shape[-1], "in"))
    return xb, xp, dzb, dzp


def run_wgrad(gpu, entry, shape, mode, ws, tuning=0, contains=(), place=PLACE):
    """dw and db, overwrite (over NaN), then accumulate (twice the gradient: still inside the budget)"""
    dt = MODE_DT[mode]
    cs = E.make_case(entry, shape, dt)
    B, Cin, Cout = shape[0], shape[3], shape[4]
    h, w_ = E.wgrad_hw(entry, shape)
    c = make_ctx(gpu, mode, ws, tuning)
    xb, xp, ldx = place.inp("x", dev(cs.x, dt, gpu), mode, "in")
    dzb, dzp, lddz = place.inp("dz", dev(cs.dz, dt, gpu), mode, "in")
    dw = place.grad("dw", nan_like(cs.dw.shape, F32, gpu))
    db = place.grad("db", nan_like(cs.db.shape, F32, gpu))
    tail = (shape[5],) if entry == "s1_wgrad" else ()
    extra = () if entry == "s1_wgrad" else (None,)          # gct2_adam_args of the 4x4 entries
    for accumulate in (0, 1):
        lib().call(FN[entry], c.handle, dt, xp, ldx, dzp, lddz, dw.ptr, db.ptr, B, h, w_, Cin, Cout, *tail, accumulate,
                   *extra, stream())
        k = 1 + accumulate
        what = f"{entry} {shape} {mode} ws={ws} accumulate={accumulate}"
        dw.check(E.expected(k * cs.dw, F32), what + " dw", ("kh", "kw", "ci", "co") if entry != "convT_wgrad" else ("kh", "kw", "co", "ci"))
        db.check(E.expected(k * cs.db, F32), what + " db", ("c",))
    return c


# (the direct fp32 kernels take no workspace: with one they would be the same launch again)
@pytest.mark.parametrize("mode,ws", [(m, w) for m in ("bf16", "f16", "f32", "f32m") for w in (False, True) if not (m == "f32" and w)])
@pytest.mark.parametrize("shape", E.WGRAD_SHAPES)
@pytest.mark.parametrize("entry", E.WGRAD_ENTRIES)
def test_wgrad_exact(gpu, entry, shape, mode, ws):
    """exact sums make the atomics path (no workspace) bit-comparable with the oracle too"""
    c = run_wgrad(gpu, entry, shape, mode, ws)
    log = check_log(c, wgrad_family(entry, shape, mode))
    if not ws:
        assert not any(t.endswith(":slabs") for t in log), log
    elif shape == (4, 32, 32, 64, 128) and log[0].startswith(("wgrad:", "f32mfma:")):
        assert all(t.endswith(":slabs") for t in log), log


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("tuning,token", [(2 << 16, "wgrad:256q:"), (3 << 16, "wgrad:128:"), (7 << 16, ":atomics"), (1 << 28, "rsplit=1:owner"),
                                          (3 << 28, "rsplit=4:slabs")])
@pytest.mark.parametrize("entry", E.WGRAD_ENTRIES)
def test_wgrad_tunings_exact(gpu, entry, tuning, token, mode):
    """both tiles, atomics kept although a workspace is there, and the forced pixel splits, at the shape whose 16 steps of 64 rows
    allow four splits"""
    c = run_wgrad(gpu, entry, E.WGRAD_TUNING_SHAPE, mode, True, tuning)
    check_log(c, "wgrad:", contains=(token,))


@pytest.mark.parametrize("tuning,token", [(1 << 28, "rsplit=1:owner"), (3 << 28, "rsplit=4:slabs")])
@pytest.mark.parametrize("entry", E.WGRAD_ENTRIES)
def test_wgrad_forced_splits_f32_matrix_exact(gpu, entry, tuning, token):
    c = run_wgrad(gpu, entry, E.WGRAD_TUNING_SHAPE, "f32m", True, tuning)
    check_log(c, "f32mfma:wgrad:", contains=(token,))


# ---- stride-1 convolutions ------------------------------------------------------------------------------------------------------------

def s1_prefix(entry, shape, mode):
    """the direct stride-1 fall-back logs nothing (include/gct2.h): None"""
    Cin, Cout = shape[3], shape[4]
    if mode.startswith("f32m"):
        return {"s1_fwd": "f32mfma:s1:", "s1_dgrad": "f32mfma:s1t:", "s1_wgrad": "f32mfma:wgrad_s1:"}[entry]
    if mode == "f32" or Cin % 8 or Cout % 8:
        return None
    return "wgrad:s1:" if entry == "s1_wgrad" else "tap:s1:"


# with and without scratch where the path takes it (the direct kernels take none)
S1_CASES = [pytest.param(e, s, m, w, id=f"{e}-{'x'.join(map(str, s))}-{m}-{'ws' if w else 'nows'}") for e in E.S1_ENTRIES for s in E.S1_SHAPES
            for m in ("bf16", "f16", "f32", "f32m") for w in (False, True) if not (w and s1_prefix(e, s, m) is None)]


def run_s1(gpu, entry, shape, mode, ws, place=PLACE, variants=None, prefix="default"):
    """the three stride-1 entries; variants as in run_fwd / run_dgrad; prefix: the launch-log family (None: nothing is logged) when it
    is not s1_prefix()'s.  Returns the log."""
    prefix = s1_prefix(entry, shape, mode) if prefix == "default" else prefix
    dt = MODE_DT[mode]
    B, H, W, Cin, Cout, KS = shape
    if entry == "s1_wgrad":
        c = run_wgrad(gpu, entry, shape, mode, ws, place=place)
    else:
        cs = E.make_case(entry, shape, dt)
        c = make_ctx(gpu, mode, ws)
        wb, wp = place.param("w", dev(cs.w, dt, gpu))
        if entry == "s1_fwd":
            xb, xp, ldx = place.inp("x", dev(cs.x, dt, gpu), mode, "in")
            bb, bp = place.param("bias", dev(cs.bias, F32, gpu))
            for relu in variants or (0, 1):
                y, ldy = place.out("y", nan_like(cs.ref.shape, dt, gpu), mode)
                lib().call(FN[entry], c.handle, dt, xp, ldx, wp, bp, y.ptr, ldy, B, H, W, Cin, Cout, KS, relu, stream())
                y.check(E.expected(np.maximum(cs.ref, 0) if relu else cs.ref, dt), f"{entry} {shape} {mode} relu={relu}")
                del y
        else:
            dzb, dzp, lddz = place.inp("dz", dev(cs.dz, dt, gpu), mode, "in")
            ab, ap, ldact = place.inp("act", dev(cs.act, dt, gpu), mode, "act")
            for masked, accumulate in variants or ((1, 0), (1, 1), (0, 0), (0, 1)):
                dx, lddx = place.out("dx", dev(cs.prev, dt, gpu) if accumulate else nan_like(cs.prev.shape, dt, gpu), mode)
                lib().call(FN[entry], c.handle, dt, dzp, lddz, wp, ap if masked else None, ldact, dx.ptr, lddx,
                           B, H, W, Cin, Cout, KS, accumulate, stream())
                dx.check(E.expected(E.dgrad_ref(cs, masked, accumulate), dt), f"{entry} {shape} {mode} mask={masked} accumulate={accumulate}")
                del dx
    if prefix is None:
        log = c.read_launch_log()
        assert log == []
        return log
    return check_log(c, prefix)


@pytest.mark.parametrize("entry,shape,mode,ws", S1_CASES)
def test_conv2d_s1_exact(gpu, entry, shape, mode, ws):
    run_s1(gpu, entry, shape, mode, ws)


# ---- Dense(3) head ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
def test_dense_fwd_bwd_exact(gpu, mode):
    """M = 1000 (a ragged last tile).  GCT2_F16: the prediction is the fp16-rounded value held in fp32 (include/gct2.h).  The entry
    points take no call context, so there is no launch log to read."""
    dt = MODE_DT[mode]
    cs = E.make_case("dense_fwd", E.DENSE_SHAPE, dt)          # (the "dense_bwd" case has the same inputs)
    M, Cin, Cout = E.DENSE_SHAPE
    Cmask = 64
    ld, off = (Cin + 13, 8) if dt != F32 else (Cin + 5, 3)
    xb, xp = E.poisoned_view(dev(cs.x, dt, gpu), ld, off)
    wb, wp = E.guarded(dev(cs.w, F32, gpu))
    bb, bp = E.guarded(dev(cs.bias, F32, gpu))
    y = Out(nan_like((M, Cout), F32, gpu), 0, 0, guard=True)
    lib().call("gct2_dense_fwd", dt, xp, ld, wp, bp, y.ptr, M, Cin, Cout, stream())
    want = E.expected(cs.pred, F16).float() if dt == F16 else E.expected(cs.pred, F32)
    y.check(want, f"dense_fwd {mode}", ("m", "o"))
    dyb, dyp = E.guarded(dev(cs.dy, F32, gpu))
    dx = Out(nan_like((M, Cmask), dt, gpu), ld, off)          # channels >= Cmask get no gradient: they stay sentinels
    dw = Out(nan_like((Cin, Cout), F32, gpu), 0, 0, guard=True)
    db = Out(nan_like((Cout,), F32, gpu), 0, 0, guard=True)
    for accumulate in (0, 1):
        lib().call("gct2_dense_bwd", dt, xp, ld, wp, dyp, dx.ptr, ld, dw.ptr, db.ptr, M, Cin, Cout, Cmask, accumulate, stream())
        k = 1 + accumulate
        dx.check(E.expected(cs.dx[:, :Cmask], dt), f"dense_bwd {mode} dx", ("m", "c"))
        dw.check(E.expected(k * cs.dw, F32), f"dense_bwd {mode} dw accumulate={accumulate}", ("c", "o"))
        db.check(E.expected(k * cs.db, F32), f"dense_bwd {mode} db accumulate={accumulate}", ("o",))


# ---- fused bias gradients of the input-gradient calls -----------------------------------------------------------------------------------

def run_bias_grads(gpu, entry, shape, mode, scratch, place=PLACE, contains=(), tuning=0):
    """db / db2 = column sums of the masked gradient of THIS call, split at a multiple of 8 inside a ragged Cin = 72; first call
    overwrites (over NaN), second adds.  include/gct2.h does not say whether the fp32 rows or the stored rows are summed, so the
    operands come from {-1, 0, 1}: |dx| <= 256 is exact in bf16 and both definitions are the same number.  Equality in every
    reduction mode: atomics (no workspace), partial rows in the workspace, and a bias queue with one flush."""
    dt = MODE_DT[mode]
    cs = E.make_case(entry, shape, dt, "pm1")
    B, H, W, Cin, Cout = shape
    split = 40
    g = E.dgrad_ref(cs, 1, 0)
    assert np.abs(g).max() <= 256 and np.abs(2 * g).max() <= 512          # the precondition: every stored value is exact in bf16
    cs_sum = g.reshape(-1, Cin).sum(0)
    c = make_ctx(gpu, mode, ws=scratch != "none", tuning=tuning)
    if scratch == "ws+queue":
        c.set_bias_queue(torch.full((1 << 20,), NAN, dtype=torch.float32, device=gpu))
    dzb, dzp, lddz = place.inp("dz", dev(cs.dz, dt, gpu), mode, "in")
    wb, wp = place.param("w", dev(cs.w, dt, gpu))
    ab, ap, ldact = place.inp("act", dev(cs.act, dt, gpu), mode, "act")
    dx, lddx = place.out("dx", nan_like(g.shape, dt, gpu), mode)
    db = place.grad("db", nan_like((split,), F32, gpu))
    db2 = place.grad("db2", nan_like((Cin - split,), F32, gpu))
    for k, (accumulate, db_acc) in enumerate([(0, 0), (1, 3)], 1):
        lib().call(FN[entry], c.handle, dt, dzp, lddz, wp, ap, ldact, dx.ptr, lddx, B, H, W, Cin, Cout, accumulate,
                   db.ptr, split, db2.ptr, db_acc, stream())
        if scratch != "ws+queue":
            what = f"{entry} {shape} {mode} {scratch} call {k}"
            dx.check(E.expected(k * g, dt), what + " dx")
            db.check(E.expected(k * cs_sum[:split], F32), what + " db", ("c",))
            db2.check(E.expected(k * cs_sum[split:], F32), what + " db2", ("c",))
    if scratch == "ws+queue":
        lib().call("gct2_bias_queue_flush", c.handle, stream())
        what = f"{entry} {shape} {mode} {scratch}"
        dx.check(E.expected(2 * g, dt), what + " dx")
        db.check(E.expected(2 * cs_sum[:split], F32), what + " db", ("c",))
        db2.check(E.expected(2 * cs_sum[split:], F32), what + " db2", ("c",))
        c.set_bias_queue(None)
    return check_log(c, tap_family(entry, shape, mode), contains)


@pytest.mark.parametrize("scratch", ["none", "ws", "ws+queue"])
@pytest.mark.parametrize("mode", ["bf16", "f16", "f32", "f32m"])
@pytest.mark.parametrize("entry,shape", E.BIAS_GRAD_CASES)
def test_fused_bias_gradients_exact(gpu, entry, shape, mode, scratch):
    """every reduction mode of the fused bias gradients on 16-byte views (run_bias_grads)"""
    run_bias_grads(gpu, entry, shape, mode, scratch)


# ---- c. overflow and non-finite gradients -----------------------------------------------------------------------------------------------

# (entry, shape, mode, workspace, tuning, log prefix): one case per form of the input-gradient kernels
DGRAD_FORMS = [
    ("conv_dgrad", (1, 4, 12, 72, 136), "{}", False, 0, "tap:convT:"),
    ("convT_dgrad", (1, 4, 12, 72, 136), "{}", False, 0, "tap:conv:"),
    ("conv_dgrad", (2, 32, 32, 64, 24), "{}", False, 2 << 24, "halo:convT:"),
    ("conv_dgrad", E.SPLITK_SHAPE, "{}", True, 0, "tap:convT:"),
    ("convT_dgrad", E.SPLITK_SHAPE, "{}", True, 0, "tap:conv:"),
    ("conv_dgrad", (1, 6, 10, 5, 7), "{}", False, 0, "direct:tap"),
    ("convT_dgrad", (1, 6, 10, 5, 7), "{}", False, 0, "direct:tap"),
    ("conv_dgrad", (1, 4, 12, 72, 136), "f32m_ws", True, 0, "f32mfma:convT:"),
    ("convT_dgrad", (1, 4, 12, 72, 136), "f32m_ws", True, 0, "f32mfma:conv:"),
]


def _forms(sixteen):
    out = []
    for entry, shape, mode, ws, tuning, prefix in DGRAD_FORMS:
        for m in (sixteen if mode == "{}" else [mode]):
            out.append(pytest.param(entry, shape, m, ws, tuning, prefix, id=f"{entry}-{'x'.join(map(str, shape))}-{m}-{prefix.strip(':')}"))
    return out


def masked_dgrad_call(gpu, cs, mode, ws, tuning, dz):
    dt = MODE_DT[mode]
    B, H, W, Cin, Cout = cs.shape
    c = make_ctx(gpu, mode, ws, tuning)
    dzb, dzp = E.poisoned_view(dev(dz, dt, gpu), *lay(mode, Cout, "in"))
    wb, wp = E.guarded(dev(cs.w, dt, gpu))
    ab, ap = E.poisoned_view(dev(cs.act, dt, gpu), *lay(mode, Cin, "act"))
    lddx, offdx = lay(mode, Cin, "out")
    dx = Out(nan_like(cs.act.shape, dt, gpu), lddx, offdx)
    lib().call(FN[cs.entry], c.handle, dt, dzp, dzb.shape[-1], wp, ap, ab.shape[-1], dx.ptr, lddx, B, H, W, Cin, Cout, 0, None, 0, None, 0, stream())
    return c, dx


@pytest.mark.parametrize("entry,shape,mode,ws,tuning,prefix", [p for p in _forms(["f16"]) if not p.values[2].startswith("f32m")])
def test_fp16_store_overflows_to_inf(gpu, entry, shape, mode, ws, tuning, prefix):
    """operands scaled by a power of two (the budget counts grid steps, so it still holds) until 1 % .. 50 % of the masked
    |gradient| reach 65520: the store must give +-inf exactly there and 65504 just below - a saturating or wrapping conversion fails"""
    cs = E.make_case(entry, shape, F16, "overflow")
    ref = E.dgrad_ref(cs, 1, 0)
    share = float(np.mean(np.abs(ref) >= 65520))
    assert 0.01 <= share <= 0.5, share
    want = E.expected(ref, F16)
    assert int(torch.isinf(want).sum()) == int((np.abs(ref) >= 65520).sum())
    c, dx = masked_dgrad_call(gpu, cs, mode, ws, tuning, cs.dz)
    dx.check(want, f"overflow {entry} {shape}")
    check_log(c, prefix)


@pytest.mark.parametrize("entry,shape,mode,ws,tuning,prefix", _forms(["f16", "bf16"]))
def test_inf_in_dz_reaches_exactly_its_input_gradients(gpu, entry, shape, mode, ws, tuning, prefix):
    """one +inf in dz; weights from a grid without zero, act with both signs.  Expectation without feeding inf to the oracle: the
    gradient of dz with that element zeroed, +-inf wherever the scatter pattern of a one-hot dz is non-zero (sign of the weight),
    and then 0 wherever act <= 0 - the mask is a SELECT (act > 0 ? g : 0, include/gct2.h): a multiplication would give NaN there.
    Equality also proves that no other element is touched."""
    dt = MODE_DT[mode]
    cs = E.make_case(entry, shape, dt, "nozero")
    hit = (cs.dz.shape[0] - 1, cs.dz.shape[1] // 2, cs.dz.shape[2] // 2, 5)
    dz0 = cs.dz.copy(); dz0[hit] = 0
    one = np.zeros_like(cs.dz); one[hit] = 1
    ref0 = E.dgrad_of(entry, dz0, cs.w, cs.act.shape)
    pat = E.dgrad_of(entry, one, cs.w, cs.act.shape)
    want = np.where(pat > 0, np.inf, np.where(pat < 0, -np.inf, ref0))
    want = np.where(cs.act > 0, want, 0.0)
    assert np.isinf(want).any() and ((pat != 0) & (cs.act <= 0)).any()          # the inf meets the mask somewhere
    dz = cs.dz.copy(); dz[hit] = np.inf
    c, dx = masked_dgrad_call(gpu, cs, mode, ws, tuning, dz)
    dx.check(E.expected(want, dt), f"inf in dz {entry} {shape} {mode}")
    check_log(c, prefix)


@pytest.mark.parametrize("mode,ws,token", [("bf16", True, ":slabs"), ("f16", True, ":slabs"), ("bf16", False, ":atomics"), ("f32m", True, ":slabs")])
@pytest.mark.parametrize("entry", E.WGRAD_ENTRIES)
def test_inf_in_dz_reaches_exactly_its_weight_gradients(gpu, entry, mode, ws, token):
    """one +inf in dz at an interior pixel, x from a grid without zero: every dw element that pixel feeds is sign(x) * inf, db of
    its channel +inf, every other element bit-equal to the reference - with ordered slabs, with atomics, on the fp32 matrix cores"""
    dt = MODE_DT[mode]
    shape = (4, 32, 32, 64, 128)
    cs = E.make_case(entry, shape, dt, "nozero")
    B, Cin, Cout = shape[0], shape[3], shape[4]
    h, w_ = E.wgrad_hw(entry, shape)
    hit = (1, cs.dz.shape[1] // 2 - 1, cs.dz.shape[2] // 2 + 1, 9)
    dz0 = cs.dz.copy(); dz0[hit] = 0
    one = np.zeros_like(cs.dz); one[hit] = 1
    dw0, db0 = E.wgrad_of(entry, cs.x, dz0)
    pat, _ = E.wgrad_of(entry, cs.x, one)
    want_dw = np.where(pat > 0, np.inf, np.where(pat < 0, -np.inf, dw0))
    want_db = db0.copy(); want_db[hit[3]] = np.inf
    assert int((pat != 0).sum()) == (16 if entry == "conv_wgrad" else 4) * Cin
    dz = cs.dz.copy(); dz[hit] = np.inf
    c = make_ctx(gpu, mode, ws)
    xb, xp, dzb, dzp = wgrad_views(gpu, cs, mode, dz=dz)
    dw = Out(nan_like(cs.dw.shape, F32, gpu), 0, 0, guard=True)
    db = Out(nan_like(cs.db.shape, F32, gpu), 0, 0, guard=True)
    lib().call(FN[entry], c.handle, dt, xp, xb.shape[-1], dzp, dzb.shape[-1], dw.ptr, db.ptr, B, h, w_, Cin, Cout, 0, None, stream())
    dw.check(E.expected(want_dw, F32), f"inf in dz {entry} {mode} dw", ("kh", "kw", "ci", "co") if entry == "conv_wgrad" else ("kh", "kw", "co", "ci"))
    db.check(E.expected(want_db, F32), f"inf in dz {entry} {mode} db", ("c",))
    check_log(c, "f32mfma:wgrad:" if mode == "f32m" else "wgrad:", contains=(token,))
