"""The rejection contract of the C entry points whose bodies share helpers in csrc/capi.hip: the 4x4 / stride-2 layer calls, the stride-1
ones, the scratch setters and gct2_adam_apply.  Every row of CASES is a call that its argument checks reject BEFORE anything is
launched; the row fixes the return code and the full error text, and rows with two mistakes fix the order of the checks.

The table runs in a fresh child process (this file as a script) whose environment hides the GPUs: the pointers are fake addresses,
and a row that slipped through its checks must find no device to launch on.  The child first asks gct2_device_check(); it runs the
table only when that says GCT2_ENODEV, otherwise it reports the visible device and the test skips.  Without a GPU nothing skips."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = 0, 1, 2
EINVAL, ENODEV = 1, 3
P = 4096                    # a fake, 16-byte aligned device address; no row lets a call get as far as reading it
CTX, ADAM = "<ctx>", "<adam>"   # replaced in the child by a live gct2_ctx handle / by a pointer to the row's gct2_adam_args


def _args(defaults, over):
    unknown = set(over) - set(defaults)
    assert not unknown, unknown
    return list({**defaults, **over}.values())


# one builder per signature of include/gct2.h: valid arguments (a call with no override would pass every check) in prototype order
def fwd(**o):           # gct2_conv4s2_fwd / gct2_convT4s2_fwd
    return _args(dict(ctx=CTX, dtype=BF16, x=P, ldx=8, w=P, bias=None, y=P, ldy=8, B=1, H=4, W=4, Cin=8, Cout=8, relu=1, stream=None), o)


def dgrad(**o):         # gct2_conv4s2_dgrad / gct2_convT4s2_dgrad
    return _args(dict(ctx=CTX, dtype=BF16, dz=P, lddz=8, w=P, act=P, ldact=8, dx=P, lddx=8, B=1, H=4, W=4, Cin=8, Cout=8, accumulate=0,
                      db=None, db_split=0, db2=None, db_accumulate=0, stream=None), o)


def wgrad(**o):         # gct2_conv4s2_wgrad / gct2_convT4s2_wgrad
    return _args(dict(ctx=CTX, dtype=BF16, x=P, ldx=8, dz=P, lddz=8, dw=P, db=None, B=1, H=4, W=4, Cin=8, Cout=8, accumulate=0, adam=None,
                      stream=None), o)


def head(**o):          # gct2_convT4s2_fwd_head_train
    return _args(dict(ctx=CTX, dtype=BF16, x=P, ldx=8, w=P, bias=None, head_w=P, head_b=None, target=P, pred=None, dy=P, lddy=64,
                      head_dw=P, head_db=None, loss=P, B=1, H=16, W=16, Cin=8, Cout=64, head_Cin=64, head_Cout=3, loss_scale_ptr=None,
                      db=None, x2=None, ldx2=0, accumulate=0, stream=None), o)


def s1_fwd(**o):        # gct2_conv2d_s1_fwd
    return _args(dict(ctx=CTX, dtype=BF16, x=P, ldx=8, w=P, bias=None, y=P, ldy=8, B=1, H=4, W=4, Cin=8, Cout=8, KS=3, relu=1, stream=None), o)


def s1_dgrad(**o):      # gct2_conv2d_s1_dgrad
    return _args(dict(ctx=CTX, dtype=BF16, dz=P, lddz=8, w=P, act=P, ldact=8, dx=P, lddx=8, B=1, H=4, W=4, Cin=8, Cout=8, KS=3, accumulate=0,
                      stream=None), o)


def s1_wgrad(**o):      # gct2_conv2d_s1_wgrad
    return _args(dict(ctx=CTX, dtype=BF16, x=P, ldx=8, dz=P, lddz=8, dw=P, db=None, B=1, H=4, W=4, Cin=8, Cout=8, KS=3, accumulate=0,
                      stream=None), o)


def adam(**o):          # the fields of a gct2_adam_args; n = 2048 holds the 16 * 8 * 8 kernel of the builders above
    return {**dict(p=P, m=P, v=P, shadow=None, shadow_dtype=F32, n=2048, alpha=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, grad_mul=1.0,
                   defer=0, slab_base=None, nslab=0, slab_stride=0), **o}


HUGE = 1 << 27              # B * H * W * 4 >= 2^31 at the 4 x 4 grid of the builders
PLANE = "a ReLU bit plane was registered (gct2_ctx_set_relu_bits), but this call neither writes nor reads one"
PLANE_SHAPE = "ReLU bit plane needs channels % 8 == 0 and ld_bytes >= channels / 8 (got 12, 1)"
KSIZE = "(odd, 1..7: 'same' padding is symmetric then)"
HEAD = "convT4s2_fwd_head_train"
HEAD_NEEDS = (f"{HEAD}: needs a 16-bit dtype, Cout = 64, H and W multiples of 16, 16-byte aligned views, a ctx workspace of "
              "B*(H/16)*(W/16)*288 floats, and 31-bit source offsets: B*H*W*ldx*2 + 2*Cin + 128 and the kernel's 16*Cin*Cout*2 bytes "
              "below 0x7ff00000")
# the fused head's size bound (halo_head_supported, csrc/halo_mfma.hip) at the builder's B = 1, H = W = 16, Cin = 8: the first ldx,
# a multiple of 8, with 256 * ldx * 2 + 2 * 8 + 128 >= 0x7ff00000; and a workspace (fake, like every pointer here) that holds its one
# partial row, so that the size is the ONLY thing the predicate can object to
HEAD_LDX_REFUSED = 0x7ff00000 // 512
HEAD_WS = (P, 288 * 4)
assert 512 * (HEAD_LDX_REFUSED - 8) + 144 < 0x7ff00000 <= 512 * HEAD_LDX_REFUSED + 144 and HEAD_LDX_REFUSED % 8 == 0


def _common(name, build, null, extra=None):
    """the four checks every layer entry point starts with (check_conv_args), in their order"""
    fn = "gct2_" + name
    rows = [(fn, build(dtype=7), {}, EINVAL, f"{name}: unknown dtype 7"),
            (fn, build(**{null: None}), {}, EINVAL, f"{name}: null pointer"),
            (fn, build(Cin=0), {}, EINVAL, f"{name}: non-positive dimension"),
            (fn, build(B=HUGE), {}, EINVAL, f"{name}: B*H*W too large for 32-bit pixel indices"),
            # two mistakes: the earlier check names the call
            (fn, build(dtype=7, **{null: None}), {}, EINVAL, f"{name}: unknown dtype 7"),
            (fn, build(B=HUGE, **(extra or {"Cin": 9})), {}, EINVAL, f"{name}: B*H*W too large for 32-bit pixel indices")]
    return rows


def _adam_rows(name):
    fn = "gct2_" + name
    return [(fn, wgrad(adam=ADAM, accumulate=1), {"adam": adam()}, EINVAL, f"{name}: the fused optimizer step needs accumulate = 0"),
            (fn, wgrad(adam=ADAM), {"adam": adam(m=None)}, EINVAL, "wgrad + adam: null arena pointers"),
            (fn, wgrad(adam=ADAM), {"adam": adam(n=1023)}, EINVAL, "wgrad + adam: range shorter than the weight tensor or misaligned"),
            (fn, wgrad(adam=ADAM), {"adam": adam(v=P + 4)}, EINVAL, "wgrad + adam: range shorter than the weight tensor or misaligned"),
            (fn, wgrad(adam=ADAM, dw=P + 8), {"adam": adam()}, EINVAL, "wgrad + adam: range shorter than the weight tensor or misaligned"),
            # the accumulate check stands in front of the arena checks, the ld check in front of both
            (fn, wgrad(adam=ADAM, accumulate=1), {"adam": adam(p=None)}, EINVAL, f"{name}: the fused optimizer step needs accumulate = 0"),
            (fn, wgrad(adam=ADAM, accumulate=1, lddz=7), {"adam": adam(p=None)}, EINVAL, f"{name}: ld smaller than channel count")]


# (entry point, arguments, {"plane": (pointer, ld_bytes) registered on the ctx first, "adam": fields of the struct behind ADAM,
#  "ws": (pointer, bytes) the ctx's workspace during this row}, code, text)
CASES = (
    # ---- gct2_conv4s2_fwd
    _common("conv4s2_fwd", fwd, "w") + [
        ("gct2_conv4s2_fwd", fwd(H=5), {}, EINVAL, "conv4s2_fwd: H=5 W=4 must be even (skip concat, train.py:114-119)"),
        ("gct2_conv4s2_fwd", fwd(W=3), {}, EINVAL, "conv4s2_fwd: H=4 W=3 must be even (skip concat, train.py:114-119)"),
        ("gct2_conv4s2_fwd", fwd(ldx=7), {}, EINVAL, "conv4s2_fwd: ld smaller than channel count"),
        ("gct2_conv4s2_fwd", fwd(ldy=7), {}, EINVAL, "conv4s2_fwd: ld smaller than channel count"),
        ("gct2_conv4s2_fwd", fwd(H=5, ldx=7), {}, EINVAL, "conv4s2_fwd: H=5 W=4 must be even (skip concat, train.py:114-119)"),
        ("gct2_conv4s2_fwd", fwd(Cout=12, ldy=16), {"plane": (P, 1)}, EINVAL, "conv4s2_fwd: " + PLANE_SHAPE),
        ("gct2_conv4s2_fwd", fwd(Cout=16, ldy=16), {"plane": (P, 1)}, EINVAL,
         "conv4s2_fwd: ReLU bit plane needs channels % 8 == 0 and ld_bytes >= channels / 8 (got 16, 1)"),
        # a rejected call has used its plane up: the next call, which accepts none, fails for its own reason
        ("gct2_conv4s2_fwd", fwd(dtype=7), {"plane": (P, 1)}, EINVAL, "conv4s2_fwd: unknown dtype 7"),
        ("gct2_conv4s2_wgrad", wgrad(ldx=7), {}, EINVAL, "conv4s2_wgrad: ld smaller than channel count")]
    # ---- gct2_conv4s2_dgrad
    + _common("conv4s2_dgrad", dgrad, "dx") + [
        ("gct2_conv4s2_dgrad", dgrad(H=6, W=5), {}, EINVAL, "conv4s2_dgrad: H=6 W=5 must be even"),
        ("gct2_conv4s2_dgrad", dgrad(lddz=7), {}, EINVAL, "conv4s2_dgrad: ld smaller than channel count"),
        ("gct2_conv4s2_dgrad", dgrad(lddx=7), {}, EINVAL, "conv4s2_dgrad: ld smaller than channel count"),
        ("gct2_conv4s2_dgrad", dgrad(ldact=7), {}, EINVAL, "conv4s2_dgrad: ld smaller than channel count"),
        ("gct2_conv4s2_dgrad", dgrad(Cin=12, lddx=16, ldact=16), {"plane": (P, 1)}, EINVAL, "conv4s2_dgrad: " + PLANE_SHAPE),
        ("gct2_conv4s2_dgrad", dgrad(db=P, db_split=-1), {}, EINVAL, "dgrad: db_split out of range"),
        ("gct2_conv4s2_dgrad", dgrad(db=P, db_split=9), {}, EINVAL, "dgrad: db_split out of range")]
    # ---- gct2_conv4s2_wgrad
    + _common("conv4s2_wgrad", wgrad, "dz") + _adam_rows("conv4s2_wgrad") + [
        ("gct2_conv4s2_wgrad", wgrad(), {"plane": (P, 1)}, EINVAL, "conv4s2_wgrad: " + PLANE),
        ("gct2_conv4s2_wgrad", wgrad(dtype=7), {"plane": (P, 1)}, EINVAL, "conv4s2_wgrad: " + PLANE),
        ("gct2_conv4s2_wgrad", wgrad(H=5), {}, EINVAL, "conv4s2_wgrad: H=5 W=4 must be even"),
        ("gct2_conv4s2_wgrad", wgrad(W=7, lddz=7), {}, EINVAL, "conv4s2_wgrad: H=4 W=7 must be even"),
        ("gct2_conv4s2_wgrad", wgrad(ldx=7), {}, EINVAL, "conv4s2_wgrad: ld smaller than channel count"),
        ("gct2_conv4s2_wgrad", wgrad(lddz=7), {}, EINVAL, "conv4s2_wgrad: ld smaller than channel count")]
    # ---- gct2_convT4s2_fwd (odd H and W are fine: the checks see the 2H x 2W output grid)
    + _common("convT4s2_fwd", fwd, "y") + [
        ("gct2_convT4s2_fwd", fwd(B=HUGE // 8), {}, EINVAL, "convT4s2_fwd: B*H*W too large for 32-bit pixel indices"),
        ("gct2_convT4s2_fwd", fwd(H=5, ldx=7), {}, EINVAL, "convT4s2_fwd: ld smaller than channel count"),
        ("gct2_convT4s2_fwd", fwd(ldy=7), {}, EINVAL, "convT4s2_fwd: ld smaller than channel count"),
        ("gct2_convT4s2_fwd", fwd(Cout=12, ldy=16), {"plane": (P, 1)}, EINVAL, "convT4s2_fwd: " + PLANE_SHAPE)]
    # ---- gct2_convT4s2_fwd_head_train
    + _common(HEAD, head, "dy", {"ldx": 7}) + [
        ("gct2_" + HEAD, head(), {"plane": (P, 8)}, EINVAL, f"{HEAD}: " + PLANE),
        ("gct2_" + HEAD, head(head_w=None), {}, EINVAL, f"{HEAD}: null pointer"),
        ("gct2_" + HEAD, head(target=None), {}, EINVAL, f"{HEAD}: null pointer"),
        ("gct2_" + HEAD, head(head_dw=None), {}, EINVAL, f"{HEAD}: null pointer"),
        ("gct2_" + HEAD, head(loss=None), {}, EINVAL, f"{HEAD}: null pointer"),
        ("gct2_" + HEAD, head(ldx=7), {}, EINVAL, f"{HEAD}: ld smaller than channel count"),
        ("gct2_" + HEAD, head(lddy=63), {}, EINVAL, f"{HEAD}: ld smaller than channel count"),
        ("gct2_" + HEAD, head(head_Cout=4), {}, EINVAL,
         f"{HEAD}: head needs <= 3 outputs and <= 3 image channels in a packed x2 (8-byte rows)"),
        ("gct2_" + HEAD, head(head_Cin=63), {}, EINVAL,
         f"{HEAD}: head needs <= 3 outputs and <= 3 image channels in a packed x2 (8-byte rows)"),
        ("gct2_" + HEAD, head(head_Cin=67), {}, EINVAL,
         f"{HEAD}: head needs <= 3 outputs and <= 3 image channels in a packed x2 (8-byte rows)"),
        ("gct2_" + HEAD, head(head_Cin=67, x2=P, ldx2=6), {}, EINVAL,
         f"{HEAD}: head needs <= 3 outputs and <= 3 image channels in a packed x2 (8-byte rows)"),
        # shape and dtype are fine, the ctx has no workspace for the partial rows / the dtype is fp32 / H is no multiple of 16
        ("gct2_" + HEAD, head(), {}, EINVAL,
         HEAD_NEEDS),
        ("gct2_" + HEAD, head(dtype=F32), {}, EINVAL,
         HEAD_NEEDS),
        ("gct2_" + HEAD, head(H=8), {}, EINVAL,
         HEAD_NEEDS),
        # the size bound, with the workspace in place: the source view at the first refused ldx, the kernel at the first refused Cin
        # (16 * Cin * 64 * 2 >= 0x7ff00000), and a source just past 4 GiB, where the kernel's int pixel-times-ldx product would wrap
        ("gct2_" + HEAD, head(ldx=HEAD_LDX_REFUSED), {"ws": HEAD_WS}, EINVAL, HEAD_NEEDS),
        ("gct2_" + HEAD, head(Cin=0x7ff00000 // 2048, ldx=0x7ff00000 // 2048), {"ws": HEAD_WS}, EINVAL, HEAD_NEEDS),
        ("gct2_" + HEAD, head(ldx=(1 << 23) + 8), {"ws": HEAD_WS}, EINVAL, HEAD_NEEDS),
        # its place in the order: behind the ld and the head-shape checks, together with the other needs of the kernel
        ("gct2_" + HEAD, head(ldx=HEAD_LDX_REFUSED, lddy=63), {"ws": HEAD_WS}, EINVAL, f"{HEAD}: ld smaller than channel count"),
        ("gct2_" + HEAD, head(ldx=HEAD_LDX_REFUSED, head_Cout=4), {"ws": HEAD_WS}, EINVAL,
         f"{HEAD}: head needs <= 3 outputs and <= 3 image channels in a packed x2 (8-byte rows)")]
    # ---- gct2_convT4s2_dgrad
    + _common("convT4s2_dgrad", dgrad, "dz") + [
        ("gct2_convT4s2_dgrad", dgrad(H=5, lddz=7), {}, EINVAL, "convT4s2_dgrad: ld smaller than channel count"),
        ("gct2_convT4s2_dgrad", dgrad(lddx=7), {}, EINVAL, "convT4s2_dgrad: ld smaller than channel count"),
        ("gct2_convT4s2_dgrad", dgrad(ldact=7), {}, EINVAL, "convT4s2_dgrad: ld smaller than channel count"),
        ("gct2_convT4s2_dgrad", dgrad(Cin=12, lddx=16, ldact=16), {"plane": (P, 1)}, EINVAL, "convT4s2_dgrad: " + PLANE_SHAPE),
        ("gct2_convT4s2_dgrad", dgrad(db2=P, db_split=9), {}, EINVAL, "dgrad: db_split out of range")]
    # ---- gct2_convT4s2_wgrad
    + _common("convT4s2_wgrad", wgrad, "dw") + _adam_rows("convT4s2_wgrad") + [
        ("gct2_convT4s2_wgrad", wgrad(), {"plane": (P, 1)}, EINVAL, "convT4s2_wgrad: " + PLANE),
        ("gct2_convT4s2_wgrad", wgrad(B=HUGE // 8), {}, EINVAL, "convT4s2_wgrad: B*H*W too large for 32-bit pixel indices"),
        ("gct2_convT4s2_wgrad", wgrad(H=5, ldx=7), {}, EINVAL, "convT4s2_wgrad: ld smaller than channel count"),
        ("gct2_convT4s2_wgrad", wgrad(lddz=7), {}, EINVAL, "convT4s2_wgrad: ld smaller than channel count")]
    # ---- the stride-1 convolutions
    + _common("conv2d_s1_fwd", s1_fwd, "x") + [
        ("gct2_conv2d_s1_fwd", s1_fwd(), {"plane": (P, 1)}, EINVAL, "conv2d_s1_fwd: " + PLANE),
        ("gct2_conv2d_s1_fwd", s1_fwd(KS=0), {}, EINVAL, "conv2d_s1_fwd: kernel size 0 " + KSIZE),
        ("gct2_conv2d_s1_fwd", s1_fwd(KS=4), {}, EINVAL, "conv2d_s1_fwd: kernel size 4 " + KSIZE),
        ("gct2_conv2d_s1_fwd", s1_fwd(KS=9, ldx=7), {}, EINVAL, "conv2d_s1_fwd: kernel size 9 " + KSIZE),
        ("gct2_conv2d_s1_fwd", s1_fwd(KS=9, Cout=0), {}, EINVAL, "conv2d_s1_fwd: non-positive dimension"),
        ("gct2_conv2d_s1_fwd", s1_fwd(ldx=7), {}, EINVAL, "conv2d_s1_fwd: ld smaller than channel count"),
        ("gct2_conv2d_s1_fwd", s1_fwd(KS=7, ldy=7), {}, EINVAL, "conv2d_s1_fwd: ld smaller than channel count")]
    + _common("conv2d_s1_dgrad", s1_dgrad, "w") + [
        ("gct2_conv2d_s1_dgrad", s1_dgrad(), {"plane": (P, 1)}, EINVAL, "conv2d_s1_dgrad: " + PLANE),
        ("gct2_conv2d_s1_dgrad", s1_dgrad(KS=-1), {}, EINVAL, "conv2d_s1_dgrad: kernel size -1 " + KSIZE),
        ("gct2_conv2d_s1_dgrad", s1_dgrad(KS=6, lddz=7), {}, EINVAL, "conv2d_s1_dgrad: kernel size 6 " + KSIZE),
        ("gct2_conv2d_s1_dgrad", s1_dgrad(lddz=7), {}, EINVAL, "conv2d_s1_dgrad: ld smaller than channel count"),
        ("gct2_conv2d_s1_dgrad", s1_dgrad(lddx=7), {}, EINVAL, "conv2d_s1_dgrad: ld smaller than channel count"),
        ("gct2_conv2d_s1_dgrad", s1_dgrad(KS=7, ldact=7), {}, EINVAL, "conv2d_s1_dgrad: ld smaller than channel count")]
    + _common("conv2d_s1_wgrad", s1_wgrad, "dw") + [
        ("gct2_conv2d_s1_wgrad", s1_wgrad(), {"plane": (P, 1)}, EINVAL, "conv2d_s1_wgrad: " + PLANE),
        ("gct2_conv2d_s1_wgrad", s1_wgrad(KS=2), {}, EINVAL, "conv2d_s1_wgrad: kernel size 2 " + KSIZE),
        ("gct2_conv2d_s1_wgrad", s1_wgrad(KS=8, ldx=7), {}, EINVAL, "conv2d_s1_wgrad: kernel size 8 " + KSIZE),
        ("gct2_conv2d_s1_wgrad", s1_wgrad(H=5, ldx=7), {}, EINVAL, "conv2d_s1_wgrad: ld smaller than channel count"),
        ("gct2_conv2d_s1_wgrad", s1_wgrad(KS=1, lddz=7), {}, EINVAL, "conv2d_s1_wgrad: ld smaller than channel count")]
    # ---- the scratch setters
    + [row for name in ("workspace", "wgrad_workspace", "bias_queue") for row in (
        (f"gct2_ctx_set_{name}", [None, P, 64], {}, EINVAL, f"ctx_set_{name}: null ctx"),
        (f"gct2_ctx_set_{name}", [None, P + 4, 64], {}, EINVAL, f"ctx_set_{name}: null ctx"),
        (f"gct2_ctx_set_{name}", [CTX, P + 8, 64], {}, EINVAL, f"ctx_set_{name}: pointer must be 16-byte aligned"),
        (f"gct2_ctx_set_{name}", [CTX, P + 1, 0], {}, EINVAL, f"ctx_set_{name}: pointer must be 16-byte aligned"))]
    # ---- gct2_adam_apply(adam, dw, nw, stream)
    + [("gct2_adam_apply", [None, P, 1024, None], {}, EINVAL, "adam_apply: null pointer"),
       ("gct2_adam_apply", [ADAM, None, 1024, None], {"adam": adam()}, EINVAL, "adam_apply: null pointer"),
       ("gct2_adam_apply", [ADAM, P, 1024, None], {"adam": adam(p=None)}, EINVAL, "wgrad + adam: null arena pointers"),
       ("gct2_adam_apply", [ADAM, P, 1024, None], {"adam": adam(v=None, nslab=-1)}, EINVAL, "wgrad + adam: null arena pointers"),
       ("gct2_adam_apply", [ADAM, P, 4096, None], {"adam": adam()}, EINVAL, "wgrad + adam: range shorter than the weight tensor or misaligned"),
       ("gct2_adam_apply", [ADAM, P + 4, 1024, None], {"adam": adam()}, EINVAL, "wgrad + adam: range shorter than the weight tensor or misaligned"),
       ("gct2_adam_apply", [ADAM, P, 1024, None], {"adam": adam(m=P + 8)}, EINVAL, "wgrad + adam: range shorter than the weight tensor or misaligned"),
       ("gct2_adam_apply", [ADAM, P, 1024, None], {"adam": adam(nslab=-1)}, EINVAL, "adam_apply: bad slab description"),
       ("gct2_adam_apply", [ADAM, P, 1024, None], {"adam": adam(nslab=2, slab_stride=1024)}, EINVAL, "adam_apply: bad slab description"),
       ("gct2_adam_apply", [ADAM, P, 1024, None], {"adam": adam(nslab=2, slab_base=P, slab_stride=1023)}, EINVAL, "adam_apply: bad slab description")]
)


def _child():
    """runs CASES against the library and prints one JSON line: {"device": code of gct2_device_check, "results": [[code, text], ...]}"""
    spec = importlib.util.spec_from_file_location("gct2_lib", os.path.join(ROOT, "gan-class-transfer2_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    lib = L.load()
    out = {"device": lib.gct2_device_check(), "results": []}
    if out["device"] == ENODEV:
        handle = ctypes.c_void_p()
        assert lib.gct2_ctx_create(ctypes.byref(handle)) == 0
        for fn, args, pre, _code, _text in CASES:
            if "plane" in pre:
                assert lib.gct2_ctx_set_relu_bits(handle.value, *pre["plane"]) == 0
            assert lib.gct2_ctx_set_workspace(handle.value, *pre.get("ws", (None, 0))) == 0      # (a row's workspace is its own)
            a = L.AdamArgs(**pre["adam"]) if "adam" in pre else None
            real = [handle.value if v == CTX else ctypes.addressof(a) if v == ADAM else v for v in args]
            code = getattr(lib, fn)(*real)
            out["results"].append([code, lib.gct2_last_error().decode()])
        lib.gct2_ctx_destroy(handle.value)
    print(json.dumps(out))


def test_rejected_calls_keep_their_codes_and_texts():
    import pytest
    env = dict(os.environ)
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if out["device"] != ENODEV:
        pytest.skip(f"a device is visible to the child process (gct2_device_check() = {out['device']}): fake pointers are not sent to it")
    assert len(out["results"]) == len(CASES) >= 35
    wrong = [(i, fn, got, [code, text]) for i, ((fn, _a, _p, code, text), got) in enumerate(zip(CASES, out["results"])) if got != [code, text]]
    assert not wrong, wrong


def test_every_folded_entry_point_is_in_the_table():
    names = {row[0] for row in CASES}
    assert names == {"gct2_conv4s2_fwd", "gct2_conv4s2_dgrad", "gct2_conv4s2_wgrad", "gct2_convT4s2_fwd", "gct2_convT4s2_fwd_head_train",
                     "gct2_convT4s2_dgrad", "gct2_convT4s2_wgrad", "gct2_conv2d_s1_fwd", "gct2_conv2d_s1_dgrad", "gct2_conv2d_s1_wgrad",
                     "gct2_ctx_set_workspace", "gct2_ctx_set_wgrad_workspace", "gct2_ctx_set_bias_queue", "gct2_adam_apply"}


if __name__ == "__main__":
    _child()
