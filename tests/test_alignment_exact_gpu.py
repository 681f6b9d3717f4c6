"""Every alignment-selected kernel path against the fp64 oracle ELEMENT BY ELEMENT (tests/alignment_cases.py has the placements, the
restated predicates and the case table; tests/test_alignment_cases_cpu.py checks them without a GPU).

The layer entry points take any element-aligned view, and the alignment of a view picks the code that runs: the tap GEMM's 8-byte
epilogue, the direct kernels behind a refusal, the image layer's per-channel loads and plain stores, the scalar staging of the fp32
matrix-core kernels, atomics instead of ordered slabs.  The engine's own buffers never leave the 16-byte side, so this file is what runs
the other one.  Inputs are the exact-sum ones of tests/exact_cases.py: every path must give the reference rounded once, bit for bit,
and leave everything beside its views untouched - there is no tolerance in this file.  Every case proves the branch it names: the
launch log shows the family (and ":e8" where the tap GEMM's 8-byte epilogue applied the epilogue itself), and the predicates restated
in tests/alignment_cases.py give the table's (family, branch) on the pointers the case really passed."""
import numpy as np
import pytest
import torch

import alignment_cases as A
import exact_cases as E
from exact_cases import F32
from test_kernels_exact_gpu import (FN, MODE_DT, check_log, dev, lib, make_ctx, nan_like, run_bias_grads, run_dgrad, run_fwd, run_s1,
                                    run_wgrad, stream)

pytestmark = pytest.mark.gpu


def group(g):
    return [pytest.param(c, id=A.case_id(c)) for c in A.CASES if c.group == g]


def proved(c, place, masked=True):
    """the restated predicates, on the pointers this case passed, name the family and branch of the table"""
    got = A.predict(c.entry, c.shape, c.mode, place.seen, c.tuning, c.workspace, masked, c.opts.get("split", False))
    want = (c.family, c.branch) if masked else (("halo:convT:", "halo") if c.group == "e" else (c.family, "e16"))
    assert got == want, (got, want)


def run_tap(gpu, c, place, **kw):
    run = run_fwd if c.entry.endswith("_fwd") else run_dgrad
    return run(gpu, c.entry, c.shape, c.mode, ws=c.workspace, tuning=c.tuning, place=place, **kw)


def no_e8(log):
    assert not any(":e8" in t for t in log), log


# ---- a, e, f: the tap GEMM's 8-byte epilogue ------------------------------------------------------------------------------------------

def narrow_tap(gpu, c):
    """forward: bias, relu 0 / 1; input gradient: mask on / off, accumulate 0 / 1 - every token with ":e8".  A narrow act alone
    (way "act8") is narrow only where the mask is read: the calls without a mask take the 16-byte side (group e: the halo kernel),
    exact as well, and say so in the log."""
    tokens = tuple(c.opts.get("contains", ()))
    place = A.Aligned(c.placement)
    if c.opts["way"] != "act8":
        run_tap(gpu, c, place, family=c.family, contains=(*tokens, ":e8"))
        return proved(c, place)
    run_tap(gpu, c, place, family=c.family, contains=(*tokens, ":e8"), variants=A.MASKED)
    proved(c, place)
    place = A.Aligned(c.placement)
    if c.group == "e":
        log = run_tap(gpu, c, place, family="halo:convT:", variants=A.UNMASKED)
    else:
        log = run_tap(gpu, c, place, family=c.family, contains=tokens, variants=A.UNMASKED)
    no_e8(log)
    proved(c, place, masked=False)


@pytest.mark.parametrize("c", group("a"))
def test_tap_8_byte_epilogue_exact(gpu, c):
    """the output 8 bytes off, an output stride of 8 k + 4, a narrow act: ragged M / K / N, the forced 128 x 128 and 256 x 128 tiles,
    the 256 x 64 tile of the convT form"""
    narrow_tap(gpu, c)


@pytest.mark.parametrize("c", group("e"))
def test_forced_halo_with_a_narrow_view_falls_back_to_the_tap_kernel(gpu, c):
    """tuning 2 << 24 forces the halo kernel, whose 16-byte epilogue refuses the view: the log shows tap:convT:, never halo:"""
    narrow_tap(gpu, c)


@pytest.mark.parametrize("c", group("f"))
def test_stride_1_forms_with_a_narrow_output_exact(gpu, c):
    place = A.Aligned(c.placement)
    log = run_s1(gpu, c.entry, c.shape, c.mode, False, place=place, prefix=c.family)
    assert all(":e8" in t for t in log), log
    proved(c, place)


# ---- b: fused bias gradients ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", group("b"))
def test_fused_bias_gradients_through_the_8_byte_epilogue_exact(gpu, c):
    """the 8-byte epilogue's own lane-to-channel map of the column sums, in the three reduction modes: atomics (no workspace), partial
    rows, a bias queue with one flush; db / db2 split at 40 and guarded.  A narrow act reaches it too: these calls are all masked.
    Where the workspace makes the call split K, the finalize kernel forms the sums behind the narrow views instead (no ":e8")."""
    place = A.Aligned(c.placement)
    split = c.opts.get("split", False)
    log = run_bias_grads(gpu, c.entry, c.shape, c.mode, c.opts["scratch"], place=place, contains=() if split else (":e8",), tuning=c.tuning)
    assert all((int(t.split("ksplit=")[1].split(":")[0]) > 1) == split for t in log), log
    if split:
        no_e8(log)
    proved(c, place)


# ---- c: split-K ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", group("c"))
def test_split_k_with_a_narrow_output_exact(gpu, c):
    """slabs in the workspace, then the finalize kernel's 8-byte loads and stores on the narrow views: ksplit > 1 in the log and no
    ":e8" (the GEMM kernel applied no epilogue)"""
    place = A.Aligned(c.placement)
    no_e8(run_tap(gpu, c, place, family=c.family, split=True))
    proved(c, place)


# ---- d, h: a registered ReLU bit plane behind a narrow forward ------------------------------------------------------------------------

GUARD_ROWS = 3


def run_plane(gpu, c):
    """relu = 1 with a registered plane: y exact, the log shows relu_bits:derived and no :bits, the plane is the packed (y > 0) of the
    exact reference, the plane bytes beside the view keep their fill"""
    dt = MODE_DT[c.mode]
    cs = E.make_case(c.entry, c.shape, dt)
    B, H, W, Cin, Cout = c.shape
    place = A.Aligned(c.placement)
    ctx = make_ctx(gpu, c.mode, c.workspace, c.tuning)
    xb, xp, ldx = place.inp("x", dev(cs.x, dt, gpu), c.mode, "in")
    wb, wp = place.param("w", dev(cs.w, dt, gpu))
    bb, bp = place.param("bias", dev(cs.bias, F32, gpu))
    y, ldy = place.out("y", nan_like(cs.ref.shape, dt, gpu), c.mode)
    npix, groups = int(np.prod(cs.ref.shape[:-1])), Cout // 8
    ldb, boff = groups + 3, 1
    bits = torch.full((npix + 2 * GUARD_ROWS, ldb), 0xA5, dtype=torch.uint8, device=gpu)
    ctx.set_relu_bits(bits.data_ptr() + GUARD_ROWS * ldb + boff, ldb)
    lib().call(FN[c.entry], ctx.handle, dt, xp, ldx, wp, bp, y.ptr, ldy, B, H, W, Cin, Cout, 1, stream())
    want = E.expected(np.maximum(cs.ref, 0), dt)
    y.check(want, f"{c.entry} {c.shape} {c.mode} with a plane")
    log = ctx.read_launch_log()
    layer = [t for t in log if not t.startswith("relu_bits:")]
    assert "relu_bits:derived" in log and not any(":bits" in t for t in log), log
    assert layer and all(t.startswith(c.family) for t in layer), log
    if c.family.startswith("tap:"):
        assert all(":e8" in t for t in layer), log
    got = bits.cpu().numpy()
    ref = np.packbits((want.float().numpy() > 0).reshape(npix, Cout), axis=1, bitorder="little")
    inner = got[GUARD_ROWS:-GUARD_ROWS]
    assert np.array_equal(inner[:, boff:boff + groups], ref)
    assert 0.1 < np.unpackbits(ref).mean() < 0.9                 # a real mask
    assert (got[:GUARD_ROWS] == 0xA5).all() and (got[-GUARD_ROWS:] == 0xA5).all()
    assert (inner[:, :boff] == 0xA5).all() and (inner[:, boff + groups:] == 0xA5).all()
    proved(c, place)


@pytest.mark.parametrize("c", group("d"))
def test_relu_plane_behind_a_narrow_forward_is_derived(gpu, c):
    run_plane(gpu, c)


# ---- g: refusals --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", group("g"))
def test_one_misaligned_operand_lands_on_the_direct_kernels_exact(gpu, c):
    """x / dz 8 bytes off or with a stride of 8 k + 4, w 8 bytes off, bias 4 bytes off, y / dx 4 or 2 bytes off an 8-byte boundary or with
    an odd stride, act 4 bytes off; weight gradients: dw 4 or 8 bytes off, x or dz 8 bytes off or with a stride of 8 k + 4 - each alone
    turns the call over to the direct kernels (the stride-1 fall-back logs nothing), which take every view"""
    place = A.Aligned(c.placement)
    if c.entry.startswith("s1_"):
        run_s1(gpu, c.entry, c.shape, c.mode, False, place=place, prefix=None)
    elif c.entry.endswith("_wgrad"):
        check_log(run_wgrad(gpu, c.entry, c.shape, c.mode, c.workspace, place=place), c.family)
    elif "act" in c.placement:
        run_tap(gpu, c, place, family=c.family, variants=A.MASKED)
    else:
        run_tap(gpu, c, place, family=c.family)
    proved(c, place)


# ---- h: the image layer -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", group("h"))
def test_image_layer_views_exact(gpu, c):
    """sources: the packed image (ld = Cin), ld = 4 at every 2-byte step of an 8-byte word, ld = 5 and 6 (one load per channel), ld = 8
    and ld = 4 at 8 bytes (8-byte pixel loads: the slots behind Cin hold NaN and must not leak); outputs narrow by pointer and by
    stride (the plain store; a registered plane is derived); the weight gradient on the same sources, and with dw 4 bytes off a
    workspace it has to leave unused (atomics: exact because the inputs are).  The log of the image layer names no load or store form
    and no slab mode: those are proved by the restated predicates alone."""
    if c.opts.get("plane"):
        return run_plane(gpu, c)
    place = A.Aligned(c.placement)
    if c.entry == "conv_fwd":
        run_tap(gpu, c, place, family=c.family)
    else:
        check_log(run_wgrad(gpu, c.entry, c.shape, c.mode, c.workspace, place=place), c.family)
    proved(c, place)


# ---- i: fp32 on the matrix cores ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", group("i"))
def test_f32_matrix_core_staging_forms_exact(gpu, c):
    """F_AVEC / F_BVEC: 16-byte or element-wise staging per operand, all four combinations by misaligning x (dz) and / or w by 4 bytes
    at K % 4 == N % 4 == 0; weight gradients also with dw 4 bytes off under a forced split of 4: atomics, never slabs"""
    place = A.Aligned(c.placement)
    if c.entry.endswith("_wgrad"):
        token = c.opts.get("token")
        log = check_log(run_wgrad(gpu, c.entry, c.shape, c.mode, c.workspace, c.tuning, place=place), c.family, contains=(token,) if token else ())
        if "dw" in c.placement:
            assert not any(":slabs" in t for t in log), log
    elif c.entry.startswith("s1_"):
        run_s1(gpu, c.entry, c.shape, c.mode, False, place=place, prefix=c.family)
    else:
        run_tap(gpu, c, place, family=c.family)
    proved(c, place)
