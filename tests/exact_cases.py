"""Exact-sum inputs for per-element kernel tests (a plain helper module: no fixtures, no GPU).

Idea: operands are integers times a power of two, sized so that EVERY partial sum of a reduction - in any order, tile, split-K slab
or atomic arrival order - is an integer multiple of one grid step below 2^22, hence exact in an fp32 accumulator.  The only rounding
left in a kernel is the documented one at its store, and its output can be compared element by element with the fp64 oracle rounded
once (torch's round-to-nearest-even conversion).

Zeros: +0 and -0 compare equal (the sign of a zero is not part of any contract in include/gct2.h); everything else is compared by
bits, NaN equals NaN, inf equals inf of the same sign.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import denoiser_oracle as O
from oracle import variants_oracle as V

F32, BF16, F16 = 0, 1, 2
TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
DTYPE_NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
SIG_BITS = {F32: 24, BF16: 8, F16: 11}        # significand widths (with the hidden bit) of the storage types
BUDGET = 1 << 22                              # two bits of slack under fp32's 24
GUARD = 64                                    # NaN / sentinel elements in front of and behind weight and bias arrays
SENTINEL = -1234.0                            # exact in f16 and fp32; bf16 stores it as -1232 (compare against the stored value)


# ---- operands -------------------------------------------------------------------------------------------------------------------

def _ints(rng, shape, m, allow_zero):
    if allow_zero:
        return rng.integers(-m, m + 1, shape).astype(np.float64)
    return (rng.integers(1, m + 1, shape) * rng.choice([-1, 1], shape)).astype(np.float64)


def exact_operands(rng, shape, dtype, k_total, allow_zero=True, max_int=None, out_dtype=None):
    """Two float64 operand arrays (shape = (shape_a, shape_b), dtype = one storage type or a pair) for a reduction of k_total
    products plus two single terms (the accumulate operand and the bias).  Values are integers times a power of two; the integer
    ranges are as wide as the storage type (8 / 11 / 24 significand bits) and the budget
        (k_total + 2) * max|a| * max|b| / lsb(a * b) < 2^22
    allow, so short reductions get wide operands.  A 16-bit OUTPUT type adds a third limit, max|a| * max|b| * sqrt(k_total + 2) <
    2^(its significand bits + 7): a sum of k products of uniform integers has a standard deviation of about max|a| max|b| sqrt(k) / 3
    grid steps, so typical sums then lose 5 to 6 bits at the store and a few percent of them are exact ties - with wider operands
    nearly every sum is inexact but hardly any is a tie, and ties are what tells round-to-nearest-even from ties-away.
    max_int narrows both ranges further (the {-1, 0, 1} cases).  Returns a namespace:
    a, b, lsb (the grid step of a * b), ma / mb (largest integers), sa / sb (a = integers / 2^sa)."""
    shape_a, shape_b = shape
    dt_a, dt_b = dtype if isinstance(dtype, tuple) else (dtype, dtype)
    room = (BUDGET - 1) // (k_total + 2)
    assert room >= 1, "reduction too long for the exact-sum budget"
    if out_dtype in (BF16, F16):
        room = max(1, min(room, int(2.0 ** (SIG_BITS[out_dtype] + 7) / math.sqrt(k_total + 2))))
    ma = min(math.isqrt(room), (1 << SIG_BITS[dt_a]) - 1)
    mb = min(room // ma, (1 << SIG_BITS[dt_b]) - 1)
    if max_int is not None:
        ma, mb = min(ma, max_int), min(mb, max_int)
    sa = 0 if max_int is not None else max(ma.bit_length() - 1, 4)
    sb = 0 if max_int is not None else max(mb.bit_length() - 1, 4)
    ia, ib = _ints(rng, shape_a, ma, allow_zero), _ints(rng, shape_b, mb, allow_zero)
    ops = SimpleNamespace(a=ia / 2.0 ** sa, b=ib / 2.0 ** sb, lsb=2.0 ** -(sa + sb), ma=ma, mb=mb, sa=sa, sb=sb, k_total=k_total,
                          step_a=2.0 ** -sa, step_b=2.0 ** -sb)
    assert_budget(ops)
    return ops


def assert_budget(ops):
    """the budget on the arrays as they are (not on the ranges they were drawn from)"""
    amax, bmax = float(np.abs(ops.a).max()), float(np.abs(ops.b).max())
    assert (ops.k_total + 2) * amax * bmax / ops.lsb < BUDGET, (ops.k_total, amax, bmax, ops.lsb)
    step_a, step_b = ops.step_a, ops.step_b      # each operand on its own grid, whose product is the grid of the sums
    assert step_a * step_b >= ops.lsb
    for v, step in ((ops.a, step_a), (ops.b, step_b)):
        assert np.array_equal(np.round(v / step) * step, v)


def exact_bias(rng, n, ops):
    """fp32 bias on the grid of the products, at most one product in size: one term of the budget"""
    m = min(ops.ma * ops.mb, (1 << 24) - 1)
    return rng.integers(-m, m + 1, n).astype(np.float64) * ops.lsb


def exact_addend(rng, shape, dtype, ops):
    """the accumulate operand (what dx holds before an accumulating call): on the product grid, at most one product in size, and
    representable in the storage type"""
    m = ops.ma * ops.mb
    q = max(0, m.bit_length() - SIG_BITS[dtype])
    return rng.integers(-(m >> q), (m >> q) + 1, shape).astype(np.float64) * ops.lsb * 2.0 ** q


def survives_storage(a, dtype):
    """operand == its round trip through the storage type"""
    return bool(np.array_equal(torch.tensor(a, dtype=torch.float64).to(TDT[dtype]).to(torch.float64).numpy(), a))


# ---- expectation and comparison ------------------------------------------------------------------------------------------------------

def expected(ref64, out_dtype):
    """the fp64 reference rounded ONCE to the output type (through float32, which must hold it exactly: it is an exact sum)"""
    t64 = torch.tensor(np.asarray(ref64, dtype=np.float64))
    t32 = t64.to(torch.float32)
    assert torch.equal(t32.to(torch.float64), t64), "the reference is not exact in float32: the inputs break the budget"
    return t32.to(TDT[out_dtype])


_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float64: torch.int64,
             torch.int32: torch.int32}


def _shared_coordinates(idx, shape, names):
    out = []
    for d, name in enumerate(names):
        lo, hi = int(idx[:, d].min()), int(idx[:, d].max())
        if lo == hi and shape[d] > 1:
            out.append(f"all in {name} = {lo}")
        elif lo > 0 and hi == shape[d] - 1:
            out.append(f"all in {name} >= {lo}")
        elif lo == 0 and hi < shape[d] - 1:
            out.append(f"all in {name} <= {hi}")
        elif lo > 0 and hi < shape[d] - 1:
            out.append(f"all in {lo} <= {name} <= {hi}")
    return out


def assert_elementwise_equal(got, want, names=("b", "h", "w", "c"), what=""):
    """bit equality per element (NaN == NaN, +0 == -0); the failure names how many elements differ, the first ten as index tuples
    with both values, and the index coordinates all mismatches share - a border, a tile, a channel range"""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    iv = _INT_VIEW[got.dtype]
    bad = got.view(iv) != want.view(iv)
    bad &= ~(torch.isnan(got) & torch.isnan(want))
    bad &= ~((got == 0) & (want == 0))
    n = int(bad.sum())
    if n == 0:
        return
    names = tuple(names)[-got.dim():] if len(names) >= got.dim() else tuple(f"d{i}" for i in range(got.dim()))
    idx = bad.nonzero().numpy()
    lines = [f"{what + ': ' if what else ''}{n} of {got.numel()} elements differ; first ({', '.join(names)}):"]
    for ix in idx[:10]:
        t = tuple(int(v) for v in ix)
        lines.append(f"  {t}: got {float(got[t])!r} want {float(want[t])!r}")
    shared = _shared_coordinates(idx, got.shape, names)
    lines.append("  shared: " + ("; ".join(shared) if shared else "nothing (spread over every coordinate)"))
    raise AssertionError("\n".join(lines))


# ---- buffers --------------------------------------------------------------------------------------------------------------------

def poisoned_view(t, ld, off, fill=float("nan")):
    """a [B, H, W, C] tensor (rank >= 2: leading dimensions are pixels) at channel offset `off` of a [B + 2, H, W, ld] buffer whose
    other channels and whose two guard images (first and last) hold `fill`: NaN for inputs, a sentinel for outputs.  Returns the
    buffer and the device pointer to channel 0 of pixel 0 of image 1."""
    C = t.shape[-1]
    assert off >= 0 and off + C <= ld
    buf = torch.full((t.shape[0] + 2, *t.shape[1:-1], ld), fill, dtype=t.dtype, device=t.device)
    buf[1:-1, ..., off:off + C] = t
    return buf, buf[1].data_ptr() + off * buf.element_size()


def view_of(buf, off, C):
    return buf[1:-1, ..., off:off + C]


def guarded(t, fill=float("nan"), offset=0):
    """a weight or bias array with GUARD elements of `fill` in front and behind; returns the flat buffer and the pointer to the data.
    offset: the data starts that many elements later (a pointer off the buffer's alignment, tests/alignment_cases.py); the front guard
    grows by them, the one behind keeps its GUARD elements"""
    flat = t.reshape(-1)
    assert offset >= 0
    buf = torch.full((flat.numel() + 2 * GUARD + offset,), fill, dtype=t.dtype, device=t.device)
    buf[GUARD + offset:GUARD + offset + flat.numel()] = flat
    return buf, buf.data_ptr() + (GUARD + offset) * buf.element_size()


def guarded_data(buf, shape):
    return buf[GUARD:buf.numel() - GUARD].reshape(shape)


def assert_outside_untouched(after, before, inside, what=""):
    """everything outside `inside` (a tuple of slices into the buffer) is bit-identical to the snapshot taken before the call"""
    iv = _INT_VIEW[after.dtype]
    a, b = after.detach().cpu().view(iv).clone(), before.detach().cpu().view(iv).clone()
    a[inside] = 0
    b[inside] = 0
    if not torch.equal(a, b):
        idx = (a != b).nonzero()
        raise AssertionError(f"{what}: {idx.shape[0]} elements outside the view changed, first at {tuple(int(v) for v in idx[0])} of {tuple(a.shape)}")


def wide_view(t, ld, fill=float("nan"), guard_pixels=None):
    """a [..., C] tensor (leading dimensions are pixels, row-major) as a view with pixel stride `ld` inside a FLAT buffer filled with
    `fill`, for strides of millions of elements (tests/test_large_views_gpu.py): `guard_pixels` pixels (default: one row, t.shape[-2])
    in front of and behind the view instead of poisoned_view's two guard images.  Returns the buffer, the strided view of it that
    holds t (a torch view: reading it gathers, writing it scatters) and the device pointer to channel 0 of pixel 0."""
    C = t.shape[-1]
    npix = t.numel() // C
    guard = (t.shape[-2] if guard_pixels is None else guard_pixels) * ld
    assert ld >= C
    buf = torch.full((guard + (npix - 1) * ld + C + guard,), fill, dtype=t.dtype, device=t.device)
    strides, s = [], ld
    for n in reversed(t.shape[:-1]):
        strides.insert(0, s)
        s *= n
    view = buf.as_strided(tuple(t.shape), (*strides, 1), guard)
    view.copy_(t)
    return buf, view, buf.data_ptr() + guard * buf.element_size()


UNTOUCHED_PIECE = 1 << 26                     # elements compared at a time by assert_outside_untouched_device


def assert_outside_untouched_device(buf, view, fill, what=""):
    """the device-side sibling of assert_outside_untouched for buffers of many GiB: everything of `buf` (filled with `fill` when it
    was made) outside `view` (a torch view of buf, e.g. wide_view's) still holds the fill value, bit for bit.  The view is MASKED -
    overwritten with the fill value: gather it first - and the whole buffer is compared in pieces of UNTOUCHED_PIECE elements (a bool
    and an int64 of temporaries each); only the count of changed elements and, on failure, the first index come to the host."""
    iv = _INT_VIEW[buf.dtype]
    view.fill_(fill)
    want = torch.full((1,), fill, dtype=buf.dtype, device=buf.device).view(iv)
    flat = buf.view(iv)
    bad = torch.zeros((), dtype=torch.int64, device=buf.device)
    for piece in flat.split(UNTOUCHED_PIECE):
        bad += torch.count_nonzero(piece != want)
    if int(bad):
        at = 0
        for piece in flat.split(UNTOUCHED_PIECE):
            hit = (piece != want).nonzero()
            if hit.numel():
                raise AssertionError(f"{what}: {int(bad)} elements outside the view changed, first at element {at + int(hit[0])} of {flat.numel()}")
            at += piece.numel()


# ---- cases: inputs and fp64 references, shared by the CPU quality checks and the GPU tests ------------------------------------------

# (B, H, W, Cin, Cout) as in tests/test_kernels_gpu.py: H, W the big grid of the Conv2D form and the small one of the transposed form
TAP_SHAPES = [(1, 4, 12, 72, 136), (3, 2, 2, 256, 64), (4, 4, 4, 512, 256), (2, 16, 16, 3, 8), (1, 8, 8, 4, 136), (1, 6, 10, 5, 7)]
SPLITK_SHAPE = (4, 4, 4, 512, 256)
TILE_SHAPES = [(1, 12, 20, 72, 136), (1, 8, 12, 264, 328)]
HALO_CASES = [("convT_fwd", (1, 32, 16, 136, 72)), ("convT_fwd", (1, 16, 16, 8, 8)), ("conv_dgrad", (2, 32, 32, 64, 24))]
WGRAD_SHAPES = [(1, 12, 20, 72, 136), (21, 16, 16, 16, 64), (9, 4, 8, 64, 64), (2, 16, 16, 3, 8), (1, 6, 10, 5, 7), (4, 32, 32, 64, 128)]
WGRAD_TUNING_SHAPE = (4, 32, 32, 64, 128)     # 16 steps of 64 rows: room for four pixel splits
S1_SHAPES = [(1, 5, 7, 3, 8, 3), (1, 9, 11, 24, 40, 5), (2, 6, 4, 40, 16, 1), (2, 4, 4, 264, 128, 3)]     # (..., KS)
DENSE_SHAPE = (1000, 67, 3)                   # M, Cin, Cout
BIAS_GRAD_CASES = [("conv_dgrad", (1, 12, 20, 72, 32)), ("convT_dgrad", (1, 12, 20, 72, 16))]
IMAGE_EXTRA_SHAPES = [(2, 16, 16, 1, 8), (2, 16, 16, 2, 8)]          # the image layer at Cin = 1 and 2 (tests/alignment_cases.py)
TAP_ENTRIES = ("conv_fwd", "convT_fwd", "conv_dgrad", "convT_dgrad")
WGRAD_ENTRIES = ("conv_wgrad", "convT_wgrad")
S1_ENTRIES = ("s1_fwd", "s1_dgrad", "s1_wgrad")
OUT_IS_STORAGE = TAP_ENTRIES + ("s1_fwd", "s1_dgrad")       # entries whose output is stored in the compute dtype


def _seed(entry, shape, dt, special):
    entry = "dense" if entry.startswith("dense") else entry      # both Dense entries run on one set of inputs
    return [sum(ord(ch) for ch in entry + str(special)), dt, *shape]


def _mask_inputs(rng, shape, dt):
    """the tensor whose ReLU produced the layer input: both signs and zeros, representable everywhere"""
    return rng.integers(-3, 4, shape).astype(np.float64) / 2.0


def wgrad_hw(entry, shape):
    """the x grid of a weight-gradient case: the transposed form runs on the halved grid (its dz is the big tensor)"""
    B, H, W = shape[:3]
    return (H // 2, W // 2) if entry == "convT_wgrad" else (H, W)


@functools.lru_cache(maxsize=None)
def make_case(entry, shape, dt, special=None):
    """inputs (float64, exactly representable in their storage types) and fp64 references of one (entry, shape, dtype) case.
    special: None; "pm1" = operands from {-1, 0, 1} (fused bias gradients); "nozero" = operand grids without zero (the inf cases);
    "overflow" = an fp16 input-gradient case scaled by a power of two until 1 % .. 50 % of |ref| reach 65520."""
    rng = np.random.default_rng(_seed(entry, shape, dt, special))
    c = SimpleNamespace(entry=entry, shape=shape, dt=dt, special=special, out_dt=dt if entry in OUT_IS_STORAGE else F32)
    kw = dict(allow_zero=special != "nozero", max_int=1 if special == "pm1" else None, out_dtype=c.out_dt)
    if entry in ("dense_fwd", "dense_bwd"):
        return _dense_case(c, rng)
    if entry == "head_train":
        return _head_case(c, rng)
    if entry == "convT_head":
        return _convT_head_case(c, rng)
    KS = shape[5] if len(shape) == 6 else 4
    B, H, W, Cin, Cout = shape[:5]
    s1 = entry.startswith("s1_")
    if entry in ("conv_fwd", "convT_fwd", "s1_fwd"):
        wshape = (4, 4, Cout, Cin) if entry == "convT_fwd" else (KS, KS, Cin, Cout)
        ops = exact_operands(rng, ((B, H, W, Cin), wshape), dt, KS * KS * Cin, **kw)
        c.x, c.w, c.ops = ops.a, ops.b, ops
        c.bias = exact_bias(rng, Cout, ops)
        f = {"conv_fwd": O.conv4s2_fwd, "convT_fwd": O.convT4s2_fwd, "s1_fwd": V.conv_s1_fwd}[entry]
        c.ref = f(c.x, c.w, c.bias)
        c.terms_of = functools.partial(_fwd_terms, c) if entry == "conv_fwd" else None
    elif entry in ("conv_dgrad", "convT_dgrad", "s1_dgrad"):
        dzshape = {"conv_dgrad": (B, H // 2, W // 2, Cout), "convT_dgrad": (B, 2 * H, 2 * W, Cout), "s1_dgrad": (B, H, W, Cout)}[entry]
        wshape = (4, 4, Cout, Cin) if entry == "convT_dgrad" else (KS, KS, Cin, Cout)
        ops = exact_operands(rng, (dzshape, wshape), dt, KS * KS * Cout, **kw)
        c.dz, c.w, c.ops = ops.a, ops.b, ops
        c.act = _mask_inputs(rng, (B, H, W, Cin), dt)
        c.prev = exact_addend(rng, (B, H, W, Cin), dt, ops)
        if special == "overflow":
            _scale_to_overflow(c)
        c.ref = dgrad_of(entry, c.dz, c.w, (B, H, W, Cin))
    else:
        h, w_ = wgrad_hw(entry, shape)
        dzshape = {"conv_wgrad": (B, h // 2, w_ // 2, Cout), "convT_wgrad": (B, 2 * h, 2 * w_, Cout), "s1_wgrad": (B, h, w_, Cout)}[entry]
        # the budget covers the column sums of dz of the SECOND (accumulating) call as well: 2 x the pixels of the larger grid
        npix = 2 * B * max(h * w_, dzshape[1] * dzshape[2])
        ops = exact_operands(rng, ((B, h, w_, Cin), dzshape), dt, npix, **kw)
        c.x, c.dz, c.ops = ops.a, ops.b, ops
        c.dw, c.db = wgrad_of(entry, c.x, c.dz, KS)
        # db sums dz alone: exact when the sum of magnitudes (twice: the accumulating call) stays below 2^24 steps of dz
        assert 2 * np.abs(c.dz).reshape(-1, Cout).sum(0).max() * 2.0 ** ops.sb < (1 << 24)
        c.ref = c.dw
        c.terms_of = functools.partial(_wgrad_terms, c) if entry == "conv_wgrad" else None
    return c


def wgrad_of(entry, x, dz, KS=4):
    """(dw, db) in the Keras layout of the layer"""
    Cin, Cout = x.shape[-1], dz.shape[-1]
    if entry == "conv_wgrad":
        return O.conv4s2_bwd(x, np.zeros((4, 4, Cin, Cout)), dz)[1:]
    if entry == "convT_wgrad":
        return O.convT4s2_bwd(x, np.zeros((4, 4, Cout, Cin)), dz)[1:]
    return V.conv_s1_bwd(x, np.zeros((KS, KS, Cin, Cout)), dz)[1:]


def dgrad_of(entry, dz, w, xshape):
    zeros = np.zeros(xshape)
    if entry == "conv_dgrad":
        return O.conv4s2_bwd(zeros, w, dz)[0]
    if entry == "convT_dgrad":
        return O.convT4s2_bwd(zeros, w, dz)[0]
    return V.conv_s1_bwd(zeros, w, dz)[0]


def dgrad_ref(c, masked, accumulate):
    """dx (+)= mask * g with the mask as a select"""
    g = np.where(c.act > 0, c.ref, 0.0) if masked else c.ref
    return g + c.prev if accumulate else g


def _scale_to_overflow(c):
    """multiplies dz by the smallest power of two for which at least 1 % of the masked |gradient| reach 65520 (fp16 rounds those to
    inf; 65504 is the largest finite value); the budget counts grid steps and is not touched"""
    g = np.where(c.act > 0, dgrad_of(c.entry, c.dz, c.w, c.act.shape), 0.0)
    for j in range(1, 15):
        share = float(np.mean(np.abs(g) * 2.0 ** j >= 65520))
        if share >= 0.01:
            break
    assert 0.01 <= share <= 0.5, share
    c.dz = c.dz * 2.0 ** j
    c.prev = c.prev * 0.0
    c.ops.a, c.ops.lsb, c.ops.step_a = c.dz, c.ops.lsb * 2.0 ** j, c.ops.step_a * 2.0 ** j
    c.overflow_share = share
    assert survives_storage(c.dz, F16)


def _dense_case(c, rng):
    """Dense(3) head: x in the compute dtype, w / b / dy fp32.  One x serves both calls: x * dy sums over M rows (dw), x * w over
    Cin (the prediction) and dy * w over Cout (dx); GCT2_F16 reads dy as fp16, so dy stays within 11 bits."""
    M, Cin, Cout = c.shape
    ops = exact_operands(rng, ((M, Cin), (M, Cout)), (c.dt, F16 if c.dt == F16 else F32), M)
    c.x = np.maximum(ops.a, 0.0)                       # the ReLU output that feeds the head
    c.dy, c.ops = ops.b, ops
    mw = min((BUDGET - 1) // ((Cin + 2) * ops.ma), (BUDGET - 1) // ((Cout + 2) * ops.mb), (1 << 24) - 1)
    if c.dt != F32:      # the tie limit of exact_operands for the 16-bit stores: dx always, the prediction in GCT2_F16
        mw = min(mw, int(2.0 ** (SIG_BITS[c.dt] + 7) / math.sqrt(Cout + 2)) // ops.mb)
    if c.dt == F16:
        mw = min(mw, int(2.0 ** (SIG_BITS[F16] + 7) / math.sqrt(Cin + 2)) // ops.ma)
    mw = max(mw, 1)
    sw = max(mw.bit_length() - 1, 4)
    c.w = _ints(rng, (Cin, Cout), mw, True) / 2.0 ** sw
    c.bias = rng.integers(-ops.ma * mw, ops.ma * mw + 1, Cout).astype(np.float64) * 2.0 ** -(ops.sa + sw)
    c.fwd_ops = SimpleNamespace(a=c.x, b=c.w, lsb=2.0 ** -(ops.sa + sw), k_total=Cin, step_a=ops.step_a, step_b=2.0 ** -sw)
    c.dx_ops = SimpleNamespace(a=c.dy, b=c.w, lsb=2.0 ** -(ops.sb + sw), k_total=Cout, step_a=ops.step_b, step_b=2.0 ** -sw)
    for o in (c.fwd_ops, c.dx_ops):
        assert_budget(o)
    c.pred = c.x @ c.w + c.bias
    c.dx = np.where(c.x > 0, c.dy @ c.w.T, 0.0)
    c.dw = c.x.T @ c.dy
    c.db = c.dy.sum(0)
    assert np.abs(c.dy).sum(0).max() * 2.0 ** ops.sb < (1 << 24)
    c.ref = c.pred if c.entry == "dense_fwd" else c.dx
    c.out_dt = c.dt if c.entry == "dense_bwd" or c.dt == F16 else F32      # the prediction is fp32 (GCT2_F16: an fp16 value held in fp32)
    c.terms_of = functools.partial(_dense_terms, c)
    return c


# ---- the terms of single outputs (order-independence check) ----------------------------------------------------------------------------

def _fwd_terms(c, index):
    b, oh, ow, o = index
    B, H, W, Cin, Cout = c.shape
    t = [c.bias[o]]
    for kh in range(4):
        for kw in range(4):
            ih, iw = 2 * oh + kh - 1, 2 * ow + kw - 1
            if 0 <= ih < H and 0 <= iw < W:
                t.extend(c.x[b, ih, iw, :] * c.w[kh, kw, :, o])
    return np.array(t)


def _wgrad_terms(c, index):
    kh, kw, i, o = index
    B, H, W, Cin, Cout = c.shape
    t = []
    for oh in range(H // 2):
        for ow in range(W // 2):
            ih, iw = 2 * oh + kh - 1, 2 * ow + kw - 1
            if 0 <= ih < H and 0 <= iw < W:
                t.extend(c.x[:, ih, iw, i] * c.dz[:, oh, ow, o])
    return np.array(t)


def _dense_terms(c, index):
    m, o = index
    return np.concatenate([[c.bias[o]], c.x[m] * c.w[:, o]])


# ---- the GPU case list (tests/test_kernels_exact_gpu.py runs it; tests/test_exact_cases_cpu.py checks the inputs of every entry) ---------

def reference_cases():
    """every (entry, shape, dtype, special) whose inputs a test of tests/test_kernels_exact_gpu.py or tests/test_alignment_exact_gpu.py
    uses"""
    out = [(entry, s, dt, None) for dt in (BF16, F16) for entry in ("conv_fwd", "conv_wgrad") for s in IMAGE_EXTRA_SHAPES]
    for dt in (F32, BF16, F16):
        for entry in TAP_ENTRIES:
            out += [(entry, s, dt, None) for s in TAP_SHAPES]
        for entry in WGRAD_ENTRIES:
            out += [(entry, s, dt, None) for s in WGRAD_SHAPES]
        for entry in S1_ENTRIES:
            out += [(entry, s, dt, None) for s in S1_SHAPES]
        out += [("dense_fwd", DENSE_SHAPE, dt, None), ("dense_bwd", DENSE_SHAPE, dt, None)]
    for dt in (BF16, F16):
        for entry in TAP_ENTRIES:
            out += [(entry, s, dt, None) for s in TILE_SHAPES]
        out += [(entry, s, dt, None) for entry, s in HALO_CASES]
    return out


OVERFLOW_CASES = [("conv_dgrad", (1, 4, 12, 72, 136)), ("convT_dgrad", (1, 4, 12, 72, 136)), ("conv_dgrad", (2, 32, 32, 64, 24)),
                  ("conv_dgrad", SPLITK_SHAPE), ("convT_dgrad", SPLITK_SHAPE), ("conv_dgrad", (1, 6, 10, 5, 7)), ("convT_dgrad", (1, 6, 10, 5, 7))]


def special_cases():
    """the cases with special operand grids: {-1, 0, 1} (fused bias gradients), scaled into fp16 overflow, grids without zero (inf)"""
    out = [(e, s, dt, "pm1") for e, s in BIAS_GRAD_CASES for dt in (F32, BF16, F16)]
    out += [(e, s, F16, "overflow") for e, s in OVERFLOW_CASES]
    out += [(e, s, dt, "nozero") for e, s in OVERFLOW_CASES for dt in (BF16, F16)]
    out += [(e, (1, 4, 12, 72, 136), F32, "nozero") for e in ("conv_dgrad", "convT_dgrad")]
    out += [(e, (4, 32, 32, 64, 128), dt, "nozero") for e in WGRAD_ENTRIES for dt in (F32, BF16, F16)]
    return out


# ---- the fused train-step head on exact inputs (tests/test_fused_exact_gpu.py) ----------------------------------------------------------
#
# gct2_dense_head_train and gct2_convT4s2_fwd_head_train chain four contractions: pred = x w + b, dx = dpred w^T, dw = x^T dpred and
# the column sums (db, db_dx, the loss).  Every one of them is kept an exact sum:
#   x = relu(integers / 2^HEAD_SA), w = integers / 2^sw, b on the grid lsb = 2^-(HEAD_SA + sw) of their products;
#   target = pred_r - delta * lsb with integers delta (pred_r: the exact prediction, rounded to fp16 first in GCT2_F16), so that
#   d = pred_r - target = delta * lsb is exact, and the loss scale is M * Cout * 2^j: gscale = scale * 2 / (M * Cout) = 2^(j + 1) for
#   any order of the one division, dpred = d * gscale exact (one fp16 rounding in GCT2_F16);  j = sw - 1 puts dpred on the grid 2^-2
#   and dx on 2^-(2 + sw) >= 2^-14: nothing is subnormal in fp16.
# The budget is taken on the arrays as drawn: the sum of the MAGNITUDES of the terms of every reduction stays below BUDGET steps of its
# grid, hence every partial sum of every order is exact in an fp32 accumulator (the sum of delta^2 below 2^24: it has one order per kernel
# and nothing is added to it).  The matrix-core kernels carry w and d as multi-term sums of the storage type and drop the product of the
# two LOW terms in the backward pass, so the columns are drawn such that never both have one: column 0 has wide weights and narrow
# deltas, column 1 narrow weights and wide deltas, column 2 both within one term.
HEAD_SHAPE = (67, 3, 72, 64)                  # Cin, Cout, ld, Cmask
HEAD_MS = (5, 16, 1000, 32775)                # < one 16-pixel group; one group; ragged 256-pixel tile and group; > one trip per wave of 512 work-groups
HEAD_WIDE_M = 64
HEAD_SA = 2                                   # x = integers / 4, at most 7 / 4
HEAD_XMAX = 7
CONVT_HEAD_SHAPES = [(1, 16, 16, 8), (2, 16, 32, 136)]       # (B, H, W, Cin) of gct2_convT4s2_fwd_head_train; Cout = 64, head 67 -> 3


def _head_ranges(M, dt):
    """per output column: largest weight integer, largest delta, and (column 1 only) the share of pixels whose delta is wide.
    The ranges shrink with M because db_dx, dw and the sum of delta^2 grow with it (tests/test_exact_cases_cpu.py decides)."""
    if M <= 64:
        return ((4095, 15, 63), (3, 511, 63), 1.0) if dt == BF16 else ((4095, 127, 63), (15, 511, 63), 1.0)
    if M <= 1000:
        return (2047, 15, 31), (3 if dt == BF16 else 7, 511, 31), 0.03
    return (319, 7, 31), (1, 15, 7), 0.0


def _round_to(a, dt):
    return torch.tensor(np.asarray(a, dtype=np.float64)).to(TDT[dt]).to(torch.float64).numpy()


def _wide_deltas(rng, n, dmax, share):
    """deltas of column 1: |delta| <= 15 everywhere, and in `share` of the pixels one with more than 8 significant bits"""
    d = rng.integers(-min(dmax, 15), min(dmax, 15) + 1, n).astype(np.float64)
    if dmax <= 256:
        return d
    wide = rng.random(n) < share
    big = (rng.integers(257, dmax + 1, n) | 1) * rng.choice([-1, 1], n)
    return np.where(wide, big, d)


def _head_tail(c, rng, xin, wmax, dmax, share, sw, tails=None):
    """everything behind the head's input `xin` [M, Cin] (exact in the storage type): kernel, bias, target, loss scale and the fp64
    references of every output of the fused head.  tails: {column: (lo, hi, share)} - in `share` of the pixels that column's delta
    is an odd integer of magnitude lo .. hi instead (the few large residuals the budget of a long reduction leaves room for)"""
    M, Cin = xin.shape
    Cout, Cmask = 3, 64
    c.sw, c.lsb = sw, c.x_step * 2.0 ** -sw
    c.w = np.stack([_ints(rng, Cin, wmax[o], True) for o in range(Cout)], 1) / 2.0 ** sw
    c.w[:, 0] = np.where(c.w[:, 0] != 0, (np.round(c.w[:, 0] * 2.0 ** sw).astype(np.int64) | 1) / 2.0 ** sw, 0.0)   # odd: the low term is there
    c.bias = rng.integers(-wmax[0], wmax[0] + 1, Cout).astype(np.float64) * c.lsb
    c.pred = xin @ c.w + c.bias
    c.pred_r = _round_to(c.pred, F16) if c.dt == F16 else c.pred
    c.delta = np.stack([rng.integers(-dmax[0], dmax[0] + 1, M).astype(np.float64), _wide_deltas(rng, M, dmax[1], share),
                        rng.integers(-dmax[2], dmax[2] + 1, M).astype(np.float64)], 1)
    for col, (lo, hi, part) in (tails or {}).items():
        big = (rng.integers(lo, hi + 1, M) | 1) * rng.choice([-1, 1], M)
        c.delta[:, col] = np.where(rng.random(M) < part, big, c.delta[:, col])
    c.target = c.pred_r - c.delta * c.lsb
    c.j = sw - 1 - int(round(math.log2(c.x_step * 4)))            # dpred on the grid 2^-2
    c.gscale = 2.0 ** (c.j + 1)
    c.loss_scale = float(M * Cout) * 2.0 ** c.j
    c.d = c.pred_r - c.target
    c.dpred = c.d * c.gscale
    if c.dt == F16:
        c.dpred = _round_to(c.dpred, F16)
    c.g = c.dpred @ c.w[:Cmask].T                                 # the unmasked gradient rows
    c.dx = np.where(xin[:, :Cmask] > 0, c.g, 0.0)
    c.dw, c.db = xin.T @ c.dpred, c.dpred.sum(0)
    c.db_dx = c.dx.sum(0)                                         # of the fp32 rows (matrix-core kernels)
    c.db_dx_stored = _round_to(c.dx, c.dt).sum(0)                 # of the stored rows (LDS kernel)
    c.loss = float((c.d * c.d).sum() / (M * Cout))
    c.dp_step, c.dx_step = 0.25, 0.25 * 2.0 ** -sw
    # what the accumulating call finds in dw / db / db_dx: on the grids, a few steps in size
    c.prev_dw = rng.integers(-64, 65, c.dw.shape) * c.x_step * c.dp_step
    c.prev_db = rng.integers(-64, 65, Cout) * c.dp_step
    c.prev_db_dx = rng.integers(-64, 65, Cmask) * c.dx_step * 256
    return c


def head_budgets(c, xin):
    """(name, sum of the magnitudes of the terms of the worst output, grid step) of every reduction of the head"""
    Cmask = 64
    dxr = _round_to(c.dx, c.dt)
    return [("pred", float((np.abs(xin) @ np.abs(c.w) + np.abs(c.bias)).max()), c.lsb),
            ("dx", float((np.abs(c.dpred) @ np.abs(c.w[:Cmask]).T).max()), c.dx_step),
            ("dw", float((np.abs(xin).T @ np.abs(c.dpred) + np.abs(c.prev_dw)).max()), c.x_step * c.dp_step),
            ("db", float((np.abs(c.dpred).sum(0) + np.abs(c.prev_db)).max()), c.dp_step),
            ("db_dx", float((np.abs(c.dx).sum(0) + np.abs(c.prev_db_dx)).max()), c.dx_step),
            ("db_dx_stored", float((np.abs(dxr).sum(0) + np.abs(c.prev_db_dx)).max()), c.dx_step)]


def _head_case(c, rng):
    """make_case("head_train", (M, Cin, Cout), dt, special): special None or "wide" (M = 64: |delta| up to 2^12 and 24-bit weights -
    the backward pass is then a two-term approximation, tests/test_fused_exact_gpu.py bounds it)"""
    M, Cin, Cout = c.shape
    assert (Cin, Cout) == HEAD_SHAPE[:2]
    c.x_step = 2.0 ** -HEAD_SA
    c.x = np.maximum(_ints(rng, (M, Cin), HEAD_XMAX, True), 0.0) * c.x_step
    if c.special == "wide":
        c.sw = 24
        c.w = _ints(rng, (Cin, Cout), (1 << 24) - 1, False) / 2.0 ** 24
        c.lsb = c.x_step * 2.0 ** -24
        c.bias = _ints(rng, Cout, 1 << 20, True) * 2.0 ** -20
        c.pred = c.x @ c.w + c.bias
        c.delta = _ints(rng, (M, Cout), 1 << 12, False)
        c.target = _round_to(c.pred - c.delta * 2.0 ** -12, F32)          # d = delta * 2^-12 up to the fp32 rounding of the target
        c.j = 1                                                           # d in [2^-12, 1], dpred = 4 d: both normal in fp16
        c.gscale = 2.0 ** (c.j + 1)
        c.loss_scale = float(M * Cout) * 2.0 ** c.j
        return c
    wmax, dmax, share = _head_ranges(M, c.dt)
    # fp16 at the largest M: db_dx keeps the mean |dx| below 256 steps, the store rounds from 2048 on - a few pixels get there
    tails = {0: (9, 15, 0.003)} if c.dt == F16 and M > 1000 else None
    return _head_tail(c, rng, c.x, wmax, dmax, share, wmax[0].bit_length(), tails)


# largest operand integer of the transposed convolution and the head's ranges, by (Cin, dtype): y = relu(convT(x) + bias) has a standard
# deviation of about 200 steps in bf16 and 1500 in fp16, so that 5 % and more of the positive y lose bits at the 16-bit conversion
# Tails: bf16 - a few column-1 residuals of 9 bits (the second term of dpred in the epilogue's two-term contractions; the column's
# weights fit one term); fp16 - a few column-0 residuals that carry dy past 2048 steps, where the fp16 store rounds.
_CONVT_HEAD_RANGES = {
    (8, BF16): (10, (511, 15, 31), (15, 31, 15), {1: (257, 511, 0.02)}), (8, F16): (28, (63, 15, 31), (1, 3, 1), {0: (33, 63, 0.015)}),
    (136, BF16): (5, (511, 15, 31), (7, 3, 7), {1: (257, 511, 0.01)}), (136, F16): (14, (63, 15, 31), (1, 1, 1), {0: (33, 63, 0.005)}),
    # Cin = 16: the B = 4 and B = 5 cases of tests/large_view_cases.py (4096 / 5120 output pixels; tests/test_large_view_cases_cpu.py
    # checks their budgets)
    (16, BF16): (9, (511, 15, 31), (4, 3, 4), {1: (257, 511, 0.004)}), (16, F16): (22, (63, 15, 31), (1, 1, 1), {0: (33, 63, 0.003)}),
}


def _convT_head_case(c, rng):
    """make_case("convT_head", (B, H, W, Cin), dt): UpShuffle_0's forward with the head in its epilogue.  Operands of the transposed
    convolution are small integers (grid 1), y an exact sum; the head reads y rounded once to the storage type and three image
    channels from the packed view, and from there everything follows _head_tail."""
    B, H, W, Cin = c.shape
    mi, wmax, dmax, tails = _CONVT_HEAD_RANGES[(Cin, c.dt)]
    ops = exact_operands(rng, ((B, H, W, Cin), (4, 4, 64, Cin)), c.dt, 4 * Cin, max_int=mi)
    c.ops, c.xc, c.wc = ops, ops.a, ops.b
    c.bc = rng.integers(-mi * mi, mi * mi + 1, 64).astype(np.float64)
    c.y = np.maximum(O.convT4s2_fwd(c.xc, c.wc, c.bc), 0.0)
    c.yr = _round_to(c.y, c.dt)
    M = B * 4 * H * W
    c.img = _ints(rng, (M, 3), HEAD_XMAX, True)
    c.x_step = 1.0
    c.x = np.concatenate([c.yr.reshape(M, 64), c.img], 1)         # the head's input
    return _head_tail(c, rng, c.x, wmax, dmax, 0.0, wmax[0].bit_length(), tails)


def fused_cases():
    """every (entry, shape, dtype, special) of tests/test_fused_exact_gpu.py's head tests"""
    out = [("head_train", (M, 67, 3), dt, None) for dt in (BF16, F16) for M in HEAD_MS]
    out += [("head_train", (HEAD_WIDE_M, 67, 3), dt, "wide") for dt in (BF16, F16)]
    out += [("convT_head", s, dt, None) for dt in (BF16, F16) for s in CONVT_HEAD_SHAPES]
    return out


# (entry, B): (B, 32, 32, 8, 8) leaves B slabs by wgrad_mfma()'s rule (one owner at B = 1); the fused optimizer step sums them
ADAM_SLAB_BS = (1, 2, 8, 9, 10, 17)


def adam_slab_shape(B):
    return (B, 32, 32, 8, 8)


def adam_cases():
    """the weight-gradient cases behind which tests/test_fused_exact_gpu.py runs the fused optimizer step"""
    out = [(e, adam_slab_shape(B), dt, None) for e in WGRAD_ENTRIES for dt in (BF16, F16) for B in ADAM_SLAB_BS]
    out += [(e, adam_slab_shape(2), F32, None) for e in WGRAD_ENTRIES]
    out += [(e, (2, 16, 16, 3, 8), dt, None) for e in WGRAD_ENTRIES for dt in (BF16, F16)]
    return out
