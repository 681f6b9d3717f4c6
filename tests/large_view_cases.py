"""Views whose byte offsets reach 2^31, 2^32 and 2^33 (a plain helper module: no fixtures, no GPU).

include/gct2.h bounds the PIXEL count of a layer call, not its strides: `ld` is any int >= the channel count, so a valid view may span
many GiB although it holds a few thousand elements.  The cases below give ONE operand of a call such a stride and keep everything
else compact; their inputs and fp64 references are the compact case's (tests/exact_cases.py: `ld` is not part of a case's seed), so a
kernel that drops a 64-bit cast, or takes a 32-bit buffer offset past its range, returns values that depend on the image index b.

Span of a view: the byte offset from its pointer to one past its last element, ((pixels - 1) * ld + C) * element size.

Tiers (the target span):
  T1 / T2 / T3   just over 2^31 / 2^32 / 2^33 bytes: `ld` is the smallest multiple of the view's alignment step for which the
                 boundary lies at or before position f (in images) of the view - TIER_GEOMETRY gives (B, f).  T1 and T2: B = 4,
                 f = 2.5: images 0 and 1 lie entirely below the boundary, image 3 entirely above, image 2 straddles it.
                 T3: B = 5, f = 4.5: images 0 .. 3 entirely below; the LAST image straddles the boundary (its lower rows above).
                 A whole image above 2^33 is not possible inside the 10 GiB a case may hold: with B <= 5 equal images the view
                 would span at least 5/4 * 2^33 bytes = 10 GiB before its guard rows.  Rows h >= H/2 + 1 of image 4 are above.
  T0             (16-bit source operands of the matrix-core paths) the largest `ld`, a multiple of 8, that the path's predicate
                 admits - restated below from the comments of tapgemm_mfma_supported / wgrad_mfma_supported / halo_head_supported;
  T0+            T0 plus 8 elements: the first `ld` the predicate refuses (the call falls back to the direct kernels; the fused
                 head, which has no fall-back, returns GCT2_EINVAL).
"""
import functools
import math
from types import SimpleNamespace

import exact_cases as E
from exact_cases import BF16, F16, F32

LIMIT = 0x7ff00000                            # the matrix-core kernels' buffer offsets: 31 bits, bit 31 = "outside the image"
TIER_BYTES = {"T1": 1 << 31, "T2": 1 << 32, "T3": 1 << 33}
TIER_GEOMETRY = {"T1": (4, 2.5), "T2": (4, 2.5), "T3": (5, 4.5), "T0": (4, None), "T0+": (4, None)}
MAX_DEVICE_BYTES = 10 << 30
WORKSPACE_BYTES = 64 << 20                    # tests/test_kernels_exact_gpu.py make_ctx(ws=True)
ES = {F32: 4, BF16: 2, F16: 2}
MODE_DT = {"bf16": BF16, "f16": F16, "f32": F32, "f32m": F32}


# ---- geometry ---------------------------------------------------------------------------------------------------------------------

def span_bytes(pixels, ld, C, es):
    return ((pixels - 1) * ld + C) * es


def image_range(b, hw, ld, C, es):
    """byte offsets [first, one past last) of image b of a [B, hw pixels, C] view"""
    return b * hw * ld * es, ((b * hw + hw - 1) * ld + C) * es


def tier_ld(tier, hw, C, es, step):
    """smallest multiple of `step` elements with the tier's boundary at or before position f (in images) of the view"""
    B, f = TIER_GEOMETRY[tier]
    ld = math.ceil(TIER_BYTES[tier] / (f * hw * es))
    return max((ld + step - 1) // step * step, (C + step - 1) // step * step)


def sides(tier, B, hw, ld, C, es):
    """(images entirely below the tier's boundary, images entirely above it)"""
    bound = TIER_BYTES[tier]
    below = [b for b in range(B) if image_range(b, hw, ld, C, es)[1] <= bound]
    above = [b for b in range(B) if image_range(b, hw, ld, C, es)[0] >= bound]
    return below, above


def last_image_rows(tier, B, h, w, ld, C, es):
    """(whole rows of the LAST image entirely below the boundary, entirely above it)"""
    bound = TIER_BYTES[tier]
    rows = [(((B - 1) * h + r) * w * ld * es, ((((B - 1) * h + r) * w + w - 1) * ld + C) * es) for r in range(h)]
    return sum(1 for lo, hi in rows if hi <= bound), sum(1 for lo, hi in rows if lo >= bound)


# ---- the predicates, restated from the comments in csrc/ ------------------------------------------------------------------------------

def tapgemm_admits(B, Hs, Ws, K, N, ldx):
    """tapgemm_mfma_supported: the source tensor counted on the BIG grid (4 * small grid) plus the shift of the lean issue (one row +
    one pixel) plus the largest tap / chunk offset, and the 16-tap weight tensor, below LIMIT"""
    src = B * Hs * Ws * 4 * ldx * 2
    shift = (2 * Ws + 1) * ldx * 2
    tap_max = (3 * 2 * Ws + 3) * ldx * 2 + K * 2
    return src + shift + tap_max < LIMIT and 16 * K * N * 2 < LIMIT


def wgrad_admits(B, Hs, Ws, ks, ldbig, ldsmall):
    """wgrad_mfma_supported: both operands below LIMIT; the big one lives on the 2Hs x 2Ws grid (stride-1: on the same grid)"""
    return B * Hs * Ws * (1 if ks else 4) * ldbig * 2 < LIMIT and B * Hs * Ws * ldsmall * 2 < LIMIT


def head_admits(B, Hs, Ws, K, N, ldx):
    """halo_head_supported: the source span plus the largest lane (7 * 16 + 16) and k-chunk (< 2 K) offset, and the kernel"""
    return B * Hs * Ws * ldx * 2 + 128 + 2 * K < LIMIT and 16 * K * N * 2 < LIMIT


def largest_ld(admits, C):
    """the largest multiple of 8 that `admits` (monotone) accepts"""
    lo, hi = (C + 7) // 8, 1 << 28
    assert admits(8 * lo) and not admits(8 * hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if admits(8 * mid) else (lo, mid)
    return 8 * lo


# ---- operands of the layer entry points ----------------------------------------------------------------------------------------------

def operands(entry, shape):
    """role -> (B, h, w, C) of every view of an entry point at a case shape (tests/exact_cases.py's shapes)"""
    B, H, W, Cin, Cout = shape[:5]
    if entry == "conv_fwd":
        return {"x": (B, H, W, Cin), "y": (B, H // 2, W // 2, Cout)}
    if entry == "convT_fwd":
        return {"x": (B, H, W, Cin), "y": (B, 2 * H, 2 * W, Cout)}
    if entry == "s1_fwd":
        return {"x": (B, H, W, Cin), "y": (B, H, W, Cout)}
    if entry == "conv_dgrad":
        return {"dz": (B, H // 2, W // 2, Cout), "act": (B, H, W, Cin), "dx": (B, H, W, Cin)}
    if entry == "convT_dgrad":
        return {"dz": (B, 2 * H, 2 * W, Cout), "act": (B, H, W, Cin), "dx": (B, H, W, Cin)}
    if entry == "s1_dgrad":
        return {"dz": (B, H, W, Cout), "act": (B, H, W, Cin), "dx": (B, H, W, Cin)}
    h, w = E.wgrad_hw(entry, shape)
    if entry == "conv_wgrad":
        return {"x": (B, h, w, Cin), "dz": (B, h // 2, w // 2, Cout)}
    if entry == "convT_wgrad":
        return {"x": (B, h, w, Cin), "dz": (B, 2 * h, 2 * w, Cout)}
    assert entry == "s1_wgrad"
    return {"x": (B, h, w, Cin), "dz": (B, h, w, Cout)}


SOURCE_ROLE = {"conv_fwd": "x", "convT_fwd": "x", "s1_fwd": "x", "conv_dgrad": "dz", "convT_dgrad": "dz", "s1_dgrad": "dz"}


def source_predicate(entry, shape, role):
    """ld -> admitted? for the 16-bit source operand `role` of a matrix-core path (every other operand compact, at its channel count
    rounded up to 8)"""
    B, H, W, Cin, Cout = shape[:5]
    up8 = lambda c: (c + 7) // 8 * 8
    if entry in SOURCE_ROLE:
        assert role == SOURCE_ROLE[entry]
        Hs, Ws = (H // 2, W // 2) if entry in ("conv_fwd", "conv_dgrad") else (H, W)
        K, N = (Cin, Cout) if entry.endswith("_fwd") else (Cout, Cin)
        return lambda ld: tapgemm_admits(B, Hs, Ws, K, N, ld)
    h, w = E.wgrad_hw(entry, shape)
    if entry == "conv_wgrad":                 # big = x on the 2Hs x 2Ws grid, small = dz
        Hs, Ws, ks, big = h // 2, w // 2, 0, "x"
    elif entry == "convT_wgrad":              # big = dz, small = x on the Hs x Ws grid
        Hs, Ws, ks, big = h, w, 0, "dz"
    else:
        Hs, Ws, ks, big = h, w, shape[5], "x"
    other = up8(Cout if role == "x" else Cin)
    return (lambda ld: wgrad_admits(B, Hs, Ws, ks, ld, other)) if role == big else (lambda ld: wgrad_admits(B, Hs, Ws, ks, other, ld))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------

def with_batch(shape, tier):
    return (TIER_GEOMETRY[tier][0], *shape[1:])


def make(kind, entry, shape, mode, role, tier, family, step=None, **kw):
    """one case: `role` of `entry` at `shape` (its B replaced by the tier's) gets the tier's stride.  family: the launch-log prefix
    the call must show (None: the path logs nothing)."""
    shape = with_batch(shape, tier)
    dt = MODE_DT[mode]
    es = kw.pop("es", None) or ES[dt]
    B, h, w, C = kw.pop("view", None) or operands(entry, shape)[role]
    step = step or (16 // es if dt != F32 or mode == "f32m" else 1)      # 16-byte pixel rows where a path wants them
    if tier in ("T0", "T0+"):
        pred = kw.pop("predicate", None) or source_predicate(entry, shape, role)
        ld = largest_ld(pred, C) + (8 if tier == "T0+" else 0)
    else:
        pred = None
        ld = tier_ld(tier, h * w, C, es, step)
    c = SimpleNamespace(kind=kind, entry=entry, shape=shape, mode=mode, dt=dt, role=role, tier=tier, family=family, ld=ld, es=es,
                        view=(B, h, w, C), predicate=pred, tuning=0, ws=False, contains=(), split=None, variants=None, special=None)
    c.__dict__.update(kw)
    c.span = span_bytes(B * h * w, ld, C, es)
    c.id = (f"{entry}-{'x'.join(map(str, shape))}-{mode}-{role}-{tier}" + (f"-{kw['tag']}" if "tag" in kw else "")
            + (f"-tuning{c.tuning:x}" if c.tuning else ""))
    return c


def device_bytes(c):
    """what the case holds on the device at its peak: the wide buffer (view + one guard row of w pixels in front and behind), the
    temporaries of the device-side untouched check (exact_cases.UNTOUCHED_PIECE elements: a bool and an int64 each), a compact buffer of
    2 guard images per other view (tests/exact_cases.py poisoned_view, strides below 2 C + 32) and its host-check clone, the scratch,
    the weights"""
    B, h, w, C = c.view
    total = c.span + 2 * w * c.ld * c.es + E.UNTOUCHED_PIECE * 9
    if c.kind in ("tap", "s1", "wgrad", "plane", "colsum", "many"):
        for role, (b, hh, ww, ch) in operands(c.entry, c.shape).items():
            if role != c.role or c.kind == "plane":
                total += 2 * (b + 2) * hh * ww * (2 * ch + 32) * c.es
        KS = c.shape[5] if len(c.shape) == 6 else 4
        total += KS * KS * c.shape[3] * c.shape[4] * 4 * 2
    else:
        # head / pointwise cases: at most 8 compact arrays (views with their guard images and clones, fp32 targets and predictions) of at
        # most 4 x the view's pixels (the head's output grid) and 80 channels of 4 bytes
        total += 8 * 4 * (B + 2) * h * w * 80 * 4
    if c.ws:
        total += WORKSPACE_BYTES
    return total


HALO, NO_HALO = 2 << 24, 1 << 24
BASE = (4, 16, 16, 8, 8)
BASE32 = (4, 32, 32, 8, 8)                    # conv_dgrad: a 16 x 16 small grid, where the halo kernel runs
S1 = (4, 16, 16, 8, 8, 3)
WIDE_N = (4, 16, 16, 8, 72)                   # N > 64: the 256 x 128 tile (tuning 5) and the transposed form's 128 x 128 one
RGB = (4, 16, 16, 3, 8)


ACC = ((1, 0), (1, 1))                       # (masked, accumulate) of the input-gradient cases: dx written, then accumulated into
# entry -> (kind, shape, tuning, 16-bit matrix-core family, fp32 direct family, fp32 matrix-core family); None: the path logs nothing
LAYER_ENTRIES = {
    "conv_fwd": ("tap", BASE, 0, "tap:conv:128x128:", "direct:tap", "f32mfma:conv:"),
    "convT_fwd": ("tap", BASE, HALO, "halo:convT:bias_act", "direct:tap", "f32mfma:convT:"),
    "conv_dgrad": ("tap", BASE32, HALO, "halo:convT:mask", "direct:tap", "f32mfma:convT:"),
    "convT_dgrad": ("tap", BASE, 0, "tap:conv:128x128:mask", "direct:tap", "f32mfma:conv:"),
    "s1_fwd": ("s1", S1, 0, "tap:s1:", None, "f32mfma:s1:"),
    "s1_dgrad": ("s1", S1, 0, "tap:s1:", None, "f32mfma:s1t:"),
    "conv_wgrad": ("wgrad", BASE, 0, "wgrad:128:", "direct:wgrad", "f32mfma:wgrad:"),
    "convT_wgrad": ("wgrad", BASE32, 0, "wgrad:128:", "direct:wgrad", "f32mfma:wgrad:"),
    "s1_wgrad": ("s1", S1, 0, "wgrad:s1:", None, "f32mfma:wgrad_s1:"),
}
DIRECT_16 = {"tap": "direct:tap", "wgrad": "direct:wgrad", "s1": None}      # where a 16-bit call goes that its predicate refuses


def is_source(entry, role):
    """the operands the 16-bit matrix-core kernels load through buffer descriptors: the tensor a forward / input-gradient call reads,
    both tensors of a weight gradient"""
    return entry.endswith("_wgrad") or SOURCE_ROLE[entry] == role


@functools.lru_cache(maxsize=None)
def layer_cases():
    """the issue's table in full: every role of every layer entry point; 16-bit (bf16 and f16 alternate): sources at T0, T0+, T1, T2,
    T3, the other roles at T1 .. T3; fp32 direct and fp32 matrix cores: every role at T2 and T3.  Then the tiles, split-K and the
    image layer, which the default dispatch of the small shapes does not reach."""
    m16 = ["bf16", "f16"]
    n = [0]

    def alt():                                # the 16-bit modes alternate: no need for the full cross product
        n[0] += 1
        return m16[n[0] % 2]

    out = []
    for entry, (kind, shape, tuning, fam16, fam32, fam32m) in LAYER_ENTRIES.items():
        kw = dict(tuning=tuning) if tuning else {}
        if entry.endswith("_dgrad"):
            kw["variants"] = ACC
        for role in operands(entry, shape):
            src = is_source(entry, role)
            for tier in (("T0", "T0+") if src else ()) + ("T1", "T2", "T3"):
                fam = fam16 if (tier == "T0" or not src) else DIRECT_16[kind]
                out.append(make(kind, entry, shape, alt(), role, tier, fam, **kw))
            for mode, fam in (("f32", fam32), ("f32m", fam32m)):
                for tier in ("T2", "T3"):
                    out.append(make(kind, entry, shape, mode, role, tier, fam, **{k: v for k, v in kw.items() if k != "tuning"}))
    # ---- the other tiles: 256 x 128 (tuning 5, N > 64), the transposed form's 256 x 64 (N <= 64) and 128 x 128 (N > 64) without the halo kernel
    out.append(make("tap", "conv_fwd", WIDE_N, alt(), "y", "T2", "tap:conv:256x128:", tuning=5))
    out.append(make("tap", "conv_fwd", WIDE_N, alt(), "x", "T0", "tap:conv:256x128:", tuning=5))
    out.append(make("tap", "convT_fwd", BASE, alt(), "y", "T2", "tap:convT:256x64:", tuning=NO_HALO))
    out.append(make("tap", "convT_fwd", BASE, alt(), "x", "T0", "tap:convT:256x64:", tuning=NO_HALO))
    out.append(make("tap", "convT_fwd", WIDE_N, alt(), "y", "T1", "tap:convT:128x128:", tuning=NO_HALO))
    # ---- split-K: the finalize kernel's opix * ld with a large output (16 output pixels: the widest rows of the file)
    out.append(make("tap", "conv_fwd", E.SPLITK_SHAPE, alt(), "y", "T2", "tap:conv:", ws=True, split=True))
    out.append(make("tap", "convT_dgrad", E.SPLITK_SHAPE, alt(), "dx", "T2", "tap:conv:", ws=True, split=True, variants=ACC))
    # ---- the image layer (Cin = 3): x rows of 4 elements, y
    for role in ("x", "y"):
        out.append(make("tap", "conv_fwd", RGB, alt(), role, "T2", "rgb:fwd", step=4 if role == "x" else 8))
        out.append(make("wgrad", "conv_wgrad", RGB, alt(), "x" if role == "x" else "dz", "T2", "rgb:wgrad", step=4 if role == "x" else 8))
    # ---- both weight-gradient tiles, forced, with slabs
    for tuning, fam in ((3 << 16, "wgrad:128:"), (2 << 16, "wgrad:256q:")):
        out.append(make("wgrad", "conv_wgrad", E.WGRAD_TUNING_SHAPE, alt(), "x", "T0", fam, tuning=tuning, ws=True))
    return out


PLANE_TIER = "T2"                             # "a bit plane whose ld_bytes makes the plane itself span more than 2^32 bytes"


@functools.lru_cache(maxsize=None)
def plane_cases():
    """the ReLU bit plane [pixels][ld_bytes] as the large operand: written by a 16-byte epilogue, derived from the stored y (fp32
    direct kernels: gct2_ctx_set_relu_bits' extra launch), read as the mask of an input gradient"""
    out = []
    for entry, shape, mode, fam, tuning, tag in (("conv_fwd", BASE, "bf16", "tap:conv:128x128:", 0, "written"),
                                                 ("convT_fwd", BASE, "f16", "halo:convT:bias_act:bits", HALO, "written"),
                                                 ("conv_fwd", BASE, "f32", "direct:tap", 0, "derived"),
                                                 ("conv_dgrad", BASE32, "bf16", "halo:convT:mask:bits", HALO, "read")):
        shape = with_batch(shape, PLANE_TIER)
        role = "y" if entry.endswith("_fwd") else "act"
        B, h, w, C = operands(entry, shape)[role]
        out.append(make("plane", entry, shape, mode, "bits", PLANE_TIER, fam, step=4, es=1, view=(B, h, w, C // 8), tuning=tuning, tag=tag))
    return out


@functools.lru_cache(maxsize=None)
def colsum_cases():
    """the fused bias gradients of a DIRECT input gradient: pw_colsum over a large dx (operands from {-1, 0, 1}: the sums are exact)"""
    return [make("colsum", "conv_dgrad", BASE32, "f32", "dx", "T2", "direct:tap", special="pm1", tag="colsum"),
            make("colsum", "conv_dgrad", (4, 32, 32, 12, 8), "bf16", "dx", "T3", "direct:tap", special="pm1", tag="colsum")]


MANY_SHAPE = (5, 512, 512, 8, 8)              # 5 * 2^18 source pixels
# (entry, wide role, ld, family, tuning): with these strides image 4 of the wide view starts exactly at 2^31 bytes (bf16).  A source of
# this size is beyond the matrix-core predicates (they count 4 x the small grid): conv_fwd and conv_wgrad run the direct kernels.
# The halo kernel runs with its OUTPUT wide: 5 * 2^20 output pixels at ld = 256.
MANY = (("conv_fwd", "x", 1024, "direct:tap", 0), ("convT_fwd", "y", 256, "halo:convT:bias_act", HALO), ("conv_wgrad", "x", 1024, "direct:wgrad", 0))


@functools.lru_cache(maxsize=None)
def many_pixel_cases():
    """many pixels, modest ld (T1): the realistic shape of a 2-GiB view"""
    out = []
    for entry, role, ld, fam, tuning in MANY:
        B, h, w, C = operands(entry, MANY_SHAPE)[role]
        c = SimpleNamespace(kind="many", entry=entry, shape=MANY_SHAPE, mode="bf16", dt=BF16, role=role, tier="T1", family=fam, ld=ld,
                            es=2, view=(B, h, w, C), predicate=None, tuning=tuning, ws=False, contains=(), split=None,
                            variants=(1,) if entry != "conv_wgrad" else None, special=None)
        c.span = span_bytes(B * h * w, ld, C, 2)
        c.id = f"{entry}-{'x'.join(map(str, MANY_SHAPE))}-bf16-{role}-T1-many"
        out.append(c)
    return out


# ---- the fused head -------------------------------------------------------------------------------------------------------------------

HEAD_GRID = (16, 16, 16)                      # H, W, Cin of gct2_convT4s2_fwd_head_train's source; Cout = 64, head 67 -> 3


def head_shape(tier):
    return (TIER_GEOMETRY[tier][0], *HEAD_GRID)


@functools.lru_cache(maxsize=None)
def head_cases():
    """role -> view: x [B, 16, 16, 16] (T0: every output per element; T0+, T1, T2: GCT2_EINVAL - family None), dy [B, 32, 32, 64] at
    T1 .. T3, the packed image x2 [B * 32 * 32, 3] (rows of 4 elements) at T1 and T2"""
    out = []
    for role, tier, mode in (("x", "T0", "bf16"), ("x", "T0+", "f16"), ("x", "T1", "bf16"), ("x", "T2", "f16"),
                             ("dy", "T1", "f16"), ("dy", "T2", "bf16"), ("dy", "T3", "f16"), ("x2", "T1", "bf16"), ("x2", "T2", "f16")):
        B, H, W, Cin = head_shape(tier)
        view = {"x": (B, H, W, Cin), "dy": (B, 2 * H, 2 * W, 64), "x2": (B, 2 * H, 2 * W, 3)}[role]
        refused = role == "x" and tier != "T0"
        out.append(make("head", "convT_head", (B, H, W, Cin, 64), mode, role, tier, None if refused else "halo:convT:head", view=view,
                        step=4 if role == "x2" else 8, predicate=(lambda ld, B=B: head_admits(B, H, W, Cin, 64, ld)), ws=True))
    return out


HEAD_REFUSAL = ("convT4s2_fwd_head_train: needs a 16-bit dtype, Cout = 64, H and W multiples of 16, 16-byte aligned views, a ctx workspace "
                "of B*(H/16)*(W/16)*288 floats, and 31-bit source offsets: B*H*W*ldx*2 + 2*Cin + 128 and the kernel's 16*Cin*Cout*2 bytes "
                "below 0x7ff00000")


# ---- pointwise entry points that take a view -----------------------------------------------------------------------------------------------

PW_GRID = (8, 8, 8)                           # h, w, C of the views of gct2_relu_mask / gct2_add (npix = B * 64)
NOISE_HW, NOISE_C = 4, 3                      # tests/pointwise_cases.py noise_case: HW = 4, C = 3, one timestep per image
DENSE_HW = (25, 10)                           # gct2_dense_fwd / _bwd: M = B * 250 rows (a ragged 128-row tile), Cin 67, Cout 3


# (entry, roles, modes it alternates through, view channels by role); every role at T1, T2 and T3
POINTWISE = (
    ("relu_mask", ("act", "d"), ("bf16", "f32", "f16")), ("add", ("dst", "src"), ("bf16", "f32", "f16")),
    ("noise_image", ("out", "out2"), ("bf16", "f32")), ("noise_image_rng", ("out", "out2"), ("f32", "bf16")),
    ("noise_image_table", ("out", "out2"), ("f16", "f32", "bf16")), ("noise_image_rng_table", ("out", "out2"), ("bf16", "f16", "f32")),
    ("dense_fwd", ("x",), ("bf16", "f32", "f16")), ("dense_bwd", ("x", "dx"), ("f32", "f16", "bf16")),
    ("dense_steps_fwd", ("x",), ("f16", "bf16", "f32")), ("dense_steps_bwd", ("x", "dx"), ("bf16", "f32", "f16")),
    ("dense2_fwd", ("x",), ("bf16", "f32", "f16")), ("dense2_bwd", ("x", "dx"), ("f16", "bf16", "f32")),
)


@functools.lru_cache(maxsize=None)
def pointwise_cases():
    """each view of each pointwise entry point at T1, T2 and T3, the dtypes alternating.  The Dense entries run on [B * 250, 67] rows
    (a ragged 128-row tile), dx on 64 channels; the matrix-core form of the hidden pair wants 16-byte rows; the noise views have rows
    of one pixel (the guard rows of 2^27-element strides stay small)."""
    out = []
    for entry, roles, modes in POINTWISE:
        k = 0
        for role in roles:
            for tier in ("T1", "T2", "T3"):
                mode = modes[k % len(modes)]
                k += 1
                B = TIER_GEOMETRY[tier][0]
                if entry in ("relu_mask", "add"):
                    shape, view, step = (B, *PW_GRID, 8), (B, *PW_GRID), 1
                elif entry.startswith("noise"):
                    shape, view, step = (B, NOISE_HW, 1, NOISE_C, NOISE_C), (B, NOISE_HW, 1, NOISE_C), 1
                else:
                    shape, view = (B, *DENSE_HW, 67, 3), (B, *DENSE_HW, 67 if role == "x" else 64)
                    step = 8 if entry.startswith("dense2") and mode != "f32" else 1
                out.append(make("pw", entry, shape, mode, role, tier, None, view=view, step=step))
    return out


# gct2_dense_head_train bounds ldx (its LDS tile holds 256 rows of ldx elements): 512 ldx + 512 Cmask + 4096 + 16 ldx <= 160 KiB, at
# Cmask = 64 ldx <= 240.  A 2-GiB x at that stride would have 4.5 million pixels - far past what the exact head inputs allow
# (tests/exact_cases.py HEAD_MS) - so for x the size contract of this entry point is its refusal.  lddx and ldx2 are not bounded: dx
# and the packed image x2 are wide at the exact head's sizes, through both kernels (the LDS-tile one without a workspace, the matrix-core
# one with a workspace and x2).
DENSE_HEAD_LDX_MAX = 240
DENSE_HEAD_REFUSAL = "dense_head_train: ldx=%d too large for the LDS tile"


@functools.lru_cache(maxsize=None)
def dense_head_cases():
    out = []
    for role, variant, tier, mode in (("dx", "lds", "T1", "f16"), ("dx", "lds", "T2", "bf16"), ("dx", "lds", "T3", "f16"),
                                      ("dx", "ws_x2", "T1", "bf16"), ("dx", "ws_x2", "T2", "f16"), ("dx", "ws_x2", "T3", "bf16"),
                                      ("x2", "ws_x2", "T1", "f16"), ("x2", "ws_x2", "T2", "bf16"), ("x2", "ws_x2", "T3", "f16")):
        B = TIER_GEOMETRY[tier][0]
        out.append(make("pw", "dense_head_train", (B, *DENSE_HW, 67, 3), mode, role, tier, None, view=(B, *DENSE_HW, 64 if role == "dx" else 3),
                        step=8 if role == "dx" else 4, variant=variant, tag=variant, ws=variant != "lds"))
    return out


def all_cases():
    return layer_cases() + plane_cases() + colsum_cases() + many_pixel_cases() + head_cases() + pointwise_cases() + dense_head_cases()
