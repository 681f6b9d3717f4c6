"""Alignment-selected kernel paths: placements, the host-side predicates restated, and the case table (a plain helper module: no
fixtures, no GPU).

The layer entry points of include/gct2.h take any element-aligned view; what the alignment of a view decides is which code runs.
Every predicate and launch function of the library compares pointer residues and `ld % 8` / `ld % 4` and picks a kernel family, an
epilogue or a load form.  This module
  * places every operand of a case at a stated (pointer residue modulo 16 bytes, ld residue modulo 8 elements) - `Aligned`, a
    tests/test_kernels_exact_gpu.py `Place` - inside NaN (inputs) or sentinel (outputs) filled buffers,
  * restates the predicates in Python on the pointers a placement really made - `predict` returns the launch-log family and the name
    of the branch the call must reach - and
  * lists the cases (`CASES`) that tests/test_alignment_cases_cpu.py checks without a GPU and tests/test_alignment_exact_gpu.py runs.

The branch names are the rows of DESIGN.md section 3, "Alignment classes" (`BRANCHES`).
"""
from collections import namedtuple

import torch

import exact_cases as E
from exact_cases import BF16, F16, F32, SENTINEL
from test_kernels_exact_gpu import FORM, MODE_DT, Out, Place

NAN = float("nan")
VIEW_ROLES = ("x", "dz", "act", "y", "dx")               # pixel views: (pointer, ld)
ARRAY_ROLES = ("w", "bias", "dw", "db", "db2")           # contiguous arrays: pointer only
FILL = {"x": NAN, "dz": NAN, "act": NAN, "w": NAN, "bias": NAN, "y": SENTINEL, "dx": SENTINEL, "dw": SENTINEL, "db": SENTINEL, "db2": SENTINEL}


# ---- placements -----------------------------------------------------------------------------------------------------------------------

def base_alignment(buf):
    """what the allocator promises for the first byte of a buffer: torch's device allocations start at multiples of 256 bytes (asserted
    wherever a view is made, not assumed), its host allocations at multiples of 64"""
    return 256 if buf.is_cuda else 64


def ld_for(C, ld_res):
    """the pixel stride of a view of C channels: ("=", n) is n itself (the packed image views), an int is the residue modulo 8 - the
    smallest stride with that residue that leaves at least one fill element between two pixels"""
    if isinstance(ld_res, tuple):
        assert ld_res[0] == "=" and ld_res[1] >= C, (C, ld_res)
        return ld_res[1]
    ld = C + 1
    while ld % 8 != ld_res:
        ld += 1
    return ld


def flat_view(t, ld, ptr_res, fill=NAN):
    """a [B, H, W, C] tensor as a view with pixel stride `ld` whose first element lies `ptr_res` bytes behind a multiple of 16, inside a
    flat buffer filled with `fill` (exact_cases.wide_view with a chosen start): at least one row of pixels plus E.GUARD elements of fill
    in front of and behind the view, and between the pixels whenever ld > C.  Returns the buffer, the strided torch view that holds t,
    and the device pointer to channel 0 of pixel 0."""
    C, es = t.shape[-1], t.element_size()
    npix = t.numel() // C
    assert ld >= C and 0 <= ptr_res < 16 and ptr_res % es == 0, (ld, C, ptr_res, es)
    guard = (t.shape[-2] + 1) * ld + E.GUARD
    start = guard
    while start * es % 16 != ptr_res:
        start += 1
    buf = torch.full((start + (npix - 1) * ld + C + guard,), fill, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % base_alignment(buf) == 0, "the allocator's alignment is what the residues are counted from"
    view = buf.as_strided(tuple(t.shape), _strides(t.shape, ld), start)
    view.copy_(t)
    return buf, view, buf.data_ptr() + start * es


def _strides(shape, ld):
    strides, s = [], ld
    for n in reversed(shape[:-1]):
        strides.insert(0, s)
        s *= n
    return (*strides, 1)


class FlatOut:
    """an output view made by flat_view inside a sentinel-filled buffer; check() compares it bit by bit and proves that nothing around
    it changed (as often as it is called: the buffer is left as it is)"""

    def __init__(self, init, ld, ptr_res):
        self.buf, self.view, self.ptr = flat_view(init, ld, ptr_res, SENTINEL)
        self.geom = (tuple(init.shape), _strides(init.shape, ld), (self.ptr - self.buf.data_ptr()) // init.element_size())
        self.before = self._masked(self.buf)

    def _masked(self, buf):
        """a copy of the buffer as integers with the view zeroed"""
        a = buf.detach().clone()
        a.as_strided(*self.geom).zero_()
        return a.view(E._INT_VIEW[a.dtype])

    def got(self):
        return self.view.contiguous()

    def check(self, want, what, names=("b", "h", "w", "c")):
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        E.assert_elementwise_equal(self.got(), want, names, what)
        after = self._masked(self.buf)
        if not torch.equal(after, self.before):
            idx = (after != self.before).nonzero()
            raise AssertionError(f"{what}: {idx.shape[0]} elements outside the view changed, first at element {int(idx[0])} of {after.numel()}")


class Aligned(Place):
    """every operand of a case at a stated alignment.  spec: role -> (pointer residue modulo 16 bytes, ld residue modulo 8 elements, or
    ("=", ld)) for the pixel views, role -> pointer residue for the arrays; roles it does not name are 16-byte aligned with an ld that is
    a multiple of 8.  `seen` keeps (pointer, ld) of everything placed, for `predict`."""

    def __init__(self, spec=None):
        self.spec = dict(spec or {})
        assert set(self.spec) <= set(VIEW_ROLES + ARRAY_ROLES), self.spec
        self.seen = {}

    def of(self, role):
        return self.spec.get(role, (0, 0) if role in VIEW_ROLES else 0)

    def inp(self, role, t, mode, kind):
        ptr_res, ld_res = self.of(role)
        ld = ld_for(t.shape[-1], ld_res)
        buf, view, ptr = flat_view(t, ld, ptr_res, FILL[role])
        self.seen[role] = (ptr, ld)
        return buf, ptr, ld

    def out(self, role, init, mode):
        ptr_res, ld_res = self.of(role)
        ld = ld_for(init.shape[-1], ld_res)
        o = FlatOut(init, ld, ptr_res)
        self.seen[role] = (o.ptr, ld)
        return o, ld

    def param(self, role, t):
        res = self.of(role)
        assert res % t.element_size() == 0
        buf, ptr = E.guarded(t, FILL[role], res // t.element_size())
        assert buf.data_ptr() % base_alignment(buf) == 0 and ptr % 16 == res
        self.seen[role] = (ptr, 0)
        return buf, ptr

    def grad(self, role, init):
        res = self.of(role)
        assert res % init.element_size() == 0
        o = Out(init, 0, 0, guard=True, goff=res // init.element_size())
        assert o.buf.data_ptr() % base_alignment(o.buf) == 0 and o.ptr % 16 == res
        self.seen[role] = (o.ptr, 0)
        return o


# ---- the shapes of the operands of an entry ---------------------------------------------------------------------------------------

def role_shapes(entry, shape):
    """role -> tensor shape of every operand of one call (exact_cases.make_case's shapes)"""
    KS = shape[5] if len(shape) == 6 else 4
    B, H, W, Cin, Cout = shape[:5]
    if entry in ("conv_fwd", "convT_fwd", "s1_fwd"):
        out = {"conv_fwd": (B, H // 2, W // 2, Cout), "convT_fwd": (B, 2 * H, 2 * W, Cout), "s1_fwd": (B, H, W, Cout)}[entry]
        wshape = (4, 4, Cout, Cin) if entry == "convT_fwd" else (KS, KS, Cin, Cout)
        return {"x": (B, H, W, Cin), "w": wshape, "bias": (Cout,), "y": out}
    if entry in ("conv_dgrad", "convT_dgrad", "s1_dgrad"):
        dz = {"conv_dgrad": (B, H // 2, W // 2, Cout), "convT_dgrad": (B, 2 * H, 2 * W, Cout), "s1_dgrad": (B, H, W, Cout)}[entry]
        wshape = (4, 4, Cout, Cin) if entry == "convT_dgrad" else (KS, KS, Cin, Cout)
        return {"dz": dz, "w": wshape, "act": (B, H, W, Cin), "dx": (B, H, W, Cin), "db": (40,), "db2": (max(Cin - 40, 1),)}
    h, w_ = E.wgrad_hw(entry, shape)
    dz = {"conv_wgrad": (B, h // 2, w_ // 2, Cout), "convT_wgrad": (B, 2 * h, 2 * w_, Cout), "s1_wgrad": (B, h, w_, Cout)}[entry]
    wshape = (4, 4, Cout, Cin) if entry == "convT_wgrad" else (KS, KS, Cin, Cout)
    return {"x": (B, h, w_, Cin), "dz": dz, "dw": wshape, "db": (Cout,)}


def role_dtype(role, mode):
    return torch.float32 if role in ("bias", "dw", "db", "db2") else E.TDT[MODE_DT[mode]]


# ---- the host-side predicates, restated ---------------------------------------------------------------------------------------------

Tap = namedtuple("Tap", "x ldx w bias act ldact y ldy K N Hs Ws form")
Wg = namedtuple("Wg", "big ldbig small ldsmall dw Cb Cs")


def tap_params(entry, shape, seen, masked=True):
    """the TapGemmParams capi.hip fills for a forward or input-gradient entry, from the (pointer, ld) of every role"""
    B, H, W, Cin, Cout = shape[:5]
    form = "s1" if entry == "s1_fwd" else "s1t" if entry == "s1_dgrad" else FORM[entry]
    if entry.endswith("_fwd"):
        Hs, Ws = (H // 2, W // 2) if entry == "conv_fwd" else (H, W)
        return Tap(*seen["x"], seen["w"][0], seen["bias"][0], 0, 0, *seen["y"], Cin, Cout, Hs, Ws, form)
    Hs, Ws = (H // 2, W // 2) if entry == "conv_dgrad" else (H, W)
    act = seen["act"] if masked else (0, 0)
    return Tap(*seen["dz"], seen["w"][0], 0, *act, *seen["dx"], Cout, Cin, Hs, Ws, form)


def wgrad_params(entry, shape, seen):
    """WgradParams: the tensor on the BIG grid first (the transposed layer's is dz)"""
    Cin, Cout = shape[3], shape[4]
    if entry == "convT_wgrad":
        return Wg(*seen["dz"], *seen["x"], seen["dw"][0], Cout, Cin)
    return Wg(*seen["x"], *seen["dz"], seen["dw"][0], Cin, Cout)


def tapgemm_mfma_alignment_ok(p):
    """tapgemm_mfma_supported's alignment lines (tapgemm_mfma.hip)"""
    if p.K % 8 or p.N % 8 or p.ldx % 8 or p.ldy % 4:
        return False
    if p.act and p.ldact % 4:
        return False
    if p.x % 16 or p.w % 16 or p.y % 8:
        return False
    if p.act and p.act % 8:
        return False
    return not (p.bias and p.bias % 16)


def tap_wide(p):
    """p.wide of tapgemm_mfma.hip: launch() - the 16-byte epilogue"""
    return p.y % 16 == 0 and p.ldy % 8 == 0 and (not p.act or (p.act % 16 == 0 and p.ldact % 8 == 0))


def halo_takes(p, forced):
    """halo_convT_wanted with the halo kernel forced (tuning 2 << 24): FORM_CONVT, 16 x 16 patches and 16-byte output and mask views"""
    return forced and p.form == "convT" and p.Hs % 16 == 0 and p.Ws % 16 == 0 and tap_wide(p)


def wgrad_mfma_alignment_ok(p):
    """wgrad_mfma_supported's alignment lines (wgrad_mfma.hip)"""
    if p.Cb % 8 or p.Cs % 8 or p.ldbig % 8 or p.ldsmall % 8:
        return False
    return not (p.big % 16 or p.small % 16 or p.dw % 16)


def slabs_possible(p):
    """the slab condition of wgrad_mfma / rgb_wgrad / f32_wgrad: ordered slabs need a 16-byte aligned dw (and a workspace)"""
    return p.dw % 16 == 0


def rgb_fwd_ok(p):
    """rgb_fwd_supported (rgb_mfma.hip); x is element-aligned by construction"""
    if p.K > 4 or p.N % 8 or p.ldy % 4:
        return False
    if p.w % 16 or p.y % 8:
        return False
    return not (p.bias and p.bias % 16)


def rgb_wgrad_ok(p):
    """rgb_wgrad_supported"""
    return p.Cb <= 4 and p.Cs % 8 == 0 and p.ldsmall % 8 == 0 and p.small % 16 == 0


def vec8(x, ldx):
    """gather_chunk's VEC8: one 8-byte load per pixel instead of one load per channel"""
    return ldx >= 4 and ldx % 4 == 0 and x % 8 == 0


def rgb_store(p):
    """the image layer's store: 16-byte stores staged through LDS for whole 128-channel tiles ("staged"), 16-byte stores straight from
    the lanes for a ragged last tile ("wide"), else the 8-byte store ("plain")"""
    if not (p.y % 16 == 0 and p.ldy % 8 == 0):
        return "plain"
    kinds = (["staged"] if p.N >= 128 else []) + (["wide"] if p.N % 128 else [])
    return "+".join(kinds)


def f32_tap_flags(p):
    """(F_AVEC, F_BVEC) of f32_tapgemm"""
    flip = p.form in ("convT", "s1t")
    avec = p.K % 4 == 0 and p.ldx % 4 == 0 and p.x % 16 == 0
    bvec = p.w % 16 == 0 and (p.K % 4 == 0 if flip else p.N % 4 == 0)
    return int(avec), int(bvec)


def f32_wgrad_flags(p):
    """(F_AVEC, F_BVEC) of f32_wgrad"""
    avec = p.Cb % 4 == 0 and p.ldbig % 4 == 0 and p.big % 16 == 0
    bvec = p.Cs % 4 == 0 and p.ldsmall % 4 == 0 and p.small % 16 == 0
    return int(avec), int(bvec)


def predict(entry, shape, mode, seen, tuning=0, workspace=False, masked=True, split=False):
    """(launch-log family, branch) of one call from the pointers it is given.  family None: the stride-1 fall-back, which logs nothing.
    split: the launch is known to split K (E.SPLITK_SHAPE with a workspace; the split heuristic is not restated here, the GPU test
    reads ksplit from the log)."""
    sixteen = mode in ("bf16", "f16")
    s1 = entry.startswith("s1_")
    if entry.endswith("_wgrad"):
        p = wgrad_params(entry, shape, seen)
        mem = "slabs-allowed" if slabs_possible(p) and workspace else "no-slabs"
        if mode.startswith("f32m"):
            return ("f32mfma:wgrad_s1:" if s1 else "f32mfma:wgrad:"), "avec%d:bvec%d:%s" % (*f32_wgrad_flags(p), mem)
        if not sixteen:
            return (None if s1 else "direct:wgrad"), "direct"
        if entry == "conv_wgrad" and rgb_wgrad_ok(p):
            return "rgb:wgrad", ("vec8" if vec8(p.big, p.ldbig) else "scalar") + ":" + mem
        if wgrad_mfma_alignment_ok(p):
            return ("wgrad:s1:" if s1 else "wgrad:"), mem
        return (None if s1 else "direct:wgrad"), "direct"
    p = tap_params(entry, shape, seen, masked)
    if mode.startswith("f32m"):
        return f"f32mfma:{p.form}:", "avec%d:bvec%d" % f32_tap_flags(p)
    if not sixteen:
        return (None if s1 else "direct:tap"), "direct"
    if entry == "conv_fwd" and rgb_fwd_ok(p):
        return "rgb:fwd", ("vec8" if vec8(p.x, p.ldx) else "scalar") + ":" + rgb_store(p)
    if not tapgemm_mfma_alignment_ok(p):
        return (None if s1 else "direct:tap"), "direct"
    if halo_takes(p, (tuning >> 24) & 3 == 2):
        return "halo:convT:", "halo"
    family = f"tap:{'s1' if s1 else p.form}:"
    if split:
        return family, "finalize8" if not tap_wide(p) else "finalize"
    return family, "e16" if tap_wide(p) else "e8"


# ---- the case table -------------------------------------------------------------------------------------------------------------------

# group: the part of the test file that runs the case; opts: what that part needs besides (variants, scratch mode, log tokens)
Case = namedtuple("Case", "group entry shape mode placement tuning workspace family branch opts")

BASE = (1, 4, 12, 72, 136)
S1_SHAPE = (1, 9, 11, 24, 40, 5)
WG_SHAPE = (1, 12, 20, 72, 136)
IMAGE_SHAPES = [(2, 16, 16, 3, 8), (1, 8, 8, 4, 136)] + E.IMAGE_EXTRA_SHAPES
IMAGE_WGRAD_SHAPES = [(2, 16, 16, 3, 8)] + E.IMAGE_EXTRA_SHAPES
SIXTEEN = ("bf16", "f16")
MASKED, UNMASKED = ((1, 0), (1, 1)), ((0, 0), (0, 1))
NO_SPLITK = 1 << 8                                       # gct2_ctx_set_tuning: forward / input-gradient GEMMs never split K


def out_role(entry):
    return "y" if entry.endswith("_fwd") else "dx"


def in_role(entry):
    return "x" if entry.endswith("_fwd") else "dz"


def narrow_ways(entry):
    """the three independent ways into the 8-byte epilogue: the output 8 bytes off, an output stride of 8 k + 4 elements (pixels
    alternate between 16- and 8-byte addresses), and - masked input gradients - an aligned dx with a narrow act"""
    r = out_role(entry)
    ways = [("ptr8", {r: (8, 0)}), ("ld4", {r: (0, 4)})]
    if r == "dx":
        ways.append(("act8", {"act": (8, 0)}))
    return ways


def _name(spec):
    def one(role, v):
        if isinstance(v, tuple):
            ld = f"ld{v[1][1]}" if isinstance(v[1], tuple) else f"ld%8={v[1]}"
            return f"{role}@{v[0]}.{ld}"
        return f"{role}@{v}"
    return "aligned" if not spec else ",".join(one(r, v) for r, v in sorted(spec.items()))


def _cases():
    out = []

    def add(group, entry, shape, modes, spec, family, branch, tuning=0, workspace=False, **opts):
        for mode in modes:
            out.append(Case(group, entry, shape, mode, dict(spec), tuning, workspace, family, branch, dict(opts)))

    def tapfam(entry):
        return f"tap:{FORM[entry]}:"

    # a. the 8-byte tap epilogue: ragged M / K / N, both forced tiles, the 256 x 64 tile of the convT form
    tile_cases = [(BASE, 0, ()), (E.TILE_SHAPES[0], 2, ("128x128:",)), (E.TILE_SHAPES[0], 5, ("256x128:",))]
    for entry in E.TAP_ENTRIES:
        for shape, tuning, tokens in tile_cases:
            for way, spec in narrow_ways(entry):
                add("a", entry, shape, SIXTEEN, spec, tapfam(entry), "e8", tuning, contains=tokens, way=way)
    for entry, shape in (("convT_fwd", (1, 16, 16, 8, 8)), ("conv_dgrad", (2, 32, 32, 64, 24))):
        for way, spec in narrow_ways(entry):
            add("a", entry, shape, SIXTEEN, spec, tapfam(entry), "e8", contains=("256x64:",), way=way)
    # b. fused bias gradients through the 8-byte epilogue, three reduction modes.  The conv-form case (K = 16 channels, 60 tiles) splits
    #    K once it has a workspace: it runs as it is (the finalize kernel's column sums behind narrow views) and with tuning bit 8
    #    (no split-K), which keeps the partial rows of the GEMM kernel's own 8-byte epilogue
    for entry, shape in E.BIAS_GRAD_CASES:
        for scratch in ("none", "ws", "ws+queue"):
            for way, spec in narrow_ways(entry):
                ws = scratch != "none"
                if entry == "convT_dgrad" and ws:
                    add("b", entry, shape, SIXTEEN, spec, tapfam(entry), "finalize8", workspace=ws, scratch=scratch, way=way, split=True)
                add("b", entry, shape, SIXTEEN, spec, tapfam(entry), "e8", NO_SPLITK if entry == "convT_dgrad" and ws else 0, ws, scratch=scratch, way=way)
    # c. split-K with a narrow output: slabs, then the finalize kernel's 8-byte form
    for entry in E.TAP_ENTRIES:
        specs = [{"y": (8, 0)}, {"y": (0, 4)}] if out_role(entry) == "y" else [{"dx": (8, 0), "act": (0, 4)}, {"dx": (0, 4), "act": (8, 0)}]
        for spec in specs:
            add("c", entry, E.SPLITK_SHAPE, SIXTEEN, spec, tapfam(entry), "finalize8", workspace=True, split=True)
    # d. a registered ReLU bit plane on a narrow forward: derived, never written by the epilogue
    for entry in ("conv_fwd", "convT_fwd"):
        for way, spec in narrow_ways(entry):
            add("d", entry, BASE, SIXTEEN, spec, tapfam(entry), "e8", way=way)
    # e. the halo kernel forced, a narrow view: the tap kernel's convT form runs
    for entry, shape in E.HALO_CASES:
        for way, spec in narrow_ways(entry):
            if entry == "conv_dgrad" and way != "act8":
                continue
            add("e", entry, shape, SIXTEEN, spec, "tap:convT:", "e8", 2 << 24, way=way)
    # f. the stride-1 forms
    for entry in ("s1_fwd", "s1_dgrad"):
        for way, spec in narrow_ways(entry)[:2]:
            add("f", entry, S1_SHAPE, SIXTEEN, spec, "tap:s1:", "e8", way=way)
    # g. refusals: one misaligned operand, alone, lands on the direct kernels
    for entry in E.TAP_ENTRIES:
        i, o = in_role(entry), out_role(entry)
        specs = [{i: (8, 0)}, {i: (0, 4)}, {"w": 8}, {o: (4, 0)}, {o: (2, 0)}, {o: (0, 1)}]
        specs += [{"bias": 4}] if o == "y" else [{"act": (4, 0)}]
        for spec in specs:
            add("g", entry, BASE, SIXTEEN, spec, "direct:tap", "direct")
    for entry, spec in (("s1_fwd", {"x": (8, 0)}), ("s1_dgrad", {"w": 8}), ("s1_wgrad", {"dw": 4})):
        add("g", entry, S1_SHAPE, SIXTEEN, spec, None, "direct")
    for entry in E.WGRAD_ENTRIES:
        for spec in ({"dw": 4}, {"dw": 8}, {"x": (8, 0)}, {"dz": (8, 0)}, {"x": (0, 4)}, {"dz": (0, 4)}):
            add("g", entry, WG_SHAPE, SIXTEEN, spec, "direct:wgrad", "direct", workspace=True)
    # h. the image layer: source views (8-byte pixel loads or one load per channel), output views, and its weight gradient
    for shape in IMAGE_SHAPES:
        Cin, Cout = shape[3], shape[4]
        store = rgb_store(Tap(0, 8, 0, 0, 0, 0, 0, 8, Cin, Cout, 0, 0, "conv"))
        sources = [({"x": (0, ("=", Cin))}, "vec8" if Cin == 4 else "scalar")]
        sources += [({"x": (r, ("=", 4))}, "scalar") for r in (2, 4, 6)]
        sources += [({"x": (8, ("=", 4))}, "vec8"), ({"x": (0, ("=", 5))}, "scalar"), ({"x": (0, ("=", 6))}, "scalar"), ({"x": (0, ("=", 8))}, "vec8")]
        for spec, load in sources:
            add("h", "conv_fwd", shape, SIXTEEN, spec, "rgb:fwd", f"{load}:{store}")
            if shape in IMAGE_WGRAD_SHAPES:
                add("h", "conv_wgrad", shape, SIXTEEN, spec, "rgb:wgrad", f"{load}:slabs-allowed", workspace=True)
        for way, spec in narrow_ways("conv_fwd"):
            add("h", "conv_fwd", shape, SIXTEEN, spec, "rgb:fwd", "vec8:plain", way=way, plane=True)
        if shape in IMAGE_WGRAD_SHAPES:
            add("h", "conv_wgrad", shape, SIXTEEN, {"dw": 4}, "rgb:wgrad", "vec8:no-slabs", workspace=True)
    # i. fp32 on the matrix cores: the four (F_AVEC, F_BVEC) combinations by operand alignment alone
    combos = [(a, b) for a in (1, 0) for b in (1, 0)]
    for entry in E.TAP_ENTRIES:
        modes = ("f32m", "f32m_ws") if entry.endswith("_fwd") else ("f32m_ws",)
        for a, b in combos:
            spec = {**({} if a else {in_role(entry): (4, 0)}), **({} if b else {"w": 4})}
            for mode in modes:
                add("i", entry, BASE, (mode,), spec, f"f32mfma:{FORM[entry]}:", f"avec{a}:bvec{b}", workspace=mode == "f32m_ws")
    add("i", "s1_fwd", S1_SHAPE, ("f32m",), {"x": (4, 0)}, "f32mfma:s1:", "avec0:bvec1")
    add("i", "s1_dgrad", S1_SHAPE, ("f32m",), {"w": 4}, "f32mfma:s1t:", "avec1:bvec0")
    for entry in E.WGRAD_ENTRIES:
        big, small = ("dz", "x") if entry == "convT_wgrad" else ("x", "dz")
        for a, b in combos:
            spec = {**({} if a else {big: (4, 0)}), **({} if b else {small: (4, 0)})}
            for ws in (False, True):
                add("i", entry, WG_SHAPE, ("f32m",), spec, "f32mfma:wgrad:", f"avec{a}:bvec{b}:" + ("slabs-allowed" if ws else "no-slabs"), workspace=ws)
        add("i", entry, E.WGRAD_TUNING_SHAPE, ("f32m",), {"dw": 4}, "f32mfma:wgrad:", "avec1:bvec1:no-slabs", 3 << 28, True, token="rsplit=4:atomics")
    return out


CASES = _cases()


def case_id(c):
    extra = "-".join(str(v) for k, v in sorted(c.opts.items()) if k in ("scratch",))
    return "-".join(x for x in (c.group, c.entry, "x".join(map(str, c.shape)), c.mode, _name(c.placement), f"t{c.tuning}" if c.tuning else "",
                                "ws" if c.workspace else "", extra) if x)


def case_special(c):
    """the operand grids of the case: {-1, 0, 1} for the fused bias gradients (group b), else the full ones"""
    return "pm1" if c.group == "b" else None


# every branch of DESIGN.md's "Alignment classes" table -> the predicate value (family, branch prefix) that reaches it
BRANCHES = {
    "tap epilogue, 8-byte": ("tap:", "e8"), "tap split-K finalize behind a narrow view": ("tap:", "finalize8"),
    "tap refusal -> direct": ("direct:tap", "direct"), "stride-1 refusal -> direct": (None, "direct"),
    "wgrad refusal -> direct": ("direct:wgrad", "direct"),
    "image forward, per-channel loads": ("rgb:fwd", "scalar:"), "image forward, 8-byte pixel loads": ("rgb:fwd", "vec8:"),
    "image forward, plain store": ("rgb:fwd", "vec8:plain"), "image forward, staged store": ("rgb:fwd", "vec8:staged"),
    "image forward, wide store": ("rgb:fwd", "vec8:wide"),
    "image wgrad, per-channel loads": ("rgb:wgrad", "scalar:"), "image wgrad, 8-byte pixel loads": ("rgb:wgrad", "vec8:"),
    "image wgrad, no slabs": ("rgb:wgrad", "vec8:no-slabs"),
    **{f"f32 tap avec{a} bvec{b}": ("f32mfma:conv", f"avec{a}:bvec{b}") for a in (0, 1) for b in (0, 1)},
    **{f"f32 tapT avec{a} bvec{b}": ("f32mfma:convT", f"avec{a}:bvec{b}") for a in (0, 1) for b in (0, 1)},
    **{f"f32 wgrad avec{a} bvec{b}": ("f32mfma:wgrad:", f"avec{a}:bvec{b}") for a in (0, 1) for b in (0, 1)},
    "f32 wgrad, split without slabs": ("f32mfma:wgrad:", "avec1:bvec1:no-slabs"),
    "f32 s1": ("f32mfma:s1:", "avec0"), "f32 s1t": ("f32mfma:s1t:", "avec1:bvec0"),
}
