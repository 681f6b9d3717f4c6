"""gct2_dense2_fwd / gct2_dense2_bwd (the hidden Dense(pixel_size, relu) layer + the Dense head of train.py:195-199 as one kernel per
direction) per element, on the GPU.

Exact-sum inputs (tests/exact_cases.py's practice): x, w1, b1 small integers with |pre-activation| <= 256, so the hidden activation h is
an integer that bf16 and fp16 hold exactly; w2 in {-1, 0, 1}; dy small integers times 2^-3 with |dh| <= 2.  Every partial sum is then
exact in fp32 in any order, and the forward output and the four parameter gradients must equal an integer float64 reference formed on
the CPU EXACTLY; dx must equal the exact value rounded once to the dtype.  (GCT2_F16 rounds the Dense output to fp16, as gct2_dense_fwd
does: the reference applies that one rounding too.)  Every case poisons what must not be read (NaN in the pad channels of x) and guards
what must not be written (sentinels around y, dx, the four gradients and the scratch).

Shapes (Cin, ldx, Chid): (67, 72, 128) the reference head and (67, 72, 32) - the matrix-core kernels in the 16-bit dtypes -, (11, 11, 8)
- the plain kernels.  M = 37 (less than a tile, odd) and 2 T + 37 with T = _lib.DENSE2_FAST_PIXELS: three work-groups and a ragged tail
in the matrix-core kernels, eleven in the plain backward kernel - at least three partial rows to add in order.

Random inputs: the plain kernels (gct2_ctx_force_direct) and the fast ones against a float64 reference that applies round_T to h.  Bound
per element, derived: every h[j] is within one unit in the last place of the dtype of the reference's, so
|y - ref| <= sum_j |w2[j,o]| ulp_T(h_j) + 2^-22 sum_j |h_j w2[j,o]| (fp32 accumulation), and the same form for every gradient with dh in
the place of h; results that are themselves rounded once more (dx to the dtype, y to fp16 under GCT2_F16) may land on the neighbouring
value: plus one ulp of that format at the reference's value.  Precondition (asserted): no pre-activation of the reference within 1e-5 of
zero, so the ReLU mask of kernel and reference cannot differ."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
MANT = {F32: 23, BF16: 7, F16: 10}                  # explicit mantissa bits: ulp_T(v) = 2^(floor(log2 |v|) - MANT)
GUARD, SENT = 64, 12345.0
SHAPES = [(67, 72, 128), (11, 11, 8), (67, 72, 32)]


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def tile():
    return lib().DENSE2_FAST_PIXELS


def m_values():
    return (37, 2 * tile() + 37)


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(n, gpu, dtype=torch.float32, fill=0.0):
    big = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=gpu)
    inner = big[GUARD:GUARD + n]
    inner.fill_(fill)
    return big, inner


def guards_intact(big, n):
    return bool((big[:GUARD] == SENT).all()) and bool((big[GUARD + n:] == SENT).all())


def round_t(a, dt):
    """float64 array rounded once to the dtype (round to nearest even), back in float64"""
    if dt == F32:
        return a.astype(np.float32).astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(TD[dt]).to(torch.float64).numpy()


def ulp(a, dt):
    a = np.abs(a)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return np.where(a > 0, 2.0 ** (e - MANT[dt]), 0.0)


def sent(dt):
    """the sentinel as the dtype holds it"""
    return float(round_t(np.array([SENT]), dt)[0])


def expected_path(dt, cin, ldx, chid):
    return "mfma" if (dt != F32 and chid in (32, 64, 128) and cin <= 80 and ldx % 8 == 0) else "plain"


class Case:
    """inputs on the CPU in float64 (already representable in the dtype) and on the device.  xoff: x starts that many elements behind
    the start of its allocation (NaN in front of it)"""

    def __init__(self, gpu, dt, M, cin, ldx, chid, cout, seed, exact, xoff=0):
        rng = np.random.default_rng(seed)
        self.dt, self.M, self.cin, self.ldx, self.chid, self.cout, self.gpu = dt, M, cin, ldx, chid, cout, gpu
        if exact:
            x = rng.integers(-2, 4, (M, cin)).astype(np.float64)
            w1 = rng.integers(-1, 2, (cin, chid)).astype(np.float64)
            b1 = rng.integers(-8, 9, (chid,)).astype(np.float64)
            w2 = rng.integers(-1, 2, (chid, cout)).astype(np.float64)
            b2 = rng.integers(-4, 5, (cout,)).astype(np.float64)
            dy = rng.integers(-4, 5, (M, cout)).astype(np.float64) * 2.0 ** -3
        else:
            x = round_t(rng.standard_normal((M, cin)), dt)
            w1 = round_t(rng.standard_normal((cin, chid)) / np.sqrt(cin), dt)
            b1 = round_t(rng.standard_normal(chid) * 0.1, F32)
            w2 = round_t(rng.standard_normal((chid, cout)) / np.sqrt(chid), F32)
            b2 = round_t(rng.standard_normal(cout) * 0.1, F32)
            dy = round_t(rng.standard_normal((M, cout)), F16 if dt == F16 else F32)
        self.x, self.w1, self.b1, self.w2, self.b2, self.dy = x, w1, b1, w2, b2, dy
        xp = np.full((M, ldx), np.nan)                          # pad channels: never multiplied
        xp[:, :cin] = x
        dev = lambda a, t=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(t).to(gpu).contiguous()
        self.d_x, self.d_w1 = dev(xp, TD[dt]), dev(w1, TD[dt])
        if xoff:
            self.x_alloc = torch.full((M * ldx + xoff,), float("nan"), dtype=TD[dt], device=gpu)
            self.x_alloc[xoff:] = self.d_x.reshape(-1)
            self.d_x = self.x_alloc[xoff:].view(M, ldx)
        self.d_b1, self.d_w2, self.d_b2, self.d_dy = dev(b1), dev(w2), dev(b2), dev(dy)
        # float64 reference with the dtype's rounding points
        self.pre = x @ w1 + b1
        self.h = round_t(np.maximum(self.pre, 0.0), dt)
        self.y_raw = self.h @ w2 + b2
        self.y = round_t(self.y_raw, F16) if dt == F16 else self.y_raw
        self.dh_raw = (self.h > 0) * (dy @ w2.T)
        self.dh = round_t(self.dh_raw, dt)
        self.dw2, self.db2 = self.h.T @ dy, dy.sum(0)
        self.dw1, self.db1 = x.T @ self.dh, self.dh.sum(0)
        self.dx_raw = (x > 0) * (self.dh @ w1.T)
        self.dx = round_t(self.dx_raw, dt)

    def scratch_floats(self):
        need = ctypes.c_size_t(0)
        lib().check(lib().load().gct2_dense2_scratch(self.M, self.cin, self.chid, self.cout, ctypes.byref(need)), "gct2_dense2_scratch")
        return need.value

    def forward(self, ctx):
        n = self.M * self.cout
        big, y = guarded(n, self.gpu, fill=float("nan"))
        lib().call("gct2_dense2_fwd", ctx.handle, self.dt, self.d_x.data_ptr(), self.ldx, self.d_w1.data_ptr(), self.d_b1.data_ptr(),
                   self.d_w2.data_ptr(), self.d_b2.data_ptr(), y.data_ptr(), self.M, self.cin, self.chid, self.cout, stream())
        torch.cuda.synchronize()
        assert guards_intact(big, n)
        return y.cpu().double().numpy().reshape(self.M, self.cout)

    def backward(self, ctx, cmask, lddx, accumulate=0, prefill=0.0, with_dx=True):
        """(dx [M, lddx] or None, dw1, db1, dw2, db2) as float64 arrays; every output and the scratch between sentinels"""
        g = self.gpu
        nsc = self.scratch_floats()
        outs = [guarded(n, g, fill=prefill) for n in (self.cin * self.chid, self.chid, self.chid * self.cout, self.cout)]
        bsc, sc = guarded(nsc, g, fill=float("nan"))
        bdx, dx = guarded(self.M * lddx, g, dtype=TD[self.dt], fill=SENT)
        assert sc.data_ptr() % 16 == 0
        lib().call("gct2_dense2_bwd", ctx.handle, self.dt, self.d_x.data_ptr(), self.ldx, self.d_w1.data_ptr(), self.d_b1.data_ptr(),
                   self.d_w2.data_ptr(), self.d_dy.data_ptr(), dx.data_ptr() if with_dx else None, lddx, outs[0][1].data_ptr(),
                   outs[1][1].data_ptr(), outs[2][1].data_ptr(), outs[3][1].data_ptr(), sc.data_ptr(), nsc, self.M, self.cin, self.chid,
                   self.cout, cmask, accumulate, stream())
        torch.cuda.synchronize()
        for (big, t), n in zip(outs, (self.cin * self.chid, self.chid, self.chid * self.cout, self.cout)):
            assert guards_intact(big, n)
        assert guards_intact(bsc, nsc) and guards_intact(bdx, self.M * lddx)
        f = lambda t, *shape: t.cpu().double().numpy().reshape(*shape)
        return (f(dx, self.M, lddx), f(outs[0][1], self.cin, self.chid), f(outs[1][1], self.chid), f(outs[2][1], self.chid, self.cout),
                f(outs[3][1], self.cout))


def new_ctx(direct=False):
    c = lib().Context()
    if direct:
        c.force_direct(True)
    c.log_launches(True)
    return c


EXACT = [pytest.param(dt, M_i, cin, ldx, chid, id=f"{NAMES[dt]}-cin{cin}-chid{chid}-m{M_i}")
         for dt in (F32, BF16, F16) for cin, ldx, chid in SHAPES for M_i in (0, 1)]


def check_exact(c, ctx, cmask):
    lddx = cmask + 8 if cmask else 8
    y = c.forward(ctx)
    assert np.array_equal(y, c.y), float(np.abs(y - c.y).max())
    dx, dw1, db1, dw2, db2 = c.backward(ctx, cmask, lddx)
    assert np.array_equal(dw1, c.dw1) and np.array_equal(db1, c.db1), (float(np.abs(dw1 - c.dw1).max()), float(np.abs(db1 - c.db1).max()))
    assert np.array_equal(dw2, c.dw2) and np.array_equal(db2, c.db2), (float(np.abs(dw2 - c.dw2).max()), float(np.abs(db2 - c.db2).max()))
    assert np.array_equal(dx[:, :cmask], c.dx[:, :cmask]), float(np.abs(dx[:, :cmask] - c.dx[:, :cmask]).max())
    assert bool((dx[:, cmask:] == sent(c.dt)).all())             # channels >= Cmask: untouched
    return dx


@pytest.mark.parametrize("dt, M_i, cin, ldx, chid", EXACT)
def test_exact_sums_forward_and_all_gradients(gpu, dt, M_i, cin, ldx, chid):
    M = m_values()[M_i]
    c = Case(gpu, dt, M, cin, ldx, chid, 3, seed=100 * chid + cin + M, exact=True)
    assert np.abs(c.pre).max() <= 256 and np.abs(c.dh_raw).max() <= 256
    neg = float((c.pre < 0).mean())
    assert 0.3 < neg < 0.7 and bool((c.pre == 0).any()), neg     # the h > 0 mask is exercised, pre-activations of exactly 0 included
    ctx = new_ctx()
    check_exact(c, ctx, cin - 3)
    want = expected_path(dt, cin, ldx, chid)
    assert ctx.read_launch_log() == [f"dense2:fwd:{want}", f"dense2:bwd:{want}"]


@pytest.mark.parametrize("dt", (BF16, F16))
def test_x_off_its_16_byte_alignment_takes_the_plain_kernels_exact(gpu, dt):
    """the other side of fast_ok's alignment line (dense2.hip): a shape the matrix-core kernels take, with x 8 bytes behind a 16-byte
    boundary, runs the plain kernels - the same exact results"""
    cin, ldx, chid = SHAPES[0]
    assert expected_path(dt, cin, ldx, chid) == "mfma"
    c = Case(gpu, dt, m_values()[0], cin, ldx, chid, 3, seed=100 * chid + cin, exact=True, xoff=4)
    assert c.x_alloc.data_ptr() % 256 == 0 and c.d_x.data_ptr() % 16 == 8
    ctx = new_ctx()
    check_exact(c, ctx, cin - 3)
    assert ctx.read_launch_log() == ["dense2:fwd:plain", "dense2:bwd:plain"]


@pytest.mark.parametrize("dt", (F32, BF16, F16))
@pytest.mark.parametrize("cout", (1, 4))
def test_exact_sums_other_output_counts(gpu, dt, cout):
    c = Case(gpu, dt, m_values()[1], 67, 72, 128, cout, seed=7 + cout, exact=True)
    check_exact(c, new_ctx(), 64)


@pytest.mark.parametrize("dt", (F32, BF16, F16))
@pytest.mark.parametrize("cin, ldx, chid", SHAPES[:2])
def test_accumulate_cmask_and_null_dx(gpu, dt, cin, ldx, chid):
    c = Case(gpu, dt, m_values()[1], cin, ldx, chid, 3, seed=31 + chid, exact=True)
    ctx = new_ctx()
    cmask = 64 if cin == 67 else 8
    # accumulate = 1 adds to pre-filled gradients exactly; Cmask leaves the channels behind it at their sentinel (lddx = Cmask + 8)
    dx, dw1, db1, dw2, db2 = c.backward(ctx, cmask, cmask + 8, accumulate=1, prefill=3.0)
    assert np.array_equal(dw1, c.dw1 + 3) and np.array_equal(db1, c.db1 + 3) and np.array_equal(dw2, c.dw2 + 3) and np.array_equal(db2, c.db2 + 3)
    assert np.array_equal(dx[:, :cmask], c.dx[:, :cmask]) and bool((dx[:, cmask:] == sent(dt)).all())
    # dx = NULL, and Cmask = 0 with a dx buffer: nothing is written there, the parameter gradients are the same
    for with_dx, cm in ((False, cmask), (True, 0)):
        dx0, dw1, db1, dw2, db2 = c.backward(ctx, cm, cmask + 8, with_dx=with_dx)
        assert bool((dx0 == sent(dt)).all())
        assert np.array_equal(dw1, c.dw1) and np.array_equal(db1, c.db1) and np.array_equal(dw2, c.dw2) and np.array_equal(db2, c.db2)


RANDOM = [pytest.param(dt, cin, ldx, chid, id=f"{NAMES[dt]}-cin{cin}-chid{chid}") for dt in (F32, BF16, F16) for cin, ldx, chid in SHAPES]


@pytest.mark.parametrize("dt, cin, ldx, chid", RANDOM)
def test_random_inputs_plain_and_fast_within_the_derived_bound(gpu, dt, cin, ldx, chid, parity_log):
    M, cout, cmask = m_values()[1], 3, (64 if cin == 67 else 8)
    # the precondition of the bound: no ambiguous ReLU mask (fp32 accumulation moves a pre-activation by ~1e-6 at these magnitudes) - the
    # first seed whose reference pre-activations all keep 1e-5 away from zero
    for seed in range(900 + chid + dt, 1000 + chid + dt):
        c = Case(gpu, dt, M, cin, ldx, chid, cout, seed=seed, exact=False)
        if np.abs(c.pre).min() > 1e-5:
            break
    assert np.abs(c.pre).min() > 1e-5
    A = np.abs
    E = 2.0 ** -22
    uh, udh = ulp(c.h, dt), ulp(c.dh, dt)
    bounds = dict(
        y=uh @ A(c.w2) + E * (A(c.h) @ A(c.w2)) + (ulp(c.y, F16) if dt == F16 else 0.0),
        dw2=uh.T @ A(c.dy) + E * (A(c.h).T @ A(c.dy)),
        db2=E * A(c.dy).sum(0),
        dw1=A(c.x).T @ udh + E * (A(c.x).T @ A(c.dh)),
        db1=udh.sum(0) + E * A(c.dh).sum(0),
        dx=((udh @ A(c.w1).T) + E * (A(c.dh) @ A(c.w1).T) + ulp(c.dx, dt))[:, :cmask])
    ref = dict(y=c.y, dw2=c.dw2, db2=c.db2, dw1=c.dw1, db1=c.db1, dx=c.dx[:, :cmask])
    measured = {}
    for direct in (True, False):
        ctx = new_ctx(direct)
        y = c.forward(ctx)
        dx, dw1, db1, dw2, db2 = c.backward(ctx, cmask, cmask + 8)
        path = "plain" if direct else expected_path(dt, cin, ldx, chid)
        assert ctx.read_launch_log() == [f"dense2:fwd:{path}", f"dense2:bwd:{path}"]
        got = dict(y=y, dw2=dw2, db2=db2, dw1=dw1, db1=db1, dx=dx[:, :cmask])
        for k in ref:
            assert np.isfinite(got[k]).all(), (k, direct)
            measured[f"{'plain' if direct else 'fast'}/{k}"] = float((A(got[k] - ref[k]) / np.maximum(bounds[k], 1e-300)).max())
    parity_log(f"dense2_random_{NAMES[dt]}_cin{cin}_chid{chid}", **measured)
    print(measured)
    assert max(measured.values()) <= 1.0, measured
