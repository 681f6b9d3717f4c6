"""gct2_noise_image_table / gct2_noise_image_rng_table (the noising of train.py:229-234 with the pair (sa, sb) read from a host-built
table instead of a formula, include/gct2.h) through the C ABI, in all three dtypes, bit for bit.

Every table lies in the middle of a larger NaN-filled allocation: a missing clamp or a wrong index shows as NaN in the output, never
as a fault.  Every output is a view inside a sentinel-filled buffer that must be unchanged around the view after the call."""
import numpy as np
import pytest
import torch

import exact_cases as E
import pointwise_cases as P
from exact_cases import BF16, F16, F32, SENTINEL
from noise_schedule_cases import TABLE4, mix_ref

pytestmark = pytest.mark.gpu

DTS = [F32, BF16, F16]
DT_IDS = ["f32", "bf16", "f16"]
EINVAL = 1
INT32_MAX = 2 ** 31 - 1
SEED, SID = 0x123456789ABCDEF, 2


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, gpu):
    return torch.tensor(np.ascontiguousarray(a)).to(gpu).contiguous()


class Out:
    """an output view [B, HW, C] at channel 0 of a sentinel-filled [B + 2, HW, ld] buffer (two guard images, pad columns up to ld),
    or a flat float32 array with guard elements around it"""

    def __init__(self, shape, tdt, gpu, ld=None):
        init = torch.full(shape, SENTINEL, dtype=tdt, device=gpu)
        self.shape = tuple(shape)
        if ld is None:
            self.buf, self.ptr = E.guarded(init, SENTINEL)
            self.inside = (slice(E.GUARD, E.GUARD + init.numel()),)
        else:
            self.buf, self.ptr = E.poisoned_view(init, ld, 0, SENTINEL)
            self.inside = (slice(1, -1), Ellipsis, slice(0, shape[-1]))
        self.before = self.buf.clone()

    def got(self):
        torch.cuda.synchronize()
        return self.buf[self.inside].reshape(self.shape).cpu()

    def check(self, want, what):
        E.assert_elementwise_equal(self.got(), want, ("b", "p", "c")[-len(self.shape):], what)
        E.assert_outside_untouched(self.buf, self.before, self.inside, what)       # pad columns and guard images keep the sentinel


def guarded_table(tab, gpu):
    """the table in the middle of a NaN-filled allocation; (buffer kept alive, device pointer, 8-byte aligned)"""
    buf, ptr = E.guarded(dev(np.asarray(tab, np.float32), gpu))
    assert ptr % 8 == 0 and torch.isnan(buf[:E.GUARD]).all() and torch.isnan(buf[-E.GUARD:]).all()
    return buf, ptr


def small_inputs(B, HW, C=3, seed=41):
    rng = np.random.default_rng([B, HW, seed])
    return P.image_values(rng, (B, HW, C)), rng.standard_normal((B, HW, C)).astype(np.float32)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_arbitrary_table(gpu, dt):
    B, HW, C, steps = 3, 5, 3, 4
    t = np.array([4, 1, 3], np.int32)
    x, eps = small_inputs(B, HW)
    keep, coef = guarded_table(TABLE4, gpu)
    out, out2 = Out((B, HW, C), E.TDT[dt], gpu, ld=4), Out((B, HW, C), E.TDT[dt], gpu, ld=7)
    xd, ed, td = dev(x, gpu), dev(eps, gpu), dev(t, gpu)
    lib().call("gct2_noise_image_table", dt, xd.data_ptr(), td.data_ptr(), ed.data_ptr(), coef, out.ptr, 4, out2.ptr, 7, B, HW, C, steps, stream())
    want = mix_ref(dt, x, eps, TABLE4[t - 1])
    assert not torch.isnan(want.float()).any()
    what = f"noise_image_table {E.DTYPE_NAMES[dt]}, arbitrary table"
    out.check(want, what + ": out (ld 4)")
    out2.check(want, what + ": out2 (ld 7)")


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_timesteps_are_clamped(gpu, dt):
    """t = 0, steps + 1, -5 and INT32_MAX read entries 1, steps, 1 and steps: nothing outside the table (NaN all around it)"""
    B, HW, C, steps = 4, 5, 3, 4
    t = np.array([0, steps + 1, -5, INT32_MAX], np.int32)
    x, eps = small_inputs(B, HW)
    keep, coef = guarded_table(TABLE4, gpu)
    xd, ed, td = dev(x, gpu), dev(eps, gpu), dev(t, gpu)
    want = mix_ref(dt, x, eps, TABLE4[np.array([1, steps, 1, steps]) - 1])
    out = Out((B, HW, C), E.TDT[dt], gpu, ld=4)
    lib().call("gct2_noise_image_table", dt, xd.data_ptr(), td.data_ptr(), ed.data_ptr(), coef, out.ptr, 4, None, 0, B, HW, C, steps, stream())
    out.check(want, f"noise_image_table {E.DTYPE_NAMES[dt]}, clamped t")
    # the rng form clamps the same way: its output is the table form's on its own draws
    draws, out_r = Out((B * HW * C,), torch.float32, gpu), Out((B, HW, C), E.TDT[dt], gpu, ld=4)
    lib().call("gct2_noise_image_rng_table", dt, xd.data_ptr(), td.data_ptr(), SEED, SID, 7, draws.ptr, coef, out_r.ptr, 4, None, 0,
               B, HW, C, steps, stream())
    out_r.check(mix_ref(dt, x, draws.got().numpy().reshape(B, HW, C), TABLE4[np.array([1, steps, 1, steps]) - 1]),
                f"noise_image_rng_table {E.DTYPE_NAMES[dt]}, clamped t")


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_rng_form(gpu, dt):
    """offset 7 and HW * C = 15: Philox counters start inside a counter and straddle both image boundaries (the pair is re-read).
    eps_out = gct2_rng_normal at that position, out = gct2_noise_image_table fed those draws, bit for bit"""
    B, HW, C, steps, off = 3, 5, 3, 4, 7
    t = np.array([4, 1, 3], np.int32)
    x, _ = small_inputs(B, HW)
    keep, coef = guarded_table(TABLE4, gpu)
    xd, td = dev(x, gpu), dev(t, gpu)
    n = B * HW * C
    draws, eps_out = Out((n,), torch.float32, gpu), Out((n,), torch.float32, gpu)
    out, out2 = Out((B, HW, C), E.TDT[dt], gpu, ld=4), Out((B, HW, C), E.TDT[dt], gpu, ld=7)
    lib().call("gct2_rng_normal", SEED, SID, off, draws.ptr, n, stream())
    lib().call("gct2_noise_image_rng_table", dt, xd.data_ptr(), td.data_ptr(), SEED, SID, off, eps_out.ptr, coef, out.ptr, 4, out2.ptr, 7,
               B, HW, C, steps, stream())
    what = f"noise_image_rng_table {E.DTYPE_NAMES[dt]}"
    eps_out.check(draws.got(), what + ": eps_out against gct2_rng_normal")
    ref = Out((B, HW, C), E.TDT[dt], gpu, ld=4)
    lib().call("gct2_noise_image_table", dt, xd.data_ptr(), td.data_ptr(), draws.ptr, coef, ref.ptr, 4, None, 0, B, HW, C, steps, stream())
    want = ref.got()
    E.assert_elementwise_equal(want, mix_ref(dt, x, draws.got().numpy().reshape(B, HW, C), TABLE4[t - 1]), ("b", "p", "c"), what + ": table form")
    out.check(want, what + ": out")
    out2.check(want, what + ": out2")
    # without eps_out: the same values
    again = Out((B, HW, C), E.TDT[dt], gpu, ld=4)
    lib().call("gct2_noise_image_rng_table", dt, xd.data_ptr(), td.data_ptr(), SEED, SID, off, None, coef, again.ptr, 4, None, 0,
               B, HW, C, steps, stream())
    again.check(want, what + ": no eps_out")


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_fast_path(gpu, dt):
    """the train step's call (3 channels into the packed 4-slot image, nothing else, stream position a multiple of 12): equal to the
    generic path (forced by asking for eps_out), and slot 3 of every pixel is written as zero - which proves the fast kernel ran"""
    B, HW, C, steps, off = 3, 8, 3, 4, 24
    t = np.array([4, 1, 3], np.int32)
    x, _ = small_inputs(B, HW)
    keep, coef = guarded_table(TABLE4, gpu)
    xd, td = dev(x, gpu), dev(t, gpu)
    general, fast = (Out((B, HW, 4), E.TDT[dt], gpu, ld=4) for _ in range(2))
    assert xd.data_ptr() % 16 == 0 and fast.ptr % 16 == 0
    eps = Out((B * HW * C,), torch.float32, gpu)
    args = (B, HW, C, steps, stream())
    lib().call("gct2_noise_image_rng_table", dt, xd.data_ptr(), td.data_ptr(), SEED, SID, off, eps.ptr, coef, general.ptr, 4, None, 0, *args)
    lib().call("gct2_noise_image_rng_table", dt, xd.data_ptr(), td.data_ptr(), SEED, SID, off, None, coef, fast.ptr, 4, None, 0, *args)
    g, f = general.got(), fast.got()
    stored_sentinel = float(torch.tensor(SENTINEL).to(E.TDT[dt]))
    assert float((g[..., 3].float() - stored_sentinel).abs().max()) == 0        # the generic kernel leaves the pad slot alone
    assert float(f[..., 3].float().abs().max()) == 0
    E.assert_elementwise_equal(f[..., :3].contiguous(), g[..., :3].contiguous(), ("b", "p", "c"), "table fast path against the generic one")
    E.assert_elementwise_equal(g[..., :3].contiguous(), mix_ref(dt, x, eps.got().numpy().reshape(B, HW, C), TABLE4[t - 1]), ("b", "p", "c"),
                               "generic path against numpy")
    E.assert_outside_untouched(fast.buf, fast.before, fast.inside, "fast path")
    E.assert_outside_untouched(general.buf, general.before, general.inside, "generic path")


def quadratic_table(dt, steps):
    import gan_class_transfer2_amd as g
    if dt == BF16:          # gct2_noise_image's GCT2_BF16 forms t as a product (include/gct2.h): the test builds that table itself
        sa, sb = P.noise_coefs_reciprocal(np.arange(1, steps + 1, dtype=np.int32), steps)
        return np.stack([sa, sb], 1).astype(np.float32)
    return g.trainer_math.noise_table("quadratic", 0.0, steps, dt)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_identity_with_the_shipped_kernels(gpu, dt):
    """one image per timestep 1 .. 200: the table form with the quadratic table gives gct2_noise_image's bits; and, from stream
    position 0, the rng table form (the fast path for the 16-bit types) gives gct2_noise_image_rng's"""
    steps = 200
    case = P.noise_case(steps)
    B, HW, C = case["x"].shape
    assert (B, HW, C) == (200, 4, 3)
    keep, coef = guarded_table(quadratic_table(dt, steps), gpu)
    xd, ed, td = dev(case["x"], gpu), dev(case["eps"], gpu), dev(case["t"], gpu)
    shipped, table = (Out((B, HW, C), E.TDT[dt], gpu, ld=4) for _ in range(2))
    lib().call("gct2_noise_image", dt, xd.data_ptr(), td.data_ptr(), ed.data_ptr(), shipped.ptr, 4, None, 0, B, HW, C, steps, stream())
    lib().call("gct2_noise_image_table", dt, xd.data_ptr(), td.data_ptr(), ed.data_ptr(), coef, table.ptr, 4, None, 0, B, HW, C, steps, stream())
    table.check(shipped.got(), f"noise_image_table {E.DTYPE_NAMES[dt]} against gct2_noise_image (b = t_int - 1)")
    shipped_r, table_r = (Out((B, HW, 4), E.TDT[dt], gpu, ld=4) for _ in range(2))
    lib().call("gct2_noise_image_rng", dt, xd.data_ptr(), td.data_ptr(), SEED, SID, 0, None, shipped_r.ptr, 4, None, 0, B, HW, C, steps, stream())
    lib().call("gct2_noise_image_rng_table", dt, xd.data_ptr(), td.data_ptr(), SEED, SID, 0, None, coef, table_r.ptr, 4, None, 0,
               B, HW, C, steps, stream())
    table_r.check(shipped_r.got(), f"noise_image_rng_table {E.DTYPE_NAMES[dt]} against gct2_noise_image_rng (b = t_int - 1)")


def test_rejections(gpu):
    L = lib()
    raw = L.load()
    B, HW, C, steps = 3, 5, 3, 4
    x, eps = small_inputs(B, HW)
    keep, coef = guarded_table(TABLE4, gpu)
    xd, ed, td = dev(x, gpu), dev(eps, gpu), dev(np.array([4, 1, 3], np.int32), gpu)
    out = Out((B, HW, C), torch.float32, gpu, ld=4)
    plain = lambda coef, steps: raw.gct2_noise_image_table(F32, xd.data_ptr(), td.data_ptr(), ed.data_ptr(), coef, out.ptr, 4, None, 0,
                                                           B, HW, C, steps, stream())
    rng = lambda coef, steps: raw.gct2_noise_image_rng_table(F32, xd.data_ptr(), td.data_ptr(), SEED, SID, 0, None, coef, out.ptr, 4, None, 0,
                                                             B, HW, C, steps, stream())
    for fn in (plain, rng):
        assert fn(None, steps) == EINVAL                              # NULL coef
        assert fn(coef + 4, steps) == EINVAL                          # coef + 1 (a float further): not 8-byte aligned
        assert fn(coef, 0) == EINVAL and fn(coef, -1) == EINVAL       # steps < 1
    torch.cuda.synchronize()
    E.assert_outside_untouched(out.buf, out.before, (slice(0, 0),), "a refused call")        # nothing was launched: all sentinel
    with pytest.raises(L.Gct2Error):
        L.call("gct2_noise_image_table", F32, xd.data_ptr(), td.data_ptr(), ed.data_ptr(), None, out.ptr, 4, None, 0, B, HW, C, steps, stream())
    assert plain(coef, steps) == 0 and rng(coef, steps) == 0
    torch.cuda.synchronize()
