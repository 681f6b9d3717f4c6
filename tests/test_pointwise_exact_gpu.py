"""The kernels that make the train step's inputs and the sampler's pointwise steps, ELEMENT BY ELEMENT against host references
(tests/pointwise_cases.py, oracle/denoiser_oracle.noise_image_f32): the Philox streams as include/gct2.h defines them, the noising,
the per-image mix, the sampler's mix / update, the ReLU mask and the add.

Integers and float32 op chains are compared bit for bit (+0 == -0, NaN == NaN: exact_cases.assert_elementwise_equal); the normals,
whose log2 / sin / cos run on the hardware's transcendental units, within NORMAL_ABS_BOUND of a float64 Box-Muller of the same
uniforms.  Every output is a view inside a sentinel-filled buffer (guard elements or guard images in front and behind, pad columns
up to ld) that must be unchanged around the view after each call.
"""
import numpy as np
import pytest
import torch

import exact_cases as E
import pointwise_cases as P
from exact_cases import BF16, F16, F32, SENTINEL
from oracle import denoiser_oracle as O

pytestmark = pytest.mark.gpu

DTS = [F32, BF16, F16]
DT_IDS = ["f32", "bf16", "f16"]
INT_SENTINEL = -1234

# |z_gpu - z_ref| of gct2_rng_normal / gct2_noise_image_rng's draws against pointwise_cases.normal_ref (float64).
# Measured on an MI355X over every case of this file (profiles/rng_parity.json): E = 5.266e-07, at z = -4.03 in the long draw.
# The bound is 4 E = 2.1e-6 rounded up to a power of two: the error depends on which uniforms a case happens to draw, while a
# wrong lane, pair, counter word or key word gives independent normals, differences of order 1.
NORMAL_MEASURED_E = 5.266e-07
NORMAL_ABS_BOUND = 2.0 ** -18
assert NORMAL_ABS_BOUND / 2 < 4 * NORMAL_MEASURED_E <= NORMAL_ABS_BOUND

# case -> max |z_gpu - z_ref|.  Every test that measures re-records the maximum so far through parity_log with the number of cases
# behind it: the record is the file's E once `cases` has reached NORMAL_CASES (a run of a part of the file leaves complete = 0)
_normal_err = {}
NORMAL_CASES = len(P.SEEDS) * (len(P.OFFSETS) + 1) + 1 + 3          # per seed: every offset, two lengths at the carry; the long draw; noise_rng per dtype


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """an output view inside a sentinel-filled buffer: flat with GUARD elements around it, or [B, ..., C] at channel offset `off` of
    a [B + 2, ..., ld] buffer (two guard images).  check() compares bit by bit and proves that nothing around the view changed."""

    def __init__(self, shape, tdt, gpu, ld=None, off=0, fill=SENTINEL):
        init = torch.full(shape, fill, dtype=tdt, device=gpu)
        self.shape = tuple(shape)
        if ld is None:
            self.buf, self.ptr = E.guarded(init, fill)
            self.inside = (slice(E.GUARD, E.GUARD + init.numel()),)
        else:
            self.buf, self.ptr = E.poisoned_view(init, ld, off, fill)
            self.inside = (slice(1, -1), Ellipsis, slice(off, off + shape[-1]))
        self.before = self.buf.clone()

    def at(self, index):
        """device pointer to flat element `index` of a flat view"""
        return self.ptr + index * self.buf.element_size()

    def set(self, values):
        self.buf[self.inside] = values.reshape(self.buf[self.inside].shape)
        self.before = self.buf.clone()

    def got(self):
        torch.cuda.synchronize()
        return self.buf[self.inside].reshape(self.shape).cpu()

    def untouched_outside(self, what):
        torch.cuda.synchronize()
        E.assert_outside_untouched(self.buf, self.before, self.inside, what)

    def check(self, want, what, names=("b", "p", "c")):
        E.assert_elementwise_equal(self.got(), want, names, what)
        self.untouched_outside(what)


def dev(a, gpu, tdt=None):
    t = torch.tensor(np.ascontiguousarray(a))
    return (t if tdt is None else t.to(tdt)).to(gpu).contiguous()


def check_normals(got, seed, sid, off, what, parity_log):
    """got: float32 CPU tensor of the draws at [off, off + n) - finite, within NORMAL_ABS_BOUND of the float64 reference"""
    z = got.numpy().astype(np.float64).reshape(-1)
    ref = P.normal_ref(seed, sid, off, z.size)
    assert np.isfinite(z).all(), what
    err = np.abs(z - ref)
    _normal_err[what] = float(err.max())
    worst = max(_normal_err.values())
    print(f"{what}: max |z_gpu - z_ref| = {err.max():.4g} at element {int(err.argmax())} (z = {ref[int(err.argmax())]:.4g}); file maximum so far {worst:.4g}")
    parity_log("rng_normal_abs_err", E=worst, cases=len(_normal_err), complete=int(len(_normal_err) == NORMAL_CASES),
               asserted_bound=NORMAL_ABS_BOUND)
    bad = np.nonzero(err > NORMAL_ABS_BOUND)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {z.size} normals off by more than {NORMAL_ABS_BOUND:.3g}, first at element {bad[0]}: " \
                          f"got {z[bad[0]]!r} want {ref[bad[0]]!r}"


# ---- gct2_rng_uniform_int ------------------------------------------------------------------------------------------------------------

def draw_ints(gpu, seed, sid, off, n, lo, hi):
    out = Out((n,), torch.int32, gpu, fill=INT_SENTINEL)
    lib().call("gct2_rng_uniform_int", seed, sid, off, out.ptr, n, lo, hi, stream())
    return out


@pytest.mark.parametrize("seed_index", range(len(P.SEEDS)))
def test_uniform_int_bit_for_bit(gpu, seed_index):
    """every offset (0 .. 5 inside the first counters; 2^34 - 6: mid-counter, across the wrap of the low counter word) and range
    (one value, negative, all of int32 = range 2^32) at n = 1003, and every n (single elements, 255 / 256 / 257 around a work-group)
    on two ranges; seeds that differ only in their high words give the streams the host reference gives - different ones"""
    seed, sid = P.SEEDS[seed_index]
    for off in P.OFFSETS:
        for lo, hi in P.INT_RANGES:
            what = f"seed {seed:#x} stream {sid:#x} offset {off} n 1003 range [{lo}, {hi}]"
            draw_ints(gpu, seed, sid, off, 1003, lo, hi).check(torch.tensor(P.uniform_int_ref(seed, sid, off, 1003, lo, hi)), what, ("e",))
        for n in P.INT_NS:
            for lo, hi in ((1, 200), (P.INT32_MIN, P.INT32_MAX)):
                what = f"seed {seed:#x} stream {sid:#x} offset {off} n {n} range [{lo}, {hi}]"
                draw_ints(gpu, seed, sid, off, n, lo, hi).check(torch.tensor(P.uniform_int_ref(seed, sid, off, n, lo, hi)), what, ("e",))


@pytest.mark.parametrize("off,split", [(0, 377), (5, 2), (P.CARRY, 5), (P.CARRY - 300, 295)])
def test_uniform_int_split_draw_equals_one_call(gpu, off, split):
    seed, sid = P.SEEDS[-1]
    n = 1003
    out = Out((n,), torch.int32, gpu, fill=INT_SENTINEL)
    lib().call("gct2_rng_uniform_int", seed, sid, off, out.ptr, split, 1, 200, stream())
    lib().call("gct2_rng_uniform_int", seed, sid, off + split, out.at(split), n - split, 1, 200, stream())
    out.check(torch.tensor(P.uniform_int_ref(seed, sid, off, n, 1, 200)), f"offset {off} split at {split}", ("e",))


def test_uniform_int_rejects_an_empty_range(gpu):
    out = Out((8,), torch.int32, gpu, fill=INT_SENTINEL)
    with pytest.raises(lib().Gct2Error):
        lib().call("gct2_rng_uniform_int", 1, 2, 0, out.ptr, 8, 5, 4, stream())
    out.check(torch.full((8,), INT_SENTINEL, dtype=torch.int32), "rejected call", ("e",))


# ---- gct2_rng_normal -----------------------------------------------------------------------------------------------------------------

def draw_normals(gpu, seed, sid, off, n):
    out = Out((n,), torch.float32, gpu)
    lib().call("gct2_rng_normal", seed, sid, off, out.ptr, n, stream())
    return out


@pytest.mark.parametrize("seed_index", range(len(P.SEEDS)))
def test_normal_per_element(gpu, seed_index, parity_log):
    seed, sid = P.SEEDS[seed_index]
    for off in P.OFFSETS:
        for n in ((16, 1003) if off == P.CARRY else (1003,)):
            what = f"rng_normal seed {seed:#x} stream {sid:#x} offset {off} n {n}"
            out = draw_normals(gpu, seed, sid, off, n)
            check_normals(out.got(), seed, sid, off, what, parity_log)
            out.untouched_outside(what)


def test_normal_grid_stride_loop(gpu, parity_log):
    """2048 work-groups of 256 and 1031 elements more: the second trip of the grid-stride loop, from a stream position inside a counter"""
    seed, sid = P.SEEDS[-1]
    out = draw_normals(gpu, seed, sid, 3, P.NORMAL_LONG_N)
    check_normals(out.got(), seed, sid, 3, f"rng_normal n {P.NORMAL_LONG_N}", parity_log)
    out.untouched_outside("rng_normal, long draw")


def test_normal_split_draw_equals_one_call(gpu):
    seed, sid = P.SEEDS[-1]
    n, split = 1003, 5
    one = draw_normals(gpu, seed, sid, P.CARRY, n)
    two = Out((n,), torch.float32, gpu)
    lib().call("gct2_rng_normal", seed, sid, P.CARRY, two.ptr, split, stream())
    lib().call("gct2_rng_normal", seed, sid, P.CARRY + split, two.at(split), n - split, stream())
    two.check(one.got(), "split at the carry", ("e",))


# ---- gct2_noise_image_rng at the carry -----------------------------------------------------------------------------------------------------

def noise_rng_inputs(gpu, B, HW):
    rng = np.random.default_rng([B, HW, 34])
    x = dev(P.image_values(rng, (B, HW, 3)), gpu)
    t = dev(rng.integers(1, 201, B).astype(np.int32), gpu)
    return x, t


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_noise_rng_general_kernel_at_the_carry(gpu, dt, parity_log):
    """24 elements from 2^34 - 6: the first thread owns counter 2^32 - 2 from its third element on, the third thread counter 2^32.
    eps_out = the gct2_rng_normal stream there, the output = gct2_noise_image on those draws, bit for bit"""
    B, HW, C, steps, off = 2, 4, 3, 200, P.CARRY
    seed, sid = P.SEEDS[-1]
    x, t = noise_rng_inputs(gpu, B, HW)
    eps = Out((B * HW * C,), torch.float32, gpu)
    out, out2 = Out((B, HW, C), E.TDT[dt], gpu, ld=8, off=2), Out((B, HW, C), E.TDT[dt], gpu, ld=4, off=0)
    lib().call("gct2_noise_image_rng", dt, x.data_ptr(), t.data_ptr(), seed, sid, off, eps.ptr, out.ptr, 8, out2.ptr, 4, B, HW, C, steps, stream())
    what = f"noise_image_rng {E.DTYPE_NAMES[dt]} at the carry"
    check_normals(eps.got(), seed, sid, off, what, parity_log)
    eps.untouched_outside(what)
    stream_draws = draw_normals(gpu, seed, sid, off, B * HW * C)
    eps.check(stream_draws.got(), what + ": eps_out against gct2_rng_normal", ("e",))
    ref = Out((B, HW, C), E.TDT[dt], gpu, ld=8, off=2)
    lib().call("gct2_noise_image", dt, x.data_ptr(), t.data_ptr(), eps.ptr, ref.ptr, 8, None, 0, B, HW, C, steps, stream())
    ref.untouched_outside(what + ": gct2_noise_image")
    out.check(ref.got(), what + ": out")
    out2.check(ref.got(), what + ": out2")


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_noise_rng_four_pixel_kernel_at_the_carry(gpu, dt):
    """the train step's kernel (3 channels into the packed 4-slot image, nothing else, stream position a multiple of 12) from
    element 2^34 - 4: its first thread owns counters 2^32 - 1, 2^32 and 2^32 + 1.  Bit-identical to the general kernel (taken when
    eps_out is asked for); slot 3 is written as zero - which also proves that the four-pixel kernel is the one that ran"""
    B, HW, C, steps, off = 2, 8, 3, 200, (1 << 34) - 4
    assert off % 12 == 0 and off >> 2 == (1 << 32) - 1
    seed, sid = P.SEEDS[-1]
    x, t = noise_rng_inputs(gpu, B, HW)
    general, fast = (Out((B, HW, 4), E.TDT[dt], gpu, ld=4, off=0) for _ in range(2))
    assert x.data_ptr() % 16 == 0 and fast.ptr % 16 == 0
    eps = Out((B * HW * C,), torch.float32, gpu)
    lib().call("gct2_noise_image_rng", dt, x.data_ptr(), t.data_ptr(), seed, sid, off, eps.ptr, general.ptr, 4, None, 0, B, HW, C, steps, stream())
    lib().call("gct2_noise_image_rng", dt, x.data_ptr(), t.data_ptr(), seed, sid, off, None, fast.ptr, 4, None, 0, B, HW, C, steps, stream())
    g, f = general.got(), fast.got()
    stored_sentinel = float(torch.tensor(SENTINEL).to(E.TDT[dt]))            # (bf16 holds -1234 as -1232)
    assert float((g[..., 3].float() - stored_sentinel).abs().max()) == 0    # the general kernel leaves the pad slot alone
    assert float(f[..., 3].float().abs().max()) == 0
    E.assert_elementwise_equal(f[..., :3].contiguous(), g[..., :3].contiguous(), ("b", "p", "c"), "four-pixel kernel against the general one")
    assert float(f[..., :3].float().abs().max()) > 0
    general.untouched_outside("general kernel")
    fast.untouched_outside("four-pixel kernel")


@pytest.mark.parametrize("which", ["x", "out"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_noise_rng_packed_call_off_its_alignment_takes_the_general_kernel(gpu, dt, which):
    """the other side of the four-pixel kernel's alignment condition (pointwise.hip: launch_noise_rng): the train step's call with x
    4 bytes, or out 8 bytes, off a 16-byte boundary runs the general kernel - the aligned call's bits in channels 0 .. 2, slot 3 left
    alone (the four-pixel kernel writes a zero there), nothing beside the view touched"""
    B, HW, C, steps, off = 2, 8, 3, 200, 24
    seed, sid = P.SEEDS[-1]
    x, t = noise_rng_inputs(gpu, B, HW)
    fast = Out((B, HW, 4), E.TDT[dt], gpu, ld=4, off=0)
    assert x.data_ptr() % 16 == 0 and fast.ptr % 16 == 0
    lib().call("gct2_noise_image_rng", dt, x.data_ptr(), t.data_ptr(), seed, sid, off, None, fast.ptr, 4, None, 0, B, HW, C, steps, stream())
    f = fast.got()
    assert float(f[..., 3].float().abs().max()) == 0 and float(f[..., :3].float().abs().max()) > 0      # the four-pixel kernel ran
    xb, xp = E.guarded(x, offset=1 if which == "x" else 0)
    flat = Out(((B * HW + 2) * 4,), E.TDT[dt], gpu)              # the packed image between two guard pixels: it starts 8 bytes in
    op = flat.at(4) if which == "out" else flat.at(8)
    assert flat.ptr % 16 == 0 and (xp % 16, op % 16) == ((4, 0) if which == "x" else (0, 8))
    lib().call("gct2_noise_image_rng", dt, xp, t.data_ptr(), seed, sid, off, None, op, 4, None, 0, B, HW, C, steps, stream())
    got = flat.got()
    first = 1 if which == "out" else 2
    g = got.reshape(B * HW + 2, 4)[first:first + B * HW].reshape(B, HW, 4)
    stored_sentinel = float(torch.tensor(SENTINEL).to(E.TDT[dt]))
    assert float((g[..., 3].float() - stored_sentinel).abs().max()) == 0
    E.assert_elementwise_equal(g[..., :3].contiguous(), f[..., :3].contiguous(), ("b", "p", "c"), f"general kernel, {which} off its alignment")
    rest = torch.cat([got[:4 * first], got[4 * (first + B * HW):]]).float()
    assert float((rest - stored_sentinel).abs().max()) == 0
    flat.untouched_outside("general kernel")


# ---- gct2_noise_image, fp32 and bf16 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", P.NOISE_STEPS)
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_noise_image_bit_for_bit(gpu, dt, steps):
    """one image per timestep 1 .. steps against noise_image_f32: every operation rounded to fp32 on its own, bf16 one more rounding
    at the store.  fp32: t = t_int / (steps + 1) by DIVISION like train.py:87 (t_int times the rounded reciprocal gives another
    sqrt(a) at 36 of the 200 timesteps, and an fp32 output shows it).  bf16: the kernel's documented rule is the reciprocal form,
    which on these images gives the same bf16 values (tests/test_pointwise_cases_cpu.py); test_noise_image_bf16_rule_at_ties pins it"""
    case = P.noise_case(steps)
    B, HW, C = case["x"].shape
    x, eps, t = dev(case["x"], gpu), dev(case["eps"], gpu), dev(case["t"], gpu)
    out, out2 = Out((B, HW, C), E.TDT[dt], gpu, ld=8, off=2), Out((B, HW, C), E.TDT[dt], gpu, ld=4, off=0)
    lib().call("gct2_noise_image", dt, x.data_ptr(), t.data_ptr(), eps.data_ptr(), out.ptr, 8, out2.ptr, 4, B, HW, C, steps, stream())
    want = torch.tensor(O.noise_image_f32(case["x"], case["t"], case["eps"], steps, E.DTYPE_NAMES[dt])).to(E.TDT[dt])
    what = f"noise_image {E.DTYPE_NAMES[dt]} steps {steps} (b = t_int - 1)"
    out.check(want, what)
    out2.check(want, what + ": out2")


def test_noise_image_bf16_rule_at_ties(gpu):
    """GCT2_BF16 forms t = t_int * fl(1 / (steps + 1)) (include/gct2.h): 8 images of 8 pixels, each holding an element whose bf16
    value tells that from the division (a tie of the store; tests/test_pointwise_cases_cpu.py) - bit for bit against the documented form"""
    c = P.noise_tie_case()
    B, HW, C = c["x"].shape
    x, eps, t = dev(c["x"], gpu), dev(c["eps"], gpu), dev(c["t"], gpu)
    out = Out((B, HW, C), torch.bfloat16, gpu, ld=4, off=0)
    lib().call("gct2_noise_image", BF16, x.data_ptr(), t.data_ptr(), eps.data_ptr(), out.ptr, 4, None, 0, B, HW, C, c["steps"], stream())
    want = torch.tensor(P.noise_image_bf16_rule(c["x"], c["t"], c["eps"], c["steps"])).to(torch.bfloat16)
    out.check(want, "noise_image bf16 at ties (b = index into the timesteps of the case)")


# ---- gct2_mix_per_image ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coefs", range(len(P.MIX_COEFS)))
def test_mix_per_image_bit_for_bit(gpu, coefs):
    """fl(fl(a[b] x) + fl(c[b] eps)), every operation rounded once: a fused multiply-add differs in a sixth to a quarter of the
    elements of the images with non-trivial coefficients (tests/test_pointwise_cases_cpu.py)"""
    a, c = P.MIX_COEFS[coefs]
    x, eps = P.mix_case()
    B, per = P.MIX_SHAPE
    xd, ed, ad, cd = dev(x, gpu), dev(eps, gpu), dev(np.float32(a), gpu), dev(np.float32(c), gpu)
    out = Out((B * per,), torch.float32, gpu)
    lib().call("gct2_mix_per_image", xd.data_ptr(), ed.data_ptr(), ad.data_ptr(), cd.data_ptr(), out.ptr, B, per, stream())
    torch.cuda.synchronize()
    E.assert_elementwise_equal(out.got().reshape(B, per), torch.tensor(P.mix_per_image_f32(x, eps, a, c)), ("b", "i"), f"mix a = {a}, c = {c}")
    out.untouched_outside("mix_per_image")
    # the scale-only form, in place
    y = Out((B * per,), torch.float32, gpu)
    y.set(xd)
    lib().call("gct2_mix_per_image", y.ptr, None, ad.data_ptr(), None, y.ptr, B, per, stream())
    E.assert_elementwise_equal(y.got().reshape(B, per), torch.tensor(P.mix_per_image_f32(x, None, a, None)), ("b", "i"), f"in-place scale a = {a}")
    y.untouched_outside("mix_per_image in place")


# ---- gct2_diffusion_mix / gct2_diffusion_update -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", P.DIFFUSION_TS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_diffusion_mix_bit_for_bit(gpu, dt, t):
    x, e, _ = P.diffusion_case()
    npix, C = P.DIFFUSION_SHAPE
    a, _ = P.diffusion_alphas(t)
    xd, ed = dev(x, gpu), dev(e, gpu)
    fake = Out((npix * C,), torch.float32, gpu)
    out, out2 = Out((1, npix, C), E.TDT[dt], gpu, ld=8, off=2), Out((1, npix, C), E.TDT[dt], gpu, ld=4, off=0)
    lib().call("gct2_diffusion_mix", dt, xd.data_ptr(), ed.data_ptr(), a, fake.ptr, out.ptr, 8, out2.ptr, 4, npix, C, stream())
    want = P.diffusion_mix_f32(x, e, a)
    what = f"diffusion_mix {E.DTYPE_NAMES[dt]} t {t}"
    E.assert_elementwise_equal(fake.got().reshape(npix, C), torch.tensor(want), ("p", "c"), what + ": fake")
    fake.untouched_outside(what)
    out.check(P.rounded(want, E.TDT[dt]).reshape(1, npix, C), what + ": out")
    out2.check(P.rounded(want, E.TDT[dt]).reshape(1, npix, C), what + ": out2")


@pytest.mark.parametrize("t", P.DIFFUSION_TS)
@pytest.mark.parametrize("mode", [P.SAMPLE_X, P.SAMPLE_EPS, P.SAMPLE_SCALED_EPS, P.SAMPLE_ODE], ids=["x", "eps", "scaled_eps", "ode"])
def test_diffusion_update_bit_for_bit(gpu, mode, t):
    x, e, pred = P.diffusion_case()
    npix, C = P.DIFFUSION_SHAPE
    a, a1 = P.diffusion_alphas(t)
    fake = P.diffusion_mix_f32(x, e, a)
    pd_, fd = dev(pred, gpu), dev(fake, gpu)
    xt, et = Out((npix * C,), torch.float32, gpu), Out((npix * C,), torch.float32, gpu)
    lib().call("gct2_diffusion_update", mode, pd_.data_ptr(), fd.data_ptr(), a, a1, xt.ptr, et.ptr, npix * C, stream())
    x_want, e_want = P.diffusion_update_f32(mode, pred, fake, a, a1)
    what = f"diffusion_update mode {mode} t {t}"
    xt.check(torch.tensor(x_want).reshape(-1), what + ": x_theta", ("e",))
    if e_want is None:          # ODE: eps_theta is not touched
        et.check(torch.full((npix * C,), SENTINEL), what + ": eps_theta", ("e",))
    else:
        et.check(torch.tensor(e_want).reshape(-1), what + ": eps_theta", ("e",))


# ---- gct2_relu_mask / gct2_add ----------------------------------------------------------------------------------------------------------

HELPER_NPIX, HELPER_C = 174800, 3            # 524400 elements > 2048 work-groups x 256: the grid-stride loop's second trip


def planted(rng, tdt, specials):
    """[HELPER_NPIX, HELPER_C] standard-normal values with `specials` written at the start, at the last element of the first trip,
    at the first of the second, and at the very end"""
    v = torch.tensor(rng.standard_normal((HELPER_NPIX, HELPER_C)), dtype=torch.float32).to(tdt).reshape(-1)
    k = len(specials)
    sp = torch.tensor(specials, dtype=torch.float32).to(tdt)
    for start in (0, 2048 * 256 - k, 2048 * 256, v.numel() - k):
        v[start:start + k] = sp
    return v.reshape(HELPER_NPIX, HELPER_C)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_relu_mask_special_values(gpu, dt):
    """d = act > 0 ? d : 0 as a select: NaN, +0, -0 and -inf zero d, a positive denormal and +inf keep its bits (NaN and inf in d
    included); views with pixel strides, the loop's second trip"""
    tdt = E.TDT[dt]
    tiny = {F32: 1e-40, BF16: 1e-40, F16: 6e-8}[dt]             # denormal in the storage type
    nan, inf = float("nan"), float("inf")
    rng = np.random.default_rng([dt, 35])
    act = planted(rng, tdt, [nan, 0.0, -0.0, tiny, -tiny, inf, -inf, 1.0, -1.0, nan, tiny, inf])
    d0 = planted(rng, tdt, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, nan, nan, inf, -inf, -tiny])
    smallest_normal = {F32: 2.0 ** -126, BF16: 2.0 ** -126, F16: 2.0 ** -14}[dt]
    assert 0 < float(act.reshape(-1)[3]) < smallest_normal                                       # survived the conversion as a denormal
    actbuf, actptr = E.poisoned_view(act.to(gpu).reshape(1, HELPER_NPIX, HELPER_C), 4, 1)         # NaN around the input view
    d = Out((1, HELPER_NPIX, HELPER_C), tdt, gpu, ld=8, off=2)
    d.set(d0.to(gpu))
    lib().call("gct2_relu_mask", dt, actptr, 4, d.ptr, 8, HELPER_NPIX, HELPER_C, stream())
    want = torch.where(act.float() > 0, d0, torch.zeros_like(d0))
    d.check(want.reshape(1, HELPER_NPIX, HELPER_C), f"relu_mask {E.DTYPE_NAMES[dt]}")


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_add_special_values(gpu, dt):
    """dst += src as one fp32 add rounded once to the storage type: a sum that overflows the type is inf (fp16: 60000 + 60000),
    a NaN in src or dst comes through, inf - inf is NaN; views with pixel strides, the loop's second trip"""
    tdt = E.TDT[dt]
    big = {F32: 3e38, BF16: 3e38, F16: 60000.0}[dt]
    nan, inf = float("nan"), float("inf")
    rng = np.random.default_rng([dt, 36])
    dst0 = planted(rng, tdt, [big, -big, 1.0, nan, inf, inf, big, 0.0])
    src = planted(rng, tdt, [big, -big, nan, 1.0, -inf, 1.0, -big, -0.0])
    srcbuf, srcptr = E.poisoned_view(src.to(gpu).reshape(1, HELPER_NPIX, HELPER_C), 4, 1)
    dst = Out((1, HELPER_NPIX, HELPER_C), tdt, gpu, ld=8, off=2)
    dst.set(dst0.to(gpu))
    lib().call("gct2_add", dt, dst.ptr, 8, srcptr, 4, HELPER_NPIX, HELPER_C, stream())
    want = (dst0.float() + src.float()).to(tdt)
    assert torch.isinf(want.reshape(-1)[:2]).all() and torch.isnan(want.reshape(-1)[2:5]).all()
    dst.check(want.reshape(1, HELPER_NPIX, HELPER_C), f"add {E.DTYPE_NAMES[dt]}")
