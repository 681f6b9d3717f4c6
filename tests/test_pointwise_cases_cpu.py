"""The host references of tests/pointwise_cases.py, checked without a GPU: the Philox known answers, the edges of the uniform
formation and of the integer map, and that the inputs of tests/test_pointwise_exact_gpu.py can tell the competing formulations
apart (so that the GPU tests cannot pass vacuously)."""
import numpy as np
import pytest

from oracle import denoiser_oracle as O

import pointwise_cases as P

# Random123's known-answer vectors for philox4x32-10 (kat_vectors): counter, key, output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(v) for v in P.philox4x32_10(ctr, key)) == want


def test_philox_vectorised_equals_scalar():
    """the array form (what every stream reference uses) against one call per counter, across the low-word wrap"""
    seed, sid = P.SEEDS[-1]
    blocks, skip = P.stream_blocks(seed, sid, P.CARRY, 16)
    assert skip == P.CARRY & 3 and blocks.shape == (5, 4)
    for j in range(blocks.shape[0]):
        idx = (P.CARRY >> 2) + j
        one = P.philox4x32_10((idx & P.MASK32, idx >> 32, sid & P.MASK32, sid >> 32), (seed & P.MASK32, seed >> 32))
        assert np.array_equal(one, blocks[j])
    assert (P.CARRY >> 2) < (1 << 32) <= ((P.CARRY + 15) >> 2)               # 16 elements from CARRY cross counter 2^32


def test_high_words_of_seed_and_stream_matter():
    """the first four (seed, stream_id) pairs differ only in bit 32 of one or both: four different streams, at 0 and at the wrap"""
    for off in (0, P.CARRY):
        streams = [P.stream_words(s, i, off, 16) for s, i in P.SEEDS]
        for a in range(len(streams)):
            for b in range(a + 1, len(streams)):
                assert not np.array_equal(streams[a], streams[b]), (a, b, off)
    # and the high counter word: element 2^34 + k is not element k
    s, i = P.SEEDS[0]
    assert not np.array_equal(P.stream_words(s, i, 1 << 34, 16), P.stream_words(s, i, 0, 16))


def test_uniform_formation_edges():
    u = P.uniform_of_word(np.array([0xFFFFFFFF, 0xFFFFFF00, 0x000000FF, 0, 0x100], dtype=np.uint32))
    assert u.dtype == np.float32
    assert u[0] == 1.0 and u[1] == 1.0          # 16777215.5 is a tie between 16777215 and 16777216: to even, 2^24
    assert u[2] == 2.0 ** -25 and u[3] == 2.0 ** -25
    assert u[4] == 1.5 * 2.0 ** -24
    # u1 = 1: rad = 0 and z = 0, finite; u1 = 2^-25: the largest radius of the stream
    assert np.sqrt(-2.0 * np.log(np.float64(u[0]))) == 0.0
    assert 5.8 < np.sqrt(-2.0 * np.log(np.float64(u[2]))) < 5.9


def test_normal_ref_lanes_and_moments():
    seed, sid = P.SEEDS[-1]
    z = P.normal_ref(seed, sid, 0, 1 << 16)
    assert z.dtype == np.float64 and np.isfinite(z).all()
    assert abs(z.mean()) < 2e-2 and abs(z.std() - 1) < 2e-2
    blocks, _ = P.stream_blocks(seed, sid, 0, 8)
    u = P.uniform_of_word(blocks).astype(np.float64)
    for c in range(2):
        for pair in range(2):
            rad, ang = np.sqrt(-2 * np.log(u[c, 2 * pair])), 2 * np.pi * u[c, 2 * pair + 1]
            assert z[4 * c + 2 * pair] == rad * np.cos(ang) and z[4 * c + 2 * pair + 1] == rad * np.sin(ang)
    # a draw from the middle of a counter is the tail of the draw from its start
    assert np.array_equal(P.normal_ref(seed, sid, P.CARRY, 16), P.normal_ref(seed, sid, P.CARRY - 2, 18)[2:])


def test_uniform_int_ref_edges():
    seed, sid = P.SEEDS[-1]
    for off in (0, 3, P.CARRY):
        r = P.stream_words(seed, sid, off, 257)
        full = P.uniform_int_ref(seed, sid, off, 257, P.INT32_MIN, P.INT32_MAX)
        assert full.dtype == np.int32
        assert np.array_equal(full.astype(np.int64), P.INT32_MIN + r.astype(np.int64))          # range = 2^32: lo + r
        assert np.array_equal(P.uniform_int_ref(seed, sid, off, 257, 7, 7), np.full(257, 7, dtype=np.int32))
        for lo, hi in P.INT_RANGES:
            v = P.uniform_int_ref(seed, sid, off, 257, lo, hi).astype(np.int64)
            assert v.min() >= lo and v.max() <= hi
        two = P.uniform_int_ref(seed, sid, off, 257, P.INT32_MIN, P.INT32_MIN + 1)
        assert set(two.tolist()) == {P.INT32_MIN, P.INT32_MIN + 1}
        # the full range is not degenerate: the value a 32-bit `hi - lo + 1` (= 0) would give is lo everywhere
        assert len(set(full.tolist())) > 200


def test_noise_inputs_separate_division_from_reciprocal():
    """t_int / (steps + 1) against t_int * (1 / (steps + 1)) in float32: the GPU test's timesteps must hold enough of the cases
    where the two give another sqrt(a) (36 of 200 at steps = 200), and its data must show the difference in the output"""
    case = P.noise_case(200)
    t = case["t"]
    assert np.array_equal(t, np.arange(1, 201))
    f = np.float32
    td = t.astype(f) / f(201)
    om = f(1.0) - td
    a = (om * om) * f(0.25)
    sa_div, sb_div = np.sqrt(a), np.sqrt(f(1.0) - a)
    sa_rcp, sb_rcp = P.noise_coefs_reciprocal(t, 200)
    nsa, nsb = int((sa_div != sa_rcp).sum()), int((sb_div != sb_rcp).sum())
    print(f"steps 200: sqrt(a) differs at {nsa} timesteps, sqrt(1 - a) at {nsb}")
    assert nsa >= 30
    # the fp32 output shows it in every one of those images.  (The bf16 output cannot: a last-bit change of an fp32 sum moves its
    # bf16 rounding only at a tie, one element in 2^16 - the bf16 case pins the single rounding at the store instead.)
    want = O.noise_image_f32(case["x"], t, case["eps"], 200)
    other = case["x"] * sa_rcp[:, None, None] + case["eps"] * sb_rcp[:, None, None]
    images = int((want != other).reshape(200, -1).any(1).sum())
    print(f"f32: {images} images tell the two formulations apart")
    assert images >= 30
    # bf16 expectation = the fp32 one rounded once, and that rounding is not trivial on this data
    b16 = O.noise_image_f32(case["x"], t, case["eps"], 200, "bf16")
    assert np.array_equal(b16, O.round_bf16(want)) and (b16 != want).mean() > 0.9
    assert np.array_equal(O.round_bf16(other), P.noise_image_bf16_rule(case["x"], t, case["eps"], 200))
    # the bf16 kernel's documented rule is the reciprocal form: on these small cases it gives the same bf16 values as the division,
    # so the reference the bit-for-bit test uses is valid for it
    for steps in P.NOISE_STEPS:
        c = P.noise_case(steps)
        assert np.array_equal(O.noise_image_f32(c["x"], c["t"], c["eps"], steps, "bf16"), P.noise_image_bf16_rule(c["x"], c["t"], c["eps"], steps))


def test_noise_tie_case_separates_the_two_forms_in_bf16():
    """every image of the bf16 tie case holds an element whose bf16 value depends on the form of t (a tie of the store): without
    them the GPU test of the bf16 rule would pass for either form"""
    c = P.noise_tie_case()
    assert c["x"].shape == (P.NOISE_TIE_IMAGES, P.NOISE_TIE_HW, 3) and c["t"].shape == (P.NOISE_TIE_IMAGES,)
    rule = P.noise_image_bf16_rule(c["x"], c["t"], c["eps"], c["steps"])
    division = O.noise_image_f32(c["x"], c["t"], c["eps"], c["steps"], "bf16")
    per_image = (rule != division).reshape(P.NOISE_TIE_IMAGES, -1).sum(1)
    print(f"bf16 elements per image that differ between t_int * (1 / (steps + 1)) and t_int / (steps + 1): {per_image.tolist()}")
    assert (per_image >= 1).all()


def test_noise_image_f32_agrees_with_the_float64_oracle():
    for steps in P.NOISE_STEPS:
        case = P.noise_case(steps)
        x, eps = case["x"].reshape(steps, 4, 1, 3), case["eps"].reshape(steps, 4, 1, 3)
        ref = O.noise_image(x.astype(np.float64), case["t"], eps.astype(np.float64), steps)
        got = O.noise_image_f32(x, case["t"], eps, steps)
        assert got.dtype == np.float32
        assert np.abs(got - ref).max() <= 4 * 2.0 ** -24 * max(1.0, np.abs(ref).max())
        b16 = O.noise_image_f32(x, case["t"], eps, steps, "bf16")
        assert np.array_equal(b16, O.round_bf16(got)) and np.abs(b16 - ref).max() <= 2.0 ** -8 * np.abs(ref).max()


def test_mix_inputs_separate_fused_from_unfused():
    """fl(fl(a x) + fl(c eps)) against fma(a, x, fl(c eps)): at least 10 % of the elements of every image whose coefficients are
    both non-trivial differ (258 and 289 of 1031 on this data), none where a is 0 or 1 or c is 0"""
    x, eps = P.mix_case()
    seen = 0
    for a, c in P.MIX_COEFS:
        want, fused = P.mix_per_image_f32(x, eps, a, c), P.mix_per_image_fused(x, eps, a, c)
        assert want.dtype == np.float32 and fused.dtype == np.float32
        for b in range(P.MIX_SHAPE[0]):
            n = int((want[b] != fused[b]).sum())
            print(f"a = {a[b]}, c = {c[b]}: {n} of {P.MIX_SHAPE[1]} elements differ")
            if a[b] not in (0.0, 1.0) and c[b] not in (0.0, 1.0):
                assert n >= 0.1 * P.MIX_SHAPE[1], (a[b], c[b], n)
                seen += 1
            elif a[b] in (0.0, 1.0) or c[b] == 0.0:
                assert n == 0
    assert seen >= 2
    coefs = {v for a, c in P.MIX_COEFS for v in a + c}
    assert {0.0, 1.0} <= coefs
    # without eps: one product
    a = P.MIX_COEFS[0][0]
    assert np.array_equal(P.mix_per_image_f32(x, None, a, None), np.asarray(a, dtype=np.float32)[:, None] * x)


def test_diffusion_restatements_agree_with_float64():
    x, e, pred = P.diffusion_case()
    for t in P.DIFFUSION_TS:
        a, a1 = P.diffusion_alphas(t)
        assert 0.0 < a < a1 <= 0.25
        fake = P.diffusion_mix_f32(x, e, a)
        assert fake.dtype == np.float32
        ref = a ** 0.5 * x.astype(np.float64) + (1 - a) ** 0.5 * e
        assert np.abs(fake - ref).max() <= 4 * 2.0 ** -24 * np.abs(ref).max()
        f64, p64 = fake.astype(np.float64), pred.astype(np.float64)
        refs = {P.SAMPLE_X: (p64, (f64 - a ** 0.5 * p64) / (1 - a) ** 0.5),
                P.SAMPLE_EPS: ((f64 - p64 * (1 - a) ** 0.5) / a ** 0.5, p64),
                P.SAMPLE_SCALED_EPS: ((f64 - p64) / a ** 0.5, p64 / (1 - a) ** 0.5),
                P.SAMPLE_ODE: ((p64 * (1 - a) ** 0.5 - f64 * (1 - a1) ** 0.5) / (a1 ** 0.5 * (1 - a) ** 0.5 - a ** 0.5 * (1 - a1) ** 0.5), None)}
        for mode, (x_ref, e_ref) in refs.items():
            xt, et = P.diffusion_update_f32(mode, pred, fake, a, a1)
            assert xt.dtype == np.float32
            # aggregate agreement only (the bits are the GPU test's business); the ODE quotient subtracts nearly equal products
            assert np.linalg.norm(xt - x_ref) <= 5e-6 * np.linalg.norm(x_ref), (t, mode)
            if e_ref is None:
                assert et is None
            else:
                assert et.dtype == np.float32 and np.linalg.norm(et - e_ref) <= 5e-7 * np.linalg.norm(e_ref), (t, mode)
