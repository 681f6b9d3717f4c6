"""Dynamic thresholding without a GPU: the host math (trainer_math.quantile_rank), what the restatements of tests/dynamic_cases.py
compute (the radix select against numpy's sort on every input class, the finishing rule, the fixed clip's bits under rows {F, 1}),
the conditions tests/test_dynamic_kernels_gpu.py relies on (so it cannot pass vacuously), the three new symbols in the header, the
binding, the plan table and the built library, and the arguments generate refuses before it launches anything."""
import inspect
import math
import os
import re
import types

import numpy as np
import pytest

import dynamic_cases as D
import generate_cases as G
import img2img_cases as I
import multistep_cases as MC
import pointwise_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gct2_x0_quantile_scratch", "gct2_x0_quantile", "gct2_diffusion_step_dynamic")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    """bit equality, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the host math ---------------------------------------------------------------------------------------------------------------------------

def test_quantile_rank():
    import gan_class_transfer2_amd as g
    r = g.trainer_math.quantile_rank
    assert g.quantile_rank is r
    for n in (1, 2, 3009, 49152, 196608):
        assert r(1.0, n) == n                                          # p = 1: the maximum
        assert r(1e-12, n) == 1 and r(5e-324, n) == 1                  # a tiny p: the minimum, never rank 0
    assert r(0.5, 10) == 5 and r(0.25, 8) == 2 and r(0.75, 49152) == 36864      # p n an exact integer: that rank
    assert r(math.nextafter(0.5, 1.0), 10) == 6 and r(math.nextafter(0.25, 1.0), 8) == 3      # just above one: the next
    assert r(0.995, 49152) == 48907 and r(0.995, 196608) == 195625
    for n in (7, 3009, 3072, 525319):
        for p in (0.001, 0.5, 0.9, 0.995, 0.999):
            assert r(p, n) == D.quantile_rank(p, n) == min(n, max(1, math.ceil(p * n)))
    assert isinstance(r(0.995, 3009), int)
    for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            r(bad, 10)
    with pytest.raises(ValueError):
        r(0.5, 0)


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------

def test_key_order():
    v = np.float32([0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 3.4e38, np.inf, -np.inf, np.nan, -np.nan])
    k = D.keys(v)
    assert k[0] == k[1] == 0 and k[2] == k[3] == 1 and k[4] == k[5] and k[7] == k[8] == 0x7F800000
    assert k[1] < k[2] < k[4] < k[6] < k[7] < k[9] and k[10] > k[7]
    assert sum(D.DIGITS) == 31


@pytest.mark.parametrize("case", range(len(D.crafted_cases())), ids=[c[0] for c in D.crafted_cases()])
def test_radix_select_is_the_sort(case):
    """every input class of the GPU test, every rank it uses: the radix restatement with the shipped digit widths equals the sort"""
    name, plane, ranks = D.crafted_cases()[case]
    assert 1 in ranks and plane.shape[1] in ranks
    for row in plane:
        k = D.keys(row)
        for rank in ranks:
            assert D.radix_select(k, rank) == D.kth_key(k, rank), (name, rank)
        assert D.radix_select(k, ranks[-1], (8, 8, 8, 7)) == D.kth_key(k, ranks[-1])        # and another split of the 31 bits
    if name == "many_specials":                                        # the fallback is reached: q is inf and NaN near the top
        q = D.quantile_f32(plane, plane.shape[1])
        assert np.isinf(q[0]) and np.isnan(q[1]) and np.isnan(q[2])
        assert same_bits(D.finish(q, 0.37), np.float32([[0.37, 1.0]] * 3))
    if name == "normals":                                              # the issue's figures: 0.84, 2.8 and 84
        q = D.quantile_f32(plane, D.quantile_rank(D.PERCENTILE, plane.shape[1]))
        assert np.allclose(q, [0.84, 2.8, 84.0], rtol=0.05), q


def test_finishing_rule():
    F = np.float32(1.0)
    q = np.float32([0.5, 1.0, np.nextafter(F, np.float32(2)), 3.0, np.inf, np.nan, 0.0, 3.4e38])
    rows = D.finish(q, 1.0)
    assert same_bits(rows[:, 0], [1.0, 1.0, q[2], 3.0, 1.0, 1.0, 1.0, 3.4e38])
    assert same_bits(rows[:, 1], [1.0, 1.0, F / q[2], F / np.float32(3.0), 1.0, 1.0, 1.0, F / np.float32(3.4e38)])
    assert rows.dtype == np.float32


@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
def test_step_inputs_reach_both_branches(mode):
    """what the GPU test relies on: in every (mode, t) case of the three-image shapes at least one image has q > floor (rescaled) and
    at least one q <= floor (the fixed bound); the long one-image shape is rescaled; the radix select agrees with the sort on all of
    them; the select's x is the step's x; and over the cases more than per_image elements differ in bits from the fixed clip"""
    differ = 0
    for shape in G.SHAPES:
        B, npix, C = shape
        per = npix * C
        rank = D.quantile_rank(D.PERCENTILE, per)
        for t in P.DIFFUSION_TS:
            a_t, a_prev = G.alphas(t)
            p, f = D.step_inputs(shape, mode, t)
            rows, q = D.select_f32(mode, p, f, a_t, rank, D.FLOOR)
            assert np.isfinite(q).all()
            assert (q > D.FLOOR).any(), (shape, t, q)
            assert B == 1 or (q <= D.FLOOR).any(), (shape, t, q)
            assert B == 1 or ((rows[:, 1] == 1).any() and (rows[:, 1] < 1).sum() >= 2)
            if per < 10000:
                _, q_radix = D.select_f32(mode, p, f, a_t, rank, D.FLOOR, select=D.radix_select)
                assert same_bits(q, q_radix)
                x_est, _ = D.estimate_f32(mode, p, f, a_t)
                fixed, xf = D.fixed_clip_step_f32(mode, p, f, a_t, a_prev, D.FLOOR)
                if mode != D.SAMPLE_V:                                 # (the older case modules restate the reference's three objectives)
                    assert same_bits(x_est, P.diffusion_update_f32(mode, p, f, a_t, 0.0)[0])
                    older, xo = G.diffusion_step_f32(mode, p, f, a_t, a_prev, 0.0, D.FLOOR)
                    assert same_bits(fixed, older) and same_bits(xf, xo)
                else:                                                  # V written out here: x = fl(fl(sa f) - fl(sb p)), then the scalar clip
                    sa, sb = np.float32(np.sqrt(np.float64(a_t))), np.float32(np.sqrt(1.0 - np.float64(a_t)))
                    with np.errstate(all="ignore"):
                        xv = sa * f - sb * p
                        assert same_bits(x_est, xv) and same_bits(xf, np.clip(xv, -np.float32(D.FLOOR), np.float32(D.FLOOR)))
                got, x, _ = D.dynamic_step_f32(mode, p, f, rows, a_t, a_prev)
                differ += int((bits(got) != bits(fixed)).sum())
                finite = np.isfinite(x)
                assert np.abs(x[finite]).max() <= D.FLOOR               # the thresholded estimate lies within the floor
    assert differ > G.NPIXS[1] * G.C


@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_floor_rows_are_the_fixed_clip(mode):
    """rows {F, 1}: generate_cases.diffusion_step_f32, img2img_cases.step_masked_f32 and multistep_cases.multistep_step_f32 at clip = F,
    bit for bit (CLIP_SPECIALS in pred)"""
    p, f = G.clip_case()
    h = MC.hist_case(*p.shape)
    kn, el = I.known_case(*p.shape), I.per_element(I.mask_case("pattern", p.shape[0], p.shape[1] // G.C), G.C)
    z, z0 = G.step_case(p.shape[0], p.shape[1])
    for t in P.DIFFUSION_TS:
        a_t, a_prev = G.alphas(t)
        s2 = G.sigma2(a_t, a_prev, 1.0)
        for F in G.CLIPS:
            rows = np.float32([[F, 1.0]] * p.shape[0])
            for s, zz in ((0.0, None), (s2, z)):
                want, x = G.diffusion_step_f32(mode, p, f, a_t, a_prev, s, F, zz)
                got, x0, _ = D.dynamic_step_f32(mode, p, f, rows, a_t, a_prev, s, zz)
                assert same_bits(got, want) and same_bits(x0, x)
                want, x = I.step_masked_f32(mode, p, f, kn, el, a_t, a_prev, s, F, z0, zz)
                got, x0, _ = D.dynamic_step_f32(mode, p, f, rows, a_t, a_prev, s, zz, None, None, kn, el, z0)
                assert same_bits(got, want) and same_bits(x0, x)
            for c1 in MC.C1S:
                want = MC.multistep_step_f32(mode, p, f, h, a_t, a_prev, c1, F, kn, el, z0)
                got = D.dynamic_step_f32(mode, p, f, rows, a_t, a_prev, 0.0, None, h, c1, kn, el, z0)
                assert all(same_bits(a, b) for a, b in zip(got, want))


def test_restatement_tells_a_fused_multiply_add():
    """both contracted forms around x = x * r differ from the restatement on the arrays the GPU test uses"""
    shape = (G.B, G.NPIXS[0], G.C)
    p, f = D.step_inputs(shape, P.SAMPLE_X, 37)
    h = MC.hist_case(G.B, shape[1] * G.C)
    a_t, a_prev = G.alphas(37)
    rows, _ = D.select_f32(P.SAMPLE_X, p, f, a_t, D.quantile_rank(D.PERCENTILE, p.shape[1]), D.FLOOR)
    assert (rows[:, 1] != 1).sum() >= 2
    for c1, term in ((D.C1, 0), (0.0, 1)):
        plain, _, _ = D.dynamic_step_f32(P.SAMPLE_X, p, f, rows, a_t, a_prev, 0.0, None, h, c1)
        fused = D.dynamic_step_fused(P.SAMPLE_X, p, f, rows, a_t, a_prev, h, c1, term)
        assert (bits(plain) != bits(fused)).sum() > 0, (c1, term)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------

def test_new_entry_points_everywhere():
    import ctypes
    import gan_class_transfer2_amd as g
    L = g._lib
    raw = L.load()
    assert L.ABI_VERSION == 17 and raw.gct2_abi_version() == 17       # additions change no signature
    header = open(os.path.join(ROOT, "include", "gct2.h")).read()
    plan = open(os.path.join(ROOT, "gan-class-transfer2_amd", "csrc", "plan.hip")).read()
    for name in NEW:
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(L.SIGNATURES[name]) <= 28, name       # plan.hip MAX_ARGS
        assert hasattr(raw, name)
    assert L.SIGNATURES[NEW[0]] == [L._i, L._sz, ctypes.POINTER(ctypes.c_size_t)] and NEW[0] not in L.PLANNABLE
    assert L.SIGNATURES[NEW[1]] == [L._i, L._vp, L._vp, L._d, ctypes.c_uint32, L._d, L._vp, L._vp, L._vp, L._sz, L._i, L._sz, L._vp]
    step = L.SIGNATURES[NEW[2]]
    assert len(step) == 28 and step[2:8] == [L._vp] * 6 and step[8:12] == [L._d] * 4 and step[12:17] == [L._u64] * 5 and step[-1] is L._vp
    for name in NEW[1:]:
        assert name in L.PLANNABLE and f"GCT2_ENTRY({name})" in plan
    for word in ("key_i = bits(x_i) & 0x7fffffff", "s_b = (q_b > F && q_b < INFINITY) ? q_b : F", "r_b = (s_b == F) ? 1.0f : F / s_b",
                 "x = x < -s ? -s : (x > s ? s : x)", "x = x * r", "e = (f - sa * x) / sb", "the WHOLE network estimate",
                 "profiles/dynamic_threshold_bench.json"):
        assert word in header, word
    need = ctypes.c_size_t(0)
    L.call(NEW[0], 64, 128 * 128 * 3, ctypes.byref(need))              # (host only: no device is touched)
    assert 0 < need.value <= 64 * 32768


def test_a_plan_records_the_calls():
    import gan_class_transfer2_amd as g
    L = g._lib
    plan = L.Plan()
    plan.begin(execute=False)
    try:
        L.call(NEW[1], 0, 64, None, 0.1, 7, 1.0, 64, None, 64, 1 << 20, 1, 12, None)
        L.call(NEW[2], 0, 0, 64, 64, None, None, None, 64, 0.1, 0.2, 0.0, 0.0, 1, 5, 0, 0, 12, 64, None, None, 64, 4, None, 0, 1, 12, 3, None)
    finally:
        plan.end()
    assert plan.n == 2


# ---- what generate refuses before any launch ---------------------------------------------------------------------------------------------------

def fake_denoiser(**switches):
    """an engine that has nothing but what generate reads before it launches: touching anything else is an AttributeError"""
    kw = dict(predict_x=True, predict_scaled_epsilon=False, ordinary_differential_equation=False)
    kw.update(switches)
    eng = types.SimpleNamespace(steps=6, noise_schedule="quadratic", alpha_dash_offset=0.0, **kw)
    return types.SimpleNamespace(ensure_engine=lambda: eng)


def test_generate_refuses_bad_dynamic_arguments(tmp_path):
    import gan_class_transfer2_amd as g
    den = fake_denoiser()
    sig = inspect.signature(g.generate).parameters
    # None stands for the defaults 0.995 and 1.0: "given" is then exact, an explicit 0.995 without the switch is refused too
    assert sig["dynamic_percentile"].default is None and sig["dynamic_floor"].default is None and sig["return_thresholds"].default is False
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf"), "high", True):
        with pytest.raises(ValueError, match="dynamic_percentile"):
            g.generate(den, 2, size=16, clip_denoised="dynamic", dynamic_percentile=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-60, "low", True):
        with pytest.raises(ValueError, match="dynamic_floor"):
            g.generate(den, 2, size=16, clip_denoised="dynamic", dynamic_floor=bad)
    for clip in (None, False, True, 0.5):                              # the dynamic arguments without the switch
        for kw in (dict(dynamic_percentile=0.9), dict(dynamic_floor=2.0), dict(return_thresholds=True), dict(dynamic_percentile=0.995),
                   dict(dynamic_floor=1.0)):
            with pytest.raises(ValueError, match='clip_denoised="dynamic"'):
                g.generate(den, 2, size=16, clip_denoised=clip, **kw)
    for bad in ("Dynamic", "static", "", "1.0"):                      # any other string: today's message, extended
        with pytest.raises(ValueError, match='"dynamic" or a finite bound'):
            g.generate(den, 2, size=16, clip_denoised=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):               # and the fixed bound's own refusals stay
        with pytest.raises(ValueError, match="finite bound > 0"):
            g.generate(den, 2, size=16, clip_denoised=bad)
    # every other refusal comes before any launch with the switch on, the ODE objective among them
    with pytest.raises(ValueError, match="ordinary_differential_equation"):
        g.generate(fake_denoiser(ordinary_differential_equation=True), 2, ordinary_differential_equation=True, size=16, clip_denoised="dynamic")
    for kw, what in ((dict(num_steps=7), "num_steps"), (dict(solver="dpm2m", eta=1.0), "eta"), (dict(strength=0.5), "init"),
                     (dict(return_steps=[5], num_steps=3), "return_steps"), (dict(batch_size=0), "batch_size")):
        with pytest.raises(ValueError, match=what):
            g.generate(den, 2, size=16, clip_denoised="dynamic", **kw)
    with pytest.raises(ValueError, match="return_thresholds"):
        g.generate_to_dir(den, 2, str(tmp_path), clip_denoised="dynamic", return_thresholds=True)
