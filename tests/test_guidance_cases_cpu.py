"""Two-network guidance without a GPU: the host math (trainer_math.guidance_table, guidance_launches), what the restatements of
tests/guidance_cases.py compute (the combine against a fused multiply-add and against the older restatements of the step), the conditions
tests/test_guidance_kernels_gpu.py relies on (so it cannot pass vacuously), the two new symbols in the header, the binding, the plan
table and the built library, and the arguments generate refuses before it launches anything."""
import inspect
import math
import os
import re
import types

import numpy as np
import pytest

import dynamic_cases as D
import generate_cases as G
import guidance_cases as GC
import img2img_cases as I
import multistep_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gct2_x0_quantile_guided", "gct2_diffusion_step_guided")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the host math ---------------------------------------------------------------------------------------------------------------------------

def test_guidance_table_forms():
    import gan_class_transfer2_amd as g
    table = g.trainer_math.guidance_table
    assert g.guidance_table is table
    assert table(2.5, 6) == [2.5] * 6 and table(1, 3) == [1.0, 1.0, 1.0] and table(np.float32(0.5), 2) == [0.5, 0.5]
    assert table(lambda t: 1.0 + t / 2, 4) == [1.5, 2.0, 2.5, 3.0]                # f(t), t = 1..steps; entry t - 1
    assert table([3.0, 1.0, 0.0, -1.0], 4) == [3.0, 1.0, 0.0, -1.0] and table(np.array([1.0, 2.0]), 2) == [1.0, 2.0]
    assert table((2.0, 2.0, 2.0), 3) == [2.0] * 3
    assert all(type(w) is float for w in table(np.float32(2.0), 3) + table(lambda t: np.float64(t), 3) + table([1, 2, 3], 3))
    # the interval keeps the weight inside and is 1.0 - the main network alone - outside, in every form
    assert table(3.0, 6, (2, 4)) == [1.0, 3.0, 3.0, 3.0, 1.0, 1.0]
    assert table(3.0, 6, (1, 6)) == [3.0] * 6 and table(3.0, 6, (6, 6)) == [1.0] * 5 + [3.0] and table(3.0, 6, [1, 1]) == [3.0] + [1.0] * 5
    assert table(lambda t: float(t), 5, (2, 3)) == [1.0, 2.0, 3.0, 1.0, 1.0]
    assert table([5.0, 4.0, 3.0, 2.0], 4, (np.int64(3), 4)) == [1.0, 1.0, 3.0, 2.0]


def test_guidance_table_refusals():
    import gan_class_transfer2_amd as g
    table = g.trainer_math.guidance_table
    for bad in (True, False, None, "3", float("nan"), float("inf"), -float("inf"), 1e39, np.bool_(True)):
        with pytest.raises(ValueError):
            table(bad, 6)
    for bad in ([1.0, 2.0], [1.0] * 7, [1.0, 2.0, True, 1.0, 1.0, 1.0], [1.0, float("nan"), 1.0, 1.0, 1.0, 1.0], [1.0, "2", 1.0, 1.0, 1.0, 1.0],
                [1.0, None, 1.0, 1.0, 1.0, 1.0], [1e39] * 6):
        with pytest.raises(ValueError):
            table(bad, 6)
    for bad in (lambda t: float("inf") if t == 4 else 1.0, lambda t: None, lambda t: True, lambda t: "w"):
        with pytest.raises(ValueError):
            table(bad, 6)
    for bad in ((0, 3), (1, 7), (4, 3), (2,), (1, 2, 3), 3, (1.0, 3), (True, 3), ("1", "3"), (-1, 2)):
        with pytest.raises(ValueError, match="guidance_interval"):
            table(2.0, 6, bad)
    with pytest.raises(ValueError):
        table(2.0, 0)


def test_launch_decision():
    import gan_class_transfer2_amd as g
    launches = g.trainer_math.guidance_launches
    assert g.guidance_launches is launches
    # all ones: no new entry point, no guide evaluation, no views, no copy - guide=None launch for launch
    assert launches([1.0] * 5) == (False, [(False, False, False)] * 5) and launches([1, 1.0]) == (False, [(False, False, False)] * 2)
    assert launches([]) == (False, [])
    # a constant weight: the copy at the start of the batch, every step reads the guide, every step but the last writes its views
    start, steps = launches([3.0] * 4)
    assert start and steps == [(True, True, True)] * 3 + [(True, True, False)]
    # an interval in the middle: the step BEFORE it runs the guided entry point only to write the views
    start, steps = launches([1.0, 1.0, 2.0, 2.0, 1.0, 1.0])
    assert not start
    assert steps == [(False, False, False), (True, False, True), (True, True, True), (True, True, False), (False, False, False), (False, False, False)]
    # the first step run is guided: the copy; w = 0 is guided too (the guide alone)
    assert launches([0.0, 1.0, 0.5]) == (True, [(True, True, False), (True, False, True), (True, True, False)])
    for weights in ([1.0, 2.0, 1.0, 3.0, 3.0, 1.0], [2.0], [1.0], [1.0, 1.0 + 2.0 ** -52], [0.0, 0.0]):
        start, steps = launches(weights)
        guided = [w != 1.0 for w in weights]
        assert start == guided[0] and len(steps) == len(weights)
        for k, (entry, pg, views) in enumerate(steps):
            assert pg == guided[k]                                         # the guide is evaluated exactly where w != 1
            assert views == (k + 1 < len(weights) and guided[k + 1])       # views are written exactly before guided steps
            assert entry == (pg or views)                                  # the new entry point only where it is needed
        # the guide's views are current at every guided step: written by the copy or by the step before
        for k in range(len(weights)):
            assert not guided[k] or (start if k == 0 else steps[k - 1][2])


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------

def test_the_combine():
    pm, pg, *_ = GC.planes(75)
    assert same_bits(GC.combine_f32(pm, pg, 0.0), pg)                           # w = 0: the guide's bits (finite, non-zero planes)
    one = GC.combine_f32(pm, pg, 1.0)                                           # w = 1: the main plane up to the rounding of pg + (pm - pg)
    assert np.abs(one - pm).max() <= 2 * np.spacing(np.abs(np.stack([pm, pg])).max())
    for w in (0.5, 3.0, -1.0):
        p = GC.combine_f32(pm, pg, w)
        want = pg.astype(np.float64) + w * (pm.astype(np.float64) - pg.astype(np.float64))
        assert np.abs(p - want).max() <= 4 * np.spacing(np.float32(np.abs(want).max()))
        assert p.dtype == np.float32 and not same_bits(p, pm) and not same_bits(p, pg)
    big = np.random.default_rng(5).standard_normal((GC.B, 4800)).astype(np.float32)
    assert (bits(GC.combine_f32(big, big[::-1], 3.0)) != bits(GC.combine_fused(big, big[::-1], 3.0))).sum() > 0      # it tells an fma


@pytest.mark.parametrize("mode", G.MODES, ids=G.MODE_IDS)
def test_step_restatement_is_the_older_ones(mode):
    """guidance_cases.step_f32 on one plane: generate_cases.diffusion_step_f32, img2img_cases.step_masked_f32 and
    multistep_cases.multistep_step_f32, bit for bit, with no clip and with one"""
    pm, pg, f, h, kn, m = GC.planes(75)
    el = I.per_element(m, GC.C)
    z, z0 = G.step_case(GC.B, 75)
    a_t, a_prev = G.alphas(GC.T)
    s2 = G.sigma2(a_t, a_prev, 1.0)
    for clip in (0.0, 0.5):
        for s, zz in ((0.0, None), (s2, z)):
            want, x = G.diffusion_step_f32(mode, pm, f, a_t, a_prev, s, clip, zz)
            got = GC.step_f32(mode, pm, f, a_t, a_prev, clip=clip, s2=s, z=zz)
            assert same_bits(got[0], want) and same_bits(got[1], x)
            want, x = I.step_masked_f32(mode, pm, f, kn, el, a_t, a_prev, s, clip, z0, zz)
            got = GC.step_f32(mode, pm, f, a_t, a_prev, clip=clip, s2=s, z=zz, known=kn, mask_el=el, z0=z0)
            assert same_bits(got[0], want) and same_bits(got[1], x)
        for c1 in (0.0, GC.C1):
            for k, e, zz in ((None, None, None), (kn, el, z0)):
                want = MC.multistep_step_f32(mode, pm, f, h, a_t, a_prev, c1, clip, k, e, zz)
                got = GC.step_f32(mode, pm, f, a_t, a_prev, clip=clip, hist=h, c1=c1, known=k, mask_el=e, z0=zz)
                assert all(same_bits(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("mode", GC.MODES, ids=GC.MODE_IDS)
def test_case_inputs_are_meaningful(mode):
    """what the GPU tests rely on: on every shape the guided result differs from both unguided ones at every weight but the one that IS
    an unguided one; at the w > 1 of the threshold cases some |x0| exceeds the floor and the select engages for some image; the guided
    select's x is the guided step's x"""
    a_t, a_prev = G.alphas(GC.T)
    for per in sorted({s[0] for s in GC.STEP_SHAPES.values()} | {GC.SELECT_PER_IMAGE}):
        pm, pg, f, h, kn, m = GC.planes(per, mode)
        main = GC.step_f32(mode, pm, f, a_t, a_prev)
        guide = GC.step_f32(mode, pg, f, a_t, a_prev)
        assert not same_bits(main[0], guide[0])
        for w in GC.WEIGHTS:
            got = GC.guided_step_f32(mode, pm, pg, w, f, a_t, a_prev)
            assert np.isfinite(got[0]).all() and not same_bits(got[0], main[0])
            assert same_bits(got[0], guide[0]) == (w == 0.0) and same_bits(got[1], guide[1]) == (w == 0.0)
        x, _ = D.estimate_f32(mode, GC.combine_f32(pm, pg, GC.W_THRESHOLD), f, a_t)
        assert (np.abs(x) > GC.FLOOR).any()
        rank = D.quantile_rank(GC.PERCENTILE, per)
        rows, q = GC.guided_select_f32(mode, pm, pg, GC.W_THRESHOLD, f, a_t, rank, GC.FLOOR)
        assert (q > GC.FLOOR).any() and (rows[:, 1] < 1).any(), (per, q)
        plain_rows, _ = D.select_f32(mode, pm, f, a_t, rank, GC.FLOOR)
        assert not same_bits(rows, plain_rows)                                   # the guided select is not the main plane's
        got = GC.guided_step_f32(mode, pm, pg, GC.W_THRESHOLD, f, a_t, a_prev, rows=rows)
        assert np.abs(got[1]).max() <= GC.FLOOR                                 # the thresholded estimate lies within the floor
        fixed = GC.guided_step_f32(mode, pm, pg, GC.W_THRESHOLD, f, a_t, a_prev, clip=GC.FLOOR)
        assert not same_bits(got[0], fixed[0])
        assert same_bits(D.quantile_f32(x, rank), q)
    m = GC.planes(75)[5]
    assert ((m > 0) & (m < 1)).any() and (m <= 0).any() and (m >= 1).any()       # a fractional mask, and both selects


def test_perturbed_parameters():
    params = {"b": np.ones((2, 3), np.float32), "a": np.zeros(4, np.float32), "n": np.arange(3)}
    one, two = GC.perturbed(params), GC.perturbed(params)
    assert all(np.array_equal(one[k], two[k]) for k in params) and np.array_equal(one["n"], params["n"])
    assert all(one[k].dtype == params[k].dtype and one[k].shape == params[k].shape for k in params)
    assert not np.array_equal(one["a"], params["a"]) and abs(float(one["b"].mean()) - 1.0) < 0.2


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------

def test_new_entry_points_everywhere():
    import ctypes
    import gan_class_transfer2_amd as g
    L = g._lib
    raw = L.load()
    assert L.ABI_VERSION == 17 and raw.gct2_abi_version() == 17       # additions change no signature
    header = open(os.path.join(ROOT, "include", "gct2.h")).read()
    plan = open(os.path.join(ROOT, "gan-class-transfer2_amd", "csrc", "plan.hip")).read()
    max_args = int(re.search(r"constexpr int MAX_ARGS = (\d+);", plan).group(1))
    for name in NEW:
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(L.SIGNATURES[name]) <= max_args, name
        assert hasattr(raw, name) and name in L.PLANNABLE and f"GCT2_ENTRY({name})" in plan
    sel, step = L.SIGNATURES[NEW[0]], L.SIGNATURES[NEW[1]]
    old_sel, old_step = L.SIGNATURES["gct2_x0_quantile"], L.SIGNATURES["gct2_diffusion_step_dynamic"]
    assert sel == old_sel[:2] + [L._vp, L._d] + old_sel[2:]                       # gct2_x0_quantile + pred_guide, w
    assert len(step) == len(old_step) + 7 == 35
    assert step == old_step[:3] + [L._vp, L._d] + old_step[3:12] + [L._d] + old_step[12:24] + [L._vp, L._i, L._vp, L._i] + old_step[24:]
    for word in ("d = pred - pred_guide", "t = (float)w * d", "p = pred_guide + t", "out4 without out3 is GCT2_EINVAL", "clip must then be 0",
                 "(float)w must be 1", "profiles/guidance_bench.json"):
        assert word in header, word
    need, same = ctypes.c_size_t(0), ctypes.c_size_t(0)               # the same scratch-size function serves both selects
    L.call("gct2_x0_quantile_scratch", 3, GC.SELECT_PER_IMAGE, ctypes.byref(need))
    assert need.value > 0


def test_a_plan_records_the_calls():
    import gan_class_transfer2_amd as g
    L = g._lib
    plan = L.Plan()
    plan.begin(execute=False)
    try:
        L.call(NEW[0], 0, 64, 64, 3.0, None, 0.1, 7, 1.0, 64, None, 64, 1 << 20, 1, 12, None)
        L.call(NEW[1], 0, 0, 64, 64, 3.0, 64, None, None, None, 64, 0.1, 0.2, 0.0, 0.0, 0.0, 1, 5, 0, 0, 12, 64, None, None, 64, 4, None, 0, 64, 4,
               None, 0, 1, 12, 3, None)
    finally:
        plan.end()
    assert plan.n == 2


# ---- what generate refuses before any launch ---------------------------------------------------------------------------------------------------

def fake_denoiser(**over):
    """an engine that has nothing but what generate reads before it launches: touching anything else is an AttributeError"""
    kw = dict(steps=6, noise_schedule="quadratic", alpha_dash_offset=0.0, predict_x=True, predict_scaled_epsilon=False,
              ordinary_differential_equation=False, dtype=0, device="cuda:0")
    kw.update(over)
    eng = types.SimpleNamespace(**kw)
    return types.SimpleNamespace(ensure_engine=lambda: eng)


def test_generate_refuses_bad_guidance_arguments(tmp_path):
    import gan_class_transfer2_amd as g
    den, guide = fake_denoiser(), fake_denoiser()
    sig = inspect.signature(g.generate).parameters
    assert sig["guide"].default is None and sig["guidance_scale"].default is None and sig["guidance_interval"].default is None
    assert sig["guide_use_ema"].default is False
    run = lambda d=den, **kw: g.generate(d, 2, size=16, **kw)
    for kw in (dict(guidance_scale=2.0), dict(guidance_interval=(1, 3)), dict(guidance_scale=1.0, guidance_interval=(1, 3)), dict(guide_use_ema=True)):
        with pytest.raises(ValueError, match="guide"):
            run(**kw)                                                            # the guidance arguments without a guide
    with pytest.raises(ValueError, match="guidance_scale"):
        run(guide=guide)                                                         # a guide without a weight
    with pytest.raises(ValueError, match="guidance_scale"):
        run(guide=guide, guidance_interval=(1, 3))
    with pytest.raises(ValueError, match="clone_denoiser"):
        run(guide=den, guidance_scale=2.0)                                       # the same engine
    for other in (dict(steps=8), dict(noise_schedule="cosine"), dict(alpha_dash_offset=0.01)):
        with pytest.raises(ValueError, match="steps, noise schedule and offset"):
            run(guide=fake_denoiser(**other), guidance_scale=2.0)
    with pytest.raises(ValueError, match="objective"):
        run(guide=fake_denoiser(predict_x=False), guidance_scale=2.0)            # the guide predicts epsilon, the main one x
    with pytest.raises(ValueError, match="objective"):
        run(fake_denoiser(predict_x=False), guide=guide, guidance_scale=2.0, predict_x=False)      # the explicit switches apply to both
    with pytest.raises(ValueError, match="dtype"):
        run(guide=fake_denoiser(dtype=1), guidance_scale=2.0)
    ode = dict(ordinary_differential_equation=True)
    with pytest.raises(ValueError, match="ordinary_differential_equation"):
        run(fake_denoiser(**ode), guide=fake_denoiser(**ode), guidance_scale=2.0, **ode)
    for bad in (float("nan"), float("inf"), 1e39, True, "2", [1.0] * 5, [1.0, 2.0, float("nan"), 1.0, 1.0, 1.0], lambda t: float("inf")):
        with pytest.raises(ValueError, match="guidance_scale"):
            run(guide=guide, guidance_scale=bad)
    for bad in ((0, 3), (1, 7), (4, 3), (1.5, 3), (2,)):
        with pytest.raises(ValueError, match="guidance_interval"):
            run(guide=guide, guidance_scale=2.0, guidance_interval=bad)
    # every other refusal still comes before any launch with a guide given
    for kw, what in ((dict(num_steps=7), "num_steps"), (dict(solver="dpm2m", eta=1.0), "eta"), (dict(strength=0.5), "init"),
                     (dict(batch_size=0), "batch_size"), (dict(clip_denoised="static"), "dynamic")):
        with pytest.raises(ValueError, match=what):
            run(guide=guide, guidance_scale=2.0, **kw)
    with pytest.raises(ValueError, match="guidance_scale"):
        g.generate_to_dir(den, 2, str(tmp_path), size=16, guide=guide)           # generate_to_dir passes them through
    assert not math.isnan(g.guidance_table(2.0, 6)[0])
