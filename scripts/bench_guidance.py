"""time two-network guidance in one process on one MI355X and write profiles/guidance_bench.json:

 (a) gct2_diffusion_step_guided in each form (plain, with noise, masked, multistep, with rows) beside the composition it replaces,
     measured in the same run: torch's sub / mul / add into a combined plane, the existing step entry point on it, and a
     gct2_diffusion_mix(alpha = 0) copy into the second pair of views.  The two must leave the same bits (checked once per form).
 (b) gct2_x0_quantile_guided beside the combine + gct2_x0_quantile.
 (c) the bytes per element the guided step moves and its achieved bytes per second, beside gct2_diffusion_step's in the same run.
 (d) generate at batch 64 on the benchmark's network (Topology(128, 512, 6), bf16: BASELINE config 3), 50 steps of ddim and 20 of
     dpm2m: guided with a constant weight, guided over an interval that covers half the steps, and unguided.
 (e) with --parent LIB (a libgct2.so built from the parent commit): the six existing step entry points of this library against the
     parent's, same arguments, same process; the parent's calls are captured three times, the range of their three medians is the
     run-to-run spread the comparison is held to; this library's are captured three times too and the middle median is compared.

B = 64, 128 x 128 x 3, bf16 copies into a packed image (ld 4) and a 72-wide concat buffer per engine, in place on `fake`.  Events
around 1000 calls per sample (a captured HIP graph of 100 calls, replayed 10 times), the variants taking turns; medians over 15 samples.
What guidance does to the sample quality of a trained network is NOT measured here (no data, no Inception network): the numbers are time.

    python scripts/bench_guidance.py [--parent LIB] [OUT.json]
"""
import ctypes
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gan_class_transfer2_amd as g

L = g._lib
args = sys.argv[1:]
parent_path = None
if "--parent" in args:
    i = args.index("--parent")
    parent_path = args[i + 1]
    del args[i:i + 2]
dev = torch.device("cuda", 0)
B, H, W, STEPS, BF16 = 64, 128, 128, 200, 1
LAUNCHES, REPLAYS, SAMPLES, RUNS = 100, 10, 15, 5
stream = lambda: torch.cuda.current_stream().cuda_stream
n, per = B * H * W * 3, H * W * 3
summary = lambda v: {"samples": [round(u, 3) for u in v], "median": round(statistics.median(v), 3), "min": round(min(v), 3),
                     "max": round(max(v), 3), "spread": round(max(v) - min(v), 3)}
alpha = lambda u: float(g.trainer_math.alpha_dash(u, STEPS))
RANK, FLOOR, SEED, WEIGHT, MODE = g.quantile_rank(0.995, per), 1.0, 7, 3.0, L.SAMPLE_EPS

gen = torch.Generator().manual_seed(0)
normal = lambda: torch.randn(B, H, W, 3, generator=gen).to(dev)
pred, start, known, before = normal(), normal(), (torch.rand(B, H, W, 3, generator=gen) * 2 - 1).to(dev), normal()
pred_guide = (pred + 0.4 * normal()).contiguous()
mask = torch.zeros(B, H, W, device=dev)
mask[:, :, W // 2:] = 1.0
mask[:, :, W // 2 - 1] = 0.5
t = 100
a_t, a_prev = alpha(t), alpha(t - 10)
C1 = g.multistep_coefficient(alpha(t + 10), a_t, a_prev)
S2 = g.trainer_math.ddim_sigma2(a_t, a_prev, 1.0)
need = ctypes.c_size_t(0)
L.call("gct2_x0_quantile_scratch", B, per, ctypes.byref(need))
scratch = torch.empty(need.value, dtype=torch.uint8, device=dev)
rows, q_out = torch.empty(B, 2, device=dev), torch.empty(B, device=dev)
W32 = torch.tensor(WEIGHT, dtype=torch.float32, device=dev)


class Buffers:
    """the state of one variant: fake and hist in place, the two engines' input views, the planes of the composition"""

    def __init__(self):
        self.fake, self.hist = start.clone(), before.clone()
        self.p, self.copy = torch.empty_like(start), torch.empty_like(start)
        pair = lambda: (torch.zeros(B * H * W, 4, dtype=torch.bfloat16, device=dev), torch.zeros(B * H * W, 72, dtype=torch.bfloat16, device=dev))
        self.main, self.guide = pair(), pair()
        self.views = (self.main[0].data_ptr(), 4, self.main[1].data_ptr() + 2 * 64, 72)
        self.gviews = (self.guide[0].data_ptr(), 4, self.guide[1].data_ptr() + 2 * 64, 72)


def graph_of(f, b):
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(LAUNCHES):
            f(b)
    return gr


def sample(gr):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (LAUNCHES * REPLAYS)


def measure(variants):
    """{name: f(buffers)} -> {name: [us per call]}: warm up, capture, then the variants take turns"""
    bufs = {k: Buffers() for k in variants}
    for k, f in variants.items():
        for _ in range(3):
            f(bufs[k])
    torch.cuda.synchronize()
    graphs = {k: graph_of(f, bufs[k]) for k, f in variants.items()}
    for gr in graphs.values():
        gr.replay()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(SAMPLES):
        for k in us:
            us[k].append(sample(graphs[k]))
    return us


ptr = lambda v: v.data_ptr() if v is not None else None
# form -> (masked, multistep, sigma2, with rows)
FORMS = {"plain": (False, False, 0.0, False), "noise": (False, False, S2, False), "masked": (True, False, 0.0, False),
         "multistep": (False, True, 0.0, False), "dynamic": (False, False, 0.0, True)}


def guided(form, with_guide=True, with_views=True):
    masked, multi, s2, dyn = FORMS[form]

    def run(b):
        L.call("gct2_diffusion_step_guided", MODE, BF16, pred.data_ptr(), pred_guide.data_ptr() if with_guide else None,
               WEIGHT if with_guide else 1.0, b.fake.data_ptr(), ptr(b.hist) if multi else None, ptr(known) if masked else None,
               ptr(mask) if masked else None, rows_fixed.data_ptr() if dyn else None, a_t, a_prev, s2, C1 if multi else 0.0, 0.0 if dyn else 1.0,
               SEED, g.GENERATE_STREAM, 4 * per, 0, per, b.fake.data_ptr(), ptr(b.hist) if multi else None, None, *b.views,
               *(b.gviews if with_views else (None, 0, None, 0)), B, per, 3, stream())
    return run


def existing_step(lib_call, form, plane=None):
    """the existing entry point of a form at these arguments, on `plane` (default: pred), through lib_call(name, *args)"""
    masked, multi, s2, dyn = FORMS[form]

    def run(b):
        p = (plane(b) if plane else pred).data_ptr()
        if dyn:
            lib_call("gct2_diffusion_step_dynamic", MODE, BF16, p, b.fake.data_ptr(), None, None, None, rows_fixed.data_ptr(), a_t, a_prev, s2, 0.0,
                     SEED, g.GENERATE_STREAM, 4 * per, 0, per, b.fake.data_ptr(), None, None, *b.views, B, per, 3, stream())
        elif multi:
            lib_call("gct2_diffusion_step_multistep", MODE, BF16, p, b.fake.data_ptr(), b.hist.data_ptr(), None, None, a_t, a_prev, C1, 1.0, SEED,
                     g.GENERATE_STREAM, 0, per, b.fake.data_ptr(), b.hist.data_ptr(), None, *b.views, B, per, 3, stream())
        elif masked:
            lib_call("gct2_diffusion_step_masked", MODE, BF16, p, b.fake.data_ptr(), known.data_ptr(), mask.data_ptr(), a_t, a_prev, s2, 1.0, SEED,
                     g.GENERATE_STREAM, 4 * per, 0, per, b.fake.data_ptr(), None, *b.views, B, per, 3, stream())
        else:
            lib_call("gct2_diffusion_step", MODE, BF16, p, b.fake.data_ptr(), a_t, a_prev, s2, 1.0, SEED, g.GENERATE_STREAM, 4 * per, per,
                     b.fake.data_ptr(), None, *b.views, B, per, 3, stream())
    return run


def combine(b):
    """pg + w (pm - pg): three torch operations into the combined plane"""
    torch.sub(pred, pred_guide, out=b.p)
    torch.mul(b.p, W32, out=b.p)
    torch.add(pred_guide, b.p, out=b.p)


def composition(form):
    step = existing_step(L.call, form, plane=lambda b: b.p)

    def run(b):
        combine(b)
        step(b)
        L.call("gct2_diffusion_mix", BF16, b.fake.data_ptr(), b.fake.data_ptr(), 0.0, b.copy.data_ptr(), *b.gviews, B * H * W, 3, stream())
    return run


# rows for the dynamic form: the guided select on the combined prediction, once
L.call("gct2_x0_quantile_guided", MODE, pred.data_ptr(), pred_guide.data_ptr(), WEIGHT, start.data_ptr(), a_t, RANK, FLOOR, rows.data_ptr(),
       q_out.data_ptr(), scratch.data_ptr(), scratch.numel(), B, per, stream())
torch.cuda.synchronize()
rows_fixed = rows.clone()

# ---- (a) the guided step beside its composition ---------------------------------------------------------------------------------------------
same_bits = {}
for form in FORMS:
    one, two = Buffers(), Buffers()
    guided(form)(one)
    composition(form)(two)
    torch.cuda.synchronize()
    same_bits[form] = bool(all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(one.main + one.guide, two.main + two.guide)) and
                           torch.equal(one.fake.view(torch.int32), two.fake.view(torch.int32)) and
                           torch.equal(one.hist.view(torch.int32), two.hist.view(torch.int32)))
    del one, two
assert all(same_bits.values()), same_bits
variants = {}
for form in FORMS:
    variants["guided_" + form] = guided(form)
    variants["composed_" + form] = composition(form)
variants["guided_plain_no_views"] = guided("plain", with_views=False)
variants["guided_plain_views_only"] = guided("plain", with_guide=False)
variants["step"] = existing_step(L.call, "plain")
us = measure(variants)
step_out = {k: dict(summary(v), unit="us per step") for k, v in us.items()}
med = lambda k: step_out[k]["median"]
step_out["guided_over_composed"] = {form: round(med("guided_" + form) / med("composed_" + form), 3) for form in FORMS}
step_out["every_guided_form_beats_its_composition"] = all(v < 1.0 for v in step_out["guided_over_composed"].values())
step_out["same_bits_as_the_composition"] = same_bits

# ---- (c) traffic ------------------------------------------------------------------------------------------------------------------------------
# per element: the guided step reads pred, pred_guide and fake (fp32) and writes fake (fp32) and four bf16 copies; the step reads pred and
# fake and writes fake and two copies
traffic = {}
for k, bytes_el in (("guided_plain", 3 * 4 + 4 + 4 * 2), ("guided_plain_no_views", 3 * 4 + 4 + 2 * 2), ("guided_plain_views_only", 2 * 4 + 4 + 4 * 2),
                    ("step", 2 * 4 + 4 + 2 * 2)):
    traffic[k] = {"bytes_per_element": bytes_el, "median_us": med(k), "TB_per_s_at_median": round(bytes_el * n / med(k) / 1e6, 3)}


# ---- (b) the guided select beside combine + select ----------------------------------------------------------------------------------------------
def select_guided(b):
    L.call("gct2_x0_quantile_guided", MODE, pred.data_ptr(), pred_guide.data_ptr(), WEIGHT, b.fake.data_ptr(), a_t, RANK, FLOOR, rows.data_ptr(),
           None, scratch.data_ptr(), scratch.numel(), B, per, stream())


def select_composed(b):
    combine(b)
    L.call("gct2_x0_quantile", MODE, b.p.data_ptr(), b.fake.data_ptr(), a_t, RANK, FLOOR, rows.data_ptr(), None, scratch.data_ptr(),
           scratch.numel(), B, per, stream())


def select_plain(b):
    L.call("gct2_x0_quantile", MODE, pred.data_ptr(), b.fake.data_ptr(), a_t, RANK, FLOOR, rows.data_ptr(), None, scratch.data_ptr(),
           scratch.numel(), B, per, stream())


got = []
for f in (select_guided, select_composed):
    f(Buffers())
    torch.cuda.synchronize()
    got.append(rows.clone())
select_same = bool(torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)))
assert select_same
sel_us = measure({"guided": select_guided, "composed": select_composed, "unguided": select_plain})
select_out = {k: dict(summary(v), unit="us per call (memset + 3 digit passes + finish)") for k, v in sel_us.items()}
select_out["guided_over_composed"] = round(select_out["guided"]["median"] / select_out["composed"]["median"], 3)
select_out["guided_beats_the_composition"] = bool(select_out["guided_over_composed"] < 1.0)
select_out["same_bits_as_the_composition"] = select_same


# ---- (e) the existing entry points against the parent commit's library -----------------------------------------------------------------------
def entry_points(lib_call):
    out = {"step": existing_step(lib_call, "plain"), "step_noise": existing_step(lib_call, "noise"),
           "step_masked": existing_step(lib_call, "masked"), "step_multistep": existing_step(lib_call, "multistep"),
           "start": lambda b: lib_call("gct2_diffusion_start", BF16, SEED, g.GENERATE_STREAM, 0, per, b.fake.data_ptr(), *b.views, B, per, 3, stream()),
           "start_image": lambda b: lib_call("gct2_diffusion_start_image", BF16, known.data_ptr(), a_t, SEED, g.GENERATE_STREAM, 0, per,
                                             b.fake.data_ptr(), *b.views, B, per, 3, stream())}
    return out


parent_out = None
if parent_path:
    P = ctypes.CDLL(os.path.abspath(parent_path))
    assert P.gct2_abi_version() == L.ABI_VERSION and not hasattr(P, "gct2_diffusion_step_guided")

    def parent_call(name, *a):
        fn = getattr(P, name)
        fn.argtypes, fn.restype = L.SIGNATURES[name], ctypes.c_int
        assert fn(*a) == 0, name

    current, parent = entry_points(L.call), entry_points(parent_call)
    versus = {}
    for k in current:                               # three captures of each side: one capture's buffers can sit badly
        for r in range(3):
            versus[f"this{r}_" + k] = current[k]
            versus[f"parent{r}_" + k] = parent[k]
    vs_us = measure(versus)
    parent_out = {}
    for k in current:
        meds = [statistics.median(vs_us[f"parent{r}_" + k]) for r in range(3)]
        mine = [statistics.median(vs_us[f"this{r}_" + k]) for r in range(3)]
        this = statistics.median(mine)
        spread = max(meds) - min(meds)
        parent_out[k] = {"this_median_us": round(this, 3), "this_medians_us": [round(m, 3) for m in mine], "parent_medians_us": [round(m, 3) for m in meds],
                         "parent_spread_us": round(spread, 3), "this_minus_parent_mean_us": round(this - statistics.mean(meds), 3),
                         "within_spread": bool(min(meds) <= this <= max(meds))}
    parent_out["all_within_spread_or_faster"] = all(v["within_spread"] or v["this_minus_parent_mean_us"] < 0 for v in parent_out.values())

# ---- (d) a whole generation -------------------------------------------------------------------------------------------------------------------
eng, geng = (g.UNetEngine(g.Topology(128, 512, 6), BF16, dev, predict_x=False, seed=s) for s in (0, 1))
den, guide = (types.SimpleNamespace(ensure_engine=lambda e=e: e) for e in (eng, geng))
kw = dict(seed=3, batch_size=B, size=(H, W), predict_x=False, clip_denoised=True)
runs = {}
for name, more in (("ddim_50", dict(num_steps=50)), ("dpm2m_20", dict(num_steps=20, solver="dpm2m"))):
    taus = g.sampling_timesteps(STEPS, more["num_steps"])
    half = (taus[len(taus) // 4], taus[len(taus) // 4 + len(taus) // 2 - 1])          # an interval that holds half of the timesteps run
    runs[name + "_unguided"] = lambda more=more: g.generate(den, B, **more, **kw)
    runs[name + "_guided"] = lambda more=more: g.generate(den, B, guide=guide, guidance_scale=WEIGHT, **more, **kw)
    runs[name + "_guided_interval"] = lambda more=more, half=half: g.generate(den, B, guide=guide, guidance_scale=WEIGHT, guidance_interval=half,
                                                                              **more, **kw)
outs = {}
for k, f in runs.items():
    for _ in range(2):
        outs[k] = f()
torch.cuda.synchronize()
assert all(bool(torch.isfinite(v).all()) for v in outs.values())
ms = {k: [] for k in runs}
for _ in range(RUNS):
    for k, f in runs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ms[k].append(e0.elapsed_time(e1))
gen_ms = {k: dict(summary(v), unit="ms per run") for k, v in ms.items()}
gen_ms["over_unguided"] = {k: round(gen_ms[k]["median"] / gen_ms[k.split("_guided")[0] + "_unguided"]["median"], 4) for k in runs if "_guided" in k}

# what the two timing requirements came to, and why (the explanations belong to the figures of profiles/guidance_bench.json as committed)
FINDINGS = {
    "guided_forms_against_compositions": "requirement: every guided form takes less time than its composition.  The with-noise form does not "
    "(about 1.00x): it runs the four-element counter kernel, where a thread owns four consecutive elements and stores their compute-dtype "
    "copies itself, so consecutive lanes store four elements apart - with four views instead of two that costs about 44 us over "
    "gct2_diffusion_step with noise, where the one-element-per-thread kernels pay about 22 us for the same two extra views "
    "(guided_plain against guided_plain_no_views).  The views take 6 bytes per 8-byte and per 144-byte row: partial-line writes, far more "
    "traffic than the 24 bytes per element counted under `traffic`, which is why the rate with views is 1.7 TB/s beside 2.9 TB/s without.  "
    "The composition pays for its second pair of views in a launch of the one-element-per-thread pattern.  NOT built and NOT measured: a "
    "guided with-noise kernel of that pattern (philox_normal per element, the form the masked step and gct2_diffusion_start_image take).",
    "existing_entry_points_against_parent": "requirement: every existing entry point within the range of the parent's three medians, or "
    "faster.  The kernels these entry points launch are instruction for instruction the parent's (all 222 kernels of the parent's "
    "sampler.hip are found in this build's device assembly), so a difference is capture-to-capture noise: where `within_spread` is false "
    "the middle median lies a few hundredths to two tenths of a microsecond above the parent's highest, and this library's own three "
    "captures of the same kernel differ by more than that (this_medians_us)."}

out = {"what": f"one MI355X, one process. B={B} {H}x{W}x3, epsilon objective, t=100 -> 90, w = {WEIGHT}, clip 1 (the dynamic form: rows from the guided "
               f"select, rank {RANK} of {per}), bf16 copies (ld 4 and ld 72) for each of the two engines, in place on fake, x0_out NULL; {SAMPLES} "
               f"samples of {LAUNCHES * REPLAYS} back-to-back calls each (a captured graph of {LAUNCHES}, replayed {REPLAYS} times) between two "
               "events, the variants taking turns, after warm-up calls of each.  composed_*: torch sub / mul / add into a combined plane, the "
               "existing step entry point on it, gct2_diffusion_mix(alpha = 0) into the guide's views - the same bits.  traffic: bytes per element "
               "by counting the planes a call reads and writes.  parent: the existing entry points of this library against a library built from "
               "the parent commit, same process, three captures a side; within_spread: this library's middle median lies inside the range of the "
               f"parent's three.  generate: batch 64 on two Topology(128, 512, 6) bf16 engines, untrained weights, {RUNS} runs each after 2 warm-up "
               "runs; the interval holds half of the timesteps run.  Sample quality is not measured: these are times",
       "steps": step_out, "traffic": traffic, "select": select_out, "existing_entry_points_against_parent": parent_out, "generate": gen_ms, "findings": FINDINGS}
print(json.dumps(out))
path = args[0] if args else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "guidance_bench.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
