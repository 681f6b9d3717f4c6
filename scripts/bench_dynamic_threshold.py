"""time dynamic thresholding in one process on one MI355X and write profiles/dynamic_threshold_bench.json:

 (1) gct2_x0_quantile, the whole call (the memset of the tables, three digit passes, the finish), on two inputs: standard normals in
     mode X, and an epsilon-mode input at t = steps (sa = 0.0025) whose keys share one exponent - contention in the histograms depends
     on the values.  Beside it the derived floor (a pass reads pred, and fake outside mode X, once) and the achieved bytes per second.
 (2) gct2_diffusion_step_dynamic beside gct2_diffusion_step / _step_masked / _step_multistep at the same arguments.
 (3) the select and the step against the composition they replace: gct2_diffusion_update, abs, torch.kthvalue, clamp, multiply,
     the eps re-derivation, gct2_diffusion_mix.
 (4) with --parent LIB (a libgct2.so built from the parent commit): the existing step entry points of this library against the
     parent's, same arguments, same process; the parent's calls are captured three times, the range of their three medians is the
     run-to-run spread the comparison is held to; this library's calls are captured three times too, and the middle one of its three
     medians is the figure compared (two captures of the same kernel from the same library differ by a few tenths of a microsecond).
 (5) generate at batch 64 on the benchmark's network (Topology(128, 512, 6), bf16: BASELINE config 3): 50 steps of ddim and 20 of
     dpm2m, clip_denoised="dynamic" against clip_denoised=True.

B = 64, 128 x 128 x 3, bf16 copies into a packed image (ld 4) and a 72-wide concat buffer, in place on `fake`.  Events around many
calls per sample (a captured HIP graph of LAUNCHES calls, replayed REPLAYS times), the variants taking turns; medians over SAMPLES.
What dynamic thresholding does to the sample quality of a trained network is NOT measured here: the numbers are time.

The select's other histogram form (wave-aggregated: one LDS histogram per work-group, equal digits of a wave collapsed into one add)
is a measurement build, `make -C gan-class-transfer2_amd/csrc qsel_agg` -> libgct2_qsel_agg.so; --variant LIB times it beside the
shipped one on the same inputs and checks that it gives the same bits.  The launches of a call one by one come from the profiler, in
runs of their own: `rocprofv3 --kernel-trace --stats -- python scripts/bench_dynamic_threshold.py --select-only shipped` (and
`--select-only variant --variant LIB`) runs nothing but select calls; --kernel-stats / --variant-kernel-stats CSV read the
kernel_stats files those runs leave and put the per-kernel averages beside the whole-call times.

    python scripts/bench_dynamic_threshold.py [--parent LIB] [--variant LIB] [--kernel-stats CSV] [--variant-kernel-stats CSV] [OUT.json]
"""
import ctypes
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import gan_class_transfer2_amd as g

L = g._lib
args = sys.argv[1:]


def option(name):
    """--name VALUE out of args, or None"""
    if name not in args:
        return None
    i = args.index(name)
    value = args[i + 1]
    del args[i:i + 2]
    return value


parent_path, variant_path, select_only = option("--parent"), option("--variant"), option("--select-only")
stats_paths = {"shipped": option("--kernel-stats"), "wave_aggregated": option("--variant-kernel-stats")}
dev = torch.device("cuda", 0)
B, H, W, STEPS, BF16 = 64, 128, 128, 200, 1
LAUNCHES, REPLAYS, SAMPLES, RUNS = 100, 10, 15, 5
stream = lambda: torch.cuda.current_stream().cuda_stream
n, per = B * H * W * 3, H * W * 3
summary = lambda v: {"samples": [round(u, 3) for u in v], "median": round(statistics.median(v), 3), "min": round(min(v), 3),
                     "max": round(max(v), 3), "spread": round(max(v) - min(v), 3)}
alpha = lambda u: float(g.trainer_math.alpha_dash(u, STEPS))
RANK, FLOOR, SEED = g.quantile_rank(0.995, per), 1.0, 7

gen = torch.Generator().manual_seed(0)
normal = lambda: torch.randn(B, H, W, 3, generator=gen).to(dev)
pred, start, known, before = normal(), normal(), (torch.rand(B, H, W, 3, generator=gen) * 2 - 1).to(dev), normal()
mask = torch.zeros(B, H, W, device=dev)
mask[:, :, W // 2:] = 1.0
mask[:, :, W // 2 - 1] = 0.5
t = 100
a_t, a_prev = alpha(t), alpha(t - 10)
C1 = g.multistep_coefficient(alpha(t + 10), a_t, a_prev)
S2 = g.ddim_sigma2(a_t, a_prev, 1.0) if hasattr(g, "ddim_sigma2") else g.trainer_math.ddim_sigma2(a_t, a_prev, 1.0)
need = ctypes.c_size_t(0)
L.call("gct2_x0_quantile_scratch", B, per, ctypes.byref(need))
scratch = torch.empty(need.value, dtype=torch.uint8, device=dev)
rows, q_out = torch.empty(B, 2, device=dev), torch.empty(B, device=dev)


class Buffers:
    def __init__(self):
        self.fake, self.hist = start.clone(), before.clone()
        self.x, self.e = torch.empty_like(start), torch.empty_like(start)
        self.img = torch.zeros(B * H * W, 4, dtype=torch.bfloat16, device=dev)
        self.r0 = torch.zeros(B * H * W, 72, dtype=torch.bfloat16, device=dev)
        self.views = (self.img.data_ptr(), 4, self.r0.data_ptr() + 2 * 64, 72)


def graph_of(f, b, launches=LAUNCHES):
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(launches):
            f(b)
    return gr


def sample(gr, launches=LAUNCHES, replays=REPLAYS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (launches * replays)


def measure(variants, launches=LAUNCHES, replays=REPLAYS, samples=SAMPLES):
    """{name: f(buffers)} -> {name: [us per call]}: warm up, capture, then the variants take turns"""
    bufs = {k: Buffers() for k in variants}
    for k, f in variants.items():
        for _ in range(3):
            f(bufs[k])
    torch.cuda.synchronize()
    graphs = {k: graph_of(f, bufs[k], launches) for k, f in variants.items()}
    for gr in graphs.values():
        gr.replay()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(samples):
        for k in us:
            us[k].append(sample(graphs[k], launches, replays))
    return us


# ---- (1) the select ---------------------------------------------------------------------------------------------------------------------
# the epsilon-mode input at t = steps: x = (fake - pred sb) / sa with sa = 0.0025 - standard normals put nearly every |x| between 256 and
# 1024: two exponents, the top digit's histogram takes nearly all adds in a handful of bins
a_last = alpha(STEPS)


V = None
if variant_path:
    V = ctypes.CDLL(os.path.abspath(variant_path))
    assert V.gct2_abi_version() == L.ABI_VERSION


def variant_call(name, *a):
    fn = getattr(V, name)
    fn.argtypes, fn.restype = L.SIGNATURES[name], ctypes.c_int
    assert fn(*a) == 0, name


def select(mode, p, f, a, call=L.call):
    def run(b):
        call("gct2_x0_quantile", mode, p.data_ptr(), f.data_ptr() if f is not None else None, a, RANK, FLOOR, rows.data_ptr(), q_out.data_ptr(),
               scratch.data_ptr(), scratch.numel(), B, per, stream())
    return run


select_variants = {"normals_mode_x": select(L.SAMPLE_X, pred, None, a_t), "eps_t_steps": select(L.SAMPLE_EPS, pred, start, a_last),
                   "eps_t_100": select(L.SAMPLE_EPS, pred, start, a_t)}
if select_only:                                     # a profiler run: nothing but select calls, of one library
    runs = select_variants if select_only == "shipped" else {
        "normals_mode_x": select(L.SAMPLE_X, pred, None, a_t, variant_call), "eps_t_steps": select(L.SAMPLE_EPS, pred, start, a_last, variant_call)}
    for k in ("normals_mode_x", "eps_t_steps"):     # (the two inputs run different kernels: mode X and the epsilon mode)
        for _ in range(300):
            runs[k](None)
    torch.cuda.synchronize()
    sys.exit(0)
variant_bits_equal = None
if V is not None:
    agg = {"normals_mode_x": select(L.SAMPLE_X, pred, None, a_t, variant_call), "eps_t_steps": select(L.SAMPLE_EPS, pred, start, a_last, variant_call),
           "eps_t_100": select(L.SAMPLE_EPS, pred, start, a_t, variant_call)}
    variant_bits_equal = True
    for k in agg:
        got = []
        for f in (select_variants[k], agg[k]):
            f(None)
            torch.cuda.synchronize()
            got.append((rows.clone(), q_out.clone()))
        variant_bits_equal &= bool(torch.equal(got[0][0].view(torch.int32), got[1][0].view(torch.int32)) and
                                   torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32)))
    assert variant_bits_equal
    select_variants.update({"wave_aggregated_" + k: f for k, f in agg.items()})


def per_launch(path, mode_tag):
    """{kernel: average us} of the select's kernels of one objective out of a rocprofv3 kernel_stats.csv"""
    import csv
    out = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        if "x0_select" not in name:
            continue
        if "pass_kernelILi" in name and f"pass_kernelILi{mode_tag}E" not in name:
            continue
        if "finish" in name:
            short = "finish"
        elif "pass_kernelILi" in name:                  # mangled: ...pass_kernelILi<MODE>ELi<PASS>EE...
            short = "pass_" + name.split("pass_kernelILi")[1].split("ELi")[1][0]
        else:                                           # demangled: ...pass_kernel<MODE, PASS>(...
            inside = name.split("pass_kernel<")[1].split(">")[0].split(",")
            if int(inside[0]) != mode_tag:
                continue
            short = "pass_" + inside[1].strip()
        out[short] = {"average_us": round(float(r["AverageNs"]) / 1e3, 3), "calls": int(r["Calls"])}
    return dict(sorted(out.items()))


sel_us = measure(select_variants)
select_out = {}
for k, v in sel_us.items():
    planes = 1 if k.endswith("normals_mode_x") else 2
    bytes_call = 3 * planes * n * 4
    select_out[k] = dict(summary(v), unit="us per call (memset + 3 digit passes + finish)", fp32_planes_read_per_pass=planes,
                         bytes_read_per_call=bytes_call, TB_per_s_at_median=round(bytes_call / statistics.median(v) / 1e6, 3),
                         derived_floor_us_per_pass=round(planes * n * 4 / 4.28e6, 2), derived_floor_us_per_call=round(bytes_call / 4.28e6, 2))
    which = "wave_aggregated" if k.startswith("wave_aggregated_") else "shipped"
    if stats_paths[which] and not k.endswith("eps_t_100"):
        select_out[k]["per_launch_from_profiler"] = per_launch(stats_paths[which], 0 if k.endswith("normals_mode_x") else 1)
select_variants = {k: f for k, f in select_variants.items() if not k.startswith("wave_aggregated_")}
# the result against torch.kthvalue, once
select_variants["normals_mode_x"](None)
torch.cuda.synchronize()
kth = pred.reshape(B, per).abs().kthvalue(RANK, dim=1).values
select_matches_kthvalue = bool(torch.equal(q_out, kth))
assert select_matches_kthvalue

# ---- (2) the step with a per-image bound beside the existing steps, (3) against the composition -------------------------------------------
select_variants["eps_t_100"](None)                  # rows for the steps below: the epsilon objective at t = 100
torch.cuda.synchronize()
rows_fixed = rows.clone()
MODE = L.SAMPLE_EPS


def dynamic(masked, multi, s2=0.0):
    def run(b):
        L.call("gct2_diffusion_step_dynamic", MODE, BF16, pred.data_ptr(), b.fake.data_ptr(), b.hist.data_ptr() if multi else None,
               known.data_ptr() if masked else None, mask.data_ptr() if masked else None, rows_fixed.data_ptr(), a_t, a_prev, s2,
               C1 if multi else 0.0, SEED, g.GENERATE_STREAM, 4 * per, 0, per, b.fake.data_ptr(), b.hist.data_ptr() if multi else None, None,
               *b.views, B, per, 3, stream())
    return run


def entry_points(lib_call):
    """the existing step entry points at these arguments, through `lib_call(name, *args)`"""
    def step(s2):
        return lambda b: lib_call("gct2_diffusion_step", MODE, BF16, pred.data_ptr(), b.fake.data_ptr(), a_t, a_prev, s2, 1.0, SEED, g.GENERATE_STREAM,
                                  4 * per, per, b.fake.data_ptr(), None, *b.views, B, per, 3, stream())
    return {
        "step": step(0.0), "step_noise": step(S2),
        "start": lambda b: lib_call("gct2_diffusion_start", BF16, SEED, g.GENERATE_STREAM, 0, per, b.fake.data_ptr(), *b.views, B, per, 3, stream()),
        "start_image": lambda b: lib_call("gct2_diffusion_start_image", BF16, known.data_ptr(), a_t, SEED, g.GENERATE_STREAM, 0, per,
                                          b.fake.data_ptr(), *b.views, B, per, 3, stream()),
        "step_masked": lambda b: lib_call("gct2_diffusion_step_masked", MODE, BF16, pred.data_ptr(), b.fake.data_ptr(), known.data_ptr(),
                                          mask.data_ptr(), a_t, a_prev, 0.0, 1.0, SEED, g.GENERATE_STREAM, 4 * per, 0, per, b.fake.data_ptr(), None,
                                          *b.views, B, per, 3, stream()),
        "step_multistep": lambda b: lib_call("gct2_diffusion_step_multistep", MODE, BF16, pred.data_ptr(), b.fake.data_ptr(), b.hist.data_ptr(),
                                             None, None, a_t, a_prev, C1, 1.0, SEED, g.GENERATE_STREAM, 0, per, b.fake.data_ptr(),
                                             b.hist.data_ptr(), None, *b.views, B, per, 3, stream())}


current = entry_points(L.call)
step_variants = {"dynamic": dynamic(False, False), "dynamic_noise": dynamic(False, False, S2), "dynamic_masked": dynamic(True, False),
                 "dynamic_multistep": dynamic(False, True)}
step_variants.update({k: current[k] for k in ("step", "step_noise", "step_masked", "step_multistep")})
step_us = measure(step_variants)
steps_out = {k: dict(summary(v), unit="us per step") for k, v in step_us.items()}
smed = lambda k: steps_out[k]["median"]
steps_out["dynamic_minus_existing_median_us"] = {"plain": round(smed("dynamic") - smed("step"), 3), "noise": round(smed("dynamic_noise") - smed("step_noise"), 3),
                                                 "masked": round(smed("dynamic_masked") - smed("step_masked"), 3),
                                                 "multistep": round(smed("dynamic_multistep") - smed("step_multistep"), 3)}

f32 = lambda v: torch.tensor(float(np.float32(v)), device=dev)
SA, SB, F32FLOOR = f32(np.sqrt(a_t)), f32(np.sqrt(1.0 - a_t)), f32(FLOOR)


def pair(b):
    L.call("gct2_x0_quantile", MODE, pred.data_ptr(), b.fake.data_ptr(), a_t, RANK, FLOOR, rows.data_ptr(), None, scratch.data_ptr(),
           scratch.numel(), B, per, stream())
    L.call("gct2_diffusion_step_dynamic", MODE, BF16, pred.data_ptr(), b.fake.data_ptr(), None, None, None, rows.data_ptr(), a_t, a_prev, 0.0, 0.0,
           SEED, g.GENERATE_STREAM, 0, 0, per, b.fake.data_ptr(), None, None, *b.views, B, per, 3, stream())


def composed(b):
    L.call("gct2_diffusion_update", MODE, pred.data_ptr(), b.fake.data_ptr(), a_t, a_prev, b.x.data_ptr(), b.e.data_ptr(), n, stream())
    q = b.x.reshape(B, per).abs().kthvalue(RANK, dim=1).values
    s = torch.where((q > F32FLOOR) & torch.isfinite(q), q, F32FLOOR).reshape(B, 1, 1, 1)
    x = torch.maximum(torch.minimum(b.x, s), -s) * (F32FLOOR / s)
    e = (b.fake - SA * x) / SB
    L.call("gct2_diffusion_mix", BF16, x.data_ptr(), e.data_ptr(), a_prev, b.fake.data_ptr(), *b.views, B * H * W, 3, stream())


once = {"pair": Buffers(), "composed": Buffers()}
pair(once["pair"])
composed(once["composed"])
torch.cuda.synchronize()
composition_identical = bool(torch.equal(once["pair"].fake.view(torch.int32), once["composed"].fake.view(torch.int32)))
composition_max_abs = float((once["pair"].fake - once["composed"].fake).abs().max())
del once
try:
    comp_us = measure({"select_and_step": pair, "composed": composed}, launches=10, replays=5)
    composed_how = "a captured graph of 10 calls, replayed 5 times, per sample"
except RuntimeError as err:                         # a torch operation that cannot be captured: plain launches between the events
    composed_how = f"plain launches (capture refused: {str(err)[:80]})"
    comp_us = {"select_and_step": [], "composed": []}
    bufs = {k: Buffers() for k in comp_us}
    for _ in range(SAMPLES):
        for k, f in (("select_and_step", pair), ("composed", composed)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                f(bufs[k])
            e1.record()
            torch.cuda.synchronize()
            comp_us[k].append(e0.elapsed_time(e1) * 1e3 / 50)
comp_out = {k: dict(summary(v), unit="us per step") for k, v in comp_us.items()}
comp_out.update(how=composed_how, bit_identical_after_one_step=composition_identical, max_abs_difference_after_one_step=composition_max_abs,
                select_and_step_over_composed=round(comp_out["select_and_step"]["median"] / comp_out["composed"]["median"], 3))
comp_out["new_pair_beats_the_composition"] = bool(comp_out["select_and_step_over_composed"] < 1.0)

# ---- (4) the existing entry points against the parent commit's library -----------------------------------------------------------------------
parent_out = None
if parent_path:
    P = ctypes.CDLL(os.path.abspath(parent_path))
    assert P.gct2_abi_version() == L.ABI_VERSION and not hasattr(P, "gct2_x0_quantile")

    def parent_call(name, *a):
        fn = getattr(P, name)
        fn.argtypes, fn.restype = L.SIGNATURES[name], ctypes.c_int
        assert fn(*a) == 0, name

    parent = entry_points(parent_call)
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
        parent_out[k] = {"this_median_us": round(this, 3), "this_medians_us": [round(m, 3) for m in mine], "parent_medians_us": [round(m, 3) for m in meds], "parent_spread_us": round(spread, 3),
                         "this_minus_parent_mean_us": round(this - statistics.mean(meds), 3),
                         "within_spread": bool(min(meds) - spread <= this <= max(meds) + spread),
                         "this": summary(vs_us["this1_" + k])}
    parent_out["all_within_spread_or_faster"] = all(v["within_spread"] or v["this_minus_parent_mean_us"] < 0 for v in parent_out.values())

# ---- a form that was dropped: NOT measured by this run -----------------------------------------------------------------------------------------
# The first build of gct2_diffusion_step_dynamic tested the rows pointer at run time inside the step kernels all entry points share.
# These are the figures part (4) of this script gave on that build, copied here by hand; the build is not in the repository and no run of
# this script re-measures them.  They are why the bound became a template flag of the step kernels
DROPPED_FORMS = {"runtime_test_of_rows_in_the_shared_step_kernels": {
    "status": "recorded once from a build that is not in the repository; NOT measured by the run that wrote this file",
    "existing_entry_points_against_parent_us": {"step": {"this_median_us": 19.708, "parent_medians_us": [19.816, 20.262, 19.734], "within_spread": True}, "step_noise": {"this_median_us": 26.989, "parent_medians_us": [24.803, 24.868, 24.817], "within_spread": False}, "start": {"this_median_us": 23.982, "parent_medians_us": [23.911, 23.791, 23.889], "within_spread": True}, "start_image": {"this_median_us": 19.425, "parent_medians_us": [19.419, 19.418, 19.39], "within_spread": True}, "step_masked": {"this_median_us": 24.213, "parent_medians_us": [24.097, 24.336, 24.488], "within_spread": True}, "step_multistep": {"this_median_us": 23.722, "parent_medians_us": [23.568, 23.857, 23.517], "within_spread": True}}}}

# ---- (5) a whole generation -------------------------------------------------------------------------------------------------------------------
eng = g.UNetEngine(g.Topology(128, 512, 6), BF16, dev, predict_x=False)
den = types.SimpleNamespace(ensure_engine=lambda: eng)
kw = dict(seed=3, batch_size=B, size=(H, W), predict_x=False)
runs = {"ddim_50_clip": lambda: g.generate(den, B, num_steps=50, clip_denoised=True, **kw),
        "ddim_50_dynamic": lambda: g.generate(den, B, num_steps=50, clip_denoised="dynamic", **kw),
        "dpm2m_20_clip": lambda: g.generate(den, B, num_steps=20, solver="dpm2m", clip_denoised=True, **kw),
        "dpm2m_20_dynamic": lambda: g.generate(den, B, num_steps=20, solver="dpm2m", clip_denoised="dynamic", **kw)}
outs = {}
for k, f in runs.items():
    for _ in range(2):
        outs[k] = f()
torch.cuda.synchronize()
assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) <= 1.0 for v in outs.values())
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
gen_ms["dynamic_minus_clip_ms_per_step"] = {"ddim_50": round((gen_ms["ddim_50_dynamic"]["median"] - gen_ms["ddim_50_clip"]["median"]) / 50, 4),
                                            "dpm2m_20": round((gen_ms["dpm2m_20_dynamic"]["median"] - gen_ms["dpm2m_20_clip"]["median"]) / 20, 4)}
gen_ms["dynamic_over_clip"] = {"ddim_50": round(gen_ms["ddim_50_dynamic"]["median"] / gen_ms["ddim_50_clip"]["median"], 4),
                               "dpm2m_20": round(gen_ms["dpm2m_20_dynamic"]["median"] / gen_ms["dpm2m_20_clip"]["median"], 4)}

out = {"what": f"one MI355X, one process. B={B} {H}x{W}x3, rank {RANK} of {per} (p = 0.995), floor 1, bf16 copies (ld 4 and ld 72), in place on fake, "
               f"x0_out NULL; {SAMPLES} samples of {LAUNCHES * REPLAYS} back-to-back calls each (a captured graph of {LAUNCHES}, replayed {REPLAYS} "
               "times) between two events, the variants taking turns, after warm-up calls of each; the composition with torch.kthvalue is "
               "sampled as `composition.how` says.  select: gct2_x0_quantile, whole call (graph-replayed, events); per_launch_from_profiler: "
               "the average of each of its four kernels from rocprofv3 --kernel-trace --stats over 300 plain calls in a run of its own "
               "(--kernel-stats; absent when no file was given); the derived floor is one read of the fp32 planes per pass at 4.28 TB/s.  "
               "Shipped histogram: one per wave in LDS (privatised), three digit passes (11 + 10 + 10 bits).  wave_aggregated_*: the same "
               "calls through the measurement build of the other histogram form (--variant; absent without it), same bits.  The four-pass "
               "split (8 + 8 + 8 + 7) was NOT built and is NOT measured.  steps: epsilon objective, t=100 -> 90, rows from the select.  "
               "parent: the existing entry points of this library against a library built from the parent commit, same process; the parent's "
               "calls are captured three times, the range of the three medians is the spread; this library's are captured three times too and the "
               "middle of its three medians is compared.  generate: batch 64 on Topology(128, 512, 6) "
               f"bf16, epsilon objective, untrained weights, {RUNS} runs each after 2 warm-up runs.  Sample quality is not measured: these are times",
       "select": select_out, "select_matches_torch_kthvalue": select_matches_kthvalue, "wave_aggregated_bits_equal_shipped": variant_bits_equal,
       "dropped_forms": DROPPED_FORMS, "steps": steps_out, "composition": comp_out,
       "existing_entry_points_against_parent": parent_out, "generate": gen_ms}
print(json.dumps(out))
path = args[0] if args else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dynamic_threshold_bench.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
