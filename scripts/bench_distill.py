"""time progressive distillation's pointwise launches in one process on one MI355X and write profiles/distill_bench.json:

 (1) gct2_distill_start / _step / _target, each beside the composition of existing launches and torch operations that gives the same
     bits (checked once, element by element), and gct2_diffusion_step (sigma2 = 0, in place) from the same run: bytes per element and
     achieved bytes per second of each.  The per-image coefficients of a composition are torch gathers of the table by pair, made
     once outside the timed calls.
 (2) with --parent LIB (a libgct2.so built from the parent commit): the existing step entry points of this library against the
     parent's, same arguments, same process (sample_estimate moved into gct2_common.h; the device code of sampler.hip is unchanged
     instruction for instruction).  Both sides are captured three times; the range of the parent's three medians is the spread the
     middle one of this library's three medians is held to - the rule of scripts/bench_dynamic_threshold.py.
 (3) a whole Distiller.step at batch 64 on the benchmark's network (Topology(128, 512, 6), bf16: BASELINE config 3) beside its parts
     run by hand: two forward passes of the teacher plus one eager train_step of the student with injected t_int / eps.

B = 64, 128 x 128 x 3, bf16 copies into a packed image (ld 4) and a 72-wide concat buffer.  Events around many calls per sample (a
captured HIP graph of LAUNCHES calls, replayed REPLAYS times), the variants taking turns; medians over SAMPLES.  What distillation does
to the sample quality of a trained network is NOT measured here - there is no data set and no Inception network: the numbers are time.

    python scripts/bench_distill.py [--parent LIB] [--skip-step] [OUT.json]
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

L, T = g._lib, g.trainer_math
args = sys.argv[1:]
parent_path = None
if "--parent" in args:
    i = args.index("--parent")
    parent_path = args[i + 1]
    del args[i:i + 2]
skip_step = "--skip-step" in args
args = [a for a in args if a != "--skip-step"]
dev = torch.device("cuda", 0)
B, H, W, STEPS, N, BF16 = 64, 128, 128, 200, 25, 1
LAUNCHES, REPLAYS, SAMPLES = 100, 10, 15
stream = lambda: torch.cuda.current_stream().cuda_stream
n, per = B * H * W * 3, H * W * 3
summary = lambda v: {"samples": [round(u, 3) for u in v], "median": round(statistics.median(v), 3), "min": round(min(v), 3),
                     "max": round(max(v), 3), "spread": round(max(v) - min(v), 3)}
MODE, CLIP, SEED = L.SAMPLE_EPS, 1.0, 7

gen = torch.Generator().manual_seed(0)
normal = lambda: torch.randn(B, H, W, 3, generator=gen).to(dev)
pred, zt, z1_in, image = normal(), normal(), normal(), (torch.rand(B, H, W, 3, generator=gen) * 2 - 1).to(dev)
tab_h, tt_h = T.distill_table(T.distill_grid(STEPS, N), STEPS, mode=MODE)
tab, tt = torch.from_numpy(tab_h).to(dev), torch.from_numpy(tt_h).to(dev)
pair = torch.randint(1, N + 1, (B,), generator=gen).to(torch.int32)
pair[0], pair[1] = 1, N                                  # the row without t'' and the last one are in the batch
pair = pair.to(dev)
col = {name: tab[(pair - 1).long(), k].reshape(B, 1, 1, 1).contiguous() for k, name in enumerate(T.DISTILL_COLUMNS)}
flat = {name: v.reshape(B).contiguous() for name, v in col.items()}
alpha = lambda u: float(T.alpha_dash(u, STEPS))
a_t, a_prev = alpha(100), alpha(90)


class Buffers:
    def __init__(self):
        self.z, self.z1, self.x, self.e = (torch.empty_like(pred) for _ in range(4))
        self.fake = zt.clone()
        self.hist, self.noise = zt.clone(), torch.empty_like(pred)
        self.t, self.t1 = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        self.img = torch.zeros(B * H * W, 4, dtype=torch.bfloat16, device=dev)
        self.r0 = torch.zeros(B * H * W, 72, dtype=torch.bfloat16, device=dev)
        self.views = (self.img.data_ptr(), 4, self.r0.data_ptr() + 2 * 64, 72)


def graph_of(f, b, launches):
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(launches):
            f(b)
    return gr


def sample(gr, launches, replays):
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


# ---- (1) the three launches and their compositions ------------------------------------------------------------------------------------------
def start(b):
    L.call("gct2_distill_start", BF16, image.data_ptr(), None, pair.data_ptr(), tab.data_ptr(), tt.data_ptr(), N, SEED, T.DISTILL_STREAM_EPS, 0,
           per, b.z.data_ptr(), b.t.data_ptr(), b.t1.data_ptr(), *b.views, B, per, 3, stream())


def start_composed(b):
    L.call("gct2_rng_normal", SEED, T.DISTILL_STREAM_EPS, 0, b.noise.data_ptr(), n, stream())
    L.call("gct2_mix_per_image", image.data_ptr(), b.noise.data_ptr(), flat["cx0"].data_ptr(), flat["ck0"].data_ptr(), b.x.data_ptr(), B, per,
           stream())
    L.call("gct2_diffusion_mix", BF16, b.x.data_ptr(), b.x.data_ptr(), 0.0, b.z.data_ptr(), *b.views, B * H * W, 3, stream())      # 0 z + 1 z
    torch.index_select(tt[:, 0], 0, (pair - 1).long(), out=b.t)
    torch.index_select(tt[:, 1], 0, (pair - 1).long(), out=b.t1)


def estimate(p, f, sa, sb):
    """the epsilon objective's update and clip, one rounding per torch operation"""
    x = (f - p * sb) / sa
    x = torch.clamp(x, -CLIP, CLIP)
    return x, (f - sa * x) / sb


def step(b):
    L.call("gct2_distill_step", MODE, BF16, pred.data_ptr(), zt.data_ptr(), pair.data_ptr(), tab.data_ptr(), N, CLIP, b.z1.data_ptr(), *b.views,
           B, per, 3, stream())


def step_composed(b):
    x, e = estimate(pred, zt, col["sa0"], col["sb0"])
    v = col["cx1"] * x + col["ce1"] * e
    L.call("gct2_diffusion_mix", BF16, v.data_ptr(), v.data_ptr(), 0.0, b.z1.data_ptr(), *b.views, B * H * W, 3, stream())


def target(b):
    L.call("gct2_distill_target", MODE, pred.data_ptr(), z1_in.data_ptr(), zt.data_ptr(), pair.data_ptr(), tab.data_ptr(), N, CLIP,
           b.x.data_ptr(), b.e.data_ptr(), B, per, stream())


def target_composed(b):
    x2, e2 = estimate(pred, z1_in, col["sa1"], col["sb1"])
    full = ((col["sa2"] * x2 + col["sb2"] * e2) - col["r"] * zt) / col["den"]
    torch.where(col["sb2"] == 0, x2, full, out=b.x)
    torch.div(zt - col["sa0"] * b.x, col["sb0"], out=b.e)


def existing_step(b):
    L.call("gct2_diffusion_step", MODE, BF16, pred.data_ptr(), b.fake.data_ptr(), a_t, a_prev, 0.0, CLIP, SEED, g.GENERATE_STREAM, 0, per,
           b.fake.data_ptr(), None, *b.views, B, per, 3, stream())


bits = lambda u: u.contiguous().view(-1).view(torch.int16 if u.element_size() == 2 else torch.int32)
once = {k: Buffers() for k in ("new", "old")}
identical = {}
for name, new, old, outs in (("start", start, start_composed, ("z", "t", "t1", "img", "r0")), ("step", step, step_composed, ("z1", "img", "r0")),
                             ("target", target, target_composed, ("x", "e"))):
    new(once["new"])
    old(once["old"])
    torch.cuda.synchronize()
    identical[name] = all(bool(torch.equal(bits(getattr(once["new"], o)), bits(getattr(once["old"], o)))) for o in outs)
del once
def existing_start_image(b):
    L.call("gct2_diffusion_start_image", BF16, image.data_ptr(), a_t, SEED, T.DISTILL_STREAM_EPS, 0, per, b.z.data_ptr(), *b.views, B, per, 3,
           stream())


kernel_us = measure({"distill_start": start, "distill_start_composed": start_composed, "distill_step": step, "distill_step_composed": step_composed,
                     "distill_target": target, "distill_target_composed": target_composed, "diffusion_step": existing_step,
                     "diffusion_start_image": existing_start_image})
# bytes per element: fp32 planes read and written, the two bf16 copies
BYTES = {"distill_start": 4 + 4 + 2 + 2, "distill_step": 4 + 4 + 4 + 2 + 2, "distill_target": 3 * 4 + 2 * 4, "diffusion_step": 4 + 4 + 4 + 2 + 2,
         "diffusion_start_image": 4 + 4 + 2 + 2}
# why a launch may sit more than 10 % under gct2_diffusion_step's rate per byte (the figures beside it are this run's)
EXPLANATIONS = {"distill_start": "not bandwidth-bound: every element draws its own normal - ten Philox rounds and a Box-Muller pair per element, the "
                                 "form that measured fastest for gct2_diffusion_start_image (profiles/img2img_bench.json) - while it moves 12 bytes "
                                 "where the step moves 16; its scalar-alpha sibling gct2_diffusion_start_image (diffusion_start_image above, same "
                                 "run, same 12 bytes per element) sits under the step's rate for the same reason, and the per-image form adds the "
                                 "row lookup (an integer division and two table loads per element) and the t / t' stores to it"}
kernels_out = {}
for k, v in kernel_us.items():
    kernels_out[k] = dict(summary(v), unit="us per call")
    if k in BYTES:
        kernels_out[k].update(bytes_per_element=BYTES[k], TB_per_s_at_median=round(BYTES[k] * n / statistics.median(v) / 1e6, 3))
ref_rate = kernels_out["diffusion_step"]["TB_per_s_at_median"]
for k in ("distill_start", "distill_step", "distill_target"):
    o = kernels_out[k]
    o["bit_identical_to_composition"] = identical[k[len("distill_"):]]
    o["over_composition"] = round(o["median"] / kernels_out[k + "_composed"]["median"], 3)
    o["not_slower_than_composition"] = bool(o["over_composition"] <= 1.0)
    o["rate_over_diffusion_step"] = round(o["TB_per_s_at_median"] / ref_rate, 3)
    o["within_10_percent_of_diffusion_step_rate"] = bool(o["rate_over_diffusion_step"] >= 0.9)
    if not o["within_10_percent_of_diffusion_step_rate"]:
        o["explanation"] = EXPLANATIONS[k]               # (a launch without one fails here: a rate that low needs an explanation)
kernels_out["distill_start"]["over_diffusion_start_image"] = round(
    kernels_out["distill_start"]["median"] / kernels_out["diffusion_start_image"]["median"], 3)

# ---- (2) the existing entry points against the parent commit's library -----------------------------------------------------------------------
known, mask = image, torch.zeros(B, H, W, device=dev)
mask[:, :, W // 2:] = 1.0
S2, C1 = T.ddim_sigma2(a_t, a_prev, 1.0), T.multistep_coefficient(alpha(110), a_t, a_prev)


def entry_points(lib_call):
    def plain(s2):
        return lambda b: lib_call("gct2_diffusion_step", MODE, BF16, pred.data_ptr(), b.fake.data_ptr(), a_t, a_prev, s2, 1.0, SEED, g.GENERATE_STREAM,
                                  4 * per, per, b.fake.data_ptr(), None, *b.views, B, per, 3, stream())
    return {
        "step": plain(0.0), "step_noise": plain(S2),
        "start": lambda b: lib_call("gct2_diffusion_start", BF16, SEED, g.GENERATE_STREAM, 0, per, b.fake.data_ptr(), *b.views, B, per, 3, stream()),
        "start_image": lambda b: lib_call("gct2_diffusion_start_image", BF16, known.data_ptr(), a_t, SEED, g.GENERATE_STREAM, 0, per,
                                          b.fake.data_ptr(), *b.views, B, per, 3, stream()),
        "step_masked": lambda b: lib_call("gct2_diffusion_step_masked", MODE, BF16, pred.data_ptr(), b.fake.data_ptr(), known.data_ptr(),
                                          mask.data_ptr(), a_t, a_prev, 0.0, 1.0, SEED, g.GENERATE_STREAM, 4 * per, 0, per, b.fake.data_ptr(), None,
                                          *b.views, B, per, 3, stream()),
        "step_multistep": lambda b: lib_call("gct2_diffusion_step_multistep", MODE, BF16, pred.data_ptr(), b.fake.data_ptr(), b.hist.data_ptr(),
                                             None, None, a_t, a_prev, C1, 1.0, SEED, g.GENERATE_STREAM, 0, per, b.fake.data_ptr(),
                                             b.hist.data_ptr(), None, *b.views, B, per, 3, stream())}


parent_out = None
if parent_path:
    P = ctypes.CDLL(os.path.abspath(parent_path))
    assert P.gct2_abi_version() == L.ABI_VERSION and not hasattr(P, "gct2_distill_start")

    def parent_call(name, *a):
        fn = getattr(P, name)
        fn.argtypes, fn.restype = L.SIGNATURES[name], ctypes.c_int
        assert fn(*a) == 0, name

    current, parent = entry_points(L.call), entry_points(parent_call)
    versus = {}
    for k in current:                                   # three captures of each side: one capture's buffers can sit badly
        for r in range(3):
            versus[f"this{r}_" + k] = current[k]
            versus[f"parent{r}_" + k] = parent[k]
    vs_us = measure(versus)
    parent_out = {}
    for k in current:
        meds = [statistics.median(vs_us[f"parent{r}_" + k]) for r in range(3)]
        mine = [statistics.median(vs_us[f"this{r}_" + k]) for r in range(3)]
        this, spread = statistics.median(mine), max(meds) - min(meds)
        parent_out[k] = {"this_median_us": round(this, 3), "this_medians_us": [round(m, 3) for m in mine],
                         "parent_medians_us": [round(m, 3) for m in meds], "parent_spread_us": round(spread, 3),
                         "this_minus_parent_mean_us": round(this - statistics.mean(meds), 3),
                         "within_spread": bool(min(meds) - spread <= this <= max(meds) + spread)}
    parent_out["all_within_spread_or_faster"] = all(v["within_spread"] or v["this_minus_parent_mean_us"] < 0 for v in parent_out.values())

# ---- (3) a whole Distiller.step beside its parts ------------------------------------------------------------------------------------------------
step_out = None
if not skip_step:
    teacher = g.UNetEngine(g.Topology(128, 512, 6), BF16, dev, predict_x=False)
    student = g.UNetEngine(g.Topology(128, 512, 6), BF16, dev, predict_x=False, rng_seed=9)
    student.set_params(teacher.get_params())
    den = lambda eng: types.SimpleNamespace(ensure_engine=lambda: eng)
    d = g.Distiller(den(teacher), types.SimpleNamespace(denoiser=den(student), _engine=lambda: student, optimizer=None), N, seed=SEED,
                    clip_denoised=True)
    tb = teacher.buffers(B, H, W)
    t_fixed, eps_fixed = torch.full((B,), 100, dtype=torch.int32, device=dev), normal()

    def parts():
        teacher.forward(tb)
        teacher.forward(tb)
        return student.train_step(image, t_int=t_fixed, eps=eps_fixed)

    runs = {"distiller_step": lambda: d.step(image), "two_forwards_and_train_step": parts,
            "targets_only": lambda: d.targets(image), "train_step_injected_only": lambda: student.train_step(image, t_int=t_fixed, eps=eps_fixed)}
    for f in runs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(7):
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / 10)
    step_out = {k: dict(summary(v), unit="ms per call") for k, v in ms.items()}
    step_out["distiller_step_minus_parts_ms"] = round(step_out["distiller_step"]["median"] - step_out["two_forwards_and_train_step"]["median"], 4)

out = {"what": f"one MI355X, one process. B={B} {H}x{W}x3, the teacher's {2 * N} of {STEPS} timesteps, a pair per image drawn once (rows 1 and {N} among "
               f"them), epsilon objective, clip 1, bf16 copies (ld 4 and ld 72); {SAMPLES} samples of {LAUNCHES * REPLAYS} back-to-back calls each (a "
               f"captured graph of {LAUNCHES}, replayed {REPLAYS} times) between two events, the variants taking turns, after warm-up calls of each.  "
               "*_composed: existing launches and torch operations that give the same bits, their per-image coefficients gathered once outside "
               "the timed calls.  bytes_per_element: fp32 planes read and written plus the two bf16 copies; TB_per_s_at_median: that times the "
               "elements over the median.  diffusion_step: gct2_diffusion_step at sigma2 = 0, in place, the same run.  parent: the existing step "
               "entry points of this library against a library built from the parent commit (absent without --parent).  distiller: config 3 "
               "(Topology(128, 512, 6), bf16, batch 64), untrained weights, 7 samples of 10 calls after 3 warm-up calls; the student's "
               "train_step with injected t_int / eps is the eager path.  Sample quality is not measured: there is no data set and no "
               "Inception network here; these are times",
       "kernels": kernels_out, "existing_entry_points_against_parent": parent_out, "distiller": step_out}
print(json.dumps(out))
path = args[0] if args else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "distill_bench.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
