"""time the second-order multistep step against the first-order launches beside it and against the composition it replaces, in one
process on one MI355X, and write profiles/multistep_bench.json:

 (a) gct2_diffusion_step_multistep, plain and masked, at c1 = 0 and at c1 != 0; gct2_diffusion_step and gct2_diffusion_step_masked at
     sigma2 = 0 beside them (the launches solver="ddim" makes: the floor - the new launch reads and writes one more fp32 plane); and the
     composition the plain launch replaces at c1 != 0: gct2_diffusion_update, the torch clamp / sub / mul / add of the extrapolation, the
     copy into the history, the eps re-derivation, gct2_diffusion_mix(a_prev).
     B = 64, 128 x 128 x 3, bf16 copies into a packed image (ld 4) and a 72-wide concat buffer, predict_x, clip 1, in place on `fake` and
     on the history, x0_out NULL (what generate passes at every step but the marked ones), a half-plane mask with a blended column.
     Events around many launches per sample (a captured HIP graph of LAUNCHES steps, replayed REPLAYS times, so the host's enqueue rate
     stays out of the number), the variants taking turns; median and spread over the samples.
 (b) generate at batch 64 on the benchmark's network (Topology(128, 512, 6), bf16: BASELINE config 3): 20 steps of solver="dpm2m"
     against 50 steps of solver="ddim", and both solvers at 20 steps; events around whole runs, taking turns.

What the solver does to sample quality on a trained network is NOT measured here (no data, no trained weights): the numbers are time.

    python scripts/bench_multistep.py [OUT.json]
"""
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
dev = torch.device("cuda", 0)
B, H, W, STEPS, BF16 = 64, 128, 128, 200, 1
LAUNCHES, REPLAYS, SAMPLES = 100, 10, 15
K2, K1, RUNS = 20, 50, 9
stream = lambda: torch.cuda.current_stream().cuda_stream
n, per = B * H * W * 3, H * W * 3
summary = lambda v: {"samples": [round(u, 3) for u in v], "median": round(statistics.median(v), 3), "min": round(min(v), 3),
                     "max": round(max(v), 3), "spread": round(max(v) - min(v), 3)}

# ---- (a) the launches alone ------------------------------------------------------------------------------------------------------------
gen = torch.Generator().manual_seed(0)
pred = (torch.rand(B, H, W, 3, generator=gen) * 2.5 - 1.25).to(dev)            # a tenth of the estimates beyond the clip
known = (torch.rand(B, H, W, 3, generator=gen) * 2 - 1).to(dev)
before = (torch.rand(B, H, W, 3, generator=gen) * 2 - 1).to(dev)               # the estimate of the step before
start = torch.randn(B, H, W, 3, generator=gen).to(dev)
mask = torch.zeros(B, H, W, device=dev)
mask[:, :, W // 2:] = 1.0
mask[:, :, W // 2 - 1] = 0.5
t = 100
alpha = lambda u: float(g.trainer_math.alpha_dash(u, STEPS))
a_t, a_prev = alpha(t), alpha(t - 10)
C1 = g.multistep_coefficient(alpha(t + 10), a_t, a_prev)
assert C1 > 0
CLIP, SEED, OFF0 = 1.0, 7, 0


class Buffers:
    def __init__(self):
        self.fake, self.hist = start.clone(), before.clone()
        self.x, self.e = torch.empty_like(start), torch.empty_like(start)
        self.img = torch.zeros(B * H * W, 4, dtype=torch.bfloat16, device=dev)
        self.r0 = torch.zeros(B * H * W, 72, dtype=torch.bfloat16, device=dev)
        self.views = (self.img.data_ptr(), 4, self.r0.data_ptr() + 2 * 64, 72)


def multistep(c1, masked):
    def run(b):
        L.call("gct2_diffusion_step_multistep", L.SAMPLE_X, BF16, pred.data_ptr(), b.fake.data_ptr(), b.hist.data_ptr(),
               known.data_ptr() if masked else None, mask.data_ptr() if masked else None, a_t, a_prev, c1, CLIP, SEED, g.GENERATE_STREAM, OFF0,
               per, b.fake.data_ptr(), b.hist.data_ptr(), None, *b.views, B, per, 3, stream())
    return run


def step(b):
    L.call("gct2_diffusion_step", L.SAMPLE_X, BF16, pred.data_ptr(), b.fake.data_ptr(), a_t, a_prev, 0.0, CLIP, SEED, g.GENERATE_STREAM, 0, per,
           b.fake.data_ptr(), None, *b.views, B, per, 3, stream())


def step_masked(b):
    L.call("gct2_diffusion_step_masked", L.SAMPLE_X, BF16, pred.data_ptr(), b.fake.data_ptr(), known.data_ptr(), mask.data_ptr(), a_t, a_prev,
           0.0, CLIP, SEED, g.GENERATE_STREAM, 0, OFF0, per, b.fake.data_ptr(), None, *b.views, B, per, 3, stream())


# the scalars as the kernel forms them: fp32, sa / sb from double square roots; tensors, so that torch divides (a Python scalar
# divisor may become a multiplication by its reciprocal)
f32 = lambda v: torch.tensor(float(np.float32(v)), device=dev)
SA, SB, C32 = f32(np.sqrt(a_t)), f32(np.sqrt(1.0 - a_t)), f32(C1)


def composed(b):
    L.call("gct2_diffusion_update", L.SAMPLE_X, pred.data_ptr(), b.fake.data_ptr(), a_t, a_prev, b.x.data_ptr(), b.e.data_ptr(), n, stream())
    x = torch.clamp(b.x, -CLIP, CLIP)
    d = x + C32 * (x - b.hist)
    b.hist.copy_(x)
    ed = (b.fake - SA * d) / SB
    L.call("gct2_diffusion_mix", BF16, d.data_ptr(), ed.data_ptr(), a_prev, b.fake.data_ptr(), *b.views, B * H * W, 3, stream())


variants = {"multistep_c0": multistep(0.0, False), "multistep_c1": multistep(C1, False), "multistep_masked_c0": multistep(0.0, True),
            "multistep_masked_c1": multistep(C1, True), "step": step, "step_masked": step_masked, "composed_c1": composed}
same = lambda p, q: torch.equal(p.view(torch.int32), q.view(torch.int32))
# one step of each from the same state: what agrees bit for bit (recorded, and asserted where the library's own launches are compared)
once = {k: Buffers() for k in variants}
for k, f in variants.items():
    f(once[k])
torch.cuda.synchronize()
assert all(bool(torch.isfinite(b.fake).all()) for b in once.values())
assert same(once["multistep_c0"].fake, once["step"].fake) and torch.equal(once["multistep_c0"].r0, once["step"].r0)
assert same(once["multistep_masked_c0"].fake, once["step_masked"].fake) and torch.equal(once["multistep_masked_c0"].img, once["step_masked"].img)
assert not same(once["multistep_c1"].fake, once["multistep_c0"].fake) and same(once["multistep_c1"].hist, once["multistep_c0"].hist)
p, q = once["multistep_c1"], once["composed_c1"]
composition_identical = bool(same(p.fake, q.fake) and same(p.hist, q.hist) and torch.equal(p.img, q.img) and torch.equal(p.r0, q.r0))
composition_max_abs = float((p.fake - q.fake).abs().max())
assert composition_max_abs < 1e-5
del once, p, q
bufs = {k: Buffers() for k in variants}
for k, f in variants.items():
    for _ in range(20):
        f(bufs[k])
torch.cuda.synchronize()


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


graphs = {k: graph_of(f, bufs[k]) for k, f in variants.items()}
for gr in graphs.values():
    gr.replay()
torch.cuda.synchronize()
us = {k: [] for k in variants}
for _ in range(SAMPLES):
    for k in us:
        us[k].append(sample(graphs[k]))
# bytes the algorithm needs per step: fp32 planes read and written (+ the mask) + the two bf16 copies (3 of 4 / 3 of 72 slots)
copies = B * H * W * 3 * 2 * 2
need = {"multistep_c0": n * 4 * 4 + copies, "multistep_c1": n * 4 * 5 + copies, "multistep_masked_c0": n * 4 * 5 + B * H * W * 4 + copies,
        "multistep_masked_c1": n * 4 * 6 + B * H * W * 4 + copies, "step": n * 4 * 3 + copies, "step_masked": n * 4 * 4 + B * H * W * 4 + copies}
kernels = {}
for k, v in us.items():
    kernels[k] = dict(summary(v), unit="us per step")
    if k in need:
        kernels[k].update(bytes_per_step=need[k], bytes_per_element=round(need[k] / n, 2), GB_per_s_at_median=round(need[k] / statistics.median(v) / 1e3, 1))
del graphs, bufs

# ---- (b) a whole generation ------------------------------------------------------------------------------------------------------------
eng = g.UNetEngine(g.Topology(128, 512, 6), BF16, dev)
den = types.SimpleNamespace(ensure_engine=lambda: eng)
kw = dict(seed=3, batch_size=B, size=(H, W))
runs = {f"ddim_{K1}": lambda: g.generate(den, B, num_steps=K1, **kw),
        f"dpm2m_{K2}": lambda: g.generate(den, B, num_steps=K2, solver="dpm2m", **kw),
        f"ddim_{K2}": lambda: g.generate(den, B, num_steps=K2, **kw)}
outs = {}
for k, f in runs.items():
    for _ in range(2):
        outs[k] = f()
torch.cuda.synchronize()
assert all(bool(torch.isfinite(v).all()) for v in outs.values())
assert not torch.equal(outs[f"dpm2m_{K2}"], outs[f"ddim_{K2}"])
ms = {k: [] for k in runs}
for _ in range(RUNS):
    for k, f in runs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ms[k].append(e0.elapsed_time(e1))

med = lambda k: kernels[k]["median"]
gen_ms = {k: dict(summary(v), unit="ms per run") for k, v in ms.items()}
fused_over_composed = round(med("multistep_c1") / med("composed_c1"), 3)
out = {"what": f"one MI355X, one process. kernels: B={B} {H}x{W}x3, predict_x, clip 1, t={t} -> t-10 (c1 = {C1:.4f} from t+10), bf16 copies (ld 4 "
               f"and ld 72), in place on fake and on the history, x0_out NULL, a half-plane mask with one blended column; {SAMPLES} samples of "
               f"{LAUNCHES * REPLAYS} back-to-back steps each (a captured graph of {LAUNCHES}, replayed {REPLAYS} times) between two events, the "
               "variants taking turns, after 20 warm-up steps of each. multistep_*: gct2_diffusion_step_multistep, plain and masked, at c1 = 0 "
               "(the history is written, not read) and at c1 != 0; step / step_masked: gct2_diffusion_step / gct2_diffusion_step_masked at "
               "sigma2 = 0, bit-identical to multistep_*_c0 after one step from the same state; composed_c1: gct2_diffusion_update + torch clamp, "
               "sub, mul, add, the copy into the history, the eps re-derivation (mul, sub, div) + gct2_diffusion_mix. "
               f"generate: batch {B} on Topology(128, 512, 6) bf16 at {STEPS} training steps, eta = 0, from a seed: {K2} steps of solver='dpm2m' "
               f"against {K1} and {K2} steps of solver='ddim'; {RUNS} runs each between two events, taking turns, after 2 warm-up runs of each. "
               "Sample quality on a trained network is not measured: these are times",
       "kernels": kernels,
       "composed_c1_bit_identical_to_multistep_c1": composition_identical,
       "composed_c1_max_abs_difference": composition_max_abs,
       "multistep_c1_over_composed_c1": fused_over_composed,
       "fused_launch_beats_the_composition": bool(fused_over_composed < 1.0),
       "multistep_minus_step_median_us": {"plain_c0": round(med("multistep_c0") - med("step"), 3), "plain_c1": round(med("multistep_c1") - med("step"), 3),
                                          "masked_c0": round(med("multistep_masked_c0") - med("step_masked"), 3),
                                          "masked_c1": round(med("multistep_masked_c1") - med("step_masked"), 3)},
       "generate": gen_ms}
out["generate"][f"dpm2m_{K2}_over_ddim_{K1}"] = round(gen_ms[f"dpm2m_{K2}"]["median"] / gen_ms[f"ddim_{K1}"]["median"], 3)
out["generate"][f"dpm2m_{K2}_minus_ddim_{K2}_median_ms"] = round(gen_ms[f"dpm2m_{K2}"]["median"] - gen_ms[f"ddim_{K2}"]["median"], 3)
print(json.dumps(out))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "multistep_bench.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
