"""time the weighted objective loss, a weighted train step and the sampler's mode V beside what they stand in for, in one process on
one MI355X, and write profiles/objective_loss_bench.json:

 (a) gct2_objective_loss_fwd_bwd (MSE; with a, c and eps, i.e. an epsilon / v target formed on load; with and without lam) against the
     composition it stands in for, gct2_mix_per_image (the target plane) + gct2_mse_fwd_bwd: B = 64, 128 x 128 x 3, fp32.  The
     composition cannot weight per image at all; it is the unweighted floor.
 (b) a train step of the benchmark's network (Topology(128, 512, 6), bf16, batch 64: BASELINE config 3) under the epsilon objective,
     with loss_weighting="min_snr" (eager, non-fused head, the new launch) against the same step without it (eager, fused head).
 (c) gct2_diffusion_step in mode V against mode X at sigma2 = 0 with the clip, bf16 copies, in place.
 Events around many launches per sample (a captured HIP graph of LAUNCHES launches, replayed REPLAYS times, so the host's enqueue rate
 stays out of the number), the variants taking turns; median and spread over the samples.  The steps of (b) run eagerly between two
 events, taking turns.  There is no pass / fail threshold: the numbers are quoted from the JSON.

    python scripts/bench_objective.py [OUT.json]
"""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gan_class_transfer2_amd as g

L = g._lib
dev = torch.device("cuda", 0)
B, H, W, STEPS, BF16 = 64, 128, 128, 200, 1
LAUNCHES, REPLAYS, SAMPLES = 100, 10, 15
STEP_RUNS, STEP_INNER = 9, 10
stream = lambda: torch.cuda.current_stream().cuda_stream
n, per = B * H * W * 3, H * W * 3
summary = lambda v: {"samples": [round(u, 3) for u in v], "median": round(statistics.median(v), 3), "min": round(min(v), 3),
                     "max": round(max(v), 3), "spread": round(max(v) - min(v), 3)}

# ---- (a) the loss launches ---------------------------------------------------------------------------------------------------------------
gen = torch.Generator().manual_seed(0)
pred, x, eps = (torch.randn(B, H, W, 3, generator=gen).to(dev) for _ in range(3))
t_int = torch.randint(1, STEPS + 1, (B,), generator=gen).to(dev, torch.int32)
a, c, _ = g.trainer_math.objective_coefficients(t_int, STEPS, predict_v=True)
lam = torch.from_numpy(g.trainer_math.loss_weight_table("min_snr", 5.0, STEPS, "v")).to(dev)[t_int.long()].contiguous()
need = ctypes.c_size_t(0)
L.check(L.load().gct2_objective_loss_scratch(L.LOSS_MSE, B, H, W, 3, ctypes.byref(need)), "gct2_objective_loss_scratch")


class Buffers:
    def __init__(self):
        self.dpred, self.target = torch.empty_like(pred), torch.zeros_like(pred)
        self.loss, self.partials = torch.zeros(1, device=dev), torch.zeros(1024, device=dev)
        self.scratch = torch.zeros(need.value, device=dev)


def objective(with_lam):
    def run(b):
        L.call("gct2_objective_loss_fwd_bwd", L.LOSS_MSE, pred.data_ptr(), x.data_ptr(), eps.data_ptr(), a.data_ptr(), c.data_ptr(), None,
               lam.data_ptr() if with_lam else None, b.dpred.data_ptr(), b.loss.data_ptr(), b.scratch.data_ptr(), b.scratch.numel(), B, H, W, 3,
               None, stream())
    return run


def composed(b):
    L.call("gct2_mix_per_image", x.data_ptr(), eps.data_ptr(), a.data_ptr(), c.data_ptr(), b.target.data_ptr(), B, per, stream())
    L.call("gct2_mse_fwd_bwd", pred.data_ptr(), b.target.data_ptr(), b.dpred.data_ptr(), b.loss.data_ptr(), b.partials.data_ptr(), n, None, stream())


def mse_alone(b):
    L.call("gct2_mse_fwd_bwd", pred.data_ptr(), b.target.data_ptr(), b.dpred.data_ptr(), b.loss.data_ptr(), b.partials.data_ptr(), n, None, stream())


# ---- (c) the sampler step -------------------------------------------------------------------------------------------------------------------
alpha = lambda u: float(g.trainer_math.alpha_dash(u, STEPS))
a_t, a_prev = alpha(100), alpha(90)


class StepBuffers:
    def __init__(self):
        self.fake = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
        self.img = torch.zeros(B * H * W, 4, dtype=torch.bfloat16, device=dev)
        self.r0 = torch.zeros(B * H * W, 72, dtype=torch.bfloat16, device=dev)
        self.views = (self.img.data_ptr(), 4, self.r0.data_ptr() + 2 * 64, 72)


def step(mode):
    def run(b):
        L.call("gct2_diffusion_step", mode, BF16, pred.data_ptr(), b.fake.data_ptr(), a_t, a_prev, 0.0, 1.0, 7, g.GENERATE_STREAM, 0, per,
               b.fake.data_ptr(), None, *b.views, B, per, 3, stream())
    return run


variants = {"objective_loss": (objective(False), Buffers), "objective_loss_lam": (objective(True), Buffers), "mix_plus_mse": (composed, Buffers),
            "mse_alone": (mse_alone, Buffers), "step_v": (step(L.SAMPLE_V), StepBuffers), "step_x": (step(L.SAMPLE_X), StepBuffers)}
once = {k: make() for k, (_, make) in variants.items()}
for k, (f, _) in variants.items():
    f(once[k])
torch.cuda.synchronize()
same = lambda p, q: torch.equal(p.view(torch.int32), q.view(torch.int32))
dpred_identical = bool(same(once["objective_loss"].dpred, once["mix_plus_mse"].dpred))
loss_difference = abs(float(once["objective_loss"].loss[0]) - float(once["mix_plus_mse"].loss[0])) / float(once["mix_plus_mse"].loss[0])
assert loss_difference < 1e-6 and bool(torch.isfinite(once["step_v"].fake).all())
del once
bufs = {k: make() for k, (_, make) in variants.items()}
for k, (f, _) in variants.items():
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


graphs = {k: graph_of(f, bufs[k]) for k, (f, _) in variants.items()}
for gr in graphs.values():
    gr.replay()
torch.cuda.synchronize()
us = {k: [] for k in variants}
for _ in range(SAMPLES):
    for k in us:
        us[k].append(sample(graphs[k]))
# fp32 planes the algorithm moves: three read and one written by the new launch; x, eps read, target written, pred and target read,
# dpred written by the composition
planes = {"objective_loss": 4, "objective_loss_lam": 4, "mix_plus_mse": 6, "mse_alone": 3}
kernels = {}
for k, v in us.items():
    kernels[k] = dict(summary(v), unit="us per call")
    if k in planes:
        kernels[k].update(bytes_per_call=planes[k] * n * 4, GB_per_s_at_median=round(planes[k] * n * 4 / statistics.median(v) / 1e3, 1))
del graphs, bufs

# ---- (b) a whole train step ----------------------------------------------------------------------------------------------------------------
batch = (torch.rand(B, H, W, 3, generator=gen) * 2 - 1).to(dev)
engines = {"eps_unweighted": g.UNetEngine(g.Topology(128, 512, 6), BF16, dev, predict_x=False),
           "eps_min_snr": g.UNetEngine(g.Topology(128, 512, 6), BF16, dev, predict_x=False)}
engines["eps_min_snr"].set_loss_weighting("min_snr", 5.0)
for eng in engines.values():
    for _ in range(5):
        loss = eng.train_step(batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())
ms = {k: [] for k in engines}
for _ in range(STEP_RUNS):
    for k, eng in engines.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEP_INNER):
            eng.train_step(batch)
        e1.record()
        torch.cuda.synchronize()
        ms[k].append(e0.elapsed_time(e1) / STEP_INNER)

med = lambda k: kernels[k]["median"]
steps = {k: dict(summary(v), unit="ms per step") for k, v in ms.items()}
ratio = round(med("objective_loss") / med("mix_plus_mse"), 3)
out = {"what": f"one MI355X, one process. kernels: B={B} {H}x{W}x3 fp32; objective_loss / objective_loss_lam: gct2_objective_loss_fwd_bwd, MSE, "
               "a, c and eps given (the v target formed on load), without / with lam; mix_plus_mse: gct2_mix_per_image (the target plane) + "
               "gct2_mse_fwd_bwd, which cannot weight per image; mse_alone: gct2_mse_fwd_bwd on a target that exists (the default objective's "
               f"loss). step_v / step_x: gct2_diffusion_step in mode V / X, sigma2 = 0, clip 1, t=100 -> 90, bf16 copies (ld 4 and ld 72), in "
               f"place, x0_out NULL. {SAMPLES} samples of {LAUNCHES * REPLAYS} back-to-back calls each (a captured graph of {LAUNCHES}, replayed "
               f"{REPLAYS} times) between two events, the variants taking turns, after 20 warm-up calls of each. train_step: Topology(128, 512, "
               f"6) bf16, batch {B}, epsilon objective, eager; eps_unweighted takes the fused head, eps_min_snr (loss_weighting='min_snr', gamma "
               f"5) the non-fused head path with the new launch; {STEP_RUNS} runs of {STEP_INNER} steps each between two events, taking turns, "
               "after 5 warm-up steps of each",
       "kernels": kernels,
       "objective_loss_dpred_bit_identical_to_mix_plus_mse": dpred_identical,
       "objective_loss_relative_loss_difference_to_mix_plus_mse": loss_difference,
       "objective_loss_over_mix_plus_mse": ratio,
       "new_launch_beats_the_two_it_replaces": bool(ratio < 1.0),
       "lam_costs_median_us": round(med("objective_loss_lam") - med("objective_loss"), 3),
       "step_v_minus_step_x_median_us": round(med("step_v") - med("step_x"), 3),
       "train_step": steps,
       "min_snr_step_over_unweighted_step": round(steps["eps_min_snr"]["median"] / steps["eps_unweighted"]["median"], 3)}
print(json.dumps(out))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "objective_loss_bench.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
