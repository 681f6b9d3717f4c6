"""time generation's fused pointwise step against the two launches it replaces, in one process on one MI355X, and write
profiles/generate_bench.json:

 (a) gct2_diffusion_step (eta = 0; eta = 1; eta = 0 with clip; eta = 1 on planes 4 bytes off a 16-byte boundary, which takes the
     with-noise kernel's general form instead of its four-element form) against gct2_diffusion_update + gct2_diffusion_mix on the same
     buffers -
     B = 64, 128 x 128 x 3, bf16 copies into a packed image (ld 4) and a 72-wide concat buffer, predict_x, in place on `fake`.  Events
     around many launches per sample (a captured HIP graph of LAUNCHES steps, replayed REPLAYS times, so the host's enqueue rate stays
     out of the number), the variants taking turns; median and spread over the samples.
 (b) a 50-step generate at batch 64 on the benchmark's network (Topology(128, 512, 6), bf16: BASELINE config 3) against the same
     schedule composed from the sampler's existing mix / update launches around the same graph replays; events around whole runs,
     the two taking turns.

    python scripts/bench_generate.py [OUT.json]
"""
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gan_class_transfer2_amd as g
from gan_class_transfer2_amd import sampler as SM

L = g._lib
dev = torch.device("cuda", 0)
B, H, W, STEPS, BF16 = 64, 128, 128, 200, 1
LAUNCHES, REPLAYS, SAMPLES = 100, 10, 15
K, RUNS = 50, 9
stream = lambda: torch.cuda.current_stream().cuda_stream
n, per = B * H * W * 3, H * W * 3
summary = lambda v: {"samples": [round(u, 3) for u in v], "median": round(statistics.median(v), 3), "min": round(min(v), 3),
                     "max": round(max(v), 3), "spread": round(max(v) - min(v), 3)}

# ---- (a) the launches alone ------------------------------------------------------------------------------------------------------------
gen = torch.Generator().manual_seed(0)
pred = (torch.rand(B, H, W, 3, generator=gen) * 2 - 1).to(dev)
start = torch.randn(B, H, W, 3, generator=gen).to(dev)
t = 100
a_t, a_prev = float(g.trainer_math.alpha_dash(t, STEPS)), float(g.trainer_math.alpha_dash(t - 4, STEPS))
s2 = g.ddim_sigma2(a_t, a_prev, 1.0)


pred_odd = torch.empty(n + 1, device=dev)[1:]          # the same values 4 bytes off a 16-byte boundary: the with-noise kernel's general form
pred_odd.copy_(pred.reshape(-1))


class Buffers:
    def __init__(self, odd=False):
        self.fake, self.x, self.e = start.clone(), torch.empty_like(start), torch.empty_like(start)
        if odd:
            self.fake = torch.empty(n + 1, device=dev)[1:]
            self.fake.copy_(start.reshape(-1))
        self.img = torch.zeros(B * H * W, 4, dtype=torch.bfloat16, device=dev)
        self.r0 = torch.zeros(B * H * W, 72, dtype=torch.bfloat16, device=dev)
        self.views = (self.img.data_ptr(), 4, self.r0.data_ptr() + 2 * 64, 72)


def pair(b):
    L.call("gct2_diffusion_update", L.SAMPLE_X, pred.data_ptr(), b.fake.data_ptr(), a_t, a_prev, b.x.data_ptr(), b.e.data_ptr(), n, stream())
    L.call("gct2_diffusion_mix", BF16, b.x.data_ptr(), b.e.data_ptr(), a_prev, b.fake.data_ptr(), *b.views, B * H * W, 3, stream())


def fused(sigma2, clip, odd=False):
    def run(b):
        L.call("gct2_diffusion_step", L.SAMPLE_X, BF16, (pred_odd if odd else pred).data_ptr(), b.fake.data_ptr(), a_t, a_prev, sigma2, clip, 7,
               g.GENERATE_STREAM, 0, per, b.fake.data_ptr(), None, *b.views, B, per, 3, stream())
    return run


variants = {"update_then_mix": pair, "step_eta0": fused(0.0, 0.0), "step_eta1": fused(s2, 0.0), "step_eta0_clip": fused(0.0, 1.0),
            "step_eta1_unaligned": fused(s2, 0.0, odd=True)}
bufs = {k: Buffers(odd=k.endswith("_unaligned")) for k in variants}
for k, f in variants.items():
    for _ in range(20):
        f(bufs[k])
torch.cuda.synchronize()
same = lambda p, q: torch.equal(p.view(torch.int32), q.view(torch.int32))
assert same(bufs["step_eta0"].fake, bufs["update_then_mix"].fake) and torch.equal(bufs["step_eta0"].img, bufs["update_then_mix"].img)
assert torch.equal(bufs["step_eta0"].r0, bufs["update_then_mix"].r0) and bool(torch.isfinite(bufs["step_eta1"].fake).all())
assert same(bufs["step_eta1_unaligned"].fake.contiguous(), bufs["step_eta1"].fake.reshape(-1))       # both forms give the same bits


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
# bytes the algorithm needs per step: fp32 planes read and written + the two bf16 copies (3 of 4 / 3 of 72 slots)
copies = B * H * W * 3 * 2 * 2
need = {k: n * 4 * 3 + copies for k in variants}
need["update_then_mix"] = n * 4 * (2 + 2 + 2 + 1) + copies
kernels = {}
for k, v in us.items():
    kernels[k] = dict(summary(v), unit="us per step", bytes_per_step=need[k], GB_per_s_at_median=round(need[k] / statistics.median(v) / 1e3, 1))
del graphs, bufs

# ---- (b) a whole generation ------------------------------------------------------------------------------------------------------------
eng = g.UNetEngine(g.Topology(128, 512, 6), BF16, dev)
den = types.SimpleNamespace(ensure_engine=lambda: eng)
z = torch.randn(B, H, W, 3, generator=gen).to(dev)
taus = g.sampling_timesteps(STEPS, K)


def composed():
    """generate's schedule from the sampler's existing launches: mix(alpha = 0), then per step evaluate, update, mix(alpha_prev)"""
    S = SM._Sampler(eng, STEPS, L.SAMPLE_X, H, W, True)
    fake, x, e = (torch.empty_like(z) for _ in range(3))
    S.mix(B, z, z, 0.0, fake)
    for k in range(K):
        tau = taus[K - 1 - k]
        pr = S.evaluate(B)
        S.update(pr, fake, float(g.trainer_math.alpha_dash(tau, STEPS)), 0.0, x, e)
        S.mix(B, x, e, float(g.trainer_math.alpha_dash(taus[K - 2 - k] if k < K - 1 else 0, STEPS)), fake)
    return x


runs = {"composed": composed, "generate": lambda: g.generate(den, B, num_steps=K, noise=z, batch_size=B)}
outs = {}
for k, f in runs.items():
    for _ in range(2):
        outs[k] = f()
torch.cuda.synchronize()
assert same(outs["generate"], outs["composed"]) and bool(torch.isfinite(outs["generate"]).all())
ms = {k: [] for k in runs}
for _ in range(RUNS):
    for k, f in runs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ms[k].append(e0.elapsed_time(e1))

out = {"what": f"one MI355X, one process. kernels: B={B} {H}x{W}x3, predict_x, t={t} -> t-4, bf16 copies (ld 4 and ld 72), in place on fake; "
               f"{SAMPLES} samples of {LAUNCHES * REPLAYS} back-to-back steps each (a captured graph of {LAUNCHES}, replayed {REPLAYS} times) between "
               "two events, the variants taking turns, after 20 warm-up steps of each; eta = 0 without clip is bit-identical to the pair; "
               "_unaligned: pred and fake 4 bytes off a 16-byte boundary (the with-noise kernel's general form), the same bits. "
               f"generate: {K} steps of {STEPS} at batch {B} on Topology(128, 512, 6) bf16 from a given noise, against the same schedule composed "
               f"from gct2_diffusion_update + gct2_diffusion_mix around the same forward graph; {RUNS} runs each between two events, taking "
               "turns, after 2 warm-up runs of each; outputs bit-identical",
       "kernels": kernels,
       "step_eta0_minus_pair_median_us": round(kernels["step_eta0"]["median"] - kernels["update_then_mix"]["median"], 3),
       "generate": {k: dict(summary(v), unit="ms per run") for k, v in ms.items()}}
out["generate"]["generate_minus_composed_median_ms"] = round(out["generate"]["generate"]["median"] - out["generate"]["composed"]["median"], 3)
print(json.dumps(out))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "generate_bench.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
