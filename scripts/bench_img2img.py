"""time the two launches of image-conditioned generation against what they replace, in one process on one MI355X, and write
profiles/img2img_bench.json:

 (a) gct2_diffusion_step_masked at sigma2 = 0 and at eta = 1 (and at eta = 1 on a plane 4 bytes off a 16-byte boundary: the general
     form); gct2_diffusion_step alone in the same two settings - the floor: the masked launch reads two more planes and draws the
     starting noise again; and the composition the masked launch replaces: gct2_diffusion_step with x0_out, gct2_rng_normal,
     gct2_diffusion_mix(known, z0, a_prev), then the torch select / blend of fake' and of x0 and the re-store of the two bf16 views.
     gct2_diffusion_start_image against gct2_rng_normal + gct2_diffusion_mix.
     B = 64, 128 x 128 x 3, bf16 copies into a packed image (ld 4) and a 72-wide concat buffer, predict_x, in place on `fake`, a
     half-plane mask with a blended column.  Events around many launches per sample (a captured HIP graph of LAUNCHES steps, replayed
     REPLAYS times, so the host's enqueue rate stays out of the number), the variants taking turns; median and spread over the samples.
 (b) a 50-step masked generate at batch 64 on the benchmark's network (Topology(128, 512, 6), bf16: BASELINE config 3) against the
     plain generate of the same schedule; events around whole runs, the two taking turns.

    python scripts/bench_img2img.py [OUT.json]
"""
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gan_class_transfer2_amd as g

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
known = (torch.rand(B, H, W, 3, generator=gen) * 2 - 1).to(dev)
start = torch.randn(B, H, W, 3, generator=gen).to(dev)
mask = torch.zeros(B, H, W, device=dev)
mask[:, :, W // 2:] = 1.0
mask[:, :, W // 2 - 1] = 0.5
t = 100
a_t, a_prev = float(g.trainer_math.alpha_dash(t, STEPS)), float(g.trainer_math.alpha_dash(t - 4, STEPS))
s2 = g.ddim_sigma2(a_t, a_prev, 1.0)
SEED, OFF, OFF0 = 7, 8 * n, 0                          # images back to back (image_stride = per_image): one gct2_rng_normal call draws z0

pred_odd = torch.empty(n + 1, device=dev)[1:]          # the same values 4 bytes off a 16-byte boundary: the general form
pred_odd.copy_(pred.reshape(-1))


class Buffers:
    def __init__(self):
        self.fake, self.x0 = start.clone(), torch.empty_like(start)
        self.z0, self.h = torch.empty_like(start), torch.empty_like(start)
        self.img = torch.zeros(B * H * W, 4, dtype=torch.bfloat16, device=dev)
        self.r0 = torch.zeros(B * H * W, 72, dtype=torch.bfloat16, device=dev)
        self.himg, self.hr0 = torch.zeros_like(self.img), torch.zeros_like(self.r0)
        self.views = (self.img.data_ptr(), 4, self.r0.data_ptr() + 2 * 64, 72)
        self.hviews = (self.himg.data_ptr(), 4, self.hr0.data_ptr() + 2 * 64, 72)


def masked(sigma2, odd=False):
    def run(b):
        L.call("gct2_diffusion_step_masked", L.SAMPLE_X, BF16, (pred_odd if odd else pred).data_ptr(), b.fake.data_ptr(), known.data_ptr(),
               mask.data_ptr(), a_t, a_prev, sigma2, 0.0, SEED, g.GENERATE_STREAM, OFF, OFF0, per, b.fake.data_ptr(), b.x0.data_ptr(), *b.views,
               B, per, 3, stream())
    return run


def plain(sigma2):
    def run(b):
        L.call("gct2_diffusion_step", L.SAMPLE_X, BF16, pred.data_ptr(), b.fake.data_ptr(), a_t, a_prev, sigma2, 0.0, SEED, g.GENERATE_STREAM, OFF,
               per, b.fake.data_ptr(), b.x0.data_ptr(), *b.views, B, per, 3, stream())
    return run


def select(m, p, q):
    return torch.where(m >= 1, p, torch.where(m <= 0, q, m * p + (1 - m) * q))


def composed(sigma2):
    step = plain(sigma2)

    def run(b):
        step(b)                                                                    # g in fake (and the views), x in x0
        L.call("gct2_rng_normal", SEED, g.GENERATE_STREAM, OFF0, b.z0.data_ptr(), n, stream())
        L.call("gct2_diffusion_mix", BF16, known.data_ptr(), b.z0.data_ptr(), a_prev, b.h.data_ptr(), *b.hviews, B * H * W, 3, stream())
        m = mask[..., None]
        b.fake.copy_(select(m, b.fake, b.h))
        b.x0.copy_(select(m, b.x0, known))
        v = b.fake.reshape(-1, 3).to(torch.bfloat16)
        b.img[:, :3] = v
        b.r0[:, 64:67] = v
    return run


def start_image(b):
    L.call("gct2_diffusion_start_image", BF16, known.data_ptr(), a_t, SEED, g.GENERATE_STREAM, OFF0, per, b.fake.data_ptr(), *b.views, B, per, 3,
           stream())


def start_pair(b):
    L.call("gct2_rng_normal", SEED, g.GENERATE_STREAM, OFF0, b.z0.data_ptr(), n, stream())
    L.call("gct2_diffusion_mix", BF16, known.data_ptr(), b.z0.data_ptr(), a_t, b.fake.data_ptr(), *b.views, B * H * W, 3, stream())


variants = {"masked_eta0": masked(0.0), "masked_eta1": masked(s2), "masked_eta1_unaligned": masked(s2, odd=True),
            "step_eta0": plain(0.0), "step_eta1": plain(s2), "composed_eta0": composed(0.0), "composed_eta1": composed(s2),
            "start_image": start_image, "rng_normal_then_mix": start_pair}
same = lambda p, q: torch.equal(p.view(torch.int32), q.view(torch.int32))
# one step of each from the same state: the launch and the composition it replaces give the same bits
once = {k: Buffers() for k in variants}
for k, f in variants.items():
    f(once[k])
torch.cuda.synchronize()
for eta in ("eta0", "eta1"):
    p, q = once["masked_" + eta], once["composed_" + eta]
    assert same(p.fake, q.fake) and same(p.x0, q.x0) and torch.equal(p.img, q.img) and torch.equal(p.r0, q.r0), eta
assert same(once["masked_eta1_unaligned"].fake, once["masked_eta1"].fake)
assert same(once["start_image"].fake, once["rng_normal_then_mix"].fake) and torch.equal(once["start_image"].r0, once["rng_normal_then_mix"].r0)
assert bool(torch.isfinite(once["masked_eta1"].fake).all())
del once
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
# bytes the algorithm needs per step: fp32 planes read and written + the mask + the two bf16 copies (3 of 4 / 3 of 72 slots)
copies = B * H * W * 3 * 2 * 2
need = {"masked": n * 4 * 5 + B * H * W * 4 + copies, "step": n * 4 * 4 + copies, "start_image": n * 4 * 2 + copies}
kernels = {}
for k, v in us.items():
    kernels[k] = dict(summary(v), unit="us per step")
    nb = need.get("masked" if k.startswith("masked") else "step" if k.startswith("step") else k)
    if nb:
        kernels[k].update(bytes_per_step=nb, GB_per_s_at_median=round(nb / statistics.median(v) / 1e3, 1))
del graphs, bufs

# ---- (b) a whole generation ------------------------------------------------------------------------------------------------------------
eng = g.UNetEngine(g.Topology(128, 512, 6), BF16, dev)
den = types.SimpleNamespace(ensure_engine=lambda: eng)
runs = {"generate": lambda: g.generate(den, B, num_steps=K, seed=3, batch_size=B, size=(H, W)),
        "generate_init": lambda: g.generate(den, B, num_steps=K, seed=3, batch_size=B, init=known),
        "generate_init_mask": lambda: g.generate(den, B, num_steps=K, seed=3, batch_size=B, init=known, mask=mask)}
outs = {}
for k, f in runs.items():
    for _ in range(2):
        outs[k] = f()
torch.cuda.synchronize()
assert all(bool(torch.isfinite(v).all()) for v in outs.values())
assert torch.equal(outs["generate_init_mask"][:, :, :W // 2 - 1], known[:, :, :W // 2 - 1])
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
out = {"what": f"one MI355X, one process. kernels: B={B} {H}x{W}x3, predict_x, t={t} -> t-4, bf16 copies (ld 4 and ld 72), in place on fake, x0_out "
               "written, a half-plane mask with one blended column, images back to back in the stream (image_stride = per_image, so the "
               f"composition draws z0 in one gct2_rng_normal call); {SAMPLES} samples of {LAUNCHES * REPLAYS} back-to-back steps each (a captured "
               f"graph of {LAUNCHES}, replayed {REPLAYS} times) between two events, the variants taking turns, after 20 warm-up steps of each. "
               "masked_*: gct2_diffusion_step_masked; step_*: gct2_diffusion_step alone (the floor); composed_*: gct2_diffusion_step + "
               "gct2_rng_normal + gct2_diffusion_mix + the torch select / blend of fake' and x0 + the re-store of both bf16 views, bit-identical "
               "to masked_* after one step from the same state; _unaligned: pred 4 bytes off a 16-byte boundary (the general form), the same "
               "bits.  start_image: gct2_diffusion_start_image against gct2_rng_normal + gct2_diffusion_mix, bit-identical. "
               f"generate: {K} steps of {STEPS} at batch {B} on Topology(128, 512, 6) bf16, eta = 0: plain, with init (strength 1), with init and "
               f"the mask; {RUNS} runs each between two events, taking turns, after 2 warm-up runs of each",
       "kernels": kernels,
       "masked_over_composed": {e: round(med("masked_" + e) / med("composed_" + e), 3) for e in ("eta0", "eta1")},
       "masked_minus_step_median_us": {e: round(med("masked_" + e) - med("step_" + e), 3) for e in ("eta0", "eta1")},
       "start_image_over_pair": round(med("start_image") / med("rng_normal_then_mix"), 3),
       "generate": {k: dict(summary(v), unit="ms per run") for k, v in ms.items()}}
out["generate"]["masked_minus_plain_median_ms"] = round(out["generate"]["generate_init_mask"]["median"] - out["generate"]["generate"]["median"], 3)
print(json.dumps(out))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "img2img_bench.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
