"""time gct2_noise_image_rng (the formula launch, the yardstick) against gct2_noise_image_rng_table (the table launch) in one process at
the benchmark's shape - B = 64, 128 x 128 x 3, bf16, the four-pixel fast path - and write profiles/noise_schedule_bench.json.
Warm-up, then events around many launches per sample (a captured HIP graph of LAUNCHES launches, replayed REPLAYS times, so the host's
enqueue rate stays out of the number), the two launches alternating; median and spread over the samples.

    python scripts/bench_noise_schedule.py [OUT.json]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import gan_class_transfer2_amd as g

L = g._lib
dev = torch.device("cuda", 0)
B, H, W, STEPS, BF16 = 64, 128, 128, 200, 1
LAUNCHES, REPLAYS, SAMPLES = 200, 10, 15
stream = lambda: torch.cuda.current_stream().cuda_stream
x = torch.rand(B, H, W, 3, device=dev) * 2 - 1
t = torch.randint(1, STEPS + 1, (B,), dtype=torch.int32, device=dev)
img_f, img_t = (torch.zeros(B * H * W, 4, dtype=torch.bfloat16, device=dev) for _ in range(2))
# the quadratic schedule as bf16's formula kernel forms it (t as a product): both launches then compute the same image
tt = np.arange(1, STEPS + 1, dtype=np.float32) * (np.float32(1.0) / np.float32(STEPS + 1))
a = ((np.float32(1) - tt) * (np.float32(1) - tt)) * np.float32(0.25)
coef = torch.from_numpy(np.stack([np.sqrt(a), np.sqrt(np.float32(1) - a)], 1).astype(np.float32)).to(dev)

formula = lambda: L.call("gct2_noise_image_rng", BF16, x.data_ptr(), t.data_ptr(), 1, 2, 12288, None, img_f.data_ptr(), 4, None, 0,
                         B, H * W, 3, STEPS, stream())
table = lambda: L.call("gct2_noise_image_rng_table", BF16, x.data_ptr(), t.data_ptr(), 1, 2, 12288, None, coef.data_ptr(), img_t.data_ptr(), 4,
                       None, 0, B, H * W, 3, STEPS, stream())


def graph_of(f):
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(LAUNCHES):
            f()
    return gr


def sample(gr):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (LAUNCHES * REPLAYS)


for f in (formula, table):
    for _ in range(50):
        f()
torch.cuda.synchronize()
assert torch.equal(img_f.view(torch.int16), img_t.view(torch.int16)) and bool((img_f[:, 3] == 0).all()) and bool(img_f[:, :3].abs().sum() > 0)
graphs = {"formula": graph_of(formula), "table": graph_of(table)}
for gr in graphs.values():
    gr.replay()
torch.cuda.synchronize()
us = {"formula": [], "table": []}
for _ in range(SAMPLES):
    for k in us:
        us[k].append(sample(graphs[k]))
bytes_moved = B * H * W * (12 + 8)
out = {"what": f"gct2_noise_image_rng against gct2_noise_image_rng_table on one MI355X, one process, B={B} {H}x{W}x3 bf16, the four-pixel fast "
               f"path (ldout 4, no out2, no eps_out, offset 12288); {SAMPLES} samples of {LAUNCHES * REPLAYS} back-to-back launches each (a captured graph of {LAUNCHES}, replayed "
               f"{REPLAYS} times) between two events, the two launches alternating, after 50 warm-up launches of each; outputs bit-identical (quadratic table, product form)",
       "bytes_per_launch": bytes_moved}
for k, v in us.items():
    out[k] = {"us_per_launch_samples": [round(u, 3) for u in v], "median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3),
              "max_us": round(max(v), 3), "spread_us": round(max(v) - min(v), 3), "GB_per_s_at_median": round(bytes_moved / statistics.median(v) / 1e3, 1)}
out["table_minus_formula_median_us"] = round(out["table"]["median_us"] - out["formula"]["median_us"], 3)
print(json.dumps(out))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "noise_schedule_bench.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
