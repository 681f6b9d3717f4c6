"""what a Keras SGD / RMSprop step (gct2_optimizer_apply on the non-fused optimizer path) costs on an MI355X beside the non-fused Adam
step, in one process (diagnostic): config 3 (3x128x128, batch 64, bf16), three engines - Adam with fuse_adam = False (the arena path:
gct2_adam_keras_multi over the whole arena behind the reverse pass; this tree does not touch it, so it is the parent commit's
non-fused step), SGD(0.25, 0.5, True) and RMSprop(1e-3) - each warmed with 20 steps, then rounds of 50 steps per engine, the engines
taking turns inside every round so that all three see the same box in the same second.  Device events around a round, a synchronise
behind it; medians over the rounds.  Also the three optimizer launches alone over the config-3 arena (bytes per second), alternating.
usage: python scripts/bench_optimizers.py [output.json]      (default output: profiles/optimizers_bench.json)"""
import json, os, statistics, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gan_class_transfer2_amd as g
from gan_class_transfer2_amd.engine import Topology, UNetEngine, BF16

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "optimizers_bench.json")
if not torch.cuda.is_available():
    raise SystemExit("bench_optimizers.py measures on the GPU: no HIP device visible (there is no CPU figure)")
L = g._lib
dev = torch.device("cuda", 0)
WARMUP, STEPS, ROUNDS, KERNEL_ITERS = 20, 50, 7, 2000
BATCH, SIZE = 64, 128                                         # config 3


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                # milliseconds per call


OPTIMIZERS = {"adam_non_fused": g.Adam(g.WarmUp(2e-5, 2000)), "sgd_nesterov": g.SGD(0.25, 0.5, True), "rmsprop": g.RMSprop(1e-3)}
x = torch.rand(BATCH, SIZE, SIZE, 3, device=dev) * 2 - 1
engines = {}
for name, opt in OPTIMIZERS.items():
    eng = UNetEngine(Topology(128, 512, 6), BF16, dev)
    g.Trainer(types.SimpleNamespace(engine=eng)).compile(opt, g.identity)
    eng.fuse_adam = False
    for _ in range(WARMUP):
        eng.train_step(x)
    engines[name] = eng
step_ms = {k: [] for k in engines}
for _ in range(ROUNDS):
    for name, eng in engines.items():
        step_ms[name].append(timed(lambda: eng.train_step(x), STEPS))
ms = {k: statistics.median(v) for k, v in step_ms.items()}
for k in engines:
    print("config-3 step, %-16s %.3f ms   (rounds: %s)" % (k, ms[k], " ".join("%.3f" % u for u in step_ms[k])))

# ---- the optimizer launches alone, over tensors of their own of the arena's length ----------------------------------------------------
N = engines["adam_non_fused"].arena.total
s = torch.cuda.current_stream().cuda_stream
f = lambda: torch.randn(N, dtype=torch.float32, device=dev) * 0.05
p, m, v, grad = f(), f() * 0.01, f().square(), f() * 0.01
shadow = p.to(torch.bfloat16)
apply = lambda kind, use_m, use_v, mom, nes: (lambda: L.call("gct2_optimizer_apply", kind, p.data_ptr(), m.data_ptr() if use_m else None,
                                                              v.data_ptr() if use_v else None, grad.data_ptr(), shadow.data_ptr(), BF16, N, 1e-8, mom, nes, 0.9, 1e-7, 1.0,
                                                              None, L.CLIP_NONE, 0.0, None, s))
KERNELS = {  # name: (launch, bytes per parameter: p r/w + g r + shadow w, + 8 per slot in use)
    "adam_keras_multi": (lambda: L.call("gct2_adam_keras_multi", p.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), shadow.data_ptr(), BF16, N,
                                        1e-8, 0.9, 0.999, 1e-7, 1.0, None, 0, s), 30),
    "sgd": (apply(L.OPT_SGD, False, False, 0.0, 0), 14),
    "sgd_nesterov": (apply(L.OPT_SGD, True, False, 0.5, 1), 22),
    "rmsprop": (apply(L.OPT_RMSPROP, False, True, 0.0, 0), 22),
    "rmsprop_momentum": (apply(L.OPT_RMSPROP, True, True, 0.9, 0), 30),
}
for fn, _ in KERNELS.values():
    for _ in range(5):
        fn()
kernel_us = {k: [] for k in KERNELS}
for _ in range(ROUNDS):
    for k, (fn, _) in KERNELS.items():
        kernel_us[k].append(timed(fn, KERNEL_ITERS) * 1e3)
kus = {k: statistics.median(v) for k, v in kernel_us.items()}
for k, (_, bpp) in KERNELS.items():
    print("%-18s %7.1f us  %.2f TB/s of %.0f MB (%d bytes per parameter)" % (k, kus[k], bpp * N / kus[k] / 1e6, bpp * N / 1e6, bpp))

res = {"device": torch.cuda.get_device_name(0), "config": "3x128x128, batch 64, bf16, fuse_adam = False", "warmup_steps": WARMUP, "steps_per_round": STEPS,
       "rounds": ROUNDS, "arena_elements": N,
       "step": {**{k + "_ms": round(ms[k], 4) for k in engines}, **{k + "_ms_rounds": [round(u, 4) for u in step_ms[k]] for k in engines},
                **{k + "_over_adam": round(ms[k] / ms["adam_non_fused"], 4) for k in engines if k != "adam_non_fused"}},
       "kernel": {**{k + "_us": round(kus[k], 2) for k in KERNELS}, **{k + "_bytes_per_parameter": KERNELS[k][1] for k in KERNELS},
                  **{k + "_tb_per_s": round(KERNELS[k][1] * N / kus[k] / 1e6, 3) for k in KERNELS}, "launches_per_round": KERNEL_ITERS}}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", out_path)
