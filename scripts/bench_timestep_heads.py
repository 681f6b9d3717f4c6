"""what the per-timestep heads (train.py:199, 203, 211-214; UNetEngine(timestep_heads=True)) cost on an MI355X, in one process
(diagnostic): train steps of the default bench configuration (3x128x128, batch 64, bf16) on three engines taking turns inside every
round - the default fused step (switch off), the unfused plain head (use_fused_head = False: what leaving UpShuffle_0's epilogue costs
by itself) and the switch on - each warmed with 20 steps, then rounds of 50 steps, device events around a round, medians over the rounds;
plus the two new launches alone at that shape.
usage: python scripts/bench_timestep_heads.py [output.json]      (default output: profiles/timestep_heads_bench.json)"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS, ROUNDS, KERNEL_ITERS = 20, 50, 7, 100
BATCH, SIZE, NSTEPS = 64, 128, 200

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "timestep_heads_bench.json")
sys.path.insert(0, ROOT)
import torch
import gan_class_transfer2_amd as g
from gan_class_transfer2_amd.engine import Topology, UNetEngine, BF16

if not torch.cuda.is_available():
    raise SystemExit("bench_timestep_heads.py measures on the GPU: no HIP device visible (there is no CPU figure)")
dev = torch.device("cuda", 0)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                # milliseconds per call


x = torch.rand(BATCH, SIZE, SIZE, 3, device=dev) * 2 - 1
engines = {}
for name in ("off", "off_unfused_head", "on"):
    eng = UNetEngine(Topology(128, 512, 6), BF16, dev, steps=NSTEPS, timestep_heads=(name == "on"))
    if name == "off_unfused_head":
        eng.use_fused_head = False
    for _ in range(WARMUP):
        eng.train_step(x)
    engines[name] = eng
torch.cuda.synchronize()
step_ms = {k: [] for k in engines}
for _ in range(ROUNDS):
    for name, eng in engines.items():
        step_ms[name].append(timed(lambda: eng.train_step(x), STEPS))
ms = {k: statistics.median(v) for k, v in step_ms.items()}
for k in step_ms:
    print("step, timestep_heads %-18s %.3f ms   (rounds: %s)" % (k, ms[k], " ".join("%.3f" % u for u in step_ms[k])))

# the two launches alone, on the switched-on engine's own buffers (R_0, dpred, t_int as the last step left them)
eng = engines["on"]
b, A, t = eng.buffers(BATCH, SIZE, SIZE), eng.arena, eng.topo
s = torch.cuda.current_stream().cuda_stream
scratch = eng._steps_scratch(b.loss_store, BATCH, SIZE * SIZE, t.fu(0) + 3)
dw, db, dx = torch.zeros_like(A.grad("dense.w")), torch.zeros_like(A.grad("dense.b")), torch.zeros_like(b.dR[0])
launches = {
    "dense_steps_fwd": lambda: g._lib.call("gct2_dense_steps_fwd", None, eng.dtype, b.R[0].data_ptr(), b.ld[0], A.pptr("dense.w"), A.pptr("dense.b"),
                                           b.t_int.data_ptr(), b.pred.data_ptr(), BATCH, SIZE * SIZE, t.fu(0) + 3, 3, NSTEPS, s),
    "dense_steps_bwd": lambda: g._lib.call("gct2_dense_steps_bwd", None, eng.dtype, b.R[0].data_ptr(), b.ld[0], A.pptr("dense.w"), b.t_int.data_ptr(),
                                           b.dpred.data_ptr(), dx.data_ptr(), b.ldd[0], dw.data_ptr(), db.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                           BATCH, SIZE * SIZE, t.fu(0) + 3, 3, NSTEPS, t.fu(0), 0, s),
}
kernel_us = {}
for k, fn in launches.items():
    for _ in range(3):
        fn()
    kernel_us[k] = statistics.median(timed(fn, KERNEL_ITERS) * 1e3 for _ in range(ROUNDS))
    print("%-18s %8.1f us" % (k, kernel_us[k]))

res = {"device": torch.cuda.get_device_name(0), "config": "3x128x128, batch 64, bf16, steps 200", "warmup_steps": WARMUP, "steps_per_round": STEPS,
       "rounds": ROUNDS,
       "step": {**{k + "_ms": round(ms[k], 4) for k in step_ms}, **{k + "_ms_rounds": [round(u, 4) for u in step_ms[k]] for k in step_ms},
                "on_over_off": round(ms["on"] / ms["off"], 4), "on_over_off_unfused_head": round(ms["on"] / ms["off_unfused_head"], 4)},
       "kernel_us": {k: round(v, 2) for k, v in kernel_us.items()}, "launches_per_round": KERNEL_ITERS}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", out_path)
