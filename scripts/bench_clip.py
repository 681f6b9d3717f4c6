"""what gradient clipping (Adam(clipnorm / global_clipnorm / clipvalue): gct2_grad_sumsq, gct2_adam_keras_clipped) costs on an MI355X,
in one process (diagnostic):
  kernel rate  bytes per second of gct2_grad_sumsq over the config-3 gradient arena (one segment per parameter tensor, as the engine
               lays it out) beside gct2_adam_keras_multi over the same arena, in alternating rounds - the yardstick is Adam on the
               same box, not a number fixed here.  It answers whether the fp64 adds keep the reduction HBM-bound;
  step cost    config-3 ms per step with clipping off, global_clipnorm, clipnorm and clipvalue, interleaved rounds of one engine.
               A clipped step gives up the fused / deferred per-layer Adam launches for the arena path: that, not the reduction, is
               the larger part of the difference.
Device events around back-to-back launches, a synchronise behind the last; every timed window lasts about half a second; medians
over the rounds.  --parent-tree DIR: a built checkout of the parent commit; its config-3 step (no clipping there) is timed the same way
in a process of its own on the same box, BEFORE this process takes the GPU: the "off" leg must not be slower than it.
usage: python scripts/bench_clip.py [output.json] [--parent-tree DIR]      (default output: profiles/clip_bench.json)"""
import json, os, statistics, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gan_class_transfer2_amd as g
from gan_class_transfer2_amd.engine import Topology, UNetEngine, BF16

argv = sys.argv[1:]
parent_tree = None
if "--parent-tree" in argv:
    k = argv.index("--parent-tree")
    parent_tree = os.path.abspath(argv[k + 1])
    del argv[k:k + 2]
out_path = argv[0] if argv else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "clip_bench.json")
ROUNDS = 5
KERNEL_ITERS, STEP_ITERS = 4000, 200          # ~0.03-0.2 ms per launch, ~2.5 ms per step: up to half a second per window

# the step loop of the "step cost" leg as a program of its own, for a tree that has no such script (the parent commit)
PARENT_SNIPPET = """
import statistics, sys, torch
sys.path.insert(0, sys.argv[1])
from gan_class_transfer2_amd.engine import Topology, UNetEngine, BF16
dev = torch.device("cuda", 0)
eng = UNetEngine(Topology(128, 512, 6), BF16, dev)
x = torch.rand(64, 128, 128, 3, device=dev) * 2 - 1
for _ in range(6):
    eng.train_step(x)
res = []
for _ in range(int(sys.argv[2])):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(int(sys.argv[3])):
        eng.train_step(x)
    eng.flush_deferred()
    e1.record()
    torch.cuda.synchronize()
    res.append(e0.elapsed_time(e1) / int(sys.argv[3]))
print("PARENT_MS", " ".join("%.4f" % r for r in res))
"""
parent_rounds = None
if parent_tree is not None:
    r = subprocess.run([sys.executable, "-c", PARENT_SNIPPET, parent_tree, str(ROUNDS), str(STEP_ITERS)], capture_output=True, text=True,
                       cwd=parent_tree, timeout=300)
    if r.returncode != 0:
        raise SystemExit("the parent tree's step could not be timed:\n" + r.stderr[-2000:])
    parent_rounds = [float(v) for v in [l for l in r.stdout.splitlines() if l.startswith("PARENT_MS")][-1].split()[1:]]
    print("config-3 step, parent commit  %.3f ms   (own process, same box; rounds: %s)" % (statistics.median(parent_rounds), " ".join("%.3f" % v for v in parent_rounds)))
L = g._lib
dev = torch.device("cuda", 0)
if not torch.cuda.is_available():
    raise SystemExit("bench_clip.py measures on the GPU: no HIP device visible (there is no CPU figure)")
BATCH, SIZE = 64, 128                                         # config 3
eng = UNetEngine(Topology(128, 512, 6), BF16, dev)
N = eng.arena.total
s = torch.cuda.current_stream().cuda_stream


def timed(fn, n, flush=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    if flush is not None:
        flush()                   # optimizer launches the last step held back: they belong to the timed work
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # microseconds per call


# ---- kernel rate: tensors of their own, the arena's length and the engine's segment table, so that nothing of the engine is disturbed --
f = lambda: torch.randn(N, dtype=torch.float32, device=dev) * 0.05
p, m, v, grad = f(), f() * 0.01, f().square(), f() * 0.01
shadow = p.to(torch.bfloat16)
table, nseg, npartials, partials, sumsq, segs = eng._clip_reduction()
covered = sum(c for _, c in segs)
run_sumsq = lambda: L.call("gct2_grad_sumsq", grad.data_ptr(), table.data_ptr(), nseg, npartials, 1.0, None, partials.data_ptr(), sumsq.data_ptr(), s)
run_adam = lambda: L.call("gct2_adam_keras_multi", p.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), shadow.data_ptr(), BF16, N,
                          1e-8, 0.9, 0.999, 1e-7, 1.0, None, 0, s)
SUMSQ_BYTES, ADAM_BYTES = 4 * covered + 16 * npartials, 30 * N     # g r + partials w/r; p, m, v r/w + g r + shadow w
for fn in (run_sumsq, run_adam):
    for _ in range(5):
        fn()
us_sumsq, us_adam = [], []
for _ in range(ROUNDS):                        # alternating: both see the same box in the same minute
    us_sumsq.append(timed(run_sumsq, KERNEL_ITERS))
    us_adam.append(timed(run_adam, KERNEL_ITERS))
sumsq_us, adam_us = statistics.median(us_sumsq), statistics.median(us_adam)
sumsq_tbs, adam_tbs = SUMSQ_BYTES / sumsq_us / 1e6, ADAM_BYTES / adam_us / 1e6
print("gct2_grad_sumsq        %7.1f us  %.2f TB/s of %.0f MB, %d segments, %d partials   (rounds: %s)"
      % (sumsq_us, sumsq_tbs, SUMSQ_BYTES / 1e6, nseg, npartials, " ".join("%.1f" % u for u in us_sumsq)))
print("gct2_adam_keras_multi  %7.1f us  %.2f TB/s of %.0f MB   (rounds: %s)" % (adam_us, adam_tbs, ADAM_BYTES / 1e6, " ".join("%.1f" % u for u in us_adam)))
slower = sumsq_tbs < 0.9 * adam_tbs
if slower:
    print("NOTE: gct2_grad_sumsq streams MORE THAN 10 %% slower than gct2_adam_keras_multi (%.2f vs %.2f TB/s): it moves less than a "
          "sixth of Adam's bytes in two launches, so the fixed cost of a launch and the serial second stage weigh more" % (sumsq_tbs, adam_tbs))
del p, m, v, grad, shadow

# ---- step cost: one engine, the four settings interleaved (each has its own step plans: the setting is part of their key) ----------
x = torch.rand(BATCH, SIZE, SIZE, 3, device=dev) * 2 - 1
SETTINGS = {"off": {}, "global_clipnorm": dict(global_clipnorm=1.0), "clipnorm": dict(clipnorm=1.0), "clipvalue": dict(clipvalue=0.01)}
step_us = {k: [] for k in SETTINGS}
for _ in range(ROUNDS):
    for name, kw in SETTINGS.items():
        eng.set_clipping(**kw)
        for _ in range(6):
            eng.train_step(x)
        step_us[name].append(timed(lambda: eng.train_step(x), STEP_ITERS, eng.flush_deferred))
ms = {k: statistics.median(vs) / 1e3 for k, vs in step_us.items()}
for k in SETTINGS:
    print("config-3 step, %-16s %.3f ms   (rounds: %s)" % (k, ms[k], " ".join("%.3f" % (u / 1e3) for u in step_us[k])))

res = {
    "device": torch.cuda.get_device_name(0), "arena_elements": N, "segment_elements": covered, "segments": nseg, "partials": npartials,
    "kernel_launches_per_round": KERNEL_ITERS, "steps_per_round": STEP_ITERS, "rounds": ROUNDS,
    "kernel": {"sumsq_us": round(sumsq_us, 2), "sumsq_bytes": SUMSQ_BYTES, "sumsq_tb_per_s": round(sumsq_tbs, 3), "sumsq_us_rounds": [round(u, 2) for u in us_sumsq],
               "adam_us": round(adam_us, 2), "adam_bytes": ADAM_BYTES, "adam_tb_per_s": round(adam_tbs, 3), "adam_us_rounds": [round(u, 2) for u in us_adam],
               "sumsq_rate_over_adam_rate": round(sumsq_tbs / adam_tbs, 3), "sumsq_more_than_10_percent_slower_than_adam": bool(slower)},
    "step": {"config": "3x128x128, batch 64, bf16",
             **{k + "_ms": round(ms[k], 4) for k in SETTINGS}, **{k + "_ms_rounds": [round(u / 1e3, 4) for u in step_us[k]] for k in SETTINGS},
             **{k + "_minus_off_us": round((ms[k] - ms["off"]) * 1e3, 1) for k in SETTINGS if k != "off"},
             # the parent commit (clipping not built), timed the same way in its own process on the same box (--parent-tree); without
             # that option only the range DESIGN.md section 6 records for it over six boxes is known
             "parent_off_ms": round(statistics.median(parent_rounds), 4) if parent_rounds else None,
             "parent_off_ms_rounds": parent_rounds, "parent_off_ms_range_in_design_6": [2.44, 2.52]},
}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", out_path)
