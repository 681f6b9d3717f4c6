"""what the parameter averages (Adam(use_ema=True), gct2_ema_update) cost on an MI355X, in one process (diagnostic):
  kernel rate  bytes per second of gct2_ema_update over the config-3 arena beside gct2_adam_keras_multi over the same range (the
               yardstick is Adam on the same box, in alternating rounds - not a number fixed here);
  step cost    config-3 ms per step with the averages off and on, alternating rounds of one engine.
Device events around back-to-back launches, a synchronise behind the last; every timed window lasts about half a second; medians
over the rounds.  --parent-tree DIR: a built checkout of the parent commit; its config-3 step (averages not built there) is timed the
same way in a process of its own on the same box, BEFORE this process takes the GPU.
usage: python scripts/bench_ema.py [output.json] [--parent-tree DIR]      (default output: profiles/ema_bench.json)"""
import json, os, statistics, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gan_class_transfer2_amd as g
from gan_class_transfer2_amd.engine import Topology, UNetEngine, BF16
from gan_class_transfer2_amd.trainer_math import ema_coefficients

argv = sys.argv[1:]
parent_tree = None
if "--parent-tree" in argv:
    k = argv.index("--parent-tree")
    parent_tree = os.path.abspath(argv[k + 1])
    del argv[k:k + 2]
out_path = argv[0] if argv else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ema_bench.json")
ROUNDS = 5
KERNEL_ITERS, STEP_ITERS = 4000, 200          # ~0.1 ms per launch, ~2.5 ms per step: half a second per window

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
    raise SystemExit("bench_ema.py measures on the GPU: no HIP device visible (there is no CPU figure)")
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
        flush()                   # optimizer / EMA launches the last step held back: they belong to the timed work
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # microseconds per call


# ---- kernel rate: tensors of their own, the arena's length, so that nothing of the engine is disturbed -------------------------
f = lambda: torch.randn(N, dtype=torch.float32, device=dev) * 0.05
p, m, v, grad, ema = f(), f() * 0.01, f().square(), f() * 0.01, f()
shadow, ema_shadow = p.to(torch.bfloat16), ema.to(torch.bfloat16)
mom, one_minus = ema_coefficients(0.99)
run_ema = lambda: L.call("gct2_ema_update", ema.data_ptr(), p.data_ptr(), ema_shadow.data_ptr(), BF16, N, mom, one_minus, None, s)
run_adam = lambda: L.call("gct2_adam_keras_multi", p.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), shadow.data_ptr(), BF16, N,
                          1e-8, 0.9, 0.999, 1e-7, 1.0, None, 0, s)
EMA_BYTES, ADAM_BYTES = 14 * N, 30 * N        # ema r/w + p r + shadow w; p, m, v r/w + g r + shadow w
for fn in (run_ema, run_adam):
    for _ in range(5):
        fn()
us_ema, us_adam = [], []
for _ in range(ROUNDS):                        # alternating: both see the same box in the same minute
    us_ema.append(timed(run_ema, KERNEL_ITERS))
    us_adam.append(timed(run_adam, KERNEL_ITERS))
ema_us, adam_us = statistics.median(us_ema), statistics.median(us_adam)
ema_tbs, adam_tbs = EMA_BYTES / ema_us / 1e6, ADAM_BYTES / adam_us / 1e6
print("gct2_ema_update        %7.1f us  %.2f TB/s of %.0f MB   (rounds: %s)" % (ema_us, ema_tbs, EMA_BYTES / 1e6, " ".join("%.1f" % u for u in us_ema)))
print("gct2_adam_keras_multi  %7.1f us  %.2f TB/s of %.0f MB   (rounds: %s)" % (adam_us, adam_tbs, ADAM_BYTES / 1e6, " ".join("%.1f" % u for u in us_adam)))
# the expectation is that EMA streams no slower than Adam does on the same box
slower = ema_tbs < 0.9 * adam_tbs
if slower:
    print("NOTE: gct2_ema_update streams MORE THAN 10 %% slower than gct2_adam_keras_multi (%.2f vs %.2f TB/s): per launch it moves less "
          "than half of Adam's bytes, so the fixed cost of a launch (ramp, drain, the tail block) weighs twice as much" % (ema_tbs, adam_tbs))
del p, m, v, grad, ema, shadow, ema_shadow

# ---- step cost: one engine, the averages switched off / on in alternating rounds (a switch drops the step plans - they bake in the
# averages' addresses, UNetEngine._ema_attach - so every round warms up and records again) ----
x = torch.rand(BATCH, SIZE, SIZE, 3, device=dev) * 2 - 1
step_us = {False: [], True: []}
for _ in range(ROUNDS):
    for on in (False, True):
        eng.enable_ema(0.99) if on else eng.disable_ema()
        for _ in range(6):
            eng.train_step(x)
        step_us[on].append(timed(lambda: eng.train_step(x), STEP_ITERS, eng.flush_deferred))
off_ms, on_ms = statistics.median(step_us[False]) / 1e3, statistics.median(step_us[True]) / 1e3
print("config-3 step, averages off  %.3f ms   (rounds: %s)" % (off_ms, " ".join("%.3f" % (u / 1e3) for u in step_us[False])))
print("config-3 step, averages on   %.3f ms   (rounds: %s)" % (on_ms, " ".join("%.3f" % (u / 1e3) for u in step_us[True])))

res = {
    "device": torch.cuda.get_device_name(0), "arena_elements": N, "kernel_launches_per_round": KERNEL_ITERS, "steps_per_round": STEP_ITERS, "rounds": ROUNDS,
    "kernel": {"ema_us": round(ema_us, 2), "ema_bytes": EMA_BYTES, "ema_tb_per_s": round(ema_tbs, 3), "ema_us_rounds": [round(u, 2) for u in us_ema],
               "adam_us": round(adam_us, 2), "adam_bytes": ADAM_BYTES, "adam_tb_per_s": round(adam_tbs, 3), "adam_us_rounds": [round(u, 2) for u in us_adam],
               "ema_rate_over_adam_rate": round(ema_tbs / adam_tbs, 3), "ema_more_than_10_percent_slower_than_adam": bool(slower)},
    "step": {"config": "3x128x128, batch 64, bf16", "off_ms": round(off_ms, 4), "on_ms": round(on_ms, 4), "on_minus_off_us": round((on_ms - off_ms) * 1e3, 1),
             "off_ms_rounds": [round(u / 1e3, 4) for u in step_us[False]], "on_ms_rounds": [round(u / 1e3, 4) for u in step_us[True]],
             # the parent commit (averages not built), timed the same way in its own process on the same box (--parent-tree); without
             # that option only the range DESIGN.md section 6 records for it over six boxes is known
             "parent_off_ms": round(statistics.median(parent_rounds), 4) if parent_rounds else None,
             "parent_off_ms_rounds": parent_rounds, "parent_off_ms_range_in_design_6": [2.44, 2.52]},
}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", out_path)
