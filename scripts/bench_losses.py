"""what the training losses besides the plain MSE (train.py:254-280; gct2_loss_fwd_bwd: "l1", "mse_pooled", "dct") cost on an MI355X, in
one process (diagnostic): (1) the launches of each kind alone at the config-3 (64x128x128x3) and config-5 (16x256x256x3) shapes, with
and without the gradient, the kinds taking turns; (2) config 3 (3x128x128, batch 64, bf16) train steps of five engines taking turns
inside every round - the default fused step, the unfused-head MSE step (use_fused_head = False: what the other kinds pay for leaving
UpShuffle_0's epilogue) and one engine per kind - each warmed with 20 steps, then rounds of 50 steps, device events around a round,
medians over the rounds; (3) with --parent DIR (a built checkout of the parent commit) that tree's default step, timed by a child
process that takes its turn in the same rounds on the same box.
usage: python scripts/bench_losses.py [--parent DIR] [output.json]      (default output: profiles/losses_bench.json)"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS, ROUNDS, KERNEL_ITERS = 20, 50, 7, 200
BATCH, SIZE = 64, 128                                         # config 3


def timed(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                # milliseconds per call


def default_step_server(tree):
    """child process: the default config-3 step of the package in `tree`; one line "go" in, one line of milliseconds per step out"""
    sys.path.insert(0, tree)
    import torch
    from gan_class_transfer2_amd.engine import Topology, UNetEngine, BF16
    dev = torch.device("cuda", 0)
    eng = UNetEngine(Topology(128, 512, 6), BF16, dev)
    x = torch.rand(BATCH, SIZE, SIZE, 3, device=dev) * 2 - 1
    for _ in range(WARMUP):
        eng.train_step(x)
    torch.cuda.synchronize()
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print("%.6f" % timed(lambda: eng.train_step(x), STEPS), flush=True)


if len(sys.argv) > 2 and sys.argv[1] == "--serve":
    default_step_server(sys.argv[2])
    raise SystemExit(0)

argv = sys.argv[1:]
parent = None
if argv and argv[0] == "--parent":
    parent, argv = os.path.abspath(argv[1]), argv[2:]
out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "losses_bench.json")
sys.path.insert(0, ROOT)
import torch
import gan_class_transfer2_amd as g
from gan_class_transfer2_amd.engine import Topology, UNetEngine, BF16

if not torch.cuda.is_available():
    raise SystemExit("bench_losses.py measures on the GPU: no HIP device visible (there is no CPU figure)")
L = g._lib
dev = torch.device("cuda", 0)
KINDS = {"mse": L.LOSS_MSE, "l1": L.LOSS_L1, "mse_pooled": L.LOSS_MSE_POOLED, "dct": L.LOSS_DCT}

# ---- (1) the launches alone ---------------------------------------------------------------------------------------------------------------
import ctypes
s = torch.cuda.current_stream().cuda_stream
kernel_us = {}
for tag, shape in (("config3", (64, 128, 128, 3)), ("config5", (16, 256, 256, 3))):
    pred, target = torch.randn(*shape, device=dev), torch.randn(*shape, device=dev)
    dpred, loss = torch.empty_like(pred), torch.zeros(1, device=dev)
    basis = torch.from_numpy(g.trainer_math.dct_basis(shape[1])).to(dev)
    launches = {}
    for name, code in KINDS.items():
        need = ctypes.c_size_t(0)
        L.check(L.load().gct2_loss_scratch(code, *shape, ctypes.byref(need)), "gct2_loss_scratch")
        scratch = torch.zeros(need.value, device=dev)
        for grad in (True, False):
            launches[f"{tag}_{name}_{'fwd_bwd' if grad else 'loss_only'}"] = (
                lambda code=code, scratch=scratch, grad=grad: L.call("gct2_loss_fwd_bwd", code, pred.data_ptr(), target.data_ptr(), dpred.data_ptr() if grad else None,
                                                                     loss.data_ptr(), scratch.data_ptr(), scratch.numel(), *shape, basis.data_ptr(), None, s))
    for fn in launches.values():
        for _ in range(3):
            fn()
    samples = {k: [] for k in launches}
    for _ in range(ROUNDS):
        for k, fn in launches.items():
            samples[k].append(timed(fn, KERNEL_ITERS) * 1e3)
    for k, v in samples.items():
        kernel_us[k] = statistics.median(v)
        print("%-36s %8.1f us" % (k, kernel_us[k]))

# ---- (2), (3) config-3 steps, the engines taking turns ------------------------------------------------------------------------------------
x = torch.rand(BATCH, SIZE, SIZE, 3, device=dev) * 2 - 1
engines = {}
for name in ("mse_fused_head", "mse_unfused_head", "l1", "mse_pooled", "dct"):
    eng = UNetEngine(Topology(128, 512, 6), BF16, dev)
    if name == "mse_unfused_head":
        eng.use_fused_head = False
    elif name != "mse_fused_head":
        eng.training_loss = name
    for _ in range(WARMUP):
        eng.train_step(x)
    engines[name] = eng
torch.cuda.synchronize()
child = None
if parent:
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", parent], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    assert child.stdout.readline().strip() == "ready"
step_ms = {k: [] for k in list(engines) + (["parent_default"] if child else [])}
for _ in range(ROUNDS):
    for name, eng in engines.items():
        step_ms[name].append(timed(lambda: eng.train_step(x), STEPS))
    if child:
        child.stdin.write("go\n"); child.stdin.flush()
        step_ms["parent_default"].append(float(child.stdout.readline()))
if child:
    child.stdin.close()
    child.wait(timeout=60)
ms = {k: statistics.median(v) for k, v in step_ms.items()}
for k in step_ms:
    print("config-3 step, %-18s %.3f ms   (rounds: %s)" % (k, ms[k], " ".join("%.3f" % u for u in step_ms[k])))

res = {"device": torch.cuda.get_device_name(0), "config": "3x128x128, batch 64, bf16", "warmup_steps": WARMUP, "steps_per_round": STEPS, "rounds": ROUNDS,
       "step": {**{k + "_ms": round(ms[k], 4) for k in step_ms}, **{k + "_ms_rounds": [round(u, 4) for u in step_ms[k]] for k in step_ms},
                **{k + "_over_unfused_mse": round(ms[k] / ms["mse_unfused_head"], 4) for k in ("l1", "mse_pooled", "dct")}},
       "kernel_us": {k: round(v, 2) for k, v in kernel_us.items()}, "launches_per_round": KERNEL_ITERS}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", out_path)
