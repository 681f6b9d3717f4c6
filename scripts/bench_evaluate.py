"""what evaluation (Trainer.evaluate / fit(validation_data=...)) costs on an MI355X, in one process (diagnostic), at the config-3 shape
64x128x128x3: (1) the gct2_eval_loss_rows launches of each kind (no coefficients: the default objective; and with a, c, eps and w: the
weighted epsilon objective) against the loss-only gct2_loss_fwd_bwd launches of the same kind on the same data - gct2_mse_fwd_bwd
for the MSE, which has no loss-only form and writes the gradient tensor - the launches taking turns inside every round; (2) one
config-3 (3x128x128, batch 64, bf16) evaluate_batch against Trainer.call on the same batch, taking turns.  Device events around a
window of calls, medians over the rounds.
usage: python scripts/bench_evaluate.py [output.json]      (default output: profiles/evaluate_bench.json)"""
import ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, KERNEL_ITERS, WARMUP, BATCH_ITERS = 7, 1000, 20, 50
SHAPE = (64, 128, 128, 3)                                     # config 3

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "evaluate_bench.json")
sys.path.insert(0, ROOT)
import torch
import gan_class_transfer2_amd as g

if not torch.cuda.is_available():
    raise SystemExit("bench_evaluate.py measures on the GPU: no HIP device visible (there is no CPU figure)")
L = g._lib
dev = torch.device("cuda", 0)
KINDS = {"mse": L.LOSS_MSE, "l1": L.LOSS_L1, "mse_pooled": L.LOSS_MSE_POOLED, "dct": L.LOSS_DCT}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                # milliseconds per call


def rounds(fns, n):
    """medians (and the samples) of the calls of `fns`, which take turns inside every round"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    samples = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            samples[k].append(timed(fn, n))
    return {k: statistics.median(v) for k, v in samples.items()}, samples


# ---- (1) the launches alone ---------------------------------------------------------------------------------------------------------------
s = torch.cuda.current_stream().cuda_stream
B = SHAPE[0]
pred, x, eps = (torch.randn(*SHAPE, device=dev) for _ in range(3))
dpred, loss, rows = torch.empty_like(pred), torch.zeros(1, device=dev), torch.zeros(B, device=dev)
a, c, w = (torch.rand(B, device=dev) + 0.5 for _ in range(3))
basis = torch.from_numpy(g.trainer_math.dct_basis(SHAPE[1])).to(dev)
launches = {}
for name, code in KINDS.items():
    need, need_eval = ctypes.c_size_t(0), ctypes.c_size_t(0)
    L.check(L.load().gct2_loss_scratch(code, *SHAPE, ctypes.byref(need)), "gct2_loss_scratch")
    L.check(L.load().gct2_eval_loss_scratch(code, *SHAPE, ctypes.byref(need_eval)), "gct2_eval_loss_scratch")
    scratch, scratch_eval = torch.zeros(need.value, device=dev), torch.zeros(need_eval.value, device=dev)
    if name == "mse":
        launches["mse_fwd_bwd"] = lambda scratch=scratch: L.call("gct2_mse_fwd_bwd", pred.data_ptr(), x.data_ptr(), dpred.data_ptr(), loss.data_ptr(),
                                                                 scratch.data_ptr(), pred.numel(), None, s)
    else:
        launches[name + "_loss_only"] = lambda code=code, scratch=scratch: L.call(
            "gct2_loss_fwd_bwd", code, pred.data_ptr(), x.data_ptr(), None, loss.data_ptr(), scratch.data_ptr(), scratch.numel(), *SHAPE,
            basis.data_ptr(), None, s)
    launches[name + "_eval_rows"] = lambda code=code, scratch=scratch_eval: L.call(
        "gct2_eval_loss_rows", code, pred.data_ptr(), x.data_ptr(), None, None, None, None, rows.data_ptr(), scratch.data_ptr(), scratch.numel(),
        *SHAPE, basis.data_ptr(), s)
    launches[name + "_eval_rows_weighted_epsilon"] = lambda code=code, scratch=scratch_eval: L.call(
        "gct2_eval_loss_rows", code, pred.data_ptr(), x.data_ptr(), eps.data_ptr(), a.data_ptr(), c.data_ptr(), w.data_ptr(), rows.data_ptr(),
        scratch.data_ptr(), scratch.numel(), *SHAPE, basis.data_ptr(), s)
kernel_ms, kernel_samples = rounds(launches, KERNEL_ITERS)
kernel_us = {k: v * 1e3 for k, v in kernel_ms.items()}
for k, v in kernel_us.items():
    print("%-40s %8.2f us   (rounds: %s)" % (k, v, " ".join("%.2f" % (u * 1e3) for u in kernel_samples[k])))
baseline = {"mse": "mse_fwd_bwd", "l1": "l1_loss_only", "mse_pooled": "mse_pooled_loss_only", "dct": "dct_loss_only"}
ratios = {k + "_eval_rows_over_" + baseline[k]: kernel_us[k + "_eval_rows"] / kernel_us[baseline[k]] for k in KINDS}

# ---- (2) a config-3 evaluation batch against Trainer.call --------------------------------------------------------------------------------
g.configure(compute_dtype="bfloat16")
tr = g.Trainer(g.Denoiser(device=dev))
eng = tr._engine()
xb = torch.rand(*SHAPE, device=dev) * 2 - 1
batch = {"trainer_call": lambda: tr(xb), "evaluate_batch": lambda: eng.evaluate_batch(xb)}
for fn in batch.values():
    for _ in range(WARMUP):
        fn()
batch_ms, batch_samples = rounds(batch, BATCH_ITERS)
for k in batch:
    print("config-3 %-16s %.3f ms   (rounds: %s)" % (k, batch_ms[k], " ".join("%.3f" % u for u in batch_samples[k])))

res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "rounds": ROUNDS, "launches_per_round": KERNEL_ITERS,
       "kernel_us": {k: round(v, 2) for k, v in kernel_us.items()},
       "kernel_us_rounds": {k: [round(u * 1e3, 2) for u in v] for k, v in kernel_samples.items()},
       "kernel_ratio": {k: round(v, 4) for k, v in ratios.items()},
       "batch": {"config": "3x128x128, batch 64, bf16", "warmup_calls": WARMUP, "calls_per_round": BATCH_ITERS,
                 **{k + "_ms": round(v, 4) for k, v in batch_ms.items()}, **{k + "_ms_rounds": [round(u, 4) for u in batch_samples[k]] for k in batch},
                 "evaluate_batch_over_trainer_call": round(batch_ms["evaluate_batch"] / batch_ms["trainer_call"], 4)}}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", out_path)
