"""what the image metrics of evaluation (Trainer.evaluate(metrics=...), compile(metrics=[...])) cost on an MI355X, in one process
(diagnostic), at the config-3 shape 64x128x128x3: (1) the gct2_image_metrics launch with and without SSIM, and with and without u, v
and noised (the x0 estimate of the non-default objectives), against the MSE gct2_eval_loss_rows launch on the same data - the launches
taking turns inside every round; (2) one config-3 (3x128x128, batch 64, bf16) evaluate_batch with metrics on against the same call
with metrics off, under the default objective and under the epsilon objective (which also forms the fp32 noised image), taking turns.
Device events around a window of calls, medians over the rounds.  Metrics are opt-in: there is no threshold here.
usage: python scripts/bench_metrics.py [output.json]      (default output: profiles/metrics_bench.json)"""
import ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, KERNEL_ITERS, WARMUP, BATCH_ITERS = 7, 500, 20, 50
SHAPE = (64, 128, 128, 3)                                     # config 3

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "metrics_bench.json")
sys.path.insert(0, ROOT)
import torch
import gan_class_transfer2_amd as g

if not torch.cuda.is_available():
    raise SystemExit("bench_metrics.py measures on the GPU: no HIP device visible (there is no CPU figure)")
L = g._lib
dev = torch.device("cuda", 0)
ALL = ("psnr", "ssim", "mse_x0")


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
x = torch.rand(*SHAPE, device=dev) * 2 - 1
pred, noised = x + 0.1 * torch.randn(*SHAPE, device=dev), x + 0.2 * torch.randn(*SHAPE, device=dev)
u, v = torch.rand(B, device=dev) + 0.5, -(torch.rand(B, device=dev) + 0.5)
window = torch.from_numpy(g.trainer_math.ssim_window()).to(dev)
out = torch.zeros(3, B, device=dev)
need, need_eval = ctypes.c_size_t(0), ctypes.c_size_t(0)
L.check(L.load().gct2_image_metrics_scratch(*SHAPE, window.numel(), ctypes.byref(need)), "gct2_image_metrics_scratch")
L.check(L.load().gct2_eval_loss_scratch(L.LOSS_MSE, *SHAPE, ctypes.byref(need_eval)), "gct2_eval_loss_scratch")
scratch, scratch_eval = torch.zeros(need.value, device=dev), torch.zeros(need_eval.value, device=dev)


def metrics_launch(mixed, ssim):
    return lambda: L.call("gct2_image_metrics", pred.data_ptr(), noised.data_ptr() if mixed else None, u.data_ptr() if mixed else None,
                          v.data_ptr() if mixed else None, x.data_ptr(), window.data_ptr(), window.numel(), 2.0, 0.01, 0.03, out[0].data_ptr(),
                          out[1].data_ptr(), out[2].data_ptr() if ssim else None, scratch.data_ptr(), scratch.numel(), *SHAPE, s)


launches = {
    "mse_eval_rows": lambda: L.call("gct2_eval_loss_rows", L.LOSS_MSE, pred.data_ptr(), x.data_ptr(), None, None, None, None, out[0].data_ptr(),
                                    scratch_eval.data_ptr(), scratch_eval.numel(), *SHAPE, None, s),
    "metrics_psnr": metrics_launch(False, False), "metrics_psnr_ssim": metrics_launch(False, True),
    "metrics_psnr_mixed": metrics_launch(True, False), "metrics_psnr_ssim_mixed": metrics_launch(True, True),
}
kernel_ms, kernel_samples = rounds(launches, KERNEL_ITERS)
kernel_us = {k: v * 1e3 for k, v in kernel_ms.items()}
for k, val in kernel_us.items():
    print("%-28s %8.2f us   (rounds: %s)" % (k, val, " ".join("%.2f" % (t * 1e3) for t in kernel_samples[k])))
ratios = {k + "_over_mse_eval_rows": kernel_us[k] / kernel_us["mse_eval_rows"] for k in launches if k != "mse_eval_rows"}

# ---- (2) a config-3 evaluation batch with and without metrics -------------------------------------------------------------------------------
g.configure(compute_dtype="bfloat16")
tr = g.Trainer(g.Denoiser(device=dev))
eng = tr._engine()
xb = torch.rand(*SHAPE, device=dev) * 2 - 1
batch_res = {}
for objective, predict_x in (("default", True), ("epsilon", False)):
    eng.predict_x = predict_x
    batch = {"metrics_off": lambda: eng.evaluate_batch(xb), "psnr": lambda: eng.evaluate_batch(xb, metrics=("psnr",)),
             "psnr_ssim_mse_x0": lambda: eng.evaluate_batch(xb, metrics=ALL)}
    for fn in batch.values():
        for _ in range(WARMUP):
            fn()
    batch_ms, batch_samples = rounds(batch, BATCH_ITERS)
    for k in batch:
        print("config-3 %-8s %-18s %.3f ms   (rounds: %s)" % (objective, k, batch_ms[k], " ".join("%.3f" % t for t in batch_samples[k])))
    batch_res[objective] = {**{k + "_ms": round(val, 4) for k, val in batch_ms.items()},
                            **{k + "_ms_rounds": [round(t, 4) for t in batch_samples[k]] for k in batch},
                            "psnr_over_metrics_off": round(batch_ms["psnr"] / batch_ms["metrics_off"], 4),
                            "psnr_ssim_mse_x0_over_metrics_off": round(batch_ms["psnr_ssim_mse_x0"] / batch_ms["metrics_off"], 4)}

res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "rounds": ROUNDS, "launches_per_round": KERNEL_ITERS,
       "window": "trainer_math.ssim_window(): 11 taps, sigma 1.5", "tile": 32,
       "kernel_us": {k: round(val, 2) for k, val in kernel_us.items()},
       "kernel_us_rounds": {k: [round(t * 1e3, 2) for t in val] for k, val in kernel_samples.items()},
       "kernel_ratio": {k: round(val, 4) for k, val in ratios.items()},
       "batch": {"config": "3x128x128, batch 64, bf16", "warmup_calls": WARMUP, "calls_per_round": BATCH_ITERS, **batch_res}}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", out_path)
