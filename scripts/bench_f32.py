#!/usr/bin/env python3
"""Train-step time of the fp32 engine on the matrix cores (UNetEngine(f32_matrix=True)): the reference's default precision
(train.py:34,38) at BASELINE config 3 (3x128x128, bs 64) and at the reference's own defaults (train.py:17,23: 3x256x256, bs 1).

    python scripts/bench_f32.py --steps 20 --warmup 5 [--direct-steps N [--direct-config3]]
    python scripts/bench_f32.py --steps 20 --warmup 5 --variant block_depth=1 [--direct-steps N]

Replayed steps (step plans, the engine's default), timed with device events around the K steps.  One JSON line per config:
ms/step, images/s, TFLOP/s (bench.f_train_per_image) and the fraction of the 157.3 TF fp32 peak.  --direct-steps N also times N
steps of the direct-kernel engine (the default fp32 path) in the same process: config 2 (3x64x64, bs 32), and config 3 with
--direct-config3.

--variant k=v[,k=v]: a topology variant of train.py:20,26,27 (block_depth, residual, concat) on VariantEngine at the reference's
widths (pixel_size 128, max_size 512, octaves 6), fp32 with f32_matrix on (and off) in the same process, at config 2 and at the
reference's defaults (3x256x256, bs 1); the direct-kernel runs (f32_matrix off) with --direct-steps N: N timed steps after one warm-up.
ms/step and images/s only: bench.f_train_per_image counts the default topology.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import f_train_per_image  # noqa: E402

F32_PEAK = 157.3e12          # fp32 MFMA = fp32 vector peak, MI355X


def time_steps(f32_matrix, size, batch, steps, warmup, dev):
    import gan_class_transfer2_amd as g
    topo = g.Topology(128, 512, 6)                                   # reference defaults, train.py:18-21
    eng = g.UNetEngine(topo, g.F32, dev, f32_matrix=f32_matrix)
    gen = torch.Generator().manual_seed(0)
    x = (torch.randint(0, 256, (batch, size, size, 3), generator=gen).float() / 128 - 1).to(dev)
    for _ in range(warmup):
        eng.train_step(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = eng.train_step(x)
    eng.flush_deferred()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    flops = f_train_per_image(topo, size, size) * batch
    out = dict(path="f32_matrix" if f32_matrix else "direct", size=size, batch=batch, steps=steps, warmup=warmup,
               ms_per_step=round(ms, 4), images_per_s=round(batch / ms * 1e3, 2), tflops=round(flops / ms / 1e9, 2),
               peak_frac=round(flops / ms / 1e-3 / F32_PEAK, 4), gflop_per_step=round(flops / 1e9, 1), loss=float(loss[0]))
    del eng
    torch.cuda.empty_cache()
    return out


def time_variant_steps(variant, f32_matrix, size, batch, steps, warmup, dev):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.variants import VariantEngine
    eng = VariantEngine(128, 512, 6, variant.get("block_depth", 0), variant.get("residual", False), variant.get("concat", True),
                        g.F32, dev, f32_matrix=f32_matrix)                 # reference widths, train.py:18-21
    gen = torch.Generator().manual_seed(0)
    x = (torch.randint(0, 256, (batch, size, size, 3), generator=gen).float() / 128 - 1).to(dev)
    for _ in range(warmup):
        eng.train_step(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = eng.train_step(x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    out = dict(path="f32_matrix" if f32_matrix else "direct", variant=variant, size=size, batch=batch, steps=steps, warmup=warmup,
               ms_per_step=round(ms, 4), images_per_s=round(batch / ms * 1e3, 2), loss=float(loss[0]))
    del eng
    torch.cuda.empty_cache()
    return out


def parse_variant(text):
    """block_depth=1,residual=true -> {"block_depth": 1, "residual": True}"""
    out = {}
    for item in text.split(","):
        k, v = item.split("=")
        if k not in ("block_depth", "residual", "concat"):
            raise SystemExit(f"bench_f32.py: --variant takes block_depth, residual, concat (got {k})")
        out[k] = int(v) if k == "block_depth" else v.lower() in ("1", "true", "yes")
    if not (out.get("block_depth", 0) or out.get("residual", False) or not out.get("concat", True)):
        raise SystemExit("bench_f32.py: --variant must leave the default topology")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--direct-steps", type=int, default=0)
    ap.add_argument("--direct-config3", action="store_true", help="with --direct-steps: time config 3 on the direct kernels too")
    ap.add_argument("--variant", help="k=v[,k=v] of block_depth / residual / concat: time VariantEngine instead (see above)")
    ap.add_argument("--out", help="also append the lines to this file")
    args = ap.parse_args()
    if args.steps < 20 or args.warmup < 5:
        raise SystemExit("bench_f32.py: at least 5 warm-up and 20 timed steps")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.variant:
        variant = parse_variant(args.variant)
        lines = []
        for size, batch, name in ((64, 32, "config2"), (256, 1, "reference_defaults")):
            for f32m in ((True, False) if args.direct_steps else (True,)):
                steps, warmup = (args.steps, args.warmup) if f32m else (args.direct_steps, 1)
                lines.append(json.dumps(dict(config=name, **time_variant_steps(variant, f32m, size, batch, steps, warmup, dev))))
                print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    runs = [(True, 128, 64, "config3"), (True, 256, 1, "reference_defaults")]
    if args.direct_steps:
        runs.append((False, 64, 32, "config2"))
        runs.append((True, 64, 32, "config2"))
        if args.direct_config3:
            runs.append((False, 128, 64, "config3"))
    lines = []
    for f32m, size, batch, name in runs:
        steps, warmup = (args.steps, args.warmup) if f32m else (args.direct_steps, 1)
        r = dict(config=name, **time_steps(f32m, size, batch, steps, warmup, dev))
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
