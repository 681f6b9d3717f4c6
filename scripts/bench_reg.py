"""what the L2 weight regularizer and the sign transformer (gct2_optimizer_apply_reg, gct2_grad_sumsq_l2, gct2_l2_penalty on the
non-fused optimizer path) cost on an MI355X, in one process (diagnostic): config 3 (3x128x128, batch 64, bf16), four engines - Adam
with fuse_adam = False (the arena path, gct2_adam_keras_multi behind the reverse pass: this tree does not touch it, so it is the parent
commit's non-fused step), Adam with l2 = 1e-6, SGD(1e-4, gradient_transformers=[sign_gradient]), Adam with l2 and global_clipnorm -
each warmed with 20 steps, then rounds of 50 steps per engine, the engines taking turns inside every round so that all see the same
box in the same second.  Device events around a round, a synchronise behind it; medians over the rounds.  Also the launches alone
over the config-3 arena, each beside its unregularized sibling, in alternating rounds (bytes per second, and the spread of the
sibling's own rounds).
usage: python scripts/bench_reg.py [output.json]      (default output: profiles/reg_bench.json)"""
import json, os, statistics, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gan_class_transfer2_amd as g
from gan_class_transfer2_amd.engine import Topology, UNetEngine, BF16

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "reg_bench.json")
if not torch.cuda.is_available():
    raise SystemExit("bench_reg.py measures on the GPU: no HIP device visible (there is no CPU figure)")
L = g._lib
dev = torch.device("cuda", 0)
WARMUP, STEPS, ROUNDS, KERNEL_ITERS = 20, 50, 7, 1000
BATCH, SIZE = 64, 128                                         # config 3
L2 = 1e-6


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                # milliseconds per call


ENGINES = {  # name: (optimizer, l2)
    "adam_non_fused": (g.Adam(g.WarmUp(2e-5, 2000)), None),
    "adam_l2": (g.Adam(g.WarmUp(2e-5, 2000)), L2),
    "sgd_sign": (g.SGD(1e-4, gradient_transformers=[g.sign_gradient]), None),
    "adam_l2_global_clipnorm": (g.Adam(g.WarmUp(2e-5, 2000), global_clipnorm=1.0), L2),
}
x = torch.rand(BATCH, SIZE, SIZE, 3, device=dev) * 2 - 1
engines = {}
for name, (opt, l2) in ENGINES.items():
    eng = UNetEngine(Topology(128, 512, 6), BF16, dev)
    g.Trainer(types.SimpleNamespace(engine=eng)).compile(opt, g.identity)
    eng.set_regularizer(l2)
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
    print("config-3 step, %-24s %.3f ms   (rounds: %s)" % (k, ms[k], " ".join("%.3f" % u for u in step_ms[k])))

# ---- the launches alone: the updates over tensors of their own of the arena's length, the reductions over an engine's arenas --------------
E = engines["adam_l2_global_clipnorm"]
N = E.arena.total
s = torch.cuda.current_stream().cuda_stream
f = lambda: torch.randn(N, dtype=torch.float32, device=dev) * 0.05
p, m, v, grad = f(), f() * 0.01, f().square(), f() * 0.01
shadow = p.to(torch.bfloat16)
C = g.trainer_math.l2_coefficients(L2)[1]
ptr = lambda t, used: t.data_ptr() if used else None


def sibling(kind, use_m, use_v, first, nes, second):
    if kind == L.OPT_ADAM:
        return lambda: L.call("gct2_adam_keras_clipped", p.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), shadow.data_ptr(), BF16, N, 1e-8,
                              first, second, 1e-7, 1.0, None, L.CLIP_NONE, 0.0, None, s)
    return lambda: L.call("gct2_optimizer_apply", kind, p.data_ptr(), ptr(m, use_m), ptr(v, use_v), grad.data_ptr(), shadow.data_ptr(), BF16, N, 1e-8,
                          first, nes, second, 1e-7, 1.0, None, L.CLIP_NONE, 0.0, None, s)


def reg(kind, use_m, use_v, first, nes, second, c, transform):
    return lambda: L.call("gct2_optimizer_apply_reg", kind, p.data_ptr(), ptr(m, use_m), ptr(v, use_v), grad.data_ptr(), shadow.data_ptr(), BF16, N,
                          1e-8, first, nes, second, 1e-7, 1.0, None, L.CLIP_NONE, 0.0, None, c, transform, s)


table, nseg, npartials, partials, sumsq, _ = E._clip_reduction()
coeffs = E._reg_table(E.arena._p.numel())[3]
A = E.arena
KERNELS = {  # name: (launch, bytes per parameter, the sibling it stands beside or None)
    "adam_keras_clipped": (sibling(L.OPT_ADAM, True, True, 0.9, 0, 0.999), 30, None),
    "apply_reg_adam_l2": (reg(L.OPT_ADAM, True, True, 0.9, 0, 0.999, C, L.GRAD_NONE), 30, "adam_keras_clipped"),
    "optimizer_apply_sgd": (sibling(L.OPT_SGD, False, False, 0.0, 0, 0.9), 14, None),
    "apply_reg_sgd_sign": (reg(L.OPT_SGD, False, False, 0.0, 0, 0.9, 0.0, L.GRAD_SIGN), 14, "optimizer_apply_sgd"),
    "optimizer_apply_rmsprop_momentum": (sibling(L.OPT_RMSPROP, True, True, 0.9, 0, 0.9), 30, None),
    "apply_reg_rmsprop_momentum_l2_sign": (reg(L.OPT_RMSPROP, True, True, 0.9, 0, 0.9, C, L.GRAD_SIGN), 30, "optimizer_apply_rmsprop_momentum"),
    "grad_sumsq": (lambda: L.call("gct2_grad_sumsq", A.g.data_ptr(), table.data_ptr(), nseg, npartials, 1.0, None, partials.data_ptr(),
                                  sumsq.data_ptr(), s), 4, None),
    "grad_sumsq_l2": (lambda: L.call("gct2_grad_sumsq_l2", A.g.data_ptr(), A._p.data_ptr(), table.data_ptr(), coeffs.data_ptr(), nseg, npartials, 1.0,
                                     None, partials.data_ptr(), sumsq.data_ptr(), s), 8, "grad_sumsq"),
}
for fn, _, _ in KERNELS.values():
    for _ in range(5):
        fn()
kernel_us = {k: [] for k in KERNELS}
for _ in range(ROUNDS):
    for k, (fn, _, _) in KERNELS.items():
        kernel_us[k].append(timed(fn, KERNEL_ITERS) * 1e3)
kus = {k: statistics.median(u) for k, u in kernel_us.items()}
inside = {}
for k, (_, bpp, sib) in KERNELS.items():
    note = ""
    if sib is not None and KERNELS[sib][1] == bpp:             # the same bytes: inside the spread of the sibling's own rounds?
        inside[k] = min(kernel_us[sib]) <= kus[k] <= max(kernel_us[sib])
        note = "  %s the spread of %s's rounds [%.1f, %.1f] us" % ("inside" if inside[k] else "OUTSIDE", sib, min(kernel_us[sib]), max(kernel_us[sib]))
    print("%-36s %7.1f us  %.2f TB/s of %.0f MB (%d bytes per parameter)%s" % (k, kus[k], bpp * N / kus[k] / 1e6, bpp * N / 1e6, bpp, note))

res = {"device": torch.cuda.get_device_name(0), "config": "3x128x128, batch 64, bf16, fuse_adam = False", "warmup_steps": WARMUP, "steps_per_round": STEPS,
       "rounds": ROUNDS, "arena_elements": N, "l2": L2,
       "step": {**{k + "_ms": round(ms[k], 4) for k in engines}, **{k + "_ms_rounds": [round(u, 4) for u in step_ms[k]] for k in engines},
                **{k + "_over_adam": round(ms[k] / ms["adam_non_fused"], 4) for k in engines if k != "adam_non_fused"}},
       "kernel": {**{k + "_us": round(kus[k], 2) for k in KERNELS}, **{k + "_us_rounds": [round(u, 2) for u in kernel_us[k]] for k in KERNELS},
                  **{k + "_bytes_per_parameter": KERNELS[k][1] for k in KERNELS},
                  **{k + "_tb_per_s": round(KERNELS[k][1] * N / kus[k] / 1e6, 3) for k in KERNELS},
                  **{k + "_inside_sibling_spread": bool(u) for k, u in inside.items()}, "launches_per_round": KERNEL_ITERS}}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", out_path)
