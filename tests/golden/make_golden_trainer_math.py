"""Generates tests/golden/trainer_math.npz (run from the repo root: `python tests/golden/make_golden_trainer_math.py`).

The committed file was written from `UNetEngine.objective_coefficients`, `learning_rate` and `adam_alpha` as they stood before
the Trainer host math moved into `trainer_math.py` (the `VariantEngine` copies were checked `torch.equal` / `==` to them at the
same points): it pins that the move changed no bit.  This script writes the same arrays from the shared functions; rerunning it
must reproduce the committed file's contents exactly (tests/test_trainer_math_cpu.py), so regenerate only to add points.
Contents: `acw_<predict_x><predict_scaled_epsilon><prediction_weighting><ordinary_differential_equation>` = float32 [3, 200]
(a, c, w) for t_int = 1..200, steps = 200; `lr_*` / `adam_alpha_*` = float64 at optimizer.iterations `k` for the default
hyper-parameters (base_lr 2e-5, warm_up 2000) and for a constant rate (base_lr 1e-3, warm_up 0), betas 0.9 / 0.999.
"""
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gan_class_transfer2_amd import trainer_math as TM  # noqa: E402

KS = [0, 1, 5, 1999, 2000, 2001, 100000]
HYPER = {"default": dict(base_lr=2e-5, warm_up=2000), "const": dict(base_lr=1e-3, warm_up=0)}


def main():
    t_int = torch.arange(1, 201, dtype=torch.int32)
    out = {"t_int": t_int.numpy(), "k": np.array(KS, dtype=np.int64)}
    for bits in itertools.product((False, True), repeat=4):
        out["acw_" + "".join("01"[v] for v in bits)] = torch.stack(TM.objective_coefficients(t_int, 200, *bits)).numpy()
    for tag, hp in HYPER.items():
        lrs = [TM.warmup_lr(k, **hp) for k in KS]
        out["lr_" + tag] = np.array(lrs, dtype=np.float64)
        out["adam_alpha_" + tag] = np.array([TM.adam_step_size(lr, k, 0.9, 0.999) for lr, k in zip(lrs, KS)], dtype=np.float64)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "trainer_math.npz"), **out)


if __name__ == "__main__":
    main()
