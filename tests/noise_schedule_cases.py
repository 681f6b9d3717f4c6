"""What the two GPU test files of the noise schedules share: the three mix chains of gct2_noise_image_table (include/gct2.h) in numpy
and an arbitrary table."""
import numpy as np
import torch

from oracle import denoiser_oracle as O

F32, BF16, F16 = 0, 1, 2

# arbitrary pairs (steps = 4): fp16-representable, sa^2 + sb^2 != 1, very different from entry to entry - a kernel that derives sb
# from sa, or reads a neighbouring image's pair, gives other values
TABLE4 = np.array([[0.5, 2.0], [-1.75, 0.25], [3.0, -0.5], [0.125, 1.5]], np.float32)


def mix_ref(dt, x, eps, pairs):
    """x, eps [B, HW, C] float32, pairs [B, 2] float32 (the table rows of the images) -> torch tensor of the storage dtype.
    F32: fl(fl(x * sa) + fl(eps * sb)); BF16: that rounded once more; F16: (fp16)x * (fp16)sa and (fp16)eps * (fp16)sb, each
    rounded to fp16, then their fp16 sum (numpy rounds every float16 / float32 operation on its own and fuses nothing)"""
    x, eps, pairs = np.asarray(x, np.float32), np.asarray(eps, np.float32), np.asarray(pairs, np.float32)
    shape = (-1,) + (1,) * (x.ndim - 1)
    sa, sb = pairs[:, 0].reshape(shape), pairs[:, 1].reshape(shape)
    if dt == F16:
        h = np.float16
        assert np.array_equal(pairs, pairs.astype(h).astype(np.float32))                 # the host stores fp16-representable pairs
        xs, es = x.astype(h) * sa.astype(h), eps.astype(h) * sb.astype(h)
        assert xs.dtype == h and es.dtype == h
        return torch.tensor((xs + es).astype(h))
    s = x * sa + eps * sb
    assert s.dtype == np.float32
    return torch.tensor(O.round_bf16(s)).to(torch.bfloat16) if dt == BF16 else torch.tensor(s)
