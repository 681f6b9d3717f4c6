"""Host restatement of gct2_image_grid_u8 (a plain helper module: no fixtures, no GPU) and the cases of its tests.

The three quantisations are restated from include/gct2.h with one float32 rounding per operation (numpy's float32 * and + are IEEE
single operations, as in tests/pointwise_cases.py), the grid layout from its formulas with plain loops over cells.  The value ladder
holds, for every mode and every byte q = 1..255, the float32 just below, at and just above the point where the restatement steps to
q - found by bisection over the float32 ordering, the restatement being monotone - beside the special values; 16-bit variants use the
ladder rounded to the dtype first.  tests/test_image_out_cases_cpu.py holds the restatement to exact rational arithmetic."""
import functools

import numpy as np
import torch

SUMMARY, DATASET, UNIT = 0, 1, 2
MODES = {"summary": SUMMARY, "dataset": DATASET, "unit": UNIT}
F32, BF16, F16 = 0, 1, 2
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
POISON = 0xA5
FILL = (0x12, 0xC8, 0x7F)                               # a non-black fill with three distinct bytes
f32 = np.float32

# ---- the layouts of tests/test_image_out_kernels_gpu.py: (n, H, W, cols, rows, pad, scale) ---------------------------------------------
LAYOUTS = {
    "wide_straddling_one_empty_cell": (5, 6, 8, 3, 2, 2, 1),        # GW = 32: wide path, groups straddle padding, cell 5 is empty
    "to_uint8": (5, 6, 8, 1, 5, 0, 1),                              # the plain conversion: the same memory as [n,H,W,3]
    "per_pixel": (5, 6, 6, 3, 2, 1, 1),                             # GW = 22
    "scale2_wide": (3, 6, 8, 2, 2, 4, 2),                           # GW = 44
    "scale3_general": (5, 6, 8, 2, 3, 2, 3),                        # GW = 54
    "one_image": (1, 6, 8, 1, 1, 2, 1),                             # GW = 12: wide
    "full_grid": (6, 6, 8, 3, 2, 2, 1),                             # n = cols rows exactly
    "narrow_cells": (7, 3, 1, 7, 1, 0, 1),                          # W = 1: a group of four crosses four cells (GW = 7: per pixel)
    "narrow_cells_wide": (8, 3, 1, 8, 1, 0, 1),                     # ... and on the wide path (GW = 8)
}
# n = 3, H = W = 64: several work-groups and more than one trip of the grid-stride loop on both paths.  pad = 2, cols = 2 gives
# GW = 134 (per pixel: 134 * 134 = 17956 pixels, 18 work-groups of 1024); pad = 0 gives GW = 128 (wide: 4096 groups of four, 8
# work-groups of 512)
LAYOUTS["several_work_groups_wide"] = (3, 64, 64, 2, 2, 0, 1)
LAYOUTS["several_work_groups_per_pixel"] = (3, 64, 64, 2, 2, 2, 1)
# the output above 2^31 bytes: n = 2, H = W = 2048, cols = 1, scale = 12 is 2 * 24576 * 24576 * 3 = 3.6e9 bytes, cell 1 starts at
# byte 1.8e9 and ends past 2^31
LARGE = (2, 2048, 2048, 1, 2, 0, 12)


def grid_dims(n, H, W, cols, rows, pad, scale):
    return rows * H * scale + (rows + 1) * pad, cols * W * scale + (cols + 1) * pad


def is_wide(layout, out_offset=0):
    return grid_dims(*layout)[1] % 4 == 0 and out_offset % 4 == 0


# ---- the quantisation -------------------------------------------------------------------------------------------------------------------
def z_ref(x, mode):
    """z of include/gct2.h on a float32 array: every product and sum rounded to float32 on its own"""
    x = np.asarray(x, dtype=f32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if mode == SUMMARY:
            return f32(255.5) * (f32(0.5) * x + f32(0.5))
        if mode == DATASET:
            return f32(128.0) * x + f32(128.5)
        if mode == UNIT:
            return f32(255.5) * x
    raise ValueError(mode)


def quantize_ref(x, mode):
    """q of include/gct2.h: 0 for a NaN or z < 1, 255 for z >= 255, trunc(z) otherwise"""
    z = z_ref(x, mode)
    assert z.dtype == f32
    q = np.zeros(z.shape, dtype=np.uint8)
    mid = (z >= 1) & (z < 255)
    q[mid] = np.trunc(z[mid]).astype(np.uint8)
    q[z >= 255] = 255
    return q


def grid_ref(images, mode, cols, rows, pad, scale, fill=(0, 0, 0)):
    """the whole output of gct2_image_grid_u8 for float32 images [n,H,W,3]: u8 [GH,GW,3]"""
    images = np.asarray(images, dtype=f32)
    n, H, W, _ = images.shape
    GH, GW = grid_dims(n, H, W, cols, rows, pad, scale)
    out = np.empty((GH, GW, 3), dtype=np.uint8)
    out[:] = np.array(fill, dtype=np.uint8)
    q = quantize_ref(images, mode)
    for i in range(n):
        r, c = divmod(i, cols)
        y0, x0 = pad + r * (H * scale + pad), pad + c * (W * scale + pad)
        out[y0:y0 + H * scale, x0:x0 + W * scale] = np.repeat(np.repeat(q[i], scale, axis=0), scale, axis=1)
    return out


# ---- the value ladder -------------------------------------------------------------------------------------------------------------------
def _key_to_f32(key):
    """float32 ordering as integers: key >= 0 is the bit pattern of a non-negative float, key < 0 the negative float of magnitude -key"""
    key = np.asarray(key, dtype=np.int64)
    bits = np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)
    return bits.view(f32)


def _f32_to_key(x):
    bits = np.asarray(x, dtype=f32).view(np.uint32).astype(np.int64)
    return np.where(bits & 0x80000000, -(bits & 0x7FFFFFFF), bits)


@functools.lru_cache(maxsize=None)
def steps(mode):
    """float32 [255]: for q = 1..255 the smallest float32 x (in float32 order) with quantize_ref(x) >= q"""
    target = np.arange(1, 256)
    lo = np.full(255, _f32_to_key(f32(-3e38)), dtype=np.int64)           # q(lo) = 0 < target
    hi = np.full(255, _f32_to_key(f32(3e38)), dtype=np.int64)            # q(hi) = 255 >= target
    assert quantize_ref(_key_to_f32(lo[:1]), mode)[0] == 0 and quantize_ref(_key_to_f32(hi[:1]), mode)[0] == 255
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        up = quantize_ref(_key_to_f32(mid), mode) >= target
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    return _key_to_f32(hi)


def specials():
    return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 3e38, -3e38, 1e-45, -1e-45], dtype=f32)


def dataset_values():
    """v / 128 - 1 for every byte v: what the loader makes (train.py:292), exact in float32"""
    return (np.arange(256, dtype=f32) / f32(128) - f32(1)).astype(f32)


@functools.lru_cache(maxsize=None)
def ladder(mode):
    """float32 1-D: below / at / above every step of `mode`, the specials, the loader's 256 values and seeded normals; its length is
    coprime to 3 and to 2, so that dealt round-robin (deal) every value meets every channel"""
    at = steps(mode)
    rng = np.random.default_rng(1234 + mode)
    normals = (rng.standard_normal(300) * (0.6 if mode != UNIT else 0.4) + (0.0 if mode != UNIT else 0.5)).astype(f32)
    v = np.concatenate([np.nextafter(at, f32(-np.inf)), at, np.nextafter(at, f32(np.inf)), specials(), dataset_values(), normals]).astype(f32)
    while v.size % 2 == 0 or v.size % 3 == 0:
        v = np.append(v, f32(0.25))
    return v


def ladder_as(mode, dtype):
    """the ladder rounded to the storage dtype first (and widened back exactly): what a 16-bit source can hold"""
    v = torch.from_numpy(ladder(mode).copy())
    return v.to(TORCH_DTYPE[dtype]).to(torch.float32).numpy()


def deal(values, shape):
    """values dealt round-robin over the elements of `shape` in memory order"""
    count = int(np.prod(shape))
    return np.resize(np.asarray(values, dtype=f32), count).reshape(shape)


LADDER_SHAPE = (5, 16, 17, 3)                           # 4080 elements: more than three times the longest ladder


def images_for(layout, seed=0):
    """seeded float32 images in a little more than [-1, 1] for a layout"""
    n, H, W = layout[:3]
    return (np.random.default_rng(seed).standard_normal((n, H, W, 3)) * 0.7).astype(f32)
