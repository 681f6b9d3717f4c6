"""Host restatement of gct2_image_batch_cached's draw and the cases of tests/test_data_cache_gpu.py (a plain helper module: no
fixtures, no GPU).

The draw is restated from its definition in include/gct2.h, independently of data.sample_picks (which works sample by sample on
Python integers): here a whole epoch's permutation is formed at once on numpy arrays, from tests/pointwise_cases.py's Philox.
tests/test_data_cache_cases_cpu.py checks the restatement itself (a permutation, uniform, in range) and what the cases can tell apart.
"""
import functools

import numpy as np

import pointwise_cases as P

SHUFFLE, RANDOM_CROP, FLIP = 1, 2, 4
STREAM_AUG, STREAM_ORDER = 6, 7
M32 = np.uint64(P.MASK32)
_U = np.uint64


def philox_words(seed, stream_id, idx):
    """philox(seed, stream_id, idx) for a Python-int (or a list of Python ints) idx < 2^64: uint64 array [..., 4] of 32-bit words"""
    idx = np.asarray(idx, dtype=np.uint64)
    sid = _U(stream_id)
    return P.philox4x32_10((idx & M32, idx >> _U(32), np.full_like(idx, sid & M32), np.full_like(idx, sid >> _U(32))),
                           (seed & P.MASK32, seed >> 32)).astype(np.uint64)


def fmix32(x):
    """murmur3's finaliser on uint64 arrays holding 32-bit values"""
    x = x ^ (x >> _U(16))
    x = (x * _U(0x85EBCA6B)) & M32
    x = x ^ (x >> _U(13))
    x = (x * _U(0xC2B2AE35)) & M32
    return x ^ (x >> _U(16))


def half_bits(N):
    return max(1, ((N - 1).bit_length() + 1) // 2)


def feistel_pass(v, keys, h):
    mask = _U((1 << h) - 1)
    L, R = v >> _U(h), v & mask
    for j in range(8):
        kj = _U((int(keys[j & 3]) + j * 0x9E3779B9) & P.MASK32)
        L, R = R, L ^ (fmix32(R ^ kj) & mask)
    return (L << _U(h)) | R


@functools.lru_cache(maxsize=None)
def _permutation(seed, epoch, N):
    if N == 1:
        return np.zeros(1, dtype=np.int64), 0
    h = half_bits(N)
    keys = philox_words(seed, STREAM_ORDER, epoch)
    v = feistel_pass(np.arange(N, dtype=np.uint64), keys, h)
    passes = 1
    while True:                                        # cycle walking: the values still outside [0, N) take another pass
        out = v >= _U(N)
        if not out.any():
            break
        v[out] = feistel_pass(v[out], keys, h)
        passes += 1
    v = v.astype(np.int64)
    v.setflags(write=False)
    return v, passes


def permutation(seed, epoch, N):
    """pi_epoch as an int64 array: position p -> item"""
    return _permutation(seed, epoch, N)[0]


def permutation_passes(seed, epoch, N):
    """the longest cycle walk of the epoch"""
    return _permutation(seed, epoch, N)[1]


def picks_ref(seed, first_sample, B, hw, size, flags, sample_stride=1):
    """int32 [B, 4] = (item, oy, ox, flip) of the samples k = first_sample + b * sample_stride (mod 2^64)"""
    hw = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
    N = len(hw)
    ks = [(first_sample + b * sample_stride) & ((1 << 64) - 1) for b in range(B)]
    item = np.array([int(permutation(seed, k // N, N)[k % N]) if flags & SHUFFLE else k % N for k in ks], dtype=np.int64)
    r = philox_words(seed, STREAM_AUG, ks)             # [B, 4]
    H0, W0 = hw[item, 0], hw[item, 1]
    assert (H0 >= size).all() and (W0 >= size).all()
    if flags & RANDOM_CROP:
        oy = (r[:, 0] * (H0 - size + 1).astype(np.uint64)) >> _U(32)
        ox = (r[:, 1] * (W0 - size + 1).astype(np.uint64)) >> _U(32)
    else:
        oy, ox = (H0 - size) // 2, (W0 - size) // 2
    flip = r[:, 2] >> _U(31) if flags & FLIP else np.zeros(B, dtype=np.int64)
    return np.stack([item, oy.astype(np.int64), ox.astype(np.int64), flip.astype(np.int64)], 1).astype(np.int32)


def position_table(seed, N, epochs):
    """count[item, position] over the epochs 0 .. epochs - 1"""
    count = np.zeros((N, N), dtype=np.int64)
    pos = np.arange(N)
    for e in range(epochs):
        count[permutation(seed, e, N), pos] += 1
    return count


def chi_square(count):
    """Pearson's statistic of the item-by-position table against the uniform table, and its degrees of freedom (N - 1)^2"""
    N = count.shape[0]
    expect = count.sum() / (N * N)
    return float(((count - expect) ** 2).sum() / expect), (N - 1) ** 2


# ---- the cases of tests/test_data_cache_gpu.py ------------------------------------------------------------------------------------------
PERMUTATION_NS = [1, 2, 3, 4, 5, 16, 17, 37, 64, 65, 1000, 1025]
SEEDS = [0, 5, 0x9E3779B97F4A7C15]                      # the last has all 64 bits busy
EPOCHS = [0, 1, (1 << 32) + 7]
# odd sizes: the byte offsets of the later images take every alignment mod 4, and so do the rows inside an image
SOURCE_HW = [(32, 32), (32, 57), (45, 32), (33, 35), (47, 34), (39, 41), (71, 90)]
POOL_PAD = 16
SIZES = [32, 30]                                       # the four-pixel path and the per-element path
BATCHES = [5, 64]
FLAGS = list(range(8))
CASE_SEED = 0x9E3779B97F4A7C15
FIRST_SAMPLES = [0, len(SOURCE_HW) - 2, (1 << 32) + 3]  # N - 2: an epoch boundary inside the batch


@functools.lru_cache(maxsize=None)
def sources():
    """the seven decoded images (uint8 HWC, read-only)"""
    rng = np.random.default_rng(41)
    imgs = tuple(rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SOURCE_HW)
    for im in imgs:
        im.setflags(write=False)
    return imgs


def pool_layout(imgs):
    """(pool bytes with POOL_PAD spare bytes behind the last image, int64 offsets, int32 hw)"""
    sizes = np.array([im.size for im in imgs], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    pool = np.concatenate([im.reshape(-1) for im in imgs] + [np.zeros(POOL_PAD, dtype=np.uint8)])
    return pool, offsets, np.array([im.shape[:2] for im in imgs], dtype=np.int32)


def gpu_cases():
    """(size, B, flags, first_sample) of every drawn launch of the GPU test"""
    return [(size, B, flags, first) for size in SIZES for B in BATCHES for flags in FLAGS for first in FIRST_SAMPLES]


def source_alignments(picks, offsets, hw, size):
    """the set of (byte address mod 4, flip) over the first source byte of every group of four output pixels of every row of the
    picked crops: what the four-pixel path's shifts see"""
    seen = set()
    for item, oy, ox, flip in np.asarray(picks, dtype=np.int64):
        W0 = int(hw[item][1])
        y = np.arange(size)[:, None]
        x0 = np.arange(0, size - 3, 4)[None, :]
        sx0 = ox + (size - 4 - x0 if flip else x0)
        a = int(offsets[item]) + ((oy + y) * W0 + sx0) * 3
        seen |= {(int(m), int(flip)) for m in np.unique(a % 4)}
    return seen
