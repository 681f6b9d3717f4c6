"""Host references of the RNG streams and the pointwise step kernels (a plain helper module: no fixtures, no GPU).

The streams are restated from their definition in include/gct2.h (gct2_rng_uniform_int / gct2_rng_normal), the Philox4x32-10 round
function from Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC'11): two 32x32 -> 64 bit products per round, the key
bumped by the Weyl constants between rounds.  Integer arithmetic is exact, so gct2_rng_uniform_int is compared bit for bit; the
normals are a float64 Box-Muller of the documented float32 uniforms, and the kernel's hardware log2 / sin / cos are bounded against it.

The float32 restatements (noise_image_f32 lives in oracle/denoiser_oracle.py beside noise_image_f16) round every operation to
float32 on its own, in the order include/gct2.h gives: numpy's float32 +, -, *, / and sqrt are IEEE single operations.
"""
import functools

import numpy as np
import torch

from oracle import denoiser_oracle as O

MASK32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # the two multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # key increments: golden ratio, sqrt(3) - 1
SAMPLE_X, SAMPLE_EPS, SAMPLE_SCALED_EPS, SAMPLE_ODE = 0, 1, 2, 3

# ---- the cases of tests/test_pointwise_exact_gpu.py (tests/test_pointwise_cases_cpu.py checks what they can tell apart) --------------
# (seed, stream_id): the first four differ only in their high words, the last has all 64 bits of both busy
SEEDS = [(1, 2), (1 + (1 << 32), 2), (1, 2 + (1 << 32)), (1 + (1 << 32), 2 + (1 << 32)), (0x9E3779B97F4A7C15, 0xD1B54A32D192ED03)]
CARRY = (1 << 34) - 6                                  # element 2^34 = counter 2^32: the low counter word wraps, the high one becomes 1
OFFSETS = [0, 1, 2, 3, 5, CARRY]
INT_NS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 1003]
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INT_RANGES = [(1, 200), (7, 7), (-5, 5), (0, INT32_MAX), (INT32_MIN, INT32_MIN + 1), (INT32_MIN, INT32_MAX)]
NORMAL_LONG_N = 2048 * 256 + 1031                      # the grid is capped at 2048 work-groups of 256: the first length with a second trip
NOISE_STEPS = (200, 6)
MIX_SHAPE = (3, 1031)                                  # B, per_image
# per-image (a, c) of gct2_mix_per_image: two images with both coefficients non-trivial, and 0 / 1 in every position
MIX_COEFS = [((0.4871, 1.9375, 1.0), (0.8733, 0.3331, 0.0)), ((0.0, 1.0, 0.4871), (1.0, 1.0, 0.3331))]
DIFFUSION_TS = (1, 37, 199, 200)
DIFFUSION_STEPS = 200
DIFFUSION_SHAPE = (1003, 3)                            # npix, C


# ---- Philox4x32-10 ------------------------------------------------------------------------------------------------------------------

def philox4x32_10(counter_words, key_words):
    """counter_words: four uint32 words (scalars or equally shaped arrays), key_words: two.  Returns the four output words as a
    uint32 array [..., 4]."""
    c = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK32) for w in counter_words]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key_words[0]) & MASK32, int(key_words[1]) & MASK32
    lo32, sh = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]               # < 2^64: both factors are below 2^32
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return np.stack(c, -1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _stream_blocks(seed, stream_id, first_counter, ncounters):
    idx = np.arange(ncounters, dtype=np.uint64) + np.uint64(first_counter)
    sid = np.uint64(stream_id)
    words = philox4x32_10((idx & np.uint64(MASK32), idx >> np.uint64(32), np.full_like(idx, sid & np.uint64(MASK32)),
                           np.full_like(idx, sid >> np.uint64(32))), (seed & MASK32, seed >> 32))
    words.setflags(write=False)
    return words


def stream_blocks(seed, stream_id, offset, n):
    """the Philox outputs [ncounters, 4] that cover elements [offset, offset + n) and the index of element `offset` in their
    flattening: counter = (idx, stream_id) as four words, key = seed as two, element e uses counter e >> 2"""
    first = offset >> 2
    return _stream_blocks(seed, stream_id, first, ((offset + n + 3) >> 2) - first), offset & 3


def stream_words(seed, stream_id, offset, n):
    """word e & 3 of counter e >> 2 for the elements e = offset .. offset + n - 1"""
    blocks, skip = stream_blocks(seed, stream_id, offset, n)
    return blocks.reshape(-1)[skip:skip + n]


def uniform_int_ref(seed, stream_id, offset, n, lo, hi):
    """lo + ((r * range) >> 32) with range = hi - lo + 1 in 64 bits (up to 2^32: then the result is lo + r); int32 array"""
    assert INT32_MIN <= lo <= hi <= INT32_MAX
    r = stream_words(seed, stream_id, offset, n).astype(np.uint64)
    rng_ = np.uint64(hi - lo + 1)
    return (np.int64(lo) + ((r * rng_) >> np.uint64(32)).astype(np.int64)).astype(np.int32)


def uniform_of_word(r):
    """u = ((float)(r >> 8) + 0.5f) * 2^-24 in float32, each operation rounded to float32: (0, 1], 1.0 at r >> 8 = 2^24 - 1"""
    r = np.asarray(r, dtype=np.uint32)
    return ((r >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def normal_ref(seed, stream_id, offset, n):
    """float64 Box-Muller of the float32 uniforms: words (0, 1) of a counter make elements 4c (cos) and 4c + 1 (sin), words (2, 3)
    elements 4c + 2 and 4c + 3"""
    blocks, skip = stream_blocks(seed, stream_id, offset, n)
    u = uniform_of_word(blocks)
    assert u.dtype == np.float32
    u = u.astype(np.float64).reshape(-1, 2, 2)          # [counter, pair, (u1, u2)]
    rad = np.sqrt(-2.0 * np.log(u[..., 0]))
    ang = 2.0 * np.pi * u[..., 1]
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1)
    return z.reshape(-1)[skip:skip + n]


# ---- float32 restatements ------------------------------------------------------------------------------------------------------------------

def _f32(a):
    return np.asarray(a, dtype=np.float32)


def mix_per_image_f32(x, eps, a, c):
    """gct2_mix_per_image: fl(fl(a[b] x) + fl(c[b] eps)); eps None: fl(a[b] x).  x, eps [B, per_image]"""
    ax = _f32(a)[:, None] * _f32(x)
    return ax if eps is None else ax + _f32(c)[:, None] * _f32(eps)


def mix_per_image_fused(x, eps, a, c):
    """the contracted form fma(a[b], x, fl(c[b] eps)) - what the kernel must NOT compute (the product a x is exact in float64)"""
    ce = (_f32(c)[:, None] * _f32(eps)).astype(np.float64)
    return (_f32(a)[:, None].astype(np.float64) * _f32(x).astype(np.float64) + ce).astype(np.float32)


def diffusion_mix_f32(x, e, alpha):
    """gct2_diffusion_mix: a32 = float32(alpha), sa = sqrt(a32), sb = sqrt(1 - a32) in float32, fake = fl(fl(sa x) + fl(sb e));
    the copies stored in the compute dtype are one rounding of fake"""
    a32 = np.float32(alpha)
    sa, sb = np.sqrt(a32), np.sqrt(np.float32(1.0) - a32)
    assert sa.dtype == np.float32 and sb.dtype == np.float32
    return sa * _f32(x) + sb * _f32(e)


def diffusion_update_f32(mode, pred, fake, alpha, alpha_prev):
    """gct2_diffusion_update: the coefficients are square roots in double, each cast once to float32 (the ODE denominator is formed in
    double and cast once); then the formulas of include/gct2.h, one float32 rounding per operation, true division.
    Returns (x_theta, eps_theta); eps_theta is None in ODE mode (not touched)."""
    p, f = _f32(pred), _f32(fake)
    dsa, dsb = np.sqrt(np.float64(alpha)), np.sqrt(1.0 - np.float64(alpha))
    sa, sb = np.float32(dsa), np.float32(dsb)
    if mode == SAMPLE_X:
        return p.copy(), (f - sa * p) / sb
    if mode == SAMPLE_EPS:
        return (f - p * sb) / sa, p.copy()
    if mode == SAMPLE_SCALED_EPS:
        return (f - p) / sa, p / sb
    dsa1, dsb1 = np.sqrt(np.float64(alpha_prev)), np.sqrt(1.0 - np.float64(alpha_prev))
    sb1, den = np.float32(dsb1), np.float32(dsa1 * dsb - dsa * dsb1)
    return (p * sb - f * sb1) / den, None


def noise_coefs_reciprocal(t_int, steps):
    """(sa, sb) with t = t_int * fl(1 / (steps + 1)) instead of the reference's division (train.py:87): GCT2_F32 must not use it
    (an fp32 output shows the difference); GCT2_BF16 is documented to (include/gct2.h: a bf16 output shows it only at ties)"""
    t = _f32(t_int) * (np.float32(1.0) / np.float32(steps + 1))
    om = np.float32(1.0) - t
    a = (om * om) * np.float32(0.25)
    return np.sqrt(a), np.sqrt(np.float32(1.0) - a)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def image_values(rng, shape):
    """x as the input contract leaves it: u8 / 128 - 1, exact in every storage type"""
    return (rng.integers(0, 256, shape).astype(np.float32) / np.float32(128.0)) - np.float32(1.0)


@functools.lru_cache(maxsize=None)
def noise_case(steps):
    """one image per timestep 1 .. steps, HW = 4, C = 3"""
    rng = np.random.default_rng([steps, 31])
    B, HW, C = steps, 4, 3
    case = dict(x=image_values(rng, (B, HW, C)), eps=rng.standard_normal((B, HW, C)).astype(np.float32),
                t=np.arange(1, steps + 1, dtype=np.int32))
    for v in case.values():
        v.setflags(write=False)
    return case


def noise_image_bf16_rule(x, t_int, eps, steps):
    """gct2_noise_image's GCT2_BF16 as include/gct2.h documents it: noise_image_f32's op chain with t = t_int * fl(1 / (steps + 1)),
    rounded once to bf16 (float32 array holding the values)"""
    sa, sb = noise_coefs_reciprocal(t_int, steps)
    shape = (-1,) + (1,) * (np.ndim(x) - 1)
    return O.round_bf16(_f32(x) * sa.reshape(shape) + _f32(eps) * sb.reshape(shape))


NOISE_TIE_POOL_HW, NOISE_TIE_HW, NOISE_TIE_IMAGES = 4096, 8, 8


@functools.lru_cache(maxsize=None)
def noise_tie_case():
    """the bf16 rule can be told from the division only where the fp32 sum is a tie of the bf16 store, about one element in 2^16:
    from a pool of random images at the timesteps where the two forms give another sqrt(a) or sqrt(1 - a) (steps = 200), the
    groups of four pixels that hold such an element are kept - NOISE_TIE_IMAGES images of NOISE_TIE_HW pixels, each with at least one"""
    steps = 200
    f = np.float32
    t_all = np.arange(1, steps + 1, dtype=np.int32)
    td = t_all.astype(f) / f(steps + 1)
    a = ((f(1.0) - td) * (f(1.0) - td)) * f(0.25)
    sa_r, sb_r = noise_coefs_reciprocal(t_all, steps)
    t = t_all[(np.sqrt(a) != sa_r) | (np.sqrt(f(1.0) - a) != sb_r)]
    rng = np.random.default_rng(37)
    shape = (t.size, NOISE_TIE_POOL_HW, 3)
    x, eps = image_values(rng, shape), rng.standard_normal(shape).astype(np.float32)
    hit = (noise_image_bf16_rule(x, t, eps, steps) != O.noise_image_f32(x, t, eps, steps, "bf16")).any(-1)      # [image, pixel]
    groups = hit.reshape(t.size, -1, 4).any(-1)
    xs, es, ts = [], [], []
    for b in np.nonzero(groups.any(1))[0][:NOISE_TIE_IMAGES]:
        g = int(np.nonzero(groups[b])[0][0])
        g = min(g, groups.shape[1] - 2)                                    # this group of four pixels and its neighbour
        xs.append(x[b, 4 * g:4 * g + NOISE_TIE_HW]); es.append(eps[b, 4 * g:4 * g + NOISE_TIE_HW]); ts.append(t[b])
    case = dict(x=np.stack(xs), eps=np.stack(es), t=np.array(ts, dtype=np.int32), steps=steps)
    for v in (case["x"], case["eps"], case["t"]):
        v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def mix_case():
    rng = np.random.default_rng(32)
    x, eps = (rng.standard_normal(MIX_SHAPE).astype(np.float32) for _ in range(2))
    x.setflags(write=False)
    eps.setflags(write=False)
    return x, eps


@functools.lru_cache(maxsize=None)
def diffusion_case():
    rng = np.random.default_rng(33)
    arrs = tuple(rng.standard_normal(DIFFUSION_SHAPE).astype(np.float32) for _ in range(3))       # x_theta, eps_theta, pred
    for v in arrs:
        v.setflags(write=False)
    return arrs


def diffusion_alphas(t):
    """(alpha, alpha_prev) as the sampler forms them: Python floats"""
    return float(O.alpha_dash(t, DIFFUSION_STEPS)), float(O.alpha_dash(t - 1, DIFFUSION_STEPS))


def rounded(a32, tdt):
    """a float32 array rounded once to the torch dtype (torch's round-to-nearest-even conversion)"""
    return torch.tensor(np.ascontiguousarray(a32, dtype=np.float32)).to(tdt)
