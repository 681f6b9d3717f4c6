"""Host references and case tables of dynamic thresholding (a plain helper module: no fixtures, no GPU): gct2_x0_quantile restated from
include/gct2.h - the keys, the order statistic by numpy's sort of the uint32 keys (the ground truth), a pure-numpy radix select with
the shipped digit widths, the finishing rule - and gct2_diffusion_step_dynamic in float32, one rounding per numpy operation, on top of
generate_cases / img2img_cases / multistep_cases; the crafted planes and the scaled step inputs of tests/test_dynamic_kernels_gpu.py.
"""
import functools

import numpy as np

import generate_cases as G
import img2img_cases as I
import multistep_cases as MC
from pointwise_cases import SAMPLE_EPS, SAMPLE_SCALED_EPS, SAMPLE_X

SAMPLE_V = 5
MODES = [SAMPLE_X, SAMPLE_EPS, SAMPLE_SCALED_EPS, SAMPLE_V]
MODE_IDS = ["x", "eps", "scaled_eps", "v"]
DIGITS = (11, 10, 10)                                  # the shipped digit widths, top digit first: 31 key bits
PERCENTILE, FLOOR = 0.995, 1.0
# per-image scales of the step inputs, in units of the estimate's own spread: at p = 0.995 the statistic of k N(0, 1) is about 2.8 k, so
# the first image stays under the floor (the fixed bound), the other two are rescaled.  One image (the long shape): rescaled
SCALES = (0.2, 1.0, 30.0)
C1 = 1.37


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def quantile_rank(p, n):
    """trainer_math.quantile_rank restated: min(n, max(1, ceil(p n)))"""
    return min(n, max(1, int(np.ceil(np.float64(p) * n))))


# ---- the select ----------------------------------------------------------------------------------------------------------------------------

def estimate_f32(mode, pred, fake, a_t):
    """(x, e) float32: gct2_diffusion_step's UNCLIPPED update, one rounding per operation; mode X does not read fake"""
    with np.errstate(all="ignore"):
        p = _f32(pred)
        sa, sb = np.float32(np.sqrt(np.float64(a_t))), np.float32(np.sqrt(1.0 - np.float64(a_t)))
        if mode == SAMPLE_X:
            return p.copy(), None if fake is None else (_f32(fake) - sa * p) / sb
        f = _f32(fake)
        if mode == SAMPLE_EPS:
            return (f - p * sb) / sa, p.copy()
        if mode == SAMPLE_SCALED_EPS:
            return (f - p) / sa, p / sb
        assert mode == SAMPLE_V
        return sa * f - sb * p, sb * f + sa * p


def keys(x):
    """bits(x) & 0x7fffffff as uint32: the order of |x| with -0 = +0, +inf above every finite value, every NaN above +inf"""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def kth_key(k, rank):
    """the rank-th smallest (1-based) of a row of keys: numpy's sort, the ground truth"""
    return np.sort(np.asarray(k, dtype=np.uint32), kind="stable")[rank - 1]


def radix_select(k, rank, digits=DIGITS):
    """the kernel's algorithm in numpy: per digit, top first, the histogram of the digit over the keys whose higher digits equal the
    prefix found so far, then the bin that holds the rank left"""
    k = np.asarray(k, dtype=np.uint32)
    assert sum(digits) == 31 and 1 <= rank <= k.size
    shift, prefix, left = 31, 0, int(rank)
    for bits in digits:
        live = k[(k >> np.uint32(shift)) == prefix] if shift < 31 else k
        shift -= bits
        hist = np.bincount(((live >> np.uint32(shift)) & np.uint32((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)
        below = np.cumsum(hist) - hist
        digit = int(np.nonzero((below < left) & (left <= below + hist))[0][0])
        left -= int(below[digit])
        prefix = (prefix << bits) | digit
    return np.uint32(prefix)


def quantile_f32(x, rank, select=kth_key):
    """q [B] float32 (raw bits) of x [B, per_image]"""
    return np.array([select(keys(row), rank) for row in x], dtype=np.uint32).view(np.float32)


def finish(q, floor):
    """rows [B, 2] = {s, r}: s = (q > F && q < inf) ? q : F, r = (s == F) ? 1 : F / s (one float32 division)"""
    q, F = _f32(q), np.float32(floor)
    with np.errstate(all="ignore"):
        s = np.where((q > F) & (q < np.float32(np.inf)), q, F).astype(np.float32)
        r = np.where(s == F, np.float32(1.0), F / s).astype(np.float32)
    return np.stack([s, r], 1)


def select_f32(mode, pred, fake, a_t, rank, floor, select=kth_key):
    """gct2_x0_quantile: (rows [B, 2], q [B])"""
    x, _ = estimate_f32(mode, pred, fake, a_t)
    q = quantile_f32(x, rank, select)
    return finish(q, floor), q


# ---- the step ------------------------------------------------------------------------------------------------------------------------------

def threshold_f32(mode, pred, fake, a_t, rows):
    """(x, e) float32 after the per-image bound: the clip to [-s, s] (a NaN stays), ONE rounded multiply by r, eps re-derived"""
    with np.errstate(all="ignore"):
        x, _ = estimate_f32(mode, pred, fake, a_t)
        f = _f32(fake)
        sa, sb = np.float32(np.sqrt(np.float64(a_t))), np.float32(np.sqrt(1.0 - np.float64(a_t)))
        s, r = _f32(rows)[:, :1], _f32(rows)[:, 1:]
        x = np.where(x < -s, -s, np.where(x > s, s, x)).astype(np.float32)
        x = x * r
        e = (f - sa * x) / sb
        assert x.dtype == np.float32 and e.dtype == np.float32
        return x, e


def dynamic_step_f32(mode, pred, fake, rows, a_t, a_prev, s2=0.0, z=None, hist=None, c1=None, known=None, mask_el=None, z0=None):
    """gct2_diffusion_step_dynamic as include/gct2.h states it.  c1 None: the plain / masked step (z the step's draws when s2 != 0);
    a number: the multistep form (hist read at c1 != 0).  known, mask_el, z0: the masked form.  Returns (fake', x0_out, hist_out)."""
    with np.errstate(all="ignore"):
        f = _f32(fake)
        x, e = threshold_f32(mode, pred, fake, a_t, rows)
        sa, sb, cx, ce, cz = G.step_coefficients(a_t, a_prev, 0.0 if c1 is not None else s2)
        c = np.float32(0.0 if c1 is None else c1)
        if c == 0:
            g = cx * x + ce * e
        else:
            d = x + c * (x - _f32(hist))
            ed = (f - sa * d) / sb
            g = cx * d + ce * ed
        if c1 is None and np.float32(s2) != 0:
            g = g + cz * _f32(z)
        assert g.dtype == np.float32
        if known is None:
            return g, x, x
        h = I.kept_f32(known, a_prev, z0)
        return I.blend_f32(mask_el, g, h), I.blend_f32(mask_el, x, _f32(known)), x


def fixed_clip_step_f32(mode, pred, fake, a_t, a_prev, clip):
    """gct2_diffusion_step at sigma2 = 0 with the scalar clip, for all four objectives (generate_cases restates three): (fake', x)"""
    rows = np.float32([[clip, 1.0]] * np.asarray(pred).shape[0])
    got, x, _ = dynamic_step_f32(mode, pred, fake, rows, a_t, a_prev)
    return got, x


def dynamic_step_fused(mode, pred, fake, rows, a_t, a_prev, hist, c1, term=0):
    """the contracted forms around the rescale - what the kernel must NOT compute, at c1 != 0 where x r meets an addition (a product of
    two float32 values is exact in float64): term 0 is d = fma(x, r, fl(c (fl(x r) - hist))), the multiply by r folded into the
    extrapolation; term 1 is e = fl(f - sa x) with the product sa x unrounded, the eps line's own fused multiply-add at c1 = 0.
    Returns fake' of the plain multistep form"""
    with np.errstate(all="ignore"):
        f = _f32(fake)
        x, _ = estimate_f32(mode, pred, fake, a_t)
        sa, sb, cx, ce, _ = G.step_coefficients(a_t, a_prev, 0.0)
        s, r = _f32(rows)[:, :1], _f32(rows)[:, 1:]
        xc = np.where(x < -s, -s, np.where(x > s, s, x)).astype(np.float32)
        x = xc * r
        if term == 0:
            c = np.float32(c1)
            d = (xc.astype(np.float64) * r.astype(np.float64) + (c * (x - _f32(hist))).astype(np.float64)).astype(np.float32)
            ed = (f - sa * d) / sb
            return cx * d + ce * ed
        e = (f.astype(np.float64) - np.float64(sa) * x.astype(np.float64)).astype(np.float32) / sb
        return cx * x + ce * e


# ---- the step inputs -------------------------------------------------------------------------------------------------------------------------

def step_scale(mode, a_t):
    """the factor that puts the estimate's spread at about 1 for unit-normal pred and fake: the epsilon modes divide by sqrt(a_t)"""
    return float(np.sqrt(a_t)) if mode in (SAMPLE_EPS, SAMPLE_SCALED_EPS) else 1.0


@functools.lru_cache(maxsize=None)
def step_inputs(shape, mode, t):
    """(pred, fake) float32 [B, per_image] of a (mode, t) case: multistep_cases.step_inputs (CLIP_SPECIALS planted in pred where the
    shape has generate_cases' images) with pred and fake of image b times SCALES[b] step_scale - the planted NaN and infinities
    survive the scaling, fewer of them than the elements above the rank"""
    B, npix, C = shape
    p, f = (a.copy() for a in MC.step_inputs(shape))
    a_t, _ = G.alphas(t)
    with np.errstate(all="ignore"):
        for b in range(B):
            k = np.float32((SCALES[b] if B > 1 else SCALES[1]) * step_scale(mode, a_t))
            p[b] *= k
            f[b] *= k
    p.setflags(write=False)
    f.setflags(write=False)
    return p, f


# ---- crafted planes for the select in mode X: the smallest inputs where each digit pass can go wrong -------------------------------------------

def _from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def crafted_cases(per_image=G.NPIXS[0] * G.C):
    """[(name, plane float32 [3, per_image], ranks)]: three images with different distributions in every plane (a cross-image mix-up
    shows), signs alternating so that the keys, not the values, decide"""
    n = per_image
    rng = np.random.default_rng([n, 71])
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    normal = lambda k: (rng.standard_normal(n) * k).astype(np.float32)
    shuffled = lambda v: rng.permutation(_f32(v))
    ends = (1, 2, n // 2, n - 1, n)
    cases = []
    # all equal / two values with the boundary at n // 3 / a run of ties around the middle
    two = np.where(np.arange(n) < n // 3, 0.75, 1.5).astype(np.float32)
    ties = np.concatenate([np.linspace(0.1, 0.5, n // 2 - 50), np.full(100, 0.625), np.linspace(0.7, 3.0, n - n // 2 - 50)])
    cases.append(("equal_two_ties", np.stack([np.full(n, -2.5, np.float32) * sign, shuffled(two) * sign, shuffled(ties) * sign]),
                  ends + (n // 3 - 1, n // 3, n // 3 + 1, n // 2 - 50, n // 2 - 49, n // 2 + 50, n // 2 + 51)))
    # neighbours that differ only in the lowest key bit / only in the top bit of each digit (bits 30, 19, 9) / only in the lowest bit of
    # each digit (20, 10, 0)
    base = np.uint32(0x3F800000)
    low = _from_bits(base + (np.arange(n) % 2).astype(np.uint32))
    tops = _from_bits(np.uint32(0x1F8AAAAA) ^ (np.uint32(1) << np.uint32([30, 19, 9])[np.arange(n) % 3]))
    lows = _from_bits(np.uint32(0x3F8AAAAA) ^ (np.uint32(1) << np.uint32([20, 10, 0])[np.arange(n) % 3]))
    cases.append(("single_bits", np.stack([shuffled(low) * sign, shuffled(tops), shuffled(lows) * sign]),
                  ends + (n // 3, n // 3 + 1, n // 3 + 2, 2 * (n // 3), 2 * (n // 3) + 1, 2 * (n // 3) + 2, (n + 1) // 2, (n + 1) // 2 + 1)))
    # denormals and both zeros / a few infinities and NaNs that do not reach the rank / a wide spread of exponents
    den = _from_bits(rng.integers(0, 1 << 23, n).astype(np.uint32))
    den[: n // 4] = 0.0
    den[n // 4: n // 2] = -0.0
    few = normal(1.0)
    few[:7] = _f32([np.inf, -np.inf, np.nan, -np.nan, np.inf, np.nan, -np.inf])
    wide = (rng.standard_normal(n) * np.exp(rng.uniform(-40, 40, n))).astype(np.float32)
    cases.append(("denormals_few_specials_wide", np.stack([shuffled(den) * sign, shuffled(few), wide]),
                  ends + (n // 4, n // 2, n // 2 + 1, n - 8, n - 7, n - 6, quantile_rank(PERCENTILE, n))))
    # so many infinities and NaNs that q is inf or NaN at the ranks near the top: the fallback rows {F, 1}
    many_inf, many_nan, both = normal(3.0), normal(0.3), normal(1.0)
    many_inf[: n // 10] = np.inf * sign[: n // 10]
    many_nan[: n // 10] = np.nan
    both[: n // 20], both[n // 20: n // 10] = np.inf, _from_bits(np.full(n // 10 - n // 20, 0xFFC00001, np.uint32))
    cases.append(("many_specials", np.stack([shuffled(many_inf), shuffled(many_nan), shuffled(both)]),
                  ends + (n - n // 10, n - n // 10 + 1, n - n // 20, n - n // 20 + 1, quantile_rank(PERCENTILE, n))))
    # the issue's scales: standard normals times 0.3, 1 and 30
    cases.append(("normals", np.stack([normal(0.3), normal(1.0), normal(30.0)]), ends + (quantile_rank(0.5, n), quantile_rank(PERCENTILE, n))))
    for _, plane, _ in cases:
        assert plane.shape == (3, n) and plane.dtype == np.float32
        plane.setflags(write=False)
    return tuple(cases)
