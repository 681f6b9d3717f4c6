"""Gradient clipping (Keras Adam(clipnorm / global_clipnorm / clipvalue) [TF]) restated in numpy, and the inputs of its tests.

The arithmetic is the one include/gct2.h defines for gct2_grad_sumsq and gct2_adam_keras_clipped, nothing measured:
    k   = fl32(inv_scale * grad_mul),  g' = fl32(g * k)                                   (as gct2_adam_keras_multi forms them)
    sumsq[s] = sum over segment s of (double)g'^2, every square and sum in float64;  sumsq[nseg] = their sum in segment order
    VALUE:        g'' = min(max(g', -clip), clip), NaN stays NaN
    NORM:         l2 = sumsq > 0 ? (float)sqrt(sumsq) : 1;  g'' = fl(fl(g' * clip) / max(l2, clip))
    GLOBAL_NORM:  nrm = (float)sqrt(sumsq);  scale = isfinite(nrm) ? fl(clip * min(1 / nrm, 1 / clip)) : NaN;  g'' = fl(g' * scale)
followed by Keras Adam in float32, every product, sum, quotient and root rounded once, in the order of adam_keras_update.
PARITY UNPINNED w.r.t. TensorFlow (there is none here): the formulas are those of tf.clip_by_norm / tf.clip_by_global_norm /
tf.clip_by_value as documented."""
import numpy as np

F = np.float32
CLIP_NONE, CLIP_VALUE, CLIP_NORM, CLIP_GLOBAL_NORM = 0, 1, 2, 3
CHUNK = 32768                       # GCT2_SUMSQ_CHUNK (tests compare it with the binding's constant)
MAX_SEGMENTS = 1024                 # GCT2_SUMSQ_MAX_SEGMENTS
ALIGN = 64                          # segments start at multiples of 64 elements, as tensors do in the engines' arenas
GUARD = 64                          # NaN elements in front of the first and behind the last segment
SEGMENT_LENGTHS = (1, 3, 4, 5, 63, 64, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7)


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
def scaled(g, grad_mul=1.0, inv_scale=1.0):
    """g' of the optimizer kernels: one float32 factor, one float32 product per element"""
    k = F(inv_scale) * F(grad_mul)
    with np.errstate(all="ignore"):
        return np.asarray(g, dtype=F) * k


def sumsq(gp):
    """float64 sum of the squares of float32 values (each square is exact in float64)"""
    x = np.asarray(gp, dtype=F).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.sum(x * x)


def segment_sumsq(gp, segs):
    """[sumsq of every (begin, count) segment ..., their sum in segment order] as float64"""
    out = [sumsq(gp[b:b + c]) for b, c in segs]
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for v in out:
            total = total + v
    return np.array(out + [total], dtype=np.float64)


def clip(gp, mode, threshold=0.0, ss=None):
    """g'' from g' (float32 array); ss: the ONE float64 sum of squares the two norm modes read"""
    gp = np.asarray(gp, dtype=F)
    c = F(threshold)
    with np.errstate(all="ignore"):
        if mode == CLIP_NONE:
            return gp
        if mode == CLIP_VALUE:
            return np.minimum(np.maximum(gp, -c), c)                 # numpy's minimum / maximum propagate NaN, as TensorFlow's
        ss = np.float64(ss)
        if mode == CLIP_NORM:
            l2 = F(np.sqrt(ss)) if ss > 0 else F(1.0)
            return (gp * c) / np.maximum(l2, c)
        if mode == CLIP_GLOBAL_NORM:
            nrm = F(np.sqrt(ss))
            scale = c * np.minimum(F(1.0) / nrm, F(1.0) / c) if np.isfinite(nrm) else F(np.nan)
            return gp * scale
    raise ValueError(mode)


def adam(p, m, v, g2, alpha, beta_1, beta_2, epsilon):
    """adam_keras_update in float32: (p, m, v) after one step on the (clipped) gradient g2"""
    p, m, v, g2 = (np.asarray(a, dtype=F) for a in (p, m, v, g2))
    alpha, b1, b2, eps = F(alpha), F(beta_1), F(beta_2), F(epsilon)
    ob1, ob2 = F(1.0) - b1, F(1.0) - b2
    with np.errstate(all="ignore"):
        m = b1 * m + ob1 * g2
        v = b2 * v + (ob2 * g2) * g2
        p = p - (alpha * m) / (np.sqrt(v) + eps)
    return p, m, v


def clipped_adam(p, m, v, g, alpha, beta_1, beta_2, epsilon, mode, threshold, ss=None, grad_mul=1.0, inv_scale=1.0):
    return adam(p, m, v, clip(scaled(g, grad_mul, inv_scale), mode, threshold, ss), alpha, beta_1, beta_2, epsilon)


def clip_arena(g, segs, mode, threshold, grad_mul=1.0, inv_scale=1.0):
    """what an engine's clipped step feeds to Adam over a whole gradient arena: VALUE and GLOBAL_NORM over every element (padding
    included - it is zero), NORM per tensor over exactly its elements (elements outside every segment get no update: NaN here, so that
    a caller who used them would notice)"""
    gp = scaled(g, grad_mul, inv_scale)
    if mode in (CLIP_NONE, CLIP_VALUE):
        return clip(gp, mode, threshold)
    ss = segment_sumsq(gp, segs)
    if mode == CLIP_GLOBAL_NORM:
        return clip(gp, mode, threshold, ss[-1])
    out = np.full(gp.shape, np.nan, dtype=F)
    for s, (b, c) in enumerate(segs):
        out[b:b + c] = clip(gp[b:b + c], mode, threshold, ss[s])
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def layout(lengths=SEGMENT_LENGTHS, align=ALIGN, guard=GUARD):
    """[(begin, count)] at `align`-aligned starts behind `guard` leading elements, and the buffer length with `guard` trailing ones"""
    segs, at = [], guard
    for n in lengths:
        at = (at + align - 1) // align * align
        segs.append((at, n))
        at += n
    return segs, (at + align - 1) // align * align + guard


def partial_counts(segs):
    return [(c + CHUNK - 1) // CHUNK for _, c in segs]


def poisoned(values_of, segs, total):
    """a float32 buffer that is NaN everywhere (gaps, alignment padding, both guards) except inside the segments"""
    buf = np.full(total, np.nan, dtype=F)
    for s, (b, c) in enumerate(segs):
        buf[b:b + c] = values_of(s, c)
    return buf


def exact_values(rng, n):
    """integers times 2^-4 of magnitude at most 2^10: every square is an integer times 2^-8 below 2^20, and every partial sum of a
    segment or of all segments an integer times 2^-8 - exact in float64 in ANY order as long as it stays below 2^53 * 2^-8"""
    return (rng.integers(-(1 << 14), (1 << 14) + 1, size=n).astype(np.float64) * 2.0 ** -4).astype(F)


def assert_exact_bound(segs):
    """the 2^53 bound of exact_values: total count * (2^14)^2 integer units of 2^-8 must stay below 2^53"""
    units = sum(c for _, c in segs) * (1 << 28)
    assert units < (1 << 53), units
    return units
