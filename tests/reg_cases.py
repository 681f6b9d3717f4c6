"""The L2 weight regularizer and the sign transformer (train.py:47-48, 71-74, 80) restated in numpy, and the inputs of their tests.

The arithmetic is the one include/gct2.h defines for gct2_optimizer_apply_reg, gct2_grad_sumsq_l2 and gct2_l2_penalty, nothing
measured: all float32, every operation rounded once, in this order (g' = clip_cases.scaled, as every optimizer kernel forms it):
    c   = (float)(2.0 * (double)(float)l2)
    g_r = g' + c * p                 with p the parameter before the step; c == 0: g_r = g', nothing is added
    g_c = clip_cases.clip(g_r)       the norm modes read the float64 sum of squares of g_r
    g_t = g_c > 0 ? 1 : g_c < 0 ? -1 : g_c == 0 ? +0 : g_c          (GRAD_SIGN; GRAD_NONE: g_t = g_c)
    the kind's update on g_t:        clip_cases.adam / optimizer_cases.sgd / optimizer_cases.rmsprop, unchanged
    penalty = (float)((double)(float)l2 * S),  total = (float)((double)loss + (double)(float)l2 * S),  S = float64 sum of p^2
PARITY UNPINNED w.r.t. TensorFlow (there is none here)."""
import numpy as np

import clip_cases as K
import optimizer_cases as OC

F = np.float32
ADAM, SGD, RMSPROP = 0, OC.SGD, OC.RMSPROP          # GCT2_OPT_*
GRAD_NONE, GRAD_SIGN = 0, 1                         # GCT2_GRAD_*


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
def coefficient(l2):
    """c of the penalty gradient 2 l2 w: l2 held as float32, doubled in float64, rounded once"""
    return F(2.0 * float(F(l2)))


def regularized(gp, p, c):
    """g_r from g' and p (float32 arrays); c == 0 returns g' itself: the add is skipped, not computed"""
    gp = np.asarray(gp, dtype=F)
    if F(c) == 0:
        return gp
    with np.errstate(all="ignore"):
        return gp + F(c) * np.asarray(p, dtype=F)


def sign(x):
    """tf.sign: +-1, +0 for either zero, NaN stays NaN"""
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        return np.where(x > 0, F(1.0), np.where(x < 0, F(-1.0), np.where(x == 0, F(0.0), x))).astype(F)


def gradient(g, p, c=0.0, transform=GRAD_NONE, mode=K.CLIP_NONE, threshold=0.0, ss=None, grad_mul=1.0, inv_scale=1.0):
    """what the kind's update reads: penalty gradient, clipping, transformer - in Keras' order"""
    gc = K.clip(regularized(K.scaled(g, grad_mul, inv_scale), p, c), mode, threshold, ss)
    return sign(gc) if transform == GRAD_SIGN else gc


def update(kind, p, m, v, g2, lr, hyper):
    """(p, m, v) after the kind's step on the finished gradient g2; a slot the kind does not use comes back as it went in"""
    if kind == ADAM:
        return K.adam(p, m, v, g2, lr, hyper["beta_1"], hyper["beta_2"], hyper["epsilon"])
    if kind == SGD:
        p2, m2 = OC.sgd(p, m, g2, lr, hyper.get("momentum", 0.0), hyper.get("nesterov", False))
        return p2, m2, v
    return OC.rmsprop(p, m, v, g2, lr, hyper.get("rho", 0.9), hyper.get("momentum", 0.0), hyper.get("epsilon", 1e-7))


def apply(kind, p, m, v, g, lr, hyper, c=0.0, transform=GRAD_NONE, mode=K.CLIP_NONE, threshold=0.0, ss=None, grad_mul=1.0, inv_scale=1.0):
    """one gct2_optimizer_apply_reg over flat arrays"""
    return update(kind, p, m, v, gradient(g, p, c, transform, mode, threshold, ss, grad_mul, inv_scale), lr, hyper)


def regularized_sumsq(g, p, segs, coeffs, grad_mul=1.0, inv_scale=1.0):
    """gct2_grad_sumsq_l2: [float64 sum of g_r^2 over every (begin, count) segment with its own coefficient ..., their sum in order]"""
    gp = K.scaled(g, grad_mul, inv_scale)
    out = [K.sumsq(regularized(gp[b:b + n], p[b:b + n], c)) for (b, n), c in zip(segs, coeffs)]
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for s in out:
            total = total + s
    return np.array(out + [total], dtype=np.float64)


def penalty(loss, S, l2):
    """(penalty, total) of gct2_l2_penalty: the product and the sum in float64, each result rounded once to float32"""
    with np.errstate(all="ignore"):
        r = np.float64(F(l2)) * np.float64(S)
        return F(r), F(np.float64(F(loss)) + r)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def plant_zeros_and_cancellations(g, p, segs, c, factors):
    """in every segment long enough, overwrite the first elements of g and p (in place) so that the sign of a zero sum is pinned:
        [0] g = +0, p = -0   (+0 + -0 = +0)        [1] g = -0, p = -0   (-0 + -0 = -0, whose sign is +0)
        [2] g = -0, p = +1   (the penalty alone)   [3 + j] g = -(c * p) / factors[j]: g' = g * factors[j] cancels c * p exactly
    factors: the powers of two the tests scale g by (grad_mul, grad_mul * inv_scale).  Returns the positions of the cancellations."""
    at = []
    for b, n in segs:
        if n < 3 + len(factors):
            continue
        g[b], p[b] = F(0.0), F(-0.0)
        g[b + 1], p[b + 1] = F(-0.0), F(-0.0)
        g[b + 2], p[b + 2] = F(-0.0), F(1.0)
        for j, k in enumerate(factors):
            i = b + 3 + j
            g[i] = -(F(c) * p[i]) / F(k)
            assert F(g[i] * F(k)) + F(c) * p[i] == 0 and np.isfinite(g[i]) and g[i] != 0
            at.append(i)
    return at


def exact_parameters(rng, n):
    """integers times 2^-4 of magnitude at most 2^10, like clip_cases.exact_values"""
    return K.exact_values(rng, n)


def assert_exact_bound_l2(segs):
    """the 2^53 bound of gct2_grad_sumsq_l2 on exact_values / exact_parameters with c = 2^-2: x = g + p / 4 is an integer times 2^-6 of
    magnitude at most 2^10 + 2^8 = 1280, x^2 an integer times 2^-12 of at most 1280^2 * 2^12 units; every partial sum stays exact in
    float64 in ANY order while the total count of units stays below 2^53"""
    units = sum(n for _, n in segs) * 1280 * 1280 * (1 << 12)
    assert units < (1 << 53), units
    return units
