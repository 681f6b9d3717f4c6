"""Host references of the v objective and of the weighted objective loss (a plain helper module: no fixtures, no GPU): float32
restatements of include/gct2.h, one rounding per numpy operation like tests/generate_cases.py's - gct2_diffusion_update's mode V
(v_update), the step kernels around it (v_step_f32, v_multistep_f32), gct2_objective_loss_fwd_bwd (objective_loss_reference) - and
the closed forms of the min-SNR-gamma weights (min_snr_weights).
"""
import itertools

import numpy as np

import generate_cases as G

SAMPLE_V = 5
MSE, L1 = 0, 1
KINDS = (MSE, L1)
KIND_IDS = ("mse", "l1")
# the loss kernel's tile: a work-group covers 256 threads x 4 groups x 4 floats = 4096 elements of ONE image (csrc/loss_kernels.hip,
# eval_chunks): (2,40,40,3) has n_img = 4800, two work-groups per image
TILE = 4096
LOSS_SHAPES = [(3, 5, 7, 3), (1, 1, 1, 1), (2, 16, 16, 3), (2, 40, 40, 3)]
assert LOSS_SHAPES[-1][1] * LOSS_SHAPES[-1][2] * LOSS_SHAPES[-1][3] > TILE
LOSS_SCALES = (1.0, 1024.0)


def presence_combinations():
    """every legal presence combination of (a, c, eps, w, lam) as a tuple of five bools: c needs eps, and a with eps needs c; eps or c
    without a are legal and ignored (the target is x)"""
    out = []
    for a, c, eps, w, lam in itertools.product((False, True), repeat=5):
        if c and not eps:
            continue
        if a and eps and not c:
            continue
        out.append((a, c, eps, w, lam))
    return out


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def roots(a_t):
    """(sa, sb) float32: the square roots in double, one cast each"""
    return np.float32(np.sqrt(np.float64(a_t))), np.float32(np.sqrt(1.0 - np.float64(a_t)))


def v_update(pred, fake, a_t):
    """gct2_diffusion_update(GCT2_SAMPLE_V): x = fl(fl(sa f) - fl(sb p)), e = fl(fl(sb f) + fl(sa p))"""
    p, f = _f32(pred), _f32(fake)
    sa, sb = roots(a_t)
    with np.errstate(all="ignore"):
        x = sa * f - sb * p
        e = sb * f + sa * p
    assert x.dtype == np.float32 and e.dtype == np.float32
    return x, e


def v_estimate(pred, fake, a_t, clip):
    """(x, e) of the step kernels in mode V: v_update, then the clip of x with e re-derived from it"""
    x, e = v_update(pred, fake, a_t)
    if clip > 0:
        sa, sb = roots(a_t)
        c = np.float32(clip)
        with np.errstate(all="ignore"):
            x = np.where(x < -c, -c, np.where(x > c, c, x)).astype(np.float32)
            e = (_f32(fake) - sa * x) / sb
    return x, e


def v_step_f32(pred, fake, a_t, a_prev, clip):
    """gct2_diffusion_step in mode V at sigma2 = 0: (fake', x)"""
    with np.errstate(all="ignore"):
        x, e = v_estimate(pred, fake, a_t, clip)
        _, _, cx, ce, _ = G.step_coefficients(a_t, a_prev, 0.0)
        out = cx * x + ce * e
    assert out.dtype == np.float32
    return out, x


def v_multistep_f32(pred, fake, hist, a_t, a_prev, c1, clip):
    """gct2_diffusion_step_multistep in mode V, the plain form: (fake', x0_out = hist_out)"""
    with np.errstate(all="ignore"):
        f = _f32(fake)
        x, e = v_estimate(pred, f, a_t, clip)
        sa, sb, cx, ce, _ = G.step_coefficients(a_t, a_prev, 0.0)
        c = np.float32(c1)
        if c == 0:
            return cx * x + ce * e, x
        d = x + c * (x - _f32(hist))
        ed = (f - sa * d) / sb
        return cx * d + ce * ed, x


def objective_loss_reference(kind, pred, x, eps=None, a=None, c=None, w=None, lam=None, s=1.0):
    """gct2_objective_loss_fwd_bwd restated: pred, x, eps [B,H,W,C]; a, c, w, lam [B] or None.  Returns (d float32, dpred float32,
    loss as a Python float in double - the caller casts it once).  Every float32 operation is one numpy operation."""
    p, xx = _f32(pred), _f32(x)
    B = p.shape[0]
    n = p.size
    col = lambda v: _f32(v).reshape(B, 1, 1, 1)
    with np.errstate(all="ignore"):
        t = xx
        if a is not None:
            t = col(a) * xx
            if eps is not None:
                t = t + col(c) * _f32(eps)
        pp = col(w) * p if w is not None else p
        d = t - pp
        assert d.dtype == np.float32
        if lam is not None and w is not None:
            g = col(lam) * col(w)
        else:
            g = col(lam) if lam is not None else (col(w) if w is not None else None)
        d64 = d.astype(np.float64)
        if kind == MSE:
            per = (d64 * d64).reshape(B, -1).sum(axis=1)
            grad = d * np.float32(-2.0 / n)
        else:
            first = d >= -d
            per = np.where(first, d, -d).astype(np.float64).reshape(B, -1).sum(axis=1)
            k1 = np.float32(1.0 / n)
            grad = np.where(first, -k1, k1).astype(np.float32)
        if g is not None:
            grad = grad * g
        dpred = np.float32(s) * grad
        assert dpred.dtype == np.float32
        lam64 = np.ones(B) if lam is None else _f32(lam).astype(np.float64)
        loss = float((lam64 * per).sum() / n)
    return d, dpred, loss


def objective_loss_f64(kind, pred, x, eps, a, c, w, lam):
    """the same loss as a smooth function in float64 (no float32 rounding): what the finite differences differentiate"""
    p, xx = np.asarray(pred, np.float64), np.asarray(x, np.float64)
    B, n = p.shape[0], p.size
    col = lambda v: np.asarray(v, np.float64).reshape(B, 1, 1, 1)
    d = col(a) * xx + col(c) * np.asarray(eps, np.float64) - col(w) * p
    per = (d * d if kind == MSE else np.abs(d)).reshape(B, -1).sum(axis=1)
    return float((np.asarray(lam, np.float64) * per).sum() / n)


def min_snr_weights(alpha, gamma, objective):
    """the closed forms of min-SNR-gamma over an array of alphas (float64): x: min(SNR, g); eps: min(SNR, g) / SNR written without the
    0 / 0; v: min(SNR, g) / (SNR + 1)"""
    a = np.asarray(alpha, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = np.where(a >= 1.0, np.inf, a / (1.0 - a))
        clipped = np.minimum(snr, gamma)
        if objective == "x":
            return clipped, snr
        if objective == "eps":
            return np.where(snr <= gamma, 1.0, gamma / snr), snr
        return np.where(np.isinf(snr), 0.0, clipped / (snr + 1.0)), snr


def loss_inputs(shape, seed=0, integers=False):
    """pred, x, eps [B,H,W,C] and a, c, w, lam [B], float32.  integers: small integers (and powers of two for the vectors), so that
    every product and every sum is exact in float32 and in float64"""
    rng = np.random.default_rng([seed, *shape])
    B = shape[0]
    if integers:
        planes = [rng.integers(-8, 9, shape).astype(np.float32) for _ in range(3)]
        vecs = [rng.choice([0.5, 1.0, 2.0, -1.0], B).astype(np.float32) for _ in range(3)] + [rng.choice([0.5, 1.0, 2.0, 4.0], B).astype(np.float32)]
    else:
        planes = [rng.standard_normal(shape).astype(np.float32) for _ in range(3)]
        vecs = [rng.uniform(-1.5, 1.5, B).astype(np.float32) for _ in range(3)] + [rng.uniform(0.05, 3.0, B).astype(np.float32)]
    return dict(zip(("pred", "x", "eps", "a", "c", "w", "lam"), planes + vecs))
