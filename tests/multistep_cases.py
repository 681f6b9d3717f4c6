"""Host references and case tables of the second-order multistep sampler (a plain helper module: no fixtures, no GPU):
gct2_diffusion_step_multistep restated from include/gct2.h in float32, one rounding per numpy operation, on top of
generate_cases / img2img_cases; one DPM-Solver++ 2M step in float64 written from the paper's form (Lu, Zhou, Bao, Chen, Li, Zhu,
"DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models", 2022, algorithm 2) and in the kernel's extrapolated
form; a Gaussian data model whose optimal denoiser and probability-flow solution are closed-form, and the runs over it that
measure a solver's order of accuracy; the cases of tests/test_multistep_kernels_gpu.py.
"""
import functools
import math

import numpy as np

import generate_cases as G
import img2img_cases as I
from oracle import denoiser_oracle as O
from pointwise_cases import SAMPLE_EPS, SAMPLE_X

# ---- the cases of tests/test_multistep_kernels_gpu.py ----------------------------------------------------------------------------------
C1S = (0.0, 0.5, 1.37)                                 # no extrapolation, uniform spacing in lambda, a value that is no power of two
CLIPS = (0.0,) + tuple(G.CLIPS)                        # off, 1.0, 0.5


@functools.lru_cache(maxsize=None)
def hist_case(images, per_image):
    """the estimate of the step before, float32 [images, per_image]: standard normals (as far from x as two independent draws are)"""
    rng = np.random.default_rng([images, per_image, 59])
    h = rng.standard_normal((images, per_image)).astype(np.float32)
    h.setflags(write=False)
    return h


def step_inputs(shape):
    """(pred, fake) of a shape (B, npix, C): generate_cases.clip_case (CLIP_SPECIALS planted in pred) where it has that shape's images,
    plain standard normals for the long one-image shape"""
    B, npix, C = shape
    return G.clip_case(npix) if (B, C) == (G.B, G.C) else G.step_case(B, npix * C)


# ---- float32 restatement -----------------------------------------------------------------------------------------------------------------

def _f32(a):
    return np.asarray(a, dtype=np.float32)


def multistep_step_f32(mode, pred, fake, hist, a_t, a_prev, c1, clip, known=None, mask_el=None, z0=None):
    """gct2_diffusion_step_multistep as include/gct2.h states it, every operation rounded to float32 on its own.  hist: hist_in (not
    read at (float)c1 == 0: may be None).  known, mask_el (the mask per ELEMENT, img2img_cases.per_element) and z0 (the starting noise's
    draws) select the masked form.  Returns (fake', x0_out, hist_out)."""
    with np.errstate(all="ignore"):
        p, f = _f32(pred), _f32(fake)
        x, e = G._estimate(mode, p, f, a_t, clip)
        sa, sb, cx, ce, _ = G.step_coefficients(a_t, a_prev, 0.0)
        c = np.float32(c1)
        if c == 0:
            g = cx * x + ce * e
        else:
            d = x + c * (x - _f32(hist))
            ed = (f - sa * d) / sb
            g = cx * d + ce * ed
        assert g.dtype == np.float32 and x.dtype == np.float32
        if known is None:
            return g, x, x
        h = I.kept_f32(known, a_prev, z0)
        return I.blend_f32(mask_el, g, h), I.blend_f32(mask_el, x, _f32(known)), x


def multistep_step_fused(mode, pred, fake, hist, a_t, a_prev, c1, clip):
    """a contracted form of the extrapolation - what the kernel must NOT compute: d = fma(c, x - hist, x)"""
    with np.errstate(all="ignore"):
        p, f = _f32(pred), _f32(fake)
        x, _ = G._estimate(mode, p, f, a_t, clip)
        sa, sb, cx, ce, _ = G.step_coefficients(a_t, a_prev, 0.0)
        c = np.float32(c1)
        d = (x.astype(np.float64) + np.float64(c) * (x - _f32(hist)).astype(np.float64)).astype(np.float32)
        ed = (f - sa * d) / sb
        return cx * d + ce * ed, x, x


# ---- float64 references ------------------------------------------------------------------------------------------------------------------

def half_log_snr(a):
    return 0.5 * math.log(a / (1.0 - a))


def dpm2m_step_paper_f64(x_t, x0, x0_prev, a_before, a_t, a_prev):
    """one DPM-Solver++ 2M step as the paper writes it (algorithm 2), in float64, alpha = sqrt(a), sigma = sqrt(1 - a),
    lambda = log(alpha / sigma): h = lambda' - lambda, r = h_prev / h, D = (1 + 1 / (2 r)) x0 - 1 / (2 r) x0_prev, and
    x' = (sigma' / sigma) x - alpha' (exp(-h) - 1) D.  x0_prev None: the first-order step, D = x0"""
    x_t, x0 = np.asarray(x_t, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    h = half_log_snr(a_prev) - half_log_snr(a_t)
    if x0_prev is None:
        D = x0
    else:
        r = (half_log_snr(a_t) - half_log_snr(a_before)) / h
        D = (1.0 + 1.0 / (2.0 * r)) * x0 - 1.0 / (2.0 * r) * np.asarray(x0_prev, dtype=np.float64)
    return math.sqrt(1.0 - a_prev) / math.sqrt(1.0 - a_t) * x_t - math.sqrt(a_prev) * math.expm1(-h) * D


def dpm2m_step_extrapolated_f64(x_t, x0, x0_prev, c1, a_t, a_prev):
    """the form the kernel computes, in float64: D = x0 + c1 (x0 - x0_prev), then the DDIM re-noising of D with eps re-derived from it,
    cx D + ce (x - sa D) / sb"""
    x_t, x0 = np.asarray(x_t, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    D = x0 if x0_prev is None else x0 + c1 * (x0 - np.asarray(x0_prev, dtype=np.float64))
    return math.sqrt(a_prev) * D + math.sqrt(1.0 - a_prev) * (x_t - math.sqrt(a_t) * D) / math.sqrt(1.0 - a_t)


# ---- the Gaussian data model: the integrator's order of accuracy, exactly ---------------------------------------------------------------------
# data x0 ~ N(mu, s^2) per element.  Then x_t ~ N(sqrt(a) mu, a s^2 + 1 - a), the optimal denoiser E[x0 | x_t] is linear in x_t, and the
# probability-flow ODE keeps every sample at its quantile: (x(a) - sqrt(a) mu) / sqrt(a s^2 + 1 - a) is constant along a trajectory.
ORDER_STEPS = 200                                      # the quadratic schedule at the reference's step count
ORDER_LOW, ORDER_HIGH = 20, 200                        # the runs connect the states at these two timesteps
ORDER_STRIDES = (20, 10, 5)                            # 10, 19 and 37 timesteps
ORDER_SHAPE = (2, 5, 3)                                # B images of 5 pixels x 3 channels
ORDER_MODES = (SAMPLE_X, SAMPLE_EPS)
ORDER_SEED = 61
# the issue's three conditions, on the max-abs errors E1 (every c1 = 0) and E2 (multistep_coefficient) at 19 and 37 timesteps
ORDER_FIRST_RATIO_MAX, ORDER_SECOND_RATIO_MIN = 2.3, 3.0


def order_alpha(t):
    return float(O.alpha_dash(t, ORDER_STEPS))


def order_timesteps(d):
    return list(range(ORDER_LOW, ORDER_HIGH + 1, d))


@functools.lru_cache(maxsize=None)
def gaussian_case():
    """(mu in [-0.5, 0.5], s in [0.2, 0.8], x_T): float64 [B, per_image]; x_T is a sample of the marginal at t = ORDER_HIGH"""
    rng = np.random.default_rng(ORDER_SEED)
    B, npix, C = ORDER_SHAPE
    mu, s = rng.uniform(-0.5, 0.5, (B, npix * C)), rng.uniform(0.2, 0.8, (B, npix * C))
    a = order_alpha(ORDER_HIGH)
    x_T = math.sqrt(a) * mu + np.sqrt(a * s * s + 1.0 - a) * rng.standard_normal((B, npix * C))
    for v in (mu, s, x_T):
        v.setflags(write=False)
    return mu, s, x_T


def exact_flow(a, a_T, x_T, mu, s):
    """the probability-flow ODE's solution at alpha a through x_T at alpha a_T, float64"""
    return math.sqrt(a) * mu + np.sqrt((a * s * s + 1.0 - a) / (a_T * s * s + 1.0 - a_T)) * (x_T - math.sqrt(a_T) * mu)


def denoiser_gain(a, s):
    """sqrt(a) s^2 / (a s^2 + 1 - a), float64 [B, per_image]: the optimal denoiser is mu + gain (x_t - sqrt(a) mu)"""
    return math.sqrt(a) * s * s / (a * s * s + 1.0 - a)


def order_schedule(d, ascending, second, coefficient):
    """the steps of one run: [(t, a_t, a_prev, c1)] in the order they are taken.  Descending from ORDER_HIGH to ORDER_LOW (ascending: the
    other way) over order_timesteps(d); every step goes to the next timestep's alpha; c1 = coefficient(alpha of the timestep evaluated
    before, a_t, a_prev) when `second`, with None at the first step, else 0"""
    ts = order_timesteps(d)
    if not ascending:
        ts = ts[::-1]
    out = []
    for k in range(len(ts) - 1):
        a_t, a_prev = order_alpha(ts[k]), order_alpha(ts[k + 1])
        c1 = coefficient(order_alpha(ts[k - 1]) if k else None, a_t, a_prev) if second else 0.0
        out.append((ts[k], a_t, a_prev, c1))
    return out


def order_ends(ascending):
    """(start, exact end) of a run, float64: the exact states at ORDER_HIGH and ORDER_LOW of the trajectory through gaussian_case's x_T"""
    mu, s, x_T = gaussian_case()
    a_T = order_alpha(ORDER_HIGH)
    x_low = exact_flow(order_alpha(ORDER_LOW), a_T, x_T, mu, s)
    return (x_low, x_T) if ascending else (x_T, x_low)


def order_prediction(mode, fake, a_t, mu, gain):
    """the network's output for the state `fake` at alpha a_t: the optimal x0 (SAMPLE_X), or the eps that goes with it
    (fake - sa x0) / sb (SAMPLE_EPS).  Array operations only: numpy float32 arrays on the host, torch tensors on the device - mu and
    gain are in the array type of fake"""
    sa, sb = math.sqrt(a_t), math.sqrt(1.0 - a_t)
    x0 = mu + gain * (fake - sa * mu)
    return x0 if mode == SAMPLE_X else (fake - sa * x0) / sb


def order_error_f32(mode, d, ascending, second, coefficient, step=multistep_step_f32):
    """the max-abs error of one run of the float32 restatement against the exact flow"""
    mu, s, _ = gaussian_case()
    start, end = order_ends(ascending)
    fake, hist = _f32(start), None
    for _, a_t, a_prev, c1 in order_schedule(d, ascending, second, coefficient):
        pred = order_prediction(mode, fake, a_t, _f32(mu), _f32(denoiser_gain(a_t, s)))
        assert pred.dtype == np.float32
        fake, _, hist = step(mode, pred, fake, hist, a_t, a_prev, c1, 0.0)
    return float(np.abs(fake.astype(np.float64) - end).max())


def order_conditions(E1, E2):
    """the three conditions on {timesteps: error} of the first-order (E1) and the second-order (E2) runs; returns the figures"""
    r1, r2 = E1[19] / E1[37], E2[19] / E2[37]
    assert r1 <= ORDER_FIRST_RATIO_MAX, (r1, E1, E2)                 # halving the step halves the first-order error
    assert r2 >= ORDER_SECOND_RATIO_MIN, (r2, E1, E2)                # and takes the second-order error down by more than 3 (4 in the limit)
    assert E2[19] < E1[37], (E1, E2)                                 # half the evaluations, and still the smaller error
    return r1, r2
