"""Host references and case tables of image-conditioned generation (a plain helper module: no fixtures, no GPU):
gct2_diffusion_start_image and gct2_diffusion_step_masked restated from include/gct2.h in float32, one rounding per numpy operation,
on top of generate_cases.diffusion_step_f32; the contracted blends the kernel must NOT compute; the blended step, the masked sampler
and the inversion loop in float64; the mask cases of tests/test_img2img_kernels_gpu.py.
"""
import functools

import numpy as np

import generate_cases as G
from oracle import denoiser_oracle as O

# the per-pixel pattern: kept, regenerated, two blends, below 0 and above 1 (act as 0 and 1), a value that underflows against 1 and a NaN
PATTERN = (0.0, 1.0, 0.5, 0.25, -0.5, 1.5, 1e-30, float("nan"))
# between the two ends the pattern mask also draws these: m g is exact for a power of two m, so fma(m, g, .) cannot differ from the
# unfused blend at 0.5 / 0.25 - at 0.3 and 0.7 both contracted forms can
INTERIOR = (0.3, 0.7)
MASK_KINDS = ("pattern", "ones", "zeros", "half")


def _f32(a):
    return np.asarray(a, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def mask_case(kind, images, npix):
    """float32 [images, npix], one value per pixel: PATTERN at the start and at the end of every image (random values of PATTERN
    and INTERIOR between), all ones, all zeros, or the first half of every image kept and the second regenerated"""
    if kind == "ones":
        m = np.ones((images, npix), np.float32)
    elif kind == "zeros":
        m = np.zeros((images, npix), np.float32)
    elif kind == "half":
        m = np.zeros((images, npix), np.float32)
        m[:, npix // 2:] = 1.0
    else:
        assert kind == "pattern"
        rng = np.random.default_rng([images, npix, 47])
        m = np.float32(PATTERN + INTERIOR)[rng.integers(0, len(PATTERN) + len(INTERIOR), (images, npix))]
        if npix >= 2 * len(PATTERN):                    # (images of a pixel or two keep their random values)
            m[:, :len(PATTERN)] = np.float32(PATTERN)
            m[:, -len(PATTERN):] = np.float32(PATTERN)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def known_case(images, per_image):
    """the clean images, float32 [images, per_image] in [-1, 1)"""
    rng = np.random.default_rng([images, per_image, 53])
    k = (np.floor(rng.uniform(0, 256, (images, per_image))) / 128 - 1).astype(np.float32)
    k.setflags(write=False)
    return k


def per_element(mask, C):
    """[images, npix] -> [images, npix * C]: a pixel's value for each of its C channels"""
    return np.repeat(_f32(mask), C, axis=1)


# ---- float32 restatements --------------------------------------------------------------------------------------------------------------

def start_image_f32(known, a, z0):
    """gct2_diffusion_start_image: A = (float)a, cx = sqrtf(A), ck = sqrtf(1.f - A), fake = cx known + ck z0"""
    A = np.float32(a)
    cx, ck = np.sqrt(A), np.sqrt(np.float32(1.0) - A)
    out = cx * _f32(known) + ck * _f32(z0)
    assert out.dtype == np.float32
    return out


def kept_f32(known, a_prev, z0):
    """h of gct2_diffusion_step_masked: the same formula at a_prev"""
    return start_image_f32(known, a_prev, z0)


def _select(m, g, h, blend):
    with np.errstate(all="ignore"):
        return np.where(m >= 1, g, np.where(m <= 0, h, blend)).astype(np.float32)


def blend_f32(m, g, h):
    """m >= 1 ? g : (m <= 0 ? h : m g + (1.f - m) h), every operation rounded on its own; a NaN m fails both comparisons and blends"""
    m, g, h = _f32(m), _f32(g), _f32(h)
    with np.errstate(all="ignore"):
        b = m * g + (np.float32(1.0) - m) * h
    assert b.dtype == np.float32
    return _select(m, g, h, b)


def blend_fused(m, g, h, term=0):
    """the contracted blends - what the kernel must NOT compute: term 0 is fma(m, g, fl((1 - m) h)), term 1 is fma(1 - m, h, fl(m g))
    (a product of two float32 values is exact in float64)"""
    m, g, h = _f32(m), _f32(g), _f32(h)
    with np.errstate(all="ignore"):
        om = np.float32(1.0) - m
        if term == 0:
            b = (m.astype(np.float64) * g.astype(np.float64) + (om * h).astype(np.float64)).astype(np.float32)
        else:
            b = ((m * g).astype(np.float64) + om.astype(np.float64) * h.astype(np.float64)).astype(np.float32)
    return _select(m, g, h, b)


def step_masked_f32(mode, pred, fake, known, mask_el, a_t, a_prev, s2, clip, z0, z=None, blend=blend_f32):
    """gct2_diffusion_step_masked as include/gct2.h states it.  mask_el: the mask per ELEMENT (per_element).  Returns (fake', x0)."""
    g, x = G.diffusion_step_f32(mode, pred, fake, a_t, a_prev, s2, clip, z)
    h = kept_f32(known, a_prev, z0)
    return blend(mask_el, g, h), blend(mask_el, x, _f32(known))


# ---- float64 references ------------------------------------------------------------------------------------------------------------------

def blend_f64(m, g, h):
    m = np.clip(np.asarray(m, dtype=np.float64), 0.0, 1.0)
    return np.where(m >= 1, g, np.where(m <= 0, h, m * g + (1.0 - m) * h))


def step_masked_f64(mode, pred, fake, known, mask_el, a_t, a_prev, s2, clip, z0, z=None):
    """the blended step in float64 (finite inputs, no NaN mask): (fake', x0)"""
    g, x = G.ddim_step_f64(mode, pred, fake, a_t, a_prev, s2, clip, z)
    kn = np.asarray(known, dtype=np.float64)
    h = np.sqrt(a_prev) * kn + np.sqrt(1.0 - a_prev) * np.asarray(z0, dtype=np.float64)
    return blend_f64(mask_el, g, h), blend_f64(mask_el, x, kn)


def masked_sample_f64(denoise, known, mask_el, z0, taus, steps, mode, run=None, eta=0.0, clip=0.0, z=None):
    """generate(init=known, mask=...) in float64: `denoise(fake, t)` is the network, taus the K ascending timesteps, `run` how many of
    them are visited (the K' last of the sampling order; None: all), z0 the starting noise, z[k] the noise of step k of the FULL
    schedule (0-based, sampling order: the step at taus[K - 1 - k]).  Returns the composited x0 of the last step."""
    K = len(taus)
    run = K if run is None else run
    kn, z0 = np.asarray(known, dtype=np.float64), np.asarray(z0, dtype=np.float64)
    a0 = float(O.alpha_dash(taus[run - 1], steps))
    fake = np.sqrt(a0) * kn + np.sqrt(1.0 - a0) * z0
    x0 = None
    for k in range(K - run, K):
        tau = taus[K - 1 - k]
        a_t = float(O.alpha_dash(tau, steps))
        a_prev = float(O.alpha_dash(taus[K - 2 - k] if k < K - 1 else 0, steps))
        s2 = G.sigma2(a_t, a_prev, eta)
        fake, x0 = step_masked_f64(mode, denoise(fake, tau), fake, kn, mask_el, a_t, a_prev, s2, clip, z0, None if z is None else z[k])
    return x0


def invert_f64(denoise, images, taus, steps, mode, start_eps=None):
    """encode in float64: the forward loop of train.py:364-413 over the ascending timesteps taus.  x = images, e = images (or start_eps);
    per step fake = sqrt(a) x + sqrt(1 - a) e, one evaluation, then x and e by objective.  Returns the last e: the latent."""
    x = np.asarray(images, dtype=np.float64)
    e = x if start_eps is None else np.asarray(start_eps, dtype=np.float64)
    for tau in taus:
        a = float(O.alpha_dash(tau, steps))
        fake = np.sqrt(a) * x + np.sqrt(1.0 - a) * e
        # (a_prev = 1, sigma2 = 0: ddim_step_f64's second result is x0; eps follows from it)
        _, x = G.ddim_step_f64(mode, denoise(fake, tau), fake, a, 1.0, 0.0, 0.0)
        e = (fake - np.sqrt(a) * x) / np.sqrt(1.0 - a)
    return e
