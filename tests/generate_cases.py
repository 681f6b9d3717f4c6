"""Host references and case tables of generation (a plain helper module: no fixtures, no GPU): gct2_diffusion_step restated from
include/gct2.h in float32, one rounding per numpy operation like tests/pointwise_cases.py's restatements; the same step in float64
from the DDIM paper's eq. 12 (Song, Meng, Ermon, "Denoising Diffusion Implicit Models", ICLR 2021); the shapes, offsets and inputs
of tests/test_generate_kernels_gpu.py.
"""
import functools

import numpy as np

import pointwise_cases as P
from oracle import denoiser_oracle as O
from pointwise_cases import SAMPLE_EPS, SAMPLE_SCALED_EPS, SAMPLE_X

MODES = [SAMPLE_X, SAMPLE_EPS, SAMPLE_SCALED_EPS]
MODE_IDS = ["x", "eps", "scaled_eps"]

# ---- the cases of tests/test_generate_kernels_gpu.py ----------------------------------------------------------------------------------
B, C = 3, 3
NPIXS = (1003, 1024)                                   # per_image = 3009 (not a multiple of 4: every image starts elsewhere in a counter) / 3072
# one length past the grid cap of 2048 work-groups of 256: the second trip of the one-element-per-thread loop (sigma^2 = 0).  525319 is
# no multiple of 3, so the long case is one image of 525319 one-channel pixels (B, npix, C)
LONG_SHAPE = (1, P.NORMAL_LONG_N, 1)
SHAPES = [(B, NPIXS[0], C), (B, NPIXS[1], C), LONG_SHAPE]
SHAPE_IDS = ["3x1003x3", "3x1024x3", "1x525319x1"]
LDOUT, LDOUT2 = 4, 67
# the with-noise kernel walks one image per blockIdx.y and a Philox counter (four elements) per thread, 2048 work-groups at the most:
# more images than work-groups (the image loop's second trip), and one image of more than 2048 x 256 counters (the counter loop's)
MANY_IMAGES_SHAPE = (2051, 1, 3)
LONG_RNG_SHAPE = (1, 4 * 2048 * 256 + 1031, 1)
# the with-noise kernel's four-element form (16-byte accesses): taken when the planes are 16-byte aligned and offset, image_stride and
# per_image are multiples of 4 (what generate passes): images back to back, from 0 and from two counters in front of the wrap of the low
# counter word; its counter loop's second trip needs an image of more than 4 x 2048 x 256 elements, a multiple of 4
LONG_VEC_SHAPE = (1, 4 * 2048 * 256 + 1028, 1)
ALIGNED_OFFSETS = (0, P.CARRY - 2)
assert all(o % 4 == 0 for o in ALIGNED_OFFSETS) and LONG_VEC_SHAPE[1] % 4 == 0
OFFSETS = P.OFFSETS                                   # 0, 1, 2, 3, 5 and CARRY (the low counter word wraps inside the draw)
SEED, SID = P.SEEDS[-1]
ETAS = (0.7, 1.0)
CLIPS = (1.0, 0.5)


def image_stride(per_image):
    """images per_image + 5 apart (+ 6 where that is a multiple of 4): image b starts at another lane of its counter than image b - 1"""
    s = per_image + 5
    return s + 1 if s % 4 == 0 else s


def alphas(t):
    """(a_t, a_prev) of one step of the full schedule at steps = 200: Python floats, as the sampler forms them"""
    return P.diffusion_alphas(t)


def sigma2(a_t, a_prev, eta):
    """trainer_math.ddim_sigma2 restated: eta^2 (1 - a_prev) / (1 - a_t) (1 - a_t / a_prev), clamped to [0, 1 - a_prev]"""
    s = eta * eta * (1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev)
    return min(max(s, 0.0), 1.0 - a_prev)


@functools.lru_cache(maxsize=None)
def step_case(images, per_image):
    """(pred, fake) float32 [images, per_image]: standard normals"""
    rng = np.random.default_rng([images, per_image, 41])
    arrs = tuple(rng.standard_normal((images, per_image)).astype(np.float32) for _ in range(2))
    for v in arrs:
        v.setflags(write=False)
    return arrs


CLIP_SPECIALS = (2.0, -2.0, 1.0, -1.0, 0.5, -0.5, float("nan"), float("inf"), -float("inf"), 0.75, 1.0000001, -1.0000001)


@functools.lru_cache(maxsize=None)
def clip_case(npix=NPIXS[0]):
    """step_case with CLIP_SPECIALS planted in pred at the start of every image and at its end: in X mode x = pred, so the estimate lies
    beyond both bounds of CLIPS, on them, just past them, is a NaN and both infinities; in the epsilon modes the division by
    sqrt(a_t) <= 0.5 puts most estimates beyond the bounds, and the planted NaN / infinities reach x through (f - p sb) / sa"""
    pred, fake = (a.copy() for a in step_case(B, npix * C))
    k = len(CLIP_SPECIALS)
    pred[:, :k] = np.float32(CLIP_SPECIALS)
    pred[:, -k:] = np.float32(CLIP_SPECIALS)
    pred.setflags(write=False)
    fake.setflags(write=False)
    return pred, fake


# ---- float32 restatement -----------------------------------------------------------------------------------------------------------------

def _f32(a):
    return np.asarray(a, dtype=np.float32)


def step_coefficients(a_t, a_prev, s2):
    """(sa, sb, cx, ce, cz) float32: sa, sb square roots in double cast once; cx, ce, cz float32 square roots of float32 values"""
    sa, sb = np.float32(np.sqrt(np.float64(a_t))), np.float32(np.sqrt(1.0 - np.float64(a_t)))
    A, S = np.float32(a_prev), np.float32(s2)
    cx, ce, cz = np.sqrt(A), np.sqrt((np.float32(1.0) - A) - S), np.sqrt(S)
    assert all(v.dtype == np.float32 for v in (sa, sb, cx, ce, cz))
    return sa, sb, cx, ce, cz


def _estimate(mode, p, f, a_t, clip):
    """(x, e) float32: gct2_diffusion_update's, then the clip of x with e re-derived from it"""
    x, e = P.diffusion_update_f32(mode, p, f, a_t, 0.0)
    if clip > 0:
        sa, sb = np.float32(np.sqrt(np.float64(a_t))), np.float32(np.sqrt(1.0 - np.float64(a_t)))
        c = np.float32(clip)
        x = np.where(x < -c, -c, np.where(x > c, c, x)).astype(np.float32)       # a NaN fails both comparisons and stays
        e = (f - sa * x) / sb
    return x, e


def diffusion_step_f32(mode, pred, fake, a_t, a_prev, s2, clip, z=None):
    """gct2_diffusion_step as include/gct2.h states it, every operation rounded to float32 on its own.  Returns (fake', x)."""
    with np.errstate(all="ignore"):
        p, f = _f32(pred), _f32(fake)
        x, e = _estimate(mode, p, f, a_t, clip)
        _, _, cx, ce, cz = step_coefficients(a_t, a_prev, s2)
        out = cx * x + ce * e
        if np.float32(s2) != 0:
            out = out + cz * _f32(z)
        assert out.dtype == np.float32 and x.dtype == np.float32
        return out, x


def diffusion_step_fused(mode, pred, fake, a_t, a_prev, s2, clip, z=None, term=0):
    """the contracted forms of the re-noising - what the kernel must NOT compute: term 0 is fma(cx, x, fl(ce e)), term 1 is
    fma(ce, e, fl(cx x)) (a product of two float32 values is exact in float64).  At t = 1 of the quadratic schedule cx = sqrt(0.25) is
    a power of two, cx x is exact and term 0 cannot differ; term 1 can"""
    with np.errstate(all="ignore"):
        p, f = _f32(pred), _f32(fake)
        x, e = _estimate(mode, p, f, a_t, clip)
        _, _, cx, ce, cz = step_coefficients(a_t, a_prev, s2)
        if term == 0:
            out = (np.float64(cx) * x.astype(np.float64) + (ce * e).astype(np.float64)).astype(np.float32)
        else:
            out = ((cx * x).astype(np.float64) + np.float64(ce) * e.astype(np.float64)).astype(np.float32)
        if np.float32(s2) != 0:
            out = out + cz * _f32(z)
        return out, x


# ---- float64 reference ------------------------------------------------------------------------------------------------------------------

def ddim_step_f64(mode, pred, fake, a_t, a_prev, s2, clip, z=None):
    """DDIM eq. 12 in float64: x0 and eps from the prediction by objective, x0 clipped (eps re-derived), then
    x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev - sigma^2) eps + sigma z.  Returns (x_prev, x0)."""
    p, f = np.asarray(pred, dtype=np.float64), np.asarray(fake, dtype=np.float64)
    sa, sb = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    if mode == SAMPLE_X:
        x0, eps = p, (f - sa * p) / sb
    elif mode == SAMPLE_EPS:
        x0, eps = (f - sb * p) / sa, p
    else:
        x0, eps = (f - p) / sa, p / sb
    if clip > 0:
        x0 = np.clip(x0, -clip, clip)
        eps = (f - sa * x0) / sb
    out = np.sqrt(a_prev) * x0 + np.sqrt(max(1.0 - a_prev - s2, 0.0)) * eps
    if s2 > 0:
        out = out + np.sqrt(s2) * np.asarray(z, dtype=np.float64)
    return out, x0


def ddim_sample_f64(denoise, noise, taus, steps, mode, eta=0.0, clip=0.0, z=None):
    """the whole sampler in float64: `denoise(fake, t)` is the network, taus the ascending timesteps, z[k] the noise of step k (0-based,
    sampling order).  Returns the x0 estimate of the last step."""
    fake = np.asarray(noise, dtype=np.float64)
    K = len(taus)
    x0 = None
    for k in range(K):
        tau = taus[K - 1 - k]
        a_t = float(O.alpha_dash(tau, steps))
        a_prev = float(O.alpha_dash(taus[K - 2 - k] if k < K - 1 else 0, steps))
        s2 = sigma2(a_t, a_prev, eta)
        fake, x0 = ddim_step_f64(mode, denoise(fake, tau), fake, a_t, a_prev, s2, clip, None if z is None else z[k])
    return x0
