"""Host references and case tables of two-network guidance (a plain helper module: no fixtures, no GPU): the combine
p = p_guide + w (p_main - p_guide) restated from include/gct2.h in float32, one rounding per numpy operation; gct2_x0_quantile_guided and
gct2_diffusion_step_guided on top of it and of dynamic_cases / generate_cases / img2img_cases; the planes and shapes of
tests/test_guidance_kernels_gpu.py and the perturbation that makes the guide of tests/test_guidance_step_gpu.py.
"""
import functools

import numpy as np

import dynamic_cases as D
import generate_cases as G
import img2img_cases as I
from dynamic_cases import MODE_IDS, MODES, SAMPLE_V  # noqa: F401

B, C = 3, 3
WEIGHTS = (0.0, 0.5, 3.0)
W_THRESHOLD = 3.0                                      # the w > 1 of the threshold cases
FLOOR, PERCENTILE = 1.0, 0.995
C1 = 1.37
# the step's shapes: (per_image, offset, offset0, image_stride) - 75 = 5x5x3 is no multiple of 4 (the general counter path); 192 = 8x8x3
# with offsets and a stride that are multiples of 4 (the four-element path, given 16-byte aligned planes); 192 off that alignment
STEP_SHAPES = {"75": (75, 3, 2 + 7 * 75, G.image_stride(75)), "192_aligned": (192, 8, 8 + 4 * 192, 192), "192_unaligned": (192, 5, 3 + 4 * 192, 197)}
SELECT_PER_IMAGE = 4800                                # 40x40x3: more than one work-group per image (QSEL_PER_GROUP = 4096)
T = 37                                                 # the timestep of the kernel cases (generate_cases.alphas: a_t about 0.17)
GUIDE_SEED, GUIDE_SIGMA = 1234, 0.05                   # the guide of the end-to-end tests: the golden parameters + sigma N(0, 1), this seed


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def combine_f32(pred, pred_guide, w):
    """d = p_main - p_guide; t = (float)w d; p = p_guide + t: three float32 operations, each rounded once"""
    with np.errstate(all="ignore"):
        pm, pg = _f32(pred), _f32(pred_guide)
        d = pm - pg
        t = np.float32(w) * d
        p = pg + t
        assert d.dtype == t.dtype == p.dtype == np.float32
        return p


def combine_fused(pred, pred_guide, w):
    """what the kernel must NOT compute: p = fma(w, d, p_guide), the product unrounded (exact in float64)"""
    pm, pg = _f32(pred), _f32(pred_guide)
    d = pm - pg
    return (pg.astype(np.float64) + np.float64(np.float32(w)) * d.astype(np.float64)).astype(np.float32)


def guided_select_f32(mode, pred, pred_guide, w, fake, a_t, rank, floor):
    """gct2_x0_quantile_guided: gct2_x0_quantile on the combined plane - (rows [B, 2], q [B])"""
    return D.select_f32(mode, combine_f32(pred, pred_guide, w), fake, a_t, rank, floor)


def step_f32(mode, pred, fake, a_t, a_prev, rows=None, clip=0.0, s2=0.0, z=None, hist=None, c1=None, known=None, mask_el=None, z0=None):
    """every form of the step on ONE prediction plane, all four objectives: rows [B, 2] the per-image bound, else the scalar clip (0: none,
    the estimate and eps as the update left them).  c1 None: the plain / masked step; a number: the multistep form.
    Returns (fake', x0_out, hist_out)"""
    if rows is None and clip > 0:
        rows = np.float32([[clip, 1.0]] * _f32(pred).shape[0])     # (the fixed clip is the bound {clip, 1}: tests/test_dynamic_cases_cpu.py)
    if rows is not None:
        return D.dynamic_step_f32(mode, pred, fake, rows, a_t, a_prev, s2, z, hist, c1, known, mask_el, z0)
    with np.errstate(all="ignore"):
        f = _f32(fake)
        x, e = D.estimate_f32(mode, pred, fake, a_t)
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


def guided_step_f32(mode, pred, pred_guide, w, fake, a_t, a_prev, **kw):
    """gct2_diffusion_step_guided: step_f32 on the combined plane (pred_guide None: on pred)"""
    p = _f32(pred) if pred_guide is None else combine_f32(pred, pred_guide, w)
    return step_f32(mode, p, fake, a_t, a_prev, **kw)


# ---- the planes ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planes(per_image, mode=None):
    """(pred, pred_guide, fake, hist, known, mask per pixel) float32 [B, ...]: finite, non-zero standard normals; the guide's prediction is
    the main one plus an independent N(0, 0.4^2) - a weaker network's - so that w = 3 moves the estimate by about 0.8 sigma.  With a mode
    the planes are scaled by dynamic_cases.step_scale, which puts the estimate's spread at about 1 under the epsilon objectives.  The
    mask is fractional: 0, 1, values between and beyond, no NaN"""
    rng = np.random.default_rng([per_image, 97])
    pm, f, h, kn = (rng.standard_normal((B, per_image)).astype(np.float32) for _ in range(4))
    pg = (pm + 0.4 * rng.standard_normal((B, per_image))).astype(np.float32)
    if mode is not None:
        a_t, _ = G.alphas(T)
        k = np.float32(D.step_scale(mode, a_t))
        pm, pg, f = pm * k, pg * k, f * k
    m = np.float32([0.0, 1.0, 0.5, 0.25, -0.5, 1.5, 0.75, 1e-30])[rng.integers(0, 8, (B, per_image // C))]
    out = (pm, pg, f, h, kn, m)
    for a in out:
        assert a.dtype == np.float32 and np.isfinite(a).all()
        a.setflags(write=False)
    assert (pm != 0).all() and (pg != 0).all() and (f != 0).all()
    return out


def perturbed(params, seed=GUIDE_SEED, sigma=GUIDE_SIGMA):
    """the guide's parameters: every float tensor of `params` plus sigma N(0, 1) from one fixed-seed generator, in sorted key order"""
    rng = np.random.default_rng(seed)
    out = {}
    for k in sorted(params):
        v = np.asarray(params[k])
        out[k] = (v + sigma * rng.standard_normal(v.shape)).astype(v.dtype) if v.dtype.kind == "f" else v
    return out
