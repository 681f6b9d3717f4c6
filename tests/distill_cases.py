"""Host references and case tables of progressive distillation (a plain helper module: no fixtures, no GPU): gct2_distill_start /
_step / _target restated from include/gct2.h in float32, one rounding per numpy operation like tests/generate_cases.py's restatements,
and a float64 twin of the teacher's two DDIM steps and the target solve from the paper (Salimans & Ho 2022, appendix G: the x~ that
makes one DDIM step from z_t land on the teacher's z''); the shapes and inputs of tests/test_distill_kernels_gpu.py.
"""
import functools
import math

import numpy as np

from pointwise_cases import SAMPLE_EPS, SAMPLE_SCALED_EPS, SAMPLE_X

SAMPLE_V = 5
MODES = [SAMPLE_X, SAMPLE_EPS, SAMPLE_SCALED_EPS, SAMPLE_V]
MODE_IDS = ["x", "eps", "scaled_eps", "v"]
# the columns of a table row (include/gct2.h GCT2_DISTILL_ROW)
SA0, SB0, SA1, SB1, SA2, SB2, RR, DEN, CX0, CK0, CX1, CE1 = range(12)
ROW = 12

# ---- the cases of tests/test_distill_kernels_gpu.py ------------------------------------------------------------------------------------
B, C = 3, 3
STEPS, N = 200, 25                                      # the teacher takes 50 of 200 timesteps
PAIRS = (N, 1, 13)                                      # the last row, the first (no t'': the x0 end point) and a middle one in one batch
# per_image 5 x 7 x 3 = 105: no multiple of 4 (the target's one-element form) and no multiple of the work-group (the tail);
# 16 x 16 x 3 = 768: the target's four-element form, three work-groups of the one-element kernels
NPIXS = (35, 256)
LDOUT, LDOUT2 = 4, 67
SEED, SID = 0x9E3779B97F4A7C15, 9
CLIPS = (0.0, 1.0)
SPECIALS = (2.0, -2.0, 1.0, -1.0, float("nan"), float("inf"), -float("inf"), 1.0000001)


def _f32(a):
    return np.asarray(a, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def planes(images, per_image, count=4):
    """`count` float32 [images, per_image] planes of standard normals; SPECIALS planted at the start of every image of the FIRST
    plane (the prediction): beyond, on and just past the clip bound, a NaN and both infinities"""
    rng = np.random.default_rng([images, per_image, 83])
    arrs = [rng.standard_normal((images, per_image)).astype(np.float32) for _ in range(count)]
    arrs[0][:, :len(SPECIALS)] = np.float32(SPECIALS)
    for v in arrs:
        v.setflags(write=False)
    return tuple(arrs)


# ---- the table in doubles -----------------------------------------------------------------------------------------------------------------

def pair_alphas(taus, alpha):
    """[(a0, a1, a2)] per pair j = 1..N of an ascending grid: alpha(taus[2j-1]), alpha(taus[2j-2]), alpha(taus[2j-3]); a2 = 1 at j = 1"""
    n = len(taus) // 2
    return [(alpha(taus[2 * j - 1]), alpha(taus[2 * j - 2]), alpha(taus[2 * j - 3]) if j > 1 else 1.0) for j in range(1, n + 1)]


def table_f64(alphas):
    """float64 [N, 8]: {sa0, sb0, sa1, sb1, sa2, sb2, r, den} unrounded"""
    rows = []
    for a0, a1, a2 in alphas:
        sa0, sb0, sa1, sb1, sa2, sb2 = (f(a) for a in (a0, a1, a2) for f in (lambda a: math.sqrt(a), lambda a: math.sqrt(1.0 - a)))
        r = sb2 / sb0
        rows.append([sa0, sb0, sa1, sb1, sa2, sb2, r, sa2 - r * sa0])
    return np.array(rows, dtype=np.float64)


def table_f32(alphas):
    """float32 [N, 12] as include/gct2.h states it: table_f64 rounded once, then gct2_diffusion_start_image's pair at a0 and
    gct2_diffusion_step's re-noising pair at a1 - float32 roots of float32 alphas"""
    t = table_f64(alphas).astype(np.float32)
    ext = []
    for a0, a1, _ in alphas:
        A0, A1 = np.float32(a0), np.float32(a1)
        ext.append([np.sqrt(A0), np.sqrt(np.float32(1.0) - A0), np.sqrt(A1), np.sqrt(np.float32(1.0) - A1)])
    out = np.concatenate([t, np.array(ext, dtype=np.float32)], axis=1)
    assert out.dtype == np.float32 and out.shape[1] == ROW
    return out


def rows_of(table, pair):
    """[B, ROW, 1]: the row of every image, pair clamped into 1..N as the kernels clamp it"""
    n = table.shape[0]
    j = np.clip(np.asarray(pair, dtype=np.int64), 1, n) - 1
    return np.asarray(table)[j][:, :, None]


# ---- float32 restatement -----------------------------------------------------------------------------------------------------------------

def estimate_f32(mode, p, f, sa, sb, clip):
    """(x, e) float32: gct2_diffusion_step's update with per-image sa, sb [B, 1], then the clip of x with e re-derived from it"""
    with np.errstate(all="ignore"):
        p, f = _f32(p), _f32(f)
        if mode == SAMPLE_X:
            x, e = p.copy(), (f - sa * p) / sb
        elif mode == SAMPLE_EPS:
            x, e = (f - p * sb) / sa, p.copy()
        elif mode == SAMPLE_SCALED_EPS:
            x, e = (f - p) / sa, p / sb
        else:
            assert mode == SAMPLE_V
            x, e = sa * f - sb * p, sb * f + sa * p
        if clip > 0:
            c = np.float32(clip)
            x = np.where(x < -c, -c, np.where(x > c, c, x)).astype(np.float32)       # a NaN fails both comparisons and stays
            e = (f - sa * x) / sb
        assert x.dtype == np.float32 and e.dtype == np.float32
        return x, e


def start_f32(table, pair, x, e):
    """gct2_distill_start: z0 = fl(fl(cx0 x) + fl(ck0 e))"""
    r = rows_of(table, pair)
    out = r[:, CX0] * _f32(x) + r[:, CK0] * _f32(e)
    assert out.dtype == np.float32
    return out


def step_f32(mode, table, pair, pred, z0, clip):
    """gct2_distill_step: the estimate at (sa0, sb0), re-noised with (cx1, ce1)"""
    with np.errstate(all="ignore"):
        r = rows_of(table, pair)
        x, e = estimate_f32(mode, pred, z0, r[:, SA0], r[:, SB0], clip)
        out = r[:, CX1] * x + r[:, CE1] * e
        assert out.dtype == np.float32
        return out


def target_f32(mode, table, pair, pred2, z1, z0, clip):
    """gct2_distill_target in the stated operation order.  Returns (xt, et, x2, e2)"""
    with np.errstate(all="ignore"):
        r = rows_of(table, pair)
        z0 = _f32(z0)
        x2, e2 = estimate_f32(mode, pred2, z1, r[:, SA1], r[:, SB1], clip)
        full = ((r[:, SA2] * x2 + r[:, SB2] * e2) - r[:, RR] * z0) / r[:, DEN]
        xt = np.where(r[:, SB2] == 0, x2, full).astype(np.float32)
        et = (z0 - r[:, SA0] * xt) / r[:, SB0]
        assert full.dtype == np.float32 and et.dtype == np.float32
        return xt, et, x2, e2


def student_input_f32(table, pair, xt, et):
    """what a student handed (xt, et) at timestep t is noised to, with the table's own roots: fl(fl(sa0 xt) + fl(sb0 et))"""
    r = rows_of(table, pair)
    return r[:, SA0] * _f32(xt) + r[:, SB0] * _f32(et)


# ---- float64 twin ---------------------------------------------------------------------------------------------------------------------------

def estimate_f64(mode, p, f, sa, sb, clip=0.0):
    p, f = np.asarray(p, dtype=np.float64), np.asarray(f, dtype=np.float64)
    if mode == SAMPLE_X:
        x, e = p, (f - sa * p) / sb
    elif mode == SAMPLE_EPS:
        x, e = (f - sb * p) / sa, p
    elif mode == SAMPLE_SCALED_EPS:
        x, e = (f - p) / sa, p / sb
    else:
        x, e = sa * f - sb * p, sb * f + sa * p
    if clip > 0:
        x = np.clip(x, -clip, clip)
        e = (f - sa * x) / sb
    return x, e


def prediction_f64(mode, x, e, sa, sb):
    """what a perfect network of the objective predicts for the clean image x and the noise e"""
    return {SAMPLE_X: x, SAMPLE_EPS: e, SAMPLE_SCALED_EPS: sb * e, SAMPLE_V: sa * e - sb * x}[mode]


def solve_f64(t64, x2, e2, z0):
    """the target solve in float64 on rows t64 [B, 8, 1] of table_f64: (xt, et, z'')"""
    x2, e2, z0 = (np.asarray(v, dtype=np.float64) for v in (x2, e2, z0))
    z2 = t64[:, SA2] * x2 + t64[:, SB2] * e2
    xt = (z2 - t64[:, RR] * z0) / t64[:, DEN]
    et = (z0 - t64[:, SA0] * xt) / t64[:, SB0]
    return xt, et, z2


def two_steps_f64(mode, t64, pred1, pred2, z0, clip=0.0):
    """the teacher's two DDIM steps in float64 for given predictions: (z1, x2, e2)"""
    x1, e1 = estimate_f64(mode, pred1, z0, t64[:, SA0], t64[:, SB0], clip)
    z1 = t64[:, SA1] * x1 + t64[:, SB1] * e1
    x2, e2 = estimate_f64(mode, pred2, z1, t64[:, SA1], t64[:, SB1], clip)
    return z1, x2, e2
