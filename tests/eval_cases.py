"""gct2_eval_loss_rows (include/gct2.h) restated in float64 numpy, for the CPU and GPU tests of evaluation: the training loss of every
image of a batch on its own, the objective's target and the prediction weight formed on the fly.

The arithmetic is the header's, nothing measured.  Per image b and element, in float32 with every operation rounded once:
    target = x | fl(a[b] x) | fl(fl(a[b] x) + fl(c[b] eps));   p = pred | fl(w[b] pred);   d = fl(target - p)
and per image, in float64: MSE S(d^2) / n_img; L1 S(max(d, -d)) / n_img; pooled S(d^2) / n_img + S((qsum / 256)^2) / n2_img; DCT
S(E^2) / n_img with E = G D G^T.  `rows` returns the float64 values, `rows_bits` their one rounding to float32.

Exact-sum inputs (the method of tests/exact_cases.py and loss_cases.py): pred, x and eps are integers in {-1, 0, 1} and a, c, w come
from {1, 2, 0.5}, so every d is an integer or a half-integer with |d| <= 6, every square a multiple of 1/4 and every partial sum, in
any order, exact - in float32 through the DCT passes (a sum of 8 signed permutation matrices as the basis: |E| <= 384 in steps of
1/2) and in float64 behind them.  A kernel must then reproduce the restatement bit for bit, whatever its summation order."""
import numpy as np

import loss_cases as K

f32, f64 = np.float32, np.float64
COEFFICIENTS = np.array([1.0, 2.0, 0.5], f32)
MODES = ("plain", "a_c", "a_only", "w_only")     # which of (a, c, w) a call passes: none; a and c with eps; a alone, eps NULL; w alone


def _per_image(v, like):
    return np.asarray(v, f32).reshape((-1,) + (1,) * (like.ndim - 1))


def residual(pred, x, eps=None, a=None, c=None, w=None):
    """d [B,H,W,C] float32 by the rule of gct2_mix_per_image: no fused multiply-add, one rounding per operation"""
    pred, x = np.asarray(pred, f32), np.asarray(x, f32)
    if c is not None and eps is None:
        raise ValueError("c without eps")
    target = x
    if a is not None:
        target = _per_image(a, x) * x
        if eps is not None:
            target = target + _per_image(c, x) * np.asarray(eps, f32)
    p = pred if w is None else _per_image(w, pred) * pred
    d = target - p
    assert d.dtype == f32
    return d


def rows_of_residual(kind, d, G=None):
    """float64 [B]: the loss of `kind` over each image of d alone"""
    B, H, W, C = d.shape
    n_img = H * W * C
    dd = d.astype(f64)
    if kind == K.MSE:
        return (dd * dd).reshape(B, -1).sum(axis=1) / n_img
    if kind == K.L1:
        return np.maximum(dd, -dd).reshape(B, -1).sum(axis=1) / n_img
    if kind == K.MSE_POOLED:
        assert H % 16 == 0 and W % 16 == 0
        q = dd.reshape(B, H // 16, 16, W // 16, 16, C).sum(axis=(2, 4))
        n2_img = (H // 16) * (W // 16) * C
        return (dd * dd).reshape(B, -1).sum(axis=1) / n_img + ((q / 256.0) ** 2).reshape(B, -1).sum(axis=1) / n2_img
    assert kind == K.DCT and H == W == np.shape(G)[0] == np.shape(G)[1]
    G = np.asarray(G, f64)
    E = np.einsum("kh,bhwc,lw->bklc", G, dd, G)
    return (E * E).reshape(B, -1).sum(axis=1) / n_img


def rows(kind, pred, x, eps=None, a=None, c=None, w=None, G=None):
    return rows_of_residual(kind, residual(pred, x, eps, a, c, w), G)


def rows_bits(kind, pred, x, eps=None, a=None, c=None, w=None, G=None):
    return rows(kind, pred, x, eps, a, c, w, G).astype(f32)


def mode_arguments(mode, eps, a, c, w):
    """(eps, a, c, w) as a call of `mode` passes them (None = NULL)"""
    return {"plain": (None, None, None, None), "a_c": (eps, a, c, None), "a_only": (None, a, None, None), "w_only": (None, None, None, w)}[mode]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def exact_inputs(rng, shape, kind, zero_image=None):
    """dict(pred, x, eps, a, c, w, G): exact-sum inputs (module docstring).  zero_image: that image gets pred = x and eps = 0, and
    coefficients 1 - an all-zero residual in every mode"""
    B = shape[0]
    draw = lambda: rng.integers(-1, 2, size=shape).astype(f32)
    pred, x, eps = draw(), draw(), draw()
    a, c, w = (rng.choice(COEFFICIENTS, size=B).astype(f32) for _ in range(3))
    if zero_image is not None:
        pred[zero_image] = x[zero_image]
        eps[zero_image] = 0.0
        a[zero_image] = c[zero_image] = w[zero_image] = 1.0
    G = None
    if kind == K.DCT:
        G = K.signed_permutation_basis(rng, shape[1])
        K.assert_exact_bound(G)
    return dict(pred=pred, x=x, eps=eps, a=a, c=c, w=w, G=G)


def assert_exact(kind, d, G=None):
    """the claims of the module docstring on one residual: half-integers with |d| <= 6, and a DCT whose entries stay exact in float32"""
    assert np.array_equal(d * 2, np.round(d * 2)) and np.abs(d).max() <= 6
    if kind == K.DCT:
        E = np.einsum("kh,bhwc,lw->bklc", np.asarray(G, f64), d.astype(f64), np.asarray(G, f64))
        assert np.abs(E).max() <= 384 and np.array_equal(E * 2, np.round(E * 2))
        assert (E * E).reshape(d.shape[0], -1).sum(axis=1).max() * 4 < 2 ** 53


def real_inputs(rng, shape, kind, basis=None):
    """standard-normal tensors, coefficients in [0.25, 1.5); basis: the DCT basis of the size (the caller's, e.g. trainer_math.dct_basis)"""
    B = shape[0]
    draw = lambda: rng.standard_normal(shape).astype(f32)
    coef = lambda: rng.uniform(0.25, 1.5, size=B).astype(f32)
    return dict(pred=draw(), x=draw(), eps=draw(), a=coef(), c=coef(), w=coef(), G=basis if kind == K.DCT else None)


def ulps(got, want):
    """|got - want| in units of the last place of want (float32), elementwise"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    return np.abs(got.astype(f64) - want.astype(f64)) / np.spacing(np.abs(want)).astype(f64)


def fp32_dct_rows_error(d, G32, ref_rows):
    """e32 of the DCT tolerance, per image (tests/test_losses_gpu.py's rule): the two products in numpy float32 from the fp32 basis
    against the float64 restatement, as relative errors of the rows"""
    E, _ = K.dct_planes(d, G32, f32)
    got = (E.astype(f64) ** 2).reshape(d.shape[0], -1).sum(axis=1) / (d.size // d.shape[0])
    return np.abs(got - ref_rows) / np.abs(ref_rows)
