"""The four training losses of Trainer.call (train.py:254-280) and their gradients restated in float64 numpy, for the CPU and GPU tests
of gct2_loss_fwd_bwd.

The arithmetic is the one include/gct2.h defines, nothing measured: d = fl32(target - pred), the sums in float64, and the gradient
twice - `dpred` in float64 (the comparison target on real-valued inputs) and `dpred_bits` rounded exactly as the header states it
(float32 products and sums, each rounded on its own; the comparison target, bit for bit, on exact-sum inputs).  `loss` is the float64
value, `loss_bits` its one rounding to float32.

Exact-sum inputs (the method of tests/exact_cases.py): pred and target are small integers with d in {-1, 0, 1}, the DCT basis a sum of
8 signed permutation matrices, so that every partial sum in any order is an integer far below 2^22 and every kernel must reproduce the
restatement bit for bit."""
import numpy as np

MSE, L1, MSE_POOLED, DCT = 0, 1, 2, 3
KINDS = {"mse": MSE, "l1": L1, "mse_pooled": MSE_POOLED, "dct": DCT}
f32, f64 = np.float32, np.float64


def residual(pred, target):
    """d = fl32(target - pred)"""
    return np.asarray(target, f32) - np.asarray(pred, f32)


def _result(loss, dpred, dpred_bits):
    return dict(loss=float(loss), loss_bits=f32(loss), dpred=np.asarray(dpred, f64), dpred_bits=np.asarray(dpred_bits, f32))


def mse(pred, target, s=1.0):
    """train.py:272 as gct2_mse_fwd_bwd computes it: dpred = (pred - target) * (s * 2 / n) with the factor formed in float32, loss =
    (float)(sum * (double)(1.0f / n))"""
    pred, target = np.asarray(pred, f32), np.asarray(target, f32)
    n = pred.size
    e = pred - target
    scale = f32(s) * f32(2.0) / f32(n)
    S = np.sum(e.astype(f64) ** 2)
    return dict(loss=float(S / n), loss_bits=f32(S * f64(f32(1.0) / f32(n))), dpred=2.0 * s * e.astype(f64) / n, dpred_bits=e * scale)


def l1(pred, target, s=1.0):
    """train.py:268-270: mean(maximum(t - p, p - t)); a tie sends the gradient to the first operand, a NaN to the second (TF's
    _MaximumGrad: x >= y)"""
    d = residual(pred, target)
    n = d.size
    first = d >= -d
    c = f32(1.0 / n)
    S = np.sum(np.where(first, d, -d).astype(f64))
    return _result(S / n, np.where(first, -1.0, 1.0) * s / n, f32(s) * np.where(first, -c, c).astype(f32))


def cell_sums(d):
    """qsum: the sum of d over each pixel's 16 x 16 cell and channel, float64, [B, H/16, W/16, C]"""
    B, H, W, C = d.shape
    return d.astype(f64).reshape(B, H // 16, 16, W // 16, 16, C).sum(axis=(2, 4))


def mse_pooled(pred, target, s=1.0):
    """train.py:274-280: MSE + the MSE of avg_pool2d(., 16, 16, 'SAME') (H, W multiples of 16: no padding); pooling d"""
    d = residual(pred, target)
    B, H, W, C = d.shape
    assert H % 16 == 0 and W % 16 == 0
    n, n2 = d.size, B * (H // 16) * (W // 16) * C
    q = cell_sums(d)
    S1, S2 = np.sum(d.astype(f64) ** 2), np.sum((q / 256.0) ** 2)
    up = lambda a: np.repeat(np.repeat(a, 16, axis=1), 16, axis=2)
    c1, c2 = f32(-2.0 / n), f32(-2.0 / (65536.0 * n2))
    bits = f32(s) * ((d * c1) + (up(q.astype(f32)) * c2))
    return _result(S1 / n + S2 / n2, s * (d.astype(f64) * (-2.0 / n) + up(q) * (-2.0 / (65536.0 * n2))), bits)


def dct_planes(d, G, dtype=f64):
    """(E, V) = (G D G^T, G^T E G) for every [size, size] plane D = d[b, :, :, c], the four products in `dtype`; both [B, size, size, C]"""
    G = np.asarray(G, dtype)
    D = np.moveaxis(np.asarray(d, dtype), 3, 1)                     # [B, C, h, w]
    T = np.matmul(G, D)                                             # over h
    E = np.matmul(T, G.T)                                           # over w
    U = np.matmul(E, G)                                             # over the second frequency index
    V = np.matmul(G.T, U)                                           # over the first
    return np.moveaxis(E, 1, 3), np.moveaxis(V, 1, 3)


def dct(pred, target, G, s=1.0):
    """train.py:254-260, 265: mean(dct2d(t - p)^2) with dct2d(D) = G D G^T (the reference leaves it transposed; the mean does not see
    that); dpred = s * V * (-2 / n), V = G^T E G"""
    d = residual(pred, target)
    B, H, W, C = d.shape
    assert H == W == np.shape(G)[0] == np.shape(G)[1]
    n = d.size
    E, V = dct_planes(d, G)
    c1 = f32(-2.0 / n)
    return _result(np.sum(E ** 2) / n, s * V * (-2.0 / n), f32(s) * (V.astype(f32) * c1))


def restate(kind, pred, target, G=None, s=1.0):
    if kind == DCT:
        return dct(pred, target, G, s)
    return {MSE: mse, L1: l1, MSE_POOLED: mse_pooled}[kind](pred, target, s)


def dct_basis_reference(size):
    """the reference's G in float64: tf.signal.dct(norm='ortho') [TF] times frequency_weights = 1 / (k + 1) (train.py:255-259)"""
    k, m = np.arange(size, dtype=f64)[:, None], np.arange(size, dtype=f64)[None, :]
    sigma = np.where(k == 0, np.sqrt(1.0 / size), np.sqrt(2.0 / size))
    return sigma / (k + 1.0) * np.cos(np.pi * (2.0 * m + 1.0) * k / (2.0 * size))


# ---- exact-sum inputs ----------------------------------------------------------------------------------------------------------------
def exact_pair(rng, shape):
    """(pred, target): integers, pred in {-1, 0, 1} and target = pred + d with d in {-1, 0, 1}"""
    pred = rng.integers(-1, 2, size=shape).astype(f32)
    d = rng.integers(-1, 2, size=shape).astype(f32)
    return pred, pred + d


def signed_permutation_basis(rng, size, terms=8):
    """a sum of `terms` signed permutation matrices: every row and column has absolute sum <= terms"""
    G = np.zeros((size, size), f32)
    for _ in range(terms):
        perm, sign = rng.permutation(size), rng.choice(np.array([-1.0, 1.0], f32), size=size)
        G[np.arange(size), perm] += sign
    return G


def assert_exact_bound(G, terms=8):
    """with |d| <= 1 every partial sum of the four products, in any order, is an integer of magnitude <= terms^4 = 4096 < 2^22, hence
    exact in float32: |G D| <= 8, |E| <= 64, |E G| <= 512, |V| <= 4096"""
    G = np.asarray(G, f64)
    assert np.array_equal(G, np.round(G))
    assert np.abs(G).sum(axis=0).max() <= terms and np.abs(G).sum(axis=1).max() <= terms
    assert terms ** 4 < 2 ** 22
    return terms ** 2, terms ** 4


def rel_l2(got, want):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    return float(np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-300))


def max_rel(got, want):
    """max |got - want| / max |want|"""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def fp32_dct_error(pred, target, G32, ref):
    """e32 of the DCT tolerance: the same four products with numpy float32 matmuls from the fp32 basis, against the float64
    restatement `ref`: (max |d dpred| / max |dpred|, relative loss error)"""
    d = residual(pred, target)
    E, V = dct_planes(d, G32, f32)
    n = d.size
    dp = V * f32(-2.0 / n)
    loss = np.sum(E.astype(f64) ** 2) / n
    return max_rel(dp, ref["dpred"]), abs(loss - ref["loss"]) / abs(ref["loss"])
