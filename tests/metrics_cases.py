"""gct2_image_metrics restated in numpy from include/gct2.h, and the inputs its tests use.

The x0 estimate is formed in float32 with one rounding per operation (numpy never fuses a multiply and an add); everything behind it
is float64: d^2 and the products a a, b b, a b of two floats are exact there, so only the sums round.  The filter is evaluated
separably, rows then columns, as the header says the kernel does; filter_direct is the 2-D form of the same F.

Tolerance of a kernel result against this restatement (derived, not measured): the kernel's arithmetic is float64, so the one
rounding to float32 dominates: |got - want| <= max(1 float32 ulp of want, 1e-11).  The absolute floor covers SSIM values near zero,
where the float64 cancellation error of a map value is about 2^-52 / C2 ~ 6e-14 times a few operations."""
import numpy as np

f32, f64 = np.float32, np.float64
MAX_VAL, K1, K2 = 2.0, 0.01, 0.03
COEFFICIENTS = np.array([1.0, 2.0, 0.5], f32)

WINDOWS = {
    "gauss11": None,                                              # trainer_math.ssim_window(): filled in by window()
    "one": np.array([1.0], f32),
    "box8": np.full(8, 0.125, f32),
    "dyadic4": np.array([0.25, 0.5, 0.125, 0.125], f32),
}


def gaussian(K=11, sigma=1.5):
    """the Gaussian taps exp(-((i - (K - 1) / 2)^2) / (2 sigma^2)), written a second time: normalised in float64, rounded once"""
    i = np.arange(K, dtype=f64) - (K - 1) / 2.0
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(f32)


def window(name):
    return gaussian() if name == "gauss11" else WINDOWS[name]


def _per_image(v, like):
    return np.asarray(v, f32).reshape((-1,) + (1,) * (like.ndim - 1))


def estimate(pred, noised=None, u=None, v=None):
    """e [B,H,W,C] float32: pred, or fl(fl(u[b] noised) + fl(v[b] pred))"""
    pred = np.asarray(pred, f32)
    if u is None:
        assert noised is None and v is None
        return pred
    un = _per_image(u, pred) * np.asarray(noised, f32)
    vp = _per_image(v, pred) * pred
    assert un.dtype == f32 and vp.dtype == f32
    return un + vp


def filter_separable(q, w):
    """F(q) [B,H-K+1,W-K+1,C] in float64: along W first, then along H (VALID)"""
    q, w = np.asarray(q, f64), np.asarray(w, f64)
    K = len(w)
    OH, OW = q.shape[1] - K + 1, q.shape[2] - K + 1
    rows = np.zeros(q.shape[:2] + (OW,) + q.shape[3:], f64)
    for s in range(K):
        rows += w[s] * q[:, :, s:s + OW]
    out = np.zeros((q.shape[0], OH, OW, q.shape[3]), f64)
    for r in range(K):
        out += w[r] * rows[:, r:r + OH]
    return out


def filter_direct(q, w):
    """the same F as one double sum over the K x K window"""
    q, w = np.asarray(q, f64), np.asarray(w, f64)
    K = len(w)
    OH, OW = q.shape[1] - K + 1, q.shape[2] - K + 1
    out = np.zeros((q.shape[0], OH, OW, q.shape[3]), f64)
    for r in range(K):
        for s in range(K):
            out += (w[r] * w[s]) * q[:, r:r + OH, s:s + OW]
    return out


def ssim_map(e, x, w, max_val=MAX_VAL, k1=K1, k2=K2, F=filter_separable):
    """lum * cs at every window position and channel, float64 [B,H-K+1,W-K+1,C]"""
    a, b = np.asarray(e, f32).astype(f64), np.asarray(x, f32).astype(f64)
    C1, C2 = (f64(f32(k1)) * f64(f32(max_val))) ** 2, (f64(f32(k2)) * f64(f32(max_val))) ** 2
    ma, mb, A, Bq, AB = F(a, w), F(b, w), F(a * a, w), F(b * b, w), F(a * b, w)
    mab, msq = ma * mb, ma * ma + mb * mb
    lum = (2.0 * mab + C1) / (msq + C1)
    cs = ((2.0 * AB - 2.0 * mab) + C2) / (((A + Bq) - msq) + C2)
    return lum * cs


def metrics(pred, x, w=None, noised=None, u=None, v=None, max_val=MAX_VAL, k1=K1, k2=K2):
    """dict(mse, psnr, ssim) float64 [B] each (ssim None without a window), and e"""
    e = estimate(pred, noised, u, v)
    x = np.asarray(x, f32)
    d = x - e
    assert d.dtype == f32
    B = d.shape[0]
    dd = d.astype(f64)
    m = (dd * dd).reshape(B, -1).sum(axis=1) / (d.size // B)
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(f64(f32(max_val)) * f64(f32(max_val)) / m)
    ssim = None if w is None else ssim_map(e, x, w, max_val, k1, k2).reshape(B, -1).mean(axis=1)
    return dict(mse=m, psnr=psnr, ssim=ssim, e=e)


def tolerance(want):
    """max(1 float32 ulp of want, 1e-11), elementwise (infinite where want is: such a value must match exactly)"""
    want = np.asarray(want, f64)
    with np.errstate(invalid="ignore", over="ignore"):
        ulp = np.spacing(np.abs(want).astype(f32)).astype(f64)
    return np.maximum(ulp, 1e-11)


def assert_close(got, want, tag=""):
    got, want = np.asarray(got), np.asarray(want, f64)
    assert got.dtype == f32 and got.shape == want.shape, tag
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf].astype(f32)), (tag, got, want)
    assert not np.isnan(got).any() and not np.isnan(want).any(), (tag, got, want)
    err = np.abs(got[~inf].astype(f64) - want[~inf])
    assert (err <= tolerance(want[~inf])).all(), (tag, got, want, err)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def exact_inputs(rng, shape):
    """integers in {-1, 0, 1} and coefficients in {1, 2, 0.5}: e and d are half-integers, every d^2 and every partial sum of them is
    exact in float64 - the mean squared error must come back bit for bit whatever the order of the sum"""
    draw = lambda: rng.integers(-1, 2, size=shape).astype(f32)
    coef = lambda: rng.choice(COEFFICIENTS, size=shape[0]).astype(f32)
    return dict(pred=draw(), x=draw(), noised=draw(), u=coef(), v=coef())


def _coefficients(rng, B):
    return dict(u=rng.uniform(0.5, 2.0, size=B).astype(f32), v=-rng.uniform(0.25, 1.5, size=B).astype(f32))


def noisy_pair(rng, shape, sigma=0.1):
    """x uniform in [-1, 1) and pred = x + noise; noised another noisy copy"""
    x = rng.uniform(-1, 1, size=shape).astype(f32)
    pred = (x + sigma * rng.standard_normal(shape)).astype(f32)
    noised = (x + 2 * sigma * rng.standard_normal(shape)).astype(f32)
    return dict(pred=pred, x=x, noised=noised, **_coefficients(rng, shape[0]))


def independent_pair(rng, shape):
    draw = lambda: rng.uniform(-1, 1, size=shape).astype(f32)
    return dict(pred=draw(), x=draw(), noised=draw(), **_coefficients(rng, shape[0]))


def flat_pair(rng, shape):
    """0.75 +- 1e-3 on both sides: A - mu_a^2 cancels nearly everything (with u = 1.5, v = -0.5 the estimate is as flat)"""
    draw = lambda: (0.75 + 1e-3 * rng.uniform(-1, 1, size=shape)).astype(f32)
    B = shape[0]
    return dict(pred=draw(), x=draw(), noised=draw(), u=np.full(B, 1.5, f32), v=np.full(B, -0.5, f32))


REAL_INPUTS = {"noisy": noisy_pair, "independent": independent_pair, "flat": flat_pair}


def constant_ssim(p, q, max_val=MAX_VAL, k1=K1):
    """SSIM of two constant images a = p, b = q under a window that sums to 1: the variances and the covariance vanish, cs = 1"""
    C1 = (f64(f32(k1)) * f64(f32(max_val))) ** 2
    p, q = f64(f32(p)), f64(f32(q))
    return (2 * p * q + C1) / (p * p + q * q + C1)
