"""gct2_eval_loss_rows through the C ABI on the GPU: the training loss per image, with the objective's target and the prediction weight
formed inside the kernel (tests/eval_cases.py restates it in float64).

Exact-sum inputs must come back bit for bit, per image.  Real values: MSE, L1 and pooled MSE within 1 ulp of float32(restatement) -
every term is exact in float64, the order-dependent error of a float64 sum of <= 2^16 terms is far below 2^-24, and there is one final
rounding; the DCT rows within the bound tests/test_losses_gpu.py derives for the DCT loss (4 x the error of the same products in
numpy float32, at least 1e-6), per image.  Every buffer carries guard zones: NaN around what a kernel may read (and the inputs must
be bit-unchanged afterwards), sentinels around `rows`, a scratch of exactly the reported size whose inside starts as NaN."""
import ctypes

import numpy as np
import pytest
import torch

import eval_cases as E
import loss_cases as K

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, 12345.0
POINTWISE = [(1, 4, 4, 3), (3, 5, 7, 3), (5, 16, 16, 3), (2, 32, 16, 1), (2, 16, 48, 4)]
POOLED = [(5, 16, 16, 3), (2, 32, 16, 1), (2, 16, 48, 4)]
DCTS = [(3, 8, 8, 3), (3, 20, 20, 3)]
CASES = ([(K.MSE, s) for s in POINTWISE] + [(K.L1, s) for s in POINTWISE] + [(K.MSE_POOLED, s) for s in POOLED] + [(K.DCT, s) for s in DCTS])
NAMES = {K.MSE: "mse", K.L1: "l1", K.MSE_POOLED: "mse_pooled", K.DCT: "dct"}
ident = lambda c: f"{NAMES[c[0]]}-{'x'.join(map(str, c[1]))}"


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """a flat float32 device buffer [GUARD + shift | n | GUARD]: `inner` is what the kernel gets (shift: floats by which it misses a
    16-byte boundary), the guards must keep their fill"""

    def __init__(self, gpu, n, fill, values=None, shift=0):
        self.n, self.fill, self.lo = n, fill, GUARD + shift
        self.full = torch.full((n + 2 * GUARD + shift,), fill, dtype=torch.float32, device=gpu)
        assert self.full.data_ptr() % 16 == 0
        self.inner = self.full[self.lo:self.lo + n]
        if values is not None:
            self.inner.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32).ravel()))
        self.before = self.full.clone()

    def ptr(self):
        return self.inner.data_ptr()

    def guards_intact(self):
        g = torch.cat([self.full[:self.lo], self.full[self.lo + self.n:]])
        return bool(torch.isnan(g).all()) if np.isnan(self.fill) else bool((g == self.fill).all())

    def unchanged(self):
        return torch.equal(self.full.view(torch.int32), self.before.view(torch.int32))


class Case:
    """one kind and shape on the device; run(mode) launches with the arguments of that mode, checks every guard and returns rows"""

    def __init__(self, gpu, kind, v, shift=0):
        self.gpu, self.kind, self.shape = gpu, kind, v["pred"].shape
        B, n = self.shape[0], v["pred"].size
        self.pred, self.x, self.eps = (Guarded(gpu, n, np.nan, v[k], shift) for k in ("pred", "x", "eps"))
        self.a, self.c, self.w = (Guarded(gpu, B, np.nan, v[k]) for k in ("a", "c", "w"))
        self.basis = Guarded(gpu, v["G"].size, np.nan, v["G"]) if v["G"] is not None else None
        need = ctypes.c_size_t(0)
        lib().check(lib().load().gct2_eval_loss_scratch(kind, *self.shape, ctypes.byref(need)), "gct2_eval_loss_scratch")
        self.need = need.value
        self.rows, self.scratch = Guarded(gpu, B, SENTINEL), Guarded(gpu, self.need, SENTINEL)
        self.inputs = [self.pred, self.x, self.eps, self.a, self.c, self.w] + ([self.basis] if self.basis else [])

    def arguments(self, mode, **over):
        eps, a, c, w = E.mode_arguments(mode, self.eps.ptr(), self.a.ptr(), self.c.ptr(), self.w.ptr())
        B, H, W, C = self.shape
        args = dict(kind=self.kind, pred=self.pred.ptr(), x=self.x.ptr(), eps=eps, a=a, c=c, w=w, rows=self.rows.ptr(),
                    scratch=self.scratch.ptr(), scratch_floats=self.need, B=B, H=H, W=W, C=C,
                    basis=self.basis.ptr() if self.basis else None, stream=stream())
        assert not set(over) - set(args)
        args.update(over)
        return list(args.values())

    def prepare(self):
        self.rows.full.fill_(SENTINEL)
        self.scratch.inner.fill_(float("nan"))
        torch.cuda.synchronize()                                            # (the fills ran on the current stream)

    def run(self, mode):
        self.prepare()
        lib().call("gct2_eval_loss_rows", *self.arguments(mode))
        torch.cuda.synchronize()
        assert all(t.unchanged() for t in self.inputs)                      # pred, x, eps (and the rest) are read only, bit for bit
        assert self.rows.guards_intact() and self.scratch.guards_intact()
        rows = self.rows.inner.cpu().numpy()
        assert not np.isnan(rows).any()                                     # no NaN leaked from a guard or from unwritten scratch
        return rows


def bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def want_rows(kind, v, mode):
    eps, a, c, w = E.mode_arguments(mode, v["eps"], v["a"], v["c"], v["w"])
    return E.rows(kind, v["pred"], v["x"], eps, a, c, w, v["G"]), E.residual(v["pred"], v["x"], eps, a, c, w)


# ---- 1. exact sums: bit for bit, per image -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_exact_inputs_bit_for_bit_per_image(gpu, case):
    kind, shape = case
    zero = 1 if shape[0] > 1 else None
    v = E.exact_inputs(np.random.default_rng(7), shape, kind, zero_image=zero)
    run = Case(gpu, kind, v)
    for mode in E.MODES:
        want, d = want_rows(kind, v, mode)
        E.assert_exact(kind, d, v["G"])
        got = run.run(mode)
        assert np.array_equal(bits(got), bits(want.astype(np.float32))), (mode, got, want)
        assert want.max() > 0
        if zero is not None:                                                # the neighbour of an all-zero residual: exactly +0.0
            assert bits(got)[zero] == 0 and got[zero - 1] > 0 and (zero + 1 >= shape[0] or got[zero + 1] > 0), (mode, got)


# ---- 2. real values --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_real_values_against_float64_per_image(gpu, case):
    import gan_class_transfer2_amd as g
    kind, shape = case
    v = E.real_inputs(np.random.default_rng(11), shape, kind, g.trainer_math.dct_basis(shape[1]) if kind == K.DCT else None)
    run = Case(gpu, kind, v)
    for mode in E.MODES:
        want, d = want_rows(kind, v, mode)
        got = run.run(mode)
        if kind != K.DCT:
            u = E.ulps(got, want.astype(np.float32))
            print(f"{ident(case)} {mode}: max ulps {u.max():.3g}")
            assert u.max() <= 1, (mode, got, want)
            continue
        e32 = E.fp32_dct_rows_error(d, v["G"], want)
        err = np.abs(got.astype(np.float64) - want) / want
        print(f"{ident(case)} {mode}: rel {err.max():.3g} (e32 {e32.max():.3g})")
        assert (err <= np.maximum(1e-6, 4 * e32)).all(), (mode, err, e32)


# ---- 3. operands off the 16-byte grid: the same elements, the same bits ---------------------------------------------------------------------
@pytest.mark.parametrize("case", [(K.MSE, (3, 5, 7, 3)), (K.L1, (3, 5, 7, 3)), (K.MSE_POOLED, (2, 32, 16, 1)), (K.DCT, (3, 8, 8, 3))], ids=ident)
def test_misaligned_operands_give_the_same_bits(gpu, case):
    import gan_class_transfer2_amd as g
    kind, shape = case
    v = E.real_inputs(np.random.default_rng(13), shape, kind, g.trainer_math.dct_basis(shape[1]) if kind == K.DCT else None)
    aligned = Case(gpu, kind, v)
    for shift in (1, 2, 3):
        shifted = Case(gpu, kind, v, shift=shift)
        assert shifted.pred.ptr() % 16 == 4 * shift
        for mode in ("plain", "a_c"):
            assert np.array_equal(bits(shifted.run(mode)), bits(aligned.run(mode))), (shift, mode)


def test_same_bits_run_to_run_and_on_two_streams(gpu):
    v = E.real_inputs(np.random.default_rng(17), (5, 16, 16, 3), K.MSE_POOLED)
    run = Case(gpu, K.MSE_POOLED, v)
    first = run.run("a_c")
    assert np.array_equal(bits(run.run("a_c")), bits(first))
    side = torch.cuda.Stream()
    run.prepare()
    with torch.cuda.stream(side):
        lib().call("gct2_eval_loss_rows", *run.arguments("a_c", stream=side.cuda_stream))
    torch.cuda.synchronize()
    assert np.array_equal(bits(run.rows.inner.cpu().numpy()), bits(first))


# ---- 4. every rejection launches nothing ---------------------------------------------------------------------------------------------------
def _rejections(run):
    B, H, W, C = run.shape
    other = torch.zeros(8, dtype=torch.float32, device=run.gpu)
    return [("plain", dict(kind=4)), ("plain", dict(kind=-1)), ("plain", dict(pred=None)), ("plain", dict(x=None)), ("plain", dict(rows=None)),
            ("plain", dict(scratch=None)), ("plain", dict(B=0)), ("plain", dict(H=-H)), ("plain", dict(W=0)), ("plain", dict(C=0)),
            ("plain", dict(C=5)), ("plain", dict(kind=K.MSE_POOLED, H=H + 8)), ("plain", dict(kind=K.DCT, W=2 * W, basis=other.data_ptr())),
            ("plain", dict(kind=K.DCT, H=18, W=18, basis=other.data_ptr())), ("plain", dict(kind=K.DCT, basis=None)),
            ("plain", dict(kind=K.DCT, basis=other.data_ptr() + 4)), ("plain", dict(c=run.c.ptr())), ("a_c", dict(c=None)),
            ("plain", dict(scratch=run.scratch.ptr() + 4)), ("plain", dict(scratch=run.scratch.ptr() + 8)),
            ("plain", dict(scratch_floats=run.need - 1)), ("plain", dict(scratch_floats=0)), ("plain", dict(B=65536)),
            ("plain", dict(B=65535, H=128, W=128)), ("plain", dict(B=2, H=32768, W=32768, C=1))]


@pytest.mark.parametrize("kind, shape", [(K.MSE, (5, 16, 16, 3)), (K.DCT, (3, 20, 20, 3))], ids=lambda v: str(v))
def test_every_rejection_launches_nothing(gpu, kind, shape):
    v = E.exact_inputs(np.random.default_rng(3), shape, kind)
    if v["G"] is None:
        v["G"] = K.signed_permutation_basis(np.random.default_rng(3), shape[1])      # (the DCT rows of the table need a valid basis)
    run = Case(gpu, kind, v)
    L = lib().load()
    run.prepare()
    for mode, over in _rejections(run):
        rc = L.gct2_eval_loss_rows(*run.arguments(mode, **over))
        assert rc == 1, (mode, over, rc)
        assert L.gct2_last_error().decode().startswith("eval_loss_rows: "), (mode, over)
    torch.cuda.synchronize()
    assert bool((run.rows.full == SENTINEL).all())                            # rows keeps its poison
    assert bool(torch.isnan(run.scratch.inner).all()) and run.scratch.guards_intact()
    assert all(t.unchanged() for t in run.inputs)
    # ... and the same buffers still serve a valid call
    want, _ = want_rows(kind, v, "plain")
    assert np.array_equal(bits(run.run("plain")), bits(want.astype(np.float32)))
