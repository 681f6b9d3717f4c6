"""gct2_image_metrics through the C ABI on the GPU against the float64 restatement of tests/metrics_cases.py.

Exact-sum inputs: the mean squared error comes back bit for bit, and without u also equals the MSE rows of gct2_eval_loss_rows on the
same tensors.  Real inputs: every figure within max(1 float32 ulp of the restatement, 1e-11) (metrics_cases: derived, the kernel's
arithmetic is float64).  The kernel's tile is GCT2_METRICS_TILE = 32 pixels a side: (2, 43, 45, 3) has, under the 11-tap window, a
33 x 35 grid of window positions - one and three past the tile, two tiles each way, the second nearly empty; under the other windows
the grids are 43 x 45, 36 x 38 and 40 x 42.  (3, 17, 19, 4) and the 11 / 12-pixel shapes stay inside one tile.

Every launch runs between guards: each tensor is an interior slice of a NaN-filled buffer that misses a 16-byte boundary by one float
(and must be bit-unchanged afterwards), the outputs sit between sentinels, the scratch has exactly the reported size and starts as
NaN."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_cases as M

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, 12345.0
SMALL = [(1, 11, 11, 1), (2, 11, 12, 3), (3, 12, 11, 3), (2, 16, 16, 3), (3, 17, 19, 4), (2, 43, 45, 3)]
LARGE = (2, 128, 128, 3)
CASES = [(s, w) for s in SMALL for w in M.WINDOWS]
MODES = ("plain", "mixed")            # u NULL; u, v and noised given
ident = lambda c: f"{'x'.join(map(str, c[0]))}-{c[1]}"
f32, f64 = np.float32, np.float64


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.asarray(a, f32).view(np.int32)


class Guarded:
    """a flat float32 device buffer [GUARD + shift | n | GUARD]: `inner` is what the kernel gets, the guards must keep their fill"""

    def __init__(self, gpu, n, fill, values=None, shift=0):
        self.n, self.fill, self.lo = n, fill, GUARD + shift
        self.full = torch.full((n + 2 * GUARD + shift,), fill, dtype=torch.float32, device=gpu)
        assert self.full.data_ptr() % 16 == 0
        self.inner = self.full[self.lo:self.lo + n]
        if values is not None:
            self.inner.copy_(torch.from_numpy(np.ascontiguousarray(values, f32).ravel()))
        self.before = self.full.clone()

    def ptr(self):
        return self.inner.data_ptr()

    def guards_intact(self):
        g = torch.cat([self.full[:self.lo], self.full[self.lo + self.n:]])
        return bool(torch.isnan(g).all()) if np.isnan(self.fill) else bool((g == self.fill).all())

    def unchanged(self):
        return torch.equal(self.full.view(torch.int32), self.before.view(torch.int32))


class Case:
    """one set of inputs and one window on the device; run(mode) launches, checks every guard and returns dict(mse, psnr, ssim)"""

    def __init__(self, gpu, v, window, shift=1):
        self.gpu, self.shape, self.K = gpu, v["pred"].shape, len(window)
        B, n = self.shape[0], v["pred"].size
        self.pred, self.x, self.noised = (Guarded(gpu, n, np.nan, v[k], shift) for k in ("pred", "x", "noised"))
        self.u, self.v = (Guarded(gpu, B, np.nan, v[k], shift) for k in ("u", "v"))
        self.window = Guarded(gpu, self.K, np.nan, window, shift)
        need = ctypes.c_size_t(0)
        lib().check(lib().load().gct2_image_metrics_scratch(*self.shape, self.K, ctypes.byref(need)), "gct2_image_metrics_scratch")
        self.need = need.value
        self.out = {k: Guarded(gpu, B, SENTINEL) for k in ("mse", "psnr", "ssim")}
        self.scratch = Guarded(gpu, self.need, SENTINEL)
        self.inputs = [self.pred, self.x, self.noised, self.u, self.v, self.window]

    def arguments(self, mode, **over):
        mixed = mode == "mixed"
        B, H, W, C = self.shape
        args = dict(pred=self.pred.ptr(), noised=self.noised.ptr() if mixed else None, u=self.u.ptr() if mixed else None,
                    v=self.v.ptr() if mixed else None, x=self.x.ptr(), window=self.window.ptr(), K=self.K, max_val=M.MAX_VAL, k1=M.K1, k2=M.K2,
                    mse=self.out["mse"].ptr(), psnr=self.out["psnr"].ptr(), ssim=self.out["ssim"].ptr(), scratch=self.scratch.ptr(),
                    scratch_floats=self.need, B=B, H=H, W=W, C=C, stream=stream())
        assert not set(over) - set(args)
        args.update(over)
        return list(args.values())

    def run(self, mode, **over):
        for o in self.out.values():
            o.full.fill_(SENTINEL)
        self.scratch.inner.fill_(float("nan"))
        torch.cuda.synchronize()                                            # (the fills ran on the current stream)
        lib().call("gct2_image_metrics", *self.arguments(mode, **over))
        torch.cuda.synchronize()
        assert all(t.unchanged() for t in self.inputs)                      # everything handed in is read only, bit for bit
        assert all(o.guards_intact() for o in self.out.values()) and self.scratch.guards_intact()
        got = {k: o.inner.cpu().numpy() for k, o in self.out.items()}
        assert not any(np.isnan(g).any() for g in got.values())             # no NaN leaked from a guard or from unwritten scratch
        return got


def restated(v, window, mode):
    mixed = mode == "mixed"
    return M.metrics(v["pred"], v["x"], window, v["noised"] if mixed else None, v["u"] if mixed else None, v["v"] if mixed else None)


def assert_all_close(got, want, tag):
    for k in ("mse", "psnr", "ssim"):
        M.assert_close(got[k], want[k], (tag, k))


def eval_mse_rows(gpu, case):
    """the MSE rows of gct2_eval_loss_rows on the same pred and x"""
    need = ctypes.c_size_t(0)
    lib().check(lib().load().gct2_eval_loss_scratch(0, *case.shape, ctypes.byref(need)), "gct2_eval_loss_scratch")
    scratch = torch.zeros(max(4, need.value), dtype=torch.float32, device=gpu)
    rows = torch.zeros(case.shape[0], dtype=torch.float32, device=gpu)
    lib().call("gct2_eval_loss_rows", 0, case.pred.ptr(), case.x.ptr(), None, None, None, None, rows.data_ptr(), scratch.data_ptr(),
               scratch.numel(), *case.shape, None, stream())
    torch.cuda.synchronize()
    return rows.cpu().numpy()


# ---- 1. exact sums: the mean squared error bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_exact_inputs_bit_for_bit(gpu, case):
    shape, wname = case
    v = M.exact_inputs(np.random.default_rng(7), shape)
    run = Case(gpu, v, M.window(wname))
    for mode in MODES:
        want = restated(v, M.window(wname), mode)
        d = v["x"] - want["e"]
        assert np.array_equal(d * 2, np.round(d * 2)) and np.abs(d).max() <= 5          # half-integers: every partial sum is exact
        got = run.run(mode)
        assert np.array_equal(bits(got["mse"]), bits(want["mse"].astype(f32))), (case, mode, got["mse"], want["mse"])
        assert_all_close(got, want, (case, mode))
        if mode == "plain":
            assert np.array_equal(bits(got["mse"]), bits(eval_mse_rows(gpu, run))), case


# ---- 2. real inputs: one float32 ulp ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_real_inputs_within_one_ulp(gpu, case):
    shape, wname = case
    w = M.window(wname)
    for k, (kind, build) in enumerate(M.REAL_INPUTS.items()):
        v = build(np.random.default_rng(11 + k), shape)
        run = Case(gpu, v, w)
        for mode in MODES:
            want = restated(v, w, mode)
            assert np.isfinite(want["psnr"]).all() and (want["mse"] > 0).all()
            assert_all_close(run.run(mode), want, (case, kind, mode))


def test_the_benchmark_image_size_once(gpu):
    w = M.window("gauss11")
    v = M.noisy_pair(np.random.default_rng(5), LARGE)
    run = Case(gpu, v, w, shift=0)
    for mode in MODES:
        assert_all_close(run.run(mode), restated(v, w, mode), (LARGE, mode))


# ---- 3. exact cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_identical_images(gpu, case):
    shape, wname = case
    x = np.random.default_rng(3).uniform(-1, 1, size=shape).astype(f32)
    B = shape[0]
    # mixed: u = 2, v = -1 on noised = pred = x gives fl(fl(2 x) - x) = x exactly
    v = dict(pred=x, x=x, noised=x, u=np.full(B, 2.0, f32), v=np.full(B, -1.0, f32))
    run = Case(gpu, v, M.window(wname))
    for mode in MODES:
        got = run.run(mode)
        assert np.array_equal(got["mse"], np.zeros(B, f32)) and np.isposinf(got["psnr"]).all(), (case, mode, got)
        assert np.array_equal(bits(got["ssim"]), bits(np.ones(B, f32))), (case, mode, got["ssim"])


@pytest.mark.parametrize("wname", ["one", "box8", "dyadic4"])
@pytest.mark.parametrize("shape", [(2, 16, 16, 3), (2, 43, 45, 3)], ids=lambda s: "x".join(map(str, s)))
def test_constant_images_give_the_closed_form(gpu, shape, wname):
    """under the windows that sum to exactly 1 (tests/test_metrics_cases_cpu.py says why the float32 Gaussian is not one of them)"""
    B = shape[0]
    for p, q in ((0.5, -0.25), (0.3, 0.7), (0.0, 0.6)):
        a, b = np.full(shape, p, f32), np.full(shape, q, f32)
        v = dict(pred=a, x=b, noised=a, u=np.ones(B, f32), v=np.ones(B, f32))
        got = Case(gpu, v, M.window(wname)).run("plain")
        M.assert_close(got["ssim"], np.full(B, M.constant_ssim(p, q)), (shape, wname, p, q))
        d = f64(f32(q)) - f64(f32(p))
        M.assert_close(got["mse"], np.full(B, f64(f32(d)) ** 2), (shape, wname, p, q))


# ---- 4. determinism and isolation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 17, 19, 4), (2, 43, 45, 3)], ids=lambda s: "x".join(map(str, s)))
def test_two_launches_agree_and_images_do_not_mix(gpu, shape):
    w = M.window("gauss11")
    v = M.independent_pair(np.random.default_rng(9), shape)
    run = Case(gpu, v, w)
    for mode in MODES:
        first, second = run.run(mode), run.run(mode)
        for k in first:
            assert np.array_equal(bits(first[k]), bits(second[k])), (shape, mode, k)
        for b in range(shape[0]):                                           # each image launched alone: the same bits as its row
            alone = Case(gpu, {k: a[b:b + 1] for k, a in v.items()}, w).run(mode)
            for k in first:
                assert bits(alone[k])[0] == bits(first[k])[b], (shape, mode, k, b)


# ---- 5. optional outputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 11, 11, 1), (2, 43, 45, 3)], ids=lambda s: "x".join(map(str, s)))
def test_null_outputs_are_skipped_and_change_nothing_else(gpu, shape):
    w = M.window("gauss11")
    v = M.noisy_pair(np.random.default_rng(13), shape)
    run = Case(gpu, v, w)
    for mode in MODES:
        full = run.run(mode)
        no_ssim = run.run(mode, ssim=None)
        assert (no_ssim["ssim"] == SENTINEL).all()                          # the buffer nobody named keeps its fill
        assert np.array_equal(bits(no_ssim["mse"]), bits(full["mse"])) and np.array_equal(bits(no_ssim["psnr"]), bits(full["psnr"]))
        bare = run.run(mode, ssim=None, window=None)                        # ... and the window is not needed then
        assert np.array_equal(bits(bare["mse"]), bits(full["mse"])) and np.array_equal(bits(bare["psnr"]), bits(full["psnr"]))
        no_psnr = run.run(mode, psnr=None)
        assert (no_psnr["psnr"] == SENTINEL).all()
        assert np.array_equal(bits(no_psnr["mse"]), bits(full["mse"])) and np.array_equal(bits(no_psnr["ssim"]), bits(full["ssim"]))
        only = run.run(mode, psnr=None, ssim=None)
        assert np.array_equal(bits(only["mse"]), bits(full["mse"])) and (only["psnr"] == SENTINEL).all() and (only["ssim"] == SENTINEL).all()


def test_a_scratch_one_float_short_is_refused(gpu):
    v = M.noisy_pair(np.random.default_rng(1), (2, 16, 16, 3))
    run = Case(gpu, v, M.window("gauss11"))
    with pytest.raises(lib().Gct2Error, match=f"{run.need - 1} floats of scratch, this shape needs {run.need}"):
        lib().call("gct2_image_metrics", *run.arguments("plain", scratch_floats=run.need - 1))
    torch.cuda.synchronize()
    assert all((o.full == SENTINEL).all() for o in run.out.values()) and bool((run.scratch.full == SENTINEL).all())      # nothing was launched
