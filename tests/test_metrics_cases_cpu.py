"""The image metrics without a GPU: the restatement of tests/metrics_cases.py against itself, the host arithmetic of trainer_math
(METRICS, ssim_window, x0_coefficients against the sampler oracle's update), the binding, and every GCT2_EINVAL class of
gct2_image_metrics with fake pointers in a child process that sees no device (the pattern of tests/test_capi_contract_cpu.py: the
child reports gct2_device_check() first and the test skips when a device is visible to it)."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import metrics_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = 1, 3
f32, f64 = np.float32, np.float64


def tm():
    import gan_class_transfer2_amd as g
    return g.trainer_math


# ---- 1. the restatement against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.WINDOWS))
def test_identical_images_give_zero_infinity_and_exactly_one(name):
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, size=(2, 17, 19, 3)).astype(f32)
    out = M.metrics(x, x, M.window(name))
    assert np.array_equal(out["mse"], [0.0, 0.0]) and np.isposinf(out["psnr"]).all() and np.array_equal(out["ssim"], [1.0, 1.0])


@pytest.mark.parametrize("name", list(M.WINDOWS))
@pytest.mark.parametrize("kind", list(M.REAL_INPUTS))
def test_separable_and_direct_filters_agree(name, kind):
    v = M.REAL_INPUTS[kind](np.random.default_rng(2), (2, 17, 19, 3))
    w = M.window(name)
    sep = M.ssim_map(v["pred"], v["x"], w)
    direct = M.ssim_map(v["pred"], v["x"], w, F=M.filter_direct)
    assert np.abs(sep - direct).max() <= 1e-12
    assert np.array_equal(sep.reshape(2, -1).mean(axis=1).astype(f32), direct.reshape(2, -1).mean(axis=1).astype(f32))


@pytest.mark.parametrize("name", ["one", "box8", "dyadic4"])
def test_constant_images_give_the_closed_form(name):
    """(under a window that sums to exactly 1: the float32 Gaussian taps sum to 1 - 1.4e-9, which leaves A - mu_a^2 = p^2 s^2 (1 - s^2)
    instead of 0 and moves cs by (p - q)^2 * 3e-9 / C2 ~ 1e-6)"""
    w = M.window(name)
    assert w.astype(f64).sum() == 1.0
    for p, q in ((0.5, -0.25), (0.3, 0.7), (-0.9, -0.9), (0.0, 0.6)):
        a, b = np.full((1, 16, 17, 2), p, f32), np.full((1, 16, 17, 2), q, f32)
        got = M.metrics(a, b, w)
        assert abs(got["ssim"][0] - M.constant_ssim(p, q)) <= 1e-12
        assert got["mse"][0] == pytest.approx((f64(f32(q)) - f64(f32(p))) ** 2, rel=1e-6)


def test_the_window_sums_to_one_and_is_symmetric():
    w = tm().ssim_window()
    assert w.dtype == f32 and w.shape == (11,) and np.array_equal(w, w[::-1])
    assert abs(w.astype(f64).sum() - 1.0) <= np.spacing(f32(1.0))
    assert np.array_equal(w, M.gaussian())                      # the same formula, written twice
    assert np.array_equal(tm().ssim_window(1), [1.0]) and tm().ssim_window(16, 2.0).shape == (16,)
    for bad in (dict(K=0), dict(K=17), dict(sigma=0.0), dict(sigma=float("nan"))):
        with pytest.raises(ValueError):
            tm().ssim_window(**bad)


# ---- 2. x0_coefficients against the oracle's update ---------------------------------------------------------------------------------------
def oracle_update(steps, alpha, mode_switches):
    """the nested `update` of oracle/sampler_oracle.py's log_sample (train.py:382-413), rebuilt around our own alpha and switches: the
    code object is the oracle's, only the closure cells are supplied here"""
    from oracle import sampler_oracle as S
    code = next(c for c in S.log_sample.__code__.co_consts if isinstance(c, types.CodeType) and c.co_name == "update")
    cells = dict(a=alpha, **mode_switches)
    assert set(code.co_freevars) == set(cells), code.co_freevars
    return types.FunctionType(code, S.__dict__, "update", None, tuple(types.CellType(cells[n]) for n in code.co_freevars))


SWITCHES = {1: dict(ode=False, px=False, pse=False), 2: dict(ode=False, px=False, pse=True), 3: dict(ode=True, px=True, pse=False)}


@pytest.mark.parametrize("schedule", [("quadratic", 0.0), ("cosine", 0.0)], ids=["default", "cosine_table"])
@pytest.mark.parametrize("mode", [1, 2, 3], ids=["epsilon", "scaled_epsilon", "ode"])
def test_x0_coefficients_reproduce_the_oracles_update(mode, schedule, steps=200):
    T = tm()
    from oracle import denoiser_oracle as O
    if schedule == ("quadratic", 0.0):
        alpha = lambda t: float(O.alpha_dash(t, steps))
    else:
        alpha = lambda t: float(T.alpha_dash(t, steps, *schedule))
    update = oracle_update(steps, alpha, SWITCHES[mode])
    rng = np.random.default_rng(mode)
    ts = np.array([1, 2, steps // 2, steps])
    u, v = T.x0_coefficients(ts, steps, mode, *schedule)
    assert u.dtype == f32 and v.dtype == f32 and u.shape == v.shape == (4,)
    if mode == 1 and schedule[0] == "quadratic":
        assert 395 < abs(u[-1]) < 405                            # 1 / sqrt(alpha_dash(steps)) = 2 (steps + 1)
    for k, t in enumerate(ts):
        fake = rng.uniform(-1, 1, size=(1, 4, 4, 3)).astype(f32)
        pred = rng.uniform(-1, 1, size=(1, 4, 4, 3)).astype(f32)
        want, _ = update(pred.astype(f64), fake.astype(f64), None, None, int(t))
        got = M.estimate(pred, fake, u[k:k + 1], v[k:k + 1])
        # float32 rounding of the operands: each coefficient (2^-24 relative), each product, and the sum, whose size is at most
        # S = |u||fake| + |v||pred|: three roundings of at most 2^-24 S each; the oracle's own float64 error is below 1e-12 S
        S = abs(f64(u[k])) * np.abs(fake) + abs(f64(v[k])) * np.abs(pred)
        assert (np.abs(got.astype(f64) - want) <= 3.001 * 2.0 ** -24 * S).all(), (mode, schedule, t)
    # a torch tensor gathers the same entries
    import torch
    tu, tv = T.x0_coefficients(torch.tensor(ts, dtype=torch.int32), steps, mode, *schedule)
    assert np.array_equal(tu.numpy(), u) and np.array_equal(tv.numpy(), v) and tu.is_contiguous()


def test_predict_x_needs_no_coefficients():
    T = tm()
    assert T.x0_coefficients(np.array([1, 2]), 200, 0) == (None, None) and T.x0_tables(200, 0) is None
    assert [T.x0_mode(*s) for s in ((True, False, False), (False, False, False), (False, True, False), (True, False, True), (False, True, True))] == [0, 1, 2, 3, 3]


# ---- 3. the binding -------------------------------------------------------------------------------------------------------------------
def test_binding_plan_table_and_abi():
    import gan_class_transfer2_amd as g
    L = g._lib
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert L.SIGNATURES["gct2_image_metrics"] == [vp, vp, vp, vp, vp, vp, i, f, f, f, vp, vp, vp, vp, sz, i, i, i, i, vp]
    assert L.SIGNATURES["gct2_image_metrics_scratch"] == [i, i, i, i, i, ctypes.POINTER(ctypes.c_size_t)]
    assert "gct2_image_metrics" in L.PLANNABLE and "gct2_image_metrics_scratch" not in L.PLANNABLE
    with open(os.path.join(ROOT, "gan-class-transfer2_amd", "csrc", "plan.hip")) as fh:
        assert "GCT2_ENTRY(gct2_image_metrics)" in fh.read()
    with open(os.path.join(ROOT, "include", "gct2.h")) as fh:
        header = fh.read()
    assert "int gct2_image_metrics(" in header and "int gct2_image_metrics_scratch(" in header
    assert L.ABI_VERSION == 17 and L.load().gct2_abi_version() == 17
    need = ctypes.c_size_t(0)
    assert L.load().gct2_image_metrics_scratch(2, 43, 45, 3, 11, ctypes.byref(need)) == 0
    assert need.value == 4 * 2 * (2 * 2 * 3)                    # one float64 pair per 32 x 32 tile, channel and image


# ---- 4. names ---------------------------------------------------------------------------------------------------------------------------
def test_check_metrics_and_compile():
    import gan_class_transfer2_amd as g
    T = g.trainer_math
    assert T.METRICS == ("mse_x0", "psnr", "ssim")
    assert T.check_metrics(None) == () and T.check_metrics([]) == () and T.check_metrics("psnr") == ("psnr",)
    assert T.check_metrics(["ssim", "mse_x0"]) == ("ssim", "mse_x0")
    for bad in (["mse"], ["psnr", "psnr"], [3], ["ssim", "PSNR"]):
        with pytest.raises(ValueError):
            T.check_metrics(bad)

    class NoEngine:
        engine = None

    tr = g.Trainer(NoEngine())
    assert tr.metrics == ()
    tr.compile(g.Adam(1e-3), g.identity)                         # the two-argument form
    assert tr.metrics == ()
    tr.compile(g.Adam(1e-3), g.identity, metrics=["ssim", "psnr"])
    assert tr.metrics == ("ssim", "psnr")
    optimizer = tr.optimizer
    with pytest.raises(ValueError, match="unknown metric"):
        tr.compile(g.Adam(1e-3), g.identity, metrics=["accuracy"])
    assert tr.metrics == ("ssim", "psnr") and tr.optimizer is optimizer        # a refused compile changes nothing
    tr.compile(g.Adam(1e-3), g.identity)
    assert tr.metrics == ()


# ---- 5. every GCT2_EINVAL class, fake pointers, no device -----------------------------------------------------------------------------------
P = 0x7F0000000000          # fake, 16-byte aligned "device" addresses; never dereferenced: every row is refused before any launch


def call(**over):
    """the arguments of gct2_image_metrics, all valid (B=2, 16 x 16 x 3, K=11, 2 x 1 x 3 pairs of scratch), then `over`"""
    a = dict(pred=P, noised=P + 0x10000, u=P + 0x20000, v=P + 0x20100, x=P + 0x30000, window=P + 0x40000, K=11, max_val=2.0, k1=0.01, k2=0.03,
             mse=P + 0x50000, psnr=P + 0x50100, ssim=P + 0x50200, scratch=P + 0x60000, scratch_floats=24, B=2, H=16, W=16, C=3, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values())


NULL_POINTER = "image_metrics: null pointer"
ALIGN = "image_metrics: scratch must be 16-byte aligned, the other pointers 4-byte aligned"
CASES = [
    (call(pred=None), NULL_POINTER), (call(x=None), NULL_POINTER), (call(mse=None), NULL_POINTER), (call(scratch=None), NULL_POINTER),
    (call(noised=None), "image_metrics: u without noised or v"), (call(v=None), "image_metrics: u without noised or v"),
    (call(u=None), "image_metrics: noised or v without u"), (call(u=None, noised=None), "image_metrics: noised or v without u"),
    (call(u=None, v=None), "image_metrics: noised or v without u"),
    (call(window=None), "image_metrics: ssim without window"),
    (call(B=0), "image_metrics: non-positive dims B=0 H=16 W=16"), (call(H=-1), "image_metrics: non-positive dims B=2 H=-1 W=16"),
    (call(W=0), "image_metrics: non-positive dims B=2 H=16 W=0"),
    (call(C=0), "image_metrics: C=0 outside 1..4"), (call(C=5), "image_metrics: C=5 outside 1..4"),
    (call(K=0), "image_metrics: K=0 outside 1..16"), (call(K=17), "image_metrics: K=17 outside 1..16"),
    (call(H=10), "image_metrics: a 10 x 16 image is smaller than the 11 x 11 window"),
    (call(W=10), "image_metrics: a 16 x 10 image is smaller than the 11 x 11 window"),
    (call(max_val=0.0), "image_metrics: max_val must be finite and > 0"), (call(max_val=-2.0), "image_metrics: max_val must be finite and > 0"),
    (call(max_val=float("inf")), "image_metrics: max_val must be finite and > 0"),
    (call(max_val=float("nan")), "image_metrics: max_val must be finite and > 0"),
    (call(k1=-0.01), "image_metrics: k1 and k2 must be finite and >= 0"), (call(k2=float("nan")), "image_metrics: k1 and k2 must be finite and >= 0"),
    (call(k2=float("inf")), "image_metrics: k1 and k2 must be finite and >= 0"),
    (call(pred=P + 2), ALIGN), (call(x=P + 1), ALIGN), (call(noised=P + 0x10002), ALIGN), (call(u=P + 0x20001), ALIGN), (call(v=P + 0x20103), ALIGN),
    (call(window=P + 0x40002), ALIGN), (call(mse=P + 0x50002), ALIGN), (call(psnr=P + 0x50102), ALIGN), (call(ssim=P + 0x50201), ALIGN),
    (call(scratch=P + 0x60004), ALIGN), (call(scratch=P + 0x60008), ALIGN),
    (call(B=65536, H=11, W=11, C=1, scratch_floats=1 << 20), "image_metrics: B=65536 above 65535 (one grid row per image)"),
    (call(B=32768, H=256, W=256, C=1, scratch_floats=1 << 24), "image_metrics: B*H*W*C at or beyond 2^31"),
    (call(scratch_floats=23), "image_metrics: 23 floats of scratch, this shape needs 24 (gct2_image_metrics_scratch)"),
    (call(H=33, scratch_floats=24), "image_metrics: 24 floats of scratch, this shape needs 48 (gct2_image_metrics_scratch)"),
    # accepted without SSIM: a small image, no window - refused for the next mistake in line
    (call(ssim=None, window=None, H=4, W=4, scratch_floats=23), "image_metrics: 23 floats of scratch, this shape needs 24 (gct2_image_metrics_scratch)"),
    # the order of two mistakes: the earlier class of the header's list wins
    (call(pred=None, u=None), NULL_POINTER),
    (call(noised=None, window=None), "image_metrics: u without noised or v"),
    (call(window=None, C=9), "image_metrics: ssim without window"),
    (call(K=17, H=10), "image_metrics: K=17 outside 1..16"),
    (call(H=10, max_val=0.0), "image_metrics: a 10 x 16 image is smaller than the 11 x 11 window"),
    (call(max_val=0.0, pred=P + 2), "image_metrics: max_val must be finite and > 0"),
    (call(pred=P + 2, B=65536), ALIGN),
    (call(B=65536, H=11, W=11, C=1, scratch_floats=0), "image_metrics: B=65536 above 65535 (one grid row per image)"),
]
SCRATCH_CASES = [
    ([2, 16, 16, 3, 11, None], "image_metrics_scratch: null output pointer"),
    ([0, 16, 16, 3, 11, "out"], "image_metrics_scratch: non-positive dims B=0 H=16 W=16"),
    ([2, 16, 16, 5, 11, "out"], "image_metrics_scratch: C=5 outside 1..4"),
    ([2, 16, 16, 3, 0, "out"], "image_metrics_scratch: K=0 outside 1..16"),
    ([65536, 1, 1, 1, 1, "out"], "image_metrics_scratch: B=65536 above 65535 (one grid row per image)"),
    ([32768, 256, 256, 1, 1, "out"], "image_metrics_scratch: B*H*W*C at or beyond 2^31"),
]


def _child():
    """runs the rows against the library and prints one JSON line: {"device": code of gct2_device_check, "results": [[code, text], ...]}"""
    spec = importlib.util.spec_from_file_location("gct2_lib", os.path.join(ROOT, "gan-class-transfer2_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    lib = L.load()
    out = {"device": lib.gct2_device_check(), "results": [], "scratch": []}
    if out["device"] == ENODEV:
        for args, _text in CASES:
            code = lib.gct2_image_metrics(*args)
            out["results"].append([code, lib.gct2_last_error().decode()])
        need = ctypes.c_size_t(0)
        for args, _text in SCRATCH_CASES:
            code = lib.gct2_image_metrics_scratch(*[ctypes.byref(need) if a == "out" else a for a in args])
            out["scratch"].append([code, lib.gct2_last_error().decode()])
    print(json.dumps(out))


def test_rejected_calls_keep_their_codes_and_texts():
    env = dict(os.environ)
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if out["device"] != ENODEV:
        pytest.skip(f"a device is visible to the child process (gct2_device_check() = {out['device']}): fake pointers are not sent to it")
    for rows, got in ((CASES, out["results"]), (SCRATCH_CASES, out["scratch"])):
        assert len(got) == len(rows)
        wrong = [(k, have, text) for k, ((_a, text), have) in enumerate(zip(rows, got)) if have != [EINVAL, text]]
        assert not wrong, wrong


if __name__ == "__main__":
    _child()
