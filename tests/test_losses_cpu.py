"""CPU tier of the training losses (train.py:254-280; gct2_loss_fwd_bwd): the float64 restatement of tests/loss_cases.py against torch
autograd and scipy, the two entry points declared, exported, bound and (the launching one) plannable, every rejection before any
launch, and the host logic that carries the `training_loss` global from the module to the engine's call list."""
import ctypes
import types

import numpy as np
import pytest
import torch

import gan_class_transfer2_amd as g
import loss_cases as K

P = 4096                    # a fake, 16-byte aligned device address: every call below is rejected before anything reads it
EINVAL = 1


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _autograd(kind, pred, target, G=None):
    p = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(target, dtype=torch.float64)
    if kind == "l1":
        loss = torch.maximum(t - p, p - t).mean()
    elif kind == "mse":
        loss = ((t - p) ** 2).mean()
    elif kind == "mse_pooled":
        pool = lambda a: torch.nn.functional.avg_pool2d(a.permute(0, 3, 1, 2), 16, 16)
        loss = ((t - p) ** 2).mean() + ((pool(t) - pool(p)) ** 2).mean()
    else:
        Gt = torch.tensor(np.asarray(G, np.float64))
        D = (t - p).permute(0, 3, 1, 2)
        loss = ((Gt @ D @ Gt.T) ** 2).mean()
    loss.backward()
    return float(loss.detach()), p.grad.numpy()


@pytest.mark.parametrize("kind, shape", [("mse", (2, 5, 7, 3)), ("l1", (2, 5, 7, 3)), ("mse_pooled", (2, 16, 32, 3)), ("dct", (2, 20, 20, 3))])
def test_restatement_equals_torch_autograd(kind, shape):
    rng = np.random.default_rng(3)
    pred, target = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    G = g.trainer_math.dct_basis(shape[1]) if kind == "dct" else None
    r = K.restate(K.KINDS[kind], pred, target, G)
    # (the restatement takes d = fl32(target - pred); autograd gets that same d as its residual)
    d = K.residual(pred, target).astype(np.float64)
    loss, grad = _autograd(kind, np.zeros(shape), d, G)
    assert abs(r["loss"] - loss) <= 1e-12 * abs(loss)
    assert np.allclose(r["dpred"], grad, rtol=1e-11, atol=1e-15)
    # the stated float32 rounding of the gradient stays within a few float32 ulps of its largest element
    assert np.abs(r["dpred_bits"] - r["dpred"]).max() <= 4 * 2.0 ** -24 * np.abs(r["dpred"]).max()
    # the loss scale multiplies the gradient and nothing else
    r2 = K.restate(K.KINDS[kind], pred, target, G, s=2.0 ** 15)
    assert r2["loss"] == r["loss"] and np.array_equal(r2["dpred_bits"], r["dpred_bits"] * np.float32(2.0 ** 15))


def test_l1_tie_and_nan_convention():
    """maximum(t - p, p - t) under TF's _MaximumGrad (x >= y): a tie sends the gradient to the first operand (d(t - p)/dp = -1), a NaN
    to the second (+1)"""
    pred = np.array([[[[0.0], [1.0], [2.0], [np.nan]]]], np.float32)
    target = np.array([[[[0.0], [3.0], [1.0], [1.0]]]], np.float32)
    r = K.l1(pred, target)
    c = np.float32(0.25)
    assert np.array_equal(r["dpred_bits"].ravel(), [-c, -c, c, c])
    assert np.isnan(r["loss"])
    assert K.l1(pred[..., :3, :], target[..., :3, :])["loss"] == (0.0 + 2.0 + 1.0) / 3


@pytest.mark.parametrize("size", [4, 20, 128, 256])
def test_dct_basis_is_the_orthonormal_dct_times_the_frequency_weights(size):
    G = g.trainer_math.dct_basis(size)
    assert G.dtype == np.float32 and G.shape == (size, size)
    ref = K.dct_basis_reference(size)
    assert np.array_equal(G, ref.astype(np.float32))                   # float64, rounded once
    # without the weights the rows are orthonormal
    W = ref * (np.arange(size) + 1.0)[:, None]
    assert np.abs(W @ W.T - np.eye(size)).max() < 1e-13
    fft = pytest.importorskip("scipy.fft")
    x = np.random.default_rng(size).standard_normal((3, size))
    want = fft.dct(x, norm="ortho", axis=-1) / (np.arange(size) + 1.0)
    assert np.abs(x @ ref.T - want).max() < 1e-14 * size


def test_exact_basis_bound():
    rng = np.random.default_rng(1)
    for size in (4, 20, 48, 144):
        G = K.signed_permutation_basis(rng, size)
        assert K.assert_exact_bound(G) == (64, 4096)
        pred, target = K.exact_pair(rng, (2, size, size, 3))
        d = K.residual(pred, target)
        assert set(np.unique(d)) <= {-1.0, 0.0, 1.0}
        E, V = K.dct_planes(d, G)
        assert np.abs(E).max() <= 64 and np.abs(V).max() <= 4096
        E32, V32 = K.dct_planes(d, G, np.float32)                       # exact in float32 too, whatever the order
        assert np.array_equal(E32, E) and np.array_equal(V32, V)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_loss_entry_points_are_declared_exported_bound_and_plannable():
    L = g._lib
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(raw, "gct2_loss_fwd_bwd") and hasattr(raw, "gct2_loss_scratch")
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert L.SIGNATURES["gct2_loss_fwd_bwd"] == [i, vp, vp, vp, vp, vp, sz, i, i, i, i, vp, vp, vp]
    assert L.SIGNATURES["gct2_loss_scratch"] == [i, i, i, i, i, ctypes.POINTER(sz)]
    assert "gct2_loss_fwd_bwd" in L.PLANNABLE and "gct2_loss_scratch" not in L.PLANNABLE
    assert (L.LOSS_MSE, L.LOSS_L1, L.LOSS_MSE_POOLED, L.LOSS_DCT) == (0, 1, 2, 3) == (K.MSE, K.L1, K.MSE_POOLED, K.DCT)
    assert lib.gct2_abi_version() == L.ABI_VERSION == 17              # an addition changes no signature
    header = open(L.os.path.join(L._HERE, "..", "include", "gct2.h")).read()
    for name, code in (("MSE", 0), ("L1", 1), ("MSE_POOLED", 2), ("DCT", 3)):
        assert f"#define GCT2_LOSS_{name} {code}" in header
    plan = L.Plan()
    idx = ctypes.c_int(-1)
    arr = (ctypes.c_uint64 * 14)()
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_loss_fwd_bwd", arr, 14, ctypes.byref(idx)) == 0 and idx.value == 0
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_loss_fwd_bwd", arr, 13, None) == EINVAL
    assert b"takes 14 arguments" in lib.gct2_last_error()
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_loss_scratch", arr, 6, None) == EINVAL and b"not an entry point" in lib.gct2_last_error()
    # the recorded call (all-zero arguments) is rejected by its own checks when the plan runs: nothing is launched
    failed = ctypes.c_int(-1)
    assert lib.gct2_plan_run(plan.handle, 0, 1, ctypes.byref(failed)) == EINVAL and failed.value == 0
    assert b"loss_fwd_bwd: " in lib.gct2_last_error()


def _scratch(kind, B, H, W, C):
    need = ctypes.c_size_t(0)
    rc = g._lib.load().gct2_loss_scratch(kind, B, H, W, C, ctypes.byref(need))
    return rc, need.value


def _loss(**o):
    a = dict(kind=K.L1, pred=P, target=P + 65536, dpred=P + 131072, loss=P + 196608, scratch=P + 262144, scratch_floats=1 << 24,
             B=2, H=16, W=16, C=3, basis=P + (1 << 27), ls=None, stream=None)
    assert not set(o) - set(a)
    a.update(o)
    return list(a.values())


@pytest.mark.parametrize("args, text", [
    (_loss(kind=4), "unknown loss kind 4"),
    (_loss(kind=-1), "unknown loss kind -1"),
    (_loss(pred=None), "null pointer"),
    (_loss(target=None), "null pointer"),
    (_loss(loss=None), "null pointer"),
    (_loss(scratch=None), "null pointer"),
    (_loss(kind=K.MSE, scratch_floats=1023), "1023 floats of scratch"),
    (_loss(kind=K.L1, scratch_floats=0), "floats of scratch"),
    (_loss(kind=K.MSE_POOLED, B=64, H=128, W=128, scratch_floats=4 * 64 * 64 - 1), "floats of scratch"),
    (_loss(kind=K.DCT, scratch_floats=2 * 16 * 16 * 3), "floats of scratch"),
    (_loss(kind=K.MSE_POOLED, H=24), "multiples of 16"),
    (_loss(kind=K.MSE_POOLED, W=8), "multiples of 16"),
    (_loss(kind=K.DCT, W=32), "H == W == size"),
    (_loss(kind=K.DCT, H=18, W=18), "multiple of 4"),
    (_loss(kind=K.DCT, basis=None), "needs a basis"),
    (_loss(kind=K.DCT, basis=P + 8), "16-byte aligned"),
    (_loss(scratch=P + 262144 + 4), "16-byte aligned"),
    (_loss(pred=P + 2), "4-byte aligned"),
    (_loss(dpred=P + 131072 + 1), "4-byte aligned"),
    (_loss(B=0), "must be positive"),
    (_loss(H=-16), "must be positive"),
    (_loss(W=0), "must be positive"),
    (_loss(C=0), "C=0 in 1..4"),
    (_loss(C=5), "C=5 in 1..4"),
    # two mistakes: the kind and the shape are checked before the pointers
    (_loss(kind=9, pred=None), "unknown loss kind 9"),
    (_loss(kind=K.MSE_POOLED, H=24, pred=None), "multiples of 16"),
])
def test_loss_fwd_bwd_rejects_bad_arguments_without_a_device(args, text):
    lib = g._lib.load()
    assert lib.gct2_loss_fwd_bwd(*args) == EINVAL
    msg = lib.gct2_last_error().decode()
    assert msg.startswith("loss_fwd_bwd: ") and text in msg, msg


def test_loss_scratch_sizes():
    lib = g._lib.load()
    for kind in range(4):
        for shape in ((2, 16, 16, 3), (1, 16, 16, 1), (64, 128, 128, 3), (8, 256, 256, 3)):
            rc, need = _scratch(kind, *shape)
            n = int(np.prod(shape))
            assert rc == 0 and need >= 1024 and need % 4 == 0
            if kind == K.DCT:
                assert n + 1024 <= need <= n + max(1024, n // 64)      # one plane set plus the partial sums
            else:
                assert need <= max(1024, n // 64)
    assert _scratch(K.L1, 3, 5, 7, 3) == (0, 1024) and _scratch(K.MSE, 1, 1, 100003, 1) == (0, 1024)
    assert _scratch(K.MSE_POOLED, 64, 128, 128, 3) == (0, 4 * 64 * 64)  # two fp64 sums per 16 x 16 cell
    for bad in ((4, 2, 16, 16, 3), (K.MSE_POOLED, 2, 24, 16, 3), (K.DCT, 2, 16, 32, 3), (K.DCT, 2, 18, 18, 3), (K.L1, 0, 16, 16, 3),
                (K.L1, 2, 16, 16, 5)):
        assert _scratch(*bad)[0] == EINVAL and lib.gct2_last_error().decode().startswith("loss_scratch: ")
    assert lib.gct2_loss_scratch(K.L1, 2, 16, 16, 3, None) == EINVAL


# ---- host logic ------------------------------------------------------------------------------------------------------------------------
class _Calls:
    """stands in for _lib.call in the modules under test: the host logic below runs without a device and nothing is launched"""

    def __init__(self):
        self.log = []

    def __call__(self, name, *args):
        self.log.append((name, args))


def _host_engine(monkeypatch, B=2, H=32, W=32, **kw):
    """a UNetEngine with only the attributes the loss dispatch reads, and a CPU buffer set"""
    from gan_class_transfer2_amd import engine as E, trainer_math as TM

    class Stub(E.UNetEngine):
        def __init__(self, **a):
            self.__dict__.update(a)

        def _stream(self):
            return 0

    calls = _Calls()
    monkeypatch.setattr(E, "call", calls)
    monkeypatch.setattr(TM, "call", calls)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    b = types.SimpleNamespace(B=B, H=H, W=W, pred=z(B, H, W, 3), dpred=z(B, H, W, 3), loss=z(1), partials=z(1024), loss_store={})
    eng = Stub(lib=g._lib.load(), device=torch.device("cpu"), ls_state=None, dtype=g.BF16, use_fused_head=True, workspace=object(),
               topo=g.Topology(128, 512, 6), predict_x=True, prediction_weighting=False, ordinary_differential_equation=False, **kw)
    return eng, b, calls


def test_default_engine_calls_what_it_called_before(monkeypatch):
    eng, b, calls = _host_engine(monkeypatch)
    assert eng.training_loss == "mse" and g.trainer_math.TRAINING_LOSSES == ("mse", "l1", "mse_pooled", "dct")
    assert eng.fused_head_ok()
    x = torch.zeros(2, 32, 32, 3)
    assert eng.loss_and_dpred(b, x, True) is b.loss
    (name, args), = calls.log
    assert name == "gct2_mse_fwd_bwd" and b.loss_store == {}           # nothing new is named, nothing new is allocated
    assert isinstance(args[1], g._lib.Slot) and args[1].key == "x" and args[1].value == x.data_ptr()
    assert args[0] == b.pred.data_ptr() and args[2:] == (b.dpred.data_ptr(), b.loss.data_ptr(), b.partials.data_ptr(), b.pred.numel(), None, 0)
    del calls.log[:]
    eng.loss_and_dpred(b, x, grad=False)                                # Trainer.call with "mse": the same call as ever
    assert calls.log[0][0] == "gct2_mse_fwd_bwd" and calls.log[0][1][2] == b.dpred.data_ptr()


@pytest.mark.parametrize("kind", ["l1", "mse_pooled", "dct"])
def test_other_kinds_go_through_loss_fwd_bwd(monkeypatch, kind):
    eng, b, calls = _host_engine(monkeypatch)
    eng.training_loss = kind
    assert not eng.fused_head_ok()                                      # the head kernels carry the MSE only
    x = torch.zeros(2, 32, 32, 3)
    eng.loss_and_dpred(b, x, True)
    (name, a), = calls.log
    assert name == "gct2_loss_fwd_bwd" and a[0] == K.KINDS[kind]
    (scratch, basis), = b.loss_store.values()                           # allocated on first use, kept with the buffer set
    need = _scratch(K.KINDS[kind], 2, 32, 32, 3)[1]
    assert scratch.numel() == need and scratch.dtype == torch.float32
    assert a[1] == b.pred.data_ptr() and isinstance(a[2], g._lib.Slot) and a[2].key == "x" and a[2].value == x.data_ptr()
    assert a[3:11] == (b.dpred.data_ptr(), b.loss.data_ptr(), scratch.data_ptr(), need, 2, 32, 32, 3) and a[12:] == (None, 0)
    if kind == "dct":
        assert a[11] == basis.data_ptr() and np.array_equal(basis.numpy(), g.trainer_math.dct_basis(32))
    else:
        assert basis is None and a[11] is None
    del calls.log[:]
    eng.loss_and_dpred(b, x, grad=False)                                # Trainer.call: no gradients -> dpred = NULL, the same scratch
    assert calls.log[0][1][3] is None and calls.log[0][1][5] == scratch.data_ptr() and len(b.loss_store) == 1
    # prediction_weighting composes around it: scale the prediction, the loss, scale the gradient - and no gradient pass without one
    del calls.log[:]
    w = torch.ones(2)
    eng.weighted_loss_and_dpred(b, x, w)
    assert [n for n, _ in calls.log] == ["gct2_mix_per_image", "gct2_loss_fwd_bwd", "gct2_mix_per_image"]
    del calls.log[:]
    eng.weighted_loss_and_dpred(b, x, w, grad=False)
    assert [n for n, _ in calls.log] == ["gct2_mix_per_image", "gct2_loss_fwd_bwd"]


def test_a_shape_the_kind_refuses_raises_before_any_call(monkeypatch):
    eng, b, calls = _host_engine(monkeypatch, H=24, W=24)
    b.pred = torch.zeros(2, 24, 24, 3)
    eng.training_loss = "mse_pooled"
    with pytest.raises(g.Gct2Error, match="multiples of 16"):
        eng.loss_and_dpred(b, torch.zeros(2, 24, 24, 3))
    assert calls.log == [] and b.loss_store == {}


def test_training_loss_global_reaches_the_engine():
    M = g.model
    assert M.training_loss == "mse"
    seen = []
    eng = types.SimpleNamespace(training_loss="mse")
    den = types.SimpleNamespace(engine=eng, ensure_engine=lambda **kw: (seen.append(kw), eng)[1])
    tr = M.Trainer(den)
    try:
        for kind in ("dct", "l1", "mse_pooled", "mse"):
            M.configure(training_loss=kind)
            assert tr._engine() is eng and eng.training_loss == kind
            assert all(getattr(eng, k) == v for k, v in M.objective_switches().items())
        assert set(M.objective_switches()) == set(g.trainer_math.OBJECTIVE_SWITCHES)       # the four objective globals, as before
        M.configure(training_loss="huber")
        with pytest.raises(ValueError, match="unknown training_loss 'huber'"):
            tr._engine()
        assert eng.training_loss == "mse" and len(seen) == 4            # refused before anything was built or changed
    finally:
        M.configure(training_loss="mse")


def test_plan_key_names_the_kind():
    import inspect
    from gan_class_transfer2_amd import engine as E
    assert "self.training_loss" in inspect.getsource(E.UNetEngine._plan_key)
