"""CPU tier of evaluation (Trainer.evaluate, fit(validation_data=...), gct2_eval_loss_rows): the float64 restatement of
tests/eval_cases.py against the batch losses of tests/loss_cases.py, the two entry points declared, exported, bound and (the launching
one) plannable, every rejection before any launch, loss_by_timestep, the finite validation pass of ImageDataset on the host, and the
argument checks of fit / evaluate that need no device."""
import ctypes

import numpy as np
import pytest
import torch

import eval_cases as E
import gan_class_transfer2_amd as g
import loss_cases as K

P = 4096                    # a fake, 16-byte aligned device address: every call below is rejected before anything reads it
EINVAL = 1
SHAPES = {K.MSE: (3, 5, 7, 3), K.L1: (3, 5, 7, 3), K.MSE_POOLED: (2, 32, 16, 1), K.DCT: (3, 20, 20, 3)}


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [K.MSE, K.L1, K.MSE_POOLED, K.DCT])
@pytest.mark.parametrize("mode", E.MODES)
def test_mean_of_the_rows_is_the_batch_loss(kind, mode):
    rng = np.random.default_rng(5)
    shape = SHAPES[kind]
    v = E.real_inputs(rng, shape, kind, g.trainer_math.dct_basis(shape[1]))
    eps, a, c, w = E.mode_arguments(mode, v["eps"], v["a"], v["c"], v["w"])
    d = E.residual(v["pred"], v["x"], eps, a, c, w)
    got = E.rows(kind, v["pred"], v["x"], eps, a, c, w, v["G"])
    assert got.shape == (shape[0],) and got.dtype == np.float64
    # loss_cases takes (pred, target) and forms d = fl32(target - pred): hand it this d as the target of a zero prediction
    want = K.restate(kind, np.zeros(shape, np.float32), d, v["G"])["loss"]
    assert abs(got.mean() - want) <= 1e-12 * abs(want), (got.mean(), want)
    # ... and each row is that loss on the image alone
    for b in range(shape[0]):
        one = K.restate(kind, np.zeros((1,) + shape[1:], np.float32), d[b:b + 1], v["G"])["loss"]
        assert abs(got[b] - one) <= 1e-12 * abs(one)


def test_residual_follows_the_mix_rule():
    f = np.float32
    x, eps, pred = np.full((2, 1, 1, 1), f(0.1)), np.full((2, 1, 1, 1), f(0.7)), np.full((2, 1, 1, 1), f(0.3))
    a, c, w = np.array([3.0, 0.5], f), np.array([0.3, 7.0], f), np.array([1.1, 0.9], f)
    assert np.array_equal(E.residual(pred, x), x - pred)
    assert np.array_equal(E.residual(pred, x, None, a).ravel(), [f(a[b] * f(0.1)) - f(0.3) for b in range(2)])
    want = [f(f(f(a[b] * f(0.1)) + f(c[b] * f(0.7))) - f(w[b] * f(0.3))) for b in range(2)]
    assert np.array_equal(E.residual(pred, x, eps, a, c, w).ravel(), want)
    with pytest.raises(ValueError):
        E.residual(pred, x, None, a, c)


@pytest.mark.parametrize("kind, shape", [(K.MSE, (3, 5, 7, 3)), (K.L1, (3, 5, 7, 3)), (K.MSE_POOLED, (2, 32, 16, 1)), (K.DCT, (3, 8, 8, 3)),
                                         (K.DCT, (3, 20, 20, 3))])
def test_exact_inputs_are_exact(kind, shape):
    rng = np.random.default_rng(2)
    v = E.exact_inputs(rng, shape, kind, zero_image=1)
    for mode in E.MODES:
        eps, a, c, w = E.mode_arguments(mode, v["eps"], v["a"], v["c"], v["w"])
        d = E.residual(v["pred"], v["x"], eps, a, c, w)
        E.assert_exact(kind, d, v["G"])
        assert not d[1].any() and d[0].any()
        r = E.rows(kind, v["pred"], v["x"], eps, a, c, w, v["G"])
        assert r[1] == 0.0 and r[0] > 0
        # any summation order gives the same float64 sums: reversed elements, float32 DCT passes
        rev = E.rows_of_residual(kind, d[:, ::-1, ::-1, :].copy(), None if v["G"] is None else v["G"][::-1, ::-1].copy())
        assert np.array_equal(rev, r)
        if kind == K.DCT:
            E32, _ = K.dct_planes(d, v["G"], np.float32)
            assert np.array_equal((E32.astype(np.float64) ** 2).reshape(shape[0], -1).sum(axis=1) / d[0].size, r)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_eval_entry_points_are_declared_exported_bound_and_plannable():
    L = g._lib
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(raw, "gct2_eval_loss_rows") and hasattr(raw, "gct2_eval_loss_scratch")
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert L.SIGNATURES["gct2_eval_loss_rows"] == [i, vp, vp, vp, vp, vp, vp, vp, vp, sz, i, i, i, i, vp, vp]
    assert L.SIGNATURES["gct2_eval_loss_scratch"] == [i, i, i, i, i, ctypes.POINTER(sz)]
    assert "gct2_eval_loss_rows" in L.PLANNABLE and "gct2_eval_loss_scratch" not in L.PLANNABLE
    assert lib.gct2_abi_version() == L.ABI_VERSION == 17              # an addition changes no signature
    header = open(L.os.path.join(L._HERE, "..", "include", "gct2.h")).read()
    assert "int gct2_eval_loss_rows(" in header and "int gct2_eval_loss_scratch(" in header
    plan = L.Plan()
    idx = ctypes.c_int(-1)
    arr = (ctypes.c_uint64 * 16)()
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_eval_loss_rows", arr, 16, ctypes.byref(idx)) == 0 and idx.value == 0
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_eval_loss_scratch", arr, 6, None) == EINVAL


def _scratch(kind, B, H, W, C):
    need = ctypes.c_size_t(0)
    rc = g._lib.load().gct2_eval_loss_scratch(kind, B, H, W, C, ctypes.byref(need))
    return rc, need.value


def _rows(**o):
    a = dict(kind=K.L1, pred=P, x=P + 65536, eps=P + 131072, a=P + 196608, c=P + 196608 + 1024, w=P + 196608 + 2048, rows=P + 196608 + 4096,
             scratch=P + 262144, scratch_floats=1 << 24, B=2, H=16, W=16, C=3, basis=P + (1 << 27), stream=None)
    assert not set(o) - set(a)
    a.update(o)
    return list(a.values())


REJECTED = [
    (_rows(kind=4), "unknown loss kind 4"),
    (_rows(kind=-1), "unknown loss kind -1"),
    (_rows(pred=None), "null pointer"),
    (_rows(x=None), "null pointer"),
    (_rows(rows=None), "null pointer"),
    (_rows(scratch=None), "null pointer"),
    (_rows(B=0), "must be positive"),
    (_rows(H=-16), "must be positive"),
    (_rows(W=0), "must be positive"),
    (_rows(C=0), "C=0 in 1..4"),
    (_rows(C=5), "C=5 in 1..4"),
    (_rows(kind=K.MSE_POOLED, H=24), "multiples of 16"),
    (_rows(kind=K.MSE_POOLED, W=8), "multiples of 16"),
    (_rows(kind=K.DCT, W=32), "H == W == size"),
    (_rows(kind=K.DCT, H=18, W=18), "multiple of 4"),
    (_rows(kind=K.DCT, basis=None), "needs a basis"),
    (_rows(kind=K.DCT, basis=P + 8), "16-byte aligned"),
    (_rows(eps=None), "c without eps"),
    (_rows(c=None), "a and eps without c"),
    (_rows(scratch=P + 262144 + 4), "16-byte aligned"),
    (_rows(pred=P + 2), "4-byte aligned"),
    (_rows(scratch_floats=3), "3 floats of scratch"),
    (_rows(kind=K.MSE_POOLED, B=64, H=128, W=128, scratch_floats=4 * 64 * 64 - 1), "floats of scratch"),
    (_rows(kind=K.DCT, scratch_floats=2 * 2 * 16 * 16 * 3), "floats of scratch"),
    (_rows(B=65536, H=4, W=4), "above 65535"),
    (_rows(B=65535, H=128, W=128), "beyond 2^31"),
    (_rows(B=2, H=32768, W=32768, C=1), "beyond 2^31"),
    # two mistakes: the kind and the shape are checked before the pointers
    (_rows(kind=9, pred=None), "unknown loss kind 9"),
    (_rows(kind=K.MSE_POOLED, H=24, pred=None), "multiples of 16"),
]


@pytest.mark.parametrize("args, text", REJECTED)
def test_eval_loss_rows_rejects_bad_arguments_without_a_device(args, text):
    lib = g._lib.load()
    assert lib.gct2_eval_loss_rows(*args) == EINVAL
    msg = lib.gct2_last_error().decode()
    assert msg.startswith("eval_loss_rows: ") and text in msg, msg


def test_eval_scratch_sizes():
    lib = g._lib.load()
    for kind in range(4):
        for shape in ((2, 16, 16, 3), (1, 16, 16, 1), (64, 128, 128, 3), (8, 256, 256, 3)):
            rc, need = _scratch(kind, *shape)
            n = int(np.prod(shape))
            assert rc == 0 and need >= 4 and need % 4 == 0
            if kind == K.DCT:
                assert 2 * n < need <= 2 * n + max(1024, n // 64)     # the residual plane, the first pass's plane, the partial sums
            else:
                assert need <= max(1024, n // 64)
    assert _scratch(K.L1, 3, 5, 7, 3) == (0, 8)                         # one fp64 partial per image, rounded up to 16 bytes
    assert _scratch(K.MSE_POOLED, 64, 128, 128, 3) == (0, 4 * 64 * 64)  # two fp64 sums per 16 x 16 cell
    for bad in ((4, 2, 16, 16, 3), (K.MSE_POOLED, 2, 24, 16, 3), (K.DCT, 2, 16, 32, 3), (K.DCT, 2, 18, 18, 3), (K.L1, 0, 16, 16, 3),
                (K.L1, 2, 16, 16, 5), (K.L1, 65536, 4, 4, 3), (K.MSE, 65535, 128, 128, 3)):
        assert _scratch(*bad)[0] == EINVAL and lib.gct2_last_error().decode().startswith("eval_loss_scratch: ")
    assert lib.gct2_eval_loss_scratch(K.L1, 2, 16, 16, 3, None) == EINVAL


# ---- loss_by_timestep ------------------------------------------------------------------------------------------------------------------
def test_loss_by_timestep_counts_means_and_empty_bins():
    f = g.trainer_math.loss_by_timestep
    loss = np.array([1.0, 2.0, 4.0, 8.0, 16.0], np.float32)
    t = np.array([1, 6, 1, 3, 6], np.int32)
    counts, means = f(loss, t, 6)
    assert counts.dtype == np.int64 and means.dtype == np.float64
    assert counts.tolist() == [2, 0, 1, 0, 0, 2]
    assert means[[0, 2, 5]].tolist() == [2.5, 8.0, 9.0] and np.isnan(means[[1, 3, 4]]).all()
    # three bins of two timesteps each: t = 1, 2 | 3, 4 | 5, 6
    counts, means = f(torch.tensor(loss), torch.tensor(t), 6, bins=3)
    assert counts.tolist() == [2, 1, 2] and means.tolist() == [2.5, 8.0, 9.0]
    # unequal bins: 7 timesteps in 2 bins are (t - 1) * 2 // 7: t = 1..4 | 5..7
    counts, _ = f(np.ones(7), np.arange(1, 8), 7, bins=2)
    assert counts.tolist() == [4, 3]
    counts, means = f(np.zeros(0), np.zeros(0, np.int32), 4)
    assert counts.tolist() == [0] * 4 and np.isnan(means).all()
    # float64 sums: a float32 accumulation of these would lose the small terms
    counts, means = f(np.array([1e8, 1.0, 1.0, 1.0, 1.0], np.float32), np.ones(5, np.int64), 2)
    assert means[0] == (1e8 + 4.0) / 5
    for bad in (dict(per_image=loss, t=t, steps=5), dict(per_image=loss, t=t[:4], steps=6), dict(per_image=loss, t=t, steps=6, bins=7),
                dict(per_image=loss, t=t, steps=6, bins=0), dict(per_image=loss, t=t.astype(np.float32), steps=6),
                dict(per_image=loss, t=t - 1, steps=6)):
        with pytest.raises(ValueError):
            f(**bad)


# ---- ImageDataset.validation on the host -------------------------------------------------------------------------------------------------
def _images():
    rng = np.random.default_rng(0)
    shapes = [(8, 8), (9, 12), (11, 8), (8, 13), (10, 10)]            # margins 0, odd and even, in both directions
    return [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in shapes]


def test_validation_dataset_is_one_deterministic_ordered_pass():
    imgs = _images()
    ds = g.ImageDataset.validation(imgs, 8, 2, device=torch.device("cpu"))
    assert ds.finite is True
    first = list(ds.host_batches())
    assert [len(b[0]) for b in first] == [2, 2, 1]                      # the partial last batch is kept
    flat = [im for b in first for im in b[0]]
    assert len(flat) == 5 and all(np.array_equal(x, y) for x, y in zip(flat, imgs))        # the order of the source
    dims = np.concatenate([b[1] for b in first])
    assert dims.dtype == np.int32 and dims.shape == (5, 5)
    want = [(H0, W0, (H0 - 8) // 2, (W0 - 8) // 2, 0) for H0, W0 in (im.shape[:2] for im in imgs)]
    assert dims.tolist() == [list(w) for w in want]
    assert dims[1].tolist() == [9, 12, 0, 2, 0] and dims[2].tolist() == [11, 8, 1, 0, 0] and dims[3].tolist() == [8, 13, 0, 2, 0]
    assert not dims[:, 4].any()                                          # no flip
    second = list(ds.host_batches())                                     # iterating again: the same batches
    assert len(second) == len(first)
    for (ia, da), (ib, db) in zip(first, second):
        assert np.array_equal(da, db) and all(np.array_equal(x, y) for x, y in zip(ia, ib))
    with pytest.raises(ValueError):
        list(g.ImageDataset.validation(imgs + [np.zeros((7, 9, 3), np.uint8)], 8, 2, device=torch.device("cpu")).host_batches())


def test_validation_dataset_sorts_files_and_training_mode_is_unchanged(tmp_path):
    imgs = _images()
    names = ["b.npy", "a.npy", "c.npy"]
    for n, im in zip(names, imgs):
        np.save(tmp_path / n, im)
    ds = g.ImageDataset.validation(str(tmp_path / "*.npy"), 8, 4, device=torch.device("cpu"), decoder=np.load)
    (got, dims), = list(ds.host_batches())
    assert [im.shape for im in got] == [imgs[1].shape, imgs[0].shape, imgs[2].shape]        # a.npy, b.npy, c.npy
    # the existing constructor: endless, shuffled, random crops - and says so
    train = g.ImageDataset(imgs, 8, 2, device=torch.device("cpu"), seed=3)
    assert train.finite is False
    it = train.host_batches()
    a = [next(it) for _ in range(4)]
    it2 = g.ImageDataset(imgs, 8, 2, device=torch.device("cpu"), seed=3).host_batches()
    for (ia, da) in a:
        ib, db = next(it2)
        assert np.array_equal(da, db) and len(ia) == 2


# ---- argument checks of evaluate / fit that need no device ---------------------------------------------------------------------------
def test_evaluate_and_fit_refuse_bad_arguments_before_anything_is_built():
    tr = g.Trainer(g.Denoiser())
    endless = g.ImageDataset(_images(), 8, 2, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="never ends"):
        tr.evaluate(endless)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="steps"):
            tr.evaluate([], steps=bad)
    with pytest.raises(RuntimeError, match="compile"):
        tr.fit([], validation_data=[])
    tr.compile(g.Adam(1e-3), g.identity)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="validation_freq"):
            tr.fit([], validation_data=[], validation_freq=bad)
    with pytest.raises(ValueError, match="never ends"):
        tr.fit([], validation_data=endless)
    assert tr.denoiser.engine is None                                    # nothing was built on the way
