"""CPU tier of the device-resident image cache: the restated draw of tests/data_cache_cases.py is a uniform permutation with draws in
range, data.sample_picks equals it, the stream cuts into batches and shards as identities, the loader state is one integer, and the C
entry point is declared, exported, bound, plannable and rejects bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import data_cache_cases as D
import gan_class_transfer2_amd as g
from gan_class_transfer2_amd import data as data_mod

P = 4096                    # a fake, 16-byte aligned device address: every call below is rejected before anything reads it
EINVAL = 1
HW = np.array(D.SOURCE_HW, dtype=np.int32)


# ---- the permutation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", D.PERMUTATION_NS)
def test_every_epoch_is_a_permutation_and_epochs_differ(N):
    for seed in D.SEEDS:
        perms = [D.permutation(seed, e, N) for e in D.EPOCHS + [2]]
        for p in perms:
            assert p.shape == (N,) and np.array_equal(np.sort(p), np.arange(N))
        if N >= 16:                                    # (N! orders: below that two epochs may well agree)
            assert not np.array_equal(perms[0], perms[1]) and not np.array_equal(perms[1], perms[3])
        assert all(D.permutation_passes(seed, e, N) <= 64 for e in D.EPOCHS)      # the domain is < 4N: the walk is short
    # data.epoch_permutation, position by position
    got = [data_mod.epoch_permutation(D.SEEDS[2], D.EPOCHS[2], p, N) for p in range(N)]
    assert got == D.permutation(D.SEEDS[2], D.EPOCHS[2], N).tolist()


def test_successive_epochs_differ_at_small_n():
    """at N = 5 there are only 120 orders: over 64 epochs many distinct ones must show up"""
    assert len({tuple(D.permutation(5, e, 5)) for e in range(64)}) > 30


@pytest.mark.parametrize("N, epochs", [(37, 2000), (5, 4000)])
def test_item_by_position_table_is_uniform(N, epochs):
    """a condition, not a tolerance: chi^2 of the table stays below dof + 4 sqrt(2 dof) (1310.9 against 1296 + 204 at N = 37 and 15.3
    against 16 + 22.6 at N = 5, seed 5; a four-round network gives 142 at N = 5)"""
    chi2, dof = D.chi_square(D.position_table(5, N, epochs))
    print(f"N={N} epochs={epochs}: chi^2 = {chi2:.1f}, dof = {dof}, bound = {dof + 4 * np.sqrt(2 * dof):.1f}")
    assert dof == (N - 1) ** 2
    assert chi2 < dof + 4 * np.sqrt(2 * dof)


# ---- data.sample_picks against the restatement ------------------------------------------------------------------------------------------
def test_sample_picks_equals_the_restatement_on_every_gpu_case():
    for size, B, flags, first in D.gpu_cases():
        got = g.sample_picks(D.CASE_SEED, first, B, HW, size, flags)
        assert got.dtype == np.int32 and got.shape == (B, 4)
        assert np.array_equal(got, D.picks_ref(D.CASE_SEED, first, B, HW, size, flags)), (size, B, flags, first)
    for seed in D.SEEDS:
        for flags in D.FLAGS:
            args = (seed, (1 << 32) + 3, 17, HW, 32, flags)
            assert np.array_equal(g.sample_picks(*args, sample_stride=3), D.picks_ref(*args, sample_stride=3))
    wrap = ((1 << 64) - 2, 5, HW, 30, 7)               # the sample index wraps mod 2^64
    assert np.array_equal(g.sample_picks(3, *wrap), D.picks_ref(3, *wrap))
    big = np.array([[100, 4000]] * 1025, dtype=np.int32)
    assert np.array_equal(g.sample_picks(9, 1000, 64, big, 64, 7), D.picks_ref(9, 1000, 64, big, 64, 7))


def test_sample_picks_refuses_what_the_kernel_would_clamp():
    with pytest.raises(ValueError, match="cannot be cropped"):
        g.sample_picks(0, 0, 7, HW, 33, 0)
    for bad in (dict(B=0), dict(size=0), dict(flags=8), dict(sample_stride=0)):
        a = dict(seed=0, first_sample=0, B=4, hw=HW, size=32, flags=7, sample_stride=1)
        a.update(bad)
        with pytest.raises(ValueError):
            g.sample_picks(**a)


def test_draws_stay_in_range_and_are_zero_where_nothing_can_move():
    for size in D.SIZES:
        picks = D.picks_ref(D.CASE_SEED, 0, 7 * 300, HW, size, 7)
        item, oy, ox, flip = picks.T
        H0, W0 = HW[item, 0], HW[item, 1]
        assert (0 <= item).all() and (item < 7).all() and set(flip.tolist()) == {0, 1}
        assert (0 <= oy).all() and (oy <= H0 - size).all() and (0 <= ox).all() and (ox <= W0 - size).all()
        assert (oy[H0 == size] == 0).all() and (ox[W0 == size] == 0).all()
        if size == 32:
            assert (H0 == size).any() and (W0 == size).any()
        for i in range(7):                             # every origin of a small range is reached, both ends included
            if HW[i, 0] - size < 16:
                assert set(oy[item == i].tolist()) == set(range(HW[i, 0] - size + 1)), i
        # every epoch of seven samples holds every item once
        assert all(sorted(item[e * 7:(e + 1) * 7].tolist()) == list(range(7)) for e in range(300))
        centre = D.picks_ref(D.CASE_SEED, 0, 7, HW, size, 0)
        assert np.array_equal(centre, np.stack([np.arange(7), (HW[:, 0] - size) // 2, (HW[:, 1] - size) // 2, np.zeros(7, int)], 1))


def test_batch_cuts_and_shards_are_identities_on_picks():
    seed, size, flags = D.SEEDS[2], 30, 7
    whole = g.sample_picks(seed, 3, 24, HW, size, flags)
    assert np.array_equal(whole, np.concatenate([g.sample_picks(seed, 3 + 4 * i, 4, HW, size, flags) for i in range(6)]))
    assert np.array_equal(whole[:8], np.concatenate([g.sample_picks(seed, 3, 5, HW, size, flags), g.sample_picks(seed, 8, 3, HW, size, flags)]))
    world = 3
    for rank in range(world):
        assert np.array_equal(g.sample_picks(seed, 3 + rank, 8, HW, size, flags, sample_stride=world), whole[rank::world])


# ---- the loader's host arithmetic ---------------------------------------------------------------------------------------------------------
def _host_dataset(monkeypatch, **kw):
    """a CachedImageDataset on the CPU whose launches are recorded instead of made: (first_sample, B, sample_stride) per batch"""
    def batch_at(self, first_sample, B, sample_stride=1, picks_out=None):
        self.log.append((first_sample, B, sample_stride))
        return torch.zeros(B, self.size, self.size, 3)

    monkeypatch.setattr(g.CachedImageDataset, "batch_at", batch_at)
    ds = g.CachedImageDataset(list(D.sources()), device=torch.device("cpu"), **kw)
    ds.log = []
    return ds, ds.log


def test_the_pool_holds_the_images_and_its_spare_bytes(monkeypatch):
    ds, _ = _host_dataset(monkeypatch, size=32, batch_size=4, seed=3)
    pool, offsets, hw = D.pool_layout(D.sources())
    assert len(ds) == 7 and ds.pool.dtype == torch.uint8 and ds.pool.numel() == pool.size and g._lib.DATA_POOL_PAD == D.POOL_PAD == 16
    assert np.array_equal(ds.pool.numpy(), pool) and np.array_equal(ds.offsets_d.numpy(), offsets) and np.array_equal(ds.hw_d.numpy(), hw)
    assert ds.offsets_d.dtype == torch.int64 and ds.hw_d.dtype == torch.int32
    assert (ds.flags, ds.finite) == (7, False)
    assert g.CachedImageDataset([np.zeros((32, 32, 3), np.uint8)], 32, 1, device=torch.device("cpu"), crop=False).flags == 5
    with pytest.raises(ValueError, match="cannot be cropped to 64x64x3"):
        g.CachedImageDataset(list(D.sources()), 64, 4, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="crop=False needs size x size images"):
        g.CachedImageDataset(list(D.sources()), 32, 4, device=torch.device("cpu"), crop=False)
    with pytest.raises(ValueError, match="no files match"):
        g.CachedImageDataset("/nonexistent/*.png", 32, 4, device=torch.device("cpu"))
    # ImageDataset.cache() hands its own settings on; a validation dataset stays one
    base = g.ImageDataset(list(D.sources()), size=30, batch_size=3, device=torch.device("cpu"), seed=11, crop=True)
    c = base.cache(workers=2)
    assert (c.size, c.batch_size, c.seed, c.flags, c.finite, c.shard) == (30, 3, 11, 7, False, (0, 1))
    v = g.ImageDataset.validation(list(D.sources()), size=30, batch_size=3, device=torch.device("cpu")).cache()
    assert (v.flags, v.finite) == (0, True)


def test_iteration_advances_one_integer_and_state_round_trips(monkeypatch):
    ds, log = _host_dataset(monkeypatch, size=32, batch_size=4, seed=(1 << 63) + 9)
    it = iter(ds)
    for _ in range(3):
        x, y = next(it)
        assert x is y and tuple(x.shape) == (4, 32, 32, 3)
    assert log == [(0, 4, 1), (4, 4, 1), (8, 4, 1)]
    state = ds.state_dict()
    assert state == {"seed": (1 << 63) + 9, "next_sample": 12}
    other, log2 = _host_dataset(monkeypatch, size=32, batch_size=4, seed=0)
    other.load_state_dict(dict(state))
    assert other.state_dict() == state
    next(iter(other))
    next(it)
    assert log2 == [(12, 4, 1)] and log[-1] == (12, 4, 1) and len(log) == 4
    assert np.array_equal(other.picks(12, 4), g.sample_picks(state["seed"], 12, 4, HW, 32, 7))


def test_shards_take_interleaved_samples_and_their_union_is_the_stream(monkeypatch):
    world = 3
    seen = []
    for rank in range(world):
        ds, log = _host_dataset(monkeypatch, size=32, batch_size=4, seed=1, shard=(rank, world))
        it = iter(ds)
        next(it), next(it)
        assert log == [(rank, 4, world), (12 + rank, 4, world)] and ds.state_dict()["next_sample"] == 24
        seen += [first + b * stride for first, B, stride in log for b in range(B)]
    assert sorted(seen) == list(range(24))
    with pytest.raises(ValueError, match="rank"):
        _host_dataset(monkeypatch, size=32, batch_size=4, shard=(3, 3))


def test_a_validation_pass_is_finite_and_keeps_the_partial_batch(monkeypatch):
    ds, log = _host_dataset(monkeypatch, size=30, batch_size=3, validation=True)
    assert ds.finite and ds.flags == 0
    assert [tuple(x.shape) for x, _ in ds] == [(3, 30, 30, 3), (3, 30, 30, 3), (1, 30, 30, 3)]
    assert log == [(0, 3, 1), (3, 3, 1), (6, 1, 1)]
    assert len(list(ds)) == 3 and log[3:] == log[:3]   # nothing advanced: the second pass is the first


def test_batches_need_a_device():
    ds = g.CachedImageDataset(list(D.sources()), 32, 4, device=torch.device("cpu"))
    with pytest.raises(g.Gct2Error, match="HIP kernel"):
        next(iter(ds))


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------
def test_image_batch_cached_is_exported_bound_and_plannable():
    L = g._lib
    lib = L.load()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "gct2_image_batch_cached")
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    assert L.SIGNATURES["gct2_image_batch_cached"] == [vp, vp, vp, i, u64, u64, u64, i, vp, vp, vp, i, i, vp]
    assert "gct2_image_batch_cached" in L.PLANNABLE
    assert lib.gct2_abi_version() == L.ABI_VERSION == 17              # an addition changes no signature
    assert (L.DATA_SHUFFLE, L.DATA_RANDOM_CROP, L.DATA_FLIP) == (D.SHUFFLE, D.RANDOM_CROP, D.FLIP) == (1, 2, 4)
    from gan_class_transfer2_amd import trainer_math as TM
    assert (TM.DATA_STREAM_AUG, TM.DATA_STREAM_ORDER) == (D.STREAM_AUG, D.STREAM_ORDER) == (6, 7)
    plan = L.Plan()
    idx = ctypes.c_int(-1)
    arr = (ctypes.c_uint64 * 14)()
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_image_batch_cached", arr, 14, ctypes.byref(idx)) == 0 and idx.value == 0
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_image_batch_cached", arr, 13, None) == EINVAL
    assert b"takes 14 arguments" in lib.gct2_last_error()
    # the recorded call (all-zero arguments) is rejected by its own checks when the plan runs: nothing is launched
    failed = ctypes.c_int(-1)
    assert lib.gct2_plan_run(plan.handle, 0, 1, ctypes.byref(failed)) == EINVAL and failed.value == 0
    assert b"image_batch_cached: null pointer" in lib.gct2_last_error()


def _args(**o):
    a = dict(pool=P, offsets=P + 4096, hw=P + 8192, N=7, seed=1, first_sample=0, sample_stride=1, flags=7, picks_in=None, picks_out=None,
             dst=P + 12288, B=4, size=32, stream=None)
    assert not set(o) - set(a)
    a.update(o)
    return list(a.values())


@pytest.mark.parametrize("args, text", [
    (_args(pool=None), "null pointer"),
    (_args(offsets=None), "null pointer"),
    (_args(hw=None), "null pointer"),
    (_args(dst=None), "null pointer"),
    (_args(B=0), "must be positive"),
    (_args(B=-3), "must be positive"),
    (_args(N=0), "must be positive"),
    (_args(N=-1), "must be positive"),
    (_args(size=0), "must be positive"),
    (_args(size=-32), "must be positive"),
    (_args(size=16385), "larger than 16384"),
    (_args(flags=8), "unknown flag bits"),
    (_args(flags=-1), "unknown flag bits"),
    (_args(sample_stride=0), "sample_stride == 0"),
    (_args(size=16384, B=1 << 20), "work-groups"),
])
def test_image_batch_cached_rejects_bad_arguments_without_a_device(args, text):
    lib = g._lib.load()
    assert lib.gct2_image_batch_cached(*args) == EINVAL
    msg = lib.gct2_last_error().decode()
    assert msg.startswith("image_batch_cached: ") and text in msg, msg


# ---- what the GPU cases can tell apart ------------------------------------------------------------------------------------------------------
def test_gpu_cases_reach_every_source_alignment_flipped_and_not():
    _, offsets, hw = D.pool_layout(D.sources())
    assert {int(o) % 4 for o in offsets} == {0, 1, 3} and sorted(D.SIZES) == [30, 32] and 32 % 4 == 0 and 30 % 4 != 0
    seen = set()
    for size, B, flags, first in D.gpu_cases():
        if size % 4 == 0:
            seen |= D.source_alignments(D.picks_ref(D.CASE_SEED, first, B, hw, size, flags), offsets, hw, size)
    assert seen == {(m, f) for m in range(4) for f in (0, 1)}
    # an epoch boundary falls inside the batches that start at N - 2, and 2^32 + 3 needs the high word of the sample index
    assert D.FIRST_SAMPLES == [0, 5, (1 << 32) + 3] and len(D.SOURCE_HW) == 7
    a = D.picks_ref(D.CASE_SEED, (1 << 32) + 3, 5, hw, 32, 7)
    assert not np.array_equal(a, D.picks_ref(D.CASE_SEED, 3, 5, hw, 32, 7))
