"""gct2_image_batch_cached and CachedImageDataset on the GPU, bit for bit: the picks the kernel draws equal data.sample_picks, the
images equal the oracle's decode_contract of the picked source and gct2_image_prepare fed with the same picks, on the four-pixel path
(size 32) and the per-element path (size 30), at every flag set, across an epoch boundary and at a sample index above 2^32.  Outputs
sit between guard rows (tests/test_kernels_exact_gpu.py's idiom); the cases are tests/data_cache_cases.py's, and
tests/test_data_cache_cases_cpu.py shows that they reach every source alignment, flipped and not."""
import numpy as np
import pytest
import torch

import data_cache_cases as D
from oracle import sampler_oracle as S

pytestmark = pytest.mark.gpu

NAN = float("nan")
PICK_GUARD = -77


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


class Pool:
    def __init__(self, imgs, gpu):
        pool, offsets, hw = D.pool_layout(imgs)
        self.imgs, self.offsets, self.hw, self.N = imgs, offsets, hw, len(imgs)
        self.pool_d, self.offsets_d, self.hw_d = (torch.from_numpy(a).to(gpu) for a in (pool, offsets, hw))


@pytest.fixture(scope="module")
def pool(gpu):
    return Pool(D.sources(), gpu)


def run(pool, gpu, B, size, flags=0, first=0, stride=1, picks_in=None, seed=D.CASE_SEED, shift=0, pool_ptr=None):
    """one launch into a NaN-guarded dst and a guarded picks_out; returns (dst [B,size,size,3], picks [B,4]) on the host after
    proving that nothing outside them changed.  shift: dst starts that many floats later (an unaligned dst)"""
    buf = torch.full(((B + 2) * size * size * 3 + 4,), NAN, dtype=torch.float32, device=gpu)
    per = size * size * 3
    lo = per + shift
    picks = torch.full((B + 2, 4), PICK_GUARD, dtype=torch.int32, device=gpu)
    pin = torch.from_numpy(np.ascontiguousarray(picks_in, dtype=np.int32)).to(gpu) if picks_in is not None else None
    lib().call("gct2_image_batch_cached", pool_ptr or pool.pool_d.data_ptr(), pool.offsets_d.data_ptr(), pool.hw_d.data_ptr(), pool.N, seed,
               first, stride, flags, pin.data_ptr() if pin is not None else None, picks[1].data_ptr(), buf.data_ptr() + 4 * lo, B, size, stream())
    torch.cuda.synchronize()
    host = buf.cpu()
    assert torch.isnan(host[:lo]).all() and torch.isnan(host[lo + B * per:]).all(), "dst: a guard element changed"
    assert not torch.isnan(host[lo:lo + B * per]).any(), "dst: an element was not written"
    p = picks.cpu().numpy()
    assert (p[0] == PICK_GUARD).all() and (p[-1] == PICK_GUARD).all(), "picks_out: a guard row changed"
    return host[lo:lo + B * per].reshape(B, size, size, 3).numpy(), p[1:-1]


def contract(pool, picks, size):
    """oracle.sampler_oracle.decode_contract of every pick (float64)"""
    return np.stack([S.decode_contract(pool.imgs[i], oy, ox, bool(fl), size) for i, oy, ox, fl in picks])


def prepared(pool, gpu, picks, size):
    """gct2_image_prepare fed with the same picks, reading the same pool"""
    B = len(picks)
    off = torch.from_numpy(pool.offsets[picks[:, 0]]).to(gpu)
    dims = torch.from_numpy(np.concatenate([pool.hw[picks[:, 0]], picks[:, 1:]], 1).astype(np.int32)).to(gpu)
    out = torch.empty(B, size, size, 3, dtype=torch.float32, device=gpu)
    lib().call("gct2_image_prepare", pool.pool_d.data_ptr(), off.data_ptr(), dims.data_ptr(), out.data_ptr(), B, size, stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("size", D.SIZES)
@pytest.mark.parametrize("B", D.BATCHES)
def test_drawn_batches_are_bit_exact(gpu, pool, size, B):
    import gan_class_transfer2_amd as g
    for flags in D.FLAGS:
        for first in D.FIRST_SAMPLES:
            what = f"size={size} B={B} flags={flags} first_sample={first}"
            x, picks = run(pool, gpu, B, size, flags, first)
            want = g.sample_picks(D.CASE_SEED, first, B, pool.hw, size, flags)
            assert np.array_equal(picks, want), what
            assert np.array_equal(x.astype(np.float64), contract(pool, want, size)), what
            assert same_bits(x, prepared(pool, gpu, want, size)), what
            given, picks2 = run(pool, gpu, B, size, flags, first, picks_in=want)         # nothing drawn: the same bits
            assert np.array_equal(picks2, want) and same_bits(given, x), what


def test_stride_and_seed_reach_the_draw(gpu, pool):
    import gan_class_transfer2_amd as g
    whole, picks = run(pool, gpu, 24, 32, 7, first=3)
    for rank in range(3):                              # the data-parallel slice: rank r of 3 takes every third sample
        x, p = run(pool, gpu, 8, 32, 7, first=3 + rank, stride=3)
        assert np.array_equal(p, picks[rank::3]) and same_bits(x, whole[rank::3])
    for seed in D.SEEDS:
        _, p = run(pool, gpu, 24, 30, 7, first=(1 << 64) - 5, seed=seed)                 # (the sample index wraps mod 2^64)
        assert np.array_equal(p, g.sample_picks(seed, (1 << 64) - 5, 24, pool.hw, 30, 7))


def test_an_unaligned_dst_or_pool_takes_the_per_element_path_with_the_same_bits(gpu, pool):
    aligned, picks = run(pool, gpu, 5, 32, 7, first=1)
    for shift in (1, 2, 3):
        x, p = run(pool, gpu, 5, 32, 7, first=1, shift=shift)
        assert np.array_equal(p, picks) and same_bits(x, aligned)
    # ... and so does a pool that is not 4-byte aligned (the four-pixel path reads aligned dwords)
    for shift in (1, 2, 3):
        moved = torch.zeros(pool.pool_d.numel() + 4, dtype=torch.uint8, device=gpu)
        moved[shift:shift + pool.pool_d.numel()] = pool.pool_d
        x, p = run(pool, gpu, 5, 32, 7, first=1, pool_ptr=moved.data_ptr() + shift)
        assert np.array_equal(p, picks) and same_bits(x, aligned)


@pytest.mark.parametrize("size", D.SIZES)
def test_the_last_image_of_the_pool_at_its_bottom_right_corner(gpu, pool, size):
    """the loads nearest the pool's end, unflipped and flipped"""
    last = pool.N - 1
    H0, W0 = pool.hw[last]
    assert pool.offsets[last] + H0 * W0 * 3 + D.POOL_PAD == pool.pool_d.numel()
    given = np.array([[last, H0 - size, W0 - size, 0], [last, H0 - size, W0 - size, 1], [last, H0 - size, 0, 1]], dtype=np.int32)
    x, picks = run(pool, gpu, 3, size, picks_in=given)
    assert np.array_equal(picks, given) and np.array_equal(x.astype(np.float64), contract(pool, given, size))


def test_offsets_above_4_gib(gpu):
    """one 40 x 40 image at byte 2^32 + 5 of an otherwise uninitialised pool: the address arithmetic is 64-bit"""
    at = (1 << 32) + 5
    big = torch.empty((1 << 32) + (64 << 10), dtype=torch.uint8, device=gpu)
    img = np.random.default_rng(43).integers(0, 256, (40, 40, 3), dtype=np.uint8)
    big[at:at + img.size].copy_(torch.from_numpy(img.reshape(-1)))                       # placed through a view: nothing else is written

    class One:
        imgs, offsets, hw, N = [img], np.array([at], dtype=np.int64), np.array([[40, 40]], dtype=np.int32), 1
        pool_d = big
        offsets_d, hw_d = torch.tensor([at], dtype=torch.int64, device=gpu), torch.tensor([[40, 40]], dtype=torch.int32, device=gpu)

    given = np.array([[0, 0, 0, 0], [0, 0, 0, 1]], dtype=np.int32)
    x, picks = run(One, gpu, 2, 40, picks_in=given)                                      # the four-pixel path: the whole image
    assert np.array_equal(picks, given) and np.array_equal(x.astype(np.float64), contract(One, given, 40))
    given = np.array([[0, 2, 1, 1], [0, 0, 2, 0]], dtype=np.int32)
    x, picks = run(One, gpu, 2, 38, picks_in=given)                                      # the per-element path
    assert np.array_equal(picks, given) and np.array_equal(x.astype(np.float64), contract(One, given, 38))
    x, picks = run(One, gpu, 3, 36, flags=7, first=5)                                    # drawn: N = 1
    assert (picks[:, 0] == 0).all() and np.array_equal(x.astype(np.float64), contract(One, picks, 36))


def clamped(img, oy, ox, flip, size):
    """what include/gct2.h promises for a sample it had to clamp: source pixels beyond the image land on its last row / column"""
    H0, W0 = img.shape[:2]
    ys = np.minimum(oy + np.arange(size), H0 - 1)
    xs = np.minimum(ox + (np.arange(size)[::-1] if flip else np.arange(size)), W0 - 1)
    return img[ys][:, xs].astype(np.float64) / 128 - 1


@pytest.mark.parametrize("size", D.SIZES)
def test_bad_picks_are_clamped_and_reported(gpu, pool, size):
    """a test of the clamp: every address stays inside the picked image, the row reports item = -1, its neighbours keep their bits"""
    good = np.array([[6, 3, 5, 1], [3, 1, 2, 0]], dtype=np.int32)
    bad = np.array([[7, 0, 0, 0], [-1, 0, 1, 1], [1 << 30, 0, 0, 0], [1, 5, 0, 0], [1, 0, 57, 1], [2, -3, 0, 0], [6, 0, -1, 1]], dtype=np.int32)
    given = np.concatenate([good[:1], bad, good[1:]])
    x, picks = run(pool, gpu, len(given), size, picks_in=given)
    assert np.array_equal(picks[[0, -1]], good) and np.array_equal(x[[0, -1]].astype(np.float64), contract(pool, good, size))
    assert (picks[1:-1, 0] == -1).all()
    for row, (item, oy, ox, flip) in enumerate(bad, 1):
        item = min(max(int(item), 0), pool.N - 1)
        H0, W0 = pool.hw[item]
        oy, ox = min(max(int(oy), 0), H0 - size), min(max(int(ox), 0), W0 - size)
        assert picks[row, 1:].tolist() == [oy, ox, flip], row
        assert np.array_equal(x[row].astype(np.float64), S.decode_contract(pool.imgs[item], oy, ox, bool(flip), size)), row


def test_an_image_smaller_than_the_crop_is_clamped_and_reported(gpu, pool):
    size = 36                                          # images 0 .. 4 are smaller in one direction at least
    assert [i for i, (h, w) in enumerate(D.SOURCE_HW) if h < size or w < size] == [0, 1, 2, 3, 4]
    given = np.array([[6, 1, 2, 1], [0, 0, 0, 0], [1, 0, 4, 1], [2, 3, 0, 0], [6, 35, 54, 0]], dtype=np.int32)
    x, picks = run(pool, gpu, 5, size, picks_in=given)
    assert picks[:, 0].tolist() == [6, -1, -1, -1, 6]
    assert np.array_equal(x[[0, 4]].astype(np.float64), contract(pool, given[[0, 4]], size))
    for row in (1, 2, 3):
        item, oy, ox, flip = given[row]
        H0, W0 = pool.hw[item]
        oy, ox = min(oy, max(H0 - size, 0)), min(ox, max(W0 - size, 0))
        assert picks[row, 1:].tolist() == [oy, ox, flip]
        assert np.array_equal(x[row].astype(np.float64), clamped(pool.imgs[item], oy, ox, flip, size)), row
    # drawn from a table with such an entry: the same report
    x, picks = run(pool, gpu, 14, size, flags=7, first=0)
    assert sorted(picks[:, 0].tolist()) == [-1] * 10 + [5, 5, 6, 6]      # two epochs: five of the seven items are too small
    assert (x >= -1).all() and (x < 1).all()
    kept = picks[picks[:, 0] >= 0]
    assert np.array_equal(x[picks[:, 0] >= 0].astype(np.float64), contract(pool, kept, size))


# ---- CachedImageDataset ---------------------------------------------------------------------------------------------------------------------
def take(ds, n):
    it = iter(ds)
    out = [next(it)[0] for _ in range(n)]
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def test_cached_dataset_is_a_function_of_seed_and_sample_index(gpu):
    import gan_class_transfer2_amd as g
    imgs = list(D.sources())
    a = g.CachedImageDataset(imgs, size=32, batch_size=8, device=gpu, seed=D.CASE_SEED)
    b = g.CachedImageDataset(imgs, size=32, batch_size=8, device=gpu, seed=D.CASE_SEED)
    first, second = take(a, 4), take(b, 4)
    assert all(x.shape == (8, 32, 32, 3) and x.dtype == np.float32 for x in first)
    assert all(same_bits(x, y) for x, y in zip(first, second))
    assert not same_bits(first[0], take(g.CachedImageDataset(imgs, size=32, batch_size=8, device=gpu, seed=1), 1)[0])
    # the oracle on the host restatement of the picks
    for i, x in enumerate(first):
        picks = a.picks(8 * i, 8)
        assert np.array_equal(x.astype(np.float64), np.stack([S.decode_contract(imgs[j], oy, ox, bool(fl), 32) for j, oy, ox, fl in picks]))
    # batch_size 8 against 2 x 4
    halves = take(g.CachedImageDataset(imgs, size=32, batch_size=4, device=gpu, seed=D.CASE_SEED), 8)
    assert all(same_bits(first[i], np.concatenate(halves[2 * i:2 * i + 2])) for i in range(4))
    # the state after three batches resumes with the fourth
    c = g.CachedImageDataset(imgs, size=32, batch_size=8, device=gpu, seed=D.CASE_SEED)
    it = iter(c)
    for _ in range(3):
        next(it)
    state = c.state_dict()
    assert state == {"seed": D.CASE_SEED, "next_sample": 24}
    d = g.ImageDataset(imgs, size=32, batch_size=8, device=gpu, seed=7).cache()
    d.load_state_dict(state)
    assert same_bits(take(d, 1)[0], first[3]) and same_bits(next(it)[0].cpu().numpy(), first[3])
    # two shards of one stream
    shards = [take(g.CachedImageDataset(imgs, size=32, batch_size=4, device=gpu, seed=D.CASE_SEED, shard=(r, 2)), 2) for r in range(2)]
    for i in range(2):
        both = np.empty_like(first[i])
        both[0::2], both[1::2] = shards[0][i], shards[1][i]
        assert same_bits(both, first[i])


def test_cached_validation_pass_equals_the_uncached_one(gpu):
    import gan_class_transfer2_amd as g
    imgs = list(D.sources())
    plain = g.ImageDataset.validation(imgs, size=30, batch_size=3, device=gpu)
    cached = plain.cache()
    assert cached.finite and cached.flags == 0
    want = [x.cpu().numpy() for x, _ in plain]
    for _ in range(2):                                 # it ends, and a second pass gives the same batches
        got = [x.cpu().numpy() for x, _ in cached]
        assert [x.shape[0] for x in got] == [3, 3, 1] == [x.shape[0] for x in want]
        assert all(same_bits(x, y) for x, y in zip(got, want))


def test_fit_takes_a_cached_dataset(gpu):
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd import model as M
    g.configure(size=16, pixel_size=8, max_size=16, octaves=2, compute_dtype="float32")
    try:
        cached = g.CachedImageDataset(list(D.sources()), size=16, batch_size=4, device=gpu, seed=2)
        tr = g.Trainer(g.Denoiser())
        ex = cached.batch_at(0, 4)
        tr(ex)                                         # train.py:505-509 warm-up call
        tr.compile(g.Adam(g.WarmUp(2e-5, M.warm_up)), g.identity)
        hist = tr.fit(cached, steps_per_epoch=2, epochs=1, verbose=0)
        assert len(hist["loss"]) == 1 and np.isfinite(hist["loss"][0]) and cached.state_dict()["next_sample"] >= 8
    finally:
        g.configure(size=256, pixel_size=128, max_size=512, octaves=6, compute_dtype=None)


def test_a_recorded_call_replays_with_first_sample_moved(gpu, pool):
    L = lib()
    B, size = 5, 32
    out = torch.full((B, size, size, 3), NAN, dtype=torch.float32, device=gpu)
    picks = torch.zeros((B, 4), dtype=torch.int32, device=gpu)
    plan = L.Plan()
    plan.begin(execute=False)
    L.call("gct2_image_batch_cached", pool.pool_d.data_ptr(), pool.offsets_d.data_ptr(), pool.hw_d.data_ptr(), pool.N, D.CASE_SEED,
           L.Slot("first_sample", 0), 1, 7, None, picks.data_ptr(), out.data_ptr(), B, size, stream())
    plan.end()
    for first in (0, 5, (1 << 32) + 3):
        plan.set("first_sample", first)
        plan.run_segment(0)
        torch.cuda.synchronize()
        eager, want = run(pool, gpu, B, size, 7, first)
        assert np.array_equal(picks.cpu().numpy(), want) and same_bits(out.cpu().numpy(), eager), first
