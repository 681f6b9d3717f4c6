"""Input pipeline of the reference (train.py:285-297, 313-321): list_files -> shuffle(1000) -> repeat -> decode_file
(decode, random crop to size x size, random left-right flip, value/128 - 1, returned as the pair (image, image)) -> batch ->
prefetch.

Decoding is host work (PIL, like tf.image.decode_jpeg it accepts JPEG and PNG and always yields 3 channels); everything
after it runs on the GPU in one launch per batch (gct2_image_prepare): the decoded bytes of a batch are uploaded once, the crop
origins and flip flags are drawn on the host from a seeded numpy generator.  A background thread keeps `prefetch` batches
ready (tf.data.AUTOTUNE in the reference).

Opt-in, the reference's commented-out `.cache("cache")` (train.py:317) kept in HBM: ImageDataset.cache() / CachedImageDataset decode every
item ONCE into a device pool; a batch is then one launch (gct2_image_batch_cached) that picks, crops, flips and casts with draws from the
project's Philox streams - a function of (seed, running sample index), restated on the host by sample_picks."""
from __future__ import annotations

import glob
import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import DATA_FLIP, DATA_POOL_PAD, DATA_RANDOM_CROP, DATA_SHUFFLE, Gct2Error, call
from .trainer_math import DATA_STREAM_AUG, DATA_STREAM_ORDER


def shuffle_repeat(items: Sequence, buffer_size: int, rng: np.random.Generator) -> Iterator:
    """tf.data's .shuffle(buffer_size).repeat(): a buffer of `buffer_size` elements is kept filled from the (endlessly repeated,
    per-epoch reshuffled like list_files) source and a uniformly random slot is emitted and refilled."""
    if not len(items):
        raise ValueError("empty dataset")

    def source():
        while True:
            order = rng.permutation(len(items))          # list_files shuffles the file order every epoch
            for i in order:
                yield items[i]

    src = source()
    buf = [next(src) for _ in range(min(buffer_size, len(items)))]
    while True:
        j = int(rng.integers(len(buf)))
        out, buf[j] = buf[j], next(src)
        yield out


def decode_rgb(path: str) -> np.ndarray:
    """tf.image.decode_jpeg(file, 3) (train.py:287): uint8 [H, W, 3]."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


class ImageDataset:
    """iterable of (image, image) batches, fp32 [B, size, size, 3] in [-1, 1) on the HIP device (train.py:292-293, 316-320).

    source: a glob pattern (train.py:5, 313) or a list of decoded uint8 HWC arrays (synthetic / in-memory data)."""

    def __init__(self, source, size: int, batch_size: int, device: Optional[torch.device] = None, seed: int = 0,
                 shuffle_buffer: int = 1000, prefetch: int = 2, crop: bool = True, decoder: Callable[[str], np.ndarray] = decode_rgb):
        self.items = sorted(glob.glob(source)) if isinstance(source, str) else list(source)
        if not self.items:
            raise ValueError(f"no files match {source!r}")
        self.size, self.batch_size, self.crop, self.decoder = size, batch_size, crop, decoder
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.seed, self.rng = seed, np.random.default_rng(seed)
        self.shuffle_buffer, self.prefetch = shuffle_buffer, prefetch
        self.finite = False             # training mode: an endless shuffled stream (ImageDataset.validation builds the finite form)

    @classmethod
    def validation(cls, source, size: int, batch_size: int, device: Optional[torch.device] = None,
                   decoder: Callable[[str], np.ndarray] = decode_rgb, prefetch: int = 2) -> "ImageDataset":
        """the held-out folder (the reference's test/ beside train/) for Trainer.evaluate and fit(validation_data=...): ONE pass over
        the items in sorted order (a list keeps its order), the centre size x size crop with origin ((H0 - size) // 2, (W0 - size) // 2),
        no flip, the last partial batch kept - nothing is drawn, so iterating it again gives the same batches.  The device side is the
        training one (gct2_image_prepare)."""
        ds = cls(source, size, batch_size, device=device, shuffle_buffer=1, prefetch=prefetch, crop=True, decoder=decoder)
        ds.finite = True
        return ds

    def cache(self, workers: int = 16, shard: Optional[Tuple[int, int]] = None) -> "CachedImageDataset":
        """the reference's commented-out `.cache("cache")` (train.py:317), in HBM: every item is decoded ONCE and kept on the device; see
        CachedImageDataset.  The same items, size, batch_size, device, seed, crop and decoder; a validation dataset stays one: its
        cached batches are bit-identical to the uncached ones."""
        return CachedImageDataset(self.items, self.size, self.batch_size, device=self.device, seed=self.seed, crop=self.crop,
                                  validation=self.finite, shard=shard, workers=workers, decoder=self.decoder)

    # ---- host side: pick, decode, draw the augmentation --------------------------------------------------------------------
    def _decoded(self, it) -> np.ndarray:
        im = self.decoder(it) if isinstance(it, str) else np.ascontiguousarray(it, dtype=np.uint8)
        if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < self.size or im.shape[1] < self.size:
            raise ValueError(f"image of shape {im.shape} cannot be cropped to {self.size}x{self.size}x3 (tf.image.random_crop "
                             "raises here, train.py:289)")
        return im

    def _validation_batches(self) -> Iterator[Tuple[List[np.ndarray], np.ndarray]]:
        for first in range(0, len(self.items), self.batch_size):
            imgs = [self._decoded(it) for it in self.items[first:first + self.batch_size]]
            dims = np.zeros((len(imgs), 5), dtype=np.int32)
            for b, im in enumerate(imgs):
                H0, W0 = im.shape[:2]
                dims[b] = (H0, W0, (H0 - self.size) // 2, (W0 - self.size) // 2, 0)
            yield imgs, dims

    def host_batches(self) -> Iterator[Tuple[List[np.ndarray], np.ndarray]]:
        if self.finite:
            yield from self._validation_batches()
            return
        stream = shuffle_repeat(self.items, self.shuffle_buffer, self.rng)
        while True:
            imgs, dims = [], np.zeros((self.batch_size, 5), dtype=np.int32)
            for b in range(self.batch_size):
                it = next(stream)
                im = self.decoder(it) if isinstance(it, str) else np.ascontiguousarray(it, dtype=np.uint8)
                H0, W0 = im.shape[:2]
                if im.ndim != 3 or im.shape[2] != 3 or H0 < self.size or W0 < self.size:
                    raise ValueError(f"image of shape {im.shape} cannot be cropped to {self.size}x{self.size}x3 (tf.image.random_crop "
                                     "raises here, train.py:289)")
                if not self.crop and (H0, W0) != (self.size, self.size):
                    raise ValueError("crop=False needs size x size images (tf.broadcast_to, train.py:290)")
                oy = int(self.rng.integers(H0 - self.size + 1)) if self.crop else 0
                ox = int(self.rng.integers(W0 - self.size + 1)) if self.crop else 0
                dims[b] = (H0, W0, oy, ox, int(self.rng.integers(2)))       # random_flip_left_right: p = 1/2
                imgs.append(im)
            yield imgs, dims

    # ---- device side ------------------------------------------------------------------------------------------------------
    def to_device(self, imgs: List[np.ndarray], dims: np.ndarray, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
        sizes = np.array([im.size for im in imgs], dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        packed = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs]))
        st = stream or torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            src = packed.to(self.device, non_blocking=True)
            off_d = torch.from_numpy(offsets).to(self.device, non_blocking=True)
            dims_d = torch.from_numpy(np.ascontiguousarray(dims)).to(self.device, non_blocking=True)
            out = torch.empty(len(imgs), self.size, self.size, 3, dtype=torch.float32, device=self.device)
            call("gct2_image_prepare", src.data_ptr(), off_d.data_ptr(), dims_d.data_ptr(), out.data_ptr(), len(imgs), self.size,
                 st.cuda_stream)
            for t in (src, off_d, dims_d):
                t.record_stream(st)
        return out

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        q: "queue.Queue" = queue.Queue(maxsize=max(1, self.prefetch))
        stop = threading.Event()
        # the loader's own stream, picked like the engine's (engine.distinct_stream: one that shares a hardware queue neither with the
        # consumer's stream nor with the streams a train step of this consumer already runs on)
        from .engine import distinct_stream
        dev = self.device if self.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        side = distinct_stream(dev, "data", torch.cuda.current_stream(dev))

        def worker():
            try:
                for imgs, dims in self.host_batches():
                    if stop.is_set():
                        return
                    x = self.to_device(imgs, dims, side)
                    ev = torch.cuda.Event()
                    ev.record(side)
                    q.put((x, ev))
                q.put(None)                     # a finite (validation) pass is over
            except BaseException as e:          # surface decoder / shape errors in the consumer
                q.put(e)

        th = threading.Thread(target=worker, daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if isinstance(item, BaseException):
                    raise item
                if item is None:
                    return
                x, ev = item
                torch.cuda.current_stream(self.device).wait_event(ev)
                x.record_stream(torch.cuda.current_stream(self.device))
                yield x, x                      # labels = the image itself (train.py:293)
        finally:
            stop.set()


# ---- the device-resident cache: host restatement of gct2_image_batch_cached's draw (include/gct2.h) -----------------------------------
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _philox(seed: int, stream_id: int, idx: int) -> List[int]:
    """the four words of counter idx on stream stream_id, as gct2_rng_uniform_int defines them (Philox4x32-10; Python ints)"""
    c = [idx & _M32, (idx >> 32) & _M32, stream_id & _M32, (stream_id >> 32) & _M32]
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & _M32, (p0 >> 32) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c


def _fmix32(x: int) -> int:
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    return x ^ (x >> 16)


def epoch_permutation(seed: int, epoch: int, p: int, N: int, _keys: Optional[List[int]] = None) -> int:
    """pi_epoch(p): the stateless permutation of [0, N) that orders an epoch of the cache - an eight-round Feistel network over
    2h bits, h = max(1, (bitlen(N - 1) + 1) // 2), keyed by philox(seed, DATA_STREAM_ORDER, epoch), cycle-walked until the value is < N"""
    if N == 1:
        return 0
    h = max(1, ((N - 1).bit_length() + 1) // 2)
    mask = (1 << h) - 1
    ks = _keys if _keys is not None else _philox(seed, DATA_STREAM_ORDER, epoch)
    v = p
    while True:
        L, R = v >> h, v & mask
        for j in range(8):
            kj = (ks[j & 3] + j * 0x9E3779B9) & _M32
            L, R = R, L ^ (_fmix32(R ^ kj) & mask)
        v = (L << h) | R
        if v < N:
            return v


def sample_picks(seed: int, first_sample: int, B: int, hw, size: int, flags: int, sample_stride: int = 1) -> np.ndarray:
    """int32 [B, 4] = (item, oy, ox, flip) of the samples k = first_sample + b * sample_stride of a cache whose image i has the size
    hw[i] = (H0, W0): what gct2_image_batch_cached draws in its kernel, restated with Python integers from include/gct2.h.  Tells which
    file was in which batch; tests/test_data_cache_gpu.py compares the kernel's picks_out with it."""
    hw = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
    N = len(hw)
    if N <= 0 or B <= 0 or size <= 0 or sample_stride <= 0 or flags & ~(DATA_SHUFFLE | DATA_RANDOM_CROP | DATA_FLIP):
        raise ValueError(f"sample_picks: N={N} B={B} size={size} sample_stride={sample_stride} flags={flags}")
    out = np.zeros((B, 4), dtype=np.int32)
    keys = {}
    for b in range(B):
        k = (int(first_sample) + b * int(sample_stride)) & _M64
        e, p = divmod(k, N)
        if flags & DATA_SHUFFLE:
            if e not in keys:
                keys[e] = _philox(seed, DATA_STREAM_ORDER, e)
            item = epoch_permutation(seed, e, p, N, keys[e])
        else:
            item = p
        H0, W0 = int(hw[item, 0]), int(hw[item, 1])
        if H0 < size or W0 < size:
            raise ValueError(f"sample_picks: image {item} of size {H0}x{W0} cannot be cropped to {size}x{size}")
        r = _philox(seed, DATA_STREAM_AUG, k) if flags & (DATA_RANDOM_CROP | DATA_FLIP) else [0, 0, 0, 0]
        if flags & DATA_RANDOM_CROP:
            oy, ox = (r[0] * (H0 - size + 1)) >> 32, (r[1] * (W0 - size + 1)) >> 32
        else:
            oy, ox = (H0 - size) // 2, (W0 - size) // 2
        out[b] = (item, oy, ox, r[2] >> 31 if flags & DATA_FLIP else 0)
    return out


class CachedImageDataset:
    """ImageDataset with every item decoded ONCE into a pool in HBM (the reference's commented-out `.cache("cache")`, train.py:317):
    iterable of (image, image) batches, fp32 [B, size, size, 3] in [-1, 1) on the HIP device.

    source: a glob pattern or a list of paths / decoded uint8 HWC arrays.  Building decodes on a pool of at most 16 threads (PIL
    releases the GIL), checks every shape against `size` (and crop=False) and uploads the bytes, an int64 offset table and an int32
    (H0, W0) table.  Iterating uses no thread and no queue: each batch is ONE C call on the current stream (gct2_image_batch_cached)
    into a fresh tensor; which image, the crop origin and the flip are drawn in the kernel from the Philox streams DATA_STREAM_ORDER /
    DATA_STREAM_AUG, so sample k of the stream is a function of (seed, k): the batches do not depend on batch_size, state_dict() is
    {"seed", "next_sample"}, and sample_picks() restates every draw on the host.

    The order is NOT the default loader's: every epoch is a full permutation of the items (a new one per epoch), not the sliding
    window of shuffle(1000).  crop=False (size x size sources) draws no crop; validation=True is ImageDataset.validation's pass - one
    pass in the given (sorted) order, centre crop, no flip, the partial last batch kept - with the uncached pass's bits.
    shard=(rank, world_size): this rank's batch b holds the samples next_sample + rank + world_size * b, and next_sample advances by
    batch_size * world_size: the union over the ranks is the unsharded stream."""

    def __init__(self, source, size: int, batch_size: int, device: Optional[torch.device] = None, seed: int = 0, crop: bool = True,
                 validation: bool = False, shard: Optional[Tuple[int, int]] = None, workers: int = 16,
                 decoder: Callable[[str], np.ndarray] = decode_rgb):
        items = sorted(glob.glob(source)) if isinstance(source, str) else list(source)
        if not items:
            raise ValueError(f"no files match {source!r}")
        if size <= 0 or batch_size <= 0:
            raise ValueError(f"size={size} and batch_size={batch_size} must be positive")
        rank, world = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))
        if not 0 <= rank < world:
            raise ValueError(f"shard={shard!r}: rank must lie in [0, world_size)")
        if validation and world != 1:
            raise ValueError("a validation pass is not sharded")
        self.size, self.batch_size, self.crop, self.finite, self.shard = size, batch_size, crop, bool(validation), (rank, world)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.seed, self.next_sample = int(seed) & _M64, 0
        self.flags = 0 if validation else DATA_SHUFFLE | DATA_FLIP | (DATA_RANDOM_CROP if crop else 0)

        def decoded(it) -> np.ndarray:
            im = decoder(it) if isinstance(it, str) else np.ascontiguousarray(it, dtype=np.uint8)
            if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < size or im.shape[1] < size:
                raise ValueError(f"image of shape {im.shape} cannot be cropped to {size}x{size}x3 (tf.image.random_crop "
                                 "raises here, train.py:289)")
            if not validation and not crop and im.shape[:2] != (size, size):
                raise ValueError("crop=False needs size x size images (tf.broadcast_to, train.py:290)")
            return im

        with ThreadPoolExecutor(max_workers=max(1, min(16, int(workers)))) as pool:
            imgs = list(pool.map(decoded, items))
        self.hw = np.array([im.shape[:2] for im in imgs], dtype=np.int32).reshape(-1, 2)
        sizes = np.array([im.size for im in imgs], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        total = int(sizes.sum())
        # the pool: the images back to back + the spare bytes gct2_image_batch_cached's aligned loads may touch behind the last one
        self.pool = torch.empty(total + DATA_POOL_PAD, dtype=torch.uint8, device=self.device)
        self.pool[total:].zero_()
        first = 0
        while first < len(imgs):                       # uploaded in pieces of about 256 MiB: the host never holds a second copy of the set
            last, nbytes = first, 0
            while last < len(imgs) and (last == first or nbytes + imgs[last].size <= (256 << 20)):
                nbytes += imgs[last].size
                last += 1
            piece = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs[first:last]]))
            at = int(self.offsets[first])
            self.pool[at:at + nbytes].copy_(piece)
            first = last
        self.offsets_d = torch.from_numpy(self.offsets).to(self.device)
        self.hw_d = torch.from_numpy(self.hw).to(self.device)

    def __len__(self) -> int:
        return len(self.hw)

    # ---- one batch = one launch -----------------------------------------------------------------------------------------------
    def batch_at(self, first_sample: int, B: int, sample_stride: int = 1, picks_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the samples first_sample + b * sample_stride, b < B: a fresh fp32 [B, size, size, 3] tensor, filled by one launch on the
        current stream; picks_out (int32 [B, 4] on the device) receives the picks the kernel used"""
        if self.device.type != "cuda":
            raise Gct2Error("CachedImageDataset: batches are made by a HIP kernel, this dataset was built on " + str(self.device))
        out = torch.empty(B, self.size, self.size, 3, dtype=torch.float32, device=self.device)
        call("gct2_image_batch_cached", self.pool.data_ptr(), self.offsets_d.data_ptr(), self.hw_d.data_ptr(), len(self.hw), self.seed,
             int(first_sample) & _M64, int(sample_stride), self.flags, None, picks_out.data_ptr() if picks_out is not None else None,
             out.data_ptr(), B, self.size, torch.cuda.current_stream(self.device).cuda_stream)
        return out

    def picks(self, first_sample: int, B: int, sample_stride: int = 1) -> np.ndarray:
        """sample_picks of this cache: (item, oy, ox, flip) of the samples first_sample + b * sample_stride"""
        return sample_picks(self.seed, first_sample, B, self.hw, self.size, self.flags, sample_stride)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        if self.finite:                                 # nothing is drawn and nothing advances: iterating again gives the same batches
            for first in range(0, len(self.hw), self.batch_size):
                x = self.batch_at(first, min(self.batch_size, len(self.hw) - first))
                yield x, x
            return
        rank, world = self.shard
        while True:
            first = self.next_sample
            self.next_sample = (first + self.batch_size * world) & _M64       # before the yield: state_dict() names the NEXT batch
            x = self.batch_at(first + rank, self.batch_size, world)
            yield x, x                                  # labels = the image itself (train.py:293)

    # ---- resuming: the whole loader state is one integer ---------------------------------------------------------------------
    def state_dict(self) -> dict:
        return {"seed": self.seed, "next_sample": self.next_sample}

    def load_state_dict(self, state: dict) -> None:
        self.seed, self.next_sample = int(state["seed"]) & _M64, int(state["next_sample"]) & _M64
