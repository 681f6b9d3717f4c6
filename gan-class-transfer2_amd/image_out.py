"""Samples as pictures: the output side of the pipeline (files -> HBM -> train -> sample -> files).

`to_uint8` / `image_grid` turn a batch on the device into uint8 - a whole grid with padding, empty cells and integer upscaling - in ONE
launch (gct2_image_grid_u8, include/gct2.h); `save_images` writes that grid as one PNG.  `ImageWriter` takes uint8 tensors off the
device without stopping the caller: one non-blocking copy into a pinned buffer of a small ring, an event, and a bounded thread pool
that waits for the event and runs the PNG encoder.  `SummarySink` is the `sink` of sampler.make_log_sample (the reference's seven
summaries per epoch, train.py:356-361, 488-496, as PNG files and one CSV), `generate_to_dir` writes n samples to a folder that
ImageDataset / CachedImageDataset read back.  Nothing here touches training state, and nothing else in the package calls it."""
from __future__ import annotations

import math
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import BF16, F16, F32, U8_DATASET, U8_SUMMARY, U8_UNIT, Gct2Error, call

MODES = {"summary": U8_SUMMARY, "dataset": U8_DATASET, "unit": U8_UNIT}
_DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
MAX_THREADS = 16
# the tags of the reference's image summaries (train.py:356, 489-496) and the one this project's log_sample adds
SUMMARY_TAGS = ("denoised", "step_1", "step_0.25", "step_0.5", "step_0.75", "fake", "epsilon_theta")


def _layout(n: int, cols: Optional[int]) -> Tuple[int, int]:
    """(cols, rows) of a grid of n cells: cols defaults to ceil(sqrt(n))"""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"image_grid: n must be a positive int, got {n!r}")
    if cols is None:
        cols = math.isqrt(n - 1) + 1
    if isinstance(cols, bool) or not isinstance(cols, int) or cols < 1:
        raise ValueError(f"image_grid: cols must be a positive int, got {cols!r}")
    return cols, -(-n // cols)


def grid_shape(n: int, H: int, W: int, cols: Optional[int] = None, padding: int = 2, scale: int = 1) -> Tuple[int, int]:
    """(GH, GW) of the grid image_grid lays n images of H x W out on: GH = rows H scale + (rows + 1) padding,
    GW = cols W scale + (cols + 1) padding, rows = ceil(n / cols), cols = ceil(sqrt(n)) by default (include/gct2.h)"""
    cols, rows = _layout(n, cols)
    return rows * H * scale + (rows + 1) * padding, cols * W * scale + (cols + 1) * padding


def _fill_rgb(fill) -> int:
    try:
        r, g, b = (int(v) for v in fill)
    except (TypeError, ValueError):
        raise ValueError(f"image_grid: fill must be three bytes (R, G, B), got {fill!r}") from None
    if any(v < 0 or v > 255 for v in (r, g, b)):
        raise ValueError(f"image_grid: fill must be three bytes (R, G, B), got {fill!r}")
    return r | g << 8 | b << 16


def _check_images(images) -> Tuple[int, int, int]:
    """(n, H, W) of a batch the kernel takes: a float [n,H,W,3] tensor on the device"""
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[3] != 3 or images.shape[0] < 1:
        raise ValueError(f"image_grid: images must be [n,H,W,3], got {tuple(getattr(images, 'shape', ()))}")
    if images.dtype not in _DTYPES:
        raise ValueError(f"image_grid: images must be float32, bfloat16 or float16, got {images.dtype}")
    if images.device.type != "cuda":
        raise Gct2Error("image_grid: the conversion is a HIP kernel, these images live on " + str(images.device))
    return int(images.shape[0]), int(images.shape[1]), int(images.shape[2])


def _grid(images: torch.Tensor, cols: int, rows: int, padding: int, scale: int, fill, mode: str, shape) -> torch.Tensor:
    if mode not in MODES:
        raise ValueError(f"image_grid: mode must be one of {sorted(MODES)!r}, got {mode!r}")
    n, H, W = _check_images(images)
    images = images.contiguous()
    out = torch.empty(shape, dtype=torch.uint8, device=images.device)
    call("gct2_image_grid_u8", images.data_ptr(), _DTYPES[images.dtype], n, H, W, MODES[mode], cols, rows, int(padding), int(scale),
         _fill_rgb(fill), out.data_ptr(), torch.cuda.current_stream(images.device).cuda_stream)
    return out


def to_uint8(images: torch.Tensor, mode: str = "summary") -> torch.Tensor:
    """images [n,H,W,3] (fp32, bf16 or fp16, on the device) -> uint8 [n,H,W,3] on the device, one launch on the current stream.
    mode: "summary" the reference's tf.summary.image(x * 0.5 + 0.5) for x in [-1, 1]; "dataset" the exact inverse of the loader's
    value / 128 - 1; "unit" for x already in [0, 1] (include/gct2.h GCT2_U8_*).  It is the grid of one column without padding: the
    same memory."""
    n, H, W = _check_images(images)
    return _grid(images, 1, n, 0, 1, (0, 0, 0), mode, (n, H, W, 3))


def image_grid(images: torch.Tensor, cols: Optional[int] = None, padding: int = 2, scale: int = 1, fill=(0, 0, 0),
               mode: str = "summary") -> torch.Tensor:
    """images [n,H,W,3] on the device -> ONE uint8 [GH,GW,3] picture on the device (grid_shape), one launch: image i in cell
    (i / cols, i % cols), `padding` pixels of `fill` (R, G, B bytes) around and between the cells and in the cells past n, every
    source pixel repeated scale x scale times (nearest neighbour: 32 x 32 samples can be looked at)."""
    n, H, W = _check_images(images)
    cols, rows = _layout(n, cols)
    return _grid(images, cols, rows, padding, scale, fill, mode, grid_shape(n, H, W, cols, int(padding), int(scale)) + (3,))


def _encode_png(array: np.ndarray, path: str, compress_level: int) -> None:
    """PIL's PNG encoder into a temporary name beside `path`, then a rename: a reader never sees half a file"""
    from PIL import Image
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = f"{path}.{os.getpid()}.{threading.get_ident()}.tmp"
    try:
        Image.fromarray(array).save(tmp, format="PNG", compress_level=compress_level)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


def save_images(images: torch.Tensor, path: str, compress_level: int = 1, **grid_kw) -> str:
    """image_grid(images, **grid_kw) as one PNG at `path`, written before the call returns"""
    grid = image_grid(images, **grid_kw)
    _encode_png(grid.cpu().numpy(), str(path), compress_level)
    return str(path)


class _Slot:
    """one pinned host buffer of the ring and the copy that is in flight into it"""
    __slots__ = ("pinned", "event", "keep", "left", "lock")

    def __init__(self):
        self.pinned, self.event, self.keep, self.left, self.lock = None, None, None, 0, threading.Lock()


class ImageWriter:
    """asynchronous PNG writer.  write(path, image) launches nothing: a device uint8 tensor [H,W,3] (write_many: [k,H,W,3], one file
    per image, ONE copy) goes into one of `max_pending` pinned host buffers with a non-blocking copy on the current stream and an
    event; a pool of `threads` workers (1..16, never sized by the machine's CPU count) waits for the event, encodes with PIL at
    `compress_level` into a temporary name and renames.  The caller blocks only while `max_pending` copies are in flight: host memory
    stays bounded and a slow disk slows the producer down.  Host uint8 arrays take the same route without the copy.  flush() / close()
    join and re-raise the first encoder or filesystem error - a failed write is never silent.  Relative paths are taken inside
    `directory`.  Use as a context manager, or call close()."""

    def __init__(self, directory: str = ".", threads: int = 4, max_pending: int = 4, compress_level: int = 1):
        if isinstance(threads, bool) or not isinstance(threads, int) or not 1 <= threads <= MAX_THREADS:
            raise ValueError(f"ImageWriter: threads must lie in 1..{MAX_THREADS}, got {threads!r}")
        if isinstance(max_pending, bool) or not isinstance(max_pending, int) or max_pending < 1:
            raise ValueError(f"ImageWriter: max_pending must be a positive int, got {max_pending!r}")
        self.directory, self.threads, self.max_pending, self.compress_level = str(directory), threads, max_pending, int(compress_level)
        self._pool = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="gct2-image-writer")
        self._free: "queue.Queue[_Slot]" = queue.Queue()
        for _ in range(max_pending):
            self._free.put(_Slot())
        self._futures: List = []
        self._closed = False

    @property
    def pending(self) -> int:
        """how many copies are in flight (their files not all written yet): 0..max_pending"""
        return self.max_pending - self._free.qsize()

    def path_of(self, path: str) -> str:
        return path if os.path.isabs(path) else os.path.join(self.directory, path)

    def write(self, path: str, image, block: bool = True) -> str:
        """queue one uint8 [H,W,3] image for `path`; returns the full path at once.  block=False raises queue.Full instead of waiting
        when max_pending copies are in flight"""
        if getattr(image, "ndim", 0) != 3:
            raise ValueError(f"ImageWriter.write: one [H,W,3] image per call (write_many takes a batch), got {tuple(getattr(image, 'shape', ()))}")
        return self.write_many([path], image[None], block)[0]

    def write_many(self, paths: Sequence[str], images, block: bool = True) -> List[str]:
        """queue uint8 [k,H,W,3] as k files with ONE device-to-host copy; returns the full paths at once"""
        if self._closed:
            raise RuntimeError("ImageWriter: closed")
        shape = tuple(getattr(images, "shape", ()))
        if len(shape) != 4 or shape[3] != 3 or shape[0] != len(paths) or shape[0] < 1 or \
                (images.dtype != torch.uint8 if isinstance(images, torch.Tensor) else images.dtype != np.uint8):
            raise ValueError(f"ImageWriter: {len(paths)} paths need uint8 [{len(paths)},H,W,3], got {getattr(images, 'dtype', None)} {shape}")
        full = [self.path_of(str(p)) for p in paths]
        try:
            slot = self._free.get(block=block)             # back-pressure: waits while every buffer is in flight
        except queue.Empty:
            raise queue.Full(f"ImageWriter: {self.max_pending} copies are in flight") from None
        try:
            if isinstance(images, torch.Tensor) and images.device.type == "cuda":
                images = images.contiguous()
                count = images.numel()
                if slot.pinned is None or slot.pinned.numel() < count:
                    slot.pinned = torch.empty(count, dtype=torch.uint8, pin_memory=True)
                slot.pinned[:count].copy_(images.view(-1), non_blocking=True)
                slot.event = torch.cuda.Event()
                slot.event.record(torch.cuda.current_stream(images.device))
                slot.keep = images                         # (alive until the copy has been waited for)
                host = slot.pinned[:count].view(shape).numpy()
            else:                                          # host data: a private copy, the caller may reuse its array
                slot.event, slot.keep = None, None
                host = np.array(images.numpy() if isinstance(images, torch.Tensor) else images, dtype=np.uint8, order="C")
            slot.left = len(full)
            for k, p in enumerate(full):
                self._futures.append(self._pool.submit(self._job, slot, host, k, p))
        except BaseException:
            slot.event = slot.keep = None
            self._free.put(slot)
            raise
        return full

    def _job(self, slot: _Slot, host: np.ndarray, k: int, path: str) -> None:
        try:
            if slot.event is not None:
                slot.event.synchronize()
            self._encode(host[k], path)
        finally:
            with slot.lock:
                slot.left -= 1
                last = slot.left == 0
            if last:                                       # every file of this copy is out: the buffer may take the next one
                slot.event = slot.keep = None
                self._free.put(slot)

    def _encode(self, array: np.ndarray, path: str) -> None:
        _encode_png(array, path, self.compress_level)

    def flush(self) -> None:
        """wait for everything queued so far; re-raise the first error"""
        futures, self._futures = self._futures, []
        first = None
        for f in futures:
            try:
                f.result()
            except BaseException as e:                     # noqa: BLE001 - re-raised below
                first = first or e
        if first is not None:
            raise first

    def close(self) -> None:
        """flush() and stop the workers; further writes are refused"""
        if self._closed:
            return
        self._closed = True
        try:
            self.flush()
        finally:
            self._pool.shutdown(wait=True)

    def __enter__(self) -> "ImageWriter":
        return self

    def __exit__(self, exc_type, exc, tb) -> None:
        if exc_type is None:
            self.close()
        else:                                              # an error is already on its way: stop the workers, do not mask it
            self._closed = True
            self._pool.shutdown(wait=True)


class SummarySink:
    """`sink` of sampler.make_log_sample: what the reference hands to tf.summary (train.py:356-361, 488-496) as files.  For every 4-D
    tensor of log_sample's result one PNG `<directory>/<tag>/<epochs:06d>.png` - a one-row grid without padding of the first
    `max_outputs` images (the 10 of train.py:489-496) in mode "summary", every pixel scale x scale - and one row `epochs,example_loss`
    appended to `<directory>/scalars.csv`.  With its own writer it returns once the files are written; a `writer` handed in is
    flushed by its owner.

        LambdaCallback(on_epoch_begin=make_log_sample(denoiser, example_image, example, dictionary, sink=SummarySink("logs/run")))"""

    def __init__(self, directory: str, max_outputs: int = 10, scale: int = 1, writer: Optional[ImageWriter] = None):
        if isinstance(max_outputs, bool) or not isinstance(max_outputs, int) or max_outputs < 1:
            raise ValueError(f"SummarySink: max_outputs must be a positive int, got {max_outputs!r}")
        self.directory, self.max_outputs, self.scale = str(directory), max_outputs, int(scale)
        self._own = writer is None
        self.writer = ImageWriter(self.directory) if writer is None else writer

    def __call__(self, epochs: int, images: Dict[str, torch.Tensor]) -> None:
        for tag, value in images.items():
            if isinstance(value, torch.Tensor) and value.dim() == 4:
                shown = value[:self.max_outputs]
                grid = image_grid(shown, cols=int(shown.shape[0]), padding=0, scale=self.scale, mode="summary")
                self.writer.write(os.path.abspath(os.path.join(self.directory, tag, f"{int(epochs):06d}.png")), grid)
        if "example_loss" in images:
            os.makedirs(self.directory, exist_ok=True)
            path = os.path.join(self.directory, "scalars.csv")
            new = not os.path.exists(path)
            with open(path, "a") as fh:
                if new:
                    fh.write("epochs,example_loss\n")
                fh.write(f"{int(epochs)},{float(images['example_loss']):.9g}\n")
        if self._own:
            self.writer.flush()

    def close(self) -> None:
        if self._own:
            self.writer.close()
        else:
            self.writer.flush()


def generate_to_dir(denoiser, n: int, directory: str, pattern: str = "{:06d}.png", mode: str = "summary",
                    writer: Optional[ImageWriter] = None, **generate_kw) -> List[str]:
    """n samples of sampler.generate as n PNG files `directory/pattern.format(g)`, g = first_index + position: generate runs batch by
    batch (batch_size from the keywords, default min(n, 64)); every batch is one to_uint8 launch and one copy, and while the writer
    encodes it the next batch is generated.  By generate's contract file g holds the same pixels whatever the batch size.  noise=
    and init= are cut along with the batches (mask= too where it is per image); return_steps is refused.  Returns the paths, after
    flush(): every file is on disk."""
    from .sampler import generate
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"generate_to_dir: n must be a positive int, got {n!r}")
    if mode not in MODES:
        raise ValueError(f"generate_to_dir: mode must be one of {sorted(MODES)!r}, got {mode!r}")
    if generate_kw.get("return_steps"):
        raise ValueError("generate_to_dir: return_steps has no file to go to; call generate")
    if generate_kw.get("return_thresholds"):
        raise ValueError("generate_to_dir: return_thresholds has no file to go to; call generate")
    generate_kw.pop("return_steps", None)
    generate_kw.pop("return_thresholds", None)
    bs = generate_kw.pop("batch_size", None)
    bs = min(n, 64) if bs is None else bs
    if isinstance(bs, bool) or not isinstance(bs, int) or bs < 1:
        raise ValueError(f"generate_to_dir: batch_size must be a positive int, got {bs!r}")
    first_index = int(generate_kw.pop("first_index", 0))
    per_image = {k: generate_kw.pop(k) for k in ("noise", "init", "mask") if generate_kw.get(k) is not None}
    own = writer is None
    w = ImageWriter(directory) if own else writer
    paths: List[str] = []
    try:
        for g0 in range(0, n, bs):
            B = min(bs, n - g0)
            cut = {k: (v[g0:g0 + B] if k != "mask" or (isinstance(v, torch.Tensor) and v.dim() >= 3) else v) for k, v in per_image.items()}
            images = generate(denoiser, B, first_index=first_index + g0, batch_size=B, **cut, **generate_kw)
            names = [os.path.abspath(os.path.join(str(directory), pattern.format(first_index + g0 + i))) for i in range(B)]
            paths += w.write_many(names, to_uint8(images, mode))
        w.flush()
    finally:
        if own:
            w.close()
    return paths
