"""time the device-resident image cache beside the loader it stands in for, in one process on one MI355X, and write
profiles/image_cache_bench.json:

 (a) the launch: gct2_image_batch_cached at 64 x 128 x 128 x 3 from 256 x 256 sources in its three forms - picks given (picks_in),
     drawn inside the kernel, and the per-element path (forced by a dst that is not 16-byte aligned) - beside gct2_image_prepare of the
     default loader on the same picks and the same pool.  Events around many launches per sample (a captured HIP graph of LAUNCHES
     launches, replayed REPLAYS times, so the host's enqueue rate stays out of the number), the forms taking turns; median and spread
     over the samples, and the bytes per second each form achieves (12.6 MB written, 3.1 MB of crops read).
 (b) the loader: batches per second of iterating ImageDataset and of iterating its .cache(), batch 64 of 128 x 128 crops, over the
     same SOURCES in-memory 256 x 256 arrays and over the same images as PNG files written by PIL into a temporary directory; the
     one-off build time of the cache is reported beside them.
 Acceptance (the JSON says whether it holds): the launch with picks_in is not slower than gct2_image_prepare beyond the run-to-run
 spread measured here; the drawing form gets that spread plus the cost of the draw, which is reported, not bounded.  The loader ratio
 is reported and is no threshold.

    python scripts/bench_image_cache.py [OUT.json]
"""
import glob
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import gan_class_transfer2_amd as g

L = g._lib
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
B, SIZE, SRC, SOURCES, SEED = 64, 128, 256, 256, 7
LAUNCHES, REPLAYS, SAMPLES = 100, 10, 15
PLAIN_BATCHES, FILE_BATCHES, CACHED_BATCHES = 30, 12, 2000
stream = lambda: torch.cuda.current_stream().cuda_stream
summary = lambda v: {"samples": [round(u, 3) for u in v], "median": round(statistics.median(v), 3), "min": round(min(v), 3),
                     "max": round(max(v), 3), "spread": round(max(v) - min(v), 3)}

rng = np.random.default_rng(0)
images = [rng.integers(0, 256, (SRC, SRC, 3), dtype=np.uint8) for _ in range(SOURCES)]

# ---- (a) the launch ----------------------------------------------------------------------------------------------------------------------
cached = g.CachedImageDataset(images, size=SIZE, batch_size=B, device=dev, seed=SEED)
picks = cached.picks(0, B)
picks_d = torch.from_numpy(picks).to(dev)
prep_off = torch.from_numpy(cached.offsets[picks[:, 0]]).to(dev)
prep_dims = torch.from_numpy(np.concatenate([cached.hw[picks[:, 0]], picks[:, 1:]], 1).astype(np.int32)).to(dev)
n = B * SIZE * SIZE * 3


def cached_call(picks_in, shift):
    def run(buf):
        L.call("gct2_image_batch_cached", cached.pool.data_ptr(), cached.offsets_d.data_ptr(), cached.hw_d.data_ptr(), len(cached), SEED, 0, 1,
               cached.flags, picks_d.data_ptr() if picks_in else None, None, buf.data_ptr() + 4 * shift, B, SIZE, stream())
    return run


def prepare_call(buf):
    L.call("gct2_image_prepare", cached.pool.data_ptr(), prep_off.data_ptr(), prep_dims.data_ptr(), buf.data_ptr(), B, SIZE, stream())


forms = {"cached_picks_in": cached_call(True, 0), "cached_drawn": cached_call(False, 0), "cached_per_element": cached_call(False, 1),
         "image_prepare": prepare_call}
shifts = {"cached_per_element": 1}
bufs = {k: torch.zeros(n + 4, dtype=torch.float32, device=dev) for k in forms}
for k, f in forms.items():
    for _ in range(20):
        f(bufs[k])
torch.cuda.synchronize()
view = lambda k: bufs[k][shifts.get(k, 0):shifts.get(k, 0) + n].view(torch.int32)
identical = all(bool(torch.equal(view(k), view("image_prepare"))) for k in forms)
assert identical, "the forms disagree"


def graph_of(f, b):
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(LAUNCHES):
            f(b)
    return gr


def sample(gr):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (LAUNCHES * REPLAYS)


graphs = {k: graph_of(f, bufs[k]) for k, f in forms.items()}
for gr in graphs.values():
    gr.replay()
torch.cuda.synchronize()
us = {k: [] for k in forms}
for _ in range(SAMPLES):
    for k in us:
        us[k].append(sample(graphs[k]))
moved = n * 4 + n                                       # fp32 written + the crops' bytes read
launch = {k: dict(summary(v), unit="us per call", bytes_per_call=moved, GB_per_s_at_median=round(moved / statistics.median(v) / 1e3, 1))
          for k, v in us.items()}
del graphs, bufs
med = lambda k: launch[k]["median"]
spread = max(launch["cached_picks_in"]["spread"], launch["image_prepare"]["spread"])
draw_cost = round(med("cached_drawn") - med("cached_picks_in"), 3)


# ---- (b) the loader ------------------------------------------------------------------------------------------------------------------------
def batches_per_second(ds, count):
    it = iter(ds)
    next(it)                                            # (the default loader starts its thread and its stream here)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        x, _ = next(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if hasattr(it, "close"):
        it.close()
    return round(count / dt, 2)


def build_seconds(ds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = ds.cache()
    torch.cuda.synchronize()
    return c, round(time.perf_counter() - t0, 3)


loader = {}
plain = g.ImageDataset(images, size=SIZE, batch_size=B, device=dev, seed=SEED)
c, built = build_seconds(plain)
loader["arrays"] = {"default_batches_per_s": batches_per_second(plain, PLAIN_BATCHES), "cached_batches_per_s": batches_per_second(c, CACHED_BATCHES),
                    "cache_build_s": built}
del c
with tempfile.TemporaryDirectory() as tmp:
    from PIL import Image
    for i, im in enumerate(images):
        Image.fromarray(im).save(os.path.join(tmp, f"{i:04d}.png"))
    files = g.ImageDataset(os.path.join(tmp, "*.png"), size=SIZE, batch_size=B, device=dev, seed=SEED)
    assert len(files.items) == SOURCES == len(glob.glob(os.path.join(tmp, "*.png")))
    c, built = build_seconds(files)
    loader["png_files"] = {"default_batches_per_s": batches_per_second(files, FILE_BATCHES), "cached_batches_per_s": batches_per_second(c, CACHED_BATCHES),
                           "cache_build_s": built}
    del c
for v in loader.values():
    v["cached_over_default"] = round(v["cached_batches_per_s"] / v["default_batches_per_s"], 1)
    v["cached_images_per_s"] = round(v["cached_batches_per_s"] * B)
    v["default_images_per_s"] = round(v["default_batches_per_s"] * B)

out = {"what": f"one MI355X, one process. launch: B={B} {SIZE}x{SIZE}x3 fp32 crops from {SOURCES} sources of {SRC}x{SRC}x3 bytes in one pool, "
               "flags shuffle | random crop | flip; cached_picks_in / cached_drawn: gct2_image_batch_cached on its four-pixel path with the picks "
               "given / drawn in the kernel; cached_per_element: the same call with a dst 4 bytes off 16-byte alignment, which takes the "
               "per-element path; image_prepare: gct2_image_prepare on the same picks and pool. "
               f"{SAMPLES} samples of {LAUNCHES * REPLAYS} back-to-back calls each (a captured graph of {LAUNCHES}, replayed {REPLAYS} times) "
               "between two events, the forms taking turns, after 20 warm-up calls of each; bytes_per_call = fp32 written + crop bytes read. "
               f"loader: wall-clock batches per second of iterating ImageDataset ({PLAIN_BATCHES} batches over arrays, {FILE_BATCHES} over PNG "
               f"files) and its .cache() ({CACHED_BATCHES} batches), synchronised at both ends, after one batch of warm-up; cache_build_s: decode "
               "(16 threads) + upload, once",
       "launch": launch,
       "all_forms_bit_identical": identical,
       "run_to_run_spread_us": spread,
       "picks_in_minus_image_prepare_median_us": round(med("cached_picks_in") - med("image_prepare"), 3),
       "picks_in_not_slower_than_image_prepare": bool(med("cached_picks_in") <= med("image_prepare") + spread),
       "draw_costs_median_us": draw_cost,
       "four_pixel_path_over_per_element_path": round(med("cached_drawn") / med("cached_per_element"), 3),
       "loader": loader}
print(json.dumps(out))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "image_cache_bench.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
