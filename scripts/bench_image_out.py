"""time the image output path in one process on one MI355X and write profiles/image_out_bench.json (the protocol of
scripts/bench_image_cache.py: events around a captured graph of LAUNCHES calls replayed REPLAYS times, SAMPLES samples, the forms
taking turns, medians, needed bytes and GB/s):

 (a) the launch: 64 x 128 x 128 x 3 fp32 as to_uint8, as an 8 x 8 grid with pad = 2 and as a scale = 2 grid, each beside the torch
     composition that yields the same bytes (mul, add, mul, clamp, to(uint8); repeat_interleave; slice-assign into a pre-filled grid),
     beside the per-pixel path of the same call (an out one byte off its alignment) and beside the mirror launch,
     gct2_image_batch_cached at the same batch.  No figure is fixed; the ratios are recorded.
 (b) the copy: device-to-host of the uint8 batch against the fp32 batch it replaces, into pinned memory.
 (c) end to end: generate_to_dir of 512 images at 128 x 128 (dpm2m, 20 steps, batch 64, config 3, bf16) with 1, 4 and 16 writer
     threads at compress_level 1, beside generate alone and beside the naive loop (.cpu() of the fp32 batch, numpy conversion and
     Image.save on the caller's thread); images per second.

    python scripts/bench_image_out.py [OUT.json]
"""
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
B, SIZE = 64, 128
LAUNCHES, REPLAYS, SAMPLES = 100, 10, 15
TOTAL, STEPS_RUN, COMPRESS = 512, 20, 1
stream = lambda: torch.cuda.current_stream().cuda_stream
summary = lambda v: {"samples": [round(u, 3) for u in v], "median": round(statistics.median(v), 3), "min": round(min(v), 3),
                     "max": round(max(v), 3), "spread": round(max(v) - min(v), 3)}

x = (torch.randn(B, SIZE, SIZE, 3, generator=torch.Generator().manual_seed(0)) * 0.6).to(dev)
LAYOUTS = {"to_uint8": (1, B, 0, 1), "grid_8x8_pad2": (8, 8, 2, 1), "grid_8x8_pad2_scale2": (8, 8, 2, 2)}      # cols, rows, pad, scale
FILL = (0x12, 0xC8, 0x7F)
shape = lambda cols, rows, pad, scale: (rows * SIZE * scale + (rows + 1) * pad, cols * SIZE * scale + (cols + 1) * pad, 3)


def kernel_call(layout, shift):
    cols, rows, pad, scale = layout

    def run(buf):
        L.call("gct2_image_grid_u8", x.data_ptr(), L.F32, B, SIZE, SIZE, L.U8_SUMMARY, cols, rows, pad, scale,
               FILL[0] | FILL[1] << 8 | FILL[2] << 16, buf.data_ptr() + shift, stream())
    return run


def torch_call(layout):
    cols, rows, pad, scale = layout
    fill = torch.tensor(FILL, dtype=torch.uint8, device=dev)

    def run(buf):
        # tf.summary.image's conversion with torch ops; z < 1 -> 0 and the saturation are the clamp and the truncating cast
        q = ((x * 0.5 + 0.5) * 255.5).clamp(0.0, 255.0).to(torch.uint8)
        if scale > 1:
            q = q.repeat_interleave(scale, 1).repeat_interleave(scale, 2)
        out = buf[:int(np.prod(shape(*layout)))].view(shape(*layout))
        if layout == LAYOUTS["to_uint8"]:
            out.view(q.shape).copy_(q)
            return
        out[:] = fill
        h, w = SIZE * scale, SIZE * scale
        cells = out[pad:, pad:].unfold(0, h, h + pad).unfold(1, w, w + pad)          # [rows, cols, 3, h, w]
        cells.copy_(q.view(rows, cols, h, w, 3).permute(0, 1, 4, 2, 3))
    return run


forms, sizes = {}, {}
for name, layout in LAYOUTS.items():
    forms[name] = kernel_call(layout, 0)
    forms[name + "_per_pixel"] = kernel_call(layout, 1)
    forms[name + "_torch"] = torch_call(layout)
    sizes[name] = sizes[name + "_per_pixel"] = sizes[name + "_torch"] = int(np.prod(shape(*layout)))

# the mirror: gct2_image_batch_cached at the same batch (profiles/image_cache_bench.json)
rng = np.random.default_rng(0)
cached = g.CachedImageDataset([rng.integers(0, 256, (256, 256, 3), dtype=np.uint8) for _ in range(256)], size=SIZE, batch_size=B, device=dev, seed=7)
mirror_out = torch.empty(B, SIZE, SIZE, 3, device=dev)


def mirror(buf):
    L.call("gct2_image_batch_cached", cached.pool.data_ptr(), cached.offsets_d.data_ptr(), cached.hw_d.data_ptr(), len(cached), 7, 0, 1,
           cached.flags, None, None, mirror_out.data_ptr(), B, SIZE, stream())


forms["image_batch_cached"] = mirror
sizes["image_batch_cached"] = B * SIZE * SIZE * 3
bufs = {k: torch.zeros(sizes[k] + 8, dtype=torch.uint8, device=dev) for k in forms}
for k, f in forms.items():
    for _ in range(20):
        f(bufs[k])
torch.cuda.synchronize()
identical = {}
for name in LAYOUTS:
    n = sizes[name]
    identical[name] = bool(torch.equal(bufs[name][:n], bufs[name + "_per_pixel"][1:n + 1]) and torch.equal(bufs[name][:n], bufs[name + "_torch"][:n]))


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
launch = {}
for k, v in us.items():
    moved = x.numel() * 4 + sizes[k] if k != "image_batch_cached" else sizes[k] * 4 + sizes[k]      # fp32 read + bytes written (the mirror: the reverse)
    launch[k] = dict(summary(v), unit="us per call", bytes_per_call=moved, GB_per_s_at_median=round(moved / statistics.median(v) / 1e3, 1))
del graphs
med = lambda k: launch[k]["median"]
ratios = {name: {"kernel_over_torch": round(med(name) / med(name + "_torch"), 3), "wide_over_per_pixel": round(med(name) / med(name + "_per_pixel"), 3),
                 "kernel_over_mirror": round(med(name) / med("image_batch_cached"), 3)} for name in LAYOUTS}

# ---- (b) the copy ------------------------------------------------------------------------------------------------------------------------------
u8 = g.to_uint8(x)
pin8, pin32 = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True), torch.empty(x.shape, dtype=torch.float32, pin_memory=True)


def copy_us(dst, src, reps=50):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dst.copy_(src, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


copy_us(pin8, u8), copy_us(pin32, x)
c8, c32 = [], []
for _ in range(SAMPLES):
    c8.append(copy_us(pin8, u8))
    c32.append(copy_us(pin32, x))
copy = {"uint8": dict(summary(c8), unit="us per copy", bytes=u8.numel()), "fp32": dict(summary(c32), unit="us per copy", bytes=x.numel() * 4),
        "uint8_over_fp32": round(statistics.median(c8) / statistics.median(c32), 3)}

# ---- (c) end to end ---------------------------------------------------------------------------------------------------------------------------
g.configure(size=SIZE, pixel_size=128, max_size=512, octaves=6, compute_dtype="bfloat16")
den = g.Denoiser()
kw = dict(num_steps=STEPS_RUN, solver="dpm2m", seed=1, size=SIZE, batch_size=B, clip_denoised=True)
den.generate(B, **kw)                                       # warm-up: buffers, the captured forward pass
torch.cuda.synchronize()


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return round(TOTAL / (time.perf_counter() - t0), 1)


def naive(directory):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    for g0 in range(0, TOTAL, B):
        host = den.generate(B, first_index=g0, **kw).cpu().numpy()
        q = np.clip((host * 0.5 + 0.5) * 255.5, 0, 255).astype(np.uint8)
        for i in range(B):
            Image.fromarray(q[i]).save(os.path.join(directory, f"{g0 + i:06d}.png"), compress_level=COMPRESS)


end_to_end = {"generate_alone_images_per_s": timed(lambda: den.generate(TOTAL, **kw))}
with tempfile.TemporaryDirectory() as tmp:
    for threads in (1, 4, 16):
        with g.ImageWriter(tmp, threads=threads, max_pending=4, compress_level=COMPRESS) as w:
            end_to_end[f"generate_to_dir_{threads}_threads_images_per_s"] = timed(
                lambda: den.generate_to_dir(TOTAL, os.path.join(tmp, f"t{threads}"), writer=w, **kw))
    end_to_end["naive_loop_images_per_s"] = timed(lambda: naive(os.path.join(tmp, "naive")))
    end_to_end["files_written"] = len(os.listdir(os.path.join(tmp, "t4")))

out = {"what": f"one MI355X, one process. launch: gct2_image_grid_u8 on {B}x{SIZE}x{SIZE}x3 fp32, mode summary, as to_uint8 (cols 1, pad 0), as an 8x8 "
               "grid with pad 2 and as the same grid at scale 2; *_per_pixel: the same call with out one byte off its alignment (the per-pixel "
               "path); *_torch: the torch composition that yields the same bytes; image_batch_cached: the mirror launch at the same batch. "
               f"{SAMPLES} samples of {LAUNCHES * REPLAYS} graph-replayed calls each between two events, the forms taking turns, after 20 warm-up "
               "calls; bytes_per_call = fp32 read + bytes written. copy: non-blocking device-to-host copies into pinned memory, 50 per sample. "
               f"end_to_end: {TOTAL} images, config 3 bf16, dpm2m {STEPS_RUN} steps, batch {B}, PNG compress_level {COMPRESS}, max_pending 4, "
               "wall clock synchronised at both ends, files in a temporary directory; one run each",
       "launch": launch, "bit_identical_to_per_pixel_and_torch": identical, "ratios": ratios, "copy": copy, "end_to_end": end_to_end}
print(json.dumps(out))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "image_out_bench.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
