"""CPU tier of the image output path: the restatement of tests/image_out_cases.py agrees with exact rational arithmetic, DATASET is
the loader's inverse, the value ladder brackets every step; gct2_image_grid_u8 is declared, exported, bound, plannable and rejects bad
arguments before any launch (in a child process that sees no device: tests/test_capi_contract_cpu.py's idiom); ImageWriter on host
arrays writes what it was given, reports a failed write at flush() and keeps at most max_pending copies in flight."""
import ctypes
import importlib.util
import json
import os
import queue
import re
import subprocess
import sys
import threading
from fractions import Fraction

import numpy as np
import pytest

import image_out_cases as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = 1, 3
P = 4096                    # a fake, 16-byte aligned device address; no row lets a call get as far as reading it


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def exact_z(x, mode):
    x = Fraction(float(x))
    if mode == IO.SUMMARY:
        return Fraction(511, 2) * (x / 2 + Fraction(1, 2))
    if mode == IO.DATASET:
        return 128 * x + Fraction(257, 2)
    return Fraction(511, 2) * x


@pytest.mark.parametrize("mode", list(IO.MODES.values()))
def test_restatement_agrees_with_exact_rational_arithmetic(mode):
    """wherever the exact z is at least 2^-10 from an integer the float32 restatement gives floor(z) clamped to 0..255 (z < 1 -> 0)"""
    values = np.concatenate([IO.ladder(mode), IO.ladder_as(mode, IO.BF16), IO.ladder_as(mode, IO.F16)])
    values = values[np.isfinite(values)]
    got = IO.quantize_ref(values, mode)
    checked = 0
    for x, q in zip(values.tolist(), got.tolist()):
        z = exact_z(x, mode)
        if abs(z - round(z)) < Fraction(1, 1024):
            continue
        want = 0 if z < 1 else 255 if z >= 255 else int(z)           # int() truncates; z >= 1 here
        assert q == want, (mode, x, float(z), q, want)
        checked += 1
    assert checked > 1500                              # (the points AT a step are skipped, their neighbours mostly not)
    special = IO.quantize_ref(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], dtype=np.float32), mode)
    assert special.tolist() == [0, 255, 0, 255, 0]


@pytest.mark.parametrize("mode", list(IO.MODES.values()))
def test_ladder_brackets_every_step(mode):
    at = IO.steps(mode)
    assert at.shape == (255,) and (np.diff(at) > 0).all()
    below, above = np.nextafter(at, np.float32(-np.inf)), np.nextafter(at, np.float32(np.inf))
    q = np.arange(1, 256)
    assert np.array_equal(IO.quantize_ref(at, mode), q) and np.array_equal(IO.quantize_ref(below, mode), q - 1)
    assert np.array_equal(IO.quantize_ref(above, mode), q)
    lad = IO.ladder(mode)
    assert lad.dtype == np.float32 and lad.size % 2 and lad.size % 3 and 3 * lad.size <= np.prod(IO.LADDER_SHAPE)
    assert set(IO.quantize_ref(lad, mode).tolist()) == set(range(256))
    assert np.isnan(lad).any() and np.isinf(lad).any() and (lad == np.float32(1e-45)).any()
    dealt = IO.deal(lad, IO.LADDER_SHAPE)
    assert all(np.isin(lad[np.isfinite(lad)], dealt[..., c]).all() for c in range(3))      # every value meets every channel
    # coverage of the 16-bit ladders (no property of the code under test): fp16 has 11 significant bits, so nearly every byte is
    # still reached; bf16 has 8, so near x = 1 its values are a whole byte apart and about every other byte is reached
    assert len(set(IO.quantize_ref(IO.ladder_as(mode, IO.F16), mode).tolist())) >= 240
    assert len(set(IO.quantize_ref(IO.ladder_as(mode, IO.BF16), mode).tolist())) >= 128


def test_dataset_mode_round_trips_all_256_bytes_and_summary_does_not():
    x = IO.dataset_values()
    v = np.arange(256)
    assert np.array_equal(x.astype(np.float64), v / 128 - 1)
    assert np.array_equal(IO.quantize_ref(x, IO.DATASET), v)
    assert np.array_equal(IO.quantize_ref(x, IO.SUMMARY), (511 * v) // 512)
    assert IO.quantize_ref(x, IO.SUMMARY)[255] == 254
    assert np.array_equal(IO.quantize_ref((v / 255).astype(np.float32), IO.UNIT)[[0, 255]], [0, 255])


def test_grid_restatement_places_cells_padding_and_fill():
    n, H, W, cols, rows, pad, scale = layout = IO.LAYOUTS["scale3_general"]
    imgs = IO.images_for(layout)
    out = IO.grid_ref(imgs, IO.SUMMARY, cols, rows, pad, scale, IO.FILL)
    assert out.shape == IO.grid_dims(*layout) + (3,) == (3 * 18 + 4 * 2, 2 * 24 + 3 * 2, 3)
    q = IO.quantize_ref(imgs, IO.SUMMARY)
    for i in range(n):
        r, c = divmod(i, cols)
        for (y, x) in ((0, 0), (5, 7), (2, 3)):
            cell = out[pad + r * (H * scale + pad) + y * scale:, pad + c * (W * scale + pad) + x * scale:][:scale, :scale]
            assert (cell == q[i, y, x]).all()
    assert (out[:pad] == IO.FILL).all() and (out[:, :pad] == IO.FILL).all() and (out[-pad:] == IO.FILL).all()
    assert (out[pad + 2 * (H * scale + pad):, pad + (W * scale + pad):] == IO.FILL).all()          # cell 5 is empty
    # the conversion layout is the same memory as [n,H,W,3]
    n, H, W, cols, rows, pad, scale = IO.LAYOUTS["to_uint8"]
    imgs = IO.images_for(IO.LAYOUTS["to_uint8"])
    assert np.array_equal(IO.grid_ref(imgs, IO.DATASET, cols, rows, pad, scale).reshape(n, H, W, 3), IO.quantize_ref(imgs, IO.DATASET))
    # which path a layout takes
    paths = {k: IO.is_wide(v) for k, v in IO.LAYOUTS.items()}
    assert paths == {"wide_straddling_one_empty_cell": True, "to_uint8": True, "per_pixel": False, "scale2_wide": True,
                     "scale3_general": False, "one_image": True, "full_grid": True, "narrow_cells": False, "narrow_cells_wide": True,
                     "several_work_groups_wide": True, "several_work_groups_per_pixel": False}
    GH, GW = IO.grid_dims(*IO.LARGE)
    assert GH * GW * 3 > 1 << 31 and (GH // 2) * GW * 3 < 1 << 31 and GW % 4 == 0


def test_grid_shape_restates_the_formulas():
    import gan_class_transfer2_amd as g
    assert g.grid_shape(5, 6, 8, cols=3) == (2 * 6 + 3 * 2, 3 * 8 + 4 * 2)
    assert g.grid_shape(5, 6, 8) == g.grid_shape(5, 6, 8, cols=3)      # ceil(sqrt(5)) = 3
    assert g.grid_shape(4, 6, 8, padding=0) == (12, 16) and g.grid_shape(1, 6, 8, padding=1, scale=3) == (20, 26)
    assert g.grid_shape(9, 2, 2, padding=0) == (6, 6) and g.grid_shape(10, 2, 2, padding=0) == (6, 8)
    for layout in IO.LAYOUTS.values():
        n, H, W, cols, rows, pad, scale = layout
        assert g.grid_shape(n, H, W, cols, pad, scale) == IO.grid_dims(*layout)
    for bad in (dict(n=0), dict(cols=0), dict(n=True)):
        with pytest.raises(ValueError):
            g.grid_shape(**{**dict(n=4, H=2, W=2), **bad})


def test_the_conversion_needs_a_device():
    import torch
    import gan_class_transfer2_amd as g
    with pytest.raises(g.Gct2Error, match="HIP kernel"):
        g.to_uint8(torch.zeros(2, 4, 4, 3))
    with pytest.raises(ValueError, match=r"\[n,H,W,3\]"):
        g.image_grid(torch.zeros(2, 4, 4))
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        g.to_uint8(torch.zeros(2, 4, 4, 3, dtype=torch.float64))


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------
def test_image_grid_u8_is_declared_exported_bound_and_plannable():
    import gan_class_transfer2_amd as g
    L = g._lib
    lib = L.load()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "gct2_image_grid_u8")
    header = open(os.path.join(ROOT, "include", "gct2.h")).read()
    proto = re.search(r"\bint gct2_image_grid_u8\(([^;]*)\);", header)
    params = [p.strip() for p in proto.group(1).replace("\n", " ").split(",")]
    sig = L.SIGNATURES["gct2_image_grid_u8"]
    assert len(params) == len(sig) == 13 <= 28 and params[-1] == "void* stream" and sig[-1] is ctypes.c_void_p
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert sig == [vp, i, i, i, i, i, i, i, i, i, ctypes.c_uint32, vp, vp]
    for name, code in (("GCT2_U8_SUMMARY", 0), ("GCT2_U8_DATASET", 1), ("GCT2_U8_UNIT", 2)):
        assert re.search(rf"#define {name}\s+{code}\b", header)
    assert (L.U8_SUMMARY, L.U8_DATASET, L.U8_UNIT) == (IO.SUMMARY, IO.DATASET, IO.UNIT) == (0, 1, 2)
    assert g.image_out.MODES == IO.MODES
    assert lib.gct2_abi_version() == L.ABI_VERSION == 17              # an addition changes no signature
    assert "gct2_image_grid_u8" in L.PLANNABLE
    plan = L.Plan()
    idx = ctypes.c_int(-1)
    arr = (ctypes.c_uint64 * 13)()
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_image_grid_u8", arr, 13, ctypes.byref(idx)) == 0 and idx.value == 0
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_image_grid_u8", arr, 12, None) == EINVAL
    assert b"takes 13 arguments" in lib.gct2_last_error()
    failed = ctypes.c_int(-1)
    assert lib.gct2_plan_run(plan.handle, 0, 1, ctypes.byref(failed)) == EINVAL and failed.value == 0
    assert b"image_grid_u8: null pointer" in lib.gct2_last_error()


def _args(**o):
    a = dict(src=P, dtype=0, n=5, H=6, W=8, mode=0, cols=3, rows=2, pad=2, scale=1, fill_rgb=0x7FC812, out=P + 4096, stream=None)
    assert not set(o) - set(a)
    a.update(o)
    return list(a.values())


# every row is a call that its argument checks reject BEFORE anything is launched: (arguments, text)
CASES = [
    (_args(src=None), "null pointer"),
    (_args(out=None), "null pointer"),
    (_args(dtype=3), "unknown dtype 3"),
    (_args(dtype=-1), "unknown dtype -1"),
    (_args(mode=3), "unknown mode 3"),
    (_args(mode=-1), "unknown mode -1"),
    (_args(n=0), "must be positive"),
    (_args(n=-5), "must be positive"),
    (_args(H=0), "must be positive"),
    (_args(W=-8), "must be positive"),
    (_args(cols=0), "must be positive"),
    (_args(rows=0), "must be positive"),
    (_args(rows=-2), "must be positive"),
    (_args(cols=2, rows=2), "do not hold n=5"),
    (_args(cols=1 << 16, rows=-(1 << 16)), "must be positive"),
    (_args(scale=0), "scale=0 is outside 1..16"),
    (_args(scale=17), "scale=17 is outside 1..16"),
    (_args(pad=-1), "pad=-1 is outside 0..64"),
    (_args(pad=65), "pad=65 is outside 0..64"),
    (_args(H=16385), "larger than 16384"),
    (_args(W=16385), "larger than 16384"),
    (_args(fill_rgb=0x01000000), "bits above its 24"),
    (_args(fill_rgb=0xFF000000), "bits above its 24"),
    (_args(n=1, H=16384, W=16384, cols=1 << 15, rows=1, scale=16), "a side above 2^31 - 1"),
    (_args(n=1, H=16384, W=16384, cols=4096, rows=4096, scale=16, pad=0), "more than 2^31 - 1 work-groups"),
    (_args(n=1, H=16384, W=16384, cols=4096, rows=4096, scale=16, pad=1), "more than 2^31 - 1 work-groups"),      # (the per-pixel path)
    # two mistakes: the earlier check speaks
    (_args(src=None, dtype=7), "null pointer"),
    (_args(dtype=7, mode=9), "unknown dtype 7"),
    (_args(scale=0, pad=99), "scale=0 is outside 1..16"),
]


def _child():
    """runs CASES against the library and prints one JSON line: {"device": code of gct2_device_check, "results": [[code, text], ...]}"""
    spec = importlib.util.spec_from_file_location("gct2_lib", os.path.join(ROOT, "gan-class-transfer2_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    lib = L.load()
    out = {"device": lib.gct2_device_check(), "results": []}
    if out["device"] == ENODEV:
        for args, _text in CASES:
            code = lib.gct2_image_grid_u8(*args)
            out["results"].append([code, lib.gct2_last_error().decode()])
    print(json.dumps(out))


def test_image_grid_u8_rejects_bad_arguments_without_a_device():
    env = dict(os.environ)
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if out["device"] != ENODEV:
        pytest.skip(f"a device is visible to the child process (gct2_device_check() = {out['device']}): fake pointers are not sent to it")
    assert len(out["results"]) == len(CASES) >= 25
    wrong = [(i, got, text) for i, ((_a, text), got) in enumerate(zip(CASES, out["results"]))
             if got[0] != EINVAL or not got[1].startswith("image_grid_u8: ") or text not in got[1]]
    assert not wrong, wrong


# ---- ImageWriter on host arrays ---------------------------------------------------------------------------------------------------------------
def _pictures(k, H=9, W=7, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (k, H, W, 3), dtype=np.uint8)


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


def test_writer_files_decode_to_what_was_written(tmp_path):
    import torch
    import gan_class_transfer2_amd as g
    pics = _pictures(6)
    with g.ImageWriter(str(tmp_path), threads=3, max_pending=2) as w:
        paths = [w.write(f"a/{i}.png", pics[i]) for i in range(3)]
        given = pics[3].copy()
        paths.append(w.write(str(tmp_path / "abs.png"), given))
        given[:] = 0                                       # the caller may reuse its array at once
        paths += w.write_many(["b/4.png", "b/5.png"], torch.from_numpy(pics[4:6]))
        assert paths[0] == os.path.join(str(tmp_path), "a", "0.png") and paths[3] == str(tmp_path / "abs.png")
        w.flush()
        assert w.pending == 0
        for i, p in enumerate(paths):
            assert np.array_equal(_decode(p), pics[i]), p
    assert sorted(os.listdir(tmp_path / "a")) == ["0.png", "1.png", "2.png"]                # no temporary name is left behind
    with pytest.raises(RuntimeError, match="closed"):
        w.write("late.png", pics[0])
    for bad in (dict(threads=0), dict(threads=17), dict(threads=True), dict(max_pending=0)):
        with pytest.raises(ValueError):
            g.ImageWriter(str(tmp_path), **bad)
    with g.ImageWriter(str(tmp_path)) as w:
        assert (w.threads, w.max_pending, w.compress_level) == (4, 4, 1)
        for bad in (pics, pics[0, :, :, :2], pics[0].astype(np.float32)):
            with pytest.raises(ValueError):
                w.write("x.png", bad)
        with pytest.raises(ValueError):
            w.write_many(["only-one.png"], pics[:2])


def test_a_failed_write_is_raised_at_flush(tmp_path):
    import gan_class_transfer2_amd as g
    (tmp_path / "file").write_bytes(b"not a directory")
    pics = _pictures(3)
    w = g.ImageWriter(str(tmp_path), threads=2, max_pending=2)
    w.write("ok.png", pics[0])
    w.write("file/inside/x.png", pics[1])                 # the parent is a regular file: no user can write there
    w.write("ok2.png", pics[2])
    with pytest.raises(OSError):
        w.flush()
    w.flush()                                              # reported once
    assert np.array_equal(_decode(tmp_path / "ok.png"), pics[0]) and np.array_equal(_decode(tmp_path / "ok2.png"), pics[2])
    w.write("file/inside/y.png", pics[1])
    with pytest.raises(OSError):
        w.close()
    assert w.pending == 0


def test_max_pending_bounds_what_is_in_flight(tmp_path):
    """with the encoder held at a gate, max_pending writes return at once and the next one finds no free buffer"""
    import gan_class_transfer2_amd as g
    pics = _pictures(8)
    gate, seen = threading.Event(), []

    class Held(g.ImageWriter):
        def _encode(self, array, path):
            gate.wait()
            seen.append(self.pending)
            super()._encode(array, path)

    w = Held(str(tmp_path), threads=2, max_pending=3)
    try:
        for i in range(3):
            w.write(f"{i}.png", pics[i])
        assert w.pending == 3
        with pytest.raises(queue.Full):
            w.write("3.png", pics[3], block=False)
        assert w.pending == 3 and not os.listdir(tmp_path)
    finally:
        gate.set()                                         # (whatever happened: no worker stays behind the gate)
    for i in range(3, 8):                                  # these block until a buffer comes back
        w.write(f"{i}.png", pics[i])
    w.close()
    assert len(seen) == 8 and max(seen) <= 3 and w.pending == 0
    assert all(np.array_equal(_decode(tmp_path / f"{i}.png"), pics[i]) for i in range(8))


if __name__ == "__main__":
    _child()
