"""gct2_image_grid_u8 on the GPU, bit for bit against the restatement of tests/image_out_cases.py: every layout (wide and per-pixel
path, groups that straddle padding, empty cells, upscaling, one image, a full grid, several work-groups), every mode over the value
ladder in fp32, bf16 and fp16, a non-black fill, an out shifted by 1 and 2 bytes, and an output above 2^31 bytes.  out is pre-poisoned
with 0xA5 and sits between 0xA5 guard rows that must survive; the whole buffer is compared."""
import numpy as np
import pytest
import torch

import image_out_cases as IO

pytestmark = pytest.mark.gpu
GUARD = 64                                                  # guard bytes on either side of out


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def run(gpu, images, layout, mode, fill=(0, 0, 0), dtype=IO.F32, shift=0):
    """one launch into a poisoned, guarded out (`shift` bytes off its 4-byte alignment); returns u8 [GH,GW,3] on the host after proving
    that the guards survived"""
    n, H, W, cols, rows, pad, scale = layout
    GH, GW = IO.grid_dims(*layout)
    src = torch.from_numpy(np.ascontiguousarray(images, dtype=np.float32)).to(gpu).to(IO.TORCH_DTYPE[dtype]).contiguous()
    assert tuple(src.shape) == (n, H, W, 3)
    size = GH * GW * 3
    buf = torch.full((GUARD + size + GUARD + 4,), IO.POISON, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 4 == 0
    lo = GUARD + shift
    lib().call("gct2_image_grid_u8", src.data_ptr(), dtype, n, H, W, mode, cols, rows, pad, scale, fill[0] | fill[1] << 8 | fill[2] << 16,
               buf.data_ptr() + lo, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:lo] == IO.POISON).all() and (host[lo + size:] == IO.POISON).all(), "out: a guard byte changed"
    return host[lo:lo + size].reshape(GH, GW, 3)


def want(images, layout, mode, fill=(0, 0, 0)):
    _, _, _, cols, rows, pad, scale = layout
    return IO.grid_ref(images, mode, cols, rows, pad, scale, fill)


@pytest.mark.parametrize("name", list(IO.LAYOUTS))
def test_every_layout_is_bit_exact_on_its_path(gpu, name):
    layout = IO.LAYOUTS[name]
    imgs = IO.images_for(layout, seed=len(name))
    for mode in IO.MODES.values():
        got = run(gpu, imgs, layout, mode, IO.FILL)
        assert np.array_equal(got, want(imgs, layout, mode, IO.FILL)), (name, mode)
    # (a poisoned cell would show: the fill differs from 0xA5 in every byte)
    assert IO.POISON not in IO.FILL


@pytest.mark.parametrize("name", ["wide_straddling_one_empty_cell", "to_uint8", "scale2_wide", "several_work_groups_wide"])
def test_a_shifted_out_takes_the_per_pixel_path_with_the_same_bits(gpu, name):
    layout = IO.LAYOUTS[name]
    assert IO.is_wide(layout)
    imgs = IO.images_for(layout, seed=3)
    aligned = run(gpu, imgs, layout, IO.SUMMARY, IO.FILL)
    assert np.array_equal(aligned, want(imgs, layout, IO.SUMMARY, IO.FILL))
    for shift in (1, 2):
        assert np.array_equal(run(gpu, imgs, layout, IO.SUMMARY, IO.FILL, shift=shift), aligned), shift


@pytest.mark.parametrize("dtype", [IO.F32, IO.BF16, IO.F16])
@pytest.mark.parametrize("mode", list(IO.MODES.values()))
def test_the_value_ladder_in_every_mode_and_dtype(gpu, mode, dtype):
    """every step of the quantisation, the specials and the loader's values, on the wide path (cols = 4, pad = 0: GW = 68) and on
    the per-pixel path (cols = 3, pad = 1: GW = 55); 16-bit sources hold the ladder rounded to the dtype"""
    values = IO.ladder(mode) if dtype == IO.F32 else IO.ladder_as(mode, dtype)
    imgs = IO.deal(values, IO.LADDER_SHAPE)
    n, H, W, _ = IO.LADDER_SHAPE
    for layout in ((n, H, W, 4, 2, 0, 1), (n, H, W, 3, 2, 1, 1)):
        got = run(gpu, imgs, layout, mode, IO.FILL, dtype=dtype)
        assert np.array_equal(got, want(imgs, layout, mode, IO.FILL)), layout
    assert IO.is_wide((n, H, W, 4, 2, 0, 1)) and not IO.is_wide((n, H, W, 3, 2, 1, 1))


def test_sixteen_bit_sources_at_an_odd_element(gpu):
    """a bf16 source that starts on the second half of a dword: the six-dword loads of the wide path move to the other rows"""
    layout = IO.LAYOUTS["several_work_groups_wide"]
    n, H, W, cols, rows, pad, scale = layout
    imgs = IO.images_for(layout, seed=9)
    flat = torch.zeros(imgs.size + 1, dtype=torch.bfloat16, device=gpu)
    flat[1:] = torch.from_numpy(imgs.reshape(-1)).to(gpu).to(torch.bfloat16)
    src = flat[1:]
    assert src.data_ptr() % 4 == 2
    GH, GW = IO.grid_dims(*layout)
    out = torch.full((GH, GW, 3), IO.POISON, dtype=torch.uint8, device=gpu)
    lib().call("gct2_image_grid_u8", src.data_ptr(), IO.BF16, n, H, W, IO.SUMMARY, cols, rows, pad, scale, 0, out.data_ptr(),
               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rounded = src.to(torch.float32).cpu().numpy().reshape(n, H, W, 3)
    assert np.array_equal(out.cpu().numpy(), want(rounded, layout, IO.SUMMARY))


def test_an_output_above_two_to_the_31_bytes(gpu):
    """n = 2, H = W = 2048, cols = 1, scale = 12: 3.6e9 bytes, the whole second cell beyond byte 2^31.  Checked on the device: the view
    [rows H, s, W, s, 3] equals the scale = 1 result broadcast, and the scale = 1 result equals the restatement per element"""
    n, H, W, cols, rows, pad, scale = IO.LARGE
    GH, GW = IO.grid_dims(*IO.LARGE)
    assert GH * GW * 3 > 1 << 31
    rng = np.random.default_rng(5)
    imgs = (rng.standard_normal((n, H, W, 3)) * 0.7).astype(np.float32)
    src = torch.from_numpy(imgs).to(gpu)
    small = torch.full((n * H, W, 3), IO.POISON, dtype=torch.uint8, device=gpu)
    big = torch.full((GH, GW, 3), IO.POISON, dtype=torch.uint8, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    lib().call("gct2_image_grid_u8", src.data_ptr(), IO.F32, n, H, W, IO.SUMMARY, 1, n, 0, 1, 0, small.data_ptr(), s)
    lib().call("gct2_image_grid_u8", src.data_ptr(), IO.F32, n, H, W, IO.SUMMARY, cols, rows, pad, scale, 0, big.data_ptr(), s)
    torch.cuda.synchronize()
    assert np.array_equal(small.cpu().numpy().reshape(n, H, W, 3), IO.quantize_ref(imgs, IO.SUMMARY))
    view = big.view(n * H, scale, W, scale, 3)
    equal = bool((view == small.view(n * H, 1, W, 1, 3)).all())
    del view, big, small, src
    torch.cuda.empty_cache()                                # (7 GB go back to the device, not into the allocator's cache)
    assert equal
