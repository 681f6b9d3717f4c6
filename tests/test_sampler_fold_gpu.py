"""The identities between the sampler's entry points that csrc/sampler.hip relies on: every step is ONE per-element function
(step_element) behind two traversals, so a call with a feature switched off must give the bits of the call that never had it.  All
comparisons are bit for bit per element (+0 == -0, NaN == NaN), GPU against GPU, through tests/test_generate_kernels_gpu.py's
sentinel-guarded views; on the two shapes of tests/generate_cases.py that take the counter kernel's general form (3x1003x3) and its
four-element form (3x1024x3), fp32 and fp16 copies, the four step modes, clip 1.0.  (tests/test_multistep_kernels_gpu.py
test_c1_zero_is_the_existing_step and tests/test_img2img_kernels_gpu.py test_all_ones_is_diffusion_step_and_all_zeros_keeps_the_image
hold two of these on bf16, the first shape and three modes.)"""
import pytest
import torch

import generate_cases as G
import img2img_cases as I
import multistep_cases as MC
import test_generate_kernels_gpu as TG
import test_img2img_kernels_gpu as TI
import test_multistep_kernels_gpu as TM
from exact_cases import F16, F32
from objective_cases import SAMPLE_V
from test_generate_kernels_gpu import Outputs, dev, lib, stream
from test_multistep_kernels_gpu import MOutputs

pytestmark = pytest.mark.gpu

MODES, MODE_IDS = G.MODES + [SAMPLE_V], G.MODE_IDS + ["v"]
SHAPES, SHAPE_IDS = G.SHAPES[:2], G.SHAPE_IDS[:2]
CLIP, T = 1.0, 37
cases = lambda f: pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)(
    pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)(pytest.mark.parametrize("dt", [F32, F16], ids=["f32", "f16"])(f)))


def streams(per):
    """(offset, offset0, image_stride): multiples of 4 with the images back to back where per_image is one (the four-element form's
    condition), else the two draws at different lanes of their counters and every image at another lane than the one before"""
    return (8, 8 * per, per) if per % 4 == 0 else (8, 8 * per + 5, G.image_stride(per))


def device_inputs(gpu, shape, mask_kind):
    B, npix, C = shape
    p, f = G.step_case(B, npix * C)
    arrays = (p, f, MC.hist_case(B, npix * C), I.known_case(B, npix * C), I.mask_case(mask_kind, B, npix))
    return tuple(dev(a, gpu) for a in arrays)


def sigmas(a_t, a_prev):
    return (0.0, G.sigma2(a_t, a_prev, 0.7))


@cases
def test_multistep_without_history_is_the_step(gpu, dt, mode, shape):
    """c1 = 0, known = mask = NULL: fake', x0_out and both copies are gct2_diffusion_step's at sigma2 = 0, hist_out is its x0_out"""
    pred, fake, _, _, _ = device_inputs(gpu, shape, "ones")
    a_t, a_prev = G.alphas(T)
    plain = Outputs(shape, dt, gpu)
    TG.step(mode, dt, pred, fake.data_ptr(), a_t, a_prev, 0.0, CLIP, 0, 0, plain, shape)
    want, x = plain.fake.got(), plain.x0.got()
    o = MOutputs(shape, dt, gpu)
    TM.multistep(mode, dt, pred, fake.data_ptr(), None, None, None, a_t, a_prev, 0.0, CLIP, 0, 0, o, shape)
    o.check(dt, want, x, x, f"multistep at c1 = 0 against diffusion_step, mode {mode} shape {shape}")


@cases
def test_all_ones_mask_is_the_step(gpu, dt, mode, shape):
    """sigma2 = 0 (the flat kernel) and eta 0.7 (the counter kernel, whose own counter is the starting noise's when masked and the
    step noise's when not): the same step noise at the same offset, the same bits"""
    pred, fake, _, known, ones = device_inputs(gpu, shape, "ones")
    off, off0, stride = streams(shape[1] * shape[2])
    a_t, a_prev = G.alphas(T)
    for s2 in sigmas(a_t, a_prev):
        plain = Outputs(shape, dt, gpu)
        TG.step(mode, dt, pred, fake.data_ptr(), a_t, a_prev, s2, CLIP, off, stride, plain, shape)
        want, x = plain.fake.got(), plain.x0.got()
        o = Outputs(shape, dt, gpu)
        TI.masked(mode, dt, pred, fake.data_ptr(), known, ones, a_t, a_prev, s2, CLIP, off, off0, stride, o, shape)
        o.check(dt, want, x, f"all-ones mask against diffusion_step, mode {mode} sigma2 {s2} shape {shape}")


@cases
def test_all_zeros_mask_is_the_start_from_the_image(gpu, dt, mode, shape):
    """the kept region's value cx known + ck z0 is gct2_diffusion_start_image's at a = a_prev and the same offset0; x0_out = known"""
    pred, fake, _, known, zeros = device_inputs(gpu, shape, "zeros")
    off, off0, stride = streams(shape[1] * shape[2])
    a_t, a_prev = G.alphas(T)
    begun = Outputs(shape, dt, gpu, x0=False)
    TI.start_image(dt, known, a_prev, off0, stride, begun, shape)
    want = begun.fake.got()
    assert bool(torch.isfinite(want).all()) and not torch.equal(want, known.cpu().reshape(want.shape))
    for s2 in sigmas(a_t, a_prev):
        o = Outputs(shape, dt, gpu)
        TI.masked(mode, dt, pred, fake.data_ptr(), known, zeros, a_t, a_prev, s2, CLIP, off, off0, stride, o, shape)
        o.check(dt, want, known.cpu(), f"all-zeros mask against diffusion_start_image, mode {mode} sigma2 {s2} shape {shape}")


@cases
def test_all_ones_mask_is_the_plain_multistep(gpu, dt, mode, shape):
    """c1 = 1.37: the masked form's extrapolated fake', x0_out and hist_out are the plain form's"""
    pred, fake, hist, known, ones = device_inputs(gpu, shape, "ones")
    _, off0, stride = streams(shape[1] * shape[2])
    a_t, a_prev = G.alphas(T)
    plain = MOutputs(shape, dt, gpu)
    TM.multistep(mode, dt, pred, fake.data_ptr(), hist.data_ptr(), None, None, a_t, a_prev, 1.37, CLIP, 0, 0, plain, shape)
    want, x, hx = plain.fake.got(), plain.x0.got(), plain.hist.got()
    first = Outputs(shape, dt, gpu)
    TG.step(mode, dt, pred, fake.data_ptr(), a_t, a_prev, 0.0, CLIP, 0, 0, first, shape)
    assert not torch.equal(want, first.fake.got())                      # (the history was read: not the first-order step)
    o = MOutputs(shape, dt, gpu)
    TM.multistep(mode, dt, pred, fake.data_ptr(), hist.data_ptr(), known, ones, a_t, a_prev, 1.37, CLIP, off0, stride, o, shape)
    o.check(dt, want, x, hx, f"all-ones mask against the plain multistep, mode {mode} shape {shape}")


@cases
def test_update_estimates_are_the_step_s(gpu, dt, mode, shape):
    """no clip: gct2_diffusion_update's x is the step's x0_out; its e is the step's fake' at a_prev = 0, where the re-noising
    0 x + 1 e adds a zero to e (x is finite on these inputs)"""
    B, npix, C = shape
    n = B * npix * C
    pred, fake, _, _, _ = device_inputs(gpu, shape, "ones")
    a_t, _ = G.alphas(T)
    x, e = torch.empty(n, device=gpu), torch.empty(n, device=gpu)
    lib().call("gct2_diffusion_update", mode, pred.data_ptr(), fake.data_ptr(), a_t, 0.0, x.data_ptr(), e.data_ptr(), n, stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all())
    o = Outputs(shape, dt, gpu)
    TG.step(mode, dt, pred, fake.data_ptr(), a_t, 0.0, 0.0, 0.0, 0, 0, o, shape)
    o.check(dt, e.cpu(), x.cpu(), f"diffusion_update against diffusion_step at a_prev = 0, mode {mode} shape {shape}")
