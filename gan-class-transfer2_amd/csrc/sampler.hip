// The sampler's pointwise steps (train.py:323-496 log_sample; Denoiser.generate / encode): gct2_diffusion_mix, gct2_diffusion_update and
// the five one-launch steps gct2_diffusion_step / _start / _start_image / _step_masked / _step_multistep, which are ONE per-element
// computation (step_element) behind two traversals (sampler_flat_kernel, sampler_counter_kernel).  fp32 state, HBM-bound.
#include "gct2_common.h"
#include <algorithm>

namespace {

// ---- log_sample (train.py:323-496): the sampler's pointwise steps, fp32 state ------------------------------------------------
// fake = sqrt(a) x_theta + sqrt(1-a) eps_theta (train.py:372-375, 441-444); also stored in the compute dtype where the network
// reads its input (packed image and/or the image slice of R_0)
template <typename T>
__global__ void diffusion_mix_kernel(const float* __restrict__ x, const float* __restrict__ e, float sa, float sb,
                                     float* __restrict__ fake, T* __restrict__ out, int ldout, T* __restrict__ out2, int ldout2,
                                     size_t n, int C) {
  // plain IEEE multiplies and adds in the order of the formula, no FMA contraction: what an unfused TensorFlow op chain computes
  // (train.py:372-375), and independent of the code around it (as for adam_keras_update)
#pragma clang fp contract(off)
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float f = sa * x[i] + sb * e[i];
    fake[i] = f;
    const size_t pix = i / C;
    const int c = (int)(i - pix * C);
    out[pix * ldout + c] = from_f32<T>(f);
    if (out2) out2[pix * ldout2 + c] = from_f32<T>(f);
  }
}
// the estimates from the prediction, by objective (train.py:338-355, 382-413, 452-479; modes of include/gct2.h) - the ONE place:
//   X: x = pred, e = (fake - sa x) / sb;  EPS: e = pred, x = (fake - pred sb) / sa;  SCALED_EPS: e = pred / sb, x = (fake - pred) / sa;
//   V: x = sa fake - sb pred, e = sb fake + sa pred (pred is v = sa eps - sb x, Salimans & Ho 2022): no division, a_t = 0 is valid.
// sa = sqrt(a_t), sb = sqrt(1 - a_t)
template <int MODE>
__device__ __forceinline__ void sample_estimate(float p, float f, float sa, float sb, float& x, float& e) {
#pragma clang fp contract(off)          // (f - sa p) / sb etc. as separate roundings, like the reference's op chain (train.py:382-413)
  if (MODE == GCT2_SAMPLE_X) {
    x = p;
    e = (f - sa * p) / sb;
  } else if (MODE == GCT2_SAMPLE_EPS) {
    e = p;
    x = (f - p * sb) / sa;
  } else if (MODE == GCT2_SAMPLE_SCALED_EPS) {
    e = p / sb;
    x = (f - p) / sa;
  } else {                                  // GCT2_SAMPLE_V
    x = sa * f - sb * p;
    e = sb * f + sa * p;
  }
}
// one sampler update: sample_estimate's x / e, or
//   ODE: x = (pred sb - fake sb1) / (sa1 sb - sa sb1), e untouched; sa1 / sb1 are sa / sb at t - 1
template <int MODE>
__global__ void diffusion_update_kernel(const float* __restrict__ pred, const float* __restrict__ fake, float sa, float sb, float sb1, float den,
                                        float* __restrict__ x, float* __restrict__ e, size_t n) {
#pragma clang fp contract(off)
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float p = pred[i], f = fake[i];
    if constexpr (MODE == GCT2_SAMPLE_ODE) {
      x[i] = (p * sb - f * sb1) / den;
    } else {
      sample_estimate<MODE>(p, f, sa, sb, x[i], e[i]);
    }
  }
}

// ---- one strided DDIM / DDPM step in ONE launch (include/gct2.h: gct2_diffusion_step, _start, _start_image, _step_masked,
// _step_multistep) ----
// sample_estimate's x / e, the clip of x (and e re-derived from the clipped x), then the re-noising to a_prev with
// diffusion_mix_kernel's arithmetic and stores - x_theta and eps_theta never reach memory.  Every operation rounds once.
// The kernels' one argument: pointers a call does not use are nullptr, coefficients it does not use 0.  fake_in, fake_out, hist_in and
// hist_out may alias (in place is part of the contract: a thread reads its element, then writes it); nothing else does
struct SamplerArgs {
  const float* __restrict__ pred; const float* fake_in; const float* hist_in; const float* __restrict__ known; const float* __restrict__ mask;
  float sa, sb, clip, cx, ce, cz;           // sqrt(a_t), sqrt(1 - a_t), the clip bound or 0, the re-noising: cx x + ce e + cz z
  float ck, c1;                             // the kept region's forward process h = cx known + ck z0; the multistep extrapolation
  uint64_t seed, stream_id, offset, offset0, image_stride;     // z at offset + b image_stride + i, z0 at offset0 + b image_stride + i
  float* fake_out; float* hist_out; float* __restrict__ x0_out;
  void* __restrict__ out; int ldout; void* __restrict__ out2; int ldout2;
  int B; uint32_t per_image; int C;         // B * per_image < 2^31 (checked by the entry point)
};

template <int MODE>
__device__ __forceinline__ float step_update(float p, float f, const SamplerArgs& k, float& x) {
#pragma clang fp contract(off)
  float e;
  sample_estimate<MODE>(p, f, k.sa, k.sb, x, e);
  if (k.clip > 0.f) {                       // (wave-uniform)  a NaN fails both comparisons and stays
    const float c = k.clip;
    x = x < -c ? -c : (x > c ? c : x);
    e = (f - k.sa * x) / k.sb;
  }
  return k.cx * x + k.ce * e;
}
// Selects, not a blend, at m >= 1 and m <= 0: a NaN / infinity of g never reaches a kept pixel, a regenerated pixel has
// gct2_diffusion_step's bits
__device__ __forceinline__ float mask_select(float m, float g, float h) {
#pragma clang fp contract(off)
  return m >= 1.f ? g : (m <= 0.f ? h : m * g + (1.f - m) * h);
}
// one element of every step: p, f, kn, m the loaded inputs (0 where the call has none), z0 / z the starting noise's and the step's
// draw.  Returns fake'; x the clipped estimate (the history plane's value), x0 the composited estimate.
//   STEP_START: no update at all, the value is the draw z itself.  STEP_START_IMAGE: the value is h = cx kn + ck z0
//   (diffusion_mix_kernel's arithmetic on the draw), x0 = kn.
//   MULTI (DPM-Solver++ 2M, Lu et al. 2022): the re-noising reads d = x + c1 (x - hist) in x's place, with e re-derived from d.
//   c1 == 0 (wave-uniform; the first step, and generate's last): step_update's own fake', the history is never read.
//   NOISE: + cz z.  MASKED: the mask of the element's pixel selects between that g and h (x and kn for x0)
template <int MODE, bool MASKED, bool MULTI, bool NOISE>
__device__ __forceinline__ float step_element(float p, float f, float kn, float m, float z0, float z, size_t i, const SamplerArgs& k, float& x,
                                              float& x0) {
#pragma clang fp contract(off)
  if constexpr (MODE == STEP_START) {
    return z;
  } else if constexpr (MODE == STEP_START_IMAGE) {
    x0 = kn;
    return k.cx * kn + k.ck * z0;
  } else {
    float g = step_update<MODE>(p, f, k, x);
    if constexpr (MULTI) {
      if (k.c1 != 0.f) {
        const float d = x + k.c1 * (x - k.hist_in[i]);
        const float ed = (f - k.sa * d) / k.sb;
        g = k.cx * d + k.ce * ed;
      }
    }
    if constexpr (NOISE) g = g + k.cz * z;
    if constexpr (MASKED) {
      const float h = k.cx * kn + k.ck * z0;
      x0 = mask_select(m, x, kn);
      return mask_select(m, g, h);
    } else {
      x0 = x;
      return g;
    }
  }
}
template <typename T>
__device__ __forceinline__ void step_store(float v, size_t i, size_t pix, int c, const SamplerArgs& a) {
  a.fake_out[i] = v;
  static_cast<T*>(a.out)[pix * a.ldout + c] = from_f32<T>(v);
  if (a.out2) static_cast<T*>(a.out2)[pix * a.ldout2 + c] = from_f32<T>(v);
}
// one whole Philox counter: four consecutive elements from a flat index that is a multiple of 4, all planes 16-byte aligned - the fp32
// plane moves as a 16-byte access, the compute-dtype copies element by element (a row holds C of them)
template <typename T>
__device__ __forceinline__ void store_quad(f32x4_t v, size_t i, uint32_t pix, int c, const SamplerArgs& a) {
  *reinterpret_cast<f32x4_t*>(a.fake_out + i) = v;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    static_cast<T*>(a.out)[(size_t)pix * a.ldout + c] = from_f32<T>(v[j]);
    if (a.out2) static_cast<T*>(a.out2)[(size_t)pix * a.ldout2 + c] = from_f32<T>(v[j]);
    if (++c == a.C) { c = 0; ++pix; }
  }
}
// the four normals of one Philox counter: one Philox call and two Box-Muller pairs
__device__ __forceinline__ void counter_normals(const SamplerArgs& a, uint64_t ctr, float (&n)[4]) {
  uint32_t r[4];
  philox4x32_10(a.seed, a.stream_id, ctr, r);
  box_muller(r[0], r[1], n[0], n[1]);
  box_muller(r[2], r[3], n[2], n[3]);
}

// no step noise (sigma^2 = 0, the start from an image, every multistep call): the images are one flat range, one element per thread
// (fake_in may be fake_out and hist_in may be hist_out: a thread reads its element of both, then writes it).  Four elements per thread
// with 16-byte accesses measured SLOWER here (25.6 against 20.5 us at 64x128x128x3, profiles/generate_bench.json): consecutive lanes
// then store their copies 4 elements apart.  MASKED and STEP_START_IMAGE draw z0 through philox_normal - a whole Philox call per
// element, and still the faster form: the masked step takes 25.3 us against 28.8 us for a thread per Philox counter with 16-byte
// accesses, the start 20.3 against 26.1 us, at 64x128x128x3 (profiles/img2img_bench.json: consecutive lanes store their copies next to
// each other).  Any offset0 and image_stride
template <typename T, int MODE, bool MASKED, bool MULTI>
__global__ void sampler_flat_kernel(const SamplerArgs a) {
  const size_t n = (size_t)a.B * a.per_image, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float p = 0.f, f = 0.f, kn = 0.f, m = 0.f, z0 = 0.f;
    if constexpr (MASKED || MODE == STEP_START_IMAGE) {
      const uint32_t b = (uint32_t)i / a.per_image, within = (uint32_t)i - b * a.per_image;               // n < 2^31
      z0 = philox_normal(a.seed, a.stream_id, a.offset0 + (uint64_t)b * a.image_stride + within);
      kn = a.known[i];
    }
    const uint32_t pix = (uint32_t)i / (uint32_t)a.C;
    if constexpr (MASKED) m = a.mask[pix];
    if constexpr (MODE != STEP_START_IMAGE) { p = a.pred[i]; f = a.fake_in[i]; }
    float x, x0;
    const float v = step_element<MODE, MASKED, MULTI, false>(p, f, kn, m, z0, 0.f, i, a, x, x0);
    if constexpr (MULTI) if (a.hist_out) a.hist_out[i] = x;
    if constexpr (MODE != STEP_START_IMAGE) if (a.x0_out) a.x0_out[i] = x0;
    step_store<T>(v, i, pix, (int)((uint32_t)i - pix * (uint32_t)a.C), a);
  }
}

// with step noise, and the start from noise: noise_rng_kernel's scheme per image (blockIdx.y walks the images): one thread per Philox
// counter = up to four consecutive elements, one Philox call and two Box-Muller pairs; an image may start and end inside a counter,
// whatever the offsets, image_stride and per_image are.  The counter index is 64 bits wide, so a range across a wrap of its low word
// needs nothing special.  Not MASKED: the thread's counter is the step noise's (element offset + b image_stride + i; STEP_START: the
// value itself).  MASKED, two draws per element: the thread's counter is the STARTING noise's (offset0 + b image_stride + i).
// VEC (the launcher: offset, offset0, image_stride and per_image multiples of 4, 16-byte aligned fp32 planes - what generate passes):
// every counter lies inside its image and the fp32 planes move as 16-byte accesses, 25.0 us where the general form takes 57.3 us
// (profiles/generate_bench.json); MASKED: the step's noise z sits at the same lanes of its own counter, one more Philox call per
// thread, the mask is read per element (a group of four spans up to three pixels at C = 3), 28.1 us where the general form takes
// 76.1 us (profiles/img2img_bench.json).  General form, MASKED: z per element through philox_normal (the two draws may sit at
// different lanes of their counters)
template <typename T, int MODE, bool MASKED, bool VEC>
__global__ void sampler_counter_kernel(const SamplerArgs a) {
  constexpr bool STEP = MODE != STEP_START;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const uint64_t base = a.offset + (uint64_t)b * a.image_stride;                       // the step noise of the image
    const uint64_t own = MASKED ? a.offset0 + (uint64_t)b * a.image_stride : base, end = own + a.per_image;
    const uint64_t c0 = own >> 2;
    const size_t ncounters = (size_t)(((end + 3) >> 2) - c0);
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < ncounters; t += stride) {
      const uint64_t ctr = c0 + t;
      float n0[4];
      counter_normals(a, ctr, n0);
      if constexpr (VEC) {
        const size_t i = (size_t)b * a.per_image + 4 * t;
        float nz[4];
        if constexpr (MASKED) counter_normals(a, (base >> 2) + t, nz);
        f32x4_t p = {}, f = {}, kn = {}, v, x4;
        if constexpr (MASKED) kn = *reinterpret_cast<const f32x4_t*>(a.known + i);
        if constexpr (STEP) { p = *reinterpret_cast<const f32x4_t*>(a.pred + i); f = *reinterpret_cast<const f32x4_t*>(a.fake_in + i); }
        const uint32_t pix0 = (uint32_t)i / (uint32_t)a.C;
        const int ch0 = (int)((uint32_t)i - pix0 * (uint32_t)a.C);
        uint32_t pix = pix0;
        int c = ch0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          float x, x0;
          if constexpr (MASKED) {
            v[j] = step_element<MODE, true, false, true>(p[j], f[j], kn[j], a.mask[pix], n0[j], nz[j], i, a, x, x0);
            if (++c == a.C) { c = 0; ++pix; }
          } else {
            v[j] = step_element<MODE, false, false, true>(p[j], f[j], 0.f, 0.f, 0.f, n0[j], i, a, x, x0);
          }
          if constexpr (STEP) x4[j] = x0;
        }
        if constexpr (STEP) if (a.x0_out) *reinterpret_cast<f32x4_t*>(a.x0_out + i) = x4;
        store_quad<T>(v, i, pix0, ch0, a);
      } else {
        const uint64_t e0 = 4 * ctr;
        const uint64_t first = e0 < own ? own : e0;                 // (< end: the counter range was cut to the image)
        const uint32_t i0 = (uint32_t)b * a.per_image + (uint32_t)(first - own);
        uint32_t pix = i0 / (uint32_t)a.C, c = i0 - pix * (uint32_t)a.C;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint64_t e = e0 + j;
          if (e < first || e >= end) continue;
          const uint32_t within = (uint32_t)(e - own);
          const size_t i = (size_t)b * a.per_image + within;
          float p = 0.f, f = 0.f, v, x, x0;
          if constexpr (STEP) { p = a.pred[i]; f = a.fake_in[i]; }
          if constexpr (MASKED)
            v = step_element<MODE, true, false, true>(p, f, a.known[i], a.mask[pix], n0[j], philox_normal(a.seed, a.stream_id, base + within), i,
                                                      a, x, x0);
          else
            v = step_element<MODE, false, false, true>(p, f, 0.f, 0.f, 0.f, n0[j], i, a, x, x0);
          if constexpr (STEP) if (a.x0_out) a.x0_out[i] = x0;
          step_store<T>(v, i, pix, (int)c, a);
          if (++c == (uint32_t)a.C) { c = 0; ++pix; }
        }
      }
    }
  }
}

}  // namespace

// ---- host launchers (called from capi.hip) ------------------------------------------------------------------
int pw_diffusion_mix(int dtype, const float* x, const float* e, float a, float* fake, void* out, int ldout, void* out2, int ldout2,
                     size_t npix, int C, hipStream_t s) {
  const size_t n = npix * C;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(diffusion_mix_kernel<T>, dim3(blocks_for(n, 256)), dim3(256), 0, s, x, e, sqrtf(a), sqrtf(1.f - a), fake,
                       reinterpret_cast<T*>(out), ldout, reinterpret_cast<T*>(out2), ldout2, n, C);
  });
  return gct2_check_launch("diffusion_mix");
}
int pw_diffusion_update(int mode, const float* pred, const float* fake, double a, double a1, float* x, float* e, size_t n, hipStream_t s) {
  // every scalar in double first, like the Python floats of train.py:382-391, then one cast where it meets an fp32 tensor
  const double dsa = sqrt(a), dsb = sqrt(1. - a), dsa1 = sqrt(a1), dsb1 = sqrt(1. - a1);
  const float sa = (float)dsa, sb = (float)dsb, sb1 = (float)dsb1, den = (float)(dsa1 * dsb - dsa * dsb1);
  with_sample_mode(mode, [&](auto m) {
    hipLaunchKernelGGL(diffusion_update_kernel<decltype(m)::value>, dim3(blocks_for(n, 256)), dim3(256), 0, s, pred, fake, sa, sb, sb1, den, x,
                       e, n);
  });
  return gct2_check_launch("diffusion_update");
}
// the grid of the per-image kernels: x over the Philox counters of one image, y over the images, kMaxBlocks work-groups at the most
static dim3 step_rng_grid(int B, size_t per_image) {
  const int gx = blocks_for(per_image / 4 + 2, 256);
  const int gy = std::max(1, std::min(B, kMaxBlocks / gx));
  return dim3(gx, gy);
}
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
template <typename F> static void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}
int pw_sampler_step(const char* what, const SamplerStep& st, hipStream_t s) {
  const bool start = st.mode == STEP_START, masked = st.mask != nullptr;
  SamplerArgs k = {};
  k.pred = st.pred; k.fake_in = st.fake_in; k.hist_in = st.hist_in; k.known = st.known; k.mask = st.mask;
  k.seed = st.seed; k.stream_id = st.stream_id; k.offset = st.offset; k.offset0 = st.offset0; k.image_stride = st.image_stride;
  k.fake_out = st.fake_out; k.hist_out = st.hist_out; k.x0_out = st.x0_out;
  k.out = st.out; k.ldout = st.ldout; k.out2 = st.out2; k.ldout2 = st.ldout2;
  k.B = st.B; k.per_image = (uint32_t)st.per_image; k.C = st.C;
  float S = 0.f;
  if (st.mode == STEP_START_IMAGE) {               // pw_diffusion_mix's coefficients
    const float A = (float)st.a;
    k.cx = sqrtf(A); k.ck = sqrtf(1.f - A);
  } else if (!start) {
    // sa, sb as pw_diffusion_update forms them; the re-noising coefficients from the fp32 a_prev like pw_diffusion_mix's, and ck of the
    // kept region's forward process
    const float A = (float)st.a_prev;
    S = (float)st.sigma2;
    k.sa = (float)sqrt(st.a); k.sb = (float)sqrt(1. - st.a); k.clip = st.clip > 0. ? (float)st.clip : 0.f;
    k.cx = sqrtf(A); k.ce = sqrtf((1.f - A) - S); k.cz = sqrtf(S); k.ck = sqrtf(1.f - A);
    k.c1 = (float)st.c1;
  }
  const bool flat = st.multistep || (!start && S == 0.f);
  // the four-element form of the counter kernel: every image starts on a Philox counter and on a 16-byte boundary
  const bool vec = aligned16(st.fake_out) && st.offset % 4 == 0 && st.image_stride % 4 == 0 && st.per_image % 4 == 0 &&
                   (start || (aligned16(st.pred) && aligned16(st.fake_in) && aligned16(st.x0_out))) &&
                   (!masked || (aligned16(st.known) && st.offset0 % 4 == 0));
  const dim3 flat_grid(blocks_for((size_t)st.B * st.per_image, 256)), counter_grid = step_rng_grid(st.B, st.per_image), block(256);
  with_dtype(st.dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto launch = [&](auto m) {
      constexpr int MODE = decltype(m)::value;
      if constexpr (MODE == STEP_START) {
        with_flag(vec, [&](auto v) {
          hipLaunchKernelGGL((sampler_counter_kernel<T, MODE, false, decltype(v)::value>), counter_grid, block, 0, s, k);
        });
      } else if constexpr (MODE == STEP_START_IMAGE) {
        hipLaunchKernelGGL((sampler_flat_kernel<T, MODE, false, false>), flat_grid, block, 0, s, k);
      } else if constexpr (MODE != GCT2_SAMPLE_ODE) {    // (refused by the entry points: the ODE objective has no such step)
        with_flag(masked, [&](auto mk) {
          constexpr bool MASKED = decltype(mk)::value;
          if (flat)
            with_flag(st.multistep, [&](auto mu) {
              hipLaunchKernelGGL((sampler_flat_kernel<T, MODE, MASKED, decltype(mu)::value>), flat_grid, block, 0, s, k);
            });
          else
            with_flag(vec, [&](auto v) {
              hipLaunchKernelGGL((sampler_counter_kernel<T, MODE, MASKED, decltype(v)::value>), counter_grid, block, 0, s, k);
            });
        });
      }
    };
    if (start) launch(std::integral_constant<int, STEP_START>{});
    else if (st.mode == STEP_START_IMAGE) launch(std::integral_constant<int, STEP_START_IMAGE>{});
    else with_sample_mode(st.mode, launch);
  });
  return gct2_check_launch(what);
}
