// The sampler's pointwise steps (train.py:323-496 log_sample; Denoiser.generate / encode): gct2_diffusion_mix, gct2_diffusion_update and
// the six one-launch steps gct2_diffusion_step / _start / _start_image / _step_masked / _step_multistep / _step_dynamic, which are ONE
// per-element computation (step_element) behind two traversals (sampler_flat_kernel, sampler_counter_kernel); gct2_x0_quantile, the
// per-image order statistic of |x0| that feeds _step_dynamic (a radix select over sample_estimate's x).  fp32 state, HBM-bound.
// Two-network guidance: gct2_diffusion_step_guided and gct2_x0_quantile_guided are the same kernels with GUIDED set - the prediction is
// combined from two planes on the way in, the compute-dtype copy goes to a second engine's views on the way out.
#include "gct2_common.h"
#include <algorithm>
#include <type_traits>

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
// one sampler update: sample_estimate's x / e (gct2_common.h), or
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
  // gct2_diffusion_step_dynamic: {s_b, r_b} per image in the place of clip, else nullptr.  The LAST field: every field in front of it
  // keeps its kernarg offset.  Without DYN, 78 of the 105 step kernels are then instruction for instruction what they were without the
  // field (only the offsets of the hidden arguments behind the struct move); the 27 four-element counter kernels load B / per_image / C
  // and the hidden grid size in another order, since the two no longer sit side by side (one to six more instructions of 370 to 870)
  const float* __restrict__ rows;
};
// gct2_diffusion_step_guided: a struct of its own behind SamplerArgs, so no field of the existing kernels' argument moves.  pred_guide
// nullptr: p = pred (w is then 1).  out3 / out4: the guide engine's input views, nullptr where the call has none
struct GuidedArgs : SamplerArgs {
  const float* __restrict__ pred_guide; float w;
  void* __restrict__ out3; int ldout3; void* __restrict__ out4; int ldout4;
};
template <bool GUIDED> using StepArgs = std::conditional_t<GUIDED, GuidedArgs, SamplerArgs>;
// the prediction a guided step uses, p = p_guide + w (p_main - p_guide): three operations, each rounded once (the ONE place: the
// guided step and the guided select form the same bits)
__device__ __forceinline__ float guided_pred(float pm, float pg, float w) {
#pragma clang fp contract(off)
  const float d = pm - pg;
  const float t = w * d;
  return pg + t;
}

// the bound of image b's estimate, DYN (gct2_diffusion_step_dynamic) only: gct2_x0_quantile's {s_b, r_b}.  DYN is a template flag, not
// a test of k.rows at run time: the run-time test slowed the existing step with noise (profiles/dynamic_threshold_bench.json,
// dropped_forms: figures recorded once from that build); without DYN the kernels are the ones the other entry points always had
struct ImageBound { float s, r; };
// GUIDED kernels choose between rows and the scalar clip at run time (wave-uniform; no earlier timing depends on them, and the
// instantiation count stays what one flag costs): the scalar clip is the bound {clip, 1}, whose multiply leaves the bits alone
template <bool DYN, bool GUIDED>
__device__ __forceinline__ ImageBound image_bound(const SamplerArgs& k, uint32_t b) {
  if constexpr (DYN) return ImageBound{k.rows[2 * b], k.rows[2 * b + 1]};
  else if constexpr (GUIDED) return k.rows ? ImageBound{k.rows[2 * b], k.rows[2 * b + 1]} : ImageBound{k.clip, 1.f};
  else return ImageBound{0.f, 1.f};
}
template <int MODE, bool DYN, bool GUIDED>
__device__ __forceinline__ float step_update(float p, float f, const SamplerArgs& k, ImageBound q, float& x) {
#pragma clang fp contract(off)
  float e;
  sample_estimate<MODE>(p, f, k.sa, k.sb, x, e);
  if constexpr (DYN || GUIDED) {            // dynamic thresholding: clip to the image's own bound, rescale to the floor
    if (DYN || k.rows || q.s > 0.f) {       // (GUIDED, wave-uniform: rows, else the scalar clip where there is one)
      x = x < -q.s ? -q.s : (x > q.s ? q.s : x);
      x = x * q.r;                          // one rounded multiply; r == 1.0f leaves the bits alone
      e = (f - k.sa * x) / k.sb;
    }
  } else if (k.clip > 0.f) {                       // (wave-uniform)  a NaN fails both comparisons and stays
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
template <int MODE, bool MASKED, bool MULTI, bool NOISE, bool DYN, bool GUIDED = false>
__device__ __forceinline__ float step_element(float p, float f, float kn, float m, float z0, float z, size_t i, const SamplerArgs& k,
                                              ImageBound q, float& x, float& x0) {
#pragma clang fp contract(off)
  if constexpr (MODE == STEP_START) {
    return z;
  } else if constexpr (MODE == STEP_START_IMAGE) {
    x0 = kn;
    return k.cx * kn + k.ck * z0;
  } else {
    float g = step_update<MODE, DYN, GUIDED>(p, f, k, q, x);
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
// (A: SamplerArgs, or GuidedArgs with the guide engine's views out3 / out4, which take the same compute-dtype value)
template <typename T, typename A>
__device__ __forceinline__ void step_store(float v, size_t i, size_t pix, int c, const A& a) {
  a.fake_out[i] = v;
  static_cast<T*>(a.out)[pix * a.ldout + c] = from_f32<T>(v);
  if (a.out2) static_cast<T*>(a.out2)[pix * a.ldout2 + c] = from_f32<T>(v);
  if constexpr (std::is_same_v<A, GuidedArgs>) {
    if (a.out3) static_cast<T*>(a.out3)[pix * a.ldout3 + c] = from_f32<T>(v);
    if (a.out4) static_cast<T*>(a.out4)[pix * a.ldout4 + c] = from_f32<T>(v);
  }
}
// one whole Philox counter: four consecutive elements from a flat index that is a multiple of 4, all planes 16-byte aligned - the fp32
// plane moves as a 16-byte access, the compute-dtype copies element by element (a row holds C of them)
template <typename T, typename A>
__device__ __forceinline__ void store_quad(f32x4_t v, size_t i, uint32_t pix, int c, const A& a) {
  *reinterpret_cast<f32x4_t*>(a.fake_out + i) = v;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    static_cast<T*>(a.out)[(size_t)pix * a.ldout + c] = from_f32<T>(v[j]);
    if (a.out2) static_cast<T*>(a.out2)[(size_t)pix * a.ldout2 + c] = from_f32<T>(v[j]);
    if constexpr (std::is_same_v<A, GuidedArgs>) {
      if (a.out3) static_cast<T*>(a.out3)[(size_t)pix * a.ldout3 + c] = from_f32<T>(v[j]);
      if (a.out4) static_cast<T*>(a.out4)[(size_t)pix * a.ldout4 + c] = from_f32<T>(v[j]);
    }
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
template <typename T, int MODE, bool MASKED, bool MULTI, bool DYN, bool GUIDED = false>
__global__ void sampler_flat_kernel(const StepArgs<GUIDED> a) {
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
    if constexpr (GUIDED) if (a.pred_guide) p = guided_pred(p, a.pred_guide[i], a.w);
    const ImageBound q = image_bound<DYN, GUIDED>(a, (uint32_t)i / a.per_image);
    float x, x0;
    const float v = step_element<MODE, MASKED, MULTI, false, DYN, GUIDED>(p, f, kn, m, z0, 0.f, i, a, q, x, x0);
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
template <typename T, int MODE, bool MASKED, bool VEC, bool DYN, bool GUIDED = false>
__global__ void sampler_counter_kernel(const StepArgs<GUIDED> a) {
  constexpr bool STEP = MODE != STEP_START;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const uint64_t base = a.offset + (uint64_t)b * a.image_stride;                       // the step noise of the image
    const uint64_t own = MASKED ? a.offset0 + (uint64_t)b * a.image_stride : base, end = own + a.per_image;
    const uint64_t c0 = own >> 2;
    const ImageBound q = image_bound<DYN, GUIDED>(a, (uint32_t)b);
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
        if constexpr (GUIDED) if (a.pred_guide) {
          const f32x4_t pg = *reinterpret_cast<const f32x4_t*>(a.pred_guide + i);
#pragma unroll
          for (int j = 0; j < 4; j++) p[j] = guided_pred(p[j], pg[j], a.w);
        }
        const uint32_t pix0 = (uint32_t)i / (uint32_t)a.C;
        const int ch0 = (int)((uint32_t)i - pix0 * (uint32_t)a.C);
        uint32_t pix = pix0;
        int c = ch0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          float x, x0;
          if constexpr (MASKED) {
            v[j] = step_element<MODE, true, false, true, DYN, GUIDED>(p[j], f[j], kn[j], a.mask[pix], n0[j], nz[j], i, a, q, x, x0);
            if (++c == a.C) { c = 0; ++pix; }
          } else {
            v[j] = step_element<MODE, false, false, true, DYN, GUIDED>(p[j], f[j], 0.f, 0.f, 0.f, n0[j], i, a, q, x, x0);
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
          if constexpr (GUIDED) if (a.pred_guide) p = guided_pred(p, a.pred_guide[i], a.w);
          if constexpr (MASKED)
            v = step_element<MODE, true, false, true, DYN, GUIDED>(p, f, a.known[i], a.mask[pix], n0[j],
                                                                   philox_normal(a.seed, a.stream_id, base + within), i, a, q, x, x0);
          else
            v = step_element<MODE, false, false, true, DYN, GUIDED>(p, f, 0.f, 0.f, 0.f, n0[j], i, a, q, x, x0);
          if constexpr (STEP) if (a.x0_out) a.x0_out[i] = x0;
          step_store<T>(v, i, pix, (int)c, a);
          if (++c == (uint32_t)a.C) { c = 0; ++pix; }
        }
      }
    }
  }
}

// ---- dynamic thresholding (Saharia et al. 2022, "Imagen", section 2.3): the per-image order statistic of |x0| (include/gct2.h:
// gct2_x0_quantile) ----
// A radix select over the 31 bits of key = bits(x) & 0x7fffffff, x sample_estimate's - the step's own x0, re-formed from pred / fake on
// every pass, never stored.  Three digit passes, top first: 11 + 10 + 10 bits.  A pass histograms, per image, the digit of the keys
// whose higher digits equal the prefix found so far; the next pass (the finish after the last) scans that table for the bin that holds
// the rank left and carries {prefix, rank left} on in `state`.  Integer atomics only: the counts, hence every bit of the result, do not
// depend on the order of the adds or on the grid.
// scratch, uint32: tables [B][QSEL_ROW] (the three passes' bins side by side, zeroed by the launcher), then state [B][4] =
// {prefix, rank left} after digit 0 (written by pass 1) and after digit 1 (written by pass 2)
constexpr int QSEL_ROW = 4096, QSEL_THREADS = 256, QSEL_WAVES = QSEL_THREADS / 64, QSEL_PER_GROUP = 4096;
// the histogram in LDS.  Shipped: one per wave (privatised).  -DGCT2_QSEL_WAVE_AGGREGATE (`make qsel_agg`: libgct2_qsel_agg.so, a
// measurement build for scripts/bench_dynamic_threshold.py --variant, never loaded by the package) builds the other form instead: ONE
// histogram per work-group, equal digits of a wave collapsed into one add by ballot / readlane.  Same bits either way
#ifdef GCT2_QSEL_WAVE_AGGREGATE
constexpr int QSEL_HISTS = 1;
#else
constexpr int QSEL_HISTS = QSEL_WAVES;
#endif
__host__ __device__ constexpr int qsel_bits(int pass) { return pass == 0 ? 11 : 10; }
__host__ __device__ constexpr int qsel_shift(int pass) { return pass == 0 ? 20 : (pass == 1 ? 10 : 0); }
__host__ __device__ constexpr int qsel_offset(int pass) { return pass == 0 ? 0 : (pass == 1 ? 2048 : 3072); }

// the bin of table[0, bins) that holds the rank-th smallest (1-based, 1 <= rank <= the table's total) and the rank left inside that
// bin.  The whole work-group calls it (bins a multiple of QSEL_THREADS); scan: QSEL_THREADS words, sel: 2 words of LDS
__device__ __forceinline__ void qsel_find(const uint32_t* __restrict__ table, int bins, uint32_t rank, uint32_t* scan, uint32_t* sel,
                                          uint32_t& digit, uint32_t& left) {
  const int t = threadIdx.x, per = bins / QSEL_THREADS;
  uint32_t sum = 0;
  for (int j = 0; j < per; j++) sum += table[t * per + j];
  scan[t] = sum;
  if (t == 0) { sel[0] = 0; sel[1] = 1; }
  __syncthreads();
  for (int d = 1; d < QSEL_THREADS; d <<= 1) {          // inclusive scan of the threads' sums
    const uint32_t add = t >= d ? scan[t - d] : 0u;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const uint32_t incl = scan[t];
  uint32_t below = incl - sum;
  if (below < rank && rank <= incl) {                   // exactly one thread: its bins hold the rank
    for (int j = 0; j < per; j++) {
      const uint32_t c = table[t * per + j];
      if (rank <= below + c) { sel[0] = (uint32_t)(t * per + j); sel[1] = rank - below; break; }
      below += c;
    }
  }
  __syncthreads();
  digit = sel[0];
  left = sel[1];
  __syncthreads();                                      // (sel and scan are free again)
}

// one digit pass: blockIdx.x walks an image's elements, blockIdx.y the images.  Shipped: a histogram per wave in LDS (4 x 2048 x 4 B = 32 KB at
// the top digit, which is essentially the exponent: most of an image falls into a handful of bins, and the waves of a work-group
// would serialise on them), summed and flushed bin by bin - non-zero bins only - into the image's table
// G (gct2_x0_quantile_guided only): the guide's plane and the weight behind the existing arguments, every pass forms guided_pred before
// the estimate - the guided step's x0 bit for bit, nothing materialised
struct QselGuide { const float* __restrict__ pred_guide; float w; };
template <int MODE, int PASS, typename... G>
__global__ void __launch_bounds__(QSEL_THREADS) x0_select_pass_kernel(const float* __restrict__ pred, const float* __restrict__ fake, float sa,
                                                                      float sb, uint32_t rank, uint32_t* __restrict__ tables,
                                                                      uint32_t* __restrict__ state, int B, uint32_t per_image, G... g) {
  static_assert(sizeof...(G) == 0 || (sizeof...(G) == 1 && (std::is_same_v<G, QselGuide> && ...)), "G is nothing or one QselGuide");
  constexpr int BINS = 1 << qsel_bits(PASS), SHIFT = qsel_shift(PASS);
  __shared__ uint32_t hist[QSEL_HISTS * BINS];
  __shared__ uint32_t scan[QSEL_THREADS];
  __shared__ uint32_t sel[2];
  const int t = threadIdx.x;
  uint32_t* mine = hist + (QSEL_HISTS > 1 ? t >> 6 : 0) * BINS;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    uint32_t* table = tables + (size_t)b * QSEL_ROW;
    uint32_t prefix = 0;
    if constexpr (PASS > 0) {                           // the digit the pass before found, from its table
      uint32_t high = 0, left = rank, digit;
      if constexpr (PASS == 2) { high = state[4 * b]; left = state[4 * b + 1]; }
      qsel_find(table + qsel_offset(PASS - 1), 1 << qsel_bits(PASS - 1), left, scan, sel, digit, left);
      prefix = (high << qsel_bits(PASS - 1)) | digit;
      if (blockIdx.x == 0 && t == 0) { state[4 * b + 2 * (PASS - 1)] = prefix; state[4 * b + 2 * (PASS - 1) + 1] = left; }
    }
    for (int j = t; j < QSEL_HISTS * BINS; j += QSEL_THREADS) hist[j] = 0;
    __syncthreads();
    const float* p_b = pred + (size_t)b * per_image;
    const float* f_b = MODE == GCT2_SAMPLE_X ? nullptr : fake + (size_t)b * per_image;
    // (every lane of a wave takes the same trips: the loop runs on the wave's first element, a lane past the image counts nothing)
#ifndef GCT2_QSEL_WAVE_AGGREGATE
#pragma unroll 4
#endif
    for (uint32_t i0 = blockIdx.x * QSEL_THREADS + (t & ~63); i0 < per_image; i0 += gridDim.x * QSEL_THREADS) {
      const uint32_t i = i0 + (t & 63);
      const bool in = i < per_image;
      float p = in ? p_b[i] : 0.f;
      if constexpr (sizeof...(G) > 0) {
        const QselGuide guide = (g, ...);
        p = guided_pred(p, in ? guide.pred_guide[(size_t)b * per_image + i] : 0.f, guide.w);
      }
      float f = 0.f, x, e;
      if constexpr (MODE != GCT2_SAMPLE_X) f = in ? f_b[i] : 0.f;
      sample_estimate<MODE>(p, f, sa, sb, x, e);
      const uint32_t key = __float_as_uint(x) & 0x7fffffffu;
      bool counts = in;
      if constexpr (PASS > 0) counts = in && (key >> (SHIFT + qsel_bits(PASS))) == prefix;
      const uint32_t digit = (key >> SHIFT) & (BINS - 1);
#ifdef GCT2_QSEL_WAVE_AGGREGATE
      unsigned long long todo = __ballot(counts);
      while (todo) {                                    // (wave-uniform) one add per distinct digit among the counting lanes
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t d = (uint32_t)__shfl((int)digit, leader);
        const unsigned long long same = __ballot(counts && digit == d);
        if ((t & 63) == leader) atomicAdd(&mine[d], (uint32_t)__popcll(same));
        todo &= ~same;
      }
#else
      if (counts) atomicAdd(&mine[digit], 1u);
#endif
    }
    __syncthreads();
    for (int j = t; j < BINS; j += QSEL_THREADS) {
      uint32_t c = 0;
#pragma unroll
      for (int w = 0; w < QSEL_HISTS; w++) c += hist[w * BINS + j];
      if (c) atomicAdd(&table[qsel_offset(PASS) + j], c);
    }
    __syncthreads();                                    // (the next image zeroes the histograms)
  }
}

// the last digit from the last pass's table, then the finishing rule of include/gct2.h, once per image
__global__ void __launch_bounds__(QSEL_THREADS) x0_select_finish_kernel(const uint32_t* __restrict__ tables, const uint32_t* __restrict__ state,
                                                                        float F, float* __restrict__ rows, float* __restrict__ q_out, int B) {
  __shared__ uint32_t scan[QSEL_THREADS];
  __shared__ uint32_t sel[2];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    uint32_t digit, left;
    qsel_find(tables + (size_t)b * QSEL_ROW + qsel_offset(2), 1 << qsel_bits(2), state[4 * b + 3], scan, sel, digit, left);
    if (threadIdx.x == 0) {
      const float q = __uint_as_float((state[4 * b + 2] << qsel_bits(2)) | digit);
      const float s = (q > F && q < INFINITY) ? q : F;  // a NaN or infinite q falls back to the fixed bound
      rows[2 * b] = s;
      rows[2 * b + 1] = s == F ? 1.f : F / s;
      if (q_out) q_out[b] = q;
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
size_t pw_x0_quantile_scratch(int B) { return (size_t)B * (QSEL_ROW + 4) * sizeof(uint32_t); }
// a memset of the tables, three digit passes and the finish, all on s: no host synchronisation, nothing read back
// guided (gct2_x0_quantile_guided): the passes that combine pred with pred_guide, whatever w is
int pw_x0_quantile(int mode, const float* pred, const float* fake, double a_t, uint32_t rank, float floor, float* rows, float* q_out,
                   void* scratch, int B, size_t per_image, bool guided, const float* pred_guide, float w, hipStream_t s) {
  const char* what = guided ? "x0_quantile_guided" : "x0_quantile";
  const float sa = (float)sqrt(a_t), sb = (float)sqrt(1. - a_t);           // as pw_sampler_step forms them
  uint32_t* tables = static_cast<uint32_t*>(scratch);
  uint32_t* state = tables + (size_t)B * QSEL_ROW;
  if (hipMemsetAsync(tables, 0, (size_t)B * QSEL_ROW * sizeof(uint32_t), s) != hipSuccess) return gct2_check_launch(what);
  const int gx = blocks_for(per_image, QSEL_PER_GROUP);
  const dim3 grid(gx, std::max(1, std::min(B, kMaxBlocks / gx))), block(QSEL_THREADS);
  with_sample_mode(mode, [&](auto m) {
    constexpr int MODE = decltype(m)::value;
    if constexpr (MODE != GCT2_SAMPLE_ODE) {            // (refused by the entry point)
      if (guided) {
        const QselGuide g{pred_guide, w};
        hipLaunchKernelGGL((x0_select_pass_kernel<MODE, 0, QselGuide>), grid, block, 0, s, pred, fake, sa, sb, rank, tables, state, B, (uint32_t)per_image, g);
        hipLaunchKernelGGL((x0_select_pass_kernel<MODE, 1, QselGuide>), grid, block, 0, s, pred, fake, sa, sb, rank, tables, state, B, (uint32_t)per_image, g);
        hipLaunchKernelGGL((x0_select_pass_kernel<MODE, 2, QselGuide>), grid, block, 0, s, pred, fake, sa, sb, rank, tables, state, B, (uint32_t)per_image, g);
      } else {
        hipLaunchKernelGGL((x0_select_pass_kernel<MODE, 0>), grid, block, 0, s, pred, fake, sa, sb, rank, tables, state, B, (uint32_t)per_image);
        hipLaunchKernelGGL((x0_select_pass_kernel<MODE, 1>), grid, block, 0, s, pred, fake, sa, sb, rank, tables, state, B, (uint32_t)per_image);
        hipLaunchKernelGGL((x0_select_pass_kernel<MODE, 2>), grid, block, 0, s, pred, fake, sa, sb, rank, tables, state, B, (uint32_t)per_image);
      }
    }
  });
  hipLaunchKernelGGL(x0_select_finish_kernel, dim3(std::min(B, kMaxBlocks)), block, 0, s, tables, state, floor, rows, q_out, B);
  return gct2_check_launch(what);
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
  k.rows = st.rows;
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
  if (st.guided) {
    // gct2_diffusion_step_guided: its own instantiations (GUIDED; rows or the scalar clip at run time), never the kernels above
    GuidedArgs g = {};
    static_cast<SamplerArgs&>(g) = k;
    g.pred_guide = st.pred_guide; g.w = (float)st.w;
    g.out3 = st.out3; g.ldout3 = st.ldout3; g.out4 = st.out4; g.ldout4 = st.ldout4;
    const bool gvec = vec && (!st.pred_guide || aligned16(st.pred_guide));
    with_dtype(st.dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      with_sample_mode(st.mode, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        if constexpr (MODE != GCT2_SAMPLE_ODE) {         // (refused by the entry point)
          with_flag(masked, [&](auto mk) {
            constexpr bool MASKED = decltype(mk)::value;
            if (flat)
              with_flag(st.multistep, [&](auto mu) {
                hipLaunchKernelGGL((sampler_flat_kernel<T, MODE, MASKED, decltype(mu)::value, false, true>), flat_grid, block, 0, s, g);
              });
            else
              with_flag(gvec, [&](auto v) {
                hipLaunchKernelGGL((sampler_counter_kernel<T, MODE, MASKED, decltype(v)::value, false, true>), counter_grid, block, 0, s, g);
              });
          });
        }
      });
    });
    return gct2_check_launch(what);
  }
  with_dtype(st.dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto launch = [&](auto m) {
      constexpr int MODE = decltype(m)::value;
      if constexpr (MODE == STEP_START) {
        with_flag(vec, [&](auto v) {
          hipLaunchKernelGGL((sampler_counter_kernel<T, MODE, false, decltype(v)::value, false>), counter_grid, block, 0, s, k);
        });
      } else if constexpr (MODE == STEP_START_IMAGE) {
        hipLaunchKernelGGL((sampler_flat_kernel<T, MODE, false, false, false>), flat_grid, block, 0, s, k);
      } else if constexpr (MODE != GCT2_SAMPLE_ODE) {    // (refused by the entry points: the ODE objective has no such step)
        with_flag(masked, [&](auto mk) {
          constexpr bool MASKED = decltype(mk)::value;
          with_flag(k.rows != nullptr, [&](auto dy) {
            constexpr bool DYN = decltype(dy)::value;
            if (flat)
              with_flag(st.multistep, [&](auto mu) {
                hipLaunchKernelGGL((sampler_flat_kernel<T, MODE, MASKED, decltype(mu)::value, DYN>), flat_grid, block, 0, s, k);
              });
            else
              with_flag(vec, [&](auto v) {
                hipLaunchKernelGGL((sampler_counter_kernel<T, MODE, MASKED, decltype(v)::value, DYN>), counter_grid, block, 0, s, k);
              });
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
