// Progressive distillation (Salimans & Ho 2022; Distiller.targets): the teacher's two DDIM steps and the target solve of a batch whose
// images sit at DIFFERENT timesteps - gct2_distill_start / _step / _target (include/gct2.h).  They are sampler.hip's start from an image
// and its sigma^2 = 0 step with the scalars of the launch replaced by a row of the host's table per image (pair[b] picks it), and the
// second step fused with the solve for the student's pseudo pair; the estimate is sample_estimate (gct2_common.h), the stores are
// sampler.hip's.  fp32 state, every operation rounded once, HBM-bound.
#include "gct2_common.h"
#include <algorithm>

namespace {

// row columns (include/gct2.h GCT2_DISTILL_*)
enum { SA0 = 0, SB0, SA1, SB1, SA2, SB2, RR, DEN, CX0, CK0, CX1, CE1, ROW = GCT2_DISTILL_ROW };
static_assert(ROW == 12, "include/gct2.h and the column list disagree");

// the kernels' one argument: pointers a call does not use are nullptr
struct DistillArgs {
  const float* __restrict__ pred; const float* __restrict__ z1; const float* __restrict__ z0; const float* __restrict__ x;
  const float* __restrict__ eps;             // start: the noise handed in, or nullptr: drawn
  const int32_t* __restrict__ pair; const float* __restrict__ table; const int32_t* __restrict__ ttable; int N;
  float clip;                                // the clip bound or 0
  uint64_t seed, stream_id, offset, image_stride;
  float* __restrict__ o0; float* __restrict__ o1;      // start: z0; step: z1; target: x~ and eps~
  int32_t* __restrict__ t_out; int32_t* __restrict__ t1_out;
  void* __restrict__ out; int ldout; void* __restrict__ out2; int ldout2;
  int B; uint32_t per_image; int C;          // B * per_image < 2^31 (checked by the entry point)
};

// the row of image b: pair[b] clamped into 1..N, so no value reads outside the tables
__device__ __forceinline__ int distill_pair(const DistillArgs& a, uint32_t b) {
  const int j = a.pair[b];
  return (j < 1 ? 1 : (j > a.N ? a.N : j)) - 1;
}
__device__ __forceinline__ const float* distill_row(const DistillArgs& a, uint32_t b) { return a.table + (size_t)distill_pair(a, b) * ROW; }

// sampler.hip's step_update without the re-noising: sample_estimate, the clip of x, e re-derived from the clipped x
template <int MODE>
__device__ __forceinline__ void distill_estimate(float p, float f, float sa, float sb, float clip, float& x, float& e) {
#pragma clang fp contract(off)
  sample_estimate<MODE>(p, f, sa, sb, x, e);
  if (clip > 0.f) {                          // (wave-uniform)  a NaN fails both comparisons and stays
    x = x < -clip ? -clip : (x > clip ? clip : x);
    e = (f - sa * x) / sb;
  }
}
template <typename T>
__device__ __forceinline__ void distill_store(float v, size_t i, const DistillArgs& a) {
  const uint32_t pix = (uint32_t)i / (uint32_t)a.C;
  const int c = (int)((uint32_t)i - pix * (uint32_t)a.C);
  a.o0[i] = v;
  static_cast<T*>(a.out)[(size_t)pix * a.ldout + c] = from_f32<T>(v);
  if (a.out2) static_cast<T*>(a.out2)[(size_t)pix * a.ldout2 + c] = from_f32<T>(v);
}

// gct2_diffusion_start_image with a row per image: one element per thread, the draw through philox_normal - the form that measured
// fastest for the sibling (sampler.hip: sampler_flat_kernel; consecutive lanes store their copies next to each other)
template <typename T>
__global__ void distill_start_kernel(const DistillArgs a) {
#pragma clang fp contract(off)
  const size_t n = (size_t)a.B * a.per_image, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t b = (uint32_t)i / a.per_image, within = (uint32_t)i - b * a.per_image;                   // n < 2^31
    const float* row = distill_row(a, b);
    const float z = a.eps ? a.eps[i] : philox_normal(a.seed, a.stream_id, a.offset + (uint64_t)b * a.image_stride + within);   // (uniform)
    distill_store<T>(row[CX0] * a.x[i] + row[CK0] * z, i, a);
    if (within == 0) {
      const int j = distill_pair(a, b);
      if (a.t_out) a.t_out[b] = a.ttable[2 * j];
      if (a.t1_out) a.t1_out[b] = a.ttable[2 * j + 1];
    }
  }
}

// gct2_diffusion_step at sigma^2 = 0 with a row per image: one element per thread (sampler_flat_kernel's traversal)
template <typename T, int MODE>
__global__ void distill_step_kernel(const DistillArgs a) {
#pragma clang fp contract(off)
  const size_t n = (size_t)a.B * a.per_image, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float* row = distill_row(a, (uint32_t)i / a.per_image);
    float x, e;
    distill_estimate<MODE>(a.pred[i], a.z0[i], row[SA0], row[SB0], a.clip, x, e);
    distill_store<T>(row[CX1] * x + row[CE1] * e, i, a);
  }
}

// the teacher's second step and the solve for the student's pair, one element: z'' lives in a register
template <int MODE>
__device__ __forceinline__ void distill_target_element(float p, float f1, float f0, const float* row, float clip, float& xt, float& et) {
#pragma clang fp contract(off)
  float x2, e2;
  distill_estimate<MODE>(p, f1, row[SA1], row[SB1], clip, x2, e2);
  const float sb2 = row[SB2];
  xt = sb2 == 0.f ? x2 : ((row[SA2] * x2 + sb2 * e2) - row[RR] * f0) / row[DEN];
  et = (f0 - row[SA0] * xt) / row[SB0];
}
// no compute-dtype copies here, so nothing ties consecutive lanes to consecutive elements: VEC (the launcher: per_image a multiple of
// 4, 16-byte aligned planes) moves four elements of one image per thread as 16-byte accesses; else one element per thread
template <int MODE, bool VEC>
__global__ void distill_target_kernel(const DistillArgs a) {
  const size_t n = (size_t)a.B * a.per_image, stride = (size_t)gridDim.x * blockDim.x;
  if constexpr (VEC) {
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n / 4; q += stride) {
      const size_t i = 4 * q;
      const float* row = distill_row(a, (uint32_t)i / a.per_image);
      const f32x4_t p = *reinterpret_cast<const f32x4_t*>(a.pred + i), f1 = *reinterpret_cast<const f32x4_t*>(a.z1 + i),
                    f0 = *reinterpret_cast<const f32x4_t*>(a.z0 + i);
      f32x4_t xt, et;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float x, e;
        distill_target_element<MODE>(p[j], f1[j], f0[j], row, a.clip, x, e);
        xt[j] = x; et[j] = e;
      }
      *reinterpret_cast<f32x4_t*>(a.o0 + i) = xt;
      *reinterpret_cast<f32x4_t*>(a.o1 + i) = et;
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const float* row = distill_row(a, (uint32_t)i / a.per_image);
      distill_target_element<MODE>(a.pred[i], a.z1[i], a.z0[i], row, a.clip, a.o0[i], a.o1[i]);
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ---- host launchers (called from capi.hip, which has checked every argument) -------------------------------------------------------
int pw_distill_start(int dtype, const float* x, const float* eps, const int32_t* pair, const float* table, const int32_t* ttable, int N, uint64_t seed,
                     uint64_t stream_id, uint64_t offset, uint64_t image_stride, float* z0_out, int32_t* t_out, int32_t* t1_out, void* out,
                     int ldout, void* out2, int ldout2, int B, size_t per_image, int C, hipStream_t s) {
  DistillArgs k = {};
  k.x = x; k.eps = eps; k.pair = pair; k.table = table; k.ttable = ttable; k.N = N;
  k.seed = seed; k.stream_id = stream_id; k.offset = offset; k.image_stride = image_stride;
  k.o0 = z0_out; k.t_out = t_out; k.t1_out = t1_out; k.out = out; k.ldout = ldout; k.out2 = out2; k.ldout2 = ldout2;
  k.B = B; k.per_image = (uint32_t)per_image; k.C = C;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(distill_start_kernel<T>, dim3(blocks_for((size_t)B * per_image, 256)), dim3(256), 0, s, k);
  });
  return gct2_check_launch("distill_start");
}
int pw_distill_step(int mode, int dtype, const float* pred, const float* z0, const int32_t* pair, const float* table, int N, double clip,
                    float* z1_out, void* out, int ldout, void* out2, int ldout2, int B, size_t per_image, int C, hipStream_t s) {
  DistillArgs k = {};
  k.pred = pred; k.z0 = z0; k.pair = pair; k.table = table; k.N = N; k.clip = clip > 0. ? (float)clip : 0.f;
  k.o0 = z1_out; k.out = out; k.ldout = ldout; k.out2 = out2; k.ldout2 = ldout2;
  k.B = B; k.per_image = (uint32_t)per_image; k.C = C;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    with_sample_mode(mode, [&](auto m) {
      constexpr int MODE = decltype(m)::value;
      if constexpr (MODE != GCT2_SAMPLE_ODE)              // (refused by the entry point)
        hipLaunchKernelGGL((distill_step_kernel<T, MODE>), dim3(blocks_for((size_t)B * per_image, 256)), dim3(256), 0, s, k);
    });
  });
  return gct2_check_launch("distill_step");
}
int pw_distill_target(int mode, const float* pred2, const float* z1, const float* z0, const int32_t* pair, const float* table, int N,
                      double clip, float* x_out, float* eps_out, int B, size_t per_image, hipStream_t s) {
  DistillArgs k = {};
  k.pred = pred2; k.z1 = z1; k.z0 = z0; k.pair = pair; k.table = table; k.N = N; k.clip = clip > 0. ? (float)clip : 0.f;
  k.o0 = x_out; k.o1 = eps_out; k.B = B; k.per_image = (uint32_t)per_image; k.C = 1;
  const size_t n = (size_t)B * per_image;
  const bool vec = per_image % 4 == 0 && aligned16(pred2) && aligned16(z1) && aligned16(z0) && aligned16(x_out) && aligned16(eps_out);
  with_sample_mode(mode, [&](auto m) {
    constexpr int MODE = decltype(m)::value;
    if constexpr (MODE != GCT2_SAMPLE_ODE) {              // (refused by the entry point)
      if (vec) hipLaunchKernelGGL((distill_target_kernel<MODE, true>), dim3(blocks_for(n / 4, 256)), dim3(256), 0, s, k);
      else hipLaunchKernelGGL((distill_target_kernel<MODE, false>), dim3(blocks_for(n, 256)), dim3(256), 0, s, k);
    }
  });
  return gct2_check_launch("distill_target");
}
