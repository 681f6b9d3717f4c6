// HBM-bound kernels of the train step: RNG + noising (train.py:224-234), Dense(3) head (train.py:198-202),
// fp32 MSE and its gradient (train.py:262-272), bias gradients, Keras Adam (train.py:75) and the
// mixed-precision loss-scale state machine (train.py:82-83).  All are streaming kernels: 16-byte accesses
// where the layout allows, grids capped at a few workgroups per CU with grid-stride loops.
#include "gct2_common.h"
#include <algorithm>

namespace {

// (Philox4x32-10, box_muller and philox_normal: gct2_common.h - sampler.hip and data.hip draw from the same streams)

__global__ void rng_uniform_int_kernel(uint64_t seed, uint64_t stream_id, uint64_t offset, int32_t* out, size_t n,
                                       int lo, uint64_t range) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t e = offset + i;
  uint32_t r[4];
  philox4x32_10(seed, stream_id, e >> 2, r);
  // range = hi - lo + 1 <= 2^32 (all of int32: the result is lo + r); the sum wraps in 32 bits, and lands inside [lo, hi]
  out[i] = (int32_t)((uint32_t)lo + (uint32_t)(((uint64_t)r[e & 3] * range) >> 32));
}

__global__ void rng_normal_kernel(uint64_t seed, uint64_t stream_id, uint64_t offset, float* out, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = philox_normal(seed, stream_id, offset + i);
}

// noised = x sqrt(a) + eps sqrt(1 - a), a = alpha_dash(t) (train.py:85-93, 229-234).  fp32 / bf16: fp32 arithmetic, one rounding at
// the store.  fp16 = Keras' mixed_float16 policy, where x, eps and t are fp16 tensors (train.py:38, 227, 292): every operation
// rounds to fp16 (t/(steps+1), 1-t, the square, *0.25, both square roots, both products, the sum).
//
// Where the pair (sa, sb) comes from: NoiseFormula evaluates the reference's live line (train.py:93) per thread; NoiseTable reads
// what the host put down for the schedule in force (trainer_math.noise_table: any of train.py:88-93, or the user's own body) from
// float[steps][2], entry t - 1 = (sa, sb), as ONE 8-byte load - sb is never derived from sa.  t_int is clamped to 1..steps before the
// address is formed (the rule of gct2_dense_steps_fwd).  Both kernel arguments are wave-uniform; the mix is the same.
struct NoiseFormula { int steps1; };
struct NoiseTable { const float* coef; int steps; };
template <typename T> struct NoiseCoef {
  float sa, sb;
  __device__ __forceinline__ NoiseCoef(int t_int, NoiseTable tab) {
    const int t = t_int < 1 ? 1 : (t_int > tab.steps ? tab.steps : t_int);
    const f32x2_t p = reinterpret_cast<const f32x2_t*>(tab.coef)[t - 1];
    sa = p[0]; sb = p[1];
  }
  __device__ __forceinline__ NoiseCoef(int t_int, NoiseFormula formula) {
#pragma clang fp contract(off)      // every fp16 operation rounds on its own (no fused multiply-add): that IS the model
    const int steps1 = formula.steps1;
    if constexpr (sizeof(T) == 2 && !__is_same(T, __bf16)) {
      const _Float16 t = (_Float16)((_Float16)(float)t_int / (_Float16)(float)steps1);
      const _Float16 om = (_Float16)1.0f - t;
      const _Float16 a = (_Float16)(om * om) * (_Float16)0.25f;
      sa = (float)(_Float16)sqrtf((float)a);
      sb = (float)(_Float16)sqrtf((float)(_Float16)((_Float16)1.0f - a));
    } else {
      // fp32: a division, like train.py:87 (t_int times the rounded reciprocal gives another sqrt(a) at 36 of 200 timesteps, which
      // an fp32 output shows in its last bit).  bf16 keeps the product: there the two differ only where the fp32 sum is a tie of
      // the bf16 store (one element in ~2^16), and the 16-bit train step stays bit-identical from commit to commit.
      float t;
      if constexpr (__is_same(T, float)) t = (float)t_int / (float)steps1;
      else t = (float)t_int * (1.0f / (float)steps1);
      const float a = (1.f - t) * (1.f - t) * 0.25f;
      sa = sqrtf(a); sb = sqrtf(1.f - a);
    }
  }
  __device__ __forceinline__ T mix(float x, float eps) const {
#pragma clang fp contract(off)
    if constexpr (sizeof(T) == 2 && !__is_same(T, __bf16)) {
      const _Float16 xs = (_Float16)x * (_Float16)sa, es = (_Float16)eps * (_Float16)sb;     // x is exact in fp16 (u8/128 - 1)
      return (T)(xs + es);
    } else {
      return from_f32<T>(x * sa + eps * sb);
    }
  }
};

// noising with eps drawn on the fly from the same stream positions rng_normal_kernel would use.  One thread per Philox
// counter = 4 consecutive elements of the flattened [pixel][channel] image: one Philox call, two logs and two sin/cos pairs
// make four normals (philox_normal spends a whole call per element); values are bit-identical to it.
template <typename T, typename Src>
__global__ void noise_rng_kernel(const float* __restrict__ x, const int32_t* __restrict__ t_int, uint64_t seed, uint64_t stream_id,
                                 uint64_t offset, float* __restrict__ eps_out, T* __restrict__ out, int ldout,
                                 T* __restrict__ out2, int ldout2, size_t n, int HW, int C, Src src) {
  const uint64_t c0 = offset >> 2;
  const size_t ncounters = (size_t)(((offset + n + 3) >> 2) - c0);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < ncounters; t += stride) {
    const uint64_t ctr = c0 + t;
    uint32_t r[4];
    philox4x32_10(seed, stream_id, ctr, r);
    float nrm[4];
    box_muller(r[0], r[1], nrm[0], nrm[1]);
    box_muller(r[2], r[3], nrm[2], nrm[3]);
    // elements 4 ctr .. 4 ctr + 3 of the flattened image: (pixel, channel, batch) advance incrementally (one division per thread)
    const uint64_t e0 = 4 * ctr;
    const uint64_t first = e0 < offset ? offset : e0;
    if (first >= offset + n) continue;
    const uint32_t i0 = (uint32_t)(first - offset);
    uint32_t pix = i0 / (uint32_t)C, c = i0 - pix * (uint32_t)C;
    uint32_t b = pix / (uint32_t)HW, rem = pix - b * (uint32_t)HW;
    NoiseCoef<T> nc(1, src);
    bool have = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t e = e0 + k;
      if (e < first || e >= offset + n) continue;
      if (!have) {
        nc = NoiseCoef<T>(t_int[b], src);
        have = true;
      }
      const size_t i = (size_t)(e - offset);
      if (eps_out) eps_out[i] = nrm[k];
      const T v = nc.mix(x[i], nrm[k]);
      out[(size_t)pix * ldout + c] = v;
      if (out2) out2[(size_t)pix * ldout2 + c] = v;
      if (++c == (uint32_t)C) {
        c = 0; ++pix;
        if (++rem == (uint32_t)HW) { rem = 0; ++b; have = false; }
      }
    }
  }
}

// r06: the train step's shape of the same kernel - 3 channels into the packed 4-slot image, 16-bit storage, nothing else written, stream
// position a multiple of 12.  A thread owns 12 consecutive elements = THREE Philox counters = FOUR whole pixels: three 16-byte loads of x,
// the same counters / normals / mix as noise_rng_kernel (bit-identical), and the four pixels leave as two 16-byte stores (slot 3 = 0,
// which is what the packed image holds there) instead of twelve 2-byte ones.  11 -> 5 us at config 3, on the step's critical path.
template <typename T, typename Src>
__global__ __launch_bounds__(256) void noise_rng_px4_kernel(const float* __restrict__ x, const int32_t* __restrict__ t_int, uint64_t seed,
                                                            uint64_t stream_id, uint64_t ctr0, T* __restrict__ out, size_t ngroups, int HW,
                                                            Src src) {
  static_assert(sizeof(T) == 2, "16-bit storage types only");
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < ngroups; t += stride) {
    const uint32_t b = (uint32_t)((4 * t) / (size_t)HW);          // HW % 4 == 0: the four pixels belong to one image
    const NoiseCoef<T> nc(t_int[b], src);
    const f32x4_t* xs = reinterpret_cast<const f32x4_t*>(x) + 3 * t;
    const f32x4_t x0 = xs[0], x1 = xs[1], x2 = xs[2];
    const float xv[12] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3], x2[0], x2[1], x2[2], x2[3]};
    uint16_t v[12];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      uint32_t r[4];
      philox4x32_10(seed, stream_id, ctr0 + 3 * t + j, r);
      float nrm[4];
      box_muller(r[0], r[1], nrm[0], nrm[1]);
      box_muller(r[2], r[3], nrm[2], nrm[3]);
#pragma unroll
      for (int k = 0; k < 4; k++) v[4 * j + k] = __builtin_bit_cast(uint16_t, nc.mix(xv[4 * j + k], nrm[k]));
    }
    u32x4_t o0, o1;
    o0[0] = (uint32_t)v[0] | ((uint32_t)v[1] << 16);  o0[1] = (uint32_t)v[2];
    o0[2] = (uint32_t)v[3] | ((uint32_t)v[4] << 16);  o0[3] = (uint32_t)v[5];
    o1[0] = (uint32_t)v[6] | ((uint32_t)v[7] << 16);  o1[1] = (uint32_t)v[8];
    o1[2] = (uint32_t)v[9] | ((uint32_t)v[10] << 16); o1[3] = (uint32_t)v[11];
    u32x4_t* dst = reinterpret_cast<u32x4_t*>(out) + 2 * t;
    dst[0] = o0;
    dst[1] = o1;
  }
}

template <typename T, typename Src>
__global__ void noise_kernel(const float* __restrict__ x, const int32_t* __restrict__ t_int, const float* __restrict__ eps,
                             T* __restrict__ out, int ldout, T* __restrict__ out2, int ldout2, size_t npix, int HW, int C,
                             Src src) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t total = npix * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const size_t pix = i / C;
    const int c = (int)(i - pix * C);
    const int b = (int)(pix / HW);
    const NoiseCoef<T> nc(t_int[b], src);                      // alpha_dash, train.py:87-93
    const T v = nc.mix(x[i], eps[i]);                          // train.py:231-234
    out[pix * ldout + c] = v;
    if (out2) out2[pix * ldout2 + c] = v;
  }
}

// ---- Dense(3) head -------------------------------------------------------------------------------------
// (keras_f16_point, the mixed_float16 rounding points of the head: gct2_common.h)
template <typename T>
__global__ void dense_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w, const float* __restrict__ b,
                                 float* __restrict__ y, int M, int Cin, int Cout) {
  extern __shared__ float wsm[];                  // [Cin][4]
  for (int i = threadIdx.x; i < Cin * 4; i += blockDim.x) {
    const int o = i & 3, k = i >> 2;
    wsm[i] = (o < Cout) ? w[k * Cout + o] : 0.f;
  }
  __syncthreads();
  const int stride = gridDim.x * blockDim.x;
  for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += stride) {
    const T* xr = x + (size_t)m * ldx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < Cin; k++) {
      const float v = to_f32(xr[k]);
      a0 = fmaf(v, wsm[4 * k + 0], a0); a1 = fmaf(v, wsm[4 * k + 1], a1);
      a2 = fmaf(v, wsm[4 * k + 2], a2); a3 = fmaf(v, wsm[4 * k + 3], a3);
    }
    const float acc[4] = {a0, a1, a2, a3};
    for (int o = 0; o < Cout; o++) y[(size_t)m * Cout + o] = keras_f16_point<T>(acc[o] + (b ? b[o] : 0.f));
  }
}

// one workgroup walks tiles of PIX pixels: dx per pixel, and per-(i,o) partial sums of dw/db over the tile
template <typename T, int PIX>
__global__ __launch_bounds__(256) void dense_bwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                                        const float* __restrict__ dy, T* __restrict__ dx, int lddx,
                                                        float* __restrict__ dw, float* __restrict__ db, int M, int Cin,
                                                        int Cout, int Cmask) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* wsm = reinterpret_cast<float*>(smem_raw);          // [Cin][4]
  float* dys = wsm + Cin * 4;                               // [PIX][4]
  T* xs = reinterpret_cast<T*>(dys + PIX * 4);              // [PIX][Cin]
  const int tid = threadIdx.x;
  for (int i = tid; i < Cin * 4; i += 256) {
    const int o = i & 3, k = i >> 2;
    wsm[i] = (o < Cout) ? w[k * Cout + o] : 0.f;
  }
  const int nout = (Cin + 1) * Cout;                        // dw entries + db entries: entry e = tid + 256 k belongs to thread tid
  constexpr int ENT = 8;                                    // (Cin + 1) * Cout <= 2048
  float wacc[ENT];
#pragma unroll
  for (int k = 0; k < ENT; k++) wacc[k] = 0.f;
  const int ntiles = (M + PIX - 1) / PIX;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int mbase = tile * PIX;
    __syncthreads();
    for (int i = tid; i < PIX * Cin; i += 256) {
      const int pm = i / Cin, k = i - pm * Cin;
      xs[i] = (mbase + pm < M) ? x[(size_t)(mbase + pm) * ldx + k] : from_f32<T>(0.f);
    }
    for (int i = tid; i < PIX * 4; i += 256) {
      const int pm = i >> 2, o = i & 3;
      dys[i] = (o < Cout && mbase + pm < M) ? keras_f16_point<T>(dy[(size_t)(mbase + pm) * Cout + o]) : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < PIX * Cmask; i += 256) {
      const int pm = i / Cmask, k = i - pm * Cmask;
      if (mbase + pm >= M) continue;
      float g = dys[4 * pm] * wsm[4 * k] + dys[4 * pm + 1] * wsm[4 * k + 1] + dys[4 * pm + 2] * wsm[4 * k + 2] +
                dys[4 * pm + 3] * wsm[4 * k + 3];
      if (!(to_f32(xs[pm * Cin + k]) > 0.f)) g = 0.f;
      dx[(size_t)(mbase + pm) * lddx + k] = from_f32<T>(g);
    }
#pragma unroll
    for (int k = 0; k < ENT; k++) {
      const int e = tid + 256 * k;
      if (e >= nout) break;
      const int my_i = e / Cout, my_o = e - my_i * Cout;
      float a = wacc[k];
      if (my_i < Cin) {
        for (int pm = 0; pm < PIX; pm++) a = fmaf(to_f32(xs[pm * Cin + my_i]), dys[4 * pm + my_o], a);
      } else {
        for (int pm = 0; pm < PIX; pm++) a += dys[4 * pm + my_o];
      }
      wacc[k] = a;
    }
  }
#pragma unroll
  for (int k = 0; k < ENT; k++) {
    const int e = tid + 256 * k;
    if (e >= nout) break;
    const int my_i = e / Cout, my_o = e - my_i * Cout;
    if (my_i < Cin) atomicAdd(dw + my_i * Cout + my_o, wacc[k]);
    else if (db) atomicAdd(db + my_o, wacc[k]);
  }
}

// ---- per-timestep heads: Dense(Cout * steps), gathered by t (train.py:199, 203, 211-214) ----------------------------------
// t is constant over an image, so the gathered head is the Dense(3) head above with the weight slice s = t_int[image] - 1 of the
// (Cin, steps * Cout) kernel.  blockIdx.y = image: a work-group never sees two images.  The slice index is clamped into
// [0, steps) before any address is formed (a t_int outside 1..steps is a caller error, not an out-of-bounds access).
__device__ __forceinline__ int steps_slice(const int32_t* __restrict__ t_int, int img, int steps) {
  const int s = t_int[img] - 1;
  return s < 0 ? 0 : (s >= steps ? steps - 1 : s);
}

// dense_fwd_kernel's arithmetic (k ascending, one fmaf per term, bias last, keras_f16_point) on the image's slice: bit-identical to
// it on the image's rows with a contiguous copy of the slice
template <typename T>
__global__ __launch_bounds__(256) void dense_steps_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                                              const float* __restrict__ b, const int32_t* __restrict__ t_int,
                                                              float* __restrict__ y, int HW, int Cin, int Cout, int steps) {
  extern __shared__ float wsm[];                  // [Cin][4]
  const int img = blockIdx.y;
  const int s = steps_slice(t_int, img, steps);
  const int ldw = steps * Cout;                   // (Cin * steps * Cout < 2^31: checked by the entry point)
  for (int i = threadIdx.x; i < Cin * 4; i += blockDim.x) {
    const int o = i & 3, k = i >> 2;
    wsm[i] = (o < Cout) ? w[k * ldw + s * Cout + o] : 0.f;
  }
  __syncthreads();
  const int stride = gridDim.x * blockDim.x;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += stride) {
    const size_t m = (size_t)img * HW + p;
    const T* xr = x + m * ldx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < Cin; k++) {
      const float v = to_f32(xr[k]);
      a0 = fmaf(v, wsm[4 * k + 0], a0); a1 = fmaf(v, wsm[4 * k + 1], a1);
      a2 = fmaf(v, wsm[4 * k + 2], a2); a3 = fmaf(v, wsm[4 * k + 3], a3);
    }
    const float acc[4] = {a0, a1, a2, a3};
    for (int o = 0; o < Cout; o++) y[m * Cout + o] = keras_f16_point<T>(acc[o] + (b ? b[s * Cout + o] : 0.f));
  }
}

// work-group (chunk, image) walks the tiles chunk, chunk + gridDim.x, ... of PIX pixels of its image: dx per pixel exactly as
// dense_bwd_kernel forms it, and the per-(i,o) sums of dw / db over its pixels, which leave as ONE partial row
// part[image * gridDim.x + chunk][(Cin + 1) * Cout] - no atomics (dense_steps_finish_kernel adds the rows in order)
template <typename T, int PIX>
__global__ __launch_bounds__(256) void dense_steps_bwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                                              const int32_t* __restrict__ t_int, const float* __restrict__ dy,
                                                              T* __restrict__ dx, int lddx, float* __restrict__ part, int HW, int Cin,
                                                              int Cout, int steps, int Cmask) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* wsm = reinterpret_cast<float*>(smem_raw);          // [Cin][4]
  float* dys = wsm + Cin * 4;                               // [PIX][4]
  T* xs = reinterpret_cast<T*>(dys + PIX * 4);              // [PIX][Cin]
  const int tid = threadIdx.x, img = blockIdx.y;
  const int s = steps_slice(t_int, img, steps);
  const int ldw = steps * Cout;
  for (int i = tid; i < Cin * 4; i += 256) {
    const int o = i & 3, k = i >> 2;
    wsm[i] = (o < Cout) ? w[k * ldw + s * Cout + o] : 0.f;
  }
  const int nout = (Cin + 1) * Cout;                        // dw entries + db entries: entry e = tid + 256 k belongs to thread tid
  constexpr int ENT = 8;                                    // (Cin + 1) * Cout <= 2048
  float wacc[ENT];
#pragma unroll
  for (int k = 0; k < ENT; k++) wacc[k] = 0.f;
  const size_t m0 = (size_t)img * HW;                       // first pixel of the image
  const int ntiles = (HW + PIX - 1) / PIX;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int pbase = tile * PIX;
    __syncthreads();
    for (int i = tid; i < PIX * Cin; i += 256) {
      const int pm = i / Cin, k = i - pm * Cin;
      xs[i] = (pbase + pm < HW) ? x[(m0 + pbase + pm) * ldx + k] : from_f32<T>(0.f);
    }
    for (int i = tid; i < PIX * 4; i += 256) {
      const int pm = i >> 2, o = i & 3;
      dys[i] = (o < Cout && pbase + pm < HW) ? keras_f16_point<T>(dy[(m0 + pbase + pm) * Cout + o]) : 0.f;
    }
    __syncthreads();
    if (dx) {
      for (int i = tid; i < PIX * Cmask; i += 256) {
        const int pm = i / Cmask, k = i - pm * Cmask;
        if (pbase + pm >= HW) continue;
        float g = dys[4 * pm] * wsm[4 * k] + dys[4 * pm + 1] * wsm[4 * k + 1] + dys[4 * pm + 2] * wsm[4 * k + 2] +
                  dys[4 * pm + 3] * wsm[4 * k + 3];
        if (!(to_f32(xs[pm * Cin + k]) > 0.f)) g = 0.f;
        dx[(m0 + pbase + pm) * lddx + k] = from_f32<T>(g);
      }
    }
#pragma unroll
    for (int k = 0; k < ENT; k++) {
      const int e = tid + 256 * k;
      if (e >= nout) break;
      const int my_i = e / Cout, my_o = e - my_i * Cout;
      float a = wacc[k];
      if (my_i < Cin) {
        for (int pm = 0; pm < PIX; pm++) a = fmaf(to_f32(xs[pm * Cin + my_i]), dys[4 * pm + my_o], a);
      } else {
        for (int pm = 0; pm < PIX; pm++) a += dys[4 * pm + my_o];
      }
      wacc[k] = a;
    }
  }
  float* row = part + ((size_t)img * gridDim.x + blockIdx.x) * nout;
#pragma unroll
  for (int k = 0; k < ENT; k++) {
    const int e = tid + 256 * k;
    if (e >= nout) break;
    row[e] = wacc[k];
  }
}

// blockIdx.y = slice: entry e of dw / db of that slice = the partial rows of the images that selected it, images ascending, chunks
// ascending, one thread per entry (a fixed order: the same inputs give the same bits); a slice no image selected gets +0.0
__global__ __launch_bounds__(256) void dense_steps_finish_kernel(const float* __restrict__ part, const int32_t* __restrict__ t_int,
                                                                 float* __restrict__ dw, float* __restrict__ db, int B, int nchunk,
                                                                 int Cin, int Cout, int steps, int accumulate) {
  const int nout = (Cin + 1) * Cout, s = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nout) return;
  float acc = 0.f;
  for (int img = 0; img < B; img++) {
    if (steps_slice(t_int, img, steps) != s) continue;
    const float* rows = part + (size_t)img * nchunk * nout + e;
    for (int c = 0; c < nchunk; c++) acc += rows[(size_t)c * nout];
  }
  const int my_i = e / Cout, my_o = e - my_i * Cout;
  float* dst = my_i < Cin ? dw + (my_i * (steps * Cout) + s * Cout + my_o) : (db ? db + (s * Cout + my_o) : nullptr);
  if (dst) *dst = accumulate ? *dst + acc : acc;
}

// ---- MSE -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                  float* __restrict__ dpred, float* __restrict__ partials, size_t n,
                                                  const float* __restrict__ loss_scale_ptr) {
  const float scale = (loss_scale_ptr ? *loss_scale_ptr : 1.f) * 2.0f / (float)n;
  float acc = 0.f;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float d = pred[i] - target[i];
    acc = fmaf(d, d, acc);
    if (dpred) dpred[i] = d * scale;              // (null: gct2_loss_fwd_bwd's loss-only call)
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ float ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ __launch_bounds__(256) void mse_finish_kernel(const float* __restrict__ partials, int nparts, float* loss, float inv_n) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += (double)partials[i];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ double ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *loss = (float)((ws[0] + ws[1] + ws[2] + ws[3]) * (double)inv_n);
}

// ---- fused head for the train step: Dense(3) forward + fp32 MSE + its gradient + Dense backward, ONE pass over R_0 -------
// (train.py:198-202, 262-272 and their autodiff).  Per tile of 256 pixels: the 16-bit rows are copied to LDS with
// 16-byte loads (a tile is one contiguous byte range because consecutive pixels are `ld` apart), thread = pixel
// computes pred / dpred / the masked input gradient row (ds_read_b128; row stride ld*2 bytes is an odd multiple of
// 16 for ld = 72, hence conflict-free), the gradient rows leave through LDS as whole 16-byte chunks, and threads
// (i, o) accumulate dw[i][o] += x[pix][i] * dpred[pix][o] over the tile.
template <typename T, int PIX>
__global__ __launch_bounds__(256) void dense_head_train_kernel(const T* __restrict__ x, int ld, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ target,
                                                               float* __restrict__ pred_out, T* __restrict__ dx, int lddx,
                                                               float* __restrict__ dw, float* __restrict__ db,
                                                               float* __restrict__ partials, int M, int Cin, int Cout, int Cmask,
                                                               const float* __restrict__ loss_scale_ptr, float* __restrict__ db_dx) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int nchunk = ld >> 3;                                    // 16-byte chunks per pixel row
  T* xs = reinterpret_cast<T*>(smem_raw);                        // [PIX][ld]
  T* dxs = xs + PIX * ld;                                        // [PIX][Cmask]
  float* dps = reinterpret_cast<float*>(dxs + PIX * Cmask);      // [PIX][4]
  float* wsm = dps + PIX * 4;                                    // [ld][4]  (rows >= Cin are zero)
  const int tid = threadIdx.x;
  for (int i = tid; i < ld * 4; i += 256) {
    const int o = i & 3, k = i >> 2;
    wsm[i] = (o < Cout && k < Cin) ? w[k * Cout + o] : 0.f;
  }
  const float gscale = (loss_scale_ptr ? *loss_scale_ptr : 1.f) * 2.0f / ((float)M * (float)Cout);
  const int nout = (Cin + 1) * Cout;
  const int my_i = tid / Cout, my_o = tid - my_i * Cout;
  float wacc = 0.f, lacc = 0.f, bacc = 0.f;   // bacc: column sum of the gradient rows for channel tid (db of the layer below)
  const int ntiles = (M + PIX - 1) / PIX;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int mbase = tile * PIX;
    const int npx = min(PIX, M - mbase);
    __syncthreads();
    {   // stage the tile: npx * nchunk chunks, contiguous in memory
      const u32x4_t* src = reinterpret_cast<const u32x4_t*>(x + (size_t)mbase * ld);
      u32x4_t* dst = reinterpret_cast<u32x4_t*>(xs);
      for (int i = tid; i < npx * nchunk; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    if (tid < npx) {
      const int m = mbase + tid;
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      const u32x4_t* row = reinterpret_cast<const u32x4_t*>(xs + tid * ld);
      for (int c = 0; c < nchunk; c++) {
        const u32x4_t v = row[c];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const float lo = unpack_lo<T>(v[q]), hi = unpack_hi<T>(v[q]);
          const f32x4_t w0 = *reinterpret_cast<const f32x4_t*>(wsm + 4 * (8 * c + 2 * q));
          const f32x4_t w1 = *reinterpret_cast<const f32x4_t*>(wsm + 4 * (8 * c + 2 * q + 1));
#pragma unroll
          for (int o = 0; o < 4; o++) a[o] = fmaf(hi, w1[o], fmaf(lo, w0[o], a[o]));
        }
      }
      float dp[4] = {0.f, 0.f, 0.f, 0.f};
      for (int o = 0; o < Cout; o++) {
        const float pr = keras_f16_point<T>(a[o] + (bias ? bias[o] : 0.f));
        const float d = pr - target[(size_t)m * Cout + o];
        if (pred_out) pred_out[(size_t)m * Cout + o] = pr;
        lacc = fmaf(d, d, lacc);
        dp[o] = keras_f16_point<T>(d * gscale);
      }
      *reinterpret_cast<f32x4_t*>(dps + 4 * tid) = f32x4_t{dp[0], dp[1], dp[2], dp[3]};
      u32x4_t* drow = reinterpret_cast<u32x4_t*>(dxs + tid * Cmask);
      for (int c = 0; c < (Cmask >> 3); c++) {
        const u32x4_t v = row[c];
        u32x4_t g4;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const f32x4_t w0 = *reinterpret_cast<const f32x4_t*>(wsm + 4 * (8 * c + 2 * q));
          const f32x4_t w1 = *reinterpret_cast<const f32x4_t*>(wsm + 4 * (8 * c + 2 * q + 1));
          float g0 = dp[0] * w0[0] + dp[1] * w0[1] + dp[2] * w0[2] + dp[3] * w0[3];
          float g1 = dp[0] * w1[0] + dp[1] * w1[1] + dp[2] * w1[2] + dp[3] * w1[3];
          if (!(unpack_lo<T>(v[q]) > 0.f)) g0 = 0.f;
          if (!(unpack_hi<T>(v[q]) > 0.f)) g1 = 0.f;
          g4[q] = pack2<T>(g0, g1);
        }
        drow[c] = g4;
      }
    } else if (tid < PIX) {
      *reinterpret_cast<f32x4_t*>(dps + 4 * tid) = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    {   // gradient rows out: Cmask/8 chunks per pixel
      const int cpr = Cmask >> 3;
      for (int i = tid; i < npx * cpr; i += 256) {
        const int pm = i / cpr, c = i - pm * cpr;
        *reinterpret_cast<u32x4_t*>(dx + (size_t)(mbase + pm) * lddx + c * 8) = reinterpret_cast<const u32x4_t*>(dxs)[i];
      }
    }
    if (tid < nout) {
      if (my_i < Cin) {
        for (int pm = 0; pm < npx; pm++) wacc = fmaf(to_f32(xs[pm * ld + my_i]), dps[4 * pm + my_o], wacc);
      } else {
        for (int pm = 0; pm < npx; pm++) wacc += dps[4 * pm + my_o];
      }
    }
    if (db_dx && tid >= 256 - Cmask) {           // the last Cmask threads (idle above) sum the stored gradient rows
      const int c = tid - (256 - Cmask);
      for (int pm = 0; pm < npx; pm++) bacc += to_f32(dxs[pm * Cmask + c]);
    }
  }
  if (tid < nout) {
    if (my_i < Cin) atomicAdd(dw + my_i * Cout + my_o, wacc);
    else if (db) atomicAdd(db + my_o, wacc);
  }
  if (db_dx && tid >= 256 - Cmask) atomicAdd(db_dx + (tid - (256 - Cmask)), bacc);
  for (int off = 32; off > 0; off >>= 1) lacc += __shfl_down(lacc, off, 64);
  __shared__ float lws[4];
  if ((tid & 63) == 0) lws[tid >> 6] = lacc;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = lws[0] + lws[1] + lws[2] + lws[3];
}

// ---- the same fused head on the matrix cores ------------------------------------------------------------------------------
// One wave = 16 pixels per trip, operands straight from global memory in MFMA fragment layout (no LDS staging):
//   pred[o][pix]  = sum_c W[c][o] x[pix][c]         A = W^T (the fp32 kernel as a three-term 16-bit sum, rows o < Cout), B = x rows
//   g[c][pix]     = sum_o W[c][o] d[pix][o]         A = W rows in the permuted order below, B = d = pred - target (hi + lo)
// so the 16-bit operands carry the fp32 kernel and the fp32 residual as multi-term sums (forward ~fp32; backward ~2^-17, far
// below the 16-bit rounding of the stored gradient).
// Output row rho = 4g + r of backward MFMA ct is channel 32 (ct>>1) + 8 g + 4 (ct&1) + r: exactly the channels whose x values
// this lane already holds as its forward B fragments, so the ReLU mask and the 16-byte gradient store need no shuffle.
// dW / db / db_dx / loss are accumulated per lane and leave as one partial row per work-group (HEAD_ROW floats) for
// dense_head_finish_kernel: no atomics, fixed summation order.
// partial row layout HEAD_ROW: gct2_common.h
template <typename T>
__global__ __launch_bounds__(256, 2) void dense_head_mfma_kernel(const T* __restrict__ x, int ld, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, const float* __restrict__ target,
                                                                 float* __restrict__ pred_out, T* __restrict__ dx, int lddx,
                                                                 float* __restrict__ part, int M, int Cin, int Cout,
                                                                 const float* __restrict__ loss_scale_ptr,
                                                                 const T* __restrict__ x2, int ldx2) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, q = lane & 15;
  const float gscale = (loss_scale_ptr ? *loss_scale_ptr : 1.f) * 2.0f / ((float)M * (float)Cout);
  const float inv_gscale = 1.0f / gscale;
  auto split = [](float v, T& hi, T& lo) { hi = from_f32<T>(v); lo = from_f32<T>(v - to_f32(hi)); };
  auto pk = [](T a, T b) { return (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16); };
  // forward A operands: row o = q, reduction slots = channels 32 kk + 8 g + j
  u32x4_t a_f[3][3];                                            // three-term split: pred keeps fp32 accuracy
#pragma unroll
  for (int kk = 0; kk < 3; kk++) {
    T hi[8], mid[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int c = 32 * kk + 8 * g + j;
      const float v = (q < Cout && c < Cin && (kk < 2 || g == 0)) ? w[c * Cout + q] : 0.f;
      split(v, hi[j], mid[j]);
      const float rest = (v - to_f32(hi[j])) - to_f32(mid[j]);
      lo[j] = from_f32<T>(rest);
    }
    a_f[kk][0] = u32x4_t{pk(hi[0], hi[1]), pk(hi[2], hi[3]), pk(hi[4], hi[5]), pk(hi[6], hi[7])};
    a_f[kk][1] = u32x4_t{pk(mid[0], mid[1]), pk(mid[2], mid[3]), pk(mid[4], mid[5]), pk(mid[6], mid[7])};
    a_f[kk][2] = u32x4_t{pk(lo[0], lo[1]), pk(lo[2], lo[3]), pk(lo[4], lo[5]), pk(lo[6], lo[7])};
  }
  // backward A operands (lanes g == 0 only): row rho = q -> channel ch; slots {Whi0..2, Whi0..2, 0, 0} and {Wlo0..2, 0...}
  u32x4_t a_b[4][2];
#pragma unroll
  for (int ct = 0; ct < 4; ct++) {
    const int ch = 32 * (ct >> 1) + 8 * (q >> 2) + 4 * (ct & 1) + (q & 3);
    T hi[3], lo[3];
#pragma unroll
    for (int o = 0; o < 3; o++) split((g == 0 && o < Cout) ? w[ch * Cout + o] : 0.f, hi[o], lo[o]);
    const T z = from_f32<T>(0.f);
    a_b[ct][0] = u32x4_t{pk(hi[0], hi[1]), pk(hi[2], hi[0]), pk(hi[1], hi[2]), 0u};
    a_b[ct][1] = u32x4_t{pk(lo[0], lo[1]), pk(lo[2], z), 0u, 0u};
  }
  float bv[3];
#pragma unroll
  for (int o = 0; o < 3; o++) bv[o] = (bias && o < Cout) ? bias[o] : 0.f;
  const uint32_t tail_keep = Cin - 64;                         // valid channels in the third fragment (pad channels may hold anything)

  float wacc[3][8][3];
#pragma unroll
  for (int kk = 0; kk < 3; kk++)
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
      for (int o = 0; o < 3; o++) wacc[kk][j][o] = 0.f;
  float bacc[2][8];
#pragma unroll
  for (int kk = 0; kk < 2; kk++)
#pragma unroll
    for (int j = 0; j < 8; j++) bacc[kk][j] = 0.f;
  float dbacc[3] = {0.f, 0.f, 0.f}, lacc = 0.f;

  const int ngroups = (M + 15) >> 4;
  const int gstride = gridDim.x * 4;
  auto load = [&](int grp, u32x4_t (&xf)[3]) {
    const int p = grp * 16 + q;
    xf[0] = xf[1] = xf[2] = u32x4_t{0u, 0u, 0u, 0u};
    if (grp < ngroups && p < M) {
      const T* row = x + (size_t)p * ld + 8 * g;
      xf[0] = gload128(row);
      xf[1] = gload128(row + 32);
      if (g == 0) {
        if (x2) {   // channels 64.. live in a packed side buffer (<= 4 of them, 8-byte aligned rows)
          const u32x2_t v2 = *reinterpret_cast<const u32x2_t*>(x2 + (size_t)p * ldx2);
          xf[2] = u32x4_t{v2[0], v2[1], 0u, 0u};
        } else xf[2] = gload128(row + 64);
      }
    }
  };
  u32x4_t cur[3], nxt[3];
  int grp = blockIdx.x * 4 + wave;
  load(grp, cur);
  for (; grp < ngroups; grp += gstride) {
    load(grp + gstride, nxt);
    const int p = grp * 16 + q;
    const bool pv = p < M;
    if (g == 0) {                                              // zero the pad channels >= Cin of the third fragment
#pragma unroll
      for (int j2 = 0; j2 < 4; j2++) {
        const uint32_t keep = tail_keep >= 2u * j2 + 2u ? 0xffffffffu : (tail_keep == 2u * j2 + 1u ? 0xffffu : 0u);
        cur[2][j2] &= keep;
      }
    }
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
      acc = mfma16<T>(a_f[kk][2], cur[kk], acc);            // smallest terms first
      acc = mfma16<T>(a_f[kk][1], cur[kk], acc);
      acc = mfma16<T>(a_f[kk][0], cur[kk], acc);
    }
    // lanes g == 0: acc[o] = pred[pixel q][o]
    float d[3] = {0.f, 0.f, 0.f};
    if (g == 0 && pv) {
#pragma unroll
      for (int o = 0; o < 3; o++) {
        if (o < Cout) {
          const float pr = keras_f16_point<T>(acc[o] + bv[o]);
          d[o] = pr - target[(size_t)p * Cout + o];
          if (pred_out) pred_out[(size_t)p * Cout + o] = pr;
          lacc = fmaf(d[o], d[o], lacc);
        }
      }
    }
    // the gradient entering the Dense output, dsc = d * gscale (an fp16 tensor under mixed_float16: keras_f16_point); the backward
    // MFMAs take it unscaled (dsc / gscale, = d itself when nothing is rounded) and multiply by gscale afterwards
    T dh[3], dl[3];
    float dsc[3];
#pragma unroll
    for (int o = 0; o < 3; o++) {
      dsc[o] = keras_f16_point<T>(d[o] * gscale);
      constexpr bool kF16 = sizeof(T) == 2 && !__is_same(T, __bf16);
      split(kF16 ? dsc[o] * inv_gscale : d[o], dh[o], dl[o]);
    }
    const u32x4_t bb = {pk(dh[0], dh[1]), pk(dh[2], dl[0]), pk(dl[1], dl[2]), 0u};   // zero in lanes g > 0 (d = 0 there)
    float dp[3];
#pragma unroll
    for (int o = 0; o < 3; o++) {
      dp[o] = __shfl(dsc[o], q, 64);                           // every lane group gets the gradient of its pixel
      if (g == 0) dbacc[o] += dp[o];
    }
    u32x4_t gout[2];
#pragma unroll
    for (int ct = 0; ct < 4; ct++) {
      f32x4_t gd = {0.f, 0.f, 0.f, 0.f};
      gd = mfma16<T>(a_b[ct][0], bb, gd);
      gd = mfma16<T>(a_b[ct][1], bb, gd);
      const int kk = ct >> 1, h = ct & 1;
      float gv[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t xw = cur[kk][2 * h + (r >> 1)];
        const float xv = (r & 1) ? unpack_hi<T>(xw) : unpack_lo<T>(xw);
        gv[r] = xv > 0.f ? gd[r] * gscale : 0.f;
        bacc[kk][4 * h + r] += gv[r];
      }
      gout[kk][2 * h] = pack2<T>(gv[0], gv[1]);
      gout[kk][2 * h + 1] = pack2<T>(gv[2], gv[3]);
    }
    if (pv) {
      T* drow = dx + (size_t)p * lddx + 8 * g;
      *reinterpret_cast<u32x4_t*>(drow) = gout[0];
      *reinterpret_cast<u32x4_t*>(drow + 32) = gout[1];
    }
#pragma unroll
    for (int kk = 0; kk < 3; kk++)
#pragma unroll
      for (int j2 = 0; j2 < 4; j2++) {
        const float x0 = unpack_lo<T>(cur[kk][j2]), x1 = unpack_hi<T>(cur[kk][j2]);
#pragma unroll
        for (int o = 0; o < 3; o++) {
          wacc[kk][2 * j2][o] = fmaf(x0, dp[o], wacc[kk][2 * j2][o]);
          wacc[kk][2 * j2 + 1][o] = fmaf(x1, dp[o], wacc[kk][2 * j2 + 1][o]);
        }
      }
    cur[0] = nxt[0]; cur[1] = nxt[1]; cur[2] = nxt[2];
  }

  // ---- reductions: over the 16 pixel lanes (butterfly), then over the 4 waves (LDS), one partial row per work-group ----
  __shared__ float red[4][HEAD_ROW];
  for (int i = tid; i < 4 * HEAD_ROW; i += 256) (&red[0][0])[i] = 0.f;
  __syncthreads();
  auto bfly = [](float t) {
    t = row16_sum(t);
    return t;
  };
#pragma unroll
  for (int kk = 0; kk < 3; kk++)
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
      for (int o = 0; o < 3; o++) {
        const float t = bfly(wacc[kk][j][o]);
        const int c = 32 * kk + 8 * g + j;
        if (q == 0 && o < Cout && c < Cin && (kk < 2 || g == 0)) red[wave][c * Cout + o] = t;
      }
#pragma unroll
  for (int kk = 0; kk < 2; kk++)
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float t = bfly(bacc[kk][j]);
      if (q == 0) red[wave][224 + 32 * kk + 8 * g + j] = t;
    }
#pragma unroll
  for (int o = 0; o < 3; o++) {
    const float t = bfly(dbacc[o]);
    if (lane == 0) red[wave][216 + o] = t;
  }
  {
    const float t = bfly(lacc);
    if (lane == 0) red[wave][219] = t;
  }
  __syncthreads();
  for (int i = tid; i < HEAD_ROW; i += 256) part[(size_t)blockIdx.x * HEAD_ROW + i] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
}

// sums the head's partial rows: column -> dW / db / loss / db of the layer below.  9 work-groups x (32 columns x 32 row lanes).
__global__ __launch_bounds__(1024) void dense_head_finish_kernel(const float* __restrict__ part, int rows, float* __restrict__ dw,
                                                                 float* __restrict__ db, float* __restrict__ loss,
                                                                 float* __restrict__ db_dx, int ndw, int Cout, float inv_n,
                                                                 int accumulate) {
  const int tid = threadIdx.x, cx = tid & 31, rl = tid >> 5;
  const int c = blockIdx.x * 32 + cx;
  double acc = 0.0;
  int r = rl;
  for (; r + 7 * 32 < rows; r += 8 * 32) {        // 8 independent loads in flight, added in row order (same sums as one at a time)
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; u++) t[u] = part[(size_t)(r + 32 * u) * HEAD_ROW + c];
#pragma unroll
    for (int u = 0; u < 8; u++) acc += (double)t[u];
  }
  for (; r < rows; r += 32) acc += (double)part[(size_t)r * HEAD_ROW + c];
  __shared__ double red[32][33];
  red[rl][cx] = acc;
  __syncthreads();
  if (rl == 0) {
    double t = 0.0;
    for (int k = 0; k < 32; k++) t += red[k][cx];
    const float tf = (float)t;
    if (c < ndw) dw[c] = accumulate ? dw[c] + tf : tf;
    else if (c >= 216 && c < 216 + Cout) { if (db) db[c - 216] = accumulate ? db[c - 216] + tf : tf; }
    else if (c == 219) *loss = (float)(t * (double)inv_n);
    else if (c >= 224 && db_dx) db_dx[c - 224] = accumulate ? db_dx[c - 224] + tf : tf;
  }
}

// the four noise variants of train.py:416-431 from one eps image [H,W,C]: out[0] = eps, out[1] = nearest-upsample x4 of the
// 4x4 average pool, out[2] = rolled by one pixel along H and W, out[3] = per-pixel nearest entry of dictionary [H,W,K,C]
__global__ void noise_edits_kernel(const float* __restrict__ eps, const float* __restrict__ dict, int K, float* __restrict__ out,
                                   int H, int W, int C) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= H * W) return;
  const int h = idx / W, w = idx - h * W;
  const size_t img = (size_t)H * W * C;
  const float* px = eps + (size_t)idx * C;
  const int hs = (h + H - 1) % H, wsft = (w + W - 1) % W;     // tf.roll(x, 1, axis): out[i] = in[i - 1]
  const int h0 = h & ~3, w0 = w & ~3;
  for (int c = 0; c < C; c++) {
    out[(size_t)idx * C + c] = px[c];
    float a = 0.f;
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) a += eps[((size_t)(h0 + i) * W + (w0 + j)) * C + c];
    out[img + (size_t)idx * C + c] = a * (1.0f / 16.0f);
    out[2 * img + (size_t)idx * C + c] = eps[((size_t)hs * W + wsft) * C + c];
  }
  int best = 0;
  float bestd = 0.f;
  for (int k = 0; k < K; k++) {
    float d = 0.f;
    for (int c = 0; c < C; c++) {
      const float t = px[c] - dict[((size_t)idx * K + k) * C + c];
      d += t * t;
    }
    if (k == 0 || d < bestd) { bestd = d; best = k; }          // first minimum, like tf.argmin
  }
  for (int c = 0; c < C; c++) out[3 * img + (size_t)idx * C + c] = dict[((size_t)idx * K + best) * C + c];
}

// ---- input contract (train.py:285-293): random crop, random left-right flip, u8 -> value/128 - 1, one launch per batch ------
// src: concatenated decoded RGB images (u8, HWC); per image b: byte offset, original height/width, crop origin, flip flag
__global__ void image_prepare_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ offsets, const int32_t* __restrict__ dims,
                                     float* __restrict__ dst, int B, int size) {
  const size_t per = (size_t)size * size * 3;
  const size_t total = per * B;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int b = (int)(i / per);
    const int r = (int)(i - (size_t)b * per);
    const int c = r % 3, xy = r / 3, x = xy % size, y = xy / size;
    const int W0 = dims[5 * b + 1], oy = dims[5 * b + 2], ox = dims[5 * b + 3], flip = dims[5 * b + 4];
    const int sx = ox + (flip ? size - 1 - x : x);
    const uint8_t v = src[offsets[b] + ((size_t)(oy + y) * W0 + sx) * 3 + c];
    dst[i] = (float)v * (1.0f / 128.0f) - 1.0f;                  // exact: v/128 has at most 8 significant bits
  }
}

// ---- small helpers of the off-by-default model variants (train.py:106-112 residual add, autodiff of the fused ReLUs,
// train.py:238-252 targets): elementwise, views with a pixel stride ----------------------------------------------------------
template <typename T>
__global__ void relu_mask_kernel(const T* __restrict__ act, int ldact, T* __restrict__ d, int ldd, size_t n, int C) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const size_t pix = i / C;
    const int c = (int)(i - pix * C);
    if (!(to_f32(act[pix * ldact + c]) > 0.f)) d[pix * ldd + c] = from_f32<T>(0.f);
  }
}
template <typename T>
__global__ void add_kernel(T* __restrict__ dst, int lddst, const T* __restrict__ src, int ldsrc, size_t n, int C) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const size_t pix = i / C;
    const int c = (int)(i - pix * C);
    dst[pix * lddst + c] = from_f32<T>(to_f32(dst[pix * lddst + c]) + to_f32(src[pix * ldsrc + c]));
  }
}
// out = a[b] * x + c[b] * eps (eps may be null: out = a[b] * x), fp32, per-image coefficients; both products and the sum rounded
// once each (no FMA contraction), like the unfused op chain of train.py:238-252 and every other pointwise kernel of the step
__global__ void mix_per_image_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ a,
                                     const float* __restrict__ c, float* __restrict__ out, size_t n, size_t per_image) {
#pragma clang fp contract(off)
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const size_t b = i / per_image;
    out[i] = a[b] * x[i] + (eps ? c[b] * eps[i] : 0.f);
  }
}

// ---- bias gradient: db[c] += sum_m dz[m][c] --------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ dz, int ld, float* __restrict__ db, size_t M, int C,
                                                     int rows_per_block, float sign) {
  // thread = (channel within a 64-wide tile, one of 4 row lanes)
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rl = threadIdx.x >> 6;
  const size_t r0 = (size_t)blockIdx.y * rows_per_block;
  const size_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  float acc = 0.f;
  if (c < C)
    for (size_t r = r0 + rl; r < r1; r += 4) acc += to_f32(dz[r * ld + c]);
  __shared__ float ws[256];
  ws[threadIdx.x] = acc;
  __syncthreads();
  if (rl == 0 && c < C) atomicAdd(db + c, sign * (ws[threadIdx.x] + ws[threadIdx.x + 64] + ws[threadIdx.x + 128] + ws[threadIdx.x + 192]));
}
// 16-bit types, 16-byte loads: thread = (8-channel chunk of a 64-wide tile, one of 32 row lanes)
template <typename T>
__global__ __launch_bounds__(256) void colsum_vec_kernel(const T* __restrict__ dz, int ld, float* __restrict__ db, size_t M, int C,
                                                         int rows_per_block, float sign) {
  const int c8 = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c = blockIdx.x * 64 + c8 * 8;
  const size_t r0 = (size_t)blockIdx.y * rows_per_block;
  const size_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    for (size_t r = r0 + rl; r < r1; r += 32) {
      const u32x4_t v = gload128(dz + r * ld + c);
#pragma unroll
      for (int k = 0; k < 4; k++) { acc[2 * k] += unpack_lo<T>(v[k]); acc[2 * k + 1] += unpack_hi<T>(v[k]); }
    }
  }
  __shared__ float ws[32][65];
#pragma unroll
  for (int k = 0; k < 8; k++) ws[rl][c8 * 8 + k] = acc[k];
  __syncthreads();
  if (threadIdx.x < 64) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 32; r++) s += ws[r][threadIdx.x];
    const int cc = blockIdx.x * 64 + threadIdx.x;
    if (cc < C) atomicAdd(db + cc, sign * s);
  }
}

// ---- Keras Adam over a flat arena ------------------------------------------------------------------------
template <typename S, bool HAS_SHADOW>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                   float* __restrict__ g, S* __restrict__ shadow, size_t n, float alpha,
                                                   float b1, float b2, float eps, float grad_mul,
                                                   const gct2_loss_scale_state* __restrict__ ls, int zero_grad,
                                                   const float* __restrict__ slabs, int nslab, size_t slab_stride, size_t n_slab) {
  // slabs != NULL: the gradient of the first n_slab elements (a multiple of 4) is the ordered sum of `nslab` partial slabs
  // (slab s at slabs + s * slab_stride) left by a weight-gradient launch - it is never written to or read from g.
  // ls != NULL (LossScaleOptimizer): unscale, skip on non-finite gradients, alpha of the device-side step counter.
  const bool skip = ls && ls->found_inf != 0;
  const float inv_scale = (ls ? ls->inv_scale : 1.f) * grad_mul;
  if (ls) alpha = ls->alpha;
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const float ob1 = 1.f - b1, ob2 = 1.f - b2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4_t gv;
    if (slabs && (i << 2) < n_slab) {
      const f32x4_t* src = reinterpret_cast<const f32x4_t*>(slabs) + i;
      const size_t st4 = slab_stride >> 2;
      gv = __builtin_nontemporal_load(src);
      int sidx = 1;
      for (; sidx + 8 <= nslab; sidx += 8) {     // 8 independent slab loads in flight, added in slab order
        f32x4_t t[8];
#pragma unroll
        for (int u = 0; u < 8; u++) t[u] = __builtin_nontemporal_load(src + (size_t)(sidx + u) * st4);
#pragma unroll
        for (int u = 0; u < 8; u++) gv += t[u];
      }
      for (; sidx < nslab; sidx++) gv += __builtin_nontemporal_load(src + (size_t)sidx * st4);
    } else {
      gv = reinterpret_cast<f32x4_t*>(g)[i];
      if (zero_grad) reinterpret_cast<f32x4_t*>(g)[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    if (skip) continue;
    // everything here is touched once per step: streaming (nt) accesses keep it from displacing the GEMM operands in the L2s
    f32x4_t pv = __builtin_nontemporal_load(reinterpret_cast<f32x4_t*>(p) + i), mv = __builtin_nontemporal_load(reinterpret_cast<f32x4_t*>(m) + i),
            vv = __builtin_nontemporal_load(reinterpret_cast<f32x4_t*>(v) + i);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float pp = pv[k], mm = mv[k], v1 = vv[k];
      adam_keras_update(pp, mm, v1, gv[k] * inv_scale, alpha, b1, ob1, b2, ob2, eps);
      pv[k] = pp; mv[k] = mm; vv[k] = v1;
    }
    __builtin_nontemporal_store(pv, reinterpret_cast<f32x4_t*>(p) + i);
    __builtin_nontemporal_store(mv, reinterpret_cast<f32x4_t*>(m) + i);
    __builtin_nontemporal_store(vv, reinterpret_cast<f32x4_t*>(v) + i);
    if (HAS_SHADOW) {
      if constexpr (sizeof(S) == 2) {
        u32x2_t o = {pack2<S>(pv[0], pv[1]), pack2<S>(pv[2], pv[3])};
        reinterpret_cast<u32x2_t*>(shadow)[i] = o;
      } else {
        reinterpret_cast<f32x4_t*>(shadow)[i] = pv;
      }
    }
  }
  // tail (n % 4 elements)
  const size_t i = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float gg = g[i] * inv_scale;
    if (zero_grad) g[i] = 0.f;
    if (!skip) {
      float mm = m[i], vv = v[i], pp = p[i];
      adam_keras_update(pp, mm, vv, gg, alpha, b1, ob1, b2, ob2, eps);
      m[i] = mm; v[i] = vv; p[i] = pp;
      if (HAS_SHADOW) shadow[i] = from_f32<S>(pp);
    }
  }
}

// ---- Keras' optimizer EMA over a flat arena: average = momentum * average + (1 - momentum) * var [TF] --------------------------
template <typename S, bool HAS_SHADOW>
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, S* __restrict__ shadow, size_t n,
                                                  float momentum, float one_minus, const gct2_loss_scale_state* __restrict__ ls) {
  // two products and one sum, each rounded to fp32 (no FMA contraction: as for adam_keras_update, the bits must not depend on what
  // hipcc fuses).  ls != NULL (LossScaleOptimizer): a skipped step leaves the averages alone - nothing is written.
#pragma clang fp contract(off)
  if (ls && ls->found_inf != 0) return;
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    // touched once per step, like the optimizer's arenas: streaming accesses
    f32x4_t ev = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(ema) + i);
    const f32x4_t pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p) + i);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float a = momentum * ev[k], b = one_minus * pv[k];
      ev[k] = a + b;
    }
    __builtin_nontemporal_store(ev, reinterpret_cast<f32x4_t*>(ema) + i);
    if constexpr (HAS_SHADOW) {
      const u32x2_t o = {pack2<S>(ev[0], ev[1]), pack2<S>(ev[2], ev[3])};
      reinterpret_cast<u32x2_t*>(shadow)[i] = o;
    }
  }
  // tail (n % 4 elements)
  const size_t i = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float a = momentum * ema[i], b = one_minus * p[i];
    const float e = a + b;
    ema[i] = e;
    if constexpr (HAS_SHADOW) shadow[i] = from_f32<S>(e);
  }
}

template <typename S>
__global__ void cast_kernel(const float* __restrict__ src, S* __restrict__ dst, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = from_f32<S>(src[i]);
}

// ---- loss scale ------------------------------------------------------------------------------------------
__global__ void ls_init_kernel(gct2_loss_scale_state* s, float scale) {
  s->scale = scale; s->inv_scale = 1.f / scale; s->good_steps = 0; s->found_inf = 0;
  s->applied_steps = 0; s->alpha = 0.f; s->reserved[0] = s->reserved[1] = 0;
}
// found_inf = 0; alpha of THIS step: WarmUp (train.py:57-65, float32 like the reference) x Adam's bias correction [TF], with
// k = applied_steps = optimizer.iterations (a skipped step does not advance it)
__global__ void ls_begin_kernel(gct2_loss_scale_state* s, float base_lr, int warmup_steps, float b1, float b2) {
  s->found_inf = 0;
  const int k = s->applied_steps;
  const float lr = k < warmup_steps ? base_lr * (float)(k + 1) / (float)(warmup_steps + 1) : base_lr;
  const double t = (double)(k + 1);
  s->alpha = (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
}
__global__ void ls_check_kernel(const float* __restrict__ g, size_t n, gct2_loss_scale_state* s) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float x = g[i];
    bad |= !(fabsf(x) <= 3.402823466e38f);      // false for inf and nan
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&s->found_inf, 1);
}
__global__ void ls_update_kernel(gct2_loss_scale_state* s, int growth_interval) {
  if (s->found_inf) {
    s->scale = fmaxf(s->scale * 0.5f, 1.f); s->good_steps = 0;
  } else {
    s->applied_steps += 1;
    s->good_steps += 1;
    if (s->good_steps >= growth_interval) { s->scale *= 2.f; s->good_steps = 0; }
  }
  s->inv_scale = 1.f / s->scale;
}

// ---- gradient clipping (Keras clipnorm / global_clipnorm / clipvalue [TF]) ----------------------------------------------------
// stage one of gct2_grad_sumsq: work-group c owns partial c = one chunk of GCT2_SUMSQ_CHUNK elements (the last chunk of a segment
// may be shorter) and never reads outside its segment.  g' = fl32(g * k) as adam_kernel forms it; the square (exact) and every sum
// in fp64, in a fixed order: a thread over its own elements in address order, the 64 lanes of a wave by an xor butterfly (both
// operands of every add are the same pair on both lanes, so all lanes hold the same bits), the four waves in wave order.
// L2 (gct2_grad_sumsq_l2): the element squared is g_r = fl(g' + fl(seg_coeff[s] * p)), the regularized gradient the update kernel forms;
// a segment whose coefficient is 0 skips the add (and the read of p).  found_inf still comes from the raw g alone.
template <bool L2>
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, const float* __restrict__ p,
                                                            const gct2_sumsq_seg* __restrict__ segs, const float* __restrict__ seg_coeff, int nseg,
                                                            float grad_mul, gct2_loss_scale_state* ls, double* __restrict__ partials) {
#pragma clang fp contract(off)
  const uint64_t c = blockIdx.x;
  int lo = 0, hi = nseg - 1;                       // the last segment whose first partial is <= c (uniform over the work-group)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].first_partial <= c) lo = mid; else hi = mid - 1;
  }
  const uint64_t off = (c - segs[lo].first_partial) * (uint64_t)GCT2_SUMSQ_CHUNK, count = segs[lo].count;
  const uint64_t len = off >= count ? 0 : (count - off < (uint64_t)GCT2_SUMSQ_CHUNK ? count - off : (uint64_t)GCT2_SUMSQ_CHUNK);
  const float* __restrict__ src = g + segs[lo].begin + off;       // 16-byte aligned: begin and the chunk are multiples of 4 elements
  const float k = (ls ? ls->inv_scale : 1.f) * grad_mul;
  float coef = 0.f;
  const float* __restrict__ psrc = nullptr;
  if constexpr (L2) { coef = seg_coeff[lo]; psrc = p + segs[lo].begin + off; }
  const bool reg = L2 && coef != 0.f;              // uniform over the work-group
  const uint32_t n4 = (uint32_t)(len >> 2);
  double acc = 0.0;
  bool bad = false;
#pragma unroll 4
  for (uint32_t i = threadIdx.x; i < n4; i += 256) {
    const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(src) + i);     // read once per step: streaming
    f32x4_t w = {0.f, 0.f, 0.f, 0.f};
    if (reg) w = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(psrc) + i);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      bad |= !(fabsf(v[e]) <= 3.402823466e38f);    // the RAW element: false for inf and nan (ls_check_kernel's test)
      float x32 = v[e] * k;
      if (reg) { const float t = coef * w[e]; x32 = x32 + t; }
      const double x = (double)x32;
      acc = acc + x * x;
    }
  }
  if (threadIdx.x < (uint32_t)(len & 3)) {         // tail (len % 4 elements)
    const float r = src[((size_t)n4 << 2) + threadIdx.x];
    bad |= !(fabsf(r) <= 3.402823466e38f);
    float x32 = r * k;
    if (reg) { const float t = coef * psrc[((size_t)n4 << 2) + threadIdx.x]; x32 = x32 + t; }
    const double x = (double)x32;
    acc = acc + x * x;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc = acc + __shfl_xor(acc, d, 64);
  const bool wave_bad = __any(bad);
  __shared__ double ws[4];
  if ((threadIdx.x & 63) == 0) {
    ws[threadIdx.x >> 6] = acc;
    if (ls && wave_bad) atomicOr(&ls->found_inf, 1);      // the flag gct2_scale_check_finite sets (an integer atomic: order-free)
  }
  __syncthreads();
  if (threadIdx.x == 0) partials[c] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}
// stage two: one work-group; thread s adds the partials of segment s in index order, then thread 0 adds the segments in segment order
__global__ __launch_bounds__(256) void sumsq_final_kernel(const gct2_sumsq_seg* __restrict__ segs, int nseg, const double* __restrict__ partials,
                                                          double* __restrict__ sumsq) {
  __shared__ double seg_sum[GCT2_SUMSQ_MAX_SEGMENTS];
  for (int s = threadIdx.x; s < nseg; s += 256) {
    const uint64_t np = (segs[s].count + GCT2_SUMSQ_CHUNK - 1) / GCT2_SUMSQ_CHUNK;
    const double* __restrict__ src = partials + segs[s].first_partial;
    double acc = 0.0;
    for (uint64_t i = 0; i < np; i++) acc = acc + src[i];
    seg_sum[s] = acc;
    sumsq[s] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int s = 0; s < nseg; s++) acc = acc + seg_sum[s];
    sumsq[nseg] = acc;
  }
}

// the launch-uniform operand of a norm mode, formed once per thread from the ONE fp64 sum of squares the launch reads
__device__ __forceinline__ float clip_operand(int mode, float clip, const double* __restrict__ sumsq) {
#pragma clang fp contract(off)
  if (mode == GCT2_CLIP_NORM) {
    const double ss = *sumsq;
    const float l2 = ss > 0.0 ? (float)sqrt(ss) : 1.f;
    return fmaxf(l2, clip);
  }
  if (mode == GCT2_CLIP_GLOBAL_NORM) {
    const float nrm = (float)sqrt(*sumsq);         // the double square root, rounded once to fp32
    return fabsf(nrm) <= 3.402823466e38f ? clip * fminf(1.f / nrm, 1.f / clip) : __builtin_nanf("");
  }
  return 0.f;
}
// the step between g' and adam_keras_update; `a` is the launch-uniform operand of the mode (clip_operand)
__device__ __forceinline__ float clip_grad(float g, int mode, float clip, float a) {
#pragma clang fp contract(off)
  switch (mode) {
    case GCT2_CLIP_VALUE: return g < -clip ? -clip : (g > clip ? clip : g);      // a NaN fails both comparisons and stays (TF's minimum / maximum)
    case GCT2_CLIP_NORM: { const float t = g * clip; return t / a; }             // tf.clip_by_norm: (g * clip) / max(l2, clip)
    case GCT2_CLIP_GLOBAL_NORM: return g * a;                                    // tf.clip_by_global_norm: g * scale
    default: return g;
  }
}

// ---- Keras SGD / RMSprop over a flat arena [TF] (include/gct2.h gct2_optimizer_apply) ---------------------------------------------
// one element of the kind's update; m / v are touched only where USE_M / KIND say so.  Every product, sum, quotient and root is
// rounded once (no contraction), in the order the header gives
template <int KIND, bool USE_M>
__device__ __forceinline__ void optimizer_update(float& p, float& m, float& v, float g, float lr, float momentum, bool nesterov, float rho,
                                                 float orho, float eps) {
#pragma clang fp contract(off)
  const float step = lr * g;
  if constexpr (KIND == GCT2_OPT_SGD) {
    if constexpr (USE_M) {
      const float a = momentum * m;
      m = a - step;
      if (nesterov) {
        const float b = momentum * m;
        p = p + (b - step);
      } else {
        p = p + m;
      }
    } else {
      p = p - step;
    }
  } else {
    const float v1 = rho * v, g2 = g * g;
    const float v2 = orho * g2;
    v = v1 + v2;
    if constexpr (USE_M) {
      const float a = momentum * m, den = sqrtf(v + eps);
      m = a + step / den;
      p = p - m;
    } else {
      const float den = sqrtf(v) + eps;
      p = p - step / den;
    }
  }
}

// ---- L2 weight regularizer and sign transformer in front of any kind's update (include/gct2.h gct2_optimizer_apply_reg) -----------
// Keras' gradient_transformers=[sign_gradient] (train.py:47-48): tf.sign - a NaN stays NaN, -0 gives +0
__device__ __forceinline__ float sign_grad(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : (x == 0.f ? 0.f : x)); }
// g' -> the gradient the update reads: the penalty gradient fl(l2c * p) added (skipped, not computed, when l2c == 0), clip_grad, then
// the transformer (Keras' _transform_gradients order [TF]); l2c and transform are launch-uniform
__device__ __forceinline__ float reg_grad(float g1, float p, float l2c, int transform, int mode, float clip, float a) {
#pragma clang fp contract(off)
  if (l2c != 0.f) {
    const float t = l2c * p;
    g1 = g1 + t;
  }
  g1 = clip_grad(g1, mode, clip, a);
  return transform == GCT2_GRAD_SIGN ? sign_grad(g1) : g1;
}

// ---- the update of every non-fused step: gct2_adam_keras_clipped, gct2_optimizer_apply and gct2_optimizer_apply_reg -------------
// adam_kernel's geometry (256 threads, f32x4 main loop and a scalar tail, streaming accesses on what is touched once per step, the
// shadow packed two per dword, ls skip and ls->alpha; the gradient comes from g only and is never zeroed) for all three kinds, over
// the slots the kind uses: m only with momentum, v not for SGD - the other pointers are never dereferenced (they may be null).
// GCT2_OPT_ADAM: lr = alpha, momentum = beta1, rho = beta2, both slots in use.  Between g' and the kind's update stands clip_grad, or
// with REG reg_grad (l2c and transform stay launch-uniform run-time switches; without REG neither is read)
template <int KIND, bool USE_M, bool REG, typename S, bool HAS_SHADOW>
__global__ __launch_bounds__(256) void arena_update_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                           const float* __restrict__ g, S* __restrict__ shadow, size_t n, float lr, float momentum,
                                                           int nesterov, float rho, float eps, float grad_mul,
                                                           const gct2_loss_scale_state* __restrict__ ls, int mode, float clip,
                                                           const double* __restrict__ sumsq, float l2c, int transform) {
#pragma clang fp contract(off)
  static_assert(USE_M || KIND != GCT2_OPT_ADAM, "Adam always uses both slots");
  constexpr bool USE_V = KIND != GCT2_OPT_SGD;
  if (ls && ls->found_inf != 0) return;            // a skipped step writes nothing
  const float inv_scale = (ls ? ls->inv_scale : 1.f) * grad_mul;
  if (ls) lr = ls->alpha;
  const float a = clip_operand(mode, clip, sumsq);
  const bool nes = nesterov != 0;
  const float omom = 1.f - momentum, orho = 1.f - rho;       // (Adam: 1 - beta1, 1 - beta2)
  auto grad = [&](float g1, float pp) {
    if constexpr (REG) return reg_grad(g1, pp, l2c, transform, mode, clip, a);
    else return clip_grad(g1, mode, clip, a);
  };
  auto update = [&](float& pp, float& mm, float& vv, float gg) {
    if constexpr (KIND == GCT2_OPT_ADAM) adam_keras_update(pp, mm, vv, gg, lr, momentum, omom, rho, orho, eps);
    else optimizer_update<KIND, USE_M>(pp, mm, vv, gg, lr, momentum, nes, rho, orho, eps);
  };
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4_t gv = reinterpret_cast<const f32x4_t*>(g)[i];
    f32x4_t pv = __builtin_nontemporal_load(reinterpret_cast<f32x4_t*>(p) + i);
    f32x4_t mv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
    if constexpr (USE_M) mv = __builtin_nontemporal_load(reinterpret_cast<f32x4_t*>(m) + i);
    if constexpr (USE_V) vv = __builtin_nontemporal_load(reinterpret_cast<f32x4_t*>(v) + i);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float pp = pv[k], mm = mv[k], v1 = vv[k];
      update(pp, mm, v1, grad(gv[k] * inv_scale, pp));
      pv[k] = pp; mv[k] = mm; vv[k] = v1;
    }
    __builtin_nontemporal_store(pv, reinterpret_cast<f32x4_t*>(p) + i);
    if constexpr (USE_M) __builtin_nontemporal_store(mv, reinterpret_cast<f32x4_t*>(m) + i);
    if constexpr (USE_V) __builtin_nontemporal_store(vv, reinterpret_cast<f32x4_t*>(v) + i);
    if constexpr (HAS_SHADOW) {
      const u32x2_t o = {pack2<S>(pv[0], pv[1]), pack2<S>(pv[2], pv[3])};
      reinterpret_cast<u32x2_t*>(shadow)[i] = o;
    }
  }
  // tail (n % 4 elements)
  const size_t i = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    float pp = p[i], mm = 0.f, vv = 0.f;
    if constexpr (USE_M) mm = m[i];
    if constexpr (USE_V) vv = v[i];
    update(pp, mm, vv, grad(g[i] * inv_scale, pp));
    p[i] = pp;
    if constexpr (USE_M) m[i] = mm;
    if constexpr (USE_V) v[i] = vv;
    if constexpr (HAS_SHADOW) shadow[i] = from_f32<S>(pp);
  }
}
// gct2_l2_penalty: what Keras' train_step reports beside the data term, one thread, fp64 until the last rounding
__global__ void l2_penalty_kernel(const float* __restrict__ loss, const double* __restrict__ S, float l2, float* __restrict__ penalty,
                                  float* __restrict__ total) {
#pragma clang fp contract(off)
  const double r = (double)l2 * *S;
  *penalty = (float)r;
  *total = (float)((double)*loss + r);
}

// gct2_loss_scale_begin_schedule: ls_begin_kernel for either schedule, with or without Adam's bias correction; float32 in Keras' order
__global__ void ls_begin_schedule_kernel(gct2_loss_scale_state* s, int schedule, float initial, float steps, float decay_rate, int staircase,
                                         int bias_correction, float b1, float b2) {
#pragma clang fp contract(off)
  s->found_inf = 0;
  const int k = s->applied_steps;
  float lr;
  if (schedule == GCT2_SCHEDULE_WARMUP) {
    const int warmup_steps = (int)steps;
    lr = k < warmup_steps ? initial * (float)(k + 1) / (float)(warmup_steps + 1) : initial;
  } else {
    float q = (float)k / steps;
    if (staircase) q = floorf(q);
    const float r = decay_rate * q;
    lr = initial / (1.f + r);
  }
  if (bias_correction) {
    const double t = (double)(k + 1);
    s->alpha = (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
  } else {
    s->alpha = lr;
  }
}

}  // namespace

// ---- host launchers (called from capi.hip) ------------------------------------------------------------------
int pw_rng_uniform_int(uint64_t seed, uint64_t stream_id, uint64_t offset, int32_t* out, size_t n, int lo, int hi, hipStream_t s) {
  if (n == 0) return GCT2_OK;
  const uint64_t range = (uint64_t)((int64_t)hi - (int64_t)lo + 1);      // in 64 bits: lo = INT32_MIN, hi = INT32_MAX is 2^32
  hipLaunchKernelGGL(rng_uniform_int_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, seed, stream_id, offset, out, n, lo,
                     range);
  return gct2_check_launch("rng_uniform_int");
}
int pw_rng_normal(uint64_t seed, uint64_t stream_id, uint64_t offset, float* out, size_t n, hipStream_t s) {
  if (n == 0) return GCT2_OK;
  hipLaunchKernelGGL(rng_normal_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, seed, stream_id, offset, out, n);
  return gct2_check_launch("rng_normal");
}
// one launcher per kernel family for both coefficient sources (NoiseFormula: gct2_noise_image / _rng; NoiseTable: the _table forms)
template <typename Src>
static void launch_noise(int dtype, const float* x, const int32_t* t, const float* eps, void* out, int ldout, void* out2, int ldout2, int B,
                         int HW, int C, Src src, hipStream_t s) {
  const size_t npix = (size_t)B * HW;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((noise_kernel<T, Src>), dim3(blocks_for(npix * C, 256)), dim3(256), 0, s, x, t, eps, reinterpret_cast<T*>(out), ldout,
                       reinterpret_cast<T*>(out2), ldout2, npix, HW, C, src);
  });
}
template <typename Src>
static void launch_noise_rng(int dtype, const float* x, const int32_t* t, uint64_t seed, uint64_t sid, uint64_t off, float* eps_out,
                             void* out, int ldout, void* out2, int ldout2, int B, int HW, int C, Src src, hipStream_t s) {
  const size_t npix = (size_t)B * HW;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if constexpr (sizeof(T) == 2) {
      // the train step's call: 3 channels into the packed 4-slot image and nothing else, whole groups of four pixels / three counters
      if (C == 3 && ldout == 4 && !out2 && !eps_out && off % 12 == 0 && npix % 4 == 0 && HW % 4 == 0 && (uintptr_t)x % 16 == 0 &&
          (uintptr_t)out % 16 == 0) {
        hipLaunchKernelGGL((noise_rng_px4_kernel<T, Src>), dim3(blocks_for(npix / 4, 256)), dim3(256), 0, s, x, t, seed, sid, off >> 2,
                           reinterpret_cast<T*>(out), npix / 4, HW, src);
        return;
      }
    }
    hipLaunchKernelGGL((noise_rng_kernel<T, Src>), dim3(blocks_for(npix * C / 4 + 2, 256)), dim3(256), 0, s, x, t, seed, sid, off, eps_out,
                       reinterpret_cast<T*>(out), ldout, reinterpret_cast<T*>(out2), ldout2, npix * C, HW, C, src);
  });
}
int pw_noise(int dtype, const float* x, const int32_t* t, const float* eps, void* out, int ldout, void* out2, int ldout2, int B, int HW,
             int C, int steps, hipStream_t s) {
  launch_noise(dtype, x, t, eps, out, ldout, out2, ldout2, B, HW, C, NoiseFormula{steps + 1}, s);
  return gct2_check_launch("noise_image");
}
int pw_noise_rng(int dtype, const float* x, const int32_t* t, uint64_t seed, uint64_t sid, uint64_t off, float* eps_out, void* out,
                 int ldout, void* out2, int ldout2, int B, int HW, int C, int steps, hipStream_t s) {
  launch_noise_rng(dtype, x, t, seed, sid, off, eps_out, out, ldout, out2, ldout2, B, HW, C, NoiseFormula{steps + 1}, s);
  return gct2_check_launch("noise_image_rng");
}
int pw_noise_table(int dtype, const float* x, const int32_t* t, const float* eps, const float* coef, void* out, int ldout, void* out2,
                   int ldout2, int B, int HW, int C, int steps, hipStream_t s) {
  launch_noise(dtype, x, t, eps, out, ldout, out2, ldout2, B, HW, C, NoiseTable{coef, steps}, s);
  return gct2_check_launch("noise_image_table");
}
int pw_noise_rng_table(int dtype, const float* x, const int32_t* t, uint64_t seed, uint64_t sid, uint64_t off, float* eps_out,
                       const float* coef, void* out, int ldout, void* out2, int ldout2, int B, int HW, int C, int steps, hipStream_t s) {
  launch_noise_rng(dtype, x, t, seed, sid, off, eps_out, out, ldout, out2, ldout2, B, HW, C, NoiseTable{coef, steps}, s);
  return gct2_check_launch("noise_image_rng_table");
}
int pw_dense_fwd(int dtype, const void* x, int ldx, const float* w, const float* b, float* y, int M, int Cin, int Cout, hipStream_t s) {
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(dense_fwd_kernel<T>, dim3(blocks_for(M, 256)), dim3(256), Cin * 4 * sizeof(float), s, reinterpret_cast<const T*>(x),
                       ldx, w, b, y, M, Cin, Cout);
  });
  return gct2_check_launch("dense_fwd");
}
int pw_dense_bwd(int dtype, const void* x, int ldx, const float* w, const float* dy, void* dx, int lddx, float* dw, float* db, int M,
                 int Cin, int Cout, int Cmask, int accumulate, hipStream_t s) {
  constexpr int PIX = 128;
  if (!accumulate) {            // the kernel adds its per-work-group sums with atomics
    (void)hipMemsetAsync(dw, 0, (size_t)Cin * Cout * sizeof(float), s);
    if (db) (void)hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), s);
  }
  const int ntiles = (M + PIX - 1) / PIX;
  const int grid = ntiles < 1024 ? ntiles : 1024;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const size_t lds = (size_t)Cin * 16 + PIX * 16 + (size_t)PIX * Cin * sizeof(T);
    auto kern = dense_bwd_kernel<T, PIX>;
    if (lds > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, reinterpret_cast<const T*>(x), ldx, w, dy, reinterpret_cast<T*>(dx), lddx, dw,
                       db, M, Cin, Cout, Cmask);
  });
  return gct2_check_launch("dense_bwd");
}
// per-timestep heads.  Pixel tile of the backward kernel and the number of work-groups (= partial rows) per image: every tile its
// own work-group until the grid passes ~2048 work-groups (8 per CU), then a work-group walks several tiles of its image
constexpr int STEPS_PIX = 128;
static int dense_steps_chunks(int B, int HW) {
  const int ntiles = (HW + STEPS_PIX - 1) / STEPS_PIX;
  return std::min(ntiles, std::max(1, kMaxBlocks / B));
}
size_t dense_steps_scratch_floats(int B, int HW, int Cin, int Cout) {
  return ((size_t)B * dense_steps_chunks(B, HW) * (size_t)((Cin + 1) * Cout) + 3) / 4 * 4;
}
int pw_dense_steps_fwd(int dtype, const void* x, int ldx, const float* w, const float* b, const int32_t* t_int, float* y, int B, int HW,
                       int Cin, int Cout, int steps, hipStream_t s) {
  const int gx = std::min((HW + 255) / 256, std::max(1, kMaxBlocks / B));
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(dense_steps_fwd_kernel<T>, dim3(gx, B), dim3(256), Cin * 4 * sizeof(float), s, reinterpret_cast<const T*>(x), ldx, w,
                       b, t_int, y, HW, Cin, Cout, steps);
  });
  return gct2_check_launch("dense_steps_fwd");
}
int pw_dense_steps_bwd(int dtype, const void* x, int ldx, const float* w, const int32_t* t_int, const float* dy, void* dx, int lddx,
                       float* dw, float* db, float* scratch, int B, int HW, int Cin, int Cout, int steps, int Cmask, int accumulate,
                       hipStream_t s) {
  constexpr int PIX = STEPS_PIX;
  const int nchunk = dense_steps_chunks(B, HW);
  const int nout = (Cin + 1) * Cout;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const size_t lds = (size_t)Cin * 16 + PIX * 16 + (size_t)PIX * Cin * sizeof(T);
    auto kern = dense_steps_bwd_kernel<T, PIX>;
    if (lds > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(nchunk, B), dim3(256), lds, s, reinterpret_cast<const T*>(x), ldx, w, t_int, dy, reinterpret_cast<T*>(dx),
                       lddx, scratch, HW, Cin, Cout, steps, Cmask);
  });
  hipLaunchKernelGGL(dense_steps_finish_kernel, dim3((nout + 255) / 256, steps), dim3(256), 0, s, scratch, t_int, dw, db, B, nchunk, Cin, Cout,
                     steps, accumulate);
  return gct2_check_launch("dense_steps_bwd");
}
// the ordered finish of the head's partial rows, also used by the UpShuffle_0 forward that carries the head in its epilogue
int pw_head_finish(const float* part, int rows, float* dw, float* db, float* loss, float* db_dx, int ndw, int Cout, float inv_n,
                   int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(dense_head_finish_kernel, dim3(HEAD_ROW / 32), dim3(1024), 0, s, part, rows, dw, db, loss, db_dx, ndw, Cout, inv_n,
                     accumulate);
  return gct2_check_launch("dense_head_finish");
}

int pw_dense_head_train(const gct2_ctx& c, int dtype, const void* x, int ld, const float* w, const float* b, const float* target, float* pred,
                        void* dx, int lddx, float* dw, float* db, float* loss, float* partials, int M, int Cin, int Cout, int Cmask,
                        const float* ls, float* db_dx, const void* x2, int ldx2, int accumulate, hipStream_t s) {
  const size_t ws_bytes = c.ws_bytes;
  float* ws = c.ws;
  return with_dtype16(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    // matrix-core version: the reference head (64 masked U_0 channels + 3 image channels -> 3 outputs) with a workspace in the ctx
    if (Cmask == 64 && Cin >= 64 && Cin <= (x2 ? 68 : 72) && (x2 || ld >= 72) && Cout <= 3) {
      const int ngroups = (M + 15) / 16;
      const int grid = std::min(512, (ngroups + 3) / 4);
      if (ws && ws_bytes >= (size_t)grid * HEAD_ROW * sizeof(float)) {
        hipLaunchKernelGGL(dense_head_mfma_kernel<T>, dim3(grid), dim3(256), 0, s, reinterpret_cast<const T*>(x), ld, w, b, target, pred,
                           reinterpret_cast<T*>(dx), lddx, ws, M, Cin, Cout, ls, reinterpret_cast<const T*>(x2), ldx2);
        hipLaunchKernelGGL(dense_head_finish_kernel, dim3(HEAD_ROW / 32), dim3(1024), 0, s, ws, grid, dw, db, loss, db_dx, Cin * Cout, Cout,
                           1.0f / ((float)M * (float)Cout), accumulate);
        return gct2_check_launch("dense_head_train");
      }
    }
    if (x2) return gct2_fail(GCT2_EINVAL, "dense_head_train: a split input (x2) needs the matrix-core version: Cmask = 64, Cin <= 68, "
                                          "Cout <= 3 and a registered workspace");
    if (!accumulate) {            // the LDS-tile kernel adds its per-work-group sums with atomics
      (void)hipMemsetAsync(dw, 0, (size_t)Cin * Cout * sizeof(float), s);
      if (db) (void)hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), s);
      if (db_dx) (void)hipMemsetAsync(db_dx, 0, (size_t)Cmask * sizeof(float), s);
    }
    constexpr int PIX = 256;
    const size_t lds = (size_t)PIX * ld * 2 + (size_t)PIX * Cmask * 2 + PIX * 16 + (size_t)ld * 16;
    const int ntiles = (M + PIX - 1) / PIX;
    const int grid = ntiles < 1024 ? ntiles : 1024;
    auto kern = dense_head_train_kernel<T, PIX>;
    static size_t attr_lds = 0;
    if (lds > attr_lds) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      attr_lds = lds;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, reinterpret_cast<const T*>(x), ld, w, b, target, pred, reinterpret_cast<T*>(dx),
                       lddx, dw, db, partials, M, Cin, Cout, Cmask, ls, db_dx);
    hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(256), 0, s, partials, grid, loss, 1.0f / ((float)M * (float)Cout));
    return gct2_check_launch("dense_head_train");
  });
}
int pw_noise_edits(const float* eps, const float* dict, int K, float* out, int H, int W, int C, hipStream_t s) {
  hipLaunchKernelGGL(noise_edits_kernel, dim3((H * W + 255) / 256), dim3(256), 0, s, eps, dict, K, out, H, W, C);
  return gct2_check_launch("noise_edits");
}
int pw_image_prepare(const uint8_t* src, const int64_t* offsets, const int32_t* dims, float* dst, int B, int size, hipStream_t s) {
  hipLaunchKernelGGL(image_prepare_kernel, dim3(blocks_for((size_t)B * size * size * 3, 256)), dim3(256), 0, s, src, offsets, dims, dst, B, size);
  return gct2_check_launch("image_prepare");
}
int pw_mse(const float* pred, const float* target, float* dpred, float* loss, float* partials, size_t n, const float* ls, hipStream_t s) {
  const int nb = blocks_for(n, 1024) > 1024 ? 1024 : blocks_for(n, 1024);
  hipLaunchKernelGGL(mse_kernel, dim3(nb), dim3(256), 0, s, pred, target, dpred, partials, n, ls);
  hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(256), 0, s, partials, nb, loss, 1.0f / (float)n);
  return gct2_check_launch("mse_fwd_bwd");
}
int pw_relu_mask(int dtype, const void* act, int ldact, void* d, int ldd, size_t npix, int C, hipStream_t s) {
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(relu_mask_kernel<T>, dim3(blocks_for(npix * C, 256)), dim3(256), 0, s, reinterpret_cast<const T*>(act), ldact,
                       reinterpret_cast<T*>(d), ldd, npix * C, C);
  });
  return gct2_check_launch("relu_mask");
}
int pw_add(int dtype, void* dst, int lddst, const void* src, int ldsrc, size_t npix, int C, hipStream_t s) {
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(add_kernel<T>, dim3(blocks_for(npix * C, 256)), dim3(256), 0, s, reinterpret_cast<T*>(dst), lddst,
                       reinterpret_cast<const T*>(src), ldsrc, npix * C, C);
  });
  return gct2_check_launch("add");
}
int pw_mix_per_image(const float* x, const float* eps, const float* a, const float* c, float* out, int B, size_t per_image, hipStream_t s) {
  const size_t n = (size_t)B * per_image;
  hipLaunchKernelGGL(mix_per_image_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, x, eps, a, c, out, n, per_image);
  return gct2_check_launch("mix_per_image");
}
int pw_colsum(int dtype, const void* dz, int ld, float* db, size_t M, int C, float sign, hipStream_t s) {
  const int ctiles = (C + 63) / 64;
  int rblocks = (int)((M + 511) / 512);
  const int cap = (1024 + ctiles - 1) / ctiles;
  if (rblocks > cap) rblocks = cap;
  if (rblocks < 1) rblocks = 1;
  const int rows_per_block = (int)((M + rblocks - 1) / rblocks);
  const dim3 grid(ctiles, rblocks);
  return with_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    const T* src = reinterpret_cast<const T*>(dz);
    if constexpr (sizeof(T) == 2) {
      if (C % 8 == 0 && ld % 8 == 0 && (uintptr_t)dz % 16 == 0) {
        hipLaunchKernelGGL(colsum_vec_kernel<T>, grid, dim3(256), 0, s, src, ld, db, M, C, rows_per_block, sign);
        return gct2_check_launch("colsum_vec");
      }
    }
    hipLaunchKernelGGL(colsum_kernel<T>, grid, dim3(256), 0, s, src, ld, db, M, C, rows_per_block, sign);
    return gct2_check_launch("colsum");
  });
}
int pw_adam(float* p, float* m, float* v, float* g, void* shadow, int sdt, size_t n, float alpha, float b1, float b2, float eps,
            float grad_mul, const gct2_loss_scale_state* ls, int zero_grad, hipStream_t s, const float* slabs, int nslab, size_t slab_stride,
            size_t n_slab) {
  if (n == 0) return GCT2_OK;
  const int nb = blocks_for(n / 4 + 4, 256);
#define GCT2_ADAM(S, HS) hipLaunchKernelGGL((adam_kernel<S, HS>), dim3(nb), dim3(256), 0, s, p, m, v, g, reinterpret_cast<S*>(shadow), n, alpha, b1, b2, eps, grad_mul, ls, zero_grad, slabs, nslab, slab_stride, n_slab)
  if (!shadow) GCT2_ADAM(float, false);
  else if (sdt == GCT2_BF16) GCT2_ADAM(__bf16, true);
  else if (sdt == GCT2_F16) GCT2_ADAM(_Float16, true);
  else GCT2_ADAM(float, true);
#undef GCT2_ADAM
  return gct2_check_launch("adam_keras_multi");
}
int pw_ema(float* ema, const float* p, void* shadow, int sdt, size_t n, float momentum, float one_minus, const gct2_loss_scale_state* ls,
           hipStream_t s) {
  if (n == 0) return GCT2_OK;
  const int nb = blocks_for(n / 4 + 4, 256);
  with_shadow16(shadow, sdt, [&](auto tag, auto has_shadow) {
    using S = typename decltype(tag)::type;
    hipLaunchKernelGGL((ema_kernel<S, decltype(has_shadow)::value>), dim3(nb), dim3(256), 0, s, ema, p, reinterpret_cast<S*>(shadow), n, momentum,
                       one_minus, ls);
  });
  return gct2_check_launch("ema_update");
}
int pw_grad_sumsq(const float* g, const gct2_sumsq_seg* segs, int nseg, size_t npartials, float grad_mul, gct2_loss_scale_state* ls,
                  double* partials, double* sumsq, hipStream_t s) {
  hipLaunchKernelGGL(sumsq_partial_kernel<false>, dim3((unsigned)npartials), dim3(256), 0, s, g, (const float*)nullptr, segs, (const float*)nullptr,
                     nseg, grad_mul, ls, partials);
  if (int e = gct2_check_launch("grad_sumsq")) return e;
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, s, segs, nseg, partials, sumsq);
  return gct2_check_launch("grad_sumsq");
}
int pw_grad_sumsq_l2(const float* g, const float* p, const gct2_sumsq_seg* segs, const float* seg_coeff, int nseg, size_t npartials,
                     float grad_mul, gct2_loss_scale_state* ls, double* partials, double* sumsq, hipStream_t s) {
  hipLaunchKernelGGL(sumsq_partial_kernel<true>, dim3((unsigned)npartials), dim3(256), 0, s, g, p, segs, seg_coeff, nseg, grad_mul, ls, partials);
  if (int e = gct2_check_launch("grad_sumsq_l2")) return e;
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, s, segs, nseg, partials, sumsq);
  return gct2_check_launch("grad_sumsq_l2");
}
int pw_l2_penalty(const float* loss, const double* S, float l2, float* penalty, float* total, hipStream_t s) {
  hipLaunchKernelGGL(l2_penalty_kernel, dim3(1), dim3(1), 0, s, loss, S, l2, penalty, total);
  return gct2_check_launch("l2_penalty");
}
int pw_update(const char* what, bool reg, int kind, float* p, float* m, float* v, const float* g, void* shadow, int sdt, size_t n, float lr,
              float momentum, int nesterov, float rho, float eps, float grad_mul, const gct2_loss_scale_state* ls, int mode, float clip,
              const double* sumsq, float l2c, int transform, hipStream_t s) {
  const int nb = blocks_for(n / 4 + 4, 256);
  auto launch = [&](auto kind_c, auto use_m, auto reg_c) {
    with_shadow16(shadow, sdt, [&](auto tag, auto has_shadow) {
      using S = typename decltype(tag)::type;
      hipLaunchKernelGGL((arena_update_kernel<decltype(kind_c)::value, decltype(use_m)::value, decltype(reg_c)::value, S, decltype(has_shadow)::value>),
                         dim3(nb), dim3(256), 0, s, p, m, v, g, reinterpret_cast<S*>(shadow), n, lr, momentum, nesterov, rho, eps, grad_mul, ls,
                         mode, clip, sumsq, l2c, transform);
    });
  };
  auto with_reg = [&](auto kind_c, auto use_m) {
    if (reg) launch(kind_c, use_m, std::true_type{}); else launch(kind_c, use_m, std::false_type{});
  };
  auto with_momentum = [&](auto kind_c) {
    if (momentum > 0.f) with_reg(kind_c, std::true_type{}); else with_reg(kind_c, std::false_type{});
  };
  if (kind == GCT2_OPT_ADAM) with_reg(std::integral_constant<int, GCT2_OPT_ADAM>{}, std::true_type{});      // (momentum carries beta1)
  else if (kind == GCT2_OPT_SGD) with_momentum(std::integral_constant<int, GCT2_OPT_SGD>{});
  else with_momentum(std::integral_constant<int, GCT2_OPT_RMSPROP>{});
  return gct2_check_launch(what);
}
int pw_cast(int dtype, const float* src, void* dst, size_t n, hipStream_t s) {
  if (n == 0) return GCT2_OK;
  const int nb = blocks_for(n, 256);
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(cast_kernel<T>, dim3(nb), dim3(256), 0, s, src, reinterpret_cast<T*>(dst), n);
  });
  return gct2_check_launch("cast_from_f32");
}
int pw_ls_init(gct2_loss_scale_state* st, float scale, hipStream_t s) {
  hipLaunchKernelGGL(ls_init_kernel, dim3(1), dim3(1), 0, s, st, scale);
  return gct2_check_launch("loss_scale_init");
}
int pw_ls_begin(gct2_loss_scale_state* st, float base_lr, int warmup_steps, float b1, float b2, hipStream_t s) {
  hipLaunchKernelGGL(ls_begin_kernel, dim3(1), dim3(1), 0, s, st, base_lr, warmup_steps, b1, b2);
  return gct2_check_launch("loss_scale_begin");
}
int pw_ls_begin_schedule(gct2_loss_scale_state* st, int schedule, float initial, float steps, float decay_rate, int staircase, int bias_correction,
                         float b1, float b2, hipStream_t s) {
  hipLaunchKernelGGL(ls_begin_schedule_kernel, dim3(1), dim3(1), 0, s, st, schedule, initial, steps, decay_rate, staircase, bias_correction, b1, b2);
  return gct2_check_launch("loss_scale_begin_schedule");
}
int pw_ls_check(const float* g, size_t n, gct2_loss_scale_state* st, hipStream_t s) {
  if (n == 0) return GCT2_OK;
  hipLaunchKernelGGL(ls_check_kernel, dim3(blocks_for(n, 1024)), dim3(256), 0, s, g, n, st);
  return gct2_check_launch("scale_check_finite");
}
int pw_ls_update(gct2_loss_scale_state* st, int growth_interval, hipStream_t s) {
  hipLaunchKernelGGL(ls_update_kernel, dim3(1), dim3(1), 0, s, st, growth_interval);
  return gct2_check_launch("loss_scale_update");
}

// ---- ReLU bit plane derived from a stored activation tensor (fall-back of gct2_ctx_set_relu_bits: launches whose epilogue cannot
// write the plane - 8-byte epilogues, split-K finalize, the direct kernels): bit k of bits[pixel][c] = (y[pixel][8c + k] > 0)
namespace {
template <typename T>
__global__ void relu_bits_kernel(const T* __restrict__ y, int ldy, size_t pixels, int groups, unsigned char* __restrict__ bits, int ldbits) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pixels * (size_t)groups) return;
  const size_t pix = i / groups;
  const int gidx = (int)(i - pix * groups);
  const T* src = y + pix * ldy + 8 * gidx;
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) m |= ((float)src[k] > 0.f ? 1u : 0u) << k;
  bits[pix * ldbits + gidx] = (unsigned char)m;
}
}  // namespace
int pw_relu_bits(int dtype, const void* y, int ldy, size_t pixels, int channels, unsigned char* bits, int ldbits, hipStream_t s) {
  const int groups = channels / 8;
  const size_t n = pixels * (size_t)groups;
  if (!n) return GCT2_OK;
  const dim3 grid((unsigned)((n + 255) / 256));
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(relu_bits_kernel<T>, grid, dim3(256), 0, s, (const T*)y, ldy, pixels, groups, bits, ldbits);
  });
  return gct2_check_launch("relu_bits");
}

// gct2_stream_occupy: hold `workgroups` work-group slots for `ticks` of the constant 100-MHz counter.  Every wave watches its own
// clock, so every wave reaches the exit whatever the others do.
namespace {
__global__ __launch_bounds__(256) void occupy_kernel(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
}  // namespace
int pw_occupy(int workgroups, unsigned long long ticks, hipStream_t s) {
  hipLaunchKernelGGL(occupy_kernel, dim3(workgroups), dim3(256), 0, s, ticks);
  return gct2_check_launch("stream_occupy");
}
