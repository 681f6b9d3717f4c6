// The hidden Dense(pixel_size, relu) layer in front of the Dense(3) head (train.py:195-197, commented out in the reference) as ONE
// kernel per direction: gct2_dense2_fwd / gct2_dense2_bwd (include/gct2.h).  Per pixel m
//   h[j] = round_T(relu(b1[j] + sum_i x[m,i] w1[i,j])),   y[m,o] = b2[o] + sum_j h[j] w2[j,o]
// and h - [M, Chid], the largest tensor the network would have - is never stored: the backward kernels recompute it from x.
//   dh[j] = round_T((h[j] > 0) * sum_o dy[m,o] w2[j,o]);  dw2 = h^T dy;  db2 = sum dy;  dw1 = x^T dh;  db1 = sum dh;
//   dx[m,i] = (x[m,i] > 0) * sum_j dh[j] w1[i,j]
// Two versions of each direction:
//   plain - every dtype, Cin / Chid <= D2_PLAIN_MAX; scalar arithmetic on LDS tiles.  The reference the fast one is tested against.
//   mfma  - 16-bit dtypes, Chid in {32, 64, 128}, Cin <= 80, rows of x 16-byte aligned (ldx % 8 == 0): layer 1, dh w1^T and x^T dh on
//           v_mfma_f32_16x16x32; the 3-output product and dh are VALU work on the accumulator layout (lane l holds pixels
//           4 (l >> 4) + r, hidden unit 16 nt + (l & 15)) with one 16-lane row sum per pixel.
// No atomics: a backward work-group leaves ONE partial row [dw1 | db1 | dw2 | db2] in caller scratch and dense2_finish_kernel adds the
// rows in ascending work-group order.
#include "gct2_common.h"

namespace {

constexpr int D2_CAP = 512;          // most work-groups (= partial rows) of a backward launch
constexpr int D2_FAST_PIX = GCT2_DENSE2_FAST_PIXELS;      // pixels per work-group tile of the mfma kernels: four waves x 16
constexpr int D2_PLAIN_PIX = 16;     // pixels per work-group tile of the plain backward kernel
constexpr int D2_PLAIN_MAX = GCT2_DENSE2_PLAIN_MAX;    // largest Cin / Chid of the plain kernels (their LDS tiles: 16 x (Cin + 2 Chid + 4) floats)
constexpr int D2_KP = 96;            // mfma: layer 1's reduction length in the LDS image (Cin <= 80, zero-padded to 32 k)
constexpr int D2_W1T_LD = D2_KP + 8; // ... and its row pitch in elements (+16 bytes: rows 16 apart do not share banks)
constexpr int D2_CROWS = 80;         // mfma: rows of the channel-major images (Cin <= 80 = five 16-row tiles)
constexpr int D2_PIX_LD = D2_FAST_PIX + 8;   // mfma: row pitch of the [channel][pixel] / [hidden][pixel] images

template <typename T> __device__ __forceinline__ float round_T(float v) { return to_f32<T>(from_f32<T>(v)); }
// the plain kernels' accumulator of the two sums whose result is rounded to T: fp32 for the 16-bit dtypes (its error is far below their
// unit in the last place), fp64 for fp32 - h and dh are then the correctly rounded fp32 values, within one unit in the last place of
// any exact evaluation, which an fp32 sum of Cin products is not when the terms cancel
template <typename T> struct PlainAcc { using type = float; };
template <> struct PlainAcc<float> { using type = double; };

inline int row_floats(int Cin, int Chid, int Cout) { return (Cin * Chid + Chid + Chid * Cout + Cout + 3) / 4 * 4; }
inline int groups(int M, int pix) {
  const long long t = ((long long)M + pix - 1) / pix;
  return (int)(t < D2_CAP ? t : D2_CAP);
}

// ---- plain ---------------------------------------------------------------------------------------------------------------------
// one thread per pixel; the pixel's channels wait in LDS as fp32; i and j ascending, one fma per term, biases last
template <typename T>
__global__ __launch_bounds__(64) void dense2_plain_fwd_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ w1,
                                                              const float* __restrict__ b1, const float* __restrict__ w2,
                                                              const float* __restrict__ b2, float* __restrict__ y, int M, int Cin,
                                                              int Chid, int Cout) {
  extern __shared__ float xs[];                    // [64][Cin + 1]
  const int tid = threadIdx.x, ld = Cin + 1;
  const long long ntiles = ((long long)M + 63) / 64;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long mbase = tile * 64;
    __syncthreads();
    for (int i = tid; i < 64 * Cin; i += 64) {
      const int pm = i / Cin, k = i - pm * Cin;
      xs[pm * ld + k] = (mbase + pm < M) ? to_f32(x[(size_t)(mbase + pm) * ldx + k]) : 0.f;
    }
    __syncthreads();
    const float* xr = xs + tid * ld;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < Chid; j++) {
      typename PlainAcc<T>::type pre = 0;
      for (int i = 0; i < Cin; i++) pre = fma((typename PlainAcc<T>::type)xr[i], (typename PlainAcc<T>::type)to_f32(w1[i * Chid + j]), pre);
      const float v = (float)(pre + b1[j]);
      const float h = round_T<T>(v > 0.f ? v : 0.f);
#pragma unroll
      for (int o = 0; o < 4; o++)
        if (o < Cout) a[o] = fmaf(h, w2[j * Cout + o], a[o]);
    }
    const long long m = mbase + tid;
    if (m < M) {
#pragma unroll
      for (int o = 0; o < 4; o++)
        if (o < Cout) y[(size_t)m * Cout + o] = keras_f16_point<T>(a[o] + b2[o]);
    }
  }
}

// work-group g walks the tiles g, g + gridDim.x, ... of D2_PLAIN_PIX pixels and keeps its running sums in ITS row of `part` (entry e
// belongs to thread e % 256 for the whole launch: plain loads and stores, no atomics)
template <typename T>
__global__ __launch_bounds__(256) void dense2_plain_bwd_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ w1,
                                                               const float* __restrict__ b1, const float* __restrict__ w2,
                                                               const float* __restrict__ dy, T* __restrict__ dx, int lddx, float* part,
                                                               int rowf, int M, int Cin, int Chid, int Cout, int Cmask) {
  constexpr int PIX = D2_PLAIN_PIX;
  extern __shared__ float sm[];
  float* xs = sm;                                  // [PIX][Cin]
  float* hs = xs + PIX * Cin;                      // [PIX][Chid]
  float* dhs = hs + PIX * Chid;                    // [PIX][Chid]
  float* dys = dhs + PIX * Chid;                   // [PIX][4]
  float* row = part + (size_t)blockIdx.x * rowf;
  const int tid = threadIdx.x;
  const int n1 = Cin * Chid, n2 = Chid * Cout, total = n1 + Chid + n2 + Cout;
  const long long ntiles = ((long long)M + PIX - 1) / PIX;
  bool first = true;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long mbase = tile * PIX;
    __syncthreads();
    for (int i = tid; i < PIX * Cin; i += 256) {
      const int pm = i / Cin, k = i - pm * Cin;
      xs[i] = (mbase + pm < M) ? to_f32(x[(size_t)(mbase + pm) * ldx + k]) : 0.f;
    }
    for (int i = tid; i < PIX * 4; i += 256) {
      const int pm = i >> 2, o = i & 3;
      dys[i] = (o < Cout && mbase + pm < M) ? keras_f16_point<T>(dy[(size_t)(mbase + pm) * Cout + o]) : 0.f;
    }
    __syncthreads();
    for (int it = tid; it < PIX * Chid; it += 256) {
      const int pm = it / Chid, j = it - pm * Chid;
      typename PlainAcc<T>::type pre = 0, g = 0;
      for (int i = 0; i < Cin; i++) pre = fma((typename PlainAcc<T>::type)xs[pm * Cin + i], (typename PlainAcc<T>::type)to_f32(w1[i * Chid + j]), pre);
      const float v = (float)(pre + b1[j]);
      const float h = round_T<T>(v > 0.f ? v : 0.f);
      for (int o = 0; o < Cout; o++) g = fma((typename PlainAcc<T>::type)dys[4 * pm + o], (typename PlainAcc<T>::type)w2[j * Cout + o], g);
      hs[it] = h;
      dhs[it] = h > 0.f ? round_T<T>((float)g) : 0.f;     // (a pixel beyond M has dy = 0, hence dh = 0)
    }
    __syncthreads();
    if (dx) {
      for (int it = tid; it < PIX * Cmask; it += 256) {
        const int pm = it / Cmask, i = it - pm * Cmask;
        if (mbase + pm >= M) continue;
        float g = 0.f;
        for (int j = 0; j < Chid; j++) g = fmaf(dhs[pm * Chid + j], to_f32(w1[i * Chid + j]), g);
        if (!(xs[pm * Cin + i] > 0.f)) g = 0.f;
        dx[(size_t)(mbase + pm) * lddx + i] = from_f32<T>(g);
      }
    }
    for (int e = tid; e < total; e += 256) {
      float a = first ? 0.f : row[e];
      if (e < n1) {
        const int i = e / Chid, j = e - i * Chid;
        for (int pm = 0; pm < PIX; pm++) a = fmaf(xs[pm * Cin + i], dhs[pm * Chid + j], a);
      } else if (e < n1 + Chid) {
        const int j = e - n1;
        for (int pm = 0; pm < PIX; pm++) a += dhs[pm * Chid + j];
      } else if (e < n1 + Chid + n2) {
        const int q = e - n1 - Chid, j = q / Cout, o = q - j * Cout;
        for (int pm = 0; pm < PIX; pm++) a = fmaf(hs[pm * Chid + j], dys[4 * pm + o], a);
      } else {
        const int o = e - n1 - Chid - n2;
        for (int pm = 0; pm < PIX; pm++) a += dys[4 * pm + o];
      }
      row[e] = a;
    }
    first = false;
  }
}

// entry e of [dw1 | db1 | dw2 | db2] = the partial rows in ascending work-group order, one thread per entry
__global__ __launch_bounds__(256) void dense2_finish_kernel(const float* __restrict__ part, int rows, int rowf, float* __restrict__ dw1,
                                                            float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2,
                                                            int n1, int Chid, int n2, int Cout, int accumulate) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n1 + Chid + n2 + Cout) return;
  float acc = 0.f;
  for (int r = 0; r < rows; r++) acc += part[(size_t)r * rowf + e];
  float* dst = e < n1 ? dw1 + e : e < n1 + Chid ? db1 + (e - n1) : e < n1 + Chid + n2 ? dw2 + (e - n1 - Chid) : db2 + (e - n1 - Chid - n2);
  *dst = accumulate ? *dst + acc : acc;
}

// ---- mfma ----------------------------------------------------------------------------------------------------------------------
// eight channels [8 c, 8 c + 8) of pixel m as one A fragment: channels >= Cin (the pad channels of the row, which may hold NaN, and the
// zero padding of the reduction up to 32 k) and pixels >= M are ZERO in the register image; only 16-byte chunks that start below Cin are
// read, and those end inside the row because ldx % 8 == 0
template <typename T>
__device__ __forceinline__ u32x4_t d2_x_frag(const T* __restrict__ x, int ldx, long long m, int M, int Cin, int c) {
  u32x4_t v = {0u, 0u, 0u, 0u};
  const int ch = 8 * c;
  if (m < M && ch < Cin) {
    v = gload128(x + (size_t)m * ldx + ch);
    const int valid = Cin - ch;
    if (valid < 8) {
#pragma unroll
      for (int q = 0; q < 4; q++) v[q] &= (2 * q < valid ? 0x0000ffffu : 0u) | (2 * q + 1 < valid ? 0xffff0000u : 0u);
    }
  }
  return v;
}
// w1 (Cin, Chid) -> the [Chid][D2_KP] image layer 1 reads its B fragments from (reduction index contiguous, zeros behind Cin)
template <typename T> __device__ __forceinline__ void d2_stage_w1t(T* w1t, const T* __restrict__ w1, int Cin, int Chid, int tid) {
  for (int idx = tid; idx < D2_KP * Chid; idx += 256) {
    const int i = idx / Chid, j = idx - i * Chid;
    w1t[j * D2_W1T_LD + i] = i < Cin ? w1[i * Chid + j] : from_f32<T>(0.f);
  }
}
// pre-activations of 16 pixels x Chid hidden units: acc[nt][r] = sum_i x[pixel 4 g + r][i] w1[i][16 nt + (lane & 15)]
template <typename T, int NT>
__device__ __forceinline__ void d2_layer1(const char* w1t, const u32x4_t (&a)[3], int ksteps, int lane, f32x4_t (&acc)[NT]) {
#pragma unroll
  for (int nt = 0; nt < NT; nt++) acc[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < 3; kk++) {
    if (kk < ksteps) {
#pragma unroll
      for (int nt = 0; nt < NT; nt++) {
        const u32x4_t b = lds_read128(w1t, ((nt * 16 + (lane & 15)) * D2_W1T_LD + 32 * kk + 8 * (lane >> 4)) * 2);
        acc[nt] = mfma16<T>(a[kk], b, acc[nt]);
      }
    }
  }
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void dense2_mfma_fwd_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ w1,
                                                              const float* __restrict__ b1, const float* __restrict__ w2,
                                                              const float* __restrict__ b2, float* __restrict__ y, int M, int Cin,
                                                              int Cout) {
  constexpr int Chid = NT * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* w1t = reinterpret_cast<T*>(smem);                                        // [Chid][D2_W1T_LD]
  float* w2s = reinterpret_cast<float*>(smem + Chid * D2_W1T_LD * 2);        // [Chid][4]
  float* b1s = w2s + Chid * 4;                                                // [Chid]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
  d2_stage_w1t<T>(w1t, w1, Cin, Chid, tid);
  for (int i = tid; i < Chid * 4; i += 256) w2s[i] = (i & 3) < Cout ? w2[(i >> 2) * Cout + (i & 3)] : 0.f;
  for (int i = tid; i < Chid; i += 256) b1s[i] = b1[i];
  __syncthreads();
  const int ksteps = (Cin + 31) / 32;
  const long long ntiles = ((long long)M + D2_FAST_PIX - 1) / D2_FAST_PIX;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long m0 = tile * D2_FAST_PIX + wave * 16;
    u32x4_t a[3];
#pragma unroll
    for (int kk = 0; kk < 3; kk++) a[kk] = d2_x_frag<T>(x, ldx, m0 + c16, M, Cin, 4 * kk + g);
    f32x4_t acc[NT];
    d2_layer1<T, NT>(reinterpret_cast<const char*>(w1t), a, ksteps, lane, acc);
    float s[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int o = 0; o < 4; o++) s[r][o] = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
      const int j = nt * 16 + c16;
      const float bj = b1s[j];
      const f32x4_t w = *reinterpret_cast<const f32x4_t*>(w2s + 4 * j);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float v = acc[nt][r] + bj;
        const float h = round_T<T>(v > 0.f ? v : 0.f);
#pragma unroll
        for (int o = 0; o < 4; o++) s[r][o] = fmaf(h, w[o], s[r][o]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int o = 0; o < 4; o++) s[r][o] = row16_sum(s[r][o]);
    // lane (g, c16 = r) writes pixel 4 g + r
    const long long mo = m0 + 4 * g + c16;
    if (c16 < 4 && mo < M) {
#pragma unroll
      for (int o = 0; o < 4; o++) {
        // (a bitwise select: a ?: chain over s[r][o] becomes a table in private memory)
        uint32_t bits = 0u;
#pragma unroll
        for (int r = 0; r < 4; r++) bits |= __builtin_bit_cast(uint32_t, s[r][o]) & (c16 == r ? 0xffffffffu : 0u);
        if (o < Cout) y[(size_t)mo * Cout + o] = keras_f16_point<T>(__builtin_bit_cast(float, bits) + b2[o]);
      }
    }
  }
}

// LDS of the backward kernel, in bytes from the start (every offset a multiple of 16)
struct D2BwdLds {
  int w1t, w1s, dhs, dht, xt, w2s, b1s, fin, total, dhs_ld, fin_ld;
};
inline __host__ __device__ D2BwdLds d2_bwd_lds(int Chid) {
  D2BwdLds l;
  l.dhs_ld = Chid + 8;
  l.fin_ld = Chid * 5 + 4;
  l.w1t = 0;                                         // [Chid][D2_W1T_LD]: w1^T, layer 1's B operand
  l.w1s = l.w1t + Chid * D2_W1T_LD * 2;              // [D2_CROWS][Chid + 8]: w1, dx's B operand (rows >= Cin zero)
  l.dhs = l.w1s + D2_CROWS * l.dhs_ld * 2;           // [64][Chid + 8]: dh, dx's A operand
  l.dht = l.dhs + D2_FAST_PIX * l.dhs_ld * 2;        // [Chid][D2_PIX_LD]: dh^T, dw1's B operand
  l.xt = l.dht + Chid * D2_PIX_LD * 2;               // [D2_CROWS][D2_PIX_LD]: x^T, dw1's A operand and dx's ReLU mask
  l.w2s = l.xt + D2_CROWS * D2_PIX_LD * 2;           // fp32 [Chid][4]
  l.b1s = l.w2s + Chid * 16;                         // fp32 [Chid]
  l.fin = l.b1s + Chid * 4;                          // fp32 [4 waves][db1: Chid | dw2: Chid x 4 | db2: 4]
  l.total = l.fin + 4 * l.fin_ld * 4;
  return l;
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void dense2_mfma_bwd_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ w1,
                                                              const float* __restrict__ b1, const float* __restrict__ w2,
                                                              const float* __restrict__ dy, T* __restrict__ dx, int lddx,
                                                              float* __restrict__ part, int rowf, int M, int Cin, int Cout, int Cmask) {
  constexpr int Chid = NT * 16;
  constexpr int MAXQ = (5 * NT + 3) / 4;             // dw1 tiles (16 channels x 16 hidden units) per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const D2BwdLds L = d2_bwd_lds(Chid);
  T* w1t = reinterpret_cast<T*>(smem + L.w1t);
  T* w1s = reinterpret_cast<T*>(smem + L.w1s);
  T* dhs = reinterpret_cast<T*>(smem + L.dhs);
  T* dht = reinterpret_cast<T*>(smem + L.dht);
  T* xt = reinterpret_cast<T*>(smem + L.xt);
  float* w2s = reinterpret_cast<float*>(smem + L.w2s);
  float* b1s = reinterpret_cast<float*>(smem + L.b1s);
  float* fin = reinterpret_cast<float*>(smem + L.fin);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
  const int CT = (Cin + 15) / 16, CT16 = CT * 16;    // channel tiles (<= 5)
  d2_stage_w1t<T>(w1t, w1, Cin, Chid, tid);
  for (int idx = tid; idx < D2_CROWS * Chid; idx += 256) {
    const int i = idx / Chid, j = idx - i * Chid;
    w1s[i * L.dhs_ld + j] = i < Cin ? w1[i * Chid + j] : from_f32<T>(0.f);
  }
  for (int i = tid; i < Chid * 4; i += 256) w2s[i] = (i & 3) < Cout ? w2[(i >> 2) * Cout + (i & 3)] : 0.f;
  for (int i = tid; i < Chid; i += 256) b1s[i] = b1[i];

  const int ksteps = (Cin + 31) / 32;
  const int nct = dx ? (Cmask + 15) / 16 : 0;
  f32x4_t acc1[MAXQ];
#pragma unroll
  for (int q = 0; q < MAXQ; q++) acc1[q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float db1acc[NT], dw2acc[NT][4], db2acc[4];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    db1acc[nt] = 0.f;
#pragma unroll
    for (int o = 0; o < 4; o++) dw2acc[nt][o] = 0.f;
  }
#pragma unroll
  for (int o = 0; o < 4; o++) db2acc[o] = 0.f;

  const long long ntiles = ((long long)M + D2_FAST_PIX - 1) / D2_FAST_PIX;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long m0 = tile * D2_FAST_PIX + wave * 16;
    const int p0 = wave * 16;                        // this wave's first pixel inside the tile
    __syncthreads();                                 // the images of the previous tile have been read (first pass: the weights are staged)
    u32x4_t a[3];
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
      a[kk] = d2_x_frag<T>(x, ldx, m0 + c16, M, Cin, 4 * kk + g);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int ch = 32 * kk + 8 * g + e;
        const uint32_t u = a[kk][e >> 1];
        if (ch < CT16) reinterpret_cast<uint16_t*>(xt)[ch * D2_PIX_LD + p0 + c16] = (uint16_t)((e & 1) ? (u >> 16) : (u & 0xffffu));
      }
    }
    f32x4_t acc[NT];
    d2_layer1<T, NT>(reinterpret_cast<const char*>(w1t), a, ksteps, lane, acc);
    float dyv[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const long long m = m0 + 4 * g + r;
#pragma unroll
      for (int o = 0; o < 4; o++) dyv[r][o] = (o < Cout && m < M) ? keras_f16_point<T>(dy[(size_t)m * Cout + o]) : 0.f;
    }
#pragma unroll
    for (int o = 0; o < 4; o++) db2acc[o] += (dyv[0][o] + dyv[1][o]) + (dyv[2][o] + dyv[3][o]);
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
      const int j = nt * 16 + c16;
      const float bj = b1s[j];
      const f32x4_t w = *reinterpret_cast<const f32x4_t*>(w2s + 4 * j);
      float dh[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float v = acc[nt][r] + bj;
        const float h = round_T<T>(v > 0.f ? v : 0.f);
        float gs = 0.f;
#pragma unroll
        for (int o = 0; o < 4; o++) gs = fmaf(dyv[r][o], w[o], gs);
        dh[r] = h > 0.f ? round_T<T>(gs) : 0.f;
        db1acc[nt] += dh[r];
#pragma unroll
        for (int o = 0; o < 4; o++) dw2acc[nt][o] = fmaf(h, dyv[r][o], dw2acc[nt][o]);
        dhs[(p0 + 4 * g + r) * L.dhs_ld + j] = from_f32<T>(dh[r]);
      }
      const u32x2_t pk = {pack2<T>(dh[0], dh[1]), pack2<T>(dh[2], dh[3])};
      *reinterpret_cast<u32x2_t*>(dht + j * D2_PIX_LD + p0 + 4 * g) = pk;
    }
    __syncthreads();
    // dx of this wave's 16 pixels: dh (16 x Chid) times w1^T (Chid x 16 channels per tile)
#pragma unroll
    for (int ct = 0; ct < 5; ct++) {
      if (ct < nct) {
        f32x4_t ax = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < NT / 2; kk++) {
          const u32x4_t fa = lds_read128(reinterpret_cast<const char*>(dhs), ((p0 + c16) * L.dhs_ld + 32 * kk + 8 * g) * 2);
          const u32x4_t fb = lds_read128(reinterpret_cast<const char*>(w1s), ((ct * 16 + c16) * L.dhs_ld + 32 * kk + 8 * g) * 2);
          ax = mfma16<T>(fa, fb, ax);
        }
        const int i = ct * 16 + c16;
        if (i < Cmask) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const long long m = m0 + 4 * g + r;
            const float xv = to_f32<T>(xt[i * D2_PIX_LD + p0 + 4 * g + r]);
            if (m < M) dx[(size_t)m * lddx + i] = from_f32<T>(xv > 0.f ? ax[r] : 0.f);
          }
        }
      }
    }
    // dw1 += x^T dh over the 64 pixels of the tile: wave w owns the (channel tile, hidden tile) pairs w, w + 4, ...
#pragma unroll
    for (int q = 0; q < MAXQ; q++) {
      const int t = wave + 4 * q;
      if (t < CT * NT) {
        const int ct = t / NT, nt = t - ct * NT;
#pragma unroll
        for (int kk = 0; kk < D2_FAST_PIX / 32; kk++) {
          const u32x4_t fa = lds_read128(reinterpret_cast<const char*>(xt), ((ct * 16 + c16) * D2_PIX_LD + 32 * kk + 8 * g) * 2);
          const u32x4_t fb = lds_read128(reinterpret_cast<const char*>(dht), ((nt * 16 + c16) * D2_PIX_LD + 32 * kk + 8 * g) * 2);
          acc1[q] = mfma16<T>(fa, fb, acc1[q]);
        }
      }
    }
  }

  // the work-group's partial row
  float* row = part + (size_t)blockIdx.x * rowf;
  const int n1 = Cin * Chid;
#pragma unroll
  for (int q = 0; q < MAXQ; q++) {
    const int t = wave + 4 * q;
    if (t < CT * NT) {
      const int ct = t / NT, nt = t - ct * NT;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = ct * 16 + 4 * g + r;
        if (i < Cin) row[i * Chid + nt * 16 + c16] = acc1[q][r];
      }
    }
  }
  // db1 / dw2 / db2: the four lane rows of a wave (fixed pairs), then the four waves in ascending order
  float* myfin = fin + wave * L.fin_ld;
#pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    const float s1 = rows4_sum(db1acc[nt]);
    if (g == 0) myfin[nt * 16 + c16] = s1;
#pragma unroll
    for (int o = 0; o < 4; o++) {
      const float s2 = rows4_sum(dw2acc[nt][o]);
      if (g == 0) myfin[Chid + (nt * 16 + c16) * 4 + o] = s2;
    }
  }
#pragma unroll
  for (int o = 0; o < 4; o++) {
    const float s3 = rows4_sum(db2acc[o]);
    if (lane == 0) myfin[Chid * 5 + o] = s3;
  }
  __syncthreads();
  const int n2 = Chid * Cout;
  for (int e = tid; e < Chid + n2 + Cout; e += 256) {
    int src;
    if (e < Chid) src = e;
    else if (e < Chid + n2) { const int q = e - Chid, j = q / Cout, o = q - j * Cout; src = Chid + j * 4 + o; }
    else src = Chid * 5 + (e - Chid - n2);
    row[n1 + e] = ((fin[src] + fin[L.fin_ld + src]) + fin[2 * L.fin_ld + src]) + fin[3 * L.fin_ld + src];
  }
}

bool fast_ok(const gct2_ctx& c, int dtype, const void* x, int ldx, int Cin, int Chid) {
  return !c.force_direct && dtype != GCT2_F32 && (Chid == 32 || Chid == 64 || Chid == 128) && Cin <= D2_CROWS && ldx % 8 == 0 &&
         (uintptr_t)x % 16 == 0;
}

template <typename K> void allow_lds(K kern, size_t lds) {
  if (lds > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

}  // namespace

static_assert(D2_FAST_PIX == 64, "the mfma kernels are four waves of 16 pixels");
size_t dense2_scratch_floats(int M, int Cin, int Chid, int Cout) {
  return (size_t)groups(M, D2_PLAIN_PIX) * (size_t)row_floats(Cin, Chid, Cout);      // (the plain kernel has the smaller tile: the larger figure)
}

int dense2_fwd(gct2_ctx& c, int dtype, const void* x, int ldx, const void* w1, const float* b1, const float* w2, const float* b2, float* y,
               int M, int Cin, int Chid, int Cout, hipStream_t s) {
  if (fast_ok(c, dtype, x, ldx, Cin, Chid)) {
    gct2_log(c, "dense2:fwd:mfma");
    const int grid = groups(M, D2_FAST_PIX);
    const size_t lds = (size_t)Chid * D2_W1T_LD * 2 + (size_t)Chid * 20;
    with_dtype16(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      auto launch = [&](auto kern) {
        allow_lds(kern, lds);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, reinterpret_cast<const T*>(x), ldx, reinterpret_cast<const T*>(w1), b1, w2, b2, y,
                           M, Cin, Cout);
      };
      if (Chid == 32) launch(dense2_mfma_fwd_kernel<T, 2>);
      else if (Chid == 64) launch(dense2_mfma_fwd_kernel<T, 4>);
      else launch(dense2_mfma_fwd_kernel<T, 8>);
    });
    return gct2_check_launch("dense2_fwd");
  }
  gct2_log(c, "dense2:fwd:plain");
  const long long tiles = ((long long)M + 63) / 64;
  const int grid = (int)(tiles < 4096 ? tiles : 4096);
  const size_t lds = (size_t)64 * (Cin + 1) * sizeof(float);
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto kern = dense2_plain_fwd_kernel<T>;
    allow_lds(kern, lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), lds, s, reinterpret_cast<const T*>(x), ldx, reinterpret_cast<const T*>(w1), b1, w2, b2, y, M, Cin,
                       Chid, Cout);
  });
  return gct2_check_launch("dense2_fwd");
}

int dense2_bwd(gct2_ctx& c, int dtype, const void* x, int ldx, const void* w1, const float* b1, const float* w2, const float* dy, void* dx,
               int lddx, float* dw1, float* db1, float* dw2, float* db2, float* scratch, int M, int Cin, int Chid, int Cout, int Cmask,
               int accumulate, hipStream_t s) {
  const int rowf = row_floats(Cin, Chid, Cout);
  if (Cmask == 0) dx = nullptr;
  int rows;
  if (fast_ok(c, dtype, x, ldx, Cin, Chid)) {
    gct2_log(c, "dense2:bwd:mfma");
    rows = groups(M, D2_FAST_PIX);
    const size_t lds = (size_t)d2_bwd_lds(Chid).total;
    with_dtype16(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      auto launch = [&](auto kern) {
        allow_lds(kern, lds);
        hipLaunchKernelGGL(kern, dim3(rows), dim3(256), lds, s, reinterpret_cast<const T*>(x), ldx, reinterpret_cast<const T*>(w1), b1, w2, dy,
                           reinterpret_cast<T*>(dx), lddx, scratch, rowf, M, Cin, Cout, Cmask);
      };
      if (Chid == 32) launch(dense2_mfma_bwd_kernel<T, 2>);
      else if (Chid == 64) launch(dense2_mfma_bwd_kernel<T, 4>);
      else launch(dense2_mfma_bwd_kernel<T, 8>);
    });
  } else {
    gct2_log(c, "dense2:bwd:plain");
    rows = groups(M, D2_PLAIN_PIX);
    const size_t lds = (size_t)D2_PLAIN_PIX * (Cin + 2 * Chid + 4) * sizeof(float);
    with_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      auto kern = dense2_plain_bwd_kernel<T>;
      allow_lds(kern, lds);
      hipLaunchKernelGGL(kern, dim3(rows), dim3(256), lds, s, reinterpret_cast<const T*>(x), ldx, reinterpret_cast<const T*>(w1), b1, w2, dy,
                         reinterpret_cast<T*>(dx), lddx, scratch, rowf, M, Cin, Chid, Cout, Cmask);
    });
  }
  if (int e = gct2_check_launch("dense2_bwd")) return e;
  const int total = Cin * Chid + Chid + Chid * Cout + Cout;
  hipLaunchKernelGGL(dense2_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, s, scratch, rows, rowf, dw1, db1, dw2, db2, Cin * Chid, Chid,
                     Chid * Cout, Cout, accumulate);
  return gct2_check_launch("dense2_bwd");
}
