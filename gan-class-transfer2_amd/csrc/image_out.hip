// Samples as pictures (include/gct2.h, gct2_image_grid_u8): the quantisation of a whole batch to uint8 and its layout as a grid of
// cells - padding, empty cells and integer nearest-neighbour upscaling included - in ONE launch that writes every byte of the output.
// It is csrc/data.hip turned round: floats in, bytes out.
//
// Wide path (GW % 4 == 0 and a 4-byte aligned out): a thread owns four horizontally adjacent output pixels - 12 bytes that start on a
// dword boundary, three dword stores, 768 contiguous bytes per wave.  Where the four pixels lie inside one image and scale == 1
// their twelve source elements are contiguous: they are read as three 16-byte loads (fp32; dword aligned, which is all a global
// load needs) or as six dwords (16-bit sources whose first element sits on a dword boundary).  Every other group - one that straddles
// padding and image, an upscaled one, one in an empty cell - classifies its four pixels one by one and still leaves through the same
// three stores.  Per-pixel path (any other GW or alignment): one output pixel per thread and trip, three byte stores, the same
// classification and the same bits.  Both are grid-stride loops over size_t indices: n H W 3 and GH GW 3 may exceed 2^31.
#include "gct2_common.h"

namespace {

constexpr int kThreads = 256;

struct GridGeom {
  int n, H, W, cols, pad, scale;
  int PH, PW;               // cell pitch: H scale + pad, W scale + pad
  int GH, GW;
  uint32_t fill;            // R | G << 8 | B << 16
  int src_odd;              // a 16-bit src that starts on an odd element of its dword
};

// include/gct2.h: one float32 rounding per operation (the intrinsics keep the compiler from contracting multiply and add; the bits
// would be the same either way, 0.5 x and 128 x being exact)
__device__ __forceinline__ uint32_t quantize(float x, int mode) {
  float z;
  if (mode == GCT2_U8_SUMMARY) z = __fmul_rn(255.5f, __fadd_rn(__fmul_rn(0.5f, x), 0.5f));
  else if (mode == GCT2_U8_DATASET) z = __fadd_rn(__fmul_rn(128.0f, x), 128.5f);
  else z = __fmul_rn(255.5f, x);
  return !(z >= 1.0f) ? 0u : (z >= 255.0f ? 255u : (uint32_t)z);      // NaN and z < 1 -> 0
}

// grid row y -> (cell row r, source row sy); false in the padding
__device__ __forceinline__ bool source_row(const GridGeom& g, int y, int& r, int& sy) {
  r = y / g.PH;
  const int ly = y - r * g.PH - g.pad;
  sy = g.scale == 1 ? ly : ly / g.scale;
  return ly >= 0;           // (the last pad rows have r = rows and ly < 0)
}

// the pixel (y, x) of the grid as 24 bits R | G << 8 | B << 16
template <typename T>
__device__ __forceinline__ uint32_t grid_pixel(const T* __restrict__ src, const GridGeom& g, int mode, bool row_in, int r, int sy, int c, int lx) {
  if (row_in && lx >= 0) {
    const size_t i = (size_t)r * g.cols + c;
    if (i < (size_t)g.n) {
      const int sx = g.scale == 1 ? lx : lx / g.scale;
      const T* __restrict__ p = src + ((i * g.H + sy) * g.W + sx) * 3;
      return quantize(to_f32<T>(p[0]), mode) | quantize(to_f32<T>(p[1]), mode) << 8 | quantize(to_f32<T>(p[2]), mode) << 16;
    }
  }
  return g.fill;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void image_grid_wide_kernel(const T* __restrict__ src, uint32_t* __restrict__ out, GridGeom g, int mode,
                                                                    size_t groups) {
  const uint32_t q = (uint32_t)g.GW >> 2;                 // groups of four pixels per grid row
  const size_t step = (size_t)gridDim.x * kThreads;
  for (size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x; t < groups; t += step) {
    int y, x0;
    if ((t >> 32) == 0) { y = (int)((uint32_t)t / q); x0 = (int)((uint32_t)t - (uint32_t)y * q) * 4; }
    else { y = (int)(t / q); x0 = (int)(t - (size_t)y * q) * 4; }
    int r, sy;
    const bool row_in = source_row(g, y, r, sy);
    int c = x0 / g.PW;
    int lx = x0 - c * g.PW - g.pad;                       // in [-pad, PW - pad)
    uint32_t b[12];
    if (row_in && g.scale == 1 && lx >= 0 && lx + 3 < g.W && (size_t)r * g.cols + c < (size_t)g.n) {
      const size_t e = ((((size_t)r * g.cols + c) * g.H + sy) * g.W + lx) * 3;      // twelve contiguous source elements
      float v[12];
      if constexpr (sizeof(T) == 4) {
        __builtin_memcpy(v, src + e, 48);                 // (dword aligned: three 16-byte loads)
      } else {
        if (((e + g.src_odd) & 1) == 0) {                 // the first element sits on a dword boundary
          uint32_t w[6];
          __builtin_memcpy(w, __builtin_assume_aligned(src + e, 4), 24);
#pragma unroll
          for (int i = 0; i < 6; i++) { v[2 * i] = unpack_lo<T>(w[i]); v[2 * i + 1] = unpack_hi<T>(w[i]); }
        } else {
#pragma unroll
          for (int i = 0; i < 12; i++) v[i] = to_f32<T>(src[e + i]);
        }
      }
#pragma unroll
      for (int i = 0; i < 12; i++) b[i] = quantize(v[i], mode);
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        while (lx >= g.PW - g.pad) { lx -= g.PW; c++; }   // (the next cell; more than once only where a cell is narrower than a group)
        const uint32_t px = grid_pixel<T>(src, g, mode, row_in, r, sy, c, lx);
        b[3 * j] = px & 0xffu; b[3 * j + 1] = (px >> 8) & 0xffu; b[3 * j + 2] = px >> 16;
        lx++;
      }
    }
    uint32_t* __restrict__ o = out + t * 3;               // group t is bytes 12 t .. 12 t + 11 of the grid
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = b[4 * i] | b[4 * i + 1] << 8 | b[4 * i + 2] << 16 | b[4 * i + 3] << 24;
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void image_grid_pixel_kernel(const T* __restrict__ src, uint8_t* __restrict__ out, GridGeom g, int mode,
                                                                     size_t pixels) {
  const size_t step = (size_t)gridDim.x * kThreads;
  for (size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x; t < pixels; t += step) {
    int y, x;
    if ((t >> 32) == 0) { y = (int)((uint32_t)t / (uint32_t)g.GW); x = (int)((uint32_t)t - (uint32_t)y * (uint32_t)g.GW); }
    else { y = (int)(t / (uint32_t)g.GW); x = (int)(t - (size_t)y * (uint32_t)g.GW); }
    int r, sy;
    const bool row_in = source_row(g, y, r, sy);
    const int c = x / g.PW;
    const uint32_t px = grid_pixel<T>(src, g, mode, row_in, r, sy, c, x - c * g.PW - g.pad);
    uint8_t* __restrict__ o = out + t * 3;
    o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16);
  }
}

}  // namespace

int img_grid_u8(const void* src, int dtype, int n, int H, int W, int mode, int cols, int rows, int pad, int scale, uint32_t fill_rgb,
                uint8_t* out, hipStream_t s) {
  const long long PH = (long long)H * scale + pad, PW = (long long)W * scale + pad;
  const long long GH = rows * PH + pad, GW = cols * PW + pad;
  if (GH > 0x7fffffffLL || GW > 0x7fffffffLL)
    return gct2_fail(GCT2_EINVAL, "image_grid_u8: a grid of %lld x %lld pixels has a side above 2^31 - 1", GH, GW);
  const GridGeom g = {n, H, W, cols, pad, scale, (int)PH, (int)PW, (int)GH, (int)GW, fill_rgb,
                      (int)((reinterpret_cast<uintptr_t>(src) >> 1) & 1)};
  const bool wide = (GW & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  // thread items: groups of four pixels (wide) or pixels; two / four trips per thread where the grid is large enough
  const unsigned long long items = (unsigned long long)GH * (unsigned long long)(wide ? GW >> 2 : GW);
  const unsigned long long per_group = (unsigned long long)kThreads * (wide ? 2 : 4);
  const unsigned long long groups = (items + per_group - 1) / per_group;
  if (groups > 0x7fffffffULL)
    return gct2_fail(GCT2_EINVAL, "image_grid_u8: a grid of %lld x %lld pixels needs more than 2^31 - 1 work-groups", GH, GW);
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (wide)
      hipLaunchKernelGGL(image_grid_wide_kernel<T>, dim3((unsigned)groups), dim3(kThreads), 0, s, static_cast<const T*>(src),
                         reinterpret_cast<uint32_t*>(out), g, mode, (size_t)items);
    else
      hipLaunchKernelGGL(image_grid_pixel_kernel<T>, dim3((unsigned)groups), dim3(kThreads), 0, s, static_cast<const T*>(src), out, g, mode,
                         (size_t)items);
  });
  return gct2_check_launch("image_grid_u8");
}
