// The device-resident image cache (include/gct2.h, gct2_image_batch_cached): which image, where to crop, whether to flip, the crop,
// the flip and value / 128 - 1 of a whole batch in ONE launch that reads nothing from the host.
//
// A work-group belongs to one sample b.  Everything that decides its pick - the sample index k, the epoch's permutation, the two
// Philox calls, the table reads - depends on kernel arguments and the work-group index alone, so it is wave-uniform: the compiler
// keeps it on the scalar unit, once per wave beside the vector loads, and no second launch or global hand-over of the draws is needed.
//
// Wide path (size % 4 == 0, dst 16-byte aligned, pool 4-byte aligned): a thread owns four consecutive pixels of an output row.  Their
// 12 source bytes are contiguous whether flipped or not (flipping reverses the pixel order and keeps the channel order) and start at
// any byte alignment: the thread reads the three or four ALIGNED dwords around them (the fourth only when the start is unaligned, so at
// most 3 bytes behind the 12 are touched - the pool's spare bytes cover the last image), shifts them into place and writes three
// 16-byte stores: 48 contiguous bytes per lane, 3 KiB contiguous per wave.  No division wider than 32 bits per thread.
// Per-element path (any other size or alignment, and every clamped sample): one float per thread and trip, coordinates clamped into the
// image.  Measured at 64 x 128 x 128 x 3 (profiles/image_cache_bench.json): 6.3 us with the picks given, 7.2 us drawing them, 9.7 us on
// the per-element path, gct2_image_prepare 8.8 us.
#include "gct2_common.h"

namespace {

constexpr uint64_t kStreamAug = 6, kStreamOrder = 7;      // trainer_math.DATA_STREAM_AUG / DATA_STREAM_ORDER
constexpr int kThreads = 256;

__device__ __forceinline__ uint32_t fmix32(uint32_t x) {   // murmur3's finaliser
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}

// pi_e(p): balanced Feistel network over 2h bits keyed by the epoch, cycle-walked into [0, N).  2^(2h) < 4N: the walk is short.
__device__ __forceinline__ uint32_t epoch_permutation(uint64_t seed, uint64_t e, uint32_t p, uint32_t N) {
  if (N == 1) return 0;
  const int bits = 32 - __builtin_clz(N - 1);             // bitlen(N - 1) in 1..31
  const int h = (bits + 1) >> 1;                          // 1..16
  const uint32_t mask = (1u << h) - 1u;
  uint32_t ks[4];
  philox4x32_10(seed, kStreamOrder, e, ks);
  uint32_t v = p;
  do {
    uint32_t L = v >> h, R = v & mask;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t kj = ks[j & 3] + (uint32_t)j * 0x9E3779B9u;
      const uint32_t t = L ^ (fmix32(R ^ kj) & mask);
      L = R; R = t;
    }
    v = (L << h) | R;
  } while (v >= N);
  return v;
}

struct Pick { int item, oy, ox, flip, H0, W0, bad; };

// the pick of sample b: read from picks_in or drawn for k = first_sample + b * sample_stride; out-of-range values clamped (bad = 1)
__device__ __forceinline__ Pick resolve_pick(const int32_t* __restrict__ hw, int N, uint64_t seed, uint64_t first_sample, uint64_t sample_stride,
                                             int flags, const int32_t* __restrict__ picks_in, int b, int size) {
  Pick p;
  p.bad = 0;
  uint32_t r[4] = {0u, 0u, 0u, 0u};
  if (picks_in) {
    p.item = picks_in[4 * b];
    if (p.item < 0 || p.item >= N) { p.item = p.item < 0 ? 0 : N - 1; p.bad = 1; }
  } else {
    const uint64_t k = first_sample + (uint64_t)b * sample_stride;
    uint64_t e;
    uint32_t pos;
    if ((k >> 32) == 0) { e = (uint32_t)k / (uint32_t)N; pos = (uint32_t)k % (uint32_t)N; }      // (one division per wave, 32-bit when it can be)
    else { e = k / (uint64_t)N; pos = (uint32_t)(k % (uint64_t)N); }
    p.item = (flags & GCT2_DATA_SHUFFLE) ? (int)epoch_permutation(seed, e, pos, (uint32_t)N) : (int)pos;
    if (flags & (GCT2_DATA_RANDOM_CROP | GCT2_DATA_FLIP)) philox4x32_10(seed, kStreamAug, k, r);
  }
  p.H0 = hw[2 * p.item];
  p.W0 = hw[2 * p.item + 1];
  const int ry = p.H0 - size, rx = p.W0 - size;           // the largest origin
  if (ry < 0 || rx < 0) p.bad = 1;
  if (picks_in) {
    p.oy = picks_in[4 * b + 1]; p.ox = picks_in[4 * b + 2]; p.flip = picks_in[4 * b + 3] != 0;
    if (p.oy < 0 || p.oy > ry || p.ox < 0 || p.ox > rx) p.bad = 1;
  } else {
    if (flags & GCT2_DATA_RANDOM_CROP) {
      p.oy = ry < 0 ? 0 : (int)(((uint64_t)r[0] * (uint64_t)(uint32_t)(ry + 1)) >> 32);
      p.ox = rx < 0 ? 0 : (int)(((uint64_t)r[1] * (uint64_t)(uint32_t)(rx + 1)) >> 32);
    } else {
      p.oy = ry / 2; p.ox = rx / 2;                       // the validation pass's centre crop
    }
    p.flip = (flags & GCT2_DATA_FLIP) ? (int)(r[2] >> 31) : 0;
  }
  if (p.bad) {                                            // into the image: 0 <= origin <= max(largest origin, 0)
    p.oy = min(max(p.oy, 0), max(ry, 0));
    p.ox = min(max(p.ox, 0), max(rx, 0));
  }
  return p;
}

__device__ __forceinline__ float cast_u8(uint32_t v) { return (float)v * (1.0f / 128.0f) - 1.0f; }      // exact: v/128 has at most 8 significant bits

// grid: B * bpi work-groups, work-group j of sample b strides over the sample's thread items from j * kThreads
__global__ __launch_bounds__(kThreads) void image_batch_cached_kernel(
    const uint8_t* __restrict__ pool, const int64_t* __restrict__ offsets, const int32_t* __restrict__ hw, int N, uint64_t seed,
    uint64_t first_sample, uint64_t sample_stride, int flags, const int32_t* __restrict__ picks_in, int32_t* __restrict__ picks_out,
    float* __restrict__ dst, int size, int bpi, int wide) {
  const int b = (int)(blockIdx.x / (unsigned)bpi), j = (int)(blockIdx.x - (unsigned)b * (unsigned)bpi);
  const Pick p = resolve_pick(hw, N, seed, first_sample, sample_stride, flags, picks_in, b, size);
  if (picks_out && j == 0 && threadIdx.x == 0) {
    int32_t* o = picks_out + 4 * (size_t)b;
    o[0] = p.bad ? -1 : p.item; o[1] = p.oy; o[2] = p.ox; o[3] = p.flip;
  }
  const int64_t img = offsets[p.item];                    // byte offset of the image in the pool
  float* __restrict__ out = dst + (size_t)b * size * size * 3;
  const int step = bpi * kThreads;
  if (wide && !p.bad) {
    const int q = size >> 2, groups = size * q;           // groups of four pixels: per row, per image
    for (int g = j * kThreads + (int)threadIdx.x; g < groups; g += step) {
      const int y = g / q, x0 = (g - y * q) * 4;
      const int sx0 = p.ox + (p.flip ? size - 4 - x0 : x0);
      const int64_t a = img + ((int64_t)(p.oy + y) * p.W0 + sx0) * 3;       // first of the 12 source bytes
      const uint32_t* __restrict__ wp = reinterpret_cast<const uint32_t*>(pool + (a & ~(int64_t)3));
      const uint32_t sh = ((uint32_t)a & 3u) * 8u;
      const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = sh ? wp[3] : 0u;
      uint32_t d[3];
      d[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
      d[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
      d[2] = (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh);
      float v[12];
#pragma unroll
      for (int i = 0; i < 12; i++) v[i] = cast_u8((d[i >> 2] >> (8 * (i & 3))) & 0xffu);
      f32x4_t s[3];
#pragma unroll
      for (int i = 0; i < 12; i++) {                      // output pixel i / 3 is source pixel 3 - i / 3 when flipped, same channel
        const int m = 3 * (3 - i / 3) + i % 3;
        s[i >> 2][i & 3] = p.flip ? v[m] : v[i];
      }
      f32x4_t* __restrict__ o = reinterpret_cast<f32x4_t*>(out + ((size_t)y * size + x0) * 3);
      o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
    }
  } else {
    const int per = size * size * 3;
    const bool empty = p.H0 < 1 || p.W0 < 1;              // (a table entry without a single pixel: nothing is read)
#pragma unroll 4
    for (int i = j * kThreads + (int)threadIdx.x; i < per; i += step) {
      const int xy = i / 3, c = i - 3 * xy;
      const int y = xy / size, x = xy - y * size;
      const int sy = min(p.oy + y, p.H0 - 1), sx = min(p.ox + (p.flip ? size - 1 - x : x), p.W0 - 1);      // (only a clamped sample is cut)
      const uint32_t v = empty ? 0u : pool[img + ((int64_t)sy * p.W0 + sx) * 3 + c];
      out[i] = cast_u8(v);
    }
  }
}

}  // namespace

int data_image_batch_cached(const uint8_t* pool, const int64_t* offsets, const int32_t* hw, int N, uint64_t seed, uint64_t first_sample,
                            uint64_t sample_stride, int flags, const int32_t* picks_in, int32_t* picks_out, float* dst, int B, int size,
                            hipStream_t s) {
  const int wide = (size & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (reinterpret_cast<uintptr_t>(pool) & 3) == 0;
  // thread items of a sample: groups of four pixels, or floats; two (wide) / twelve items per thread - 24 / 12 floats - so that the
  // pick, which every wave forms for itself, is shared by as many stores on both paths
  const long long items = wide ? (long long)size * (size >> 2) : (long long)size * size * 3;
  const long long per_group = (long long)kThreads * (wide ? 2 : 12);
  const long long bpi = (items + per_group - 1) / per_group;
  if (bpi * B > 0x7fffffffLL) return gct2_fail(GCT2_EINVAL, "image_batch_cached: B=%d size=%d needs more than 2^31 - 1 work-groups", B, size);
  hipLaunchKernelGGL(image_batch_cached_kernel, dim3((unsigned)(bpi * B)), dim3(kThreads), 0, s, pool, offsets, hw, N, seed, first_sample,
                     sample_stride, flags, picks_in, picks_out, dst, size, (int)bpi, wide);
  return gct2_check_launch("image_batch_cached");
}
