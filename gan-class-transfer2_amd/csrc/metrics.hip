// Image metrics of evaluation (include/gct2.h, gct2_image_metrics): per image, the mean squared error of the x0 estimate against the
// clean image, its PSNR, and the SSIM of Wang et al. 2004 with the defaults of tf.image.ssim (a K x K window handed in as a table,
// VALID filtering, the mean of lum * cs over every window position and channel).
//
// One work-group = one image (blockIdx.y), one 32 x 32 tile of pixels and one channel (blockIdx.x).  It stages the estimate e and the
// clean image x of its tile plus the K - 1 rows / columns behind it in LDS as floats, e formed on load by the rule of
// mix_per_image_kernel; runs the separable filter over the five planes e, x, e e, x x, e x in fp64 (rows first, parked in LDS, then
// columns); and leaves ONE fp64 pair in scratch: the sum of lum * cs over the window positions that START in its tile, and the sum of
// d^2 over the pixels OF its tile.  The tiles cut the image, so every pixel is counted once although the staged regions overlap; the
// cut does not depend on K and the d^2 loop does not depend on whether SSIM was asked for, so mse and psnr have the same bits with
// and without it.  A finishing launch adds the pairs of an image in index order.  No atomics.
//
// LDS: 2 x 47 x 47 floats + 5 x 47 x 32 doubles = 76.2 KiB: two work-groups per CU (160 KiB).  Lanes walk the columns of a tile row,
// so every LDS access of a wave is to consecutive words.
#include "gct2_common.h"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int MT = 32;                       // GCT2_METRICS_TILE: pixels (and window positions) per side of a tile
constexpr int MKMAX = 16;                    // the largest window
constexpr int MHALO = MT + MKMAX - 1;        // staged rows / columns at most

struct MetricsArgs {
  const float* pred; const float* noised; const float* u; const float* v; const float* x; const float* window;
  int K, H, W, C, tiles_x, tiles_y, filter;
  double C1, C2;
  double* part;                              // [2][B][nt]: sums of lum * cs, then sums of d^2
  int nt;                                    // tiles_x * tiles_y * C
};

__device__ __forceinline__ double block_sum256(double acc, double* ws4) {
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws4[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((ws4[0] + ws4[1]) + ws4[2]) + ws4[3];
}

__global__ __launch_bounds__(256) void metrics_tile_kernel(MetricsArgs a) {
  __shared__ float se[MHALO * MHALO];
  __shared__ float sx[MHALO * MHALO];
  __shared__ double rows[5][MHALO * MT];
  __shared__ double sw[MKMAX];
  __shared__ double ws4[4];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int ch = blockIdx.x % a.C, tile = blockIdx.x / a.C;
  const int r0 = (tile / a.tiles_x) * MT, c0 = (tile % a.tiles_x) * MT;
  const int own_h = min(MT, a.H - r0), own_w = min(MT, a.W - c0);                // the pixels of this tile
  const int K = a.K;
  int noh = 0, now = 0;                                                        // the window positions that start in it
  if (a.filter) {
    noh = max(0, min(MT, a.H - K + 1 - r0));
    now = max(0, min(MT, a.W - K + 1 - c0));
    if (noh == 0 || now == 0) noh = now = 0;
  }
  // staged region: the tile itself, and with window positions everything they read: noh + K - 1 >= own_h rows (noh = 32, or the
  // region ends with the image), never a row or column outside the image
  const int hr = noh ? noh + K - 1 : own_h, hc = now ? now + K - 1 : own_w;
  const bool mix = a.u != nullptr;
  const float ub = mix ? a.u[b] : 1.f, vb = mix ? a.v[b] : 0.f;
  if (tid < K && a.filter) sw[tid] = (double)a.window[tid];
  for (int idx = tid; idx < hr * hc; idx += 256) {
    const int r = idx / hc, c = idx - r * hc;
    const size_t g = (((size_t)b * a.H + (size_t)(r0 + r)) * a.W + (size_t)(c0 + c)) * a.C + ch;
    const float p = a.pred[g];
    float e = p;
    if (mix) {
      const float un = ub * a.noised[g];
      const float vp = vb * p;
      e = un + vp;
    }
    se[r * MHALO + c] = e;
    sx[r * MHALO + c] = a.x[g];
  }
  __syncthreads();

  double acc_d = 0.0;                                                          // the same loop with and without the filter
  for (int idx = tid; idx < own_h * own_w; idx += 256) {
    const int r = idx / own_w, c = idx - r * own_w;
    const float d = sx[r * MHALO + c] - se[r * MHALO + c];
    acc_d += (double)d * (double)d;
  }

  double acc_s = 0.0;
  if (noh) {
    for (int idx = tid; idx < hr * now; idx += 256) {                          // rows: F over j at every staged row
      const int r = idx / now, j = idx - r * now;
      const float* pe = se + r * MHALO + j;
      const float* px = sx + r * MHALO + j;
      double f0 = 0.0, f1 = 0.0, f2 = 0.0, f3 = 0.0, f4 = 0.0;
      for (int s = 0; s < K; s++) {
        const double w = sw[s], ea = (double)pe[s], xb = (double)px[s];
        f0 += w * ea;
        f1 += w * xb;
        f2 += w * (ea * ea);
        f3 += w * (xb * xb);
        f4 += w * (ea * xb);
      }
      const int o = r * MT + j;
      rows[0][o] = f0; rows[1][o] = f1; rows[2][o] = f2; rows[3][o] = f3; rows[4][o] = f4;
    }
    __syncthreads();
    for (int idx = tid; idx < noh * now; idx += 256) {                         // columns, then the map value
      const int i = idx / now, j = idx - i * now;
      double ma = 0.0, mb = 0.0, A = 0.0, Bq = 0.0, AB = 0.0;
      for (int r = 0; r < K; r++) {
        const double w = sw[r];
        const int o = (i + r) * MT + j;
        ma += w * rows[0][o];
        mb += w * rows[1][o];
        A += w * rows[2][o];
        Bq += w * rows[3][o];
        AB += w * rows[4][o];
      }
      const double mab = ma * mb, msq = ma * ma + mb * mb;
      const double lum = (2.0 * mab + a.C1) / (msq + a.C1);
      const double cs = ((2.0 * AB - 2.0 * mab) + a.C2) / (((A + Bq) - msq) + a.C2);
      acc_s += lum * cs;
    }
  }
  const double sd = block_sum256(acc_d, ws4);
  const double ss = block_sum256(acc_s, ws4);
  if (tid == 0) {
    const size_t B = gridDim.y, at = (size_t)b * a.nt + blockIdx.x;
    a.part[at] = ss;
    a.part[B * a.nt + at] = sd;
  }
}

// one work-group per image: the pairs of its tiles added in index order per thread, then over the threads
__global__ __launch_bounds__(256) void metrics_finish_kernel(const double* __restrict__ part, int nt, double n_img, double n_map, double peak2,
                                                             float* __restrict__ mse, float* __restrict__ psnr, float* __restrict__ ssim) {
  __shared__ double ws4[4];
  const size_t B = gridDim.x, b = blockIdx.x;
  const double* __restrict__ ps = part + b * nt;
  const double* __restrict__ pd = part + (B + b) * nt;
  double as = 0.0, ad = 0.0;
  for (int i = threadIdx.x; i < nt; i += 256) { as += ps[i]; ad += pd[i]; }
  const double sd = block_sum256(ad, ws4);
  const double ss = block_sum256(as, ws4);
  if (threadIdx.x == 0) {
    const double m = sd / n_img;
    mse[b] = (float)m;
    if (psnr) psnr[b] = m == 0.0 ? INFINITY : (float)(10.0 * log10(peak2 / m));
    if (ssim) ssim[b] = (float)(ss / n_map);
  }
}

}  // namespace

static int metrics_tiles(int H, int W, int C, int* tx, int* ty) {
  *tx = (W + MT - 1) / MT;
  *ty = (H + MT - 1) / MT;
  return *tx * *ty * C;
}

// one fp64 pair (four floats) per tile, channel and image
size_t image_metrics_scratch_floats(int B, int H, int W, int C) {
  int tx, ty;
  return 4 * (size_t)B * metrics_tiles(H, W, C, &tx, &ty);
}

int image_metrics(const float* pred, const float* noised, const float* u, const float* v, const float* x, const float* window, int K, float max_val,
                  float k1, float k2, float* mse, float* psnr, float* ssim, float* scratch, int B, int H, int W, int C, hipStream_t s) {
  static_assert(MT == GCT2_METRICS_TILE, "include/gct2.h names the tile");
  MetricsArgs a{};
  a.pred = pred; a.noised = noised; a.u = u; a.v = v; a.x = x; a.window = window;
  a.K = K; a.H = H; a.W = W; a.C = C; a.filter = ssim != nullptr;
  a.nt = metrics_tiles(H, W, C, &a.tiles_x, &a.tiles_y);
  const double c1 = (double)k1 * (double)max_val, c2 = (double)k2 * (double)max_val;
  a.C1 = c1 * c1; a.C2 = c2 * c2;
  a.part = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(metrics_tile_kernel, dim3(a.nt, B), dim3(256), 0, s, a);
  const double n_map = ssim ? (double)(H - K + 1) * (double)(W - K + 1) * C : 1.0;
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(B), dim3(256), 0, s, a.part, a.nt, (double)H * W * C, n_map, (double)max_val * (double)max_val,
                     mse, psnr, ssim);
  return gct2_check_launch("image_metrics");
}
