// The training losses of Trainer.call besides the plain MSE (train.py:254-280; include/gct2.h gct2_loss_fwd_bwd): L1, MSE plus the MSE of
// 16 x 16 average pools, and the frequency-weighted 2-D DCT loss.  Each kind leaves the scalar loss and, unless the caller passes
// dpred = NULL, its gradient with respect to the prediction.
//
// No floating-point atomics anywhere: every work-group leaves fp64 partial sums in the caller's scratch (summed over the threads in a
// fixed order), one small launch adds them in index order and forms the loss in double - the bits depend on the inputs alone.  The
// pointwise arithmetic is fp32 without contraction (every product and sum rounds on its own, as an unfused TensorFlow op chain does).
//
// The DCT loss is four fp32 matrix products per [size, size] plane - E = G D G^T forward, V = G^T E G back - on the fp32-input matrix
// cores (v_mfma_f32_16x16x4_f32) with the conventions of f32_mfma.hip: one work-group = 4 waves = a 128 x 128 output tile, a reduction
// stage = 16 elements staged k-major through LDS rows padded to 144 floats, global loads of stage s + 1 issued before the MFMAs of
// stage s.  A pass is out[img][m][n] = sum_k A[m][k] X[img][k][n] with A = G or G^T and n running over (line, channel) pairs of the
// image: the column pass reduces over h (X rows are W*C contiguous floats), the row pass over w (a stride-C gather on the reduction
// index).  Rows, columns and reduction elements beyond `size` are staged as zeros and add exact zeros.
//
// gct2_eval_loss_rows (evaluation: the same four losses PER IMAGE, without gradients) lives here too: it forms the residual from the
// prediction, the clean image and the noise on load, keeps every partial sum inside one image, and reuses the two forward DCT passes.
//
// gct2_objective_loss_fwd_bwd (the MSE / L1 training loss with per-image weights) is that per-image kernel with the gradient store of
// the kinds above: the target is formed on load, the loss is sum_b lam[b] S_b / n from the same fp64 partial sums.
#include "gct2_common.h"
#include <algorithm>

namespace {

constexpr int LBM = 128, LBN = 128, LBK = 16, LLD = 144;     // tile rows / columns, reduction elements per stage, LDS row (floats)
constexpr int LOSS_PARTIALS = 1024;                          // floats at the head of the scratch every kind may use for its partial sums

__device__ __forceinline__ f32x4_t mfma_f32(float a, float b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// four consecutive floats; `vec`: the address is 16-byte aligned.  Both forms read the same elements: a launch computes the same bits
// whatever the alignment of its operands
__device__ __forceinline__ f32x4_t ld4(const float* src, bool vec) {
  if (vec) return *reinterpret_cast<const f32x4_t*>(src);
  return f32x4_t{src[0], src[1], src[2], src[3]};
}
__device__ __forceinline__ void st4(float* dst, f32x4_t v, bool vec) {
  if (vec) { *reinterpret_cast<f32x4_t*>(dst) = v; return; }
  dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
}

// sum of one double per thread over the 256 threads of a work-group, in a fixed order; every thread receives it
__device__ __forceinline__ double block_sum(double acc, double* ws4) {
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __syncthreads();                                   // (ws4 may still be read from an earlier sum)
  if ((threadIdx.x & 63) == 0) ws4[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((ws4[0] + ws4[1]) + ws4[2]) + ws4[3];
}

// loss = (float)(S1 / dn [+ S2 / dn2]); S1 = part[0, n1), S2 = part[n1, n1 + n2) added in index order per thread, then over the threads
__global__ __launch_bounds__(256) void loss_finish_kernel(const double* __restrict__ part, int n1, int n2, double dn, double dn2,
                                                          float* __restrict__ loss) {
#pragma clang fp contract(off)
  __shared__ double ws4[4];
  double a1 = 0.0, a2 = 0.0;
  for (int i = threadIdx.x; i < n1; i += 256) a1 += part[i];
  for (int i = threadIdx.x; i < n2; i += 256) a2 += part[n1 + i];
  const double s1 = block_sum(a1, ws4);
  const double s2 = block_sum(a2, ws4);
  if (threadIdx.x == 0) {
    const double q1 = s1 / dn;
    *loss = n2 ? (float)(q1 + s2 / dn2) : (float)q1;
  }
}

// ---- L1 (train.py:268-270): maximum(t - p, p - t), TF's _MaximumGrad sends a tie to the first operand and a NaN to the second ----
__global__ __launch_bounds__(256) void l1_kernel(const float* __restrict__ pred, const float* __restrict__ target, float* __restrict__ dpred,
                                                 double* __restrict__ partials, size_t n, float c, const float* __restrict__ loss_scale_ptr,
                                                 int vec) {
#pragma clang fp contract(off)
  __shared__ double ws4[4];
  const float s = loss_scale_ptr ? *loss_scale_ptr : 1.f;
  const size_t n4 = n >> 2, stride = (size_t)gridDim.x * 256, gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  double acc = 0.0;
  for (size_t q = gid; q < n4; q += stride) {
    const f32x4_t p = ld4(pred + 4 * q, vec), t = ld4(target + 4 * q, vec);
    f32x4_t g;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float d = t[j] - p[j], nd = -d;
      const bool first = d >= nd;
      acc += (double)(first ? d : nd);
      g[j] = s * (first ? -c : c);
    }
    if (dpred) st4(dpred + 4 * q, g, vec);
  }
  if (gid < n - 4 * n4) {                            // the last n % 4 elements: threads 0 .. 2 of work-group 0
    const size_t i = 4 * n4 + gid;
    const float d = target[i] - pred[i], nd = -d;
    const bool first = d >= nd;
    acc += (double)(first ? d : nd);
    if (dpred) dpred[i] = s * (first ? -c : c);
  }
  const double sum = block_sum(acc, ws4);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// ---- MSE + MSE of the 16 x 16 average pools (train.py:274-280): one work-group per cell, d stays in registers for the gradient ----
// a cell row is 16*C contiguous floats = 4C groups of four; thread (row r, group q) holds elements 4q .. 4q+3 of row r, channel (4q + j) % C
__global__ __launch_bounds__(256) void pooled_kernel(const float* __restrict__ pred, const float* __restrict__ target, float* __restrict__ dpred,
                                                     double* __restrict__ partials, int H, int W, int C, int ncells, float c1, float c2,
                                                     const float* __restrict__ loss_scale_ptr, int vec) {
#pragma clang fp contract(off)
  __shared__ float ds[16][64];
  __shared__ double col[64];
  __shared__ float qs[4];
  __shared__ double ws4[4];
  const int tid = threadIdx.x, cell = blockIdx.x;
  const int cw = W >> 4, chh = H >> 4;
  const int cx = cell % cw, cy = (cell / cw) % chh, b = cell / (cw * chh);
  const int groups = 4 * C;
  const bool active = tid < 16 * groups;
  const int r = tid / groups, q = tid - r * groups;
  const size_t base = (((size_t)b * H + (size_t)cy * 16 + r) * W + (size_t)cx * 16) * C + 4 * q;
  f32x4_t d = {0.f, 0.f, 0.f, 0.f};
  double acc = 0.0;
  if (active) {
    const f32x4_t p = ld4(pred + base, vec), t = ld4(target + base, vec);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      d[j] = t[j] - p[j];
      ds[r][4 * q + j] = d[j];
      acc += (double)d[j] * (double)d[j];
    }
  }
  __syncthreads();
  if (tid < 16 * C) {                                // rows first ...
    double s = 0.0;
    for (int rr = 0; rr < 16; rr++) s += (double)ds[rr][tid];
    col[tid] = s;
  }
  __syncthreads();
  if (tid < C) {                                     // ... then the 16 pixels of the row, ascending
    double s = 0.0;
    for (int x = 0; x < 16; x++) s += col[x * C + tid];
    qs[tid] = (float)s;
  }
  const double s1 = block_sum(acc, ws4);             // (its barriers also publish qs)
  if (tid == 0) {
    double s2 = 0.0;
    for (int c = 0; c < C; c++) {
      const double m = (double)qs[c] / 256.0;
      s2 += m * m;
    }
    partials[cell] = s1;
    partials[ncells + cell] = s2;
  }
  if (active && dpred) {
    const float s = loss_scale_ptr ? *loss_scale_ptr : 1.f;
    f32x4_t g;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float a = d[j] * c1, e = qs[(4 * q + j) % C] * c2;
      g[j] = s * (a + e);
    }
    st4(dpred + base, g, vec);
  }
}

// ---- DCT passes ----------------------------------------------------------------------------------------------------------------
struct DctPass {
  const float* G; int S;            // basis [S][S] row-major, 16-byte aligned; S a multiple of 4
  int at;                           // 0: A[m][k] = G[m][k];  1: A[m][k] = G[k][m]
  const float* x; const float* xsub;    // X = x, or x - xsub when xsub is set (the first pass forms d = target - pred on load)
  float* out;                       // null: nothing is stored (the loss-only call needs E's squares, not E)
  int C, N;                         // channels, columns of X per image (S * C)
  int sk, rs;                       // element (k, n) of an image lies at k * sk + (n / C) * rs + n % C; the output (m, n) likewise
  double* partials;                 // one sum of out^2 per work-group, or null
  float c1; const float* ls; int scale;     // scale: out = s * (acc * c1), s = *ls or 1
  int xvec;                         // X rows are contiguous in n and every source is 16-byte aligned
  int m_tiles, n_tiles;
};

__global__ __launch_bounds__(256) void dct_pass_kernel(DctPass p) {
#pragma clang fp contract(off)
  __shared__ float As[LBK * LLD], Bs[LBK * LLD];
  __shared__ double ws4[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int S = p.S, N = p.N, C = p.C;
  const int mt = blockIdx.x % p.m_tiles, nt = (blockIdx.x / p.m_tiles) % p.n_tiles, img = blockIdx.x / (p.m_tiles * p.n_tiles);
  const int m0 = mt * LBM, n0 = nt * LBN;
  const size_t ibase = (size_t)img * S * N;
  const float* __restrict__ x = p.x + ibase;
  const float* __restrict__ xs = p.xsub ? p.xsub + ibase : nullptr;
  const float* __restrict__ G = p.G;
  // this thread's two B groups: reduction row e / 32 of the stage, columns n0 + 4 (e % 32) .. + 3 (e = tid + 256 g); their offsets
  // inside an image row set do not change from stage to stage (-1: beyond N)
  int boff[2][4];
#pragma unroll
  for (int g = 0; g < 2; g++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int n = n0 + 4 * ((tid + 256 * g) & 31) + j;
      boff[g][j] = n < N ? (n / C) * p.rs + n % C : -1;
    }
  f32x4_t ra[2], rb[2];
  auto load_stage = [&](int k0) {
#pragma unroll
    for (int g = 0; g < 2; g++) {
      const int e = tid + 256 * g;
      f32x4_t v = {0.f, 0.f, 0.f, 0.f};
      if (!p.at) {                    // G[m][k]: 4 consecutive k of row m
        const int m = m0 + (e >> 2), k = k0 + 4 * (e & 3);
        if (m < S && k < S) v = *reinterpret_cast<const f32x4_t*>(G + (size_t)m * S + k);
      } else {                        // G[k][m]: 4 consecutive m of row k
        const int k = k0 + (e >> 5), m = m0 + 4 * (e & 31);
        if (k < S && m < S) v = *reinterpret_cast<const f32x4_t*>(G + (size_t)k * S + m);
      }
      ra[g] = v;
    }
#pragma unroll
    for (int g = 0; g < 2; g++) {
      const int k = k0 + ((tid + 256 * g) >> 5);
      f32x4_t v = {0.f, 0.f, 0.f, 0.f};
      if (k < S) {
        const size_t row = (size_t)k * p.sk;
        if (p.xvec) {                 // (N is a multiple of 4: a group is inside or outside as a whole)
          if (boff[g][0] >= 0) {
            v = *reinterpret_cast<const f32x4_t*>(x + row + boff[g][0]);
            if (xs) v -= *reinterpret_cast<const f32x4_t*>(xs + row + boff[g][0]);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (boff[g][j] >= 0) v[j] = xs ? x[row + boff[g][j]] - xs[row + boff[g][j]] : x[row + boff[g][j]];
        }
      }
      rb[g] = v;
    }
  };
  auto store_stage = [&]() {
#pragma unroll
    for (int g = 0; g < 2; g++) {
      const int e = tid + 256 * g;
      if (!p.at) {
#pragma unroll
        for (int j = 0; j < 4; j++) As[(4 * (e & 3) + j) * LLD + (e >> 2)] = ra[g][j];
      } else {
        *reinterpret_cast<f32x4_t*>(&As[(e >> 5) * LLD + 4 * (e & 31)]) = ra[g];
      }
      *reinterpret_cast<f32x4_t*>(&Bs[(e >> 5) * LLD + 4 * (e & 31)]) = rb[g];
    }
  };
  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  load_stage(0);
  for (int k0 = 0; k0 < S; k0 += LBK) {
    __syncthreads();
    store_stage();
    __syncthreads();
    const int nkg = min(4, (S - k0) >> 2);           // whole k-groups of 4 (S is a multiple of 4)
    if (k0 + LBK < S) load_stage(k0 + LBK);
    for (int kk = 0; kk < nkg; kk++) {
      const int k = kk * 4 + (lane >> 4);
      float a[4], bb[4];
#pragma unroll
      for (int i = 0; i < 4; i++) a[i] = As[k * LLD + wm * 64 + i * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 4; j++) bb[j] = Bs[k * LLD + wn * 64 + j * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = mfma_f32(a[i], bb[j], acc[i][j]);
    }
  }
  // D layout: row 4 (lane >> 4) + r, column lane & 15 of each 16 x 16 tile
  const float s = (p.scale && p.ls) ? *p.ls : 1.f;
  float* __restrict__ out = p.out ? p.out + ibase : nullptr;
  double sq = 0.0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int n = n0 + wn * 64 + j * 16 + (lane & 15);
    if (n >= N) continue;
    const size_t noff = (size_t)(n / C) * p.rs + n % C;
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int m = m0 + wm * 64 + i * 16 + 4 * (lane >> 4) + r;
        if (m >= S) continue;
        float v = acc[i][j][r];
        if (p.scale) { v = v * p.c1; v = s * v; }
        sq += (double)v * (double)v;
        if (out) out[(size_t)m * p.sk + noff] = v;
      }
    }
  }
  if (p.partials) {
    const double sum = block_sum(sq, ws4);
    if (tid == 0) p.partials[blockIdx.x] = sum;
  }
}

inline size_t round4(size_t v) { return (v + 3) / 4 * 4; }
inline int dct_tiles(int S, int C, int* mt, int* nt) {
  *mt = (S + LBM - 1) / LBM;
  *nt = (S * C + LBN - 1) / LBN;
  return *mt * *nt;
}

// ---- the per-image losses of gct2_eval_loss_rows (Trainer.evaluate) ---------------------------------------------------------------
// The residual is formed on load from the prediction, the clean image and the noise: target = x | a[b] x | a[b] x + c[b] eps (the
// rule of mix_per_image_kernel), p = pred | w[b] pred, d = target - p, every operation rounded on its own.  Neither target nor p is
// stored.  blockIdx.y (or the cell / tile index) fixes the image of a work-group: no partial sum mixes two images.
struct EvalSrc {
  const float* pred; const float* x; const float* eps;      // eps: null when the target has no noise term
  const float* a; const float* c; const float* w;           // per-image coefficients, each may be null
};
struct EvalCoef { float a, c, w; bool has_a, has_eps, has_w; };

__device__ __forceinline__ EvalCoef eval_coef(const EvalSrc& s, int b) {
  EvalCoef k;
  k.has_a = s.a != nullptr; k.has_eps = k.has_a && s.eps != nullptr; k.has_w = s.w != nullptr;
  k.a = k.has_a ? s.a[b] : 1.f; k.c = k.has_eps ? s.c[b] : 0.f; k.w = k.has_w ? s.w[b] : 1.f;
  return k;
}
__device__ __forceinline__ float eval_d(const EvalCoef& k, float p, float x, float e) {
#pragma clang fp contract(off)
  float t = x;
  if (k.has_a) {
    t = k.a * x;
    if (k.has_eps) { const float ce = k.c * e; t = t + ce; }
  }
  const float pp = k.has_w ? k.w * p : p;
  return t - pp;
}

constexpr int EVAL_MAX_CHUNKS = 64;        // work-groups per image at most (MSE, L1, the DCT's residual plane)
constexpr int EVAL_GROUPS = 4;             // 16-byte groups per thread a chunk is sized for
inline int eval_chunks(size_t n_img) {
  const size_t per = (size_t)256 * EVAL_GROUPS * 4;
  return (int)std::min<size_t>(EVAL_MAX_CHUNKS, std::max<size_t>(1, (n_img + per - 1) / per));
}

// KIND 0: sum d^2; 1: sum max(d, -d); 2: d is stored to dout ([B, n_img], the DCT's input plane) and nothing is summed.
// grid = (chunks, B).  An image starts at element b * n_img, 16-byte aligned or not: with `vec` (every base pointer is 16-byte aligned)
// the first (4 - b n_img % 4) % 4 elements and the last few are read one by one by the first threads of chunk 0 and everything between
// them in aligned groups of four; without it the groups start at the image's first element and are read element by element.
template <int KIND>
__global__ __launch_bounds__(256) void eval_rows_kernel(EvalSrc s, float* __restrict__ dout, double* __restrict__ partials, int n_img, int vec) {
#pragma clang fp contract(off)
  __shared__ double ws4[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const size_t base = (size_t)b * n_img;
  const EvalCoef k = eval_coef(s, b);
  const float* __restrict__ pp = s.pred + base;
  const float* __restrict__ xp = s.x + base;
  const float* __restrict__ ep = k.has_eps ? s.eps + base : nullptr;
  float* __restrict__ op = KIND == 2 ? dout + base : nullptr;
  const int head = vec ? min(n_img, (int)((4 - (base & 3)) & 3)) : 0;
  const int n4 = (n_img - head) >> 2, rest = n_img - head - 4 * n4;
  const int per = (n4 + gridDim.x - 1) / gridDim.x;
  const int q1 = min(n4, ((int)blockIdx.x + 1) * per);
  double acc = 0.0;
  auto term = [&](float d) {
    if (KIND == 0) acc += (double)d * (double)d;
    if (KIND == 1) { const float nd = -d; acc += (double)(d >= nd ? d : nd); }
  };
  for (int q = blockIdx.x * per + tid; q < q1; q += 256) {
    const int i = head + 4 * q;
    const f32x4_t p = ld4(pp + i, vec), x = ld4(xp + i, vec);
    const f32x4_t e = ep ? ld4(ep + i, vec) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    f32x4_t d;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      d[j] = eval_d(k, p[j], x[j], e[j]);
      term(d[j]);
    }
    if (KIND == 2) st4(op + i, d, vec);
  }
  if (blockIdx.x == 0 && tid < head + rest) {        // at most 6 elements: the unaligned head and the last n % 4
    const int i = tid < head ? tid : 4 * n4 + tid;
    const float d = eval_d(k, pp[i], xp[i], ep ? ep[i] : 0.f);
    term(d);
    if (KIND == 2) op[i] = d;
  }
  if (KIND != 2) {
    const double sum = block_sum(acc, ws4);
    if (tid == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = sum;
  }
}

// pooled MSE per image: pooled_kernel's cell layout (one work-group per 16 x 16 cell, thread = (row, group of four)), loss only, the
// cell sums kept in fp64.  partials[cell] = sum d^2, partials[ncells + cell] = sum over channels of (qsum / 256)^2
__global__ __launch_bounds__(256) void eval_pooled_kernel(EvalSrc s, double* __restrict__ partials, int H, int W, int C, int ncells, int vec) {
#pragma clang fp contract(off)
  __shared__ float ds[16][64];
  __shared__ double col[64];
  __shared__ double qs[4];
  __shared__ double ws4[4];
  const int tid = threadIdx.x, cell = blockIdx.x;
  const int cw = W >> 4, chh = H >> 4;
  const int cx = cell % cw, cy = (cell / cw) % chh, b = cell / (cw * chh);
  const EvalCoef k = eval_coef(s, b);
  const int groups = 4 * C;
  const bool active = tid < 16 * groups;
  const int r = tid / groups, q = tid - r * groups;
  const size_t base = (((size_t)b * H + (size_t)cy * 16 + r) * W + (size_t)cx * 16) * C + 4 * q;
  double acc = 0.0;
  if (active) {
    const f32x4_t p = ld4(s.pred + base, vec), x = ld4(s.x + base, vec);
    const f32x4_t e = k.has_eps ? ld4(s.eps + base, vec) : f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float d = eval_d(k, p[j], x[j], e[j]);
      ds[r][4 * q + j] = d;
      acc += (double)d * (double)d;
    }
  }
  __syncthreads();
  if (tid < 16 * C) {                                // rows first ...
    double sum = 0.0;
    for (int rr = 0; rr < 16; rr++) sum += (double)ds[rr][tid];
    col[tid] = sum;
  }
  __syncthreads();
  if (tid < C) {                                     // ... then the 16 pixels of the row, ascending
    double sum = 0.0;
    for (int x = 0; x < 16; x++) sum += col[x * C + tid];
    qs[tid] = sum;
  }
  const double s1 = block_sum(acc, ws4);             // (its barriers also publish qs)
  if (tid == 0) {
    double s2 = 0.0;
    for (int c = 0; c < C; c++) {
      const double m = qs[c] / 256.0;
      s2 += m * m;
    }
    partials[cell] = s1;
    partials[ncells + cell] = s2;
  }
}

// rows[b] = (float)(S1 / dn [+ S2 / dn2]) with S1 = part[b n1, (b + 1) n1) and S2 = part[off2 + b n2, off2 + (b + 1) n2), each added
// in index order per thread and then over the threads (loss_finish_kernel per image): one work-group per image
__global__ __launch_bounds__(256) void eval_finish_kernel(const double* __restrict__ part, int n1, int n2, size_t off2, double dn, double dn2,
                                                          float* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ double ws4[4];
  const double* __restrict__ p1 = part + (size_t)blockIdx.x * n1;
  const double* __restrict__ p2 = part + off2 + (size_t)blockIdx.x * n2;
  double a1 = 0.0, a2 = 0.0;
  for (int i = threadIdx.x; i < n1; i += 256) a1 += p1[i];
  for (int i = threadIdx.x; i < n2; i += 256) a2 += p2[i];
  const double s1 = block_sum(a1, ws4);
  const double s2 = block_sum(a2, ws4);
  if (threadIdx.x == 0) {
    const double q1 = s1 / dn;
    rows[blockIdx.x] = n2 ? (float)(q1 + s2 / dn2) : (float)q1;
  }
}

// ---- gct2_objective_loss_fwd_bwd: the weighted training loss of an objective and its gradient in one pass ---------------------------
// eval_rows_kernel's mapping (grid = (chunks, B), the unaligned head and the last n % 4 elements with the first threads of chunk 0) and
// its residual d = eval_d(...); besides the fp64 partial sum of the image's loss every element leaves its gradient:
//   KIND 0 (MSE): dpred = s * ((d * k) * g);   KIND 1 (L1): dpred = s * ((d >= -d ? -k : k) * g);   without g (HAS_G false) the product
// with g is not formed at all.  g = lam[b] * w[b], lam[b] or w[b].  dpred == nullptr: the loss only
template <int KIND>
__global__ __launch_bounds__(256) void objective_loss_kernel(EvalSrc s, const float* __restrict__ lam, float* __restrict__ dpred,
                                                             double* __restrict__ partials, int n_img, float kf,
                                                             const float* __restrict__ loss_scale_ptr, int vec) {
#pragma clang fp contract(off)
  __shared__ double ws4[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const size_t base = (size_t)b * n_img;
  const EvalCoef k = eval_coef(s, b);
  const bool has_g = lam != nullptr || k.has_w;                 // (block-uniform)
  const float g = lam ? (k.has_w ? lam[b] * k.w : lam[b]) : k.w;
  const float ls = loss_scale_ptr ? *loss_scale_ptr : 1.f;
  const float* __restrict__ pp = s.pred + base;
  const float* __restrict__ xp = s.x + base;
  const float* __restrict__ ep = k.has_eps ? s.eps + base : nullptr;
  float* __restrict__ op = dpred ? dpred + base : nullptr;
  const int head = vec ? min(n_img, (int)((4 - (base & 3)) & 3)) : 0;
  const int n4 = (n_img - head) >> 2, rest = n_img - head - 4 * n4;
  const int per = (n4 + gridDim.x - 1) / gridDim.x;
  const int q1 = min(n4, ((int)blockIdx.x + 1) * per);
  double acc = 0.0;
  auto element = [&](float d) -> float {                        // adds the loss term, returns the gradient
#pragma clang fp contract(off)
    float t;
    if (KIND == 0) {
      acc += (double)d * (double)d;
      t = d * kf;
    } else {
      const float nd = -d;
      const bool first = d >= nd;
      acc += (double)(first ? d : nd);
      t = first ? -kf : kf;
    }
    if (has_g) t = t * g;
    return ls * t;
  };
  for (int q = blockIdx.x * per + tid; q < q1; q += 256) {
    const int i = head + 4 * q;
    const f32x4_t p = ld4(pp + i, vec), x = ld4(xp + i, vec);
    const f32x4_t e = ep ? ld4(ep + i, vec) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    f32x4_t gr;
#pragma unroll
    for (int j = 0; j < 4; j++) gr[j] = element(eval_d(k, p[j], x[j], e[j]));
    if (op) st4(op + i, gr, vec);
  }
  if (blockIdx.x == 0 && tid < head + rest) {        // at most 6 elements: the unaligned head and the last n % 4
    const int i = tid < head ? tid : 4 * n4 + tid;
    const float gr = element(eval_d(k, pp[i], xp[i], ep ? ep[i] : 0.f));
    if (op) op[i] = gr;
  }
  const double sum = block_sum(acc, ws4);
  if (tid == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = sum;
}

// loss = (float)(sum_b (double)lam[b] * S_b / dn): S_b = part[b chunks, (b + 1) chunks) added in index order, the images in index order
// per thread (b = tid, tid + 256, ..) and then over the threads; lam == nullptr: every weight is 1
__global__ __launch_bounds__(256) void objective_finish_kernel(const double* __restrict__ part, const float* __restrict__ lam, int B, int chunks,
                                                               double dn, float* __restrict__ loss) {
#pragma clang fp contract(off)
  __shared__ double ws4[4];
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const double* __restrict__ p = part + (size_t)b * chunks;
    double sb = 0.0;
    for (int i = 0; i < chunks; i++) sb += p[i];
    acc += lam ? (double)lam[b] * sb : sb;
  }
  const double total = block_sum(acc, ws4);
  if (threadIdx.x == 0) *loss = (float)(total / dn);
}

}  // namespace

// floats of scratch a kind needs: the partial sums (fp64, two floats each) and, for the DCT, one [B,H,W,C] plane set behind them
int loss_scratch_floats(int kind, int B, int H, int W, int C, size_t* partial_floats, size_t* floats) {
  const size_t n = (size_t)B * H * W * C;
  size_t part = LOSS_PARTIALS, total = LOSS_PARTIALS;
  if (kind == GCT2_LOSS_MSE_POOLED) {
    part = total = std::max<size_t>(LOSS_PARTIALS, round4(4 * (size_t)B * (H / 16) * (W / 16)));
  } else if (kind == GCT2_LOSS_DCT) {
    int mt, nt;
    part = std::max<size_t>(LOSS_PARTIALS, round4(2 * (size_t)B * dct_tiles(H, C, &mt, &nt)));
    total = part + round4(n);
  }
  if (partial_floats) *partial_floats = part;
  *floats = total;
  return GCT2_OK;
}

int loss_l1(const float* pred, const float* target, float* dpred, float* loss, float* scratch, size_t n, const float* ls, hipStream_t s) {
  const size_t n4 = n / 4;
  const int nb = (int)std::min<size_t>(LOSS_PARTIALS / 2, std::max<size_t>(1, (n4 + 255) / 256));
  const int vec = !(((uintptr_t)pred | (uintptr_t)target | (uintptr_t)dpred) % 16);
  double* part = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(l1_kernel, dim3(nb), dim3(256), 0, s, pred, target, dpred, part, n, (float)(1.0 / (double)n), ls, vec);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, part, nb, 0, (double)n, 0.0, loss);
  return gct2_check_launch("loss_fwd_bwd (l1)");
}

int loss_pooled(const float* pred, const float* target, float* dpred, float* loss, float* scratch, int B, int H, int W, int C, const float* ls,
                hipStream_t s) {
  const size_t n = (size_t)B * H * W * C, cells = (size_t)B * (H / 16) * (W / 16);
  const double n2 = (double)cells * C;
  // (a cell row starts at a multiple of 16*C floats: the 16-byte groups are aligned whenever the tensors are)
  const int vec = !(((uintptr_t)pred | (uintptr_t)target | (uintptr_t)dpred) % 16);
  double* part = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(pooled_kernel, dim3((unsigned)cells), dim3(256), 0, s, pred, target, dpred, part, H, W, C, (int)cells,
                     (float)(-2.0 / (double)n), (float)(-2.0 / (65536.0 * n2)), ls, vec);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, part, (int)cells, (int)cells, (double)n, n2, loss);
  return gct2_check_launch("loss_fwd_bwd (mse_pooled)");
}

int loss_dct(const float* pred, const float* target, float* dpred, float* loss, float* scratch, int B, int S, int C, const float* basis,
             const float* ls, hipStream_t s) {
  const size_t n = (size_t)B * S * S * C;
  size_t part_floats, total;
  loss_scratch_floats(GCT2_LOSS_DCT, B, S, S, C, &part_floats, &total);
  double* part = reinterpret_cast<double*>(scratch);
  float* plane = scratch + part_floats;
  DctPass p{};
  p.G = basis; p.S = S; p.C = C; p.N = S * C;
  const int tiles = dct_tiles(S, C, &p.m_tiles, &p.n_tiles);
  const int nblocks = B * tiles;
  const bool aligned = !(((uintptr_t)pred | (uintptr_t)target | (uintptr_t)dpred) % 16);
  auto pass = [&](int at, bool column, const float* x, const float* xsub, float* out, double* partials, int scale) {
    DctPass q = p;
    q.at = at; q.x = x; q.xsub = xsub; q.out = out; q.partials = partials; q.scale = scale;
    q.c1 = (float)(-2.0 / (double)n); q.ls = ls;
    q.sk = column ? S * C : C;
    q.rs = column ? C : S * C;
    q.xvec = column && aligned;
    hipLaunchKernelGGL(dct_pass_kernel, dim3(nblocks), dim3(256), 0, s, q);
  };
  pass(0, true, target, pred, plane, nullptr, 0);                 // T = G d        (over h)
  pass(0, false, plane, nullptr, dpred, part, 0);                 // E = T G^T      (over w), sum E^2
  if (dpred) {
    pass(1, false, dpred, nullptr, plane, nullptr, 0);            // U = E G        (over the second frequency index)
    pass(1, true, plane, nullptr, dpred, nullptr, 1);             // V = G^T U      (over the first), dpred = s * (V * c1)
  }
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, part, nblocks, 0, (double)n, 0.0, loss);
  return gct2_check_launch("loss_fwd_bwd (dct)");
}

// ---- gct2_eval_loss_rows --------------------------------------------------------------------------------------------------------
// scratch: the fp64 partial sums (two floats each) and, for the DCT, the residual plane and the plane of the first pass behind them
static size_t eval_partial_floats(int kind, int B, int H, int W, int C) {
  if (kind == GCT2_LOSS_MSE_POOLED) return round4(4 * (size_t)B * (H / 16) * (W / 16));
  if (kind == GCT2_LOSS_DCT) {
    int mt, nt;
    return round4(2 * (size_t)B * dct_tiles(H, C, &mt, &nt));
  }
  return round4(2 * (size_t)B * eval_chunks((size_t)H * W * C));
}
size_t eval_scratch_floats(int kind, int B, int H, int W, int C) {
  const size_t part = eval_partial_floats(kind, B, H, W, C);
  return kind == GCT2_LOSS_DCT ? part + 2 * round4((size_t)B * H * W * C) : part;
}

int eval_loss_rows(int kind, const float* pred, const float* x, const float* eps, const float* a, const float* c, const float* w, float* rows,
                   float* scratch, int B, int H, int W, int C, const float* basis, hipStream_t s) {
  const int n_img = H * W * C;
  const EvalSrc src{pred, x, a ? eps : nullptr, a, c, w};
  const int vec = !(((uintptr_t)pred | (uintptr_t)x | (uintptr_t)src.eps) % 16);
  double* part = reinterpret_cast<double*>(scratch);
  const int chunks = eval_chunks((size_t)n_img);
  if (kind == GCT2_LOSS_MSE || kind == GCT2_LOSS_L1) {
    if (kind == GCT2_LOSS_MSE) hipLaunchKernelGGL(eval_rows_kernel<0>, dim3(chunks, B), dim3(256), 0, s, src, nullptr, part, n_img, vec);
    else hipLaunchKernelGGL(eval_rows_kernel<1>, dim3(chunks, B), dim3(256), 0, s, src, nullptr, part, n_img, vec);
    hipLaunchKernelGGL(eval_finish_kernel, dim3(B), dim3(256), 0, s, part, chunks, 0, (size_t)0, (double)n_img, 0.0, rows);
    return gct2_check_launch(kind == GCT2_LOSS_MSE ? "eval_loss_rows (mse)" : "eval_loss_rows (l1)");
  }
  if (kind == GCT2_LOSS_MSE_POOLED) {
    const int cpi = (H / 16) * (W / 16), cells = B * cpi;
    hipLaunchKernelGGL(eval_pooled_kernel, dim3((unsigned)cells), dim3(256), 0, s, src, part, H, W, C, cells, vec);
    hipLaunchKernelGGL(eval_finish_kernel, dim3(B), dim3(256), 0, s, part, cpi, cpi, (size_t)cells, (double)n_img, (double)cpi * C, rows);
    return gct2_check_launch("eval_loss_rows (mse_pooled)");
  }
  // DCT: d -> scratch, T = G d (over h) -> scratch, E = T G^T (over w) summed per tile; loss_dct's first two passes
  const int S = H;
  const size_t n = (size_t)B * n_img;
  float* dplane = scratch + eval_partial_floats(kind, B, H, W, C);
  float* tplane = dplane + round4(n);
  hipLaunchKernelGGL(eval_rows_kernel<2>, dim3(chunks, B), dim3(256), 0, s, src, dplane, nullptr, n_img, vec);
  DctPass p{};
  p.G = basis; p.S = S; p.C = C; p.N = S * C; p.at = 0; p.xsub = nullptr; p.scale = 0; p.c1 = 0.f; p.ls = nullptr;
  const int tiles = dct_tiles(S, C, &p.m_tiles, &p.n_tiles);
  DctPass col = p, row = p;
  col.x = dplane; col.out = tplane; col.partials = nullptr; col.sk = S * C; col.rs = C; col.xvec = 1;
  row.x = tplane; row.out = nullptr; row.partials = part; row.sk = C; row.rs = S * C; row.xvec = 0;
  hipLaunchKernelGGL(dct_pass_kernel, dim3(B * tiles), dim3(256), 0, s, col);
  hipLaunchKernelGGL(dct_pass_kernel, dim3(B * tiles), dim3(256), 0, s, row);
  hipLaunchKernelGGL(eval_finish_kernel, dim3(B), dim3(256), 0, s, part, tiles, 0, (size_t)0, (double)n_img, 0.0, rows);
  return gct2_check_launch("eval_loss_rows (dct)");
}

// ---- gct2_objective_loss_fwd_bwd -------------------------------------------------------------------------------------------------
// scratch: one fp64 partial sum (two floats) per (image, chunk) of eval_rows_kernel's grid
size_t objective_scratch_floats(int B, int H, int W, int C) {
  return std::max<size_t>(4, round4(2 * (size_t)B * eval_chunks((size_t)H * W * C)));
}

int objective_loss(int kind, const float* pred, const float* x, const float* eps, const float* a, const float* c, const float* w,
                   const float* lam, float* dpred, float* loss, float* scratch, int B, int H, int W, int C, const float* ls, hipStream_t s) {
  const int n_img = H * W * C;
  const double dn = (double)B * (double)n_img;
  const EvalSrc src{pred, x, a ? eps : nullptr, a, c, w};
  const int vec = !(((uintptr_t)pred | (uintptr_t)x | (uintptr_t)src.eps | (uintptr_t)dpred) % 16);
  double* part = reinterpret_cast<double*>(scratch);
  const int chunks = eval_chunks((size_t)n_img);
  if (kind == GCT2_LOSS_MSE)
    hipLaunchKernelGGL(objective_loss_kernel<0>, dim3(chunks, B), dim3(256), 0, s, src, lam, dpred, part, n_img, (float)(-2.0 / dn), ls, vec);
  else
    hipLaunchKernelGGL(objective_loss_kernel<1>, dim3(chunks, B), dim3(256), 0, s, src, lam, dpred, part, n_img, (float)(1.0 / dn), ls, vec);
  hipLaunchKernelGGL(objective_finish_kernel, dim3(1), dim3(256), 0, s, part, lam, B, chunks, dn, loss);
  return gct2_check_launch(kind == GCT2_LOSS_MSE ? "objective_loss_fwd_bwd (mse)" : "objective_loss_fwd_bwd (l1)");
}
