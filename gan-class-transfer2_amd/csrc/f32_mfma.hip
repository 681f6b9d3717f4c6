// fp32 tap GEMMs and weight gradients of the 4x4 / stride-2 layers and of the 'same' stride-1 convolutions (ks x ks, ks odd <= 7:
// Block's 3x3, the 1x1 projection) on the fp32-input matrix cores (v_mfma_f32_16x16x4_f32): the reference's default arithmetic
// (train.py:34,38: mixed_precision = False) at the MFMA rate instead of one thread per output (direct_kernels.hip).  Selected per call
// context (gct2_ctx_set_f32_math); the direct kernels stay the default and the reference.
//
// One work-group = 4 waves = a 128 x BN output tile (BN = 128, or 64 for narrow outputs), each wave 64 x BN/2 = 4 x BN/32 MFMA tiles
// of 16 x 16.  A reduction stage = 16 reduction elements, staged through LDS k-major ([k][m] and [k][n], rows padded to 144 floats:
// the 16 lanes of a k-row read 16 consecutive floats, the four k-rows of one MFMA land on four distinct 16-bank groups).
// Global -> registers for stage s + 1 is issued before the MFMAs of stage s.
//
// Reduction order (the contract of the forward / input-gradient GEMMs): stages walk the taps in the direct kernel's order (FORM_S1 /
// FORM_S1T: kh, then kw ascending, as direct_conv_s1_kernel) and, inside a tap, the channels in 16-channel chunks; an MFMA k-group is
// 4 consecutive channels of one tap with lane k-index 0 the lowest, and v_mfma_f32_16x16x4_f32 is exactly the k-ordered fmaf chain.
// An unsplit launch therefore computes every output as the same fmaf chain as direct_tapgemm_kernel / direct_conv_s1_kernel; taps
// outside the source grid and channels beyond K are staged as zeros and add exact zeros.
#include "gct2_common.h"
#include <algorithm>

namespace {

constexpr int FBM = 128, FBK = 16, FLD = 144;        // tile rows, reduction elements per stage, LDS row (floats)

__device__ __forceinline__ f32x4_t mfma_f32(float a, float b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// four consecutive floats from `src` (elements i with ok(i) only, zeros elsewhere); `vec`: all four are valid together and 16-byte aligned
__device__ __forceinline__ f32x4_t load4(const float* src, int valid, bool vec) {
  if (vec) return valid >= 4 ? *reinterpret_cast<const f32x4_t*>(src) : f32x4_t{0.f, 0.f, 0.f, 0.f};
  f32x4_t v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (j < valid) v[j] = src[j];
  return v;
}

// the MFMAs of one stage: nkg k-groups of 4 (wave-uniform) on the LDS tiles
template <int WN>
__device__ __forceinline__ void stage_mfma(const float* As, const float* Bs, int nkg, int wm, int wn, int lane, f32x4_t (&acc)[4][WN]) {
  for (int kk = 0; kk < nkg; kk++) {
    const int k = kk * 4 + (lane >> 4);
    float a[4], b[WN];
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = As[k * FLD + wm * 64 + i * 16 + (lane & 15)];
#pragma unroll
    for (int j = 0; j < WN; j++) b[j] = Bs[k * FLD + wn * (WN * 16) + j * 16 + (lane & 15)];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < WN; j++) acc[i][j] = mfma_f32(a[i], b[j], acc[i][j]);
  }
}

// the direct kernel's epilogue on one output element (opix: pixel of the output view)
template <int EPI>
__device__ __forceinline__ void epilogue(const TapGemmParams& p, float acc, size_t opix, int n) {
  float* y = reinterpret_cast<float*>(p.y) + opix * p.ldy + n;
  if (EPI == EPI_BIAS_ACT) {
    if (p.bias) acc += p.bias[n];
    if (p.relu) acc = fmaxf(acc, 0.f);
  } else {
    if (p.act && !(reinterpret_cast<const float*>(p.act)[opix * p.ldact + n] > 0.f)) acc = 0.f;
    if (p.accumulate) acc += *y;
  }
  *y = acc;
}

// flags of the launch: which operands take 16-byte loads
enum { F_AVEC = 1, F_BVEC = 2 };

// y = epilogue(sum over taps and channels); launch-z = output parity phase (FORM_CONVT), launch-y = K split (slabs in p.ws)
template <int FORM, int EPI, int BN>
__global__ __launch_bounds__(256) void f32_tapgemm_kernel(TapGemmParams p, int flags) {
  constexpr int WN = BN / 32;                        // MFMA tiles per wave along n
  constexpr bool FLIP = FORM == FORM_CONVT || FORM == FORM_S1T;   // the taps walk the source backwards, weights [tap][N][K]
  const int NT = FORM == FORM_CONV ? 4 : (FORM == FORM_CONVT ? 2 : p.ks);     // taps per direction
  const int pad = (p.ks - 1) / 2;                    // FORM_S1 / FORM_S1T
  constexpr int NBG = BN * FBK / 4 / 256;            // 4-float groups of the B stage per thread (2 or 1)
  __shared__ float As[FBK * FLD], Bs[FBK * FLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int Hs = p.Hs, Ws = p.Ws, K = p.K, N = p.N;
  const int M = p.B * Hs * Ws;
  const int mt = blockIdx.x % p.m_tiles, nt = blockIdx.x / p.m_tiles;
  const int m0 = mt * FBM, n0 = nt * BN;
  const int ph = FORM == FORM_CONVT ? (int)(blockIdx.z >> 1) : 0, pw = FORM == FORM_CONVT ? (int)(blockIdx.z & 1) : 0;
  const int Hsrc = FORM == FORM_CONV ? 2 * Hs : Hs, Wsrc = FORM == FORM_CONV ? 2 * Ws : Ws;
  const bool avec = flags & F_AVEC, bvec = flags & F_BVEC;
  const float* __restrict__ x = reinterpret_cast<const float*>(p.x);
  const float* __restrict__ w = reinterpret_cast<const float*>(p.w);
  // this thread's two A groups: pixel m0 + (e >> 2), channels 4 (e & 3) .. + 3 of the stage's chunk (e = tid + 256 g)
  int hb[2], wb[2], rowb[2];
#pragma unroll
  for (int g = 0; g < 2; g++) {
    const int m = m0 + ((tid + 256 * g) >> 2);
    int sw, sh, b;
    decode_pixel(m < M ? m : 0, Hs, Ws, -1, -1, sw, sh, b);
    if (FORM == FORM_CONV) { hb[g] = 2 * sh - 1; wb[g] = 2 * sw - 1; }
    else if (FORM == FORM_CONVT) { hb[g] = sh + ph; wb[g] = sw + pw; }
    else if (FORM == FORM_S1) { hb[g] = sh - pad; wb[g] = sw - pad; }
    else { hb[g] = sh + pad; wb[g] = sw + pad; }
    rowb[g] = b * Hsrc;
    if (m >= M) hb[g] = -4 * Hsrc - 8;               // never inside the source grid
  }
  const int nchunks = (K + FBK - 1) / FBK;
  const int niter = NT * NT * nchunks;
  const int per = (niter + p.ksplit - 1) / p.ksplit;
  const int s_lo = blockIdx.y * per, s_hi = min(niter, s_lo + per);
  f32x4_t ra[2], rb[NBG];
  auto load_stage = [&](int st) {
    const int t = st / nchunks, k0 = (st - t * nchunks) * FBK;
    const int ta = t / NT, tc = t - ta * NT;         // (kh, kw) of the stride-1 forms
    const int tap = FORM == FORM_CONV ? ta * 4 + tc : (FORM == FORM_CONVT ? (1 - ph + 2 * ta) * 4 + (1 - pw + 2 * tc) : t);
#pragma unroll
    for (int g = 0; g < 2; g++) {
      const int kq = (tid + 256 * g) & 3;
      const int h = FLIP ? hb[g] - ta : hb[g] + ta, ww = FLIP ? wb[g] - tc : wb[g] + tc;
      const int k = k0 + 4 * kq;
      const bool ok = (unsigned)h < (unsigned)Hsrc && (unsigned)ww < (unsigned)Wsrc;
      ra[g] = load4(ok ? x + ((size_t)(rowb[g] + h) * Wsrc + ww) * p.ldx + k : x, ok ? min(4, K - k) : 0, avec);
    }
#pragma unroll
    for (int g = 0; g < NBG; g++) {
      const int e = tid + 256 * g;
      if (!FLIP) {                    // [tap][K][N]: 4 consecutive n of row k
        const int k = k0 + e / (BN / 4), n = n0 + 4 * (e % (BN / 4));
        const bool ok = k < K;
        rb[g] = load4(w + ((size_t)tap * K + (ok ? k : 0)) * N + n, ok ? min(4, N - n) : 0, bvec);
      } else {                        // [tap][N][K]: 4 consecutive k of row n
        const int n = n0 + (e >> 2), k = k0 + 4 * (e & 3);
        const bool ok = n < N;
        rb[g] = load4(w + ((size_t)tap * N + (ok ? n : 0)) * K + k, ok ? min(4, K - k) : 0, bvec);
      }
    }
  };
  auto store_stage = [&]() {
#pragma unroll
    for (int g = 0; g < 2; g++) {
      const int e = tid + 256 * g, ml = e >> 2, kq = e & 3;
#pragma unroll
      for (int j = 0; j < 4; j++) As[(4 * kq + j) * FLD + ml] = ra[g][j];
    }
#pragma unroll
    for (int g = 0; g < NBG; g++) {
      const int e = tid + 256 * g;
      if (!FLIP) *reinterpret_cast<f32x4_t*>(&Bs[(e / (BN / 4)) * FLD + 4 * (e % (BN / 4))]) = rb[g];
      else {
#pragma unroll
        for (int j = 0; j < 4; j++) Bs[(4 * (e & 3) + j) * FLD + (e >> 2)] = rb[g][j];
      }
    }
  };
  f32x4_t acc[4][WN];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < WN; j++) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  if (s_lo < s_hi) load_stage(s_lo);
  for (int st = s_lo; st < s_hi; st++) {
    __syncthreads();
    store_stage();
    __syncthreads();
    const int k0 = (st % nchunks) * FBK;
    const int nkg = min(4, (K - k0 + 3) / 4);
    if (st + 1 < s_hi) load_stage(st + 1);
    stage_mfma<WN>(As, Bs, nkg, wm, wn, lane, acc);
  }
  // D layout: row 4 (lane >> 4) + r, column lane & 15 of each 16 x 16 tile
  const size_t npix = (size_t)M * (FORM == FORM_CONVT ? 4 : 1);
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = m0 + wm * 64 + i * 16 + 4 * (lane >> 4) + r;
      if (m >= M) continue;
      size_t opix = (size_t)m;
      if (FORM == FORM_CONVT) {
        int sw, sh, b;
        decode_pixel(m, Hs, Ws, -1, -1, sw, sh, b);
        opix = ((size_t)b * (2 * Hs) + 2 * sh + ph) * (2 * Ws) + 2 * sw + pw;
      }
#pragma unroll
      for (int j = 0; j < WN; j++) {
        const int n = n0 + wn * (WN * 16) + j * 16 + (lane & 15);
        if (n >= N) continue;
        if (p.ksplit > 1) p.ws[((size_t)blockIdx.y * npix + opix) * N + n] = acc[i][j][r];
        else epilogue<EPI>(p, acc[i][j][r], opix, n);
      }
    }
  }
}

// split-K: sums the ordered slabs [ksplit][npix][N] (slab order) and applies the epilogue; one thread per output element
template <int EPI>
__global__ __launch_bounds__(256) void f32_tapgemm_finalize_kernel(TapGemmParams p, size_t npix) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = npix * p.N;
  if (idx >= total) return;
  float v = 0.f;
  for (int s = 0; s < p.ksplit; s++) v += p.ws[(size_t)s * total + idx];
  epilogue<EPI>(p, v, idx / p.N, (int)(idx % p.N));
}

// dw[tap][cb][cs] (+)= sum_r big[pix_big(r, tap)][cb] * small[r][cs]: a GEMM with rows m = tap * Cb + cb, columns cs, reduction over the
// pixels r of the SMALL grid in stages of 16; launch-y = pixel split.  4x4 / stride-2 (p.ks = 0): 16 taps, tap = 4 kh + kw reads the
// big pixel (2 sh + kh - 1, 2 sw + kw - 1); stride-1 (p.ks odd): both tensors on one grid, ks * ks taps, tap = ks kh + kw reads
// (sh + kh - pad, sw + kw - pad).  out: slab rsplit index (mode 0), owner (1), atomics (2)
enum { WG_SLABS = 0, WG_OWNER = 1, WG_ATOMICS = 2 };
template <int BN>
__global__ __launch_bounds__(256) void f32_wgrad_kernel(WgradParams p, int flags, int m_tiles, int per, int mode) {
  constexpr int WN = BN / 32, NBG = BN * FBK / 4 / 256;
  __shared__ float As[FBK * FLD], Bs[FBK * FLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int ks = p.ks ? p.ks : 4, pad = p.ks ? (p.ks - 1) / 2 : 1, str = p.ks ? 1 : 2;    // taps per direction, tap offset, stride
  const int Hs = p.Hs, Ws = p.Ws, Hb = str * Hs, Wb = str * Ws, Cb = p.Cb, Cs = p.Cs;
  const int R = p.B * Hs * Ws, M = ks * ks * Cb;
  const int mt = blockIdx.x % m_tiles, nt = blockIdx.x / m_tiles;
  const int m0 = mt * FBM, n0 = nt * BN;
  const bool avec = flags & F_AVEC, bvec = flags & F_BVEC;
  const float* __restrict__ big = reinterpret_cast<const float*>(p.big);
  const float* __restrict__ small = reinterpret_cast<const float*>(p.small);
  // this thread's A rows: m0 + 4 (tid & 31) + j, j < 4 (the same for both of its groups; the groups differ in the pixel: tid >> 5, + 8)
  int dh[4], dw[4], cbj[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int m = m0 + 4 * (tid & 31) + j;
    const int tap = m / Cb, kh = tap / ks;
    cbj[j] = m - tap * Cb;
    dh[j] = m < M ? kh - pad : -4 * Hb - 8;          // an invalid row never lands inside the big grid
    dw[j] = tap - kh * ks - pad;
  }
  const int stages = (R + FBK - 1) / FBK;
  const int s_lo = blockIdx.y * per, s_hi = min(stages, s_lo + per);
  const int r_end = min(R, s_hi * FBK);
  f32x4_t ra[2], rb[NBG];
  auto load_stage = [&](int st) {
#pragma unroll
    for (int g = 0; g < 2; g++) {
      const int r = st * FBK + (tid >> 5) + 8 * g;
      int sw = 0, sh = 0, b = 0;
      if (r < r_end) decode_pixel(r, Hs, Ws, -1, -1, sw, sh, b);
      const bool rok = r < r_end;
      if (avec) {                     // Cb % 4 == 0: the four rows share one tap, 16-byte aligned
        const int h = str * sh + dh[0], ww = str * sw + dw[0];
        const bool ok = rok && (unsigned)h < (unsigned)Hb && (unsigned)ww < (unsigned)Wb;
        ra[g] = load4(ok ? big + ((size_t)(b * Hb + h) * Wb + ww) * p.ldbig + cbj[0] : big, ok ? 4 : 0, true);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int h = str * sh + dh[j], ww = str * sw + dw[j];
          const bool ok = rok && (unsigned)h < (unsigned)Hb && (unsigned)ww < (unsigned)Wb;
          ra[g][j] = ok ? big[((size_t)(b * Hb + h) * Wb + ww) * p.ldbig + cbj[j]] : 0.f;
        }
      }
    }
#pragma unroll
    for (int g = 0; g < NBG; g++) {
      const int e = tid + 256 * g;
      const int r = st * FBK + e / (BN / 4), n = n0 + 4 * (e % (BN / 4));
      const bool ok = r < r_end;
      rb[g] = load4(small + (size_t)(ok ? r : 0) * p.ldsmall + n, ok ? min(4, Cs - n) : 0, bvec);
    }
  };
  auto store_stage = [&]() {
#pragma unroll
    for (int g = 0; g < 2; g++) *reinterpret_cast<f32x4_t*>(&As[((tid >> 5) + 8 * g) * FLD + 4 * (tid & 31)]) = ra[g];
#pragma unroll
    for (int g = 0; g < NBG; g++) {
      const int e = tid + 256 * g;
      *reinterpret_cast<f32x4_t*>(&Bs[(e / (BN / 4)) * FLD + 4 * (e % (BN / 4))]) = rb[g];
    }
  };
  f32x4_t acc[4][WN];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < WN; j++) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  if (s_lo < s_hi) load_stage(s_lo);
  for (int st = s_lo; st < s_hi; st++) {
    __syncthreads();
    store_stage();
    __syncthreads();
    const int nkg = min(4, (r_end - st * FBK + 3) / 4);
    if (st + 1 < s_hi) load_stage(st + 1);
    stage_mfma<WN>(As, Bs, nkg, wm, wn, lane, acc);
  }
  const size_t n_out = (size_t)M * Cs;
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = m0 + wm * 64 + i * 16 + 4 * (lane >> 4) + r;
      if (m >= M) continue;
#pragma unroll
      for (int j = 0; j < WN; j++) {
        const int n = n0 + wn * (WN * 16) + j * 16 + (lane & 15);
        if (n >= Cs) continue;
        const size_t o = (size_t)m * Cs + n;
        if (mode == WG_SLABS) p.ws[(size_t)blockIdx.y * n_out + o] = acc[i][j][r];
        else if (mode == WG_ATOMICS) atomicAdd(p.dw + o, acc[i][j][r]);
        else p.dw[o] = p.accumulate ? p.dw[o] + acc[i][j][r] : acc[i][j][r];
      }
    }
  }
}

template <int FORM, int EPI>
void launch_tap(int bn, dim3 grid, hipStream_t s, const TapGemmParams& p, int flags) {
  if (bn == 64) hipLaunchKernelGGL((f32_tapgemm_kernel<FORM, EPI, 64>), grid, dim3(256), 0, s, p, flags);
  else hipLaunchKernelGGL((f32_tapgemm_kernel<FORM, EPI, 128>), grid, dim3(256), 0, s, p, flags);
}

}  // namespace

// fp32 forward / input-gradient tap GEMM (all four forms, both epilogues) on the matrix cores.  The fused bias gradient of the
// input-gradient calls is not this function's: run_dgrad (capi.hip) takes the column sums of the output view around it.
int f32_tapgemm(gct2_ctx& c, int form, int epi, TapGemmParams p, hipStream_t s) {
  if (form < FORM_CONV || form > FORM_S1T) return gct2_fail(GCT2_EINVAL, "f32_tapgemm: form %d", form);
  const int M = p.B * p.Hs * p.Ws;
  const int PH = form == FORM_CONVT ? 4 : 1;
  const int bn = p.N <= 64 ? 64 : 128;
  p.m_tiles = (M + FBM - 1) / FBM;
  p.n_tiles = (p.N + bn - 1) / bn;
  const int tiles = p.m_tiles * p.n_tiles * PH;
  const int taps = form == FORM_CONV ? 16 : (form == FORM_CONVT ? 4 : p.ks * p.ks);      // per launch phase
  const int niter = taps * ((p.K + FBK - 1) / FBK);
  const size_t npix = (size_t)M * PH;
  // the small-M deep levels cannot fill 256 CUs with output tiles: split the reduction into ordered slabs, >= 8 stages each
  p.ksplit = 1;
  p.ws = nullptr;
  if (c.ws && !c.no_splitk && tiles < 256) {
    int want = (512 + tiles - 1) / tiles;
    want = (int)std::min<size_t>((size_t)want, c.ws_bytes / (npix * p.N * sizeof(float)));
    want = std::min(want, niter / 8);
    if (want >= 2) {
      const int per = (niter + want - 1) / want;
      p.ksplit = (niter + per - 1) / per;
      p.ws = c.ws;
    }
  }
  const bool flip = form == FORM_CONVT || form == FORM_S1T;     // weights [tap][N][K], else [tap][K][N]
  int flags = 0;
  if (p.K % 4 == 0 && p.ldx % 4 == 0 && (uintptr_t)p.x % 16 == 0) flags |= F_AVEC;
  if ((uintptr_t)p.w % 16 == 0 && (flip ? p.K % 4 == 0 : p.N % 4 == 0)) flags |= F_BVEC;
  static const char* const names[] = {"conv", "convT", "s1", "s1t"};
  gct2_log(c, "f32mfma:%s:ksplit=%d", names[form], p.ksplit);
  const dim3 grid((unsigned)(p.m_tiles * p.n_tiles), (unsigned)p.ksplit, (unsigned)PH);
  const bool bias_act = epi == EPI_BIAS_ACT;
  switch (form) {
    case FORM_CONV:
      if (bias_act) launch_tap<FORM_CONV, EPI_BIAS_ACT>(bn, grid, s, p, flags);
      else launch_tap<FORM_CONV, EPI_MASK>(bn, grid, s, p, flags);
      break;
    case FORM_CONVT:
      if (bias_act) launch_tap<FORM_CONVT, EPI_BIAS_ACT>(bn, grid, s, p, flags);
      else launch_tap<FORM_CONVT, EPI_MASK>(bn, grid, s, p, flags);
      break;
    case FORM_S1:
      if (bias_act) launch_tap<FORM_S1, EPI_BIAS_ACT>(bn, grid, s, p, flags);
      else launch_tap<FORM_S1, EPI_MASK>(bn, grid, s, p, flags);
      break;
    default:
      if (bias_act) launch_tap<FORM_S1T, EPI_BIAS_ACT>(bn, grid, s, p, flags);
      else launch_tap<FORM_S1T, EPI_MASK>(bn, grid, s, p, flags);
  }
  if (p.ksplit > 1) {
    const dim3 fgrid((unsigned)((npix * p.N + 255) / 256));
    if (epi == EPI_BIAS_ACT) hipLaunchKernelGGL((f32_tapgemm_finalize_kernel<EPI_BIAS_ACT>), fgrid, dim3(256), 0, s, p, npix);
    else hipLaunchKernelGGL((f32_tapgemm_finalize_kernel<EPI_MASK>), fgrid, dim3(256), 0, s, p, npix);
  }
  return gct2_check_launch("f32_tapgemm");
}

// fp32 weight gradient of the 4x4 / stride-2 layers (p.ks = 0) and of the stride-1 convolutions (p.ks odd) on the matrix cores.  Pixel
// splits leave ordered slabs in the weight-gradient scratch (reduced by wgrad_reduce in slab order, or handed to the caller's optimizer
// through `defer` - the wgrad_mfma contract); without scratch: one owner per tile, or fp32 atomics when the tiles need a split to fill
// the chip.
int f32_wgrad(gct2_ctx& c, WgradParams p, hipStream_t s, WgradSlabs* defer) {
  if (defer) *defer = WgradSlabs{nullptr, 0, 0};
  const int R = p.B * p.Hs * p.Ws, M = (p.ks ? p.ks * p.ks : 16) * p.Cb;
  const int bn = p.Cs <= 64 ? 64 : 128;
  const int m_tiles = (M + FBM - 1) / FBM, tiles = m_tiles * ((p.Cs + bn - 1) / bn);
  const int stages = (R + FBK - 1) / FBK;
  // ~1024 work-groups (4 per CU), >= 16 stages (256 pixels) per split
  int rsplit = std::max(1, std::min((1024 + tiles - 1) / tiles, stages / 16));
  if (c.wgrad_split) rsplit = std::min(1 << (c.wgrad_split - 1), stages);     // forced pixel split (tuning bits 28-30)
  const size_t n = (size_t)M * p.Cs;
  size_t ws_bytes = 0;
  float* ws = c.wgrad_scratch(&ws_bytes);
  int mode = rsplit > 1 ? WG_ATOMICS : WG_OWNER;
  if (rsplit > 1 && ws && (uintptr_t)p.dw % 16 == 0) {
    const int fit = (int)std::min<size_t>((size_t)rsplit, ws_bytes / (n * sizeof(float)));
    if (fit >= 2) { rsplit = fit; mode = WG_SLABS; }
  }
  const int per = (stages + rsplit - 1) / rsplit;
  rsplit = (stages + per - 1) / per;                 // every split non-empty (each one owns a slab)
  if (rsplit == 1) mode = WG_OWNER;
  p.rsplit = rsplit;
  p.ws = mode == WG_SLABS ? ws : nullptr;
  int flags = 0;
  if (p.Cb % 4 == 0 && p.ldbig % 4 == 0 && (uintptr_t)p.big % 16 == 0) flags |= F_AVEC;
  if (p.Cs % 4 == 0 && p.ldsmall % 4 == 0 && (uintptr_t)p.small % 16 == 0) flags |= F_BVEC;
  if (mode == WG_ATOMICS && !p.accumulate) (void)hipMemsetAsync(p.dw, 0, n * sizeof(float), s);     // atomics add into the target
  gct2_log(c, "f32mfma:%s:rsplit=%d:%s", p.ks ? "wgrad_s1" : "wgrad", rsplit,
           mode == WG_SLABS ? "slabs" : (mode == WG_OWNER ? "owner" : "atomics"));
  const dim3 grid((unsigned)tiles, (unsigned)rsplit);
  if (bn == 64) hipLaunchKernelGGL((f32_wgrad_kernel<64>), grid, dim3(256), 0, s, p, flags, m_tiles, per, mode);
  else hipLaunchKernelGGL((f32_wgrad_kernel<128>), grid, dim3(256), 0, s, p, flags, m_tiles, per, mode);
  if (int e = gct2_check_launch("f32_wgrad")) return e;
  if (mode != WG_SLABS) return GCT2_OK;
  if (defer && !p.accumulate) { *defer = WgradSlabs{p.ws, rsplit, n}; return GCT2_OK; }     // the caller's optimizer kernel sums them
  return wgrad_reduce(p.ws, p.dw, n, rsplit, p.accumulate, s);
}
