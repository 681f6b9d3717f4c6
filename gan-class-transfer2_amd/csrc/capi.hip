// extern "C" boundary (include/gct2.h): argument validation, path selection (MFMA vs direct), launches.
#include "gct2_common.h"
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

// the only static storage of the library, all of it per host thread: the text of the last error, and the context that stands in
// for ctx = NULL (no scratch, automatic tiles; reset at every use)
static thread_local char g_err[512] = "";
static thread_local gct2_ctx g_null_ctx{};

int gct2_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
void gct2_log(gct2_ctx& c, const char* fmt, ...) {
  if (!c.log_on) return;
  char buf[160];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  // bounded: a log left switched on for a whole run stops growing at 1 MiB and says so once
  constexpr size_t LOG_CAP = (size_t)1 << 20;
  if (c.log.size() + sizeof(buf) + 16 > LOG_CAP) {
    if (!c.log_full) { c.log += "log:truncated;"; c.log_full = true; }
    return;
  }
  c.log += buf;
  c.log += ';';
}
int gct2_check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return gct2_fail(GCT2_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return GCT2_OK;
}

namespace {
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline bool dtype_ok(int d) { return d == GCT2_F32 || d == GCT2_BF16 || d == GCT2_F16; }
inline size_t esize(int d) { return d == GCT2_F32 ? 4 : 2; }

int check_conv_args(const char* fn, int dtype, const void* a, const void* b, const void* c, int B, int H, int W, int Cin, int Cout) {
  if (!dtype_ok(dtype)) return gct2_fail(GCT2_EINVAL, "%s: unknown dtype %d", fn, dtype);
  if (!a || !b || !c) return gct2_fail(GCT2_EINVAL, "%s: null pointer", fn);
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return gct2_fail(GCT2_EINVAL, "%s: non-positive dimension", fn);
  if ((size_t)B * H * W * 4 >= ((size_t)1 << 31)) return gct2_fail(GCT2_EINVAL, "%s: B*H*W too large for 32-bit pixel indices", fn);
  return GCT2_OK;
}
inline gct2_ctx& C(gct2_ctx* c) {
  if (c) return *c;
  g_null_ctx = gct2_ctx{};
  return g_null_ctx;
}
// The ReLU bit plane registered for THIS call (gct2_ctx_set_relu_bits is one-shot).  Every layer entry point constructs one of these
// FIRST THING - before any argument check - so that a plane never outlives the call it was registered for, whatever that call
// returns (r03 consumed it behind the checks: a rejected call leaked its plane to the next layer call).
struct PlaneTaken {
  unsigned char* bits; int ld;
  explicit PlaneTaken(gct2_ctx& c) : bits(c.relu_bits), ld(c.relu_ldbits) { c.relu_bits = nullptr; c.relu_ldbits = 0; c.relu_bits_done = 0; }
  // entry points that cannot use a plane: a pending one is a caller error
  int none(const char* fn) const {
    return bits ? gct2_fail(GCT2_EINVAL, "%s: a ReLU bit plane was registered (gct2_ctx_set_relu_bits), but this call neither writes nor reads one", fn) : GCT2_OK;
  }
  int into(const char* fn, int channels, TapGemmParams& p) const {
    if (!bits) return GCT2_OK;
    if (channels % 8 || ld < channels / 8) return gct2_fail(GCT2_EINVAL, "%s: ReLU bit plane needs channels %% 8 == 0 and ld_bytes >= channels / 8 (got %d, %d)", fn, channels, ld);
    p.bits = bits; p.ldbits = ld;
    return GCT2_OK;
  }
};
// forward calls: if the launch did not write the plane in its epilogue, derive it from the activation it stored
int finish_relu_bits(gct2_ctx& c, int dtype, const TapGemmParams& p, size_t pixels, void* stream) {
  if (!p.bits || c.relu_bits_done) return GCT2_OK;
  gct2_log(c, "relu_bits:derived");
  return pw_relu_bits(dtype, p.y, p.ldy, pixels, p.N, p.bits, p.ldbits, S(stream));
}
// fp32 on the matrix cores (gct2_ctx_set_f32_math); force_direct wins, so the direct kernels stay the independent reference
inline bool f32_on_mfma(const gct2_ctx& c, int dtype) { return dtype == GCT2_F32 && c.f32_math == GCT2_F32_MATH_MFMA && !c.force_direct; }
// forward / input-gradient launch of every form: fp32 on the fp32 matrix cores when the ctx asks for them, 16-bit on the matrix cores
// where their layouts allow it (stride-1 forms: kernel sizes <= 5), else one thread per output (the stride-1 fall-back logs nothing)
int run_tapgemm(gct2_ctx& c, int dtype, int form, int epi, const TapGemmParams& p, void* stream) {
  const bool s1 = form == FORM_S1 || form == FORM_S1T;
  if (f32_on_mfma(c, dtype)) return f32_tapgemm(c, form, epi, p, S(stream));
  if (!c.force_direct && (!s1 || p.ks <= 5) && tapgemm_mfma_supported(dtype, p)) return tapgemm_mfma(c, dtype, form, epi, p, S(stream));
  if (s1)
    return conv_s1_direct(dtype, form == FORM_S1T, p.x, p.ldx, p.w, p.bias, p.act, p.ldact, p.y, p.ldy, p.B, p.Hs, p.Ws, p.K, p.N, p.ks, p.relu,
                          p.accumulate, S(stream));
  gct2_log(c, "direct:tap");
  return tapgemm_direct(dtype, form, epi, p, S(stream));
}
// input-gradient launch with optional fused bias gradient: db (+)= column sums of the masked gradient THIS call produces
// (channels [0, split) -> db, the rest -> db2).  MFMA path: fused into the epilogue / split-K finalize.  Direct path:
// column sums of the output view after the launch, minus those before it when the launch accumulates (the fp32 matrix-core path too).
int run_dgrad(gct2_ctx& c, int dtype, int form, TapGemmParams p, size_t out_pixels, float* db, int split, float* db2, int db_acc,
              void* stream) {
  if (split < 0 || split > p.N) return gct2_fail(GCT2_EINVAL, "dgrad: db_split out of range");
  p.db = db; p.db_split = split; p.db2 = db2; p.db_acc = db_acc;
  if (!c.force_direct && tapgemm_mfma_supported(dtype, p)) return tapgemm_mfma(c, dtype, form, EPI_MASK, p, S(stream));
  const bool f32m = f32_on_mfma(c, dtype);
  if (!f32m) gct2_log(c, "direct:tap");
  // the column-sum kernels below add with atomics, at once: row sets queued for the same targets are reduced first (a queued
  // overwrite would otherwise run behind this call's add and erase it)
  if (int e = tapgemm_dbq_flush_for(c, db, split, db2, p.N - split, S(stream))) return e;
  zero_overwritten_db(p, S(stream));
  const size_t es = esize(dtype);
  auto sums = [&](float sign) -> int {
    if (db && split > 0) if (int e = pw_colsum(dtype, p.y, p.ldy, db, out_pixels, split, sign, S(stream))) return e;
    if (db2 && split < p.N)
      if (int e = pw_colsum(dtype, (const char*)p.y + (size_t)split * es, p.ldy, db2, out_pixels, p.N - split, sign, S(stream))) return e;
    return GCT2_OK;
  };
  if ((db || db2) && p.accumulate) if (int e = sums(-1.f)) return e;
  if (int e = f32m ? f32_tapgemm(c, form, EPI_MASK, p, S(stream)) : tapgemm_direct(dtype, form, EPI_MASK, p, S(stream))) return e;
  return (db || db2) ? sums(1.f) : GCT2_OK;
}
// weight-gradient launch, 4x4 / stride-2 (p.ks == 0) or stride-1 (the stride-1 fall-back logs nothing)
int run_wgrad(gct2_ctx& c, int dtype, const WgradParams& p, void* stream, WgradSlabs* defer) {
  if (f32_on_mfma(c, dtype)) return f32_wgrad(c, p, S(stream), defer);
  if (!c.force_direct && wgrad_mfma_supported(dtype, p)) return wgrad_mfma(c, dtype, p, S(stream), defer);
  if (defer) *defer = WgradSlabs{nullptr, 0, 0};
  if (p.ks)
    return conv_s1_wgrad_direct(dtype, p.big, p.ldbig, p.small, p.ldsmall, p.dw, p.B, p.Hs, p.Ws, p.Cb, p.Cs, p.ks, p.accumulate, S(stream));
  gct2_log(c, "direct:wgrad");
  return wgrad_direct(dtype, p, S(stream));
}
// bias gradient of a weight-gradient call: db (+)= column sums of dz (atomics: an overwritten target starts from zero)
int wgrad_db(gct2_ctx& c, int dtype, const void* dz, int lddz, float* db, size_t pixels, int Cout, int accumulate, void* stream) {
  if (int e = tapgemm_dbq_flush_for(c, db, Cout, nullptr, 0, S(stream))) return e;      // (an immediate writer: queued row sets of db go first)
  if (!accumulate) (void)hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), S(stream));
  return pw_colsum(dtype, dz, lddz, db, pixels, Cout, 1.f, S(stream));
}
// Keras Adam right behind a weight-gradient launch, on the same stream (gct2_adam_args): the range [p, p + n) of the caller's arenas
// starts with the layer's kernel (the engine's ranges hold the kernel only since r04: biases and Dense(3) live in one fp32 zone with
// a launch of its own); the kernel gradient comes from the slabs the launch left (never materialised) or from dw (written, not
// accumulated: no zeroing), whatever lies behind the kernel in the range from the gradient arena; nothing is zeroed
int check_adam_args(const gct2_adam_args* a, const float* dw, size_t nw) {
  if (!a->p || !a->m || !a->v) return gct2_fail(GCT2_EINVAL, "wgrad + adam: null arena pointers");
  if (a->n < nw || ((uintptr_t)a->p | (uintptr_t)a->m | (uintptr_t)a->v | (uintptr_t)dw) % 16)
    return gct2_fail(GCT2_EINVAL, "wgrad + adam: range shorter than the weight tensor or misaligned");
  return GCT2_OK;
}
// the optimizer launch of a gct2_adam_args: the kernel gradient (nw elements) is in dw or in the slabs `sl`
int run_adam(const gct2_adam_args* a, float* dw, size_t nw, const WgradSlabs& sl, void* stream) {
  return pw_adam(a->p, a->m, a->v, dw, a->shadow, a->shadow_dtype, a->n, a->alpha, a->beta1, a->beta2, a->eps, a->grad_mul, nullptr, 0,
                 S(stream), sl.base, sl.nslab, sl.stride, sl.nslab ? nw : 0);
}
int adam_after_wgrad(gct2_adam_args* a, float* dw, size_t nw, const WgradSlabs& sl, void* stream) {
  if (a->defer) {      // the caller runs the step later (gct2_adam_apply): tell it where the kernel gradient is
    a->slab_base = sl.base; a->nslab = sl.nslab; a->slab_stride = sl.stride;
    return GCT2_OK;
  }
  return run_adam(a, dw, nw, sl, stream);
}
int check_s1(const char* fn, int KS) {
  if (KS < 1 || KS > 7 || !(KS & 1)) return gct2_fail(GCT2_EINVAL, "%s: kernel size %d (odd, 1..7: 'same' padding is symmetric then)", fn, KS);
  return GCT2_OK;
}
// The three weight-gradient entry points.  x: [B, H, W, Cin]; dz: [B, H/2, W/2, Cout] (WG_CONV), [B, 2H, 2W, Cout] (WG_CONVT) or
// [B, H, W, Cout] (WG_S1, KS x KS taps); dw fp32 in the Keras layout of the layer, db fp32[Cout] or null.  The order of the checks
// is part of the interface: it decides the message of a call with more than one mistake.
enum WgradKind { WG_CONV, WG_CONVT, WG_S1 };
int wgrad_entry(gct2_ctx* ctx, const char* fn, WgradKind kind, int dtype, const void* x, int ldx, const void* dz, int lddz, float* dw, float* db,
                int B, int H, int W, int Cin, int Cout, int KS, int accumulate, gct2_adam_args* adam, void* stream) {
  gct2_ctx& c = C(ctx);
  if (int e = PlaneTaken(c).none(fn)) return e;
  const int up = kind == WG_CONVT ? 2 : 1;           // (the argument checks see the larger of the two grids)
  if (int e = check_conv_args(fn, dtype, x, dz, dw, B, up * H, up * W, Cin, Cout)) return e;
  if (kind == WG_S1) if (int e = check_s1(fn, KS)) return e;
  if (kind == WG_CONV && ((H & 1) || (W & 1))) return gct2_fail(GCT2_EINVAL, "%s: H=%d W=%d must be even", fn, H, W);
  if (ldx < Cin || lddz < Cout) return gct2_fail(GCT2_EINVAL, "%s: ld smaller than channel count", fn);
  if (adam && accumulate) return gct2_fail(GCT2_EINVAL, "%s: the fused optimizer step needs accumulate = 0", fn);
  // WgradParams: the tensor on the BIG grid first (the transposed layer's is dz)
  WgradParams p = kind == WG_CONV    ? WgradParams{x, ldx, dz, lddz, dw, B, H / 2, W / 2, Cin, Cout, 1}
                  : kind == WG_CONVT ? WgradParams{dz, lddz, x, ldx, dw, B, H, W, Cout, Cin, 1}
                                     : WgradParams{x, ldx, dz, lddz, dw, B, H, W, Cin, Cout, 1};
  p.accumulate = accumulate ? 1 : 0;
  p.ks = kind == WG_S1 ? KS : 0;
  const size_t nw = (size_t)16 * Cin * Cout, dz_pixels = (size_t)B * p.Hs * p.Ws * (kind == WG_CONVT ? 4 : 1);
  WgradSlabs sl{nullptr, 0, 0};
  WgradSlabs* defer = adam ? &sl : nullptr;
  if (adam) if (int e = check_adam_args(adam, dw, nw)) return e;
  if (kind == WG_CONV && !c.force_direct && rgb_wgrad_supported(dtype, p)) {                  // image layer (Cin <= 4)
    gct2_log(c, "rgb:wgrad");
    if (int e = rgb_wgrad(c, dtype, p, S(stream), defer)) return e;
  } else if (int e = run_wgrad(c, dtype, p, stream, defer)) return e;
  if (db) if (int e = wgrad_db(c, dtype, dz, lddz, db, dz_pixels, Cout, accumulate, stream)) return e;
  return adam ? adam_after_wgrad(adam, dw, nw, sl, stream) : GCT2_OK;
}
// the scratch setters: a ctx, and a null or 16-byte aligned buffer
int check_scratch(const char* fn, const gct2_ctx* ctx, const void* buf) {
  if (!ctx) return gct2_fail(GCT2_EINVAL, "%s: null ctx", fn);
  if (buf && ((uintptr_t)buf % 16)) return gct2_fail(GCT2_EINVAL, "%s: pointer must be 16-byte aligned", fn);
  return GCT2_OK;
}
}  // namespace

extern "C" {

int gct2_abi_version(void) { return 17; }
int gct2_build_flags(void) {
#ifdef GCT2_STAMP
  return GCT2_BUILD_STAMP;
#else
  return 0;
#endif
}
const char* gct2_last_error(void) { return g_err; }

int gct2_ctx_create(gct2_ctx** ctx) {
  if (!ctx) return gct2_fail(GCT2_EINVAL, "ctx_create: null output pointer");
  *ctx = new (std::nothrow) gct2_ctx();
  return *ctx ? GCT2_OK : gct2_fail(GCT2_EINVAL, "ctx_create: out of host memory");
}
int gct2_ctx_destroy(gct2_ctx* ctx) {
  delete ctx;
  return GCT2_OK;
}
int gct2_ctx_set_workspace(gct2_ctx* ctx, void* ws, size_t bytes) {
  if (int e = check_scratch("ctx_set_workspace", ctx, ws)) return e;
  ctx->ws = ws ? reinterpret_cast<float*>(ws) : nullptr;
  ctx->ws_bytes = ws ? bytes : 0;
  return GCT2_OK;
}
int gct2_ctx_set_wgrad_workspace(gct2_ctx* ctx, void* ws, size_t bytes) {
  if (int e = check_scratch("ctx_set_wgrad_workspace", ctx, ws)) return e;
  ctx->wws = ws ? reinterpret_cast<float*>(ws) : nullptr;
  ctx->wws_bytes = ws ? bytes : 0;
  return GCT2_OK;
}
int gct2_ctx_set_bias_queue(gct2_ctx* ctx, void* buf, size_t bytes) {
  if (int e = check_scratch("ctx_set_bias_queue", ctx, buf)) return e;
  ctx->dbq_jobs.clear();                     // (row sets recorded and not flushed are dropped: flush before changing the buffer)
  ctx->dbq_used = 0;
  ctx->dbq = buf ? reinterpret_cast<float*>(buf) : nullptr;
  ctx->dbq_floats = buf ? bytes / sizeof(float) : 0;
  return GCT2_OK;
}
int gct2_bias_queue_flush(gct2_ctx* ctx, void* stream) {
  if (!ctx) return gct2_fail(GCT2_EINVAL, "bias_queue_flush: null ctx");
  return tapgemm_dbq_flush(*ctx, S(stream));
}
int gct2_ctx_set_tuning(gct2_ctx* ctx, int v) {
  if (!ctx) return gct2_fail(GCT2_EINVAL, "ctx_set_tuning: null ctx");
  const int tap = v & 0xff, wg = (v >> 16) & 0xff, known = 0x1ff | (0xff << 16) | (0x7f << 24);
  if ((v & ~known) || (tap != 0 && tap != 2 && tap != 5) || (wg != 0 && wg != 2 && wg != 3 && wg != 4 && wg != 5 && wg != 6 && wg != 7) || ((v >> 24) & 3) == 3 || ((v >> 26) & 3) == 3)
    return gct2_fail(GCT2_EINVAL, "ctx_set_tuning: unknown tuning word 0x%x (include/gct2.h)", v);
  ctx->tap_variant = tap;
  ctx->wgrad_variant = wg;
  ctx->no_splitk = (v >> 8) & 1;
  ctx->halo_mode = (v >> 24) & 3;
  ctx->xcd_order = (v >> 26) & 3;
  ctx->wgrad_split = (v >> 28) & 7;
  return GCT2_OK;
}
int gct2_ctx_set_relu_bits(gct2_ctx* ctx, void* bits, int ld_bytes) {
  if (!ctx) return gct2_fail(GCT2_EINVAL, "ctx_set_relu_bits: null ctx");
  if (bits && ld_bytes <= 0) return gct2_fail(GCT2_EINVAL, "ctx_set_relu_bits: ld_bytes must be positive");
  ctx->relu_bits = reinterpret_cast<unsigned char*>(bits);
  ctx->relu_ldbits = bits ? ld_bytes : 0;
  return GCT2_OK;
}
int gct2_ctx_set_stamp_buffer(gct2_ctx* ctx, void* stamps, size_t bytes) {
  if (!ctx) return gct2_fail(GCT2_EINVAL, "ctx_set_stamp_buffer: null ctx");
#ifdef GCT2_STAMP
  if (stamps && ((uintptr_t)stamps % 8)) return gct2_fail(GCT2_EINVAL, "ctx_set_stamp_buffer: pointer must be 8-byte aligned");
  ctx->stamps = reinterpret_cast<unsigned long long*>(stamps);
  ctx->stamps_bytes = stamps ? bytes : 0;
  return GCT2_OK;
#else
  (void)stamps; (void)bytes;
  return gct2_fail(GCT2_EINVAL, "ctx_set_stamp_buffer: this is the product build (rebuild with make EXTRA=-DGCT2_STAMP for in-kernel stamps)");
#endif
}
int gct2_ctx_log_launches(gct2_ctx* ctx, int on) {
  if (!ctx) return gct2_fail(GCT2_EINVAL, "ctx_log_launches: null ctx");
  ctx->log_on = on != 0;
  ctx->log.clear();
  ctx->log_full = false;
  return GCT2_OK;
}
int gct2_ctx_read_launch_log(gct2_ctx* ctx, char* buf, size_t bytes, size_t* needed) {
  if (!ctx) return gct2_fail(GCT2_EINVAL, "ctx_read_launch_log: null ctx");
  const size_t need = ctx->log.size() + 1;
  if (needed) *needed = need;
  if (!buf || bytes < need)       // nothing is copied and nothing is cleared: call again with `needed` bytes
    return gct2_fail(GCT2_EINVAL, "ctx_read_launch_log: the log holds %zu bytes, the buffer %zu", need, buf ? bytes : (size_t)0);
  memcpy(buf, ctx->log.data(), need - 1);
  buf[need - 1] = 0;
  ctx->log.clear();
  ctx->log_full = false;
  return GCT2_OK;
}
int gct2_ctx_force_direct(gct2_ctx* ctx, int on) {
  if (!ctx) return gct2_fail(GCT2_EINVAL, "ctx_force_direct: null ctx");
  ctx->force_direct = on ? 1 : 0;
  return GCT2_OK;
}
int gct2_ctx_set_f32_math(gct2_ctx* ctx, int mode) {
  if (!ctx) return gct2_fail(GCT2_EINVAL, "ctx_set_f32_math: null ctx");
  if (mode != GCT2_F32_MATH_DIRECT && mode != GCT2_F32_MATH_MFMA) return gct2_fail(GCT2_EINVAL, "ctx_set_f32_math: unknown mode %d", mode);
  ctx->f32_math = mode;
  return GCT2_OK;
}

int gct2_device_check(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return gct2_fail(GCT2_ENODEV, "no HIP device");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return gct2_fail(GCT2_ENODEV, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return gct2_fail(GCT2_ENODEV, "device is %s, this library is built for gfx950", prop.gcnArchName);
  return GCT2_OK;
}

int gct2_stream_occupy(void* stream, int workgroups, double microseconds) {
  if (workgroups < 1 || workgroups > 1024 || !(microseconds >= 0.0) || microseconds > 20000.0)
    return gct2_fail(GCT2_EINVAL, "stream_occupy: 1..1024 work-groups for 0..20000 us (got %d, %g)", workgroups, microseconds);
  return pw_occupy(workgroups, (unsigned long long)(microseconds * 100.0), S(stream));
}

int gct2_conv4s2_fwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w, const float* bias, void* y, int ldy, int B, int H, int W,
                     int Cin, int Cout, int relu, void* stream) {
  gct2_ctx& c = C(ctx);
  const PlaneTaken plane(c);
  if (int e = check_conv_args("conv4s2_fwd", dtype, x, w, y, B, H, W, Cin, Cout)) return e;
  if ((H & 1) || (W & 1)) return gct2_fail(GCT2_EINVAL, "conv4s2_fwd: H=%d W=%d must be even (skip concat, train.py:114-119)", H, W);
  if (ldx < Cin || ldy < Cout) return gct2_fail(GCT2_EINVAL, "conv4s2_fwd: ld smaller than channel count");
  TapGemmParams p{x, ldx, w, bias, nullptr, 0, y, ldy, B, H / 2, W / 2, Cin, Cout, relu, 0};
  if (int e = plane.into("conv4s2_fwd", Cout, p)) return e;
  const size_t out_pixels = (size_t)B * (H / 2) * (W / 2);
  if (!c.force_direct && rgb_fwd_supported(dtype, p)) {                                       // image layer (Cin <= 4)
    gct2_log(c, "rgb:fwd");
    if (int e = rgb_fwd(dtype, p, S(stream))) return e;
    if (p.bits && rgb_fwd_writes_bits(p)) c.relu_bits_done = 1;
    return finish_relu_bits(c, dtype, p, out_pixels, stream);
  }
  if (int e = run_tapgemm(c, dtype, FORM_CONV, EPI_BIAS_ACT, p, stream)) return e;
  return finish_relu_bits(c, dtype, p, out_pixels, stream);
}

int gct2_conv4s2_dgrad(gct2_ctx* ctx, int dtype, const void* dz, int lddz, const void* w, const void* act, int ldact, void* dx, int lddx, int B,
                       int H, int W, int Cin, int Cout, int accumulate, float* db, int db_split, float* db2, int db_accumulate, void* stream) {
  gct2_ctx& c = C(ctx);
  const PlaneTaken plane(c);
  if (int e = check_conv_args("conv4s2_dgrad", dtype, dz, w, dx, B, H, W, Cin, Cout)) return e;
  if ((H & 1) || (W & 1)) return gct2_fail(GCT2_EINVAL, "conv4s2_dgrad: H=%d W=%d must be even", H, W);
  if (lddz < Cout || lddx < Cin || (act && ldact < Cin)) return gct2_fail(GCT2_EINVAL, "conv4s2_dgrad: ld smaller than channel count");
  TapGemmParams p{dz, lddz, w, nullptr, act, ldact, dx, lddx, B, H / 2, W / 2, Cout, Cin, 0, accumulate};
  if (int e = plane.into("conv4s2_dgrad", Cin, p)) return e;
  if (!act) p.bits = nullptr;                                   // the plane stands in for act: no mask asked for, none applied
  return run_dgrad(c, dtype, FORM_CONVT, p, (size_t)B * H * W, db, db_split, db2, db_accumulate, stream);
}

int gct2_conv4s2_wgrad(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* dz, int lddz, float* dw, float* db, int B, int H, int W,
                       int Cin, int Cout, int accumulate, gct2_adam_args* adam, void* stream) {
  return wgrad_entry(ctx, "conv4s2_wgrad", WG_CONV, dtype, x, ldx, dz, lddz, dw, db, B, H, W, Cin, Cout, 0, accumulate, adam, stream);
}

int gct2_convT4s2_fwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w, const float* bias, void* y, int ldy, int B, int H, int W,
                      int Cin, int Cout, int relu, void* stream) {
  gct2_ctx& c = C(ctx);
  const PlaneTaken plane(c);
  if (int e = check_conv_args("convT4s2_fwd", dtype, x, w, y, B, 2 * H, 2 * W, Cin, Cout)) return e;
  if (ldx < Cin || ldy < Cout) return gct2_fail(GCT2_EINVAL, "convT4s2_fwd: ld smaller than channel count");
  TapGemmParams p{x, ldx, w, bias, nullptr, 0, y, ldy, B, H, W, Cin, Cout, relu, 0};
  if (int e = plane.into("convT4s2_fwd", Cout, p)) return e;
  if (int e = run_tapgemm(c, dtype, FORM_CONVT, EPI_BIAS_ACT, p, stream)) return e;
  return finish_relu_bits(c, dtype, p, (size_t)B * 4 * H * W, stream);
}

int gct2_convT4s2_fwd_head_train(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w, const float* bias, const float* head_w,
                                 const float* head_b, const float* target, float* pred, void* dy, int lddy, float* head_dw, float* head_db,
                                 float* loss, int B, int H, int W, int Cin, int Cout, int head_Cin, int head_Cout,
                                 const float* loss_scale_ptr, float* db, const void* x2, int ldx2, int accumulate, void* stream) {
  gct2_ctx& c = C(ctx);
  if (int e = PlaneTaken(c).none("convT4s2_fwd_head_train")) return e;
  if (int e = check_conv_args("convT4s2_fwd_head_train", dtype, x, w, dy, B, 2 * H, 2 * W, Cin, Cout)) return e;
  if (!head_w || !target || !head_dw || !loss) return gct2_fail(GCT2_EINVAL, "convT4s2_fwd_head_train: null pointer");
  if (ldx < Cin || lddy < Cout) return gct2_fail(GCT2_EINVAL, "convT4s2_fwd_head_train: ld smaller than channel count");
  const int nimg = head_Cin - Cout;
  if (head_Cout < 1 || head_Cout > 3 || nimg < 0 || nimg > 3 || (nimg > 0 && (!x2 || ldx2 < 4 || ldx2 % 4 || (uintptr_t)x2 % 8)))
    return gct2_fail(GCT2_EINVAL, "convT4s2_fwd_head_train: head needs <= 3 outputs and <= 3 image channels in a packed x2 (8-byte rows)");
  TapGemmParams p{x, ldx, w, bias, nullptr, 0, dy, lddy, B, H, W, Cin, Cout, 1, 0};
  p.head = HeadFuse{head_w, head_b, target, pred, x2, ldx2, nullptr, loss_scale_ptr, head_Cin, head_Cout,
                    (float)((double)B * 2 * H * 2 * W * head_Cout)};
  if (c.force_direct || !halo_head_supported(c, dtype, p))
    return gct2_fail(GCT2_EINVAL, "convT4s2_fwd_head_train: needs a 16-bit dtype, Cout = 64, H and W multiples of 16, 16-byte aligned views, "
                                  "a ctx workspace of B*(H/16)*(W/16)*288 floats, and 31-bit source offsets: B*H*W*ldx*2 + 2*Cin + 128 and "
                                  "the kernel's 16*Cin*Cout*2 bytes below 0x7ff00000");
  return halo_head(c, dtype, p, head_dw, head_db, loss, db, accumulate, S(stream));
}

int gct2_convT4s2_dgrad(gct2_ctx* ctx, int dtype, const void* dz, int lddz, const void* w, const void* act, int ldact, void* dx, int lddx, int B,
                        int H, int W, int Cin, int Cout, int accumulate, float* db, int db_split, float* db2, int db_accumulate, void* stream) {
  gct2_ctx& c = C(ctx);
  const PlaneTaken plane(c);
  if (int e = check_conv_args("convT4s2_dgrad", dtype, dz, w, dx, B, 2 * H, 2 * W, Cin, Cout)) return e;
  if (lddz < Cout || lddx < Cin || (act && ldact < Cin)) return gct2_fail(GCT2_EINVAL, "convT4s2_dgrad: ld smaller than channel count");
  TapGemmParams p{dz, lddz, w, nullptr, act, ldact, dx, lddx, B, H, W, Cout, Cin, 0, accumulate};
  if (int e = plane.into("convT4s2_dgrad", Cin, p)) return e;
  if (!act) p.bits = nullptr;
  return run_dgrad(c, dtype, FORM_CONV, p, (size_t)B * H * W, db, db_split, db2, db_accumulate, stream);
}

int gct2_convT4s2_wgrad(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* dz, int lddz, float* dw, float* db, int B, int H, int W,
                        int Cin, int Cout, int accumulate, gct2_adam_args* adam, void* stream) {
  return wgrad_entry(ctx, "convT4s2_wgrad", WG_CONVT, dtype, x, ldx, dz, lddz, dw, db, B, H, W, Cin, Cout, 0, accumulate, adam, stream);
}

// ---- off-by-default model variants (train.py:20 block_depth, train.py:26 residual, train.py:29-32 targets) ----------------------
int gct2_conv2d_s1_fwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w, const float* bias, void* y, int ldy, int B, int H, int W,
                       int Cin, int Cout, int KS, int relu, void* stream) {
  gct2_ctx& c = C(ctx);
  if (int e = PlaneTaken(c).none("conv2d_s1_fwd")) return e;
  if (int e = check_conv_args("conv2d_s1_fwd", dtype, x, w, y, B, H, W, Cin, Cout)) return e;
  if (int e = check_s1("conv2d_s1_fwd", KS)) return e;
  if (ldx < Cin || ldy < Cout) return gct2_fail(GCT2_EINVAL, "conv2d_s1_fwd: ld smaller than channel count");
  TapGemmParams p{x, ldx, w, bias, nullptr, 0, y, ldy, B, H, W, Cin, Cout, relu, 0};     // third tap-GEMM form: ks x ks taps on one grid
  p.ks = KS;
  return run_tapgemm(c, dtype, FORM_S1, EPI_BIAS_ACT, p, stream);
}
int gct2_conv2d_s1_dgrad(gct2_ctx* ctx, int dtype, const void* dz, int lddz, const void* w, const void* act, int ldact, void* dx, int lddx, int B,
                         int H, int W, int Cin, int Cout, int KS, int accumulate, void* stream) {
  gct2_ctx& c = C(ctx);
  if (int e = PlaneTaken(c).none("conv2d_s1_dgrad")) return e;
  if (int e = check_conv_args("conv2d_s1_dgrad", dtype, dz, w, dx, B, H, W, Cin, Cout)) return e;
  if (int e = check_s1("conv2d_s1_dgrad", KS)) return e;
  if (lddz < Cout || lddx < Cin || (act && ldact < Cin)) return gct2_fail(GCT2_EINVAL, "conv2d_s1_dgrad: ld smaller than channel count");
  TapGemmParams p{dz, lddz, w, nullptr, act, ldact, dx, lddx, B, H, W, Cout, Cin, 0, accumulate};
  p.ks = KS;
  return run_tapgemm(c, dtype, FORM_S1T, EPI_MASK, p, stream);
}
int gct2_conv2d_s1_wgrad(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* dz, int lddz, float* dw, float* db, int B, int H, int W,
                         int Cin, int Cout, int KS, int accumulate, void* stream) {
  return wgrad_entry(ctx, "conv2d_s1_wgrad", WG_S1, dtype, x, ldx, dz, lddz, dw, db, B, H, W, Cin, Cout, KS, accumulate, nullptr, stream);
}
int gct2_relu_mask(int dtype, const void* act, int ldact, void* d, int ldd, size_t npix, int C, void* stream) {
  if (!dtype_ok(dtype) || !act || !d || C <= 0 || ldact < C || ldd < C) return gct2_fail(GCT2_EINVAL, "relu_mask: bad dtype, null pointer or ld < C");
  if (npix == 0) return GCT2_OK;
  return pw_relu_mask(dtype, act, ldact, d, ldd, npix, C, S(stream));
}
int gct2_add(int dtype, void* dst, int lddst, const void* src, int ldsrc, size_t npix, int C, void* stream) {
  if (!dtype_ok(dtype) || !dst || !src || C <= 0 || lddst < C || ldsrc < C) return gct2_fail(GCT2_EINVAL, "add: bad dtype, null pointer or ld < C");
  if (npix == 0) return GCT2_OK;
  return pw_add(dtype, dst, lddst, src, ldsrc, npix, C, S(stream));
}
int gct2_mix_per_image(const float* x, const float* eps, const float* a, const float* c, float* out, int B, size_t per_image, void* stream) {
  if (!x || !a || !out || (eps && !c) || B <= 0 || per_image == 0) return gct2_fail(GCT2_EINVAL, "mix_per_image: null pointer or empty batch");
  return pw_mix_per_image(x, eps, a, c, out, B, per_image, S(stream));
}

int gct2_dense_fwd(int dtype, const void* x, int ldx, const float* w, const float* b, float* y, int M, int Cin, int Cout, void* stream) {
  if (!dtype_ok(dtype) || !x || !w || !y) return gct2_fail(GCT2_EINVAL, "dense_fwd: bad dtype or null pointer");
  if (M <= 0 || Cin <= 0 || Cout <= 0 || Cout > 4 || ldx < Cin) return gct2_fail(GCT2_EINVAL, "dense_fwd: bad shape (Cout must be 1..4)");
  return pw_dense_fwd(dtype, x, ldx, w, b, y, M, Cin, Cout, S(stream));
}

int gct2_dense_bwd(int dtype, const void* x, int ldx, const float* w, const float* dy, void* dx, int lddx, float* dw, float* db, int M,
                   int Cin, int Cout, int Cmask, int accumulate, void* stream) {
  if (!dtype_ok(dtype) || !x || !w || !dy || !dx || !dw) return gct2_fail(GCT2_EINVAL, "dense_bwd: bad dtype or null pointer");
  if (M <= 0 || Cin <= 0 || Cout <= 0 || Cout > 4 || ldx < Cin || Cmask < 0 || Cmask > Cin || lddx < Cmask)
    return gct2_fail(GCT2_EINVAL, "dense_bwd: bad shape");
  if ((Cin + 1) * Cout > 2048) return gct2_fail(GCT2_EINVAL, "dense_bwd: (Cin+1)*Cout = %d exceeds 2048", (Cin + 1) * Cout);
  if ((size_t)Cin * 16 + 128 * 16 + (size_t)128 * Cin * esize(dtype) > 160 * 1024)
    return gct2_fail(GCT2_EINVAL, "dense_bwd: Cin=%d too large for the LDS tile", Cin);
  return pw_dense_bwd(dtype, x, ldx, w, dy, dx, lddx, dw, db, M, Cin, Cout, Cmask, accumulate, S(stream));
}

// ---- per-timestep heads (train.py:199, 203, 211-214).  The order of the checks is part of the interface. ----
static int check_steps_shape(const char* fn, int B, int HW, int Cin, int Cout, int steps) {
  if (B <= 0 || HW <= 0 || Cin <= 0 || steps <= 0) return gct2_fail(GCT2_EINVAL, "%s: non-positive dimension (B=%d HW=%d Cin=%d steps=%d)", fn, B, HW, Cin, steps);
  if (Cout < 1 || Cout > 4) return gct2_fail(GCT2_EINVAL, "%s: Cout=%d outside 1..4", fn, Cout);
  if (B > 65535 || steps > 65535) return gct2_fail(GCT2_EINVAL, "%s: B=%d / steps=%d beyond 65535 (one grid row per image / per slice)", fn, B, steps);
  if ((size_t)B * HW >= ((size_t)1 << 31)) return gct2_fail(GCT2_EINVAL, "%s: B*HW too large for 32-bit pixel indices", fn);
  if ((size_t)Cin * steps * Cout >= ((size_t)1 << 31)) return gct2_fail(GCT2_EINVAL, "%s: Cin*steps*Cout too large for 32-bit weight indices", fn);
  return GCT2_OK;
}
int gct2_dense_steps_fwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const float* w, const float* b, const int32_t* t_int, float* y,
                         int B, int HW, int Cin, int Cout, int steps, void* stream) {
  if (!dtype_ok(dtype)) return gct2_fail(GCT2_EINVAL, "dense_steps_fwd: unknown dtype %d", dtype);
  if (!x || !w || !t_int || !y) return gct2_fail(GCT2_EINVAL, "dense_steps_fwd: null pointer (x, w, t_int, y)");
  if (int e = check_steps_shape("dense_steps_fwd", B, HW, Cin, Cout, steps)) return e;
  if (ldx < Cin) return gct2_fail(GCT2_EINVAL, "dense_steps_fwd: ldx=%d smaller than Cin=%d", ldx, Cin);
  if ((size_t)Cin * 16 > 64 * 1024) return gct2_fail(GCT2_EINVAL, "dense_steps_fwd: Cin=%d too large for the LDS weight image", Cin);
  if (ctx) gct2_log(*ctx, "dense_steps:fwd");
  return pw_dense_steps_fwd(dtype, x, ldx, w, b, t_int, y, B, HW, Cin, Cout, steps, S(stream));
}
int gct2_dense_steps_scratch(int B, int HW, int Cin, int Cout, size_t* floats) {
  if (!floats) return gct2_fail(GCT2_EINVAL, "dense_steps_scratch: null output pointer");
  if (int e = check_steps_shape("dense_steps_scratch", B, HW, Cin, Cout, 1)) return e;
  if ((Cin + 1) * Cout > 2048) return gct2_fail(GCT2_EINVAL, "dense_steps_scratch: (Cin+1)*Cout = %d exceeds 2048", (Cin + 1) * Cout);
  *floats = dense_steps_scratch_floats(B, HW, Cin, Cout);
  return GCT2_OK;
}
int gct2_dense_steps_bwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const float* w, const int32_t* t_int, const float* dy, void* dx,
                         int lddx, float* dw, float* db, float* scratch, size_t scratch_floats, int B, int HW, int Cin, int Cout, int steps,
                         int Cmask, int accumulate, void* stream) {
  if (!dtype_ok(dtype)) return gct2_fail(GCT2_EINVAL, "dense_steps_bwd: unknown dtype %d", dtype);
  if (!x || !w || !t_int || !dy || !dw || !scratch) return gct2_fail(GCT2_EINVAL, "dense_steps_bwd: null pointer (x, w, t_int, dy, dw, scratch)");
  if (int e = check_steps_shape("dense_steps_bwd", B, HW, Cin, Cout, steps)) return e;
  if (ldx < Cin) return gct2_fail(GCT2_EINVAL, "dense_steps_bwd: ldx=%d smaller than Cin=%d", ldx, Cin);
  if (Cmask < 0 || Cmask > Cin || (dx && lddx < Cmask)) return gct2_fail(GCT2_EINVAL, "dense_steps_bwd: Cmask=%d outside 0..Cin or lddx=%d smaller than it", Cmask, lddx);
  if ((Cin + 1) * Cout > 2048) return gct2_fail(GCT2_EINVAL, "dense_steps_bwd: (Cin+1)*Cout = %d exceeds 2048", (Cin + 1) * Cout);
  if ((size_t)Cin * 16 + 128 * 16 + (size_t)128 * Cin * esize(dtype) > 160 * 1024)
    return gct2_fail(GCT2_EINVAL, "dense_steps_bwd: Cin=%d too large for the LDS tile", Cin);
  if ((uintptr_t)scratch % 16) return gct2_fail(GCT2_EINVAL, "dense_steps_bwd: scratch must be 16-byte aligned");
  const size_t need = dense_steps_scratch_floats(B, HW, Cin, Cout);
  if (scratch_floats < need)
    return gct2_fail(GCT2_EINVAL, "dense_steps_bwd: %zu floats of scratch, this shape needs %zu (gct2_dense_steps_scratch)", scratch_floats, need);
  if (ctx) gct2_log(*ctx, "dense_steps:bwd");
  return pw_dense_steps_bwd(dtype, x, ldx, w, t_int, dy, dx, lddx, dw, db, scratch, B, HW, Cin, Cout, steps, Cmask, accumulate, S(stream));
}

// ---- hidden Dense(pixel_size, relu) + Dense head as one kernel per direction (train.py:195-199).  The order of the checks is part of
// the interface (include/gct2.h): dtype, NULL pointers, non-positive dims, Cout, ldx, [Cmask / lddx], M, weight counts, plain-tile
// limits, [scratch alignment, scratch size]. ----
static int check_dense2_shape(const char* fn, int M, int Cin, int Chid, int Cout, int ldx) {
  if (M <= 0 || Cin <= 0 || Chid <= 0) return gct2_fail(GCT2_EINVAL, "%s: non-positive dimension (M=%d Cin=%d Chid=%d)", fn, M, Cin, Chid);
  if (Cout < 1 || Cout > 4) return gct2_fail(GCT2_EINVAL, "%s: Cout=%d outside 1..4", fn, Cout);
  if (ldx < Cin) return gct2_fail(GCT2_EINVAL, "%s: ldx=%d smaller than Cin=%d", fn, ldx, Cin);
  return GCT2_OK;
}
static int check_dense2_sizes(const char* fn, int M, int Cin, int Chid, int Cout) {
  if ((size_t)M + GCT2_DENSE2_FAST_PIXELS >= ((size_t)1 << 31)) return gct2_fail(GCT2_EINVAL, "%s: M=%d too large for 32-bit pixel indices", fn, M);
  if ((size_t)Cin * Chid >= ((size_t)1 << 31) || (size_t)Chid * Cout >= ((size_t)1 << 31))
    return gct2_fail(GCT2_EINVAL, "%s: Cin*Chid or Chid*Cout too large for 32-bit weight indices", fn);
  if (Cin > GCT2_DENSE2_PLAIN_MAX || Chid > GCT2_DENSE2_PLAIN_MAX)
    return gct2_fail(GCT2_EINVAL, "%s: Cin=%d / Chid=%d beyond %d, the plain kernel's LDS tile", fn, Cin, Chid, GCT2_DENSE2_PLAIN_MAX);
  return GCT2_OK;
}
int gct2_dense2_fwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w1, const float* b1, const float* w2, const float* b2, float* y,
                    int M, int Cin, int Chid, int Cout, void* stream) {
  if (!dtype_ok(dtype)) return gct2_fail(GCT2_EINVAL, "dense2_fwd: unknown dtype %d", dtype);
  if (!x || !w1 || !b1 || !w2 || !b2 || !y) return gct2_fail(GCT2_EINVAL, "dense2_fwd: null pointer (x, w1, b1, w2, b2, y)");
  if (int e = check_dense2_shape("dense2_fwd", M, Cin, Chid, Cout, ldx)) return e;
  if (int e = check_dense2_sizes("dense2_fwd", M, Cin, Chid, Cout)) return e;
  return dense2_fwd(C(ctx), dtype, x, ldx, w1, b1, w2, b2, y, M, Cin, Chid, Cout, S(stream));
}
int gct2_dense2_scratch(int M, int Cin, int Chid, int Cout, size_t* floats) {
  if (!floats) return gct2_fail(GCT2_EINVAL, "dense2_scratch: null output pointer");
  if (int e = check_dense2_shape("dense2_scratch", M, Cin, Chid, Cout, Cin)) return e;
  if (int e = check_dense2_sizes("dense2_scratch", M, Cin, Chid, Cout)) return e;
  *floats = dense2_scratch_floats(M, Cin, Chid, Cout);
  return GCT2_OK;
}
int gct2_dense2_bwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w1, const float* b1, const float* w2, const float* dy, void* dx,
                    int lddx, float* dw1, float* db1, float* dw2, float* db2, float* scratch, size_t scratch_floats, int M, int Cin, int Chid,
                    int Cout, int Cmask, int accumulate, void* stream) {
  if (!dtype_ok(dtype)) return gct2_fail(GCT2_EINVAL, "dense2_bwd: unknown dtype %d", dtype);
  if (!x || !w1 || !b1 || !w2 || !dy || !dw1 || !db1 || !dw2 || !db2 || !scratch)
    return gct2_fail(GCT2_EINVAL, "dense2_bwd: null pointer (x, w1, b1, w2, dy, dw1, db1, dw2, db2, scratch)");
  if (int e = check_dense2_shape("dense2_bwd", M, Cin, Chid, Cout, ldx)) return e;
  if (Cmask < 0 || Cmask > Cin || (dx && lddx < Cmask))
    return gct2_fail(GCT2_EINVAL, "dense2_bwd: Cmask=%d outside 0..Cin or lddx=%d smaller than it", Cmask, lddx);
  if (int e = check_dense2_sizes("dense2_bwd", M, Cin, Chid, Cout)) return e;
  if ((uintptr_t)scratch % 16) return gct2_fail(GCT2_EINVAL, "dense2_bwd: scratch must be 16-byte aligned");
  const size_t need = dense2_scratch_floats(M, Cin, Chid, Cout);
  if (scratch_floats < need)
    return gct2_fail(GCT2_EINVAL, "dense2_bwd: %zu floats of scratch, this shape needs %zu (gct2_dense2_scratch)", scratch_floats, need);
  return dense2_bwd(C(ctx), dtype, x, ldx, w1, b1, w2, dy, dx, lddx, dw1, db1, dw2, db2, scratch, M, Cin, Chid, Cout, Cmask, accumulate, S(stream));
}

int gct2_dense_head_train(gct2_ctx* ctx, int dtype, const void* x, int ldx, const float* w, const float* b, const float* target, float* pred,
                          void* dx, int lddx, float* dw, float* db, float* loss, float* partials, int M, int Cin, int Cout, int Cmask,
                          const float* loss_scale_ptr, float* db_dx, const void* x2, int ldx2, int accumulate, void* stream) {
  gct2_ctx& c = C(ctx);
  if (int e = PlaneTaken(c).none("dense_head_train")) return e;
  if ((dtype != GCT2_BF16 && dtype != GCT2_F16) || !x || !w || !target || !dx || !dw || !loss || !partials)
    return gct2_fail(GCT2_EINVAL, "dense_head_train: 16-bit dtypes only / null pointer (use dense_fwd + mse_fwd_bwd + dense_bwd)");
  if (x2 && (ldx2 < Cin - Cmask || ldx2 % 4 || (uintptr_t)x2 % 8 || Cin - Cmask > 4))
    return gct2_fail(GCT2_EINVAL, "dense_head_train: x2 holds at most 4 channels per pixel in 8-byte aligned rows (ldx2 multiple of 4)");
  if (M <= 0 || Cin <= 0 || Cout <= 0 || Cout > 4 || ldx < (x2 ? Cmask : Cin) || ldx % 8 || lddx % 8 || Cmask % 8 || Cmask <= 0 || Cmask > Cin ||
      lddx < Cmask || (Cin + 1) * Cout > 256)
    return gct2_fail(GCT2_EINVAL, "dense_head_train: bad shape (need ldx, lddx, Cmask multiples of 8, (Cin+1)*Cout <= 256)");
  if ((uintptr_t)x % 16 || (uintptr_t)dx % 16) return gct2_fail(GCT2_EINVAL, "dense_head_train: views must be 16-byte aligned");
  if ((size_t)256 * ldx * 2 + (size_t)256 * Cmask * 2 + 256 * 16 + (size_t)ldx * 16 > 160 * 1024)
    return gct2_fail(GCT2_EINVAL, "dense_head_train: ldx=%d too large for the LDS tile", ldx);
  return pw_dense_head_train(c, dtype, x, ldx, w, b, target, pred, dx, lddx, dw, db, loss, partials, M, Cin, Cout, Cmask, loss_scale_ptr,
                             db_dx, x2, ldx2, accumulate, S(stream));
}

int gct2_rng_uniform_int(uint64_t seed, uint64_t stream_id, uint64_t offset, int32_t* out, size_t n, int lo, int hi, void* stream) {
  if (!out || hi < lo) return gct2_fail(GCT2_EINVAL, "rng_uniform_int: null output or empty range");
  return pw_rng_uniform_int(seed, stream_id, offset, out, n, lo, hi, S(stream));
}
int gct2_rng_normal(uint64_t seed, uint64_t stream_id, uint64_t offset, float* out, size_t n, void* stream) {
  if (!out) return gct2_fail(GCT2_EINVAL, "rng_normal: null output");
  return pw_rng_normal(seed, stream_id, offset, out, n, S(stream));
}

int gct2_noise_image(int dtype, const float* x, const int32_t* t_int, const float* eps, void* out, int ldout, void* out2, int ldout2,
                     int B, int HW, int C, int steps, void* stream) {
  if (!dtype_ok(dtype) || !x || !t_int || !eps || !out) return gct2_fail(GCT2_EINVAL, "noise_image: bad dtype or null pointer");
  if (B <= 0 || HW <= 0 || C <= 0 || ldout < C || (out2 && ldout2 < C) || steps <= 0) return gct2_fail(GCT2_EINVAL, "noise_image: bad shape");
  return pw_noise(dtype, x, t_int, eps, out, ldout, out2, ldout2, B, HW, C, steps, S(stream));
}

int gct2_noise_image_rng(int dtype, const float* x, const int32_t* t_int, uint64_t seed, uint64_t stream_id, uint64_t offset,
                         float* eps_out, void* out, int ldout, void* out2, int ldout2, int B, int HW, int C, int steps, void* stream) {
  if (!dtype_ok(dtype) || !x || !t_int || !out) return gct2_fail(GCT2_EINVAL, "noise_image_rng: bad dtype or null pointer");
  if (B <= 0 || HW <= 0 || C <= 0 || ldout < C || (out2 && ldout2 < C) || steps <= 0 || (size_t)B * HW * C >= ((size_t)1 << 31))
    return gct2_fail(GCT2_EINVAL, "noise_image_rng: bad shape");
  return pw_noise_rng(dtype, x, t_int, seed, stream_id, offset, eps_out, out, ldout, out2, ldout2, B, HW, C, steps, S(stream));
}

// the table forms: coef = float[steps][2], entry t - 1 = (sa, sb), read as one 8-byte load per thread
static int noise_table_ok(const char* who, const float* coef, int steps) {
  if (!coef || (uintptr_t)coef % 8) return gct2_fail(GCT2_EINVAL, "%s: coef is NULL or not 8-byte aligned", who);
  if (steps < 1) return gct2_fail(GCT2_EINVAL, "%s: steps must be >= 1", who);
  return GCT2_OK;
}

int gct2_noise_image_table(int dtype, const float* x, const int32_t* t_int, const float* eps, const float* coef, void* out, int ldout,
                           void* out2, int ldout2, int B, int HW, int C, int steps, void* stream) {
  if (!dtype_ok(dtype) || !x || !t_int || !eps || !out) return gct2_fail(GCT2_EINVAL, "noise_image_table: bad dtype or null pointer");
  if (int rc = noise_table_ok("noise_image_table", coef, steps)) return rc;
  if (B <= 0 || HW <= 0 || C <= 0 || ldout < C || (out2 && ldout2 < C)) return gct2_fail(GCT2_EINVAL, "noise_image_table: bad shape");
  return pw_noise_table(dtype, x, t_int, eps, coef, out, ldout, out2, ldout2, B, HW, C, steps, S(stream));
}

int gct2_noise_image_rng_table(int dtype, const float* x, const int32_t* t_int, uint64_t seed, uint64_t stream_id, uint64_t offset,
                               float* eps_out, const float* coef, void* out, int ldout, void* out2, int ldout2, int B, int HW, int C,
                               int steps, void* stream) {
  if (!dtype_ok(dtype) || !x || !t_int || !out) return gct2_fail(GCT2_EINVAL, "noise_image_rng_table: bad dtype or null pointer");
  if (int rc = noise_table_ok("noise_image_rng_table", coef, steps)) return rc;
  if (B <= 0 || HW <= 0 || C <= 0 || ldout < C || (out2 && ldout2 < C) || (size_t)B * HW * C >= ((size_t)1 << 31))
    return gct2_fail(GCT2_EINVAL, "noise_image_rng_table: bad shape");
  return pw_noise_rng_table(dtype, x, t_int, seed, stream_id, offset, eps_out, coef, out, ldout, out2, ldout2, B, HW, C, steps, S(stream));
}

int gct2_diffusion_mix(int dtype, const float* x_theta, const float* eps_theta, float alpha, float* fake, void* out, int ldout, void* out2,
                       int ldout2, size_t npix, int C, void* stream) {
  if (!dtype_ok(dtype) || !x_theta || !eps_theta || !fake || !out) return gct2_fail(GCT2_EINVAL, "diffusion_mix: bad dtype or null pointer");
  if (npix == 0 || C <= 0 || ldout < C || (out2 && ldout2 < C) || !(alpha >= 0.f && alpha <= 1.f))
    return gct2_fail(GCT2_EINVAL, "diffusion_mix: bad shape or alpha outside [0, 1]");
  return pw_diffusion_mix(dtype, x_theta, eps_theta, alpha, fake, out, ldout, out2, ldout2, npix, C, S(stream));
}

int gct2_diffusion_update(int mode, const float* pred, const float* fake, double alpha, double alpha_prev, float* x_theta, float* eps_theta,
                          size_t n, void* stream) {
  if ((mode < GCT2_SAMPLE_X || mode > GCT2_SAMPLE_ODE) && mode != GCT2_SAMPLE_V) return gct2_fail(GCT2_EINVAL, "diffusion_update: unknown mode %d", mode);
  if (!pred || !fake || !x_theta || (!eps_theta && mode != GCT2_SAMPLE_ODE) || n == 0)
    return gct2_fail(GCT2_EINVAL, "diffusion_update: null pointer or n == 0");
  if (!(alpha >= 0. && alpha < 1.)) return gct2_fail(GCT2_EINVAL, "diffusion_update: alpha must be in [0, 1)");
  if (mode != GCT2_SAMPLE_X && mode != GCT2_SAMPLE_V && !(alpha > 0.)) return gct2_fail(GCT2_EINVAL, "diffusion_update: this mode divides by sqrt(alpha): alpha must be > 0");
  if (mode == GCT2_SAMPLE_ODE) {
    if (!(alpha_prev >= 0. && alpha_prev <= 1.)) return gct2_fail(GCT2_EINVAL, "diffusion_update: alpha_prev must be in [0, 1]");
    if (sqrt(alpha_prev) * sqrt(1. - alpha) - sqrt(alpha) * sqrt(1. - alpha_prev) == 0.)
      return gct2_fail(GCT2_EINVAL, "diffusion_update: alpha == alpha_prev makes the ODE step singular (train.py:386-391)");
  }
  return pw_diffusion_update(mode, pred, fake, alpha, alpha_prev, x_theta, eps_theta, n, S(stream));
}

// the image views of gct2_diffusion_step / _start: B images of per_image = H*W*C elements, flat indices below 2^31
static int step_views_ok(const char* who, int dtype, const float* fake_out, const void* out, int ldout, const void* out2, int ldout2, int B,
                         size_t per_image, int C) {
  if (!dtype_ok(dtype) || !fake_out || !out) return gct2_fail(GCT2_EINVAL, "%s: bad dtype or null pointer", who);
  if (B <= 0 || per_image == 0 || C <= 0 || per_image % (size_t)C || ldout < C || (out2 && ldout2 < C) ||
      per_image >= ((size_t)1 << 31) || (size_t)B * per_image >= ((size_t)1 << 31))
    return gct2_fail(GCT2_EINVAL, "%s: bad shape (per_image a multiple of C, ldout >= C, B * per_image < 2^31)", who);
  return GCT2_OK;
}

// the scalars every step shares, in the order every step checks them: the objective mode in front of the pointers and views ...
static int step_mode_ok(const char* who, int mode) {
  if ((mode < GCT2_SAMPLE_X || mode > GCT2_SAMPLE_SCALED_EPS) && mode != GCT2_SAMPLE_V)
    return gct2_fail(GCT2_EINVAL, "%s: mode %d (the ODE objective predicts one step back only: gct2_diffusion_update)", who, mode);
  return GCT2_OK;
}
// ... a_t and a_prev behind them
static int step_scalars_ok(const char* who, int mode, double a_t, double a_prev) {
  if (!(a_t >= 0. && a_t < 1.)) return gct2_fail(GCT2_EINVAL, "%s: a_t must be in [0, 1)", who);
  if (mode != GCT2_SAMPLE_X && mode != GCT2_SAMPLE_V && !(a_t > 0.))
    return gct2_fail(GCT2_EINVAL, "%s: this mode divides by sqrt(a_t): a_t must be > 0", who);
  if (!(a_prev >= 0. && a_prev <= 1.)) return gct2_fail(GCT2_EINVAL, "%s: a_prev must be in [0, 1]", who);
  return GCT2_OK;
}
static int step_sigma2_ok(const char* who, double a_prev, double sigma2) {
  if (!(sigma2 >= 0.) || !((1.f - (float)a_prev) - (float)sigma2 >= 0.f)) return gct2_fail(GCT2_EINVAL, "%s: sigma2 must be in [0, 1 - a_prev]", who);
  return GCT2_OK;
}
// the fields every step fills the same way
static SamplerStep step_views(int mode, int dtype, uint64_t seed, uint64_t stream_id, uint64_t image_stride, float* fake_out, void* out,
                              int ldout, void* out2, int ldout2, int B, size_t per_image, int C) {
  SamplerStep st;
  st.mode = mode; st.dtype = dtype;
  st.seed = seed; st.stream_id = stream_id; st.image_stride = image_stride;
  st.fake_out = fake_out; st.out = out; st.ldout = ldout; st.out2 = out2; st.ldout2 = ldout2;
  st.B = B; st.per_image = per_image; st.C = C;
  return st;
}

int gct2_diffusion_step(int mode, int dtype, const float* pred, const float* fake_in, double a_t, double a_prev, double sigma2, double clip,
                        uint64_t seed, uint64_t stream_id, uint64_t offset, uint64_t image_stride, float* fake_out, float* x0_out, void* out,
                        int ldout, void* out2, int ldout2, int B, size_t per_image, int C, void* stream) {
  const char* who = "diffusion_step";
  if (int rc = step_mode_ok(who, mode)) return rc;
  if (!pred || !fake_in) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (int rc = step_views_ok(who, dtype, fake_out, out, ldout, out2, ldout2, B, per_image, C)) return rc;
  if (int rc = step_scalars_ok(who, mode, a_t, a_prev)) return rc;
  if (int rc = step_sigma2_ok(who, a_prev, sigma2)) return rc;
  SamplerStep st = step_views(mode, dtype, seed, stream_id, image_stride, fake_out, out, ldout, out2, ldout2, B, per_image, C);
  st.pred = pred; st.fake_in = fake_in; st.a = a_t; st.a_prev = a_prev; st.sigma2 = sigma2; st.clip = clip;
  st.offset = offset; st.x0_out = x0_out;
  return pw_sampler_step(who, st, S(stream));
}

int gct2_diffusion_start(int dtype, uint64_t seed, uint64_t stream_id, uint64_t offset, uint64_t image_stride, float* fake_out, void* out,
                         int ldout, void* out2, int ldout2, int B, size_t per_image, int C, void* stream) {
  const char* who = "diffusion_start";
  if (int rc = step_views_ok(who, dtype, fake_out, out, ldout, out2, ldout2, B, per_image, C)) return rc;
  SamplerStep st = step_views(STEP_START, dtype, seed, stream_id, image_stride, fake_out, out, ldout, out2, ldout2, B, per_image, C);
  st.offset = offset;
  return pw_sampler_step(who, st, S(stream));
}

int gct2_diffusion_start_image(int dtype, const float* known, double a, uint64_t seed, uint64_t stream_id, uint64_t offset,
                               uint64_t image_stride, float* fake_out, void* out, int ldout, void* out2, int ldout2, int B, size_t per_image,
                               int C, void* stream) {
  const char* who = "diffusion_start_image";
  if (!known) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (int rc = step_views_ok(who, dtype, fake_out, out, ldout, out2, ldout2, B, per_image, C)) return rc;
  if (!(a >= 0. && a <= 1.)) return gct2_fail(GCT2_EINVAL, "%s: a must be in [0, 1]", who);
  SamplerStep st = step_views(STEP_START_IMAGE, dtype, seed, stream_id, image_stride, fake_out, out, ldout, out2, ldout2, B, per_image, C);
  st.known = known; st.a = a; st.offset0 = offset;
  return pw_sampler_step(who, st, S(stream));
}

int gct2_diffusion_step_masked(int mode, int dtype, const float* pred, const float* fake_in, const float* known, const float* mask, double a_t,
                               double a_prev, double sigma2, double clip, uint64_t seed, uint64_t stream_id, uint64_t offset, uint64_t offset0,
                               uint64_t image_stride, float* fake_out, float* x0_out, void* out, int ldout, void* out2, int ldout2, int B,
                               size_t per_image, int C, void* stream) {
  const char* who = "diffusion_step_masked";
  if (int rc = step_mode_ok(who, mode)) return rc;
  if (!pred || !fake_in || !known || !mask) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (int rc = step_views_ok(who, dtype, fake_out, out, ldout, out2, ldout2, B, per_image, C)) return rc;
  if (int rc = step_scalars_ok(who, mode, a_t, a_prev)) return rc;
  if (int rc = step_sigma2_ok(who, a_prev, sigma2)) return rc;
  SamplerStep st = step_views(mode, dtype, seed, stream_id, image_stride, fake_out, out, ldout, out2, ldout2, B, per_image, C);
  st.pred = pred; st.fake_in = fake_in; st.known = known; st.mask = mask;
  st.a = a_t; st.a_prev = a_prev; st.sigma2 = sigma2; st.clip = clip;
  st.offset = offset; st.offset0 = offset0; st.x0_out = x0_out;
  return pw_sampler_step(who, st, S(stream));
}

int gct2_diffusion_step_multistep(int mode, int dtype, const float* pred, const float* fake_in, const float* hist_in, const float* known,
                                  const float* mask, double a_t, double a_prev, double c1, double clip, uint64_t seed, uint64_t stream_id,
                                  uint64_t offset0, uint64_t image_stride, float* fake_out, float* hist_out, float* x0_out, void* out, int ldout,
                                  void* out2, int ldout2, int B, size_t per_image, int C, void* stream) {
  const char* who = "diffusion_step_multistep";
  if (int rc = step_mode_ok(who, mode)) return rc;
  if (!pred || !fake_in) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (!known != !mask) return gct2_fail(GCT2_EINVAL, "%s: known and mask go together (both NULL: the plain step)", who);
  if (int rc = step_views_ok(who, dtype, fake_out, out, ldout, out2, ldout2, B, per_image, C)) return rc;
  if (int rc = step_scalars_ok(who, mode, a_t, a_prev)) return rc;
  if (!std::isfinite(c1) || !std::isfinite((float)c1)) return gct2_fail(GCT2_EINVAL, "%s: c1 must be finite in fp32", who);
  if ((float)c1 != 0.f && !hist_in) return gct2_fail(GCT2_EINVAL, "%s: c1 != 0 extrapolates from hist_in, which is NULL", who);
  SamplerStep st = step_views(mode, dtype, seed, stream_id, image_stride, fake_out, out, ldout, out2, ldout2, B, per_image, C);
  st.pred = pred; st.fake_in = fake_in; st.hist_in = hist_in; st.known = known; st.mask = mask;
  st.a = a_t; st.a_prev = a_prev; st.c1 = c1; st.clip = clip; st.multistep = true;
  st.offset0 = offset0; st.hist_out = hist_out; st.x0_out = x0_out;
  return pw_sampler_step(who, st, S(stream));
}

int gct2_x0_quantile_scratch(int B, size_t per_image, size_t* bytes) {
  if (!bytes || B <= 0 || per_image == 0 || (size_t)B * per_image >= ((size_t)1 << 31))
    return gct2_fail(GCT2_EINVAL, "x0_quantile_scratch: null pointer or bad shape (B * per_image < 2^31)");
  *bytes = pw_x0_quantile_scratch(B);
  return GCT2_OK;
}

int gct2_x0_quantile(int mode, const float* pred, const float* fake, double a_t, uint32_t rank, double floor, float* rows, float* q_out,
                     void* scratch, size_t scratch_bytes, int B, size_t per_image, void* stream) {
  const char* who = "x0_quantile";
  if (int rc = step_mode_ok(who, mode)) return rc;
  if (!pred || (!fake && mode != GCT2_SAMPLE_X) || !rows || !scratch) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (B <= 0 || per_image == 0 || (size_t)B * per_image >= ((size_t)1 << 31))
    return gct2_fail(GCT2_EINVAL, "%s: bad shape (B * per_image < 2^31)", who);
  if (!(a_t >= 0. && a_t < 1.)) return gct2_fail(GCT2_EINVAL, "%s: a_t must be in [0, 1)", who);
  if (mode != GCT2_SAMPLE_X && mode != GCT2_SAMPLE_V && !(a_t > 0.))
    return gct2_fail(GCT2_EINVAL, "%s: this mode divides by sqrt(a_t): a_t must be > 0", who);
  if (rank < 1 || rank > per_image) return gct2_fail(GCT2_EINVAL, "%s: rank must be in 1..per_image", who);
  if (!std::isfinite(floor) || !std::isfinite((float)floor) || !((float)floor > 0.f))
    return gct2_fail(GCT2_EINVAL, "%s: floor must be finite and > 0 in fp32", who);
  if (scratch_bytes < pw_x0_quantile_scratch(B)) return gct2_fail(GCT2_EINVAL, "%s: scratch too small (gct2_x0_quantile_scratch)", who);
  return pw_x0_quantile(mode, pred, fake, a_t, rank, (float)floor, rows, q_out, scratch, B, per_image, false, nullptr, 1.f, S(stream));
}

int gct2_diffusion_step_dynamic(int mode, int dtype, const float* pred, const float* fake_in, const float* hist_in, const float* known,
                                const float* mask, const float* rows, double a_t, double a_prev, double sigma2, double c1, uint64_t seed,
                                uint64_t stream_id, uint64_t offset, uint64_t offset0, uint64_t image_stride, float* fake_out, float* hist_out,
                                float* x0_out, void* out, int ldout, void* out2, int ldout2, int B, size_t per_image, int C, void* stream) {
  const char* who = "diffusion_step_dynamic";
  if (int rc = step_mode_ok(who, mode)) return rc;
  if (!pred || !fake_in || !rows) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (!known != !mask) return gct2_fail(GCT2_EINVAL, "%s: known and mask go together (both NULL: the plain step)", who);
  if (int rc = step_views_ok(who, dtype, fake_out, out, ldout, out2, ldout2, B, per_image, C)) return rc;
  if (int rc = step_scalars_ok(who, mode, a_t, a_prev)) return rc;
  if (int rc = step_sigma2_ok(who, a_prev, sigma2)) return rc;
  if (!std::isfinite(c1) || !std::isfinite((float)c1)) return gct2_fail(GCT2_EINVAL, "%s: c1 must be finite in fp32", who);
  if ((float)c1 != 0.f && !hist_in) return gct2_fail(GCT2_EINVAL, "%s: c1 != 0 extrapolates from hist_in, which is NULL", who);
  // the multistep form: a history plane on either side, or an extrapolation
  const bool multistep = hist_in || hist_out || (float)c1 != 0.f;
  if (multistep && (float)sigma2 != 0.f) return gct2_fail(GCT2_EINVAL, "%s: the multistep form is deterministic: sigma2 must be 0", who);
  SamplerStep st = step_views(mode, dtype, seed, stream_id, image_stride, fake_out, out, ldout, out2, ldout2, B, per_image, C);
  st.pred = pred; st.fake_in = fake_in; st.hist_in = hist_in; st.known = known; st.mask = mask; st.rows = rows;
  st.a = a_t; st.a_prev = a_prev; st.sigma2 = sigma2; st.c1 = c1; st.multistep = multistep;
  st.offset = offset; st.offset0 = offset0; st.hist_out = hist_out; st.x0_out = x0_out;
  return pw_sampler_step(who, st, S(stream));
}

// ---- two-network guidance: the select and the step on p = pred_guide + w (pred - pred_guide), never materialised
static int guide_weight_ok(const char* who, double w) {
  if (!std::isfinite(w) || !std::isfinite((float)w)) return gct2_fail(GCT2_EINVAL, "%s: w must be finite in fp32", who);
  return GCT2_OK;
}

int gct2_x0_quantile_guided(int mode, const float* pred, const float* pred_guide, double w, const float* fake, double a_t, uint32_t rank,
                            double floor, float* rows, float* q_out, void* scratch, size_t scratch_bytes, int B, size_t per_image,
                            void* stream) {
  const char* who = "x0_quantile_guided";
  if (int rc = step_mode_ok(who, mode)) return rc;
  if (!pred || !pred_guide || (!fake && mode != GCT2_SAMPLE_X) || !rows || !scratch) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (int rc = guide_weight_ok(who, w)) return rc;
  if (B <= 0 || per_image == 0 || (size_t)B * per_image >= ((size_t)1 << 31))
    return gct2_fail(GCT2_EINVAL, "%s: bad shape (B * per_image < 2^31)", who);
  if (!(a_t >= 0. && a_t < 1.)) return gct2_fail(GCT2_EINVAL, "%s: a_t must be in [0, 1)", who);
  if (mode != GCT2_SAMPLE_X && mode != GCT2_SAMPLE_V && !(a_t > 0.))
    return gct2_fail(GCT2_EINVAL, "%s: this mode divides by sqrt(a_t): a_t must be > 0", who);
  if (rank < 1 || rank > per_image) return gct2_fail(GCT2_EINVAL, "%s: rank must be in 1..per_image", who);
  if (!std::isfinite(floor) || !std::isfinite((float)floor) || !((float)floor > 0.f))
    return gct2_fail(GCT2_EINVAL, "%s: floor must be finite and > 0 in fp32", who);
  if (scratch_bytes < pw_x0_quantile_scratch(B)) return gct2_fail(GCT2_EINVAL, "%s: scratch too small (gct2_x0_quantile_scratch)", who);
  return pw_x0_quantile(mode, pred, fake, a_t, rank, (float)floor, rows, q_out, scratch, B, per_image, true, pred_guide, (float)w, S(stream));
}

int gct2_diffusion_step_guided(int mode, int dtype, const float* pred, const float* pred_guide, double w, const float* fake_in,
                               const float* hist_in, const float* known, const float* mask, const float* rows, double a_t, double a_prev,
                               double sigma2, double c1, double clip, uint64_t seed, uint64_t stream_id, uint64_t offset, uint64_t offset0,
                               uint64_t image_stride, float* fake_out, float* hist_out, float* x0_out, void* out, int ldout, void* out2,
                               int ldout2, void* out3, int ldout3, void* out4, int ldout4, int B, size_t per_image, int C, void* stream) {
  const char* who = "diffusion_step_guided";
  if (int rc = step_mode_ok(who, mode)) return rc;
  if (!pred || !fake_in) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (int rc = guide_weight_ok(who, w)) return rc;
  if (!pred_guide && (float)w != 1.f) return gct2_fail(GCT2_EINVAL, "%s: pred_guide is NULL (p = pred): w must be 1", who);
  if (rows && clip != 0.) return gct2_fail(GCT2_EINVAL, "%s: rows is the per-image bound: clip must be 0", who);
  if (!known != !mask) return gct2_fail(GCT2_EINVAL, "%s: known and mask go together (both NULL: the plain step)", who);
  if (int rc = step_views_ok(who, dtype, fake_out, out, ldout, out2, ldout2, B, per_image, C)) return rc;
  if (out4 && !out3) return gct2_fail(GCT2_EINVAL, "%s: out4 without out3", who);
  if ((out3 && ldout3 < C) || (out4 && ldout4 < C)) return gct2_fail(GCT2_EINVAL, "%s: ldout3 / ldout4 must be >= C", who);
  if (int rc = step_scalars_ok(who, mode, a_t, a_prev)) return rc;
  if (int rc = step_sigma2_ok(who, a_prev, sigma2)) return rc;
  if (!std::isfinite(c1) || !std::isfinite((float)c1)) return gct2_fail(GCT2_EINVAL, "%s: c1 must be finite in fp32", who);
  if ((float)c1 != 0.f && !hist_in) return gct2_fail(GCT2_EINVAL, "%s: c1 != 0 extrapolates from hist_in, which is NULL", who);
  // the multistep form: a history plane on either side, or an extrapolation
  const bool multistep = hist_in || hist_out || (float)c1 != 0.f;
  if (multistep && (float)sigma2 != 0.f) return gct2_fail(GCT2_EINVAL, "%s: the multistep form is deterministic: sigma2 must be 0", who);
  SamplerStep st = step_views(mode, dtype, seed, stream_id, image_stride, fake_out, out, ldout, out2, ldout2, B, per_image, C);
  st.pred = pred; st.fake_in = fake_in; st.hist_in = hist_in; st.known = known; st.mask = mask; st.rows = rows;
  st.a = a_t; st.a_prev = a_prev; st.sigma2 = sigma2; st.c1 = c1; st.clip = clip; st.multistep = multistep;
  st.offset = offset; st.offset0 = offset0; st.hist_out = hist_out; st.x0_out = x0_out;
  st.guided = true; st.pred_guide = pred_guide; st.w = w;
  st.out3 = out3; st.ldout3 = ldout3; st.out4 = out4; st.ldout4 = ldout4;
  return pw_sampler_step(who, st, S(stream));
}

// ---- progressive distillation (distill.hip): the per-image forms of the start from an image and of the sigma^2 = 0 step, and the
// teacher's second step fused with the target solve
int gct2_distill_start(int dtype, const float* x, const float* eps, const int32_t* pair, const float* table, const int32_t* ttable, int N, uint64_t seed,
                       uint64_t stream_id, uint64_t offset, uint64_t image_stride, float* z0_out, int32_t* t_out, int32_t* t1_out, void* out,
                       int ldout, void* out2, int ldout2, int B, size_t per_image, int C, void* stream) {
  const char* who = "distill_start";
  if (!x || !pair || !table || !ttable) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (N < 1) return gct2_fail(GCT2_EINVAL, "%s: N must be >= 1", who);
  if (int rc = step_views_ok(who, dtype, z0_out, out, ldout, out2, ldout2, B, per_image, C)) return rc;
  return pw_distill_start(dtype, x, eps, pair, table, ttable, N, seed, stream_id, offset, image_stride, z0_out, t_out, t1_out, out, ldout, out2,
                          ldout2, B, per_image, C, S(stream));
}

int gct2_distill_step(int mode, int dtype, const float* pred, const float* z0, const int32_t* pair, const float* table, int N, double clip,
                      float* z1_out, void* out, int ldout, void* out2, int ldout2, int B, size_t per_image, int C, void* stream) {
  const char* who = "distill_step";
  if (int rc = step_mode_ok(who, mode)) return rc;
  if (!pred || !z0 || !pair || !table) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (N < 1) return gct2_fail(GCT2_EINVAL, "%s: N must be >= 1", who);
  if (int rc = step_views_ok(who, dtype, z1_out, out, ldout, out2, ldout2, B, per_image, C)) return rc;
  return pw_distill_step(mode, dtype, pred, z0, pair, table, N, clip, z1_out, out, ldout, out2, ldout2, B, per_image, C, S(stream));
}

int gct2_distill_target(int mode, const float* pred2, const float* z1, const float* z0, const int32_t* pair, const float* table, int N,
                        double clip, float* x_out, float* eps_out, int B, size_t per_image, void* stream) {
  const char* who = "distill_target";
  if (int rc = step_mode_ok(who, mode)) return rc;
  if (!pred2 || !z1 || !z0 || !pair || !table || !x_out || !eps_out) return gct2_fail(GCT2_EINVAL, "%s: null pointer", who);
  if (N < 1) return gct2_fail(GCT2_EINVAL, "%s: N must be >= 1", who);
  if (B <= 0 || per_image == 0 || per_image >= ((size_t)1 << 31) || (size_t)B * per_image >= ((size_t)1 << 31))
    return gct2_fail(GCT2_EINVAL, "%s: bad shape (B * per_image < 2^31)", who);
  return pw_distill_target(mode, pred2, z1, z0, pair, table, N, clip, x_out, eps_out, B, per_image, S(stream));
}

int gct2_noise_edits(const float* eps, const float* dictionary, int K, float* out, int H, int W, int C, void* stream) {
  if (!eps || !dictionary || !out) return gct2_fail(GCT2_EINVAL, "noise_edits: null pointer");
  if (H <= 0 || W <= 0 || C <= 0 || K <= 0 || (H & 3) || (W & 3))
    return gct2_fail(GCT2_EINVAL, "noise_edits: H=%d W=%d must be positive multiples of 4 (avg_pool2d(4, 4, 'SAME') without padding)", H, W);
  return pw_noise_edits(eps, dictionary, K, out, H, W, C, S(stream));
}

int gct2_image_prepare(const uint8_t* src, const int64_t* offsets, const int32_t* dims, float* dst, int B, int size, void* stream) {
  if (!src || !offsets || !dims || !dst || B <= 0 || size <= 0) return gct2_fail(GCT2_EINVAL, "image_prepare: null pointer or empty batch");
  return pw_image_prepare(src, offsets, dims, dst, B, size, S(stream));
}

int gct2_image_batch_cached(const uint8_t* pool, const int64_t* offsets, const int32_t* hw, int N, uint64_t seed, uint64_t first_sample,
                            uint64_t sample_stride, int flags, const int32_t* picks_in, int32_t* picks_out, float* dst, int B, int size,
                            void* stream) {
  if (!pool || !offsets || !hw || !dst) return gct2_fail(GCT2_EINVAL, "image_batch_cached: null pointer (pool, offsets, hw, dst)");
  if (B <= 0 || N <= 0 || size <= 0) return gct2_fail(GCT2_EINVAL, "image_batch_cached: B=%d N=%d size=%d must be positive", B, N, size);
  if (size > 16384) return gct2_fail(GCT2_EINVAL, "image_batch_cached: size=%d is larger than 16384", size);
  if (flags & ~(GCT2_DATA_SHUFFLE | GCT2_DATA_RANDOM_CROP | GCT2_DATA_FLIP)) return gct2_fail(GCT2_EINVAL, "image_batch_cached: unknown flag bits in %d", flags);
  if (sample_stride == 0) return gct2_fail(GCT2_EINVAL, "image_batch_cached: sample_stride == 0");
  return data_image_batch_cached(pool, offsets, hw, N, seed, first_sample, sample_stride, flags, picks_in, picks_out, dst, B, size, S(stream));
}

int gct2_image_grid_u8(const void* src, int dtype, int n, int H, int W, int mode, int cols, int rows, int pad, int scale, uint32_t fill_rgb,
                       uint8_t* out, void* stream) {
  if (!src || !out) return gct2_fail(GCT2_EINVAL, "image_grid_u8: null pointer (src, out)");
  if (!dtype_ok(dtype)) return gct2_fail(GCT2_EINVAL, "image_grid_u8: unknown dtype %d", dtype);
  if (mode != GCT2_U8_SUMMARY && mode != GCT2_U8_DATASET && mode != GCT2_U8_UNIT) return gct2_fail(GCT2_EINVAL, "image_grid_u8: unknown mode %d", mode);
  if (n <= 0 || H <= 0 || W <= 0 || cols <= 0 || rows <= 0)
    return gct2_fail(GCT2_EINVAL, "image_grid_u8: n=%d H=%d W=%d cols=%d rows=%d must be positive", n, H, W, cols, rows);
  if ((long long)cols * rows < n) return gct2_fail(GCT2_EINVAL, "image_grid_u8: cols=%d x rows=%d cells do not hold n=%d images", cols, rows, n);
  if (scale < 1 || scale > 16) return gct2_fail(GCT2_EINVAL, "image_grid_u8: scale=%d is outside 1..16", scale);
  if (pad < 0 || pad > 64) return gct2_fail(GCT2_EINVAL, "image_grid_u8: pad=%d is outside 0..64", pad);
  if (H > 16384 || W > 16384) return gct2_fail(GCT2_EINVAL, "image_grid_u8: H=%d W=%d is larger than 16384", H, W);
  if (fill_rgb >> 24) return gct2_fail(GCT2_EINVAL, "image_grid_u8: fill_rgb=0x%08x has bits above its 24", fill_rgb);
  return img_grid_u8(src, dtype, n, H, W, mode, cols, rows, pad, scale, fill_rgb, out, S(stream));
}

int gct2_mse_fwd_bwd(const float* pred, const float* target, float* dpred, float* loss, float* partials, size_t n,
                     const float* loss_scale_ptr, void* stream) {
  if (!pred || !target || !dpred || !loss || !partials || n == 0) return gct2_fail(GCT2_EINVAL, "mse_fwd_bwd: null pointer or n == 0");
  return pw_mse(pred, target, dpred, loss, partials, n, loss_scale_ptr, S(stream));
}

// shape rules of a loss kind (shared by gct2_loss_scratch and gct2_loss_fwd_bwd)
static int check_loss_shape(const char* fn, int kind, int B, int H, int W, int C) {
  if (kind < GCT2_LOSS_MSE || kind > GCT2_LOSS_DCT) return gct2_fail(GCT2_EINVAL, "%s: unknown loss kind %d", fn, kind);
  if (B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4) return gct2_fail(GCT2_EINVAL, "%s: B=%d H=%d W=%d must be positive, C=%d in 1..4", fn, B, H, W, C);
  if (kind == GCT2_LOSS_MSE_POOLED && ((H & 15) || (W & 15)))
    return gct2_fail(GCT2_EINVAL, "%s: H=%d W=%d must be multiples of 16 (avg_pool2d(16, 16, 'SAME') without padding)", fn, H, W);
  if (kind == GCT2_LOSS_MSE_POOLED && (size_t)B * (H / 16) * (W / 16) > ((size_t)1 << 28))
    return gct2_fail(GCT2_EINVAL, "%s: too many 16 x 16 cells", fn);
  if (kind == GCT2_LOSS_DCT && (H != W || (H & 3))) return gct2_fail(GCT2_EINVAL, "%s: the DCT loss needs H == W == size, a multiple of 4 (H=%d W=%d)", fn, H, W);
  if (kind == GCT2_LOSS_DCT && ((size_t)H * W * C >= ((size_t)1 << 31) || (size_t)B * ((H + 127) / 128) * (((size_t)W * C + 127) / 128) > ((size_t)1 << 28)))
    return gct2_fail(GCT2_EINVAL, "%s: image too large for the DCT loss", fn);
  return GCT2_OK;
}

int gct2_loss_scratch(int kind, int B, int H, int W, int C, size_t* floats) {
  if (!floats) return gct2_fail(GCT2_EINVAL, "loss_scratch: null output pointer");
  if (int e = check_loss_shape("loss_scratch", kind, B, H, W, C)) return e;
  return loss_scratch_floats(kind, B, H, W, C, nullptr, floats);
}

int gct2_loss_fwd_bwd(int kind, const float* pred, const float* target, float* dpred, float* loss, float* scratch, size_t scratch_floats,
                      int B, int H, int W, int C, const float* basis, const float* loss_scale_ptr, void* stream) {
  if (int e = check_loss_shape("loss_fwd_bwd", kind, B, H, W, C)) return e;
  if (!pred || !target || !loss || !scratch) return gct2_fail(GCT2_EINVAL, "loss_fwd_bwd: null pointer");
  if (kind == GCT2_LOSS_DCT && !basis) return gct2_fail(GCT2_EINVAL, "loss_fwd_bwd: the DCT loss needs a basis");
  if (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)dpred | (uintptr_t)loss | (uintptr_t)loss_scale_ptr) % 4 || (uintptr_t)scratch % 16 ||
      (kind == GCT2_LOSS_DCT && (uintptr_t)basis % 16))
    return gct2_fail(GCT2_EINVAL, "loss_fwd_bwd: scratch and basis must be 16-byte aligned, the other pointers 4-byte aligned");
  size_t need = 0;
  loss_scratch_floats(kind, B, H, W, C, nullptr, &need);
  if (scratch_floats < need) return gct2_fail(GCT2_EINVAL, "loss_fwd_bwd: %zu floats of scratch, this kind and shape need %zu (gct2_loss_scratch)", scratch_floats, need);
  const size_t n = (size_t)B * H * W * C;
  switch (kind) {
    case GCT2_LOSS_MSE: return pw_mse(pred, target, dpred, loss, scratch, n, loss_scale_ptr, S(stream));
    case GCT2_LOSS_L1: return loss_l1(pred, target, dpred, loss, scratch, n, loss_scale_ptr, S(stream));
    case GCT2_LOSS_MSE_POOLED: return loss_pooled(pred, target, dpred, loss, scratch, B, H, W, C, loss_scale_ptr, S(stream));
    default: return loss_dct(pred, target, dpred, loss, scratch, B, H, C, basis, loss_scale_ptr, S(stream));
  }
}

// shape rules of the per-image losses: those of the kind, plus the limits of a (chunk, image) grid and of int element indices
static int check_eval_shape(const char* fn, int kind, int B, int H, int W, int C) {
  if (int e = check_loss_shape(fn, kind, B, H, W, C)) return e;
  if (B > 65535) return gct2_fail(GCT2_EINVAL, "%s: B=%d above 65535 (one grid row per image)", fn, B);
  if ((size_t)B * H * W * C >= ((size_t)1 << 31)) return gct2_fail(GCT2_EINVAL, "%s: B*H*W*C at or beyond 2^31", fn);
  return GCT2_OK;
}

int gct2_eval_loss_scratch(int kind, int B, int H, int W, int C, size_t* floats) {
  if (!floats) return gct2_fail(GCT2_EINVAL, "eval_loss_scratch: null output pointer");
  if (int e = check_eval_shape("eval_loss_scratch", kind, B, H, W, C)) return e;
  *floats = eval_scratch_floats(kind, B, H, W, C);
  return GCT2_OK;
}

int gct2_eval_loss_rows(int kind, const float* pred, const float* x, const float* eps, const float* a, const float* c, const float* w,
                        float* rows, float* scratch, size_t scratch_floats, int B, int H, int W, int C, const float* basis, void* stream) {
  if (int e = check_eval_shape("eval_loss_rows", kind, B, H, W, C)) return e;
  if (!pred || !x || !rows || !scratch) return gct2_fail(GCT2_EINVAL, "eval_loss_rows: null pointer");
  if (c && !eps) return gct2_fail(GCT2_EINVAL, "eval_loss_rows: c without eps");
  if (a && eps && !c) return gct2_fail(GCT2_EINVAL, "eval_loss_rows: a and eps without c");
  if (kind == GCT2_LOSS_DCT && !basis) return gct2_fail(GCT2_EINVAL, "eval_loss_rows: the DCT loss needs a basis");
  if (((uintptr_t)pred | (uintptr_t)x | (uintptr_t)eps | (uintptr_t)a | (uintptr_t)c | (uintptr_t)w | (uintptr_t)rows) % 4 ||
      (uintptr_t)scratch % 16 || (kind == GCT2_LOSS_DCT && (uintptr_t)basis % 16))
    return gct2_fail(GCT2_EINVAL, "eval_loss_rows: scratch and basis must be 16-byte aligned, the other pointers 4-byte aligned");
  const size_t need = eval_scratch_floats(kind, B, H, W, C);
  if (scratch_floats < need)
    return gct2_fail(GCT2_EINVAL, "eval_loss_rows: %zu floats of scratch, this kind and shape need %zu (gct2_eval_loss_scratch)", scratch_floats, need);
  return eval_loss_rows(kind, pred, x, eps, a, c, w, rows, scratch, B, H, W, C, basis, S(stream));
}

// shape rules of the weighted objective loss: MSE / L1 under the limits of the per-image losses
static int check_objective_shape(const char* fn, int kind, int B, int H, int W, int C) {
  if (kind != GCT2_LOSS_MSE && kind != GCT2_LOSS_L1) return gct2_fail(GCT2_EINVAL, "%s: loss kind %d (GCT2_LOSS_MSE or GCT2_LOSS_L1)", fn, kind);
  return check_eval_shape(fn, kind, B, H, W, C);
}

int gct2_objective_loss_scratch(int kind, int B, int H, int W, int C, size_t* floats) {
  if (!floats) return gct2_fail(GCT2_EINVAL, "objective_loss_scratch: null output pointer");
  if (int e = check_objective_shape("objective_loss_scratch", kind, B, H, W, C)) return e;
  *floats = objective_scratch_floats(B, H, W, C);
  return GCT2_OK;
}

int gct2_objective_loss_fwd_bwd(int kind, const float* pred, const float* x, const float* eps, const float* a, const float* c, const float* w,
                                const float* lam, float* dpred, float* loss, float* scratch, size_t scratch_floats, int B, int H, int W, int C,
                                const float* loss_scale_ptr, void* stream) {
  if (int e = check_objective_shape("objective_loss_fwd_bwd", kind, B, H, W, C)) return e;
  if (!pred || !x || !loss || !scratch) return gct2_fail(GCT2_EINVAL, "objective_loss_fwd_bwd: null pointer");
  if (c && !eps) return gct2_fail(GCT2_EINVAL, "objective_loss_fwd_bwd: c without eps");
  if (a && eps && !c) return gct2_fail(GCT2_EINVAL, "objective_loss_fwd_bwd: a and eps without c");
  if (dpred && (dpred == pred || dpred == x || dpred == eps)) return gct2_fail(GCT2_EINVAL, "objective_loss_fwd_bwd: dpred aliases an input");
  if (((uintptr_t)pred | (uintptr_t)x | (uintptr_t)eps | (uintptr_t)a | (uintptr_t)c | (uintptr_t)w | (uintptr_t)lam | (uintptr_t)dpred |
       (uintptr_t)loss | (uintptr_t)loss_scale_ptr) % 4 || (uintptr_t)scratch % 16)
    return gct2_fail(GCT2_EINVAL, "objective_loss_fwd_bwd: scratch must be 16-byte aligned, the other pointers 4-byte aligned");
  const size_t need = objective_scratch_floats(B, H, W, C);
  if (scratch_floats < need)
    return gct2_fail(GCT2_EINVAL, "objective_loss_fwd_bwd: %zu floats of scratch, this shape needs %zu (gct2_objective_loss_scratch)", scratch_floats, need);
  return objective_loss(kind, pred, x, eps, a, c, w, lam, dpred, loss, scratch, B, H, W, C, loss_scale_ptr, S(stream));
}

// shape rules of the image metrics: the limits of a (tile, image) grid and of int element indices
static int check_metrics_shape(const char* fn, int B, int H, int W, int C, int K) {
  if (B <= 0 || H <= 0 || W <= 0) return gct2_fail(GCT2_EINVAL, "%s: non-positive dims B=%d H=%d W=%d", fn, B, H, W);
  if (C < 1 || C > 4) return gct2_fail(GCT2_EINVAL, "%s: C=%d outside 1..4", fn, C);
  if (K < 1 || K > 16) return gct2_fail(GCT2_EINVAL, "%s: K=%d outside 1..16", fn, K);
  return GCT2_OK;
}
static int check_metrics_size(const char* fn, int B, int H, int W, int C) {
  if (B > 65535) return gct2_fail(GCT2_EINVAL, "%s: B=%d above 65535 (one grid row per image)", fn, B);
  if ((size_t)B * H * W * C >= ((size_t)1 << 31)) return gct2_fail(GCT2_EINVAL, "%s: B*H*W*C at or beyond 2^31", fn);
  return GCT2_OK;
}

int gct2_image_metrics_scratch(int B, int H, int W, int C, int K, size_t* floats) {
  if (!floats) return gct2_fail(GCT2_EINVAL, "image_metrics_scratch: null output pointer");
  if (int e = check_metrics_shape("image_metrics_scratch", B, H, W, C, K)) return e;
  if (int e = check_metrics_size("image_metrics_scratch", B, H, W, C)) return e;
  *floats = image_metrics_scratch_floats(B, H, W, C);
  return GCT2_OK;
}

int gct2_image_metrics(const float* pred, const float* noised, const float* u, const float* v, const float* x, const float* window, int K,
                       float max_val, float k1, float k2, float* mse, float* psnr, float* ssim, float* scratch, size_t scratch_floats, int B,
                       int H, int W, int C, void* stream) {
  if (!pred || !x || !mse || !scratch) return gct2_fail(GCT2_EINVAL, "image_metrics: null pointer");
  if (u && (!noised || !v)) return gct2_fail(GCT2_EINVAL, "image_metrics: u without noised or v");
  if (!u && (noised || v)) return gct2_fail(GCT2_EINVAL, "image_metrics: noised or v without u");
  if (ssim && !window) return gct2_fail(GCT2_EINVAL, "image_metrics: ssim without window");
  if (int e = check_metrics_shape("image_metrics", B, H, W, C, K)) return e;
  if (ssim && (H < K || W < K)) return gct2_fail(GCT2_EINVAL, "image_metrics: a %d x %d image is smaller than the %d x %d window", H, W, K, K);
  if (!std::isfinite(max_val) || !(max_val > 0.f)) return gct2_fail(GCT2_EINVAL, "image_metrics: max_val must be finite and > 0");
  if (!std::isfinite(k1) || !std::isfinite(k2) || k1 < 0.f || k2 < 0.f) return gct2_fail(GCT2_EINVAL, "image_metrics: k1 and k2 must be finite and >= 0");
  if (((uintptr_t)pred | (uintptr_t)noised | (uintptr_t)u | (uintptr_t)v | (uintptr_t)x | (uintptr_t)window | (uintptr_t)mse | (uintptr_t)psnr |
       (uintptr_t)ssim) % 4 || (uintptr_t)scratch % 16)
    return gct2_fail(GCT2_EINVAL, "image_metrics: scratch must be 16-byte aligned, the other pointers 4-byte aligned");
  if (int e = check_metrics_size("image_metrics", B, H, W, C)) return e;
  const size_t need = image_metrics_scratch_floats(B, H, W, C);
  if (scratch_floats < need)
    return gct2_fail(GCT2_EINVAL, "image_metrics: %zu floats of scratch, this shape needs %zu (gct2_image_metrics_scratch)", scratch_floats, need);
  return image_metrics(pred, noised, u, v, x, window, K, max_val, k1, k2, mse, psnr, ssim, scratch, B, H, W, C, S(stream));
}

int gct2_adam_keras_multi(float* p, float* m, float* v, float* g, void* shadow, int shadow_dtype, size_t n, float alpha, float beta1,
                          float beta2, float eps, float grad_mul, const gct2_loss_scale_state* ls, int zero_grad, void* stream) {
  if (!p || !m || !v || !g) return gct2_fail(GCT2_EINVAL, "adam_keras_multi: null pointer");
  if (shadow && !dtype_ok(shadow_dtype)) return gct2_fail(GCT2_EINVAL, "adam_keras_multi: bad shadow dtype");
  if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g) % 16 || (shadow && (uintptr_t)shadow % 8))
    return gct2_fail(GCT2_EINVAL, "adam_keras_multi: arenas must be 16-byte aligned");
  return pw_adam(p, m, v, g, shadow, shadow_dtype, n, alpha, beta1, beta2, eps, grad_mul, ls, zero_grad, S(stream));
}

int gct2_adam_apply(const gct2_adam_args* a, float* dw, size_t nw, void* stream) {
  if (!a || !dw) return gct2_fail(GCT2_EINVAL, "adam_apply: null pointer");
  if (int e = check_adam_args(a, dw, nw)) return e;
  if (a->nslab < 0 || (a->nslab > 0 && (!a->slab_base || a->slab_stride < nw))) return gct2_fail(GCT2_EINVAL, "adam_apply: bad slab description");
  return run_adam(a, dw, nw, WgradSlabs{a->slab_base, a->nslab, a->slab_stride}, stream);
}

int gct2_cast_from_f32(int dtype, const float* src, void* dst, size_t n, void* stream) {
  if (!dtype_ok(dtype) || !src || !dst) return gct2_fail(GCT2_EINVAL, "cast_from_f32: bad dtype or null pointer");
  return pw_cast(dtype, src, dst, n, S(stream));
}

int gct2_ema_update(float* ema, const float* p, void* ema_shadow, int shadow_dtype, size_t n, float momentum, float one_minus,
                    const gct2_loss_scale_state* ls, void* stream) {
  if (!ema || !p) return gct2_fail(GCT2_EINVAL, "ema_update: null pointer");
  if (n == 0) return gct2_fail(GCT2_EINVAL, "ema_update: n == 0");
  if (ema_shadow && shadow_dtype != GCT2_BF16 && shadow_dtype != GCT2_F16)
    return gct2_fail(GCT2_EINVAL, "ema_update: a shadow needs a 16-bit dtype (GCT2_BF16 / GCT2_F16), got %d", shadow_dtype);
  if (((uintptr_t)ema | (uintptr_t)p) % 16 || (ema_shadow && (uintptr_t)ema_shadow % 8))
    return gct2_fail(GCT2_EINVAL, "ema_update: ema and p must be 16-byte aligned, the shadow 8-byte aligned");
  if (!(momentum >= 0.f && momentum <= 1.f)) return gct2_fail(GCT2_EINVAL, "ema_update: momentum %g outside [0, 1]", (double)momentum);
  return pw_ema(ema, p, ema_shadow, shadow_dtype, n, momentum, one_minus, ls, S(stream));
}

int gct2_sumsq_layout(const uint64_t* begin, const uint64_t* count, int nseg, gct2_sumsq_seg* out, size_t* npartials) {
  if (!begin || !count || !out || !npartials) return gct2_fail(GCT2_EINVAL, "sumsq_layout: null pointer");
  if (nseg < 1 || nseg > GCT2_SUMSQ_MAX_SEGMENTS)
    return gct2_fail(GCT2_EINVAL, "sumsq_layout: nseg = %d outside [1, %d]", nseg, GCT2_SUMSQ_MAX_SEGMENTS);
  uint64_t total = 0;
  for (int s = 0; s < nseg; s++) {                 // everything is checked before anything is filled
    if (count[s] == 0) return gct2_fail(GCT2_EINVAL, "sumsq_layout: segment %d is empty", s);
    if (begin[s] % 4) return gct2_fail(GCT2_EINVAL, "sumsq_layout: segment %d begins at %llu, not a multiple of 4 elements", s, (unsigned long long)begin[s]);
    if (begin[s] + count[s] < begin[s]) return gct2_fail(GCT2_EINVAL, "sumsq_layout: segment %d wraps around", s);
    if (s && begin[s] < begin[s - 1]) return gct2_fail(GCT2_EINVAL, "sumsq_layout: segment %d begins before segment %d (ascending order)", s, s - 1);
    if (s && begin[s] < begin[s - 1] + count[s - 1]) return gct2_fail(GCT2_EINVAL, "sumsq_layout: segments %d and %d overlap", s - 1, s);
    total += (count[s] + GCT2_SUMSQ_CHUNK - 1) / GCT2_SUMSQ_CHUNK;
  }
  if (total > 0x7fffffffull) return gct2_fail(GCT2_EINVAL, "sumsq_layout: %llu partials are more than one launch covers", (unsigned long long)total);
  uint64_t first = 0;
  for (int s = 0; s < nseg; s++) {
    out[s].begin = begin[s]; out[s].count = count[s]; out[s].first_partial = first;
    first += (count[s] + GCT2_SUMSQ_CHUNK - 1) / GCT2_SUMSQ_CHUNK;
  }
  *npartials = (size_t)first;
  return GCT2_OK;
}

int gct2_grad_sumsq(const float* g, const gct2_sumsq_seg* segs, int nseg, size_t npartials, float grad_mul, gct2_loss_scale_state* ls,
                    double* partials, double* sumsq, void* stream) {
  if (!g || !segs || !partials || !sumsq) return gct2_fail(GCT2_EINVAL, "grad_sumsq: null pointer");
  if (nseg < 1 || nseg > GCT2_SUMSQ_MAX_SEGMENTS)
    return gct2_fail(GCT2_EINVAL, "grad_sumsq: nseg = %d outside [1, %d]", nseg, GCT2_SUMSQ_MAX_SEGMENTS);
  if (npartials == 0 || npartials < (size_t)nseg || npartials > 0x7fffffffull)
    return gct2_fail(GCT2_EINVAL, "grad_sumsq: npartials = %zu is not what gct2_sumsq_layout reports for %d segments", npartials, nseg);
  if ((uintptr_t)g % 16 || ((uintptr_t)segs | (uintptr_t)partials | (uintptr_t)sumsq) % 8)
    return gct2_fail(GCT2_EINVAL, "grad_sumsq: g must be 16-byte aligned, segs / partials / sumsq 8-byte aligned");
  return pw_grad_sumsq(g, segs, nseg, npartials, grad_mul, ls, partials, sumsq, S(stream));
}

// the three entry points of the non-fused update share one list of rejections and one launcher; what differs between them is named here:
// whether the caller chooses the kind and may choose Adam, the kernels launched (reg), and three pieces of error text
struct UpdateEntry {
  const char* name;
  bool reg, adam;
  const char* kinds;              // what the unknown-kind message lists
  const char* aligned16;          // how the alignment message names the fp32 arenas
  const char* sumsq_from;         // where the sumsq message says the sums come from
};
static const UpdateEntry ADAM_KERAS_CLIPPED = {"adam_keras_clipped", false, true, "", "p, m, v and g", "gct2_grad_sumsq"};
static const UpdateEntry OPTIMIZER_APPLY = {"optimizer_apply", false, false, "GCT2_OPT_SGD / GCT2_OPT_RMSPROP; Adam is gct2_adam_keras_clipped",
                                            "p, g and the slots in use", "gct2_grad_sumsq"};
static const UpdateEntry OPTIMIZER_APPLY_REG = {"optimizer_apply_reg", true, true, "GCT2_OPT_ADAM / GCT2_OPT_SGD / GCT2_OPT_RMSPROP",
                                                "p, g and the slots in use", "gct2_grad_sumsq / gct2_grad_sumsq_l2"};

// Adam: momentum = beta1, rho = beta2, unchecked.  An entry point without a transformer or a regularizer passes GCT2_GRAD_NONE and 0
static int run_update(const UpdateEntry& e, int kind, float* p, float* m, float* v, float* g, void* shadow, int shadow_dtype, size_t n, float lr,
                      float momentum, int nesterov, float rho, float epsilon, float grad_mul, const gct2_loss_scale_state* ls, int clip_mode,
                      float clip, const double* sumsq, float l2_coeff, int transform, void* stream) {
  const bool adam = kind == GCT2_OPT_ADAM;
  if (!(adam && e.adam) && kind != GCT2_OPT_SGD && kind != GCT2_OPT_RMSPROP)
    return gct2_fail(GCT2_EINVAL, "%s: unknown kind %d (%s)", e.name, kind, e.kinds);
  if (!adam && !(momentum >= 0.f && momentum <= 1.f)) return gct2_fail(GCT2_EINVAL, "%s: momentum %g outside [0, 1]", e.name, (double)momentum);
  if (kind == GCT2_OPT_RMSPROP && !(rho >= 0.f && rho <= 1.f)) return gct2_fail(GCT2_EINVAL, "%s: rho %g outside [0, 1]", e.name, (double)rho);
  if (kind == GCT2_OPT_RMSPROP && !(epsilon >= 0.f)) return gct2_fail(GCT2_EINVAL, "%s: epsilon %g < 0", e.name, (double)epsilon);
  const bool use_m = adam || momentum > 0.f, use_v = kind != GCT2_OPT_SGD;
  if (!p || !g || (use_m && !m) || (use_v && !v)) return gct2_fail(GCT2_EINVAL, "%s: null pointer", e.name);
  if (n == 0) return gct2_fail(GCT2_EINVAL, "%s: n == 0", e.name);
  if (shadow && shadow_dtype != GCT2_BF16 && shadow_dtype != GCT2_F16)
    return gct2_fail(GCT2_EINVAL, "%s: a shadow needs a 16-bit dtype (GCT2_BF16 / GCT2_F16), got %d", e.name, shadow_dtype);
  if (((uintptr_t)p | (uintptr_t)g | (use_m ? (uintptr_t)m : 0) | (use_v ? (uintptr_t)v : 0)) % 16 || (shadow && (uintptr_t)shadow % 8) ||
      (uintptr_t)sumsq % 8)
    return gct2_fail(GCT2_EINVAL, "%s: %s must be 16-byte aligned, the shadow and sumsq 8-byte aligned", e.name, e.aligned16);
  if (clip_mode < GCT2_CLIP_NONE || clip_mode > GCT2_CLIP_GLOBAL_NORM) return gct2_fail(GCT2_EINVAL, "%s: unknown clip_mode %d", e.name, clip_mode);
  if (clip_mode != GCT2_CLIP_NONE && !(clip > 0.f && clip <= 3.402823466e38f))
    return gct2_fail(GCT2_EINVAL, "%s: clip = %g must be finite and > 0", e.name, (double)clip);
  if ((clip_mode == GCT2_CLIP_NORM || clip_mode == GCT2_CLIP_GLOBAL_NORM) && !sumsq)
    return gct2_fail(GCT2_EINVAL, "%s: clip_mode %d needs sumsq (%s)", e.name, clip_mode, e.sumsq_from);
  if (transform != GCT2_GRAD_NONE && transform != GCT2_GRAD_SIGN) return gct2_fail(GCT2_EINVAL, "%s: unknown transform %d", e.name, transform);
  if (!(l2_coeff >= 0.f && l2_coeff <= 3.402823466e38f))
    return gct2_fail(GCT2_EINVAL, "%s: l2_coeff = %g must be finite and >= 0", e.name, (double)l2_coeff);
  return pw_update(e.name, e.reg, kind, p, m, v, g, shadow, shadow_dtype, n, lr, momentum, nesterov, rho, epsilon, grad_mul, ls, clip_mode, clip,
                   sumsq, l2_coeff, transform, S(stream));
}

int gct2_adam_keras_clipped(float* p, float* m, float* v, float* g, void* shadow, int shadow_dtype, size_t n, float alpha, float beta1,
                            float beta2, float eps, float grad_mul, const gct2_loss_scale_state* ls, int clip_mode, float clip,
                            const double* sumsq, void* stream) {
  return run_update(ADAM_KERAS_CLIPPED, GCT2_OPT_ADAM, p, m, v, g, shadow, shadow_dtype, n, alpha, beta1, 0, beta2, eps, grad_mul, ls, clip_mode,
                    clip, sumsq, 0.f, GCT2_GRAD_NONE, stream);
}

int gct2_optimizer_apply(int kind, float* p, float* m, float* v, float* g, void* shadow, int shadow_dtype, size_t n, float lr, float momentum,
                         int nesterov, float rho, float epsilon, float grad_mul, const gct2_loss_scale_state* ls, int clip_mode, float clip,
                         const double* sumsq, void* stream) {
  return run_update(OPTIMIZER_APPLY, kind, p, m, v, g, shadow, shadow_dtype, n, lr, momentum, nesterov, rho, epsilon, grad_mul, ls, clip_mode,
                    clip, sumsq, 0.f, GCT2_GRAD_NONE, stream);
}

int gct2_optimizer_apply_reg(int kind, float* p, float* m, float* v, float* g, void* shadow, int shadow_dtype, size_t n, float lr, float momentum,
                             int nesterov, float rho, float epsilon, float grad_mul, const gct2_loss_scale_state* ls, int clip_mode, float clip,
                             const double* sumsq, float l2_coeff, int transform, void* stream) {
  return run_update(OPTIMIZER_APPLY_REG, kind, p, m, v, g, shadow, shadow_dtype, n, lr, momentum, nesterov, rho, epsilon, grad_mul, ls, clip_mode,
                    clip, sumsq, l2_coeff, transform, stream);
}

int gct2_grad_sumsq_l2(const float* g, const float* p, const gct2_sumsq_seg* segs, const float* seg_coeff, int nseg, size_t npartials,
                       float grad_mul, gct2_loss_scale_state* ls, double* partials, double* sumsq, void* stream) {
  if (!g || !p || !segs || !seg_coeff || !partials || !sumsq) return gct2_fail(GCT2_EINVAL, "grad_sumsq_l2: null pointer");
  if (nseg < 1 || nseg > GCT2_SUMSQ_MAX_SEGMENTS)
    return gct2_fail(GCT2_EINVAL, "grad_sumsq_l2: nseg = %d outside [1, %d]", nseg, GCT2_SUMSQ_MAX_SEGMENTS);
  if (npartials == 0 || npartials < (size_t)nseg || npartials > 0x7fffffffull)
    return gct2_fail(GCT2_EINVAL, "grad_sumsq_l2: npartials = %zu is not what gct2_sumsq_layout reports for %d segments", npartials, nseg);
  if (((uintptr_t)g | (uintptr_t)p) % 16 || ((uintptr_t)segs | (uintptr_t)partials | (uintptr_t)sumsq) % 8 || (uintptr_t)seg_coeff % 4)
    return gct2_fail(GCT2_EINVAL, "grad_sumsq_l2: g and p must be 16-byte aligned, segs / partials / sumsq 8-byte, seg_coeff 4-byte aligned");
  return pw_grad_sumsq_l2(g, p, segs, seg_coeff, nseg, npartials, grad_mul, ls, partials, sumsq, S(stream));
}

int gct2_l2_penalty(const float* loss, const double* S_, float l2, float* penalty_out, float* total_out, void* stream) {
  if (!loss || !S_ || !penalty_out || !total_out) return gct2_fail(GCT2_EINVAL, "l2_penalty: null pointer");
  if ((uintptr_t)S_ % 8 || ((uintptr_t)loss | (uintptr_t)penalty_out | (uintptr_t)total_out) % 4)
    return gct2_fail(GCT2_EINVAL, "l2_penalty: S must be 8-byte aligned, loss / penalty_out / total_out 4-byte aligned");
  if (!(l2 >= 0.f && l2 <= 3.402823466e38f)) return gct2_fail(GCT2_EINVAL, "l2_penalty: l2 = %g must be finite and >= 0", (double)l2);
  return pw_l2_penalty(loss, S_, l2, penalty_out, total_out, S(stream));
}

int gct2_loss_scale_init(gct2_loss_scale_state* st, float initial_scale, void* stream) {
  if (!st || !(initial_scale > 0.f)) return gct2_fail(GCT2_EINVAL, "loss_scale_init: null state or non-positive scale");
  return pw_ls_init(st, initial_scale, S(stream));
}
int gct2_loss_scale_begin(gct2_loss_scale_state* st, float base_lr, int warmup_steps, float beta1, float beta2, void* stream) {
  if (!st || warmup_steps < 0) return gct2_fail(GCT2_EINVAL, "loss_scale_begin: null state or negative warm-up");
  return pw_ls_begin(st, base_lr, warmup_steps, beta1, beta2, S(stream));
}
int gct2_loss_scale_begin_schedule(gct2_loss_scale_state* st, int schedule, float initial, float steps, float decay_rate, int staircase,
                                   int bias_correction, float beta1, float beta2, void* stream) {
  if (!st) return gct2_fail(GCT2_EINVAL, "loss_scale_begin_schedule: null state");
  if (schedule == GCT2_SCHEDULE_WARMUP) {
    if (!(steps >= 0.f && steps <= 16777216.f) || steps != (float)(int)steps)
      return gct2_fail(GCT2_EINVAL, "loss_scale_begin_schedule: warm-up steps %g must be a whole number in [0, 2^24]", (double)steps);
  } else if (schedule == GCT2_SCHEDULE_INVERSE_TIME_DECAY) {
    if (!(steps > 0.f)) return gct2_fail(GCT2_EINVAL, "loss_scale_begin_schedule: decay_steps %g must be > 0", (double)steps);
  } else {
    return gct2_fail(GCT2_EINVAL, "loss_scale_begin_schedule: unknown schedule %d", schedule);
  }
  return pw_ls_begin_schedule(st, schedule, initial, steps, decay_rate, staircase, bias_correction, beta1, beta2, S(stream));
}
int gct2_scale_check_finite(const float* g, size_t n, gct2_loss_scale_state* st, void* stream) {
  if (!g || !st) return gct2_fail(GCT2_EINVAL, "scale_check_finite: null pointer");
  return pw_ls_check(g, n, st, S(stream));
}
int gct2_loss_scale_update(gct2_loss_scale_state* st, int growth_interval, void* stream) {
  if (!st || growth_interval <= 0) return gct2_fail(GCT2_EINVAL, "loss_scale_update: null state or bad interval");
  return pw_ls_update(st, growth_interval, S(stream));
}

}  // extern "C"
