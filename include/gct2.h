/*
 * gct2.h - C ABI of the MI355X (gfx950) train-step kernels for relgukxilef/GAN-Class-Transfer2.
 *
 * The reference (/root/reference/train.py) has no native code and no FFI: every device op is a
 * TensorFlow/Keras call.  Each entry point below replaces one such call site (cited per function,
 * file:line into /root/reference/train.py) and is what a ctypes / cffi binding of the reference's
 * Python host code would bind.
 *
 * Conventions
 *  - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise.
 *  - activations are NHWC "views": pointer to channel 0 of pixel 0 + `ld` = distance between
 *    consecutive pixels in ELEMENTS (>= channels; lets a tensor live inside a channel slice of a
 *    wider concat buffer, which is how train.py:114-119's tf.concat becomes zero-copy).
 *  - `dtype` selects the storage/operand type of activations, activation gradients and the
 *    weight operand: GCT2_F32 (reference default, train.py:34,38), GCT2_BF16, GCT2_F16
 *    (train.py:43-45 mixed_float16).  Accumulation, biases, weight gradients, Adam state: fp32.
 *  - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *    No allocation, no host synchronisation, no ownership transfer; re-entrant across streams.
 *  - return value: GCT2_OK or an error code; nothing is launched when arguments are rejected.
 *  - operand sizes ("Operand size limits"; tests/test_large_views_gpu.py): the layer entry points bound the PIXEL count
 *    (B*H*W*4 < 2^31 on the larger grid, GCT2_EINVAL beyond); `ld` is any int >= the channel count, so a view may span many GiB.
 *    Every kernel forms the addresses of its views in 64 bits, except the loads of the 16-bit matrix-core kernels (2-GiB buffer
 *    descriptors, 31-bit lane offsets).  With Hs x Ws the smaller of a layer's two grids, a 16-bit call runs on the matrix cores only while
 *      forward / input gradient: 4*B*Hs*Ws*ld*2 + (8*Ws + 4)*ld*2 + 2*K < 0x7ff00000  (ld, K: stride and channels of the tensor the
 *                                call reads: x, or dz) and the kernel's 16*Cin*Cout*2 bytes likewise;
 *      weight gradient:          4*B*Hs*Ws*ld*2 < 0x7ff00000 for the tensor on the larger grid (stride-1: B*H*W*ld*2) and
 *                                B*Hs*Ws*ld*2 < 0x7ff00000 for the other one;
 *    beyond that it runs on the direct kernels - same results, slower, never an error.  gct2_convT4s2_fwd_head_train, which has no
 *    direct form, returns GCT2_EINVAL past its own bound (stated there).  Output, mask (act), bit-plane and fp32 views have no limit
 *    beyond the pixel count.  The pointwise entry points take size_t pixel counts, or int M / B*HW that they check against 2^31 where
 *    they index with int; gct2_dense_head_train bounds ldx by its LDS tile (its message names it).
 *  - alignment ("Alignment classes"; tests/test_alignment_exact_gpu.py): the layer entry points (gct2_conv4s2_*,
 *    gct2_convT4s2_fwd / _dgrad / _wgrad, gct2_conv2d_s1_*) take ANY element-aligned view and array: x, dz, act, y, dx at multiples of
 *    the element size with any ld >= the channel count, w likewise, bias / dw / db at multiples of 4 bytes.  Alignment selects the
 *    kernel and never the result: 16-byte aligned views whose ld is a multiple of 8 elements run the 16-byte paths (what the engine
 *    passes); an output or mask view that is only 8-byte aligned (or whose ld is 8 k + 4) runs the tap GEMM's 8-byte epilogue
 *    (launch-log token ":e8") and keeps the halo kernel out; anything less aligned on x, dz, w, bias, y, dx, act, dw runs the direct
 *    kernels; the image layer (Cin <= 4) reads a source that is not a whole number of 8-byte pixels channel by channel; the fp32
 *    matrix-core kernels stage a misaligned operand element by element; a dw that is not 16-byte aligned gets atomics or one owner
 *    instead of ordered slabs.  On exact-sum inputs (tests/exact_cases.py) every one of these paths stores the same bits; on
 *    other inputs they differ by the order of the fp32 additions only.  GCT2_EINVAL for alignment only where an entry point says so
 *    (scratch, bias-queue and optimizer arenas, gct2_convT4s2_fwd_head_train, the adam range of the weight-gradient calls).
 */
#ifndef GCT2_H
#define GCT2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { GCT2_F32 = 0, GCT2_BF16 = 1, GCT2_F16 = 2 };
enum {
  GCT2_OK = 0,
  GCT2_EINVAL = 1,   /* bad shape / stride / alignment / dtype */
  GCT2_ELAUNCH = 2,  /* HIP launch error (hipGetLastError != success) */
  GCT2_ENODEV = 3    /* no gfx950 device visible */
};

/* library / device identification ------------------------------------------------------------ */
int gct2_abi_version(void);                 /* bumps when a signature below changes (v13: ReLU bit planes; v14: pruned tuning word, launch log, no deferred row sums; v15: launch-log read reports the size it needs, step plans; v16: bias queue; v17: plan event kinds - system-scope and timed records, gct2_plan_elapsed; v17 + gct2_ema_update (additive); v17 + gct2_sumsq_layout, gct2_grad_sumsq, gct2_adam_keras_clipped (additive); v17 + gct2_optimizer_apply, gct2_loss_scale_begin_schedule (additive); v17 + gct2_loss_scratch, gct2_loss_fwd_bwd (additive); v17 + gct2_optimizer_apply_reg, gct2_grad_sumsq_l2, gct2_l2_penalty (additive); v17 + gct2_dense_steps_fwd, gct2_dense_steps_bwd, gct2_dense_steps_scratch (additive); v17 + gct2_dense2_fwd, gct2_dense2_bwd, gct2_dense2_scratch (additive); v17 + gct2_noise_image_table, gct2_noise_image_rng_table (additive); v17 + gct2_eval_loss_scratch, gct2_eval_loss_rows (additive)) */
/* how the library was built: 0 for the product build; bit 0 (GCT2_BUILD_STAMP) = diagnostic build with in-kernel phase stamps
 * (make EXTRA=-DGCT2_STAMP).  Product hosts (the Python binding, bench.py, the tests) refuse a library whose flags are not 0. */
enum { GCT2_BUILD_STAMP = 1 };
int gct2_build_flags(void);
const char* gct2_last_error(void);          /* host string describing the last non-OK return */
int gct2_device_check(void);                /* GCT2_OK iff the current device is gfx950 */
/* ABI v17, host plumbing: `workgroups` 256-thread work-groups that do nothing but hold their slots on `stream` for `microseconds`
 * (every wave spins on the constant 100-MHz s_memrealtime counter and leaves by itself; at most 20 ms).  Two users: the host mirror
 * finds out which of its streams the runtime put on ONE hardware queue (a short occupy on stream A, a marker behind a trivial one on
 * stream B: B finishing only after A means they share a queue and would block each other for the whole run - engine.py
 * `distinct_stream`), and scripts/bench_dp_overhead.py stands a collective's wire time in for a collective on a one-GPU box. */
int gct2_stream_occupy(void* stream, int workgroups, double microseconds);
/* ---- call context: caller-owned scratch + tuning, one per engine / host thread ------------------------------------------
 * The library keeps NO process-wide mutable state (ABI v11).  A gct2_ctx is a small host object created by the caller; it
 * carries (a) the caller's device scratch for split reductions / partial rows and (b) the tile-selection knobs.  A ctx is used by
 * ONE host thread at a time (the layer entry points write its one-shot ReLU plane and its launch log).  Calls that
 * share one ctx must be enqueued on ONE stream at a time per scratch area (forward / input-gradient / head calls use the
 * main workspace, *_wgrad calls the weight-gradient workspace when one is set); calls with DIFFERENT ctx objects (two
 * engines, two host threads, two streams) are fully independent.  ctx = NULL is allowed everywhere: no scratch (split-K and
 * partial-row reductions are off: same results, slower small layers, fp32 atomics for the bias sums), automatic tiles. */
typedef struct gct2_ctx gct2_ctx;
int gct2_ctx_create(gct2_ctx** ctx);
int gct2_ctx_destroy(gct2_ctx* ctx);
/* device scratch (16-byte aligned) for the split-K partial sums of layers whose output is too small to fill the chip (the
 * U-Net's bottleneck levels), the partial rows of the fused bias gradients and the Dense head.  ws = NULL removes it. */
int gct2_ctx_set_workspace(gct2_ctx* ctx, void* ws, size_t bytes);
/* optional second scratch used by the weight-gradient entry points only (their partial-tile slabs): with it *_wgrad calls
 * may run on a second stream concurrently with the forward/dgrad calls of the same ctx (the engine's reverse pass does). */
int gct2_ctx_set_wgrad_workspace(gct2_ctx* ctx, void* ws, size_t bytes);
/* Bias queue (ABI v16).  The input-gradient entry points fuse the bias gradient of the tensor they write into their epilogue and leave
 * partial rows that ONE small launch per call sums in a fixed order.  Eleven such launches sit between the input-gradient launches of a
 * reverse pass; with a queue buffer registered (16-byte aligned device memory; a few MB: rows x channels x 4 bytes per call) the calls of
 * this ctx leave their partial rows in the buffer and record the row set instead, and gct2_bias_queue_flush sums every recorded set -
 * same geometry, same order of additions, same "first writer overwrites, second adds" as the immediate launches, hence the same bits -
 * in two launches on `stream`.  All calls that fill one queue and its flush must be enqueued on ONE stream; a call whose rows do not fit
 * (or a 17th row set) first flushes what is queued and then reduces its own rows at once; buf = NULL returns to the immediate form and
 * drops row sets that were recorded and not flushed.  Program order per target is kept whoever writes it (v17): a call that writes a
 * bias gradient AT ONCE - direct kernels, an atomics epilogue taken for lack of row space, the db of a weight-gradient call - first
 * flushes the queue if a queued row set names the same target, and of the combinations that can meet in the queue only "queued
 * overwrite, then ONE add" is recorded together; a second add, a second overwrite or an overwrite behind a queued add flush first. */
int gct2_ctx_set_bias_queue(gct2_ctx* ctx, void* buf, size_t bytes);
int gct2_bias_queue_flush(gct2_ctx* ctx, void* stream);
/* tuning: forces a tile / order instead of the automatic per-layer choice (same results for every value within the stated
 * tolerances; the parity tests and scripts/bench_layer.py use it).  Unknown words are rejected.
 * bits 0-7  : forward / input-gradient tile: 0 = automatic, 2 = 128x128 (two LDS buffers), 5 = 256x128 (one buffer, 8 waves);
 * bit 8     : the forward / input-gradient GEMMs never split their reduction over work-groups (parity tests at reduced batch: the
 *             kernels of the batch-64 dispatch then run the way they do at batch 64);
 * bits 16-23: weight-gradient tile: 0 = automatic, 2 = 256x256 five-stage ring, 4 / 5 = the same in the r03 / r04 stage order
 *             (bit-identity tests of the later orders), 3 = 128x128, 6 = 128x128 with the general address code (bit-identity test of the
 *             image-aligned form), 7 = 128x128 with fp32 atomics instead of ordered slabs (arrival-order
 *             dependent: comparison tests only);
 * bits 24-25: halo-tile kernel (Conv2DTranspose forward / Conv2D input gradient): 0 = automatic, 1 = never, 2 = wherever allowed;
 * bits 26-27: tile -> XCD order of the forward / input-gradient GEMMs: 0 = automatic, 1 = bands of output pixels per XCD,
 *             2 = weight slices per XCD;
 * bits 28-30: forced pixel split of the 128x128 weight-gradient tile: 0 = automatic, v = 1..7: 2^(v-1) splits. */
int gct2_ctx_set_tuning(gct2_ctx* ctx, int v);
/* test hook: non-zero routes every convolution of this ctx through the direct (non-MFMA) kernels */
int gct2_ctx_force_direct(gct2_ctx* ctx, int on);
/* fp32 arithmetic of every convolution entry point (dtype GCT2_F32: forward, input and weight gradients of the 4x4 / stride-2 layers
 * and of the stride-1 'same' convolutions gct2_conv2d_s1_*, every KS they accept: 1, 3, 5, 7) for the calls of this ctx:
 * GCT2_F32_MATH_DIRECT (the default) = one thread per output; GCT2_F32_MATH_MFMA = LDS tiles on the exact fp32-input matrix cores
 * (v_mfma_f32_16x16x4_f32).  An unsplit forward / input-gradient launch of the MFMA mode sums every output in the direct kernel's
 * order (taps, then ascending channels: the same fmaf chain); split reductions (split-K, weight-gradient pixel splits) add ordered
 * fp32 partial sums.  force_direct wins over this setting.  Any other mode, or a NULL ctx: GCT2_EINVAL. */
enum { GCT2_F32_MATH_DIRECT = 0, GCT2_F32_MATH_MFMA = 1 };
int gct2_ctx_set_f32_math(gct2_ctx* ctx, int mode);
/* ReLU bit plane for the NEXT layer call of this ctx (r03, ABI v13; one-shot: the call consumes and clears it).
 * bits: device bytes [pixels][ld_bytes], bit k of byte c <-> channel 8c + k of the call's output view.
 *  - before gct2_conv4s2_fwd / gct2_convT4s2_fwd: the call ALSO writes bits = (y > 0) for its Cout channels (in the epilogue of the
 *    16-byte-store kernels; derived from the stored y by one extra launch on the other paths) - beside y, which is unchanged;
 *  - before gct2_conv4s2_dgrad / gct2_convT4s2_dgrad with act != NULL: the call MAY read its ReLU mask from the plane instead of
 *    act (1 byte instead of 16 per 8 channels: the mask read is a third of the epilogue traffic of these calls).  The plane must
 *    equal (act > 0) over the Cin channels of the call - which of the two a given kernel reads is unspecified.
 * Channels must be a multiple of 8, ld_bytes >= channels / 8.  bits = NULL clears a pending plane.  EVERY layer entry point that
 * takes a ctx removes a pending plane first thing, whether it succeeds or not; the ones that cannot use a plane (weight gradients,
 * the head calls, the stride-1 convolutions) return GCT2_EINVAL when one was pending. */
int gct2_ctx_set_relu_bits(gct2_ctx* ctx, void* bits, int ld_bytes);
/* diagnostic builds only (gct2_build_flags() & GCT2_BUILD_STAMP): device buffer that receives the s_memrealtime phase stamps of
 * one wave per work-group of the next stamped launch of this ctx (layout: scripts/stamp_*.py).  GCT2_EINVAL in a product build. */
int gct2_ctx_set_stamp_buffer(gct2_ctx* ctx, void* stamps, size_t bytes);

/* launch log (tests / diagnostics): while switched on, every layer entry point of this ctx appends the kernel it selected as a
 * text token ("tap:conv:256x128:mask:ksplit=1:bits;", "halo:convT:bias_act;", "wgrad:256q:rsplit=8:slabs;", "rgb:fwd;",
 * "direct:tap;", "relu_bits:derived;" ...).  gct2_ctx_log_launches(ctx, on) clears the log and switches it; read copies the
 * NUL-terminated text and clears the log.  *needed (may be NULL) receives the bytes the text needs including the NUL; when the
 * buffer is smaller (or NULL) the call returns GCT2_EINVAL and NEITHER copies NOR clears anything (ABI v15; v14 truncated
 * silently).  The log stops growing at 1 MiB and then ends with "log:truncated;".  A parity test at reduced batch uses it to
 * prove that the kernels it forced are the ones that ran. */
int gct2_ctx_log_launches(gct2_ctx* ctx, int on);
int gct2_ctx_read_launch_log(gct2_ctx* ctx, char* buf, size_t bytes, size_t* needed);

/* ---- DownShuffle = Conv2D(f, 4, 2, 'same', relu)   train.py:158-169 ------------------------- */
/* y[b,oh,ow,o] = act(bias[o] + sum_{kh,kw,i} x[b,2oh+kh-1,2ow+kw-1,i] * w[kh,kw,i,o])
 * x: [B,H,W,Cin] view, H and W even;  w: Keras kernel (4,4,Cin,Cout) of `dtype`;
 * bias: fp32[Cout] or NULL;  y: [B,H/2,W/2,Cout] view;  relu != 0 applies max(.,0). */
int gct2_conv4s2_fwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w, const float* bias,
                     void* y, int ldy, int B, int H, int W, int Cin, int Cout, int relu,
                     void* stream);

/* input gradient of the above (autodiff of train.py:161-166 inside Keras fit, train.py:516):
 * dx[b,ih,iw,i] (+)= mask * sum_{kh,kw,o} dz[b,oh,ow,o] * w[kh,kw,i,o],  ih = 2oh+kh-1.
 * dz: [B,H/2,W/2,Cout] PRE-activation gradient;  dx: [B,H,W,Cin] view.
 * act (may be NULL): [B,H,W,Cin] view of the tensor whose ReLU produced x; mask = act > 0, so dx is
 * again a pre-activation gradient.  accumulate != 0: dx += result (skip branch of the concat,
 * train.py:114-119), else dx = result.
 * Fused bias gradients (optional): since dx is the gradient w.r.t. the PRE-activation of the layer(s) that produced
 * `act`, its column sums are those layers' bias gradients.  db (+)= sums of THIS call's masked result over channels
 * [0, db_split), db2 (+)= over channels [db_split, Cin) (a concat buffer spans two layers); NULL = not wanted.
 * db_accumulate: bit 0 set -> db is added to, clear -> db is overwritten; bit 1 the same for db2.  (The skip slice of a
 * concat buffer receives two gradient contributions, train.py:114-119: the first launch overwrites, the second adds, so the
 * caller never has to zero a bias gradient.) */
int gct2_conv4s2_dgrad(gct2_ctx* ctx, int dtype, const void* dz, int lddz, const void* w, const void* act,
                       int ldact, void* dx, int lddx, int B, int H, int W, int Cin, int Cout,
                       int accumulate, float* db, int db_split, float* db2, int db_accumulate, void* stream);

/* optional optimizer step fused behind a weight-gradient call (single-replica training without loss scaling): Keras Adam
 * (as gct2_adam_keras_multi) over a contiguous parameter range of the caller's arenas that STARTS with the layer's kernel,
 * enqueued on the same stream right after the gradient.  p, m, v: fp32, start of the kernel's slice; n: elements of the
 * whole range (>= the kernel's 16*Cin*Cout; the engine's ranges are the kernel plus alignment padding - its biases live in a
 * separate fp32 zone with a launch of its own); dw (the call's gradient pointer) must be the matching start of the gradient
 * arena.  The kernel gradient is consumed straight from the launch's partial sums where it has them (it is then never
 * written to dw) or from dw; whatever lies behind the kernel in the range is read from the gradient arena.  Nothing is
 * zeroed.  Needs accumulate = 0. */
typedef struct gct2_adam_args {
  float* p; float* m; float* v;
  void* shadow; int shadow_dtype;      /* compute-dtype copy of p over the same range, or NULL */
  size_t n;
  float alpha, beta1, beta2, eps, grad_mul;
  /* defer != 0 (r04): the weight-gradient call launches NO optimizer step; it records where it left the kernel gradient - slab_base
   * / nslab / slab_stride: `nslab` partial tensors in the ctx's weight-gradient scratch (nslab = 0: the gradient is in dw) - and the
   * caller runs the step later with gct2_adam_apply(this struct, dw, 16*Cin*Cout, stream): the same launch, the same bits.  Until
   * then the scratch of that ctx must not be handed to another weight-gradient call (the engine gives such layers a ctx of their
   * own) and dw (plus whatever the range holds behind the kernel in the gradient arena) must stay untouched.  The engine uses it to run the optimizer step of the layers the
   * forward pass needs LAST inside the bottleneck window of the next forward pass. */
  int defer;
  const float* slab_base; int nslab; size_t slab_stride;     /* out (defer != 0) */
} gct2_adam_args;

/* weight + bias gradient: dw[kh,kw,i,o] += sum_{b,oh,ow} x[b,2oh+kh-1,2ow+kw-1,i]*dz[b,oh,ow,o],
 * db[o] += sum dz[..,o].  dw: fp32 (4,4,Cin,Cout), db: fp32[Cout] or NULL.  accumulate != 0: dw is a running (or
 * zeroed) buffer and is added to; accumulate == 0: dw is overwritten (saves reading it).  db follows the same flag. */
int gct2_conv4s2_wgrad(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* dz, int lddz, float* dw,
                       float* db, int B, int H, int W, int Cin, int Cout, int accumulate,
                       gct2_adam_args* adam /* or NULL */, void* stream);
/* the optimizer step a weight-gradient call with adam->defer != 0 left to the caller (see gct2_adam_args) */
int gct2_adam_apply(const gct2_adam_args* adam, float* dw, size_t nw, void* stream);

/* ---- UpShuffle = Conv2DTranspose(f, 4, 2, 'same', relu)   train.py:145-156 ------------------ */
/* y[b,2ih+kh-1,2iw+kw-1,o] += x[b,ih,iw,i] * w[kh,kw,o,i]; then bias, relu.
 * x: [B,H,W,Cin] view;  w: Keras kernel (4,4,Cout,Cin);  y: [B,2H,2W,Cout] view. */
int gct2_convT4s2_fwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w, const float* bias,
                      void* y, int ldy, int B, int H, int W, int Cin, int Cout, int relu,
                      void* stream);

/* dx[b,ih,iw,i] (+)= mask * sum_{kh,kw,o} dz[b,2ih+kh-1,2iw+kw-1,o] * w[kh,kw,o,i]
 * dz: [B,2H,2W,Cout];  dx/act: [B,H,W,Cin] views;  mask/accumulate as for conv4s2_dgrad. */
int gct2_convT4s2_dgrad(gct2_ctx* ctx, int dtype, const void* dz, int lddz, const void* w, const void* act,
                        int ldact, void* dx, int lddx, int B, int H, int W, int Cin, int Cout,
                        int accumulate, float* db, int db_split, float* db2, int db_accumulate, void* stream);

/* dw[kh,kw,o,i] (+)= sum_{b,ih,iw} x[b,ih,iw,i] * dz[b,2ih+kh-1,2iw+kw-1,o]; db[o] += sum dz; accumulate as for
 * conv4s2_wgrad. */
int gct2_convT4s2_wgrad(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* dz, int lddz, float* dw,
                        float* db, int B, int H, int W, int Cin, int Cout, int accumulate,
                        gct2_adam_args* adam /* or NULL */, void* stream);

/* ---- the reference's off-by-default model variants ------------------------------------------------------------------------
 * Block = block_depth x Conv2D(filters, 3, 1, 'same', relu) (train.py:20, 123-143) and the bias-free projection
 * Dense(input_channels) of Residual's residual=True mode (train.py:26, 104-112; a Dense on a rank-4 tensor is a 1 x 1 convolution,
 * its (Cin, Cout) kernel the same memory as (1, 1, Cin, Cout)).  Stride-1 'same' convolution, KS odd (symmetric padding):
 *   y[b,h,w,o] = act(bias[o] + sum_{kh,kw,i} x[b,h+kh-p,w+kw-p,i] w[kh,kw,i,o]),  p = (KS-1)/2;  w: (KS,KS,Cin,Cout) of `dtype`.
 * dgrad: dx[b,h,w,i] (+)= mask * sum dz[b,h-kh+p,w-kw+p,o] w[kh,kw,i,o] (mask / accumulate as for conv4s2_dgrad);
 * wgrad: dw (+)= sum x dz (fp32), db (+)= column sums of dz.  16-bit dtypes with whole 8-channel chunks (Cin, Cout and the lds
 * multiples of 8, 16-byte aligned views, KS <= 5) run on the matrix cores as a third tap-GEMM form (KS x KS taps on one grid;
 * split-K / slabs through the ctx scratch like the 4x4 layers); fp32 on the fp32 matrix cores, every shape, when the ctx is in
 * GCT2_F32_MATH_MFMA mode (gct2_ctx_set_f32_math); fp32 otherwise and the remaining 16-bit shapes (the 3-channel input of a Block in
 * front of level 0) on direct kernels, one thread per output. */
int gct2_conv2d_s1_fwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w, const float* bias, void* y, int ldy,
                       int B, int H, int W, int Cin, int Cout, int KS, int relu, void* stream);
int gct2_conv2d_s1_dgrad(gct2_ctx* ctx, int dtype, const void* dz, int lddz, const void* w, const void* act, int ldact,
                         void* dx, int lddx, int B, int H, int W, int Cin, int Cout, int KS, int accumulate, void* stream);
int gct2_conv2d_s1_wgrad(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* dz, int lddz, float* dw, float* db,
                         int B, int H, int W, int Cin, int Cout, int KS, int accumulate, void* stream);
/* d[pix,c] = act[pix,c] > 0 ? d[pix,c] : 0 - the autodiff of a fused ReLU where no producing kernel applies the mask itself */
int gct2_relu_mask(int dtype, const void* act, int ldact, void* d, int ldd, size_t npix, int C, void* stream);
/* dst[pix,c] += src[pix,c] (train.py:112 `input + ...` and the gradient joins of the variants) */
int gct2_add(int dtype, void* dst, int lddst, const void* src, int ldsrc, size_t npix, int C, void* stream);
/* out = a[b] * x + c[b] * eps, fp32, per-image coefficients (eps = NULL: out = a[b] * x): the targets and prediction weights of
 * train.py:238-252 (ODE target, epsilon / scaled-epsilon prediction, prediction_weighting).  Every operation is rounded once, as in
 * the reference's unfused op chain: fl(fl(a[b] * x) + fl(c[b] * eps)), never a fused multiply-add.  out may be x (in place). */
int gct2_mix_per_image(const float* x, const float* eps, const float* a, const float* c, float* out, int B, size_t per_image,
                       void* stream);

/* ---- Dense(3) head on a rank-4 input   train.py:198-202 ------------------------------------- */
/* y[m,o] = b[o] + sum_i x[m,i] * w[i,o];  x: [M,Cin] view of `dtype`; w fp32 (Cin,Cout), Cout <= 4;
 * y: fp32 [M,Cout] contiguous (the loss is taken in fp32, train.py:262-263).  GCT2_F16: the values are rounded to fp16
 * first (mixed_float16 Dense output, cast to fp32 at train.py:263). */
int gct2_dense_fwd(int dtype, const void* x, int ldx, const float* w, const float* b, float* y,
                   int M, int Cin, int Cout, void* stream);

/* dx[m,i] = mask * sum_o dy[m,o] w[i,o] for i < Cmask (channels >= Cmask get no gradient written);
 * dw[i,o] (+)= sum_m x[m,i] dy[m,o];  db[o] (+)= sum_m dy[m,o]  (accumulate != 0 adds, else overwrites).   dy fp32 [M,Cout].
 * mask = x[m,i] > 0 (x is the ReLU output feeding the head; train.py:188,198).  GCT2_F16: dy is rounded to fp16 on read
 * (the gradient entering a mixed_float16 Dense output is fp16). */
int gct2_dense_bwd(int dtype, const void* x, int ldx, const float* w, const float* dy, void* dx,
                   int lddx, float* dw, float* db, int M, int Cin, int Cout, int Cmask,
                   int accumulate, void* stream);

/* fused train-step head (16-bit dtypes): dense_fwd + mse_fwd_bwd + dense_bwd in ONE pass over x (= R_0):
 *   pred = x w + b;  loss = mean((pred - target)^2);  dpred = loss_scale * 2 (pred - target) / (M Cout);
 *   dx[m, i < Cmask] = (x > 0) * dpred w^T;  dw (+)= x^T dpred;  db (+)= sum dpred.
 * GCT2_F16 follows Keras' mixed_float16 rounding points (train.py:43-45): the Dense output and the gradient entering it are
 * rounded to fp16 (pred is stored as fp32 of the fp16 value); GCT2_BF16 keeps both in fp32.
 * target: fp32 [M,Cout]; pred: fp32 [M,Cout] or NULL; loss: 1 float; partials: >= 1024 floats scratch.
 * x2 (may be NULL): the input channels [Cmask, Cin) come from this second view (ldx2 elements per pixel, at most 4
 * channels, 8-byte aligned rows) instead of x - the concat [UpShuffle_0 output, image] is then never assembled at all
 * (the image lives in its packed copy only).  Needs Cmask = 64, Cout <= 3 and a registered workspace.
 * Pad channels [Cin, ldx) of x: the matrix-core version masks them, and with x2 also x's own channels [Cmask, ldx) and the slots
 * [Cin - Cmask, 4) of x2: they may hold anything, NaN included.  It runs when Cmask = 64, Cout <= 3, the registered workspace holds
 * min(512, ceil(ceil(M / 16) / 4)) * 288 floats, and 64 <= Cin <= 72 with ldx >= 72 (without x2) or 64 <= Cin <= 68 (with x2).
 * Every other call without x2 falls back, silently, to the LDS-tile version (with x2: GCT2_EINVAL), which multiplies the pad
 * channels by zero weights: they must be FINITE there, or pred, the loss and every gradient become NaN.
 * Replaces train.py:198-202 + 262-272 and their autodiff inside Keras fit (train.py:516). */
int gct2_dense_head_train(gct2_ctx* ctx, int dtype, const void* x, int ldx, const float* w, const float* b,
                          const float* target, float* pred, void* dx, int lddx, float* dw, float* db,
                          float* loss, float* partials, int M, int Cin, int Cout, int Cmask,
                          const float* loss_scale_ptr, float* db_dx /* column sums of dx, or NULL */,
                          const void* x2, int ldx2, int accumulate /* dw, db, db_dx: 0 = overwrite, else add */,
                          void* stream);

/* ---- per-timestep heads: Dense(Cout * steps) + Reshape(.., steps, Cout) + tf.gather(prediction, t - 1, batch_dims=3)
 * (train.py:199, 203, 211-214) ----
 * Because t is constant over an image, the gathered head is a Cin -> Cout head whose weight slice is picked per image; the full
 * steps * Cout outputs are never formed.  w: fp32 (Cin, steps * Cout), the Keras Dense kernel, output index s * Cout + o; b: fp32
 * [steps * Cout] or NULL; t_int: device int32[B]; image i uses slice s = t_int[i] - 1.  A t_int outside 1..steps is a caller error:
 * the kernels clamp it into range before they form an address (nothing outside the tensors is read or written).
 * x: [B * HW, Cin] view of `dtype` with ldx (pad channels [Cin, ldx) are never read); 1 <= Cout <= 4.  A work-group never mixes the
 * pixels of two images.  ctx (may be NULL) only receives the launch-log tokens "dense_steps:fwd" / "dense_steps:bwd".
 *
 * forward: y[m,o] = b[s*Cout+o] + sum_k x[m,k] w[k, s*Cout+o], fp32 [B*HW, Cout] contiguous: gct2_dense_fwd's accumulation order
 * (k ascending, one fmaf per term, bias last) and its GCT2_F16 rounding - image i's rows equal, bit for bit, gct2_dense_fwd on
 * those rows with a contiguous copy of its slice. */
int gct2_dense_steps_fwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const float* w, const float* b, const int32_t* t_int,
                         float* y, int B, int HW, int Cin, int Cout, int steps, void* stream);
/* backward: dx as gct2_dense_bwd with the image's slice (ReLU mask x > 0, channels >= Cmask untouched, GCT2_F16: dy rounded to fp16
 * on read; dx == NULL or Cmask == 0: no input gradient).  dw (Cin, steps*Cout) and db [steps*Cout] (may be NULL) are written IN FULL:
 * slice s receives the sum over the images with t_int - 1 == s, every other slice +0.0 (accumulate != 0: added instead).  No
 * atomics: every work-group (one image, one chunk of its pixels) leaves one partial row in `scratch`, and a second launch adds the
 * rows per slice over images and chunks in ascending order - the bits depend on the inputs alone.
 * scratch: device floats, 16-byte aligned, at least what gct2_dense_steps_scratch reports (host only, no launch).
 * GCT2_EINVAL before any launch: unknown dtype, NULL x / w / t_int / y (dy, dw, scratch), non-positive B / HW / Cin / steps, Cout
 * outside 1..4, ldx < Cin, lddx < Cmask, Cmask outside 0..Cin, B > 65535, B*HW or Cin*steps*Cout at or beyond 2^31 (the kernels index
 * pixels and weights with int), (Cin+1)*Cout > 2048, a Cin too large for the LDS tile, scratch_floats below the query's figure. */
int gct2_dense_steps_scratch(int B, int HW, int Cin, int Cout, size_t* floats);
int gct2_dense_steps_bwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const float* w, const int32_t* t_int, const float* dy,
                         void* dx, int lddx, float* dw, float* db, float* scratch, size_t scratch_floats, int B, int HW, int Cin,
                         int Cout, int steps, int Cmask, int accumulate, void* stream);

/* ---- the hidden Dense(Chid, relu) layer in front of the Dense(Cout) head (train.py:195-199; the first one is commented out in the
 * reference) as ONE kernel per direction: the [M, Chid] hidden activation - the largest tensor the network would have - is never
 * stored; the backward call recomputes it from x.  Per pixel m
 *   h[j]   = round_T(relu(b1[j] + sum_i x[m,i] w1[i,j]))        y[m,o] = b2[o] + sum_j h[j] w2[j,o]
 * x: [M, Cin] view of `dtype`, row pitch ldx; the pad channels [Cin, ldx) are never multiplied (the plain kernels do not read them, the
 * matrix-core ones zero them in registers): they may hold anything, NaN included.  w1: (Cin, Chid) in `dtype` - the compute-dtype operand
 * copy, as the convolutions read their kernels; b1: fp32 [Chid]; w2: fp32 (Chid, Cout); b2: fp32 [Cout]; y: fp32 [M, Cout] contiguous.
 * fp32 accumulation (the plain kernels form the two sums behind h and dh in fp64 when `dtype` is GCT2_F32, so that both are correctly
 * rounded fp32 values); round_T is ONE rounding to `dtype` (the identity for GCT2_F32) - the value a stored activation would have had,
 * so the pair means "gct2_conv2d_s1_fwd(KS = 1, relu) followed by gct2_dense_fwd".  GCT2_F16 follows their rounding points: y is rounded
 * to fp16 (stored as fp32), dy is rounded to fp16 on read.
 * backward (h recomputed):
 *   dh[j] = round_T((h[j] > 0) * sum_o dy[m,o] w2[j,o])         dw2 (+)= h^T dy     db2 (+)= sum_m dy
 *   dw1 (+)= x^T dh      db1 (+)= sum_m dh      dx[m,i] = (x[m,i] > 0) * sum_j dh[j] w1[i,j] for i < Cmask
 * (x is a ReLU output: dx is the gradient at its pre-activation, as in gct2_dense_bwd).  Channels >= Cmask of dx are left untouched;
 * dx == NULL or Cmask == 0: no input gradient.  accumulate != 0 adds to dw1 / db1 / dw2 / db2, else they are overwritten.  No atomics:
 * every work-group leaves ONE partial row [dw1 | db1 | dw2 | db2] in `scratch` and a second launch adds the rows in ascending work-group
 * order - the bits depend on the inputs alone.  scratch: device floats, 16-byte aligned, at least what gct2_dense2_scratch reports
 * (host only, no launch; monotone in M).
 * Kernels: 16-bit dtypes with Chid in {32, 64, 128}, Cin <= 80, ldx % 8 == 0 and x 16-byte aligned run layer 1, dh w1^T and x^T dh on
 * v_mfma_f32_16x16x32 (GCT2_DENSE2_FAST_PIXELS pixels per work-group; Cin is padded to a multiple of 32 with zeros inside the kernel);
 * everything else - fp32, other shapes, a ctx with gct2_ctx_force_direct - runs the plain kernels (Cin, Chid <= GCT2_DENSE2_PLAIN_MAX).
 * The launch log of ctx (may be NULL) receives "dense2:fwd:mfma" / "dense2:fwd:plain" / "dense2:bwd:mfma" / "dense2:bwd:plain".
 * GCT2_EINVAL before any launch, checked in THIS order (the first failing check names itself in gct2_last_error):
 *   1 unknown dtype; 2 NULL x / w1 / b1 / w2 / b2 / y (backward: x / w1 / b1 / w2 / dy / dw1 / db1 / dw2 / db2 / scratch); 3 non-positive
 *   M / Cin / Chid; 4 Cout outside 1..4; 5 ldx < Cin; 6 (backward) Cmask outside 0..Cin, or dx given and lddx < Cmask; 7 M at or beyond
 *   2^31 - GCT2_DENSE2_FAST_PIXELS; 8 Cin*Chid or Chid*Cout at or beyond 2^31; 9 Cin or Chid above GCT2_DENSE2_PLAIN_MAX; 10 (backward)
 *   scratch not 16-byte aligned; 11 (backward) scratch_floats below the query's figure.  gct2_dense2_scratch: NULL floats, then 3, 4, 7-9. */
#define GCT2_DENSE2_FAST_PIXELS 64
#define GCT2_DENSE2_PLAIN_MAX 256
int gct2_dense2_fwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w1, const float* b1, const float* w2, const float* b2,
                    float* y, int M, int Cin, int Chid, int Cout, void* stream);
int gct2_dense2_scratch(int M, int Cin, int Chid, int Cout, size_t* floats);
int gct2_dense2_bwd(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w1, const float* b1, const float* w2, const float* dy,
                    void* dx, int lddx, float* dw1, float* db1, float* dw2, float* db2, float* scratch, size_t scratch_floats,
                    int M, int Cin, int Chid, int Cout, int Cmask, int accumulate, void* stream);

/* UpShuffle_0's forward WITH the train-step head in its epilogue (16-bit dtypes): y = relu(convT(x) + bias) is consumed where
 * it is produced - Dense(3) + fp32 MSE + both of their gradients, exactly as gct2_dense_head_train computes them on the stored
 * activations (y is rounded to `dtype` first, like the tensor the separate call would have read) - and never written: dy
 * ([B,2H,2W,Cout] view) receives the gradient w.r.t. the layer's pre-activation, db its column sums (this layer's bias
 * gradient), head_dw / head_db the Dense gradients, loss the scalar.  Saves one write and one read of the largest activation
 * of the network plus the head launch (train.py:188, 198-202, 262-272 and their autodiff).
 * Needs Cout = 64, H and W multiples of 16, head_Cin - Cout <= 3 image channels in x2 (packed, ldx2 multiple of 4), head_Cout <= 3,
 * a ctx workspace of B*(H/16)*(W/16)*288 floats, and a source view and kernel within the 31-bit offsets of the kernel's loads:
 * B*H*W*ldx*2 + 2*Cin + 128 < 0x7ff00000 bytes (the span of x plus the largest lane and k-chunk offset added to it) and
 * 16*Cin*Cout*2 < 0x7ff00000; GCT2_EINVAL otherwise (use convT4s2_fwd + dense_head_train: this entry point has no fall-back of its
 * own).  dy, x2, target and pred are addressed with 64-bit offsets: their views may span any number of bytes. */
int gct2_convT4s2_fwd_head_train(gct2_ctx* ctx, int dtype, const void* x, int ldx, const void* w, const float* bias,
                                 const float* head_w, const float* head_b, const float* target, float* pred, void* dy,
                                 int lddy, float* head_dw, float* head_db, float* loss, int B, int H, int W, int Cin,
                                 int Cout, int head_Cin, int head_Cout, const float* loss_scale_ptr, float* db,
                                 const void* x2, int ldx2, int accumulate, void* stream);

/* ---- Trainer.call pieces   train.py:223-272 -------------------------------------------------- */
/* t_int[b] ~ U{1..steps} (train.py:224-226) and eps ~ N(0,1) (train.py:227) from a counter-based
 * Philox4x32-10 stream keyed by (seed, stream_id); `offset` = elements already drawn.
 * The stream (tests/pointwise_cases.py restates it on the host; tests/test_pointwise_exact_gpu.py pins it per element):
 *   Philox4x32-10 of Salmon et al. (SC'11), every one of the 64 bits of seed, stream_id and the counter index in use:
 *     counter = (idx & 0xffffffff, idx >> 32, stream_id & 0xffffffff, stream_id >> 32),  key = (seed & 0xffffffff, seed >> 32);
 *   element e (= offset + position in the output) uses the four output words r[0..3] of counter idx = e >> 2, so a draw may
 *   start and end inside a counter, and a draw split into several calls at any offsets equals the single call.
 *   gct2_rng_uniform_int: out = lo + ((r[e & 3] * range) >> 32) with range = hi_inclusive - lo + 1 formed in 64 bits.  Every
 *     lo <= hi_inclusive is valid, range up to 2^32 (lo = INT32_MIN, hi_inclusive = INT32_MAX: out = lo + r); hi_inclusive < lo is
 *     GCT2_EINVAL.  Integer arithmetic: the values are exact.
 *   gct2_rng_normal: Box-Muller.  Words (r[0], r[1]) make elements 4 idx (cosine) and 4 idx + 1 (sine), words (r[2], r[3]) elements
 *     4 idx + 2 and 4 idx + 3: with u = ((float)(r >> 8) + 0.5f) * 2^-24 (float32, each operation rounded; u in (0, 1], u = 1 at
 *     r >> 8 = 2^24 - 1 where 16777215.5 rounds to even), rad = sqrt(-2 ln u1), z = rad cos(2 pi u2) or rad sin(2 pi u2).
 *     Always finite (|z| < 5.9).  log2 / sin / cos run on the hardware transcendental units: within 5.3e-7 absolute of that formula
 *     evaluated in double (measured on an MI355X, profiles/rng_parity.json; the test asserts 2^-18). */
int gct2_rng_uniform_int(uint64_t seed, uint64_t stream_id, uint64_t offset, int32_t* out, size_t n,
                         int lo, int hi_inclusive, void* stream);
int gct2_rng_normal(uint64_t seed, uint64_t stream_id, uint64_t offset, float* out, size_t n,
                    void* stream);

/* noised = x*sqrt(a_b) + eps*sqrt(1-a_b), a_b = 0.25*(1 - t_b/(steps+1))^2  (train.py:85-93,229-234)
 * x, eps: fp32 [B, HW, C] contiguous; t_int: int32[B]; out: view [B*HW, C] of `dtype` with ldout.
 * GCT2_F32 / GCT2_BF16: fp32 arithmetic in the reference's order, every operation rounded once (no fused multiply-add):
 * t, om = 1 - t, a = (om * om) * 0.25, sqrt(a), sqrt(1 - a), fl(fl(x * sqrt(a)) + fl(eps * sqrt(1 - a))), and one more rounding at
 * a bf16 store.  GCT2_F32: t = (float)t_b / (float)(steps + 1), a division like train.py:87.  GCT2_BF16: t = (float)t_b *
 * (1.0f / (float)(steps + 1)); the last-bit difference this makes in sqrt(a) at some timesteps (36 of 200 at steps = 200) reaches a
 * bf16 output only where the fp32 sum is a tie of the store, about one element in 2^16 (tests/test_pointwise_exact_gpu.py pins
 * that form on images made of such ties).  GCT2_F16: every operation is rounded to fp16 as under
 * Keras' mixed_float16 policy, where x, eps and t are fp16 tensors (train.py:38, 227-234, 292).
 * out2 (may be NULL): a second view [B*HW, C] with ldout2 that receives the same values - the engine keeps a packed
 * copy of the image (ld 4) for DownShuffle_0 beside the slice of the concat buffer that Dense(3) reads. */
int gct2_noise_image(int dtype, const float* x, const int32_t* t_int, const float* eps, void* out,
                     int ldout, void* out2, int ldout2, int B, int HW, int C, int steps, void* stream);

/* the same with eps drawn inside the kernel from the positions [offset, offset + B*HW*C) of the gct2_rng_normal stream
 * (seed, stream_id): bit-identical to gct2_rng_normal followed by gct2_noise_image, without the eps round trip through HBM.
 * eps_out (may be NULL) receives the draws. */
int gct2_noise_image_rng(int dtype, const float* x, const int32_t* t_int, uint64_t seed, uint64_t stream_id,
                         uint64_t offset, float* eps_out, void* out, int ldout, void* out2, int ldout2, int B, int HW,
                         int C, int steps, void* stream);

/* the two calls above for ANY noise schedule (train.py:88-93: the author moves the `return` of alpha_dash): the kernels evaluate no
 * formula, they read the per-timestep pair from a device table the host filled in the reference's operation order
 * (trainer_math.noise_table).
 * coef: float[steps][2], 8-byte aligned; entry t - 1 = (sa, sb) = (sqrt(alpha_dash(t)), sqrt(1 - alpha_dash(t))) as the host formed
 * them - sb is never derived from sa.  Every thread reads its pair as one 8-byte load.  t_int[b] is clamped to 1..steps before the
 * address is formed (the rule of gct2_dense_steps_fwd: a value outside the range reads entry 1 or entry steps, never past the table).
 * GCT2_EINVAL for a NULL or misaligned coef and for steps < 1.
 * The mix, every operation rounded once (no fused multiply-add):
 *   GCT2_F32:  fl(fl(x * sa) + fl(eps * sb)).
 *   GCT2_BF16: the same, and one more rounding at the bf16 store.
 *   GCT2_F16:  (fp16)x * (fp16)sa and (fp16)eps * (fp16)sb, each rounded to fp16, then their fp16 sum; the host stores
 *              fp16-representable pairs for this dtype, so their conversion is exact.
 * Everything else as in the formula forms: out2, eps_out, the stream positions (gct2_noise_image_rng_table is bit-identical to
 * gct2_rng_normal followed by gct2_noise_image_table), and the train step's 16-bit fast path under the same conditions.  With the
 * table of the quadratic schedule both calls give the bits of gct2_noise_image / gct2_noise_image_rng (GCT2_BF16: with the product
 * form of t described above). */
int gct2_noise_image_table(int dtype, const float* x, const int32_t* t_int, const float* eps, const float* coef,
                           void* out, int ldout, void* out2, int ldout2, int B, int HW, int C, int steps, void* stream);
int gct2_noise_image_rng_table(int dtype, const float* x, const int32_t* t_int, uint64_t seed, uint64_t stream_id,
                               uint64_t offset, float* eps_out, const float* coef, void* out, int ldout, void* out2,
                               int ldout2, int B, int HW, int C, int steps, void* stream);

/* ---- log_sample, the reference's sampler (train.py:323-496, every objective switch of train.py:29-32): pointwise steps, fp32 state ---- */
/* fake = sqrt(alpha) x_theta + sqrt(1-alpha) eps_theta  (train.py:372-375, 441-444), alpha = alpha_dash(t) from the caller.
 * x_theta, eps_theta, fake: fp32 [npix*C]; the network input is also stored in `dtype` into the view out [npix, C] (ldout) and,
 * if non-NULL, out2 (ldout2) - the packed image and the image slice of the concat buffer. */
int gct2_diffusion_mix(int dtype, const float* x_theta, const float* eps_theta, float alpha, float* fake,
                       void* out, int ldout, void* out2, int ldout2, size_t npix, int C, void* stream);
/* one sampler update from the network's prediction, by objective (train.py:338-355, 382-413, 452-479); fp32 [n] each,
 * a = alpha = alpha_dash(t), a1 = alpha_prev = alpha_dash(t - 1) (ODE mode only, ignored otherwise):
 *   GCT2_SAMPLE_X          (predict_x)            x_theta = pred;  eps_theta = (fake - sqrt(a) pred) / sqrt(1-a)
 *   GCT2_SAMPLE_EPS        (epsilon)              eps_theta = pred;  x_theta = (fake - pred sqrt(1-a)) / sqrt(a)
 *   GCT2_SAMPLE_SCALED_EPS (predict_scaled_epsilon) eps_theta = pred / sqrt(1-a);  x_theta = (fake - pred) / sqrt(a)
 *   GCT2_SAMPLE_ODE        (ordinary_differential_equation)
 *                          x_theta = (pred sqrt(1-a) - fake sqrt(1-a1)) / (sqrt(a1) sqrt(1-a) - sqrt(a) sqrt(1-a1));
 *                          eps_theta is NOT touched (the reference never updates it in this branch; may be NULL).
 *   GCT2_SAMPLE_V          (predict_v: the network predicts v = sqrt(a) eps - sqrt(1-a) x, Salimans & Ho 2022, "Progressive
 *                          Distillation for Fast Sampling of Diffusion Models")
 *                          x_theta = fl(fl(sa fake) - fl(sb pred));  eps_theta = fl(fl(sb fake) + fl(sa pred)),
 *                          sa = (float)sqrt(a), sb = (float)sqrt(1 - a): nothing is divided, alpha = 0 is valid in this mode.
 * Mode code 4 is reserved and refused (GCT2_EINVAL) by every entry point that takes a mode.
 */
enum { GCT2_SAMPLE_X = 0, GCT2_SAMPLE_EPS = 1, GCT2_SAMPLE_SCALED_EPS = 2, GCT2_SAMPLE_ODE = 3, GCT2_SAMPLE_V = 5 };
/* alpha / alpha_prev are DOUBLES: the reference forms every coefficient (and the ODE denominator, a difference of nearly equal
 * products at steps = 200) from Python floats and only then multiplies fp32 tensors by it; the library does the same on the host. */
int gct2_diffusion_update(int mode, const float* pred, const float* fake, double alpha, double alpha_prev, float* x_theta,
                          float* eps_theta, size_t n, void* stream);
/* ---- Denoiser.generate: one strided DDIM / DDPM sampling step (Song et al., "Denoising Diffusion Implicit Models", eq. 12) in ONE
 * launch - gct2_diffusion_update, the clip of the x0 estimate and gct2_diffusion_mix to a_prev, without x_theta and eps_theta ever
 * reaching memory.  B images of per_image = H*W*C fp32 elements each, contiguous: pred, fake_in, fake_out and (may be NULL) x0_out are
 * [B * per_image]; out [B*H*W, C] (ldout) and (may be NULL) out2 (ldout2) are the network's input views in `dtype` as for
 * gct2_diffusion_mix.  fake_out may equal fake_in.  mode: GCT2_SAMPLE_X, _EPS, _SCALED_EPS or _V; GCT2_SAMPLE_ODE is GCT2_EINVAL (that
 * network predicts one step back only), and so is the reserved code 4.  a_t, a_prev, sigma2, clip are DOUBLES, like gct2_diffusion_update's.
 * GCT2_EINVAL unless a_t in [0, 1) (> 0 for the epsilon modes; 0 is valid for X and V), a_prev in [0, 1], 0 <= sigma2 and (1.f - (float)a_prev) - (float)sigma2 >= 0,
 * per_image a multiple of C, ldout >= C, B * per_image < 2^31.
 * Element i of image b, p = pred, f = fake_in; fp32, every operation rounded once (no fused multiply-add):
 *   update   sa = (float)sqrt(a_t), sb = (float)sqrt(1 - a_t) (square roots in double, one cast each), then gct2_diffusion_update:
 *              X: x = p, e = (f - sa p) / sb;   EPS: e = p, x = (f - p sb) / sa;   SCALED_EPS: e = p / sb, x = (f - p) / sa;
 *              V: x = sa f - sb p, e = sb f + sa p (each product and each sum rounded on its own)
 *   clip     only when clip > 0: c = (float)clip, x = x < -c ? -c : (x > c ? c : x) (a NaN stays NaN), then e = (f - sa x) / sb in
 *            every mode (eps re-derived from the clipped x0).  clip <= 0: x, e are gct2_diffusion_update's bits.
 *   re-noise A = (float)a_prev, S = (float)sigma2, cx = sqrtf(A), ce = sqrtf((1.f - A) - S), cz = sqrtf(S);
 *            S == 0: fake' = cx x + ce e, nothing is drawn - with clip <= 0 the bits of gct2_diffusion_update followed by
 *            gct2_diffusion_mix(alpha = a_prev);  else fake' = (cx x + ce e) + cz z with z = the normal gct2_rng_normal writes for
 *            element offset + b * image_stride + i of the stream (seed, stream_id), bit for bit, for any offset, image_stride and
 *            per_image (an image may start and end inside a Philox counter; the counter index is 64 bits wide)
 *   stores   fake_out[i] = fake'; out / out2: one rounding of fake' to `dtype` at row (b per_image + i) / C, channel (b per_image + i) % C,
 *            nothing else in the row is touched; x0_out[i] = x if given. */
int gct2_diffusion_step(int mode, int dtype, const float* pred, const float* fake_in, double a_t, double a_prev, double sigma2,
                        double clip, uint64_t seed, uint64_t stream_id, uint64_t offset, uint64_t image_stride, float* fake_out,
                        float* x0_out, void* out, int ldout, void* out2, int ldout2, int B, size_t per_image, int C, void* stream);
/* the starting noise of the same sampler: fake_out[b * per_image + i] = z of stream element offset + b * image_stride + i (the rule
 * above), also stored once rounded into out / out2.  Shapes and GCT2_EINVAL as for gct2_diffusion_step. */
int gct2_diffusion_start(int dtype, uint64_t seed, uint64_t stream_id, uint64_t offset, uint64_t image_stride, float* fake_out,
                         void* out, int ldout, void* out2, int ldout2, int B, size_t per_image, int C, void* stream);
/* ---- image-conditioned generation (generate(init=, strength=, mask=)): the start from an image and the masked step, ONE launch each.
 * Shapes, views and GCT2_EINVAL rules are gct2_diffusion_step's: B images of per_image = H*W*C fp32 elements, per_image a multiple of C,
 * ldout >= C, B * per_image < 2^31, out / out2 the network's input views in `dtype`; fp32, every operation rounded once (no fused
 * multiply-add); the bits do not depend on which kernel form runs (one element per thread where only the starting noise is drawn; with
 * the step's noise a thread per Philox counter, 16-byte accesses when offset, offset0, image_stride and per_image are multiples of 4
 * and the fp32 planes are 16-byte aligned).  known must not overlap fake_out.
 *
 * gct2_diffusion_start_image: the image `known` [B * per_image] noised to alpha a (a double in [0, 1], else GCT2_EINVAL):
 *   A = (float)a, cx = sqrtf(A), ck = sqrtf(1.f - A);  fake_out[i] = cx known[i] + ck z0[i],  z0 = the normal gct2_rng_normal writes for
 *   element offset + b * image_stride + i of the stream (seed, stream_id) - the bits of gct2_rng_normal followed by
 *   gct2_diffusion_mix(x = known, e = z0, alpha = a), the once-rounded copies in out / out2 included.  known must not be NULL. */
int gct2_diffusion_start_image(int dtype, const float* known, double a, uint64_t seed, uint64_t stream_id, uint64_t offset,
                               uint64_t image_stride, float* fake_out, void* out, int ldout, void* out2, int ldout2, int B,
                               size_t per_image, int C, void* stream);
/* gct2_diffusion_step_masked: gct2_diffusion_step with the region a mask marks as kept pinned to a known image (inpainting).  The
 * arguments of gct2_diffusion_step, plus known [B * per_image] fp32 (the clean image), mask [B * per_image / C] fp32 (one value per
 * pixel, shared by its C channels; row (b per_image + i) / C) and offset0, the stream element of image 0's STARTING noise (images
 * image_stride apart, like offset).  known and mask must not be NULL (GCT2_EINVAL); every other rule is gct2_diffusion_step's.
 * Element i of image b, m = the mask value of its pixel:
 *   x, e     gct2_diffusion_step's update and clip, bit for bit
 *   g        gct2_diffusion_step's fake': cx x + ce e, plus cz z when (float)sigma2 != 0, z at element offset + b image_stride + i
 *   h        cx known + ck z0,  ck = sqrtf(1.f - A),  z0 at element offset0 + b image_stride + i: the kept region follows the forward
 *            process with the image's own fixed starting noise (what gct2_diffusion_start_image wrote at its alpha), so a run at
 *            eta = 0 is deterministic
 *   fake'    m >= 1 ? g : (m <= 0 ? h : m g + (1.f - m) h)
 *   x0_out   m >= 1 ? x : (m <= 0 ? known : m x + (1.f - m) known)      (if given)
 * The selects are deliberate: a fully masked pixel (m >= 1) has gct2_diffusion_step's bits, and a NaN or an infinity in g or x (the
 * epsilon objectives divide by sqrt(a_t), 0.0025 at t = steps) never reaches a kept pixel (m <= 0).  Mask values outside [0, 1] act as
 * 0 or 1 through the comparisons; a NaN mask value fails both and blends to NaN.  Stores as gct2_diffusion_step's; fake_out may equal
 * fake_in.  Measured on one MI355X at 64x128x128x3, bf16 views: profiles/img2img_bench.json. */
int gct2_diffusion_step_masked(int mode, int dtype, const float* pred, const float* fake_in, const float* known, const float* mask,
                               double a_t, double a_prev, double sigma2, double clip, uint64_t seed, uint64_t stream_id, uint64_t offset,
                               uint64_t offset0, uint64_t image_stride, float* fake_out, float* x0_out, void* out, int ldout, void* out2,
                               int ldout2, int B, size_t per_image, int C, void* stream);
/* gct2_diffusion_step_multistep: one second-order multistep step of the probability-flow ODE (DPM-Solver++ 2M, Lu et al. 2022, "DPM-Solver++:
 * Fast Solver for Guided Sampling of Diffusion Probabilistic Models") in ONE launch - gct2_diffusion_step at sigma2 = 0 with the x0 estimate
 * of the re-noising replaced by D = x + c (x - hist_in), the estimate extrapolated from the one of the step before.  c1 is a host scalar
 * (trainer_math.multistep_coefficient: h / (2 h_prev) in half-log-SNR), hist_in / hist_out one fp32 plane [B * per_image] carried
 * between steps.  There is no sigma2: the solver is deterministic.
 * Shapes, views, alignment freedom and GCT2_EINVAL rules are gct2_diffusion_step's: modes X / EPS / SCALED_EPS / V (ODE and the reserved
 * code 4 refused), a_t in [0, 1) (> 0 for the epsilon modes), a_prev in [0, 1], per_image a multiple of C, ldout >= C, B * per_image < 2^31.
 * known and mask are both NULL (the plain step) or both non-NULL (the masked step: gct2_diffusion_step_masked's known [B * per_image]
 * and mask [B * per_image / C]); one without the other is GCT2_EINVAL.  seed, stream_id, offset0 and image_stride are read only in the
 * masked form, for the starting noise z0, with exactly the meaning they have in gct2_diffusion_step_masked.
 * c1 must be finite (also once cast to fp32), else GCT2_EINVAL; hist_in must not be NULL when (float)c1 != 0, else GCT2_EINVAL.
 * Aliasing: hist_out may be NULL, hist_out may equal hist_in, fake_out may equal fake_in: a thread reads its element before it writes
 * it.  x0_out (may be NULL) and known overlap nothing that is written.
 * Element i of image b, fp32, every operation rounded once (no fused multiply-add):
 *   x, e        gct2_diffusion_step's update and clip, bit for bit
 *   hist_out[i] = x: the clipped network estimate, not yet extrapolated and not yet composited
 *   c = (float)c1 == 0 (wave-uniform):  g = cx x + ce e,  cx = sqrtf(A), ce = sqrtf(1.f - A), A = (float)a_prev: the bits of
 *               gct2_diffusion_step at sigma2 = 0.  hist_in is never read: NaN / infinity garbage there (or NULL) is harmless
 *   c != 0:     d = x + c * (x - hist_in[i]);  ed = (fake_in[i] - sa d) / sb;  g = cx d + ce ed.  d is not clipped again
 *   plain form  fake' = g, x0_out = x
 *   masked form fake' and x0_out are gct2_diffusion_step_masked's selects over g, h = cx known + ck z0, x and known, bit for bit:
 *               fake' = m >= 1 ? g : (m <= 0 ? h : m g + (1.f - m) h),  x0_out = m >= 1 ? x : (m <= 0 ? known : m x + (1.f - m) known);
 *               a NaN or an infinity of g or x never reaches a kept pixel (m <= 0)
 *   stores      gct2_diffusion_step's: fake_out[i] = fake', one rounding of fake' to `dtype` in out / out2
 * Measured on one MI355X at 64x128x128x3, bf16 views: profiles/multistep_bench.json. */
int gct2_diffusion_step_multistep(int mode, int dtype, const float* pred, const float* fake_in, const float* hist_in, const float* known,
                                  const float* mask, double a_t, double a_prev, double c1, double clip, uint64_t seed, uint64_t stream_id,
                                  uint64_t offset0, uint64_t image_stride, float* fake_out, float* hist_out, float* x0_out, void* out,
                                  int ldout, void* out2, int ldout2, int B, size_t per_image, int C, void* stream);
/* ---- dynamic thresholding (generate(clip_denoised="dynamic"); Saharia et al. 2022, "Photorealistic Text-to-Image Diffusion Models with
 * Deep Language Understanding" (Imagen), section 2.3): per image and per step, a high order statistic of |x0| takes the place of the
 * fixed clip bound, and an estimate clipped to it is scaled back to the fixed bound.  Two calls per step: the select, then the step.
 *
 * gct2_x0_quantile: per image, the rank-th smallest |x0| of the step's own estimate, exactly - no interpolation, no sampling, no
 * approximation by histogram bin.  pred, fake: fp32 [B * per_image]; rows: fp32 [B][2]; q_out: fp32 [B] or NULL.
 *   key order   x_i is gct2_diffusion_step's UNCLIPPED update for the mode (X: x = p; EPS: x = (f - p sb) / sa; SCALED_EPS: x = (f - p) / sa;
 *               V: x = sa f - sb p), sa = (float)sqrt(a_t), sb = (float)sqrt(1 - a_t) formed exactly as the step forms them, every
 *               operation rounded once: the select's x_i is the step's x_i bit for bit.  key_i = bits(x_i) & 0x7fffffff, compared as
 *               uint32: the order of |x| with -0 = +0, +inf above every finite value and every NaN above +inf.
 *   statistic   q_b = the value whose key is the rank-th smallest (1-based) among the per_image keys of image b.
 *   finishing   once per image, F = (float)floor:  s_b = (q_b > F && q_b < INFINITY) ? q_b : F  (a NaN or infinite q_b falls back to
 *               the fixed bound);  r_b = (s_b == F) ? 1.0f : F / s_b  (one fp32 division);  rows[2b] = s_b, rows[2b+1] = r_b,
 *               q_out[b] = q_b (the raw bits).
 *   modes       GCT2_SAMPLE_X, _EPS, _SCALED_EPS, _V; GCT2_SAMPLE_ODE and the reserved code 4 are GCT2_EINVAL.  In mode X fake is not
 *               read and may be NULL: the call is then "the k-th smallest |v| per row" of any fp32 plane.  a_t follows
 *               gct2_diffusion_step's rules: in [0, 1), > 0 for the epsilon modes.
 *   GCT2_EINVAL unless 1 <= rank <= per_image, floor is finite and > 0 (also once cast to fp32), B * per_image < 2^31, and
 *               scratch_bytes >= what gct2_x0_quantile_scratch(B, per_image, &bytes) reports (scratch: device memory, 4-byte aligned).
 *   stream      the call assumes nothing about the scratch contents: it zeroes what it needs on `stream`.  No host synchronisation and
 *               no device-to-host copy: the call can sit between graph replays of the network.  The result is a pure function of
 *               the inputs - the same bits on every run and for every grid size: only integer atomics add (their result does not
 *               depend on the order), no floating-point atomics.
 *   how         a radix select over the 31 key bits in three digit passes (11 + 10 + 10 bits, the top digit first) and a finishing
 *               launch; every pass re-forms x from pred / fake, nothing is materialised.  Measured on one MI355X at 64x128x128x3:
 *               profiles/dynamic_threshold_bench.json. */
int gct2_x0_quantile_scratch(int B, size_t per_image, size_t* bytes);
int gct2_x0_quantile(int mode, const float* pred, const float* fake, double a_t, uint32_t rank, double floor, float* rows, float* q_out,
                     void* scratch, size_t scratch_bytes, int B, size_t per_image, void* stream);
/* gct2_diffusion_step_dynamic: the step with a per-image bound - gct2_diffusion_step, gct2_diffusion_step_masked and
 * gct2_diffusion_step_multistep in one entry point, with rows [B][2] = {s_b, r_b} (what gct2_x0_quantile wrote) in the place of the
 * scalar clip.  The arguments are the union of the masked and the multistep step's; every rule not named here is theirs.
 *   forms       known and mask both NULL: the plain step; both non-NULL: the masked step (one alone is GCT2_EINVAL).  The multistep
 *               form is taken when hist_in or hist_out is non-NULL or (float)c1 != 0; it is deterministic: with (float)sigma2 != 0
 *               it is GCT2_EINVAL.  c1 must be finite in fp32, hist_in non-NULL when (float)c1 != 0.  rows == NULL is GCT2_EINVAL.
 *   element i of image b, s = rows[2b], r = rows[2b+1], after gct2_diffusion_step's unclipped update x:
 *               x = x < -s ? -s : (x > s ? s : x)      (a NaN stays NaN)
 *               x = x * r                               (one rounded multiply; r == 1.0f leaves the bits alone)
 *               e = (f - sa * x) / sb                   (eps re-derived, as the fixed clip does)
 *               everything after that is the existing step's bits: rows {F, 1} for every image give gct2_diffusion_step /
 *               _step_masked / _step_multistep at clip = F.  hist_out and x0_out carry this thresholded x; the multistep
 *               extrapolation d = x + c (x - hist_in) is not thresholded again.  |x| <= F exactly when F is a power of two (the
 *               default 1): s fl(F / s) rounds back to F; for another F it can land one unit in the last place above it.
 *   masked form the select ran over the WHOLE network estimate, kept pixels included: the bound of an image does not know its mask.
 * Measured on one MI355X at 64x128x128x3, bf16 views: profiles/dynamic_threshold_bench.json. */
int gct2_diffusion_step_dynamic(int mode, int dtype, const float* pred, const float* fake_in, const float* hist_in, const float* known,
                                const float* mask, const float* rows, double a_t, double a_prev, double sigma2, double c1, uint64_t seed,
                                uint64_t stream_id, uint64_t offset, uint64_t offset0, uint64_t image_stride, float* fake_out,
                                float* hist_out, float* x0_out, void* out, int ldout, void* out2, int ldout2, int B, size_t per_image,
                                int C, void* stream);
/* ---- two-network guidance (generate(guide=...): autoguidance, Karras et al. 2024, "Guiding a Diffusion Model with a Bad Version of
 * Itself"; class guidance between two denoisers, Liu et al. 2022, "Compositional Visual Generation with Composable Diffusion Models"):
 * the step samples from p = p_guide + w (p_main - p_guide), two networks' predictions under the same objective at the same fake.
 *   the combine fp32, no contraction, every operation rounded once:  d = pred - pred_guide;  t = (float)w * d;  p = pred_guide + t.
 *               w = 1 is pred up to that rounding, w = 0 is pred_guide's bits on finite planes (t is a zero; a -0 of pred_guide may become +0).  p never reaches memory:
 *               the step and the select each form it from the two planes, by the same three operations, hence the same bits.
 *
 * gct2_diffusion_step_guided: ONE launch for the plain, with-noise, masked, multistep and dynamic forms of the step.  The arguments are
 * gct2_diffusion_step_dynamic's with pred_guide and w behind pred, the scalar clip behind c1 and a second pair of views out3 / out4
 * behind out / out2; every rule not named here (the forms, c1, sigma2, the alignment-selected paths, B * per_image < 2^31, the Philox
 * positions) is the existing entry points'.
 *   bound       rows == NULL: the scalar clip, 0 = none (gct2_diffusion_step's rule); rows != NULL: the per-image bound
 *               (gct2_diffusion_step_dynamic's rule), clip must then be 0, else GCT2_EINVAL.
 *   pred_guide  fp32 [B * per_image], or NULL: p = pred, and (float)w must be 1, else GCT2_EINVAL.  w must be finite in fp32.
 *   out3, out4  the guide engine's input views (compute dtype, leading dimensions ldout3 / ldout4 >= C): the kernel stores there the
 *               value it stores to out / out2.  Both may be NULL; out4 without out3 is GCT2_EINVAL.
 *   plain form  pred_guide, out3 and out4 all NULL: every output is bit for bit the existing entry point's for that form.
 *   guided form every output is bit for bit that existing entry point run on the plane p formed by the three operations above.
 *               A NaN of pred_guide under mask <= 0 never reaches a kept pixel (the masked step's selects).
 * The guided kernels are instantiations of their own (the existing entry points launch the kernels they always had) and choose between
 * rows and the scalar clip at run time.
 *
 * gct2_x0_quantile_guided: gct2_x0_quantile with pred_guide (non-NULL) and w: every digit pass forms p by the combine before the
 * estimate, so the select's x is the guided step's x bit for bit.  Same scratch (gct2_x0_quantile_scratch), same finishing rule, integer
 * atomics only, no host synchronisation.
 * Measured on one MI355X at 64x128x128x3, bf16 views: profiles/guidance_bench.json. */
int gct2_x0_quantile_guided(int mode, const float* pred, const float* pred_guide, double w, const float* fake, double a_t, uint32_t rank,
                            double floor, float* rows, float* q_out, void* scratch, size_t scratch_bytes, int B, size_t per_image,
                            void* stream);
int gct2_diffusion_step_guided(int mode, int dtype, const float* pred, const float* pred_guide, double w, const float* fake_in,
                               const float* hist_in, const float* known, const float* mask, const float* rows, double a_t, double a_prev,
                               double sigma2, double c1, double clip, uint64_t seed, uint64_t stream_id, uint64_t offset, uint64_t offset0,
                               uint64_t image_stride, float* fake_out, float* hist_out, float* x0_out, void* out, int ldout, void* out2,
                               int ldout2, void* out3, int ldout3, void* out4, int ldout4, int B, size_t per_image, int C, void* stream);
/* ---- progressive distillation (Salimans & Ho 2022, "Progressive Distillation for Fast Sampling of Diffusion Models"; Distiller):
 * a student learns to do in ONE DDIM step what its teacher does in two.  A batch holds a different timestep per image, so the
 * scalars (a_t, a_prev) of the sampler's entry points become a row of a host-built table per image:
 *   pair   [B] int32, 1-based (what gct2_rng_uniform_int(..., 1, N) draws): image b reads row clamp(pair[b], 1, N) - 1 of both tables,
 *          so no value reads outside them
 *   table  [N][GCT2_DISTILL_ROW] fp32 (trainer_math.distill_table) for the timesteps t > t' > t'' of a pair of teacher steps:
 *            {sa0, sb0, sa1, sb1, sa2, sb2, r, den, cx0, ck0, cx1, ce1}
 *          sa = (float)sqrt(a), sb = (float)sqrt(1 - a) at a = alpha(t), alpha(t'), alpha(t'') (square roots in double, one cast each:
 *          gct2_diffusion_step's sa / sb);  r = (float)(sb2 / sb0), den = (float)(sa2 - (sb2 / sb0) sa0) from the double roots, rounded
 *          once;  cx0 = sqrtf((float)alpha(t)), ck0 = sqrtf(1.f - (float)alpha(t)): gct2_diffusion_start_image's pair at a = alpha(t);
 *          cx1 = sqrtf((float)alpha(t')), ce1 = sqrtf(1.f - (float)alpha(t')): gct2_diffusion_step's re-noising pair at a_prev = alpha(t').
 *          The first pair of a grid has no t'': its end point is alpha = 1, {sa2, sb2, r, den} = {1, 0, 0, 1} (generate returns the last
 *          step's x0 estimate, not a re-noised image).  The caller guarantees sb0 > 0, den > 0 and gct2_diffusion_step's a_t rule.
 *   ttable [N][2] int32 {t, t'}
 * Shapes, views and their GCT2_EINVAL rules are gct2_diffusion_step's: B images of per_image fp32 elements, per_image a multiple of C,
 * ldout >= C, B * per_image < 2^31; also GCT2_EINVAL: a NULL pointer (t_out, t1_out and out2 may be NULL), N < 1, GCT2_SAMPLE_ODE and the
 * reserved code 4.  fp32, every operation rounded once (no fused multiply-add).  No output overlaps an input or another output.
 *
 * gct2_distill_start: gct2_diffusion_start_image with a per-image alpha.  z0_out[i] = cx0 x[i] + ck0 e, e the normal gct2_rng_normal
 *   writes for element offset + b image_stride + i of the stream (seed, stream_id) - or, eps != NULL, e = eps[i] and nothing is drawn
 *   (a pinned batch); z0 once rounded into out / out2;
 *   t_out[b] = t, t1_out[b] = t' of the image's row.  Image by image the bits of gct2_diffusion_start_image(a = alpha(t)).
 * gct2_distill_step: the teacher's first step t -> t'.  Per image gct2_diffusion_step at sigma2 = 0 with (sa0, sb0) as a_t's and
 *   (cx1, ce1) as a_prev's coefficients, the same clip (> 0: x clipped, e re-derived), bit for bit; z1_out and out / out2 are its
 *   fake_out and views.  Nothing else is stored.
 * gct2_distill_target: the teacher's second step t' -> t'' fused with the solve for the student's pseudo pair; z'' never reaches memory.
 *   Element i of image b, p = pred2, f1 = z1, f0 = z0:
 *     (x2, e2)  gct2_diffusion_step's update at (sa1, sb1) and clip, bit for bit
 *     xt = (sb2 == 0) ? x2 : fl( fl( fl(fl(sa2 x2) + fl(sb2 e2)) - fl(r f0) ) / den )
 *     et = fl( fl( f0 - fl(sa0 xt) ) / sb0 )
 *   x_out[i] = xt, eps_out[i] = et: one DDIM step from z0 with the estimate xt lands on the teacher's z'', and a student handed
 *   (xt, et) at timestep t is noised back to z0 up to rounding.  It takes no views and no C.  Four elements per thread with 16-byte
 *   accesses when per_image is a multiple of 4 and the five planes are 16-byte aligned, one element per thread otherwise: same bits.
 * Measured on one MI355X at 64x128x128x3, bf16 views: profiles/distill_bench.json. */
#define GCT2_DISTILL_ROW 12
int gct2_distill_start(int dtype, const float* x, const float* eps, const int32_t* pair, const float* table, const int32_t* ttable, int N, uint64_t seed,
                       uint64_t stream_id, uint64_t offset, uint64_t image_stride, float* z0_out, int32_t* t_out, int32_t* t1_out,
                       void* out, int ldout, void* out2, int ldout2, int B, size_t per_image, int C, void* stream);
int gct2_distill_step(int mode, int dtype, const float* pred, const float* z0, const int32_t* pair, const float* table, int N, double clip,
                      float* z1_out, void* out, int ldout, void* out2, int ldout2, int B, size_t per_image, int C, void* stream);
int gct2_distill_target(int mode, const float* pred2, const float* z1, const float* z0, const int32_t* pair, const float* table, int N,
                        double clip, float* x_out, float* eps_out, int B, size_t per_image, void* stream);
/* the four inputs of the reverse pass built from one inverted noise image eps [H,W,C] (train.py:416-431): out [4,H,W,C] =
 * eps | nearest-upsample x4 of avg_pool2d(eps, 4, 4) | tf.roll by 1 along H and W | per-pixel nearest of the K entries of
 * dictionary [H,W,K,C] (squared distance, first minimum).  H, W multiples of 4. */
int gct2_noise_edits(const float* eps, const float* dictionary, int K, float* out, int H, int W, int C,
                     void* stream);

/* ---- input contract, decode_file without the decoder (train.py:285-293) ------------------------------------------------ */
/* dst[b,y,x,c] = src_b[oy+y, ox + (flip ? size-1-x : x), c] / 128 - 1: random_crop + random_flip_left_right + the cast of
 * train.py:288-292 for a whole batch in one launch.  src: device buffer of decoded RGB images (u8, HWC) back to back;
 * offsets[b]: byte offset of image b; dims[b] = {H0, W0, oy, ox, flip} (int32, the caller draws the crop origin and the flip and
 * guarantees oy + size <= H0, ox + size <= W0); dst: fp32 [B, size, size, 3]. */
int gct2_image_prepare(const uint8_t* src, const int64_t* offsets, const int32_t* dims, float* dst, int B, int size,
                       void* stream);

/* ---- the device-resident image cache (train.py:317 `#.cache("cache")`, kept in HBM): shuffle, crop, flip and the cast of a whole
 * batch in ONE launch that reads no host data.  pool: the decoded RGB images (u8, HWC) of the whole dataset back to back;
 * offsets[i] (int64): byte offset of image i in pool; hw[i] = {H0, W0} (int32); N images.  dst: fp32 [B, size, size, 3],
 *   dst[b,y,x,c] = pool[offsets[item] + ((oy+y) W0 + ox + (flip ? size-1-x : x)) 3 + c] / 128 - 1          (exact in fp32)
 * with (item, oy, ox, flip) of sample b either read from picks_in[b] (int32 [B,4]; nothing is drawn) or, picks_in == NULL, drawn
 * for the running sample index k = first_sample + b * sample_stride (uint64, wraps) - a batch is a function of (seed, k) alone,
 * whatever the batch size.  philox(seed, sid, idx) below is the four words r[0..3] of counter idx on stream sid exactly as
 * gct2_rng_uniform_int defines them; flags is a set of GCT2_DATA_* bits.
 *   item   e = k / N, p = k % N.  Without GCT2_DATA_SHUFFLE item = p.  With it item = pi_e(p), a stateless permutation of [0, N)
 *          per epoch e: N = 1 gives 0; else h = max(1, (bitlen(N-1) + 1) / 2), mask = 2^h - 1, ks = philox(seed, 7, e), round keys
 *          kj = ks[j & 3] + j * 0x9E3779B9 (mod 2^32) for j = 0..7; v = p; one pass is L = v >> h, R = v & mask, eight rounds
 *          (L, R) <- (R, L ^ (fmix32(R ^ kj) & mask)), v = (L << h) | R; the pass is repeated until v < N (cycle walking: the domain
 *          2^(2h) is smaller than 4N); item = v.  fmix32 is murmur3's finaliser: x ^= x >> 16, x *= 0x85EBCA6B, x ^= x >> 13,
 *          x *= 0xC2B2AE35, x ^= x >> 16.
 *   crop   r = philox(seed, 6, k), (H0, W0) = hw[item].  With GCT2_DATA_RANDOM_CROP oy = (r[0] (H0-size+1)) >> 32 and
 *          ox = (r[1] (W0-size+1)) >> 32 (64-bit products); without it the centre crop oy = (H0-size)/2, ox = (W0-size)/2.
 *   flip   with GCT2_DATA_FLIP r[2] >> 31, else 0.
 * picks_out (int32 [B,4] or NULL) receives the (item, oy, ox, flip) that were used.  The kernel cannot refuse at run time: a
 * picks_in row whose item lies outside [0, N) or whose origin lies outside [0, H0-size] x [0, W0-size], and an hw entry smaller than
 * size, are CLAMPED so that no address leaves the image (item into [0, N), the origin into the image, source pixels onto the last row /
 * column), and picks_out[b] holds item = -1 with the clamped origin; a flip other than 0 counts as 1.
 * size % 4 == 0 with a 16-byte aligned dst and a 4-byte aligned pool takes the wide path (four pixels per thread: aligned dword loads
 * around their 12 source bytes, three 16-byte stores); anything else a per-element path with the same bits.  The wide path reads up
 * to 3 bytes past the 12 it needs, so THE POOL CARRIES 16 SPARE BYTES BEHIND ITS LAST IMAGE (readable, any value): the caller
 * guarantees it, as data.py's CachedImageDataset does.
 * GCT2_EINVAL before any launch: a null pool, offsets, hw or dst; B, N or size <= 0, size > 16384; unknown flag bits;
 * sample_stride == 0.  Measured on one MI355X: profiles/image_cache_bench.json. */
#define GCT2_DATA_SHUFFLE 1
#define GCT2_DATA_RANDOM_CROP 2
#define GCT2_DATA_FLIP 4
int gct2_image_batch_cached(const uint8_t* pool, const int64_t* offsets, const int32_t* hw, int N, uint64_t seed,
                            uint64_t first_sample, uint64_t sample_stride, int flags, const int32_t* picks_in, int32_t* picks_out,
                            float* dst, int B, int size, void* stream);

/* ---- samples as pictures (the other end of the pipeline: what train.py:356, 489-496 hand to tf.summary.image): a batch quantised to
 * uint8 and laid out as a grid of cells in ONE launch.  src: compact [n, H, W, 3] of `dtype` (GCT2_F32 | GCT2_BF16 | GCT2_F16; 16-bit
 * values are widened to float32 exactly first).  out: u8 [GH, GW, 3] with
 *   GH = rows H scale + (rows + 1) pad,   GW = cols W scale + (cols + 1) pad.
 * Image i sits in cell (i / cols, i % cols), whose origin is (pad + r (H scale + pad), pad + c (W scale + pad)); pixel (y, x) of a
 * cell is source pixel (y / scale, x / scale): nearest-neighbour integer upscaling.  The padding and the cells i >= n hold fill_rgb
 * (R = bits 0-7, G = 8-15, B = 16-23).  EVERY BYTE OF out IS WRITTEN BY THE ONE LAUNCH: the caller does no memset.  cols = 1,
 * pad = 0, scale = 1 is the plain conversion [n, H, W, 3] -> u8 [n, H, W, 3].
 * Quantisation, fl() one float32 rounding to nearest even:
 *   GCT2_U8_SUMMARY   z = fl(255.5 fl(fl(0.5 x) + 0.5))     x in [-1, 1]: tf.summary.image(x * 0.5 + 0.5), train.py:356, 489-496
 *   GCT2_U8_DATASET   z = fl(fl(128 x) + 128.5)              the exact inverse of the loader's value / 128 - 1 (train.py:292)
 *   GCT2_U8_UNIT      z = fl(255.5 x)                         x already in [0, 1]: masks, weights
 *   q = 0 for a NaN or z < 1,  255 for z >= 255,  (uint8)trunc(z) otherwise.
 * 0.5 x and 128 x are exact or overflow to the same infinity, so fma(0.5, x, 0.5) and fl(fl(0.5 x) + 0.5) are the same float, and so
 * are the two forms of DATASET: the bits do not depend on whether a compiler contracts the multiply-add.  SUMMARY is
 * tf.image.convert_image_dtype(..., uint8, saturate=True) as tf.summary.image applies it to floats - scale by max + 0.5, saturate,
 * truncate; parity with TensorFlow is unpinned (there is none here to compare with), and NaN -> 0 is this library's choice.  DATASET
 * gives q = v for every x = v / 128 - 1, v = 0..255; SUMMARY on the same inputs gives floor(511 v / 512), so 255 -> 254.
 * All indexing into src and out is size_t: n H W 3 and GH GW 3 may both exceed 2^31.  GW % 4 == 0 with a 4-byte aligned out takes the
 * wide path (a thread owns four adjacent output pixels: three dword stores, the sources as 16-byte loads where scale == 1 and the four
 * lie inside one image); anything else a per-pixel path with the same bits.  No strided or ld = 4 sources, no dithering.
 * GCT2_EINVAL before any launch: a null src or out; an unknown dtype or mode; n, H, W, cols or rows <= 0; cols rows < n; scale outside
 * 1..16; pad outside 0..64; H or W above 16384; fill_rgb with a non-zero top byte; GH or GW above 2^31 - 1; a work-group count above
 * 2^31 - 1.  Measured on one MI355X: profiles/image_out_bench.json. */
#define GCT2_U8_SUMMARY 0   /* tf.summary.image(x * 0.5 + 0.5): train.py:356, 489-496 */
#define GCT2_U8_DATASET 1   /* exact inverse of the loader's value/128 - 1 (train.py:292) */
#define GCT2_U8_UNIT    2   /* input already in [0,1]: masks, weights */
int gct2_image_grid_u8(const void* src, int dtype, int n, int H, int W, int mode, int cols, int rows, int pad, int scale,
                       uint32_t fill_rgb, uint8_t* out, void* stream);

/* loss = mean((target - pred)^2) in fp32 (train.py:272); dpred = loss_scale * 2 (pred-target)/n.
 * `loss` (1 float) is overwritten; `partials` is caller scratch of >= 1024 floats.
 * loss_scale_ptr: device pointer to the current loss scale (fp16 mode) or NULL for 1. */
int gct2_mse_fwd_bwd(const float* pred, const float* target, float* dpred, float* loss,
                     float* partials, size_t n, const float* loss_scale_ptr, void* stream);

/* ---- the other training losses Trainer.call carries (train.py:254-280; the author switches between them by moving a `return`) ----
 * One entry point for the four ways the reference turns target - pred into the scalar Keras minimises.  pred, target, dpred: fp32
 * [B,H,W,C] contiguous, C in 1..4; n = B*H*W*C; d = fl32(target - pred); s = *loss_scale_ptr, or 1 when it is NULL (as in
 * gct2_mse_fwd_bwd).  dpred == NULL: the loss only (Trainer.call without gradients) - nothing but `loss` and `scratch` is written.
 * Host constants are formed in double and rounded once to fp32; the pointwise arithmetic is fp32, every operation rounded on its own
 * (no contraction); no floating-point atomics: work-groups leave partial sums (fp64) in `scratch`, one launch adds them in index
 * order, and loss = (float) of a double expression of the sums - the bits depend on the inputs alone.
 *   GCT2_LOSS_MSE         exactly gct2_mse_fwd_bwd's launches and bits, with the first 1024 floats of scratch as its `partials`.
 *   GCT2_LOSS_L1          loss = S / n, S = sum max(d, -d);  dpred = fl(s * (d >= -d ? -c : c)), c = (float)(1.0 / n).  A tie sends
 *                         the gradient to the first operand of the reference's maximum(t - p, p - t) and a NaN to the second: TF's
 *                         _MaximumGrad (x >= y) [TF]; PARITY UNPINNED like the other [TF] rules.
 *   GCT2_LOSS_MSE_POOLED  H and W multiples of 16 (avg_pool2d(16, 16, 'SAME') then pads nothing; anything else: GCT2_EINVAL).  qsum =
 *                         the sum of d over a pixel's 16 x 16 cell and channel, n2 = B*(H/16)*(W/16)*C:
 *                         loss = S1 / n + S2 / n2, S1 = sum d^2, S2 = sum over cells and channels of (qsum / 256)^2;
 *                         dpred = fl(s * fl(fl(d * c1) + fl(qsum * c2))), c1 = (float)(-2.0 / n), c2 = (float)(-2.0 / (65536.0 * n2)).
 *                         The reference pools target and pred separately and subtracts the pools; pooling d differs from that only
 *                         in rounding.
 *   GCT2_LOSS_DCT         H == W == size, a multiple of 4.  basis = G, fp32 [size,size] row-major, supplied by the caller (the library
 *                         never evaluates a cosine).  Per image and channel, D = d[b,:,:,c]:  E = G D G^T,  loss = (sum E^2) / n,
 *                         dpred[b,:,:,c] = fl(s * fl(V * c1)),  V = G^T E G,  c1 = (float)(-2.0 / n).  Four fp32 matrix products per
 *                         plane on the fp32 matrix cores (each an fmaf chain over ascending reduction index), hopping
 *                         d -> scratch -> dpred -> scratch -> dpred.  The reference's G (trainer_math.dct_basis) is
 *                         tf.signal.dct(norm='ortho') times frequency_weights: G[k,m] = 1/(k+1) * sigma_k * cos(pi (2m+1) k / (2 size)),
 *                         sigma_0 = sqrt(1/size), else sqrt(2/size); dct2d leaves its result spatially transposed, which the mean
 *                         does not see.
 * scratch: device floats, 16-byte aligned, at least what gct2_loss_scratch reports for the kind and shape (the partial sums; for the
 * DCT also one [B,H,W,C] plane set).  GCT2_EINVAL before any launch: unknown kind, non-positive dims or C outside 1..4, the shape
 * rules above, NULL pred / target / loss / scratch, basis == NULL for the DCT, misaligned pointers (scratch and basis 16 bytes, the
 * rest 4), scratch_floats below gct2_loss_scratch's figure. */
#define GCT2_LOSS_MSE 0          /* train.py:272 */
#define GCT2_LOSS_L1 1           /* train.py:268-270 */
#define GCT2_LOSS_MSE_POOLED 2   /* train.py:274-280 */
#define GCT2_LOSS_DCT 3          /* train.py:254-260, 265 */
/* host only, no launch: floats of device scratch gct2_loss_fwd_bwd needs for this kind and shape */
int gct2_loss_scratch(int kind, int B, int H, int W, int C, size_t* floats);
int gct2_loss_fwd_bwd(int kind, const float* pred, const float* target, float* dpred, float* loss,
                      float* scratch, size_t scratch_floats, int B, int H, int W, int C,
                      const float* basis, const float* loss_scale_ptr, void* stream);

/* ---- evaluation (Keras Model.evaluate / fit(validation_data=...) on the reference's test/ folder): the training loss PER IMAGE ----
 * rows[b] = the loss of `kind` (the GCT2_LOSS_* codes above) over image b alone; in exact arithmetic the mean of rows over the batch
 * is gct2_loss_fwd_bwd's loss on the same batch.  The objective's target and the prediction weight are formed on load and never
 * stored.  pred, x, eps: fp32 [B,H,W,C] contiguous, C in 1..4, all three read only; a, c, w: device float[B] or NULL; rows: float[B].
 * Per element, every operation rounded once (no fused multiply-add), by the rule of gct2_mix_per_image:
 *   target = x                                 (a == NULL)
 *          = fl(a[b] * x)                      (a given, eps == NULL)
 *          = fl(fl(a[b] * x) + fl(c[b] * eps)) (a and eps given; c is then required, and c without eps is GCT2_EINVAL)
 *   p = w ? fl(w[b] * pred) : pred;   d = fl(target - p).
 * With n_img = H*W*C and S the sum over image b in fp64:
 *   GCT2_LOSS_MSE         rows[b] = (float)(S((double)d * (double)d) / n_img)
 *   GCT2_LOSS_L1          rows[b] = (float)(S(max(d, -d)) / n_img)
 *   GCT2_LOSS_MSE_POOLED  rows[b] = (float)(S(d^2) / n_img + S((qsum / 256)^2) / n2_img), qsum = the fp64 sum of d over a 16 x 16 cell
 *                         and channel, n2_img = (H/16)(W/16)C; H and W multiples of 16
 *   GCT2_LOSS_DCT         E = G D G^T per plane by the two fp32 matrix-core passes gct2_loss_fwd_bwd runs first (d is written to
 *                         scratch for them), rows[b] = (float)(S((double)E * (double)E) / n_img); shape and basis rules as there
 * No atomics; a work-group never mixes two images; work-groups leave fp64 partial sums in scratch and one finishing launch adds them
 * per image in index order: the bits depend on the inputs alone.  Images need not start at 16-byte boundaries (n_img = 105).
 * scratch: device floats, 16-byte aligned, at least what gct2_eval_loss_scratch reports (host only, no launch).
 * GCT2_EINVAL before any launch: unknown kind; NULL pred / x / rows / scratch; non-positive dims or C outside 1..4; the per-kind shape
 * rules; c without eps, or a and eps without c; a NULL or misaligned basis for the DCT; pointers not 4-byte aligned, scratch not 16-byte
 * aligned; scratch_floats below the query's figure; B > 65535; B*n_img at or beyond 2^31. */
int gct2_eval_loss_scratch(int kind, int B, int H, int W, int C, size_t* floats);
int gct2_eval_loss_rows(int kind, const float* pred, const float* x, const float* eps, const float* a, const float* c,
                        const float* w, float* rows, float* scratch, size_t scratch_floats, int B, int H, int W, int C,
                        const float* basis, void* stream);

/* ---- the training loss of an objective with per-image (per-timestep) weights, forward and backward in ONE pass ----------------------
 * configure(loss_weighting=...) (min-SNR-gamma, Hang et al. 2023, "Efficient Diffusion Training via Min-SNR Weighting Strategy", a table
 * or a callable): L = (1/B) sum_b lam[b] l_b with l_b the per-image loss of `kind`; not renormalised by sum(lam).  The objective's target
 * is formed on load by gct2_eval_loss_rows' rule and never stored, so the step needs no target plane:
 *   target = x | fl(a[b] * x) | fl(fl(a[b] * x) + fl(c[b] * eps));   p = w ? fl(w[b] * pred) : pred;   d = fl(target - p).
 * pred, x, eps: fp32 [B,H,W,C] contiguous, C in 1..4, read only; a, c, w, lam: device float[B] or NULL (lam NULL: lambda = 1);
 * dpred: fp32 [B,H,W,C] or NULL (the loss only: nothing but loss and scratch is written); it must not alias pred, x or eps.
 * With n_img = H*W*C, n = B n_img, s = *loss_scale_ptr (1 when NULL), S_b the fp64 sum over image b, and g_b = fl(lam[b] * w[b]) when
 * both are given, lam[b] or w[b] when one is, absent (no multiply) when both are NULL; fp32, every operation rounded once:
 *   GCT2_LOSS_MSE  loss = (float)(sum_b (double)lam[b] * S_b((double)d * (double)d) / n)
 *                  dpred = fl(s * fl(fl(d * k) * g_b)),  k = (float)(-2.0 / n)
 *   GCT2_LOSS_L1   loss = (float)(sum_b (double)lam[b] * S_b(max(d, -d)) / n)
 *                  dpred = fl(s * fl((d >= -d ? -k1 : k1) * g_b)),  k1 = (float)(1.0 / n)   (the tie and NaN rule of GCT2_LOSS_L1)
 * loss is never multiplied by s.  No atomics; a work-group never mixes two images; work-groups leave fp64 partial sums in scratch and one
 * finishing launch adds them in index order (per image, then over the images): the bits depend on the inputs alone.  Images need not
 * start at 16-byte boundaries (n_img = 105).  scratch: device floats, 16-byte aligned, at least what gct2_objective_loss_scratch reports
 * (host only, no launch).
 * GCT2_EINVAL before any launch: kinds other than MSE / L1; NULL pred / x / loss / scratch; c without eps, or a and eps without c;
 * non-positive dims or C outside 1..4; pointers not 4-byte aligned, scratch not 16-byte aligned; scratch_floats below the query's figure;
 * B > 65535; n at or beyond 2^31; dpred equal to pred, x or eps.  Measured on one MI355X at 64x128x128x3:
 * profiles/objective_loss_bench.json. */
int gct2_objective_loss_scratch(int kind, int B, int H, int W, int C, size_t* floats);
int gct2_objective_loss_fwd_bwd(int kind, const float* pred, const float* x, const float* eps, const float* a, const float* c,
                                const float* w, const float* lam, float* dpred, float* loss, float* scratch, size_t scratch_floats,
                                int B, int H, int W, int C, const float* loss_scale_ptr, void* stream);

/* ---- image metrics of evaluation (Keras compile(metrics=[...]); tf.image.psnr / tf.image.ssim [TF]): PER IMAGE, in image space ----
 * The x0 estimate e of image b against the clean image x: mse[b], psnr[b] and ssim[b] (Wang et al. 2004 with the defaults of
 * tf.image.ssim; parity unpinned, there is no TensorFlow here).  pred, noised, x: fp32 [B,H,W,C] contiguous, C in 1..4, all three
 * read only; u, v: device float[B] or NULL; window: device float[K], K in 1..16, the 1-D filter taps (the host passes the table:
 * trainer_math.ssim_window; nothing evaluates a Gaussian on the device); mse, psnr, ssim: float[B]; psnr and / or ssim may be NULL,
 * and a NULL ssim skips the windowed pass entirely (window may then be NULL too).
 * Per element, every operation rounded once (no fused multiply-add), by the rule of gct2_mix_per_image:
 *   e = pred                                    (u == NULL; noised and v must then be NULL too)
 *     = fl(fl(u[b] * noised) + fl(v[b] * pred)) (u given; noised and v are then required)
 *   d = fl(x - e).
 * With n_img = H*W*C and S the sum over image b in fp64:
 *   m = S((double)d * (double)d) / n_img,  mse[b] = (float)m   (the MSE row of gct2_eval_loss_rows)
 *   psnr[b] = (float)(10 * log10((double)max_val * max_val / m)) in fp64, +inf when m == 0
 * SSIM, everything in fp64: a = (double)e, b = (double)x, w = (double)window[.],
 *   F(q)[i,j,c] = sum_r sum_s w[r] w[s] q[i+r, j+s, c]   for i in [0, H-K], j in [0, W-K]   (VALID: nothing outside the image is read;
 *   evaluated separably, rows then columns),
 *   mu_a = F(a), mu_b = F(b), A = F(a a), Bq = F(b b), AB = F(a b)  (a product of two floats is exact in fp64: only the sums round),
 *   C1 = (k1 max_val)^2, C2 = (k2 max_val)^2,
 *   lum = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1),
 *   cs  = (2 AB - 2 mu_a mu_b + C2) / (A + Bq - (mu_a^2 + mu_b^2) + C2),
 *   ssim[b] = (float)(the mean of lum * cs over all (H-K+1)(W-K+1)C positions and channels).
 * Identical images give mse 0, psnr +inf and ssim exactly 1.
 * One work-group per image, GCT2_METRICS_TILE x GCT2_METRICS_TILE tile of pixels and channel.  The tiles cut the image, so d^2 counts
 * every element once although the staged regions overlap, and the cut depends on neither K nor ssim: mse and psnr have the same bits
 * with and without SSIM.  No atomics; a work-group never mixes two images; work-groups leave fp64 partial sums in scratch and one
 * finishing launch adds them per image in index order: the bits depend on the inputs alone.  Images need not start at 16-byte
 * boundaries (n_img = 121).
 * scratch: device floats, 16-byte aligned, at least what gct2_image_metrics_scratch reports (host only, no launch; K is checked,
 * the figure does not depend on it).
 * GCT2_EINVAL before any launch, in this order: NULL pred / x / mse / scratch; u without noised or v, or either of those without u;
 * ssim without window; non-positive dims, C outside 1..4, K outside 1..16; H < K or W < K when ssim is given; max_val not finite
 * or <= 0, k1 or k2 negative or not finite; pointers not 4-byte aligned, scratch not 16-byte aligned; B > 65535; B*n_img at or
 * beyond 2^31; scratch_floats below the query's figure. */
#define GCT2_METRICS_TILE 32
int gct2_image_metrics_scratch(int B, int H, int W, int C, int K, size_t* floats);
int gct2_image_metrics(const float* pred, const float* noised, const float* u, const float* v, const float* x,
                       const float* window, int K, float max_val, float k1, float k2,
                       float* mse, float* psnr, float* ssim,
                       float* scratch, size_t scratch_floats, int B, int H, int W, int C, void* stream);

/* ---- mixed precision (train.py:34,43-45,82-83) ------------------------------------------------ */
/* device-resident state of Keras' LossScaleOptimizer [TF] plus the optimizer step counter it gates: a skipped step (inf/nan
 * gradients) does not run the inner apply_gradients, so optimizer.iterations - and with it the WarmUp step and Adam's bias
 * correction - only advance on APPLIED steps.  32 bytes, 16-byte aligned. */
typedef struct {
  float scale; float inv_scale; int32_t good_steps; int32_t found_inf;
  int32_t applied_steps;   /* optimizer.iterations */
  float alpha;             /* lr(applied_steps) * sqrt(1-b2^t)/(1-b1^t), t = applied_steps+1: written by loss_scale_begin; the plain lr(applied_steps) for SGD / RMSprop (loss_scale_begin_schedule) */
  int32_t reserved[2];
} gct2_loss_scale_state;
int gct2_loss_scale_init(gct2_loss_scale_state* state, float initial_scale, void* stream);
/* start of a step: found_inf = 0 and alpha for THIS step from the WarmUp schedule (train.py:57-65: float32
 * base * (step+1) / (warmup_steps+1) while step < warmup_steps, else base) and Adam's bias correction. */
int gct2_loss_scale_begin(gct2_loss_scale_state* state, float base_lr, int warmup_steps, float beta1, float beta2,
                          void* stream);
/* found_inf |= any(!isfinite(g)) */
int gct2_scale_check_finite(const float* g, size_t n, gct2_loss_scale_state* state, void* stream);
/* dynamic update [TF]: finite -> applied_steps++, good_steps++, scale x2 every growth_interval; non-finite -> scale /2, reset. */
int gct2_loss_scale_update(gct2_loss_scale_state* state, int growth_interval, void* stream);

/* ---- optimizer   train.py:50-65, 75 (Keras Adam + WarmUp) ------------------------------------ */
/* Keras ResourceApplyAdam over a flat fp32 arena of n parameters:
 *   g' = g * grad_mul * (ls ? ls->inv_scale : 1);  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;
 *   p -= alpha * m / (sqrt(v) + eps),  alpha = lr_k * sqrt(1-b2^t)/(1-b1^t) computed by the host (lr_k from the WarmUp
 *   schedule) - or, with ls != NULL, taken from ls->alpha (the device-side step counter decides) and the whole update is
 *   skipped when ls->found_inf != 0 (LossScaleOptimizer, train.py:82-83).
 *   grad_mul: host scalar (1/world_size turns the all-reduced SUM into the data-parallel mean).
 *   shadow (may be NULL): low-precision copy of p in `shadow_dtype` written in the same pass.
 *   zero_grad != 0: g is zeroed after use (for callers that accumulate gradients; the engine never needs it). */
int gct2_adam_keras_multi(float* p, float* m, float* v, float* g, void* shadow, int shadow_dtype,
                          size_t n, float alpha, float beta1, float beta2, float eps, float grad_mul,
                          const gct2_loss_scale_state* ls, int zero_grad, void* stream);

/* Keras' optimizer EMA [TF] (Adam(use_ema=True, ema_momentum=...)): average = momentum * average + (1 - momentum) * var,
 * elementwise, fp32: new = fl(fl(momentum * ema) + fl(one_minus * p)), two products and one sum, no contraction.
 * ema, p: fp32 [n], 16-byte aligned.
 * ema_shadow (may be NULL): copy of the NEW ema in shadow_dtype (GCT2_BF16 / GCT2_F16), 8-byte aligned, written in the same pass
 *   (round to nearest even, overflow to +-inf: the bits gct2_cast_from_f32 writes).
 * one_minus: the host forms 1 - momentum in double and rounds once, as Python does in the reference stack.
 * ls (may be NULL): when ls->found_inf != 0 NOTHING is written (a skipped LossScaleOptimizer step leaves the averages alone).
 * GCT2_EINVAL before any launch: NULL ema / p, n == 0, misaligned pointers, a shadow with shadow_dtype GCT2_F32 or unknown,
 * momentum outside [0, 1] or not finite. */
int gct2_ema_update(float* ema, const float* p, void* ema_shadow, int shadow_dtype, size_t n, float momentum, float one_minus,
                    const gct2_loss_scale_state* ls, void* stream);

/* ---- gradient clipping [TF]: Keras' optimizer arguments clipvalue / clipnorm / global_clipnorm (opt-in; train.py uses none) ----
 * GCT2_CLIP_VALUE clips every element, GCT2_CLIP_NORM every variable to an L2 norm (tf.clip_by_norm), GCT2_CLIP_GLOBAL_NORM all
 * variables together (tf.clip_by_global_norm).  The two norm modes read a sum of squares that gct2_grad_sumsq leaves on the device. */
#define GCT2_CLIP_NONE 0
#define GCT2_CLIP_VALUE 1
#define GCT2_CLIP_NORM 2
#define GCT2_CLIP_GLOBAL_NORM 3
#define GCT2_SUMSQ_CHUNK 32768           /* elements one fp64 partial covers (one work-group of stage one; a multiple of 4) */
#define GCT2_SUMSQ_MAX_SEGMENTS 1024     /* largest nseg of gct2_sumsq_layout / gct2_grad_sumsq */
/* one variable inside the fp32 gradient arena: elements [begin, begin + count), its partials at [first_partial, first_partial +
 * ceil(count / GCT2_SUMSQ_CHUNK)) */
typedef struct { uint64_t begin, count, first_partial; } gct2_sumsq_seg;

/* host only, no launch: checks the segments, then fills out[nseg] and *npartials (the length of gct2_grad_sumsq's `partials`).
 * Each segment gets ceil(count / GCT2_SUMSQ_CHUNK) partials; first_partial is the running prefix.
 * GCT2_EINVAL, nothing filled: a NULL pointer, nseg outside [1, GCT2_SUMSQ_MAX_SEGMENTS], count == 0, begin % 4 != 0 (a chunk is
 * read with 16-byte loads), segments not in ascending order or overlapping. */
int gct2_sumsq_layout(const uint64_t* begin, const uint64_t* count, int nseg, gct2_sumsq_seg* out, size_t* npartials);

/* sumsq[s] = sum over segment s of (double)g'^2 for s < nseg, sumsq[nseg] = sumsq[0] + ... + sumsq[nseg-1] in segment order, where
 *   k = fl32((ls ? ls->inv_scale : 1) * grad_mul),  g' = fl32(g * k)   - the g' of gct2_adam_keras_multi.
 * The square (exact: an fp32 value squared fits fp64) and every addition are fp64.  Stage one (one launch, npartials work-groups of
 * 256 threads) leaves one partial per chunk - a chunk never straddles a segment, and elements outside every segment are never read
 * (padding and neighbouring buffers may hold NaN); stage two (one work-group) adds a segment's partials in index order and the
 * segments in segment order.  No floating-point atomics: the bits depend on the input alone, not on the order work-groups arrive in
 * or on the stream.
 * g: fp32, 16-byte aligned; segs: device copy of gct2_sumsq_layout's out[nseg]; partials: device [npartials]; sumsq: device
 * [nseg + 1]; all three 8-byte aligned.
 * ls (may be NULL): ls->found_inf |= any(!isfinite(RAW g inside a segment)) - the flag gct2_scale_check_finite sets, so a
 *   norm-clipped loss-scaled step needs no separate pass over the gradients.
 * GCT2_EINVAL before any launch: NULL g / segs / partials / sumsq, nseg outside [1, GCT2_SUMSQ_MAX_SEGMENTS], npartials == 0 or
 * < nseg, misaligned pointers. */
int gct2_grad_sumsq(const float* g, const gct2_sumsq_seg* segs, int nseg, size_t npartials, float grad_mul, gct2_loss_scale_state* ls,
                    double* partials, double* sumsq, void* stream);

/* gct2_adam_keras_multi (zero_grad = 0; same geometry, shadow write, ls skip and ls->alpha) with one step between g' and the update,
 * fp32, no contraction:
 *   GCT2_CLIP_NONE:        g'' = g'                                  (the bits of gct2_adam_keras_multi)
 *   GCT2_CLIP_VALUE:       g'' = min(max(g', -clip), clip)           (a NaN stays NaN, as TF's minimum / maximum)
 *   GCT2_CLIP_NORM:        l2 = *sumsq > 0 ? (float)sqrt(*sumsq) : 1;  g'' = fl(fl(g' * clip) / max(l2, clip))
 *   GCT2_CLIP_GLOBAL_NORM: nrm = (float)sqrt(*sumsq);  scale = isfinite(nrm) ? fl(clip * min(1 / nrm, 1 / clip)) : NaN;
 *                          g'' = fl(g' * scale)   (as in TF, a scale that is not exactly 1 below the threshold is accepted)
 * sqrt is the double one, rounded once to fp32.  sumsq: ONE fp64 value on the device (gct2_grad_sumsq's sumsq + s for a variable,
 * sumsq + nseg for the global norm), 8-byte aligned; NULL for NONE / VALUE.  shadow (may be NULL): GCT2_BF16 / GCT2_F16 copy of p.
 * GCT2_EINVAL before any launch: NULL p / m / v / g, n == 0, misaligned pointers, a shadow with shadow_dtype GCT2_F32 or unknown,
 * unknown clip_mode, clip not finite or <= 0 in a clipping mode, a norm mode with sumsq == NULL. */
int gct2_adam_keras_clipped(float* p, float* m, float* v, float* g, void* shadow, int shadow_dtype, size_t n,
                            float alpha, float beta1, float beta2, float eps, float grad_mul,
                            const gct2_loss_scale_state* ls, int clip_mode, float clip, const double* sumsq, void* stream);

/* ---- Keras SGD and RMSprop [TF] (train.py:67-78, the optimizer lines the reference keeps commented out) ----------------------
 * One entry point over a flat arena range, beside gct2_adam_keras_clipped and with its geometry, shadow write, ls skip and clipping
 * step: g' = fl(g * fl((ls ? ls->inv_scale : 1) * grad_mul)), g'' = the clipped g' exactly as gct2_adam_keras_clipped forms it, and
 * lr = ls ? ls->alpha : lr.  Then, all in fp32, every operation rounded once, no contraction:
 *   GCT2_OPT_SGD, momentum == 0:      p = p - fl(lr * g'')
 *   GCT2_OPT_SGD, momentum > 0:       m = fl(fl(momentum * m) - fl(lr * g''))           (Keras ApplyKerasMomentum, m = the velocity)
 *                 nesterov == 0:      p = p + m
 *                 nesterov != 0:      p = p + fl(fl(momentum * m) - fl(lr * g''))       (with the NEW m)
 *   GCT2_OPT_RMSPROP:                 v = fl(fl(rho * v) + fl(fl(1 - rho) * fl(g'' * g'')))
 *                 momentum == 0:      p = p - fl(fl(lr * g'') / fl(fl(sqrt(v)) + epsilon))            (epsilon outside the root)
 *                 momentum > 0:       m = fl(fl(momentum * m) + fl(fl(lr * g'') / fl(sqrt(fl(v + epsilon)))));  p = p - m
 *                                                                                       (the fused ApplyRMSProp: epsilon inside the root)
 * These are the formulas of tf.keras optimizer_v2 (the TF 2.4 - 2.6 era) [TF]; PARITY UNPINNED, like Adam's epsilon placement.
 * A slot that a kind does not use is neither read nor written and may be NULL: m for momentum == 0, v for GCT2_OPT_SGD.  That is
 * what the entry point is for: plain SGD moves 14 - 16 bytes per parameter where Adam moves 30.
 * ls->found_inf != 0: NOTHING is written.  shadow (may be NULL): GCT2_BF16 / GCT2_F16 copy of the new p.  sumsq as for
 * gct2_adam_keras_clipped.  RMSprop's centered variant needs a third slot and is not built.
 * GCT2_EINVAL before any launch: unknown kind (GCT2_OPT_ADAM included: Adam stays where it is), NULL p / g or a NULL slot the kind
 * uses, n == 0, misaligned pointers, a shadow with shadow_dtype GCT2_F32 or unknown, momentum or rho outside [0, 1], epsilon < 0,
 * and the clipping checks of gct2_adam_keras_clipped. */
#define GCT2_OPT_ADAM 0
#define GCT2_OPT_SGD 1
#define GCT2_OPT_RMSPROP 2
int gct2_optimizer_apply(int kind, float* p, float* m, float* v, float* g, void* shadow, int shadow_dtype, size_t n,
                         float lr, float momentum, int nesterov, float rho, float epsilon, float grad_mul,
                         const gct2_loss_scale_state* ls, int clip_mode, float clip, const double* sumsq, void* stream);

/* ---- L2 weight regularizer and gradient transformer [TF] (train.py:47-48, 71-74, 80: SGD(..., gradient_transformers=[sign_gradient])
 * and regularizer = tf.keras.regularizers.l2(1e-6), both commented out there) -------------------------------------------------------
 * Both sit between the raw gradient and the kind's update, where the clipping step sits.  All fp32, every operation rounded once, no
 * contraction; g' = fl(g * fl((ls ? ls->inv_scale : 1) * grad_mul)) as everywhere:
 *   1. penalty gradient (Keras adds l2 * sum(w^2) to the loss, so autodiff adds 2 l2 w):  c = (float)(2.0 * (double)(float)l2) formed by
 *      the host,  g_r = fl(g' + fl(c * p))  with p the parameter BEFORE this step's update.  c == 0: the add is skipped, not computed -
 *      the bits are those of the unregularized kernels, the sign of a zero and a non-finite p included.
 *   2. clipping of g_r exactly as gct2_adam_keras_clipped clips g' (for the norm modes *sumsq is the sum of squares of g_r:
 *      gct2_grad_sumsq_l2).
 *   3. transformer (Keras' _transform_gradients clips first, then runs gradient_transformers [TF]):
 *      GCT2_GRAD_SIGN: x > 0 ? 1 : x < 0 ? -1 : x == 0 ? +0.0f : x   (tf.sign: a NaN stays NaN, -0.0 gives +0.0)
 *   4. the kind's update, unchanged: GCT2_OPT_ADAM as gct2_adam_keras_clipped (lr = alpha, momentum = beta1, rho = beta2, epsilon;
 *      nesterov ignored; both slots in use), GCT2_OPT_SGD / GCT2_OPT_RMSPROP as gct2_optimizer_apply.
 * Geometry, streaming accesses, shadow write, ls skip (found_inf comes from the raw g alone: nothing here sets it) and ls->alpha as
 * gct2_optimizer_apply; a slot a kind does not use is neither read nor written and may be NULL.  The gradient arena is never written:
 * it keeps holding the data-term gradient.  PARITY UNPINNED w.r.t. TensorFlow.
 * GCT2_EINVAL before any launch: the checks of gct2_optimizer_apply (kind may also be GCT2_OPT_ADAM, then m and v are required and
 * momentum / rho are the unchecked betas), unknown transform, l2_coeff not finite or < 0. */
#define GCT2_GRAD_NONE 0
#define GCT2_GRAD_SIGN 1
int gct2_optimizer_apply_reg(int kind, float* p, float* m, float* v, float* g, void* shadow, int shadow_dtype, size_t n,
                             float lr, float momentum, int nesterov, float rho, float epsilon, float grad_mul,
                             const gct2_loss_scale_state* ls, int clip_mode, float clip, const double* sumsq,
                             float l2_coeff, int transform, void* stream);

/* gct2_grad_sumsq over the regularized gradient: the element squared and summed in segment s is
 *   x = fl(fl(g * k) + fl(seg_coeff[s] * p)),   k as for gct2_grad_sumsq,
 * the g_r of gct2_optimizer_apply_reg with l2_coeff = seg_coeff[s].  seg_coeff: device float[nseg], 4-byte aligned; an entry of 0 skips
 * the add (and the read of p) for that segment - such a segment's sum is gct2_grad_sumsq's, which is how tensors without a regularizer
 * (Residual's bias-free projection, train.py:107) are kept out.  p: fp32, 16-byte aligned, laid out like g (segs index both).  The same
 * two stages, the same fixed fp64 order, no floating-point atomics, nothing outside a segment is read in g or p;
 * ls->found_inf |= any(!isfinite(RAW g)) - a large or non-finite p does not set it.
 * GCT2_EINVAL before any launch: as gct2_grad_sumsq, plus NULL or misaligned p / seg_coeff. */
int gct2_grad_sumsq_l2(const float* g, const float* p, const gct2_sumsq_seg* segs, const float* seg_coeff, int nseg, size_t npartials,
                       float grad_mul, gct2_loss_scale_state* ls, double* partials, double* sumsq, void* stream);

/* what Keras' train_step reports with a regularizer, loss + sum of the regularization losses:
 *   *penalty_out = (float)((double)l2 * *S),   *total_out = (float)((double)*loss + (double)l2 * *S)
 * S: ONE fp64 value on the device, the sum of (double)p^2 over the regularized tensors - gct2_grad_sumsq pointed at the parameter arena
 * with grad_mul = 1 and ls = NULL leaves it in sumsq[nseg].  l2: the regularizer's float32 coefficient (not doubled).  loss: fp32 [1],
 * read only; penalty_out, total_out: fp32 [1] each.  One thread; the product and the sum in fp64, each result rounded once to fp32.
 * GCT2_EINVAL before any launch: a NULL or misaligned pointer (S 8-byte, the others 4-byte), l2 not finite or < 0. */
int gct2_l2_penalty(const float* loss, const double* S, float l2, float* penalty_out, float* total_out, void* stream);

/* gct2_loss_scale_begin for any schedule and optimizer: found_inf = 0 and state->alpha = the step size of THIS step at
 * k = state->applied_steps, in float32 and in Keras' order:
 *   GCT2_SCHEDULE_WARMUP (train.py:57-65):   lr = k < steps ? fl(fl(initial * (k + 1)) / (steps + 1)) : initial
 *                                            (steps = warmup_steps, a whole number; decay_rate and staircase are ignored)
 *   GCT2_SCHEDULE_INVERSE_TIME_DECAY [TF]:   q = fl((float)k / steps);  staircase: q = floorf(q);
 *                                            lr = fl(initial / fl(1 + fl(decay_rate * q)))           (steps = decay_steps > 0)
 * bias_correction != 0 (Adam): alpha = (float)(lr * sqrt(1 - beta2^t) / (1 - beta1^t)), t = k + 1, as gct2_loss_scale_begin;
 * bias_correction == 0 (SGD, RMSprop): alpha = lr exactly, beta1 / beta2 are ignored.  No other field of the state is written. */
#define GCT2_SCHEDULE_WARMUP 0
#define GCT2_SCHEDULE_INVERSE_TIME_DECAY 1
int gct2_loss_scale_begin_schedule(gct2_loss_scale_state* state, int schedule, float initial, float steps, float decay_rate,
                                   int staircase, int bias_correction, float beta1, float beta2, void* stream);

/* fp32 -> dtype cast of a flat array (initial weight shadows). */
int gct2_cast_from_f32(int dtype, const float* src, void* dst, size_t n, void* stream);

/* ---- step plans (ABI v15): Keras `fit` (train.py:516) runs one compiled train function per step; this is its counterpart ----
 * A plan is a host-side list of records - calls of the entry points above, event records, stream waits - built once and replayed
 * by ONE call per step (or per segment of a step, where the caller interleaves work of its own: the data-parallel exchange
 * hooks).  A replayed record is exactly the call it records: same entry point, same arguments, same stream - same kernels, same
 * bits.  Arguments are passed as one 64-bit slot each: pointers and 64-bit integers as they are, `int` sign-extended, `float` as
 * its bit pattern in the low 32 bits, `double` as its bit pattern.  Values that change from step to step (the input batch, RNG
 * offsets, the optimizer's alpha) are re-set with gct2_plan_set_arg before a run; structs passed by pointer (gct2_adam_args) are
 * read at run time, so the caller may update them in place.  A plan belongs to ONE host thread at a time, like the ctx objects its
 * records name; it creates one HIP event per event record (no timing, device-scope release) and destroys them with the plan.
 * Plannable entry points: every function of this header that takes a stream, plus gct2_ctx_set_relu_bits. */
typedef struct gct2_plan gct2_plan;
int gct2_plan_create(gct2_plan** plan);
int gct2_plan_destroy(gct2_plan* plan);
/* appends a call of entry point `name` ("gct2_conv4s2_fwd", ...); nargs must equal the entry point's parameter count; *index (may
 * be NULL) receives the record's position */
int gct2_plan_add_call(gct2_plan* plan, const char* name, const uint64_t* args, int nargs, int* index);
/* appends "record a new event on `stream`" / "make `stream` wait for event `event`" (an earlier add_record of this plan) */
int gct2_plan_add_record(gct2_plan* plan, void* stream, int* event);
int gct2_plan_add_wait(gct2_plan* plan, void* stream, int event);
/* ABI v17: the same record with a chosen event kind.  GCT2_EVENT_DEVICE = gct2_plan_add_record (no timing, device-scope release:
 * ordering between streams of one device); GCT2_EVENT_SYSTEM: no timing, system-scope release - for a record whose waiter hands
 * the data to ANOTHER device (the stream a collective of the data-parallel exchange is issued on); GCT2_EVENT_TIMED: a timing
 * event.  gct2_plan_elapsed: milliseconds between two TIMED records of the last run, both completed (the caller synchronised) -
 * how bench.py brackets every layer call of a replayed step without a host round trip between the event and the launch. */
enum { GCT2_EVENT_DEVICE = 0, GCT2_EVENT_SYSTEM = 1, GCT2_EVENT_TIMED = 2 };
int gct2_plan_add_record_kind(gct2_plan* plan, void* stream, int kind, int* event);
int gct2_plan_elapsed(gct2_plan* plan, int start_event, int end_event, float* ms);
int gct2_plan_size(const gct2_plan* plan, int* records);
int gct2_plan_set_arg(gct2_plan* plan, int index, int arg, uint64_t value);
/* executes records [first, first + count) in order; stops at the first record that fails, returns its status (message:
 * gct2_last_error) and, if `failed` is non-NULL, stores its index there (-1 when all succeeded) */
int gct2_plan_run(gct2_plan* plan, int first, int count, int* failed);

#ifdef __cplusplus
}
#endif
#endif /* GCT2_H */
