"""The reference's off-by-default model variants, executed layer by layer through the C ABI.

    block_depth > 0   Block = block_depth x Conv2D(filters, 3, 1, 'same', relu)                        train.py:20, 123-143
    residual = True   Residual.call = input + Dense(input_channels, use_bias=False)(module(input))     train.py:26, 104-112
    concat = False    Residual.call = module(input)                                                    train.py:27, 120-121

They change the channel plan of the whole network (a Block in front of level 0 turns the 3-channel image into pixel_size channels,
the residual form keeps every level's width), so the zero-copy plan of engine.py (built for the default topology, the metric's hot
path) does not apply: `VariantEngine` walks the nested structure of train.py:175-204 with a forward and a hand-written reverse pass
per node.  Same kernels as the hot path for DownShuffle / UpShuffle (gct2_conv4s2_*, gct2_convT4s2_*), the stride-1 convolution
entry points for Block and the 1 x 1 projection, the Dense(3) head, MSE, Keras Adam, the loss-scale state machine.  PyTorch only
moves memory here (clone, cat, contiguous slices).  Built for results (parity-tested against oracle/variants_oracle.py), not for the
roofline: these branches are unreachable at the reference's defaults.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import BF16, F16, F32, call
from .trainer_math import EVAL_STREAM_EPS, TrainerState, check_head_options, check_timesteps, glorot_limit

TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}


class _Net:
    """parameter bookkeeping shared by the nodes: one flat fp32 arena each for p, m, v, g and a compute-dtype operand copy."""

    def __init__(self, dtype: int, device: torch.device, ctx: "_lib.Context"):
        self.dtype, self.device = dtype, device
        self.specs: List[Tuple[str, Tuple[int, ...]]] = []
        self.offsets: Dict[str, int] = {}
        self.total = 0
        self.ctx = ctx
        self.t_int: Optional[torch.Tensor] = None      # device int32[B]: the timesteps of the batch in flight (per-timestep heads)
        self.steps_scratch = None                      # (B, HW, cin) -> scratch tensor of gct2_dense_steps_bwd (the engine's allocator)
        self.unregularized: set = set()      # tensors built without kernel_regularizer (Residual's projection, train.py:107)

    def declare(self, name: str, shape: Tuple[int, ...]) -> str:
        self.specs.append((name, shape))
        self.offsets[name] = self.total
        self.total += (int(np.prod(shape)) + 63) // 64 * 64
        return name

    def allocate(self) -> None:
        z = lambda dt: torch.zeros(max(self.total, 64), dtype=dt, device=self.device)
        self.p, self.m, self.v, self.g = z(torch.float32), z(torch.float32), z(torch.float32), z(torch.float32)
        self.op = z(TORCH_DTYPE[self.dtype]) if self.dtype != F32 else self.p
        self.shapes = dict(self.specs)
        # the exponential moving average of p and of the operand copy (TrainerState.enable_ema; None while EMA is off) and which
        # of the two weight sets optr / pptr hand out (TrainerState.ema_weights)
        self.ema = self.ema_op = None
        self.read_ema = False

    def view(self, arena: torch.Tensor, name: str) -> torch.Tensor:
        o, shp = self.offsets[name], self.shapes[name]
        return arena[o:o + int(np.prod(shp))].view(shp)

    def optr(self, name: str) -> int:       # operand (compute dtype) pointer
        op = self.ema_op if self.read_ema else self.op
        return op.data_ptr() + self.offsets[name] * op.element_size()

    def pptr(self, name: str) -> int:
        return (self.ema if self.read_ema else self.p).data_ptr() + 4 * self.offsets[name]

    def gptr(self, name: str) -> int:
        return self.g.data_ptr() + 4 * self.offsets[name]

    def stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream


class _Conv:
    """y = relu(conv(x) + b) for the three convolution kinds; reverse pass: ReLU mask, weight / bias gradient, input gradient.
    Kind "d1" is Dense(cout, relu) on a rank-4 tensor - the hidden layer of train.py:195-197 - as a 1 x 1 convolution: kernel (cin, cout)."""

    def __init__(self, net: _Net, name: str, kind: str, cin: int, cout: int):
        self.net, self.kind, self.cin, self.cout = net, kind, cin, cout
        shape = {"down": (4, 4, cin, cout), "up": (4, 4, cout, cin), "c3": (3, 3, cin, cout), "d1": (cin, cout)}[kind]
        self.ks = 1 if kind == "d1" else 3
        self.w, self.b = net.declare(name + ".w", shape), net.declare(name + ".b", (cout,))

    def fwd(self, x: torch.Tensor) -> torch.Tensor:
        n, (B, H, W, C) = self.net, x.shape
        assert C == self.cin, (C, self.cin)
        Ho, Wo = {"down": (H // 2, W // 2), "up": (2 * H, 2 * W), "c3": (H, W), "d1": (H, W)}[self.kind]
        y = torch.empty(B, Ho, Wo, self.cout, dtype=x.dtype, device=x.device)
        cx, dt, s = n.ctx.handle, n.dtype, n.stream()
        if self.kind == "down":
            if H % 2 or W % 2:
                raise ValueError(f"DownShuffle needs even spatial dims, got {H}x{W} (train.py:114-119)")
            call("gct2_conv4s2_fwd", cx, dt, x.data_ptr(), C, n.optr(self.w), n.pptr(self.b), y.data_ptr(), self.cout, B, H, W, C, self.cout, 1, s)
        elif self.kind == "up":
            call("gct2_convT4s2_fwd", cx, dt, x.data_ptr(), C, n.optr(self.w), n.pptr(self.b), y.data_ptr(), self.cout, B, H, W, C, self.cout, 1, s)
        else:
            call("gct2_conv2d_s1_fwd", cx, dt, x.data_ptr(), C, n.optr(self.w), n.pptr(self.b), y.data_ptr(), self.cout, B, H, W, C, self.cout, self.ks, 1, s)
        self.x, self.y = x, y
        return y

    def bwd(self, dy: torch.Tensor) -> torch.Tensor:
        n, x, y = self.net, self.x, self.y
        B, H, W, C = x.shape
        cx, dt, s = n.ctx.handle, n.dtype, n.stream()
        dz = dy.contiguous().clone()
        call("gct2_relu_mask", dt, y.data_ptr(), self.cout, dz.data_ptr(), self.cout, dz.numel() // self.cout, self.cout, s)
        dx = torch.empty_like(x)
        if self.kind == "down":
            call("gct2_conv4s2_wgrad", cx, dt, x.data_ptr(), C, dz.data_ptr(), self.cout, n.gptr(self.w), n.gptr(self.b), B, H, W, C, self.cout, 0, None, s)
            call("gct2_conv4s2_dgrad", cx, dt, dz.data_ptr(), self.cout, n.optr(self.w), None, 0, dx.data_ptr(), C, B, H, W, C, self.cout, 0,
                 None, 0, None, 0, s)
        elif self.kind == "up":
            call("gct2_convT4s2_wgrad", cx, dt, x.data_ptr(), C, dz.data_ptr(), self.cout, n.gptr(self.w), n.gptr(self.b), B, H, W, C, self.cout, 0, None, s)
            call("gct2_convT4s2_dgrad", cx, dt, dz.data_ptr(), self.cout, n.optr(self.w), None, 0, dx.data_ptr(), C, B, H, W, C, self.cout, 0,
                 None, 0, None, 0, s)
        else:
            call("gct2_conv2d_s1_wgrad", cx, dt, x.data_ptr(), C, dz.data_ptr(), self.cout, n.gptr(self.w), n.gptr(self.b), B, H, W, C, self.cout, self.ks, 0, s)
            call("gct2_conv2d_s1_dgrad", cx, dt, dz.data_ptr(), self.cout, n.optr(self.w), None, 0, dx.data_ptr(), C, B, H, W, C, self.cout, self.ks, 0, s)
        self.x = self.y = None
        return dx


class _Proj:
    """Dense(cout, use_bias=False) on a rank-4 tensor (train.py:106): a 1 x 1 convolution without bias or activation."""

    def __init__(self, net: _Net, name: str, cin: int, cout: int):
        self.net, self.cin, self.cout = net, cin, cout
        self.w = net.declare(name + ".w", (cin, cout))
        net.unregularized.add(self.w)        # train.py:107: Dense(input_shape[-1], use_bias=False), no regularizer

    def fwd(self, x):
        n, (B, H, W, C) = self.net, x.shape
        y = torch.empty(B, H, W, self.cout, dtype=x.dtype, device=x.device)
        call("gct2_conv2d_s1_fwd", n.ctx.handle, n.dtype, x.data_ptr(), C, n.optr(self.w), None, y.data_ptr(), self.cout, B, H, W, C, self.cout,
             1, 0, n.stream())
        self.x = x
        return y

    def bwd(self, dy):
        n, x = self.net, self.x
        B, H, W, C = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        call("gct2_conv2d_s1_wgrad", n.ctx.handle, n.dtype, x.data_ptr(), C, dy.data_ptr(), self.cout, n.gptr(self.w), None, B, H, W, C, self.cout,
             1, 0, n.stream())
        call("gct2_conv2d_s1_dgrad", n.ctx.handle, n.dtype, dy.data_ptr(), self.cout, n.optr(self.w), None, 0, dx.data_ptr(), C, B, H, W, C,
             self.cout, 1, 0, n.stream())
        self.x = None
        return dx


class _Seq:
    def __init__(self, nodes):
        self.nodes = [n for n in nodes if n is not None]

    def fwd(self, x):
        for n in self.nodes:
            x = n.fwd(x)
        return x

    def bwd(self, dy):
        for n in reversed(self.nodes):
            dy = n.bwd(dy)
        return dy


class _Residual:
    """train.py:97-121 in all three modes."""

    def __init__(self, net: _Net, name: str, module: _Seq, cin: int, cmod: int, residual: bool, concat: bool):
        self.net, self.module, self.cmod = net, module, cmod
        self.mode = "residual" if residual else ("concat" if concat else "module")
        self.proj = _Proj(net, name + ".dense", cmod, cin) if residual else None          # train.py:106: Dense(input_shape[-1])
        self.cout = {"residual": cin, "concat": cmod + cin, "module": cmod}[self.mode]

    def _add(self, dst, src):
        C = dst.shape[-1]
        call("gct2_add", self.net.dtype, dst.data_ptr(), C, src.data_ptr(), C, dst.numel() // C, C, self.net.stream())

    def fwd(self, x):
        m = self.module.fwd(x)
        if self.mode == "residual":                              # input + self.dense(self.module(input))
            y = x.clone()
            self._add(y, self.proj.fwd(m))
            return y
        if self.mode == "concat":                                # tf.concat([module(input), highway(input)], -1)
            return torch.cat([m, x], -1)
        return m

    def bwd(self, dy):
        if self.mode == "residual":
            dx = dy.contiguous().clone()
            self._add(dx, self.module.bwd(self.proj.bwd(dy)))
            return dx
        if self.mode == "concat":
            dx = dy[..., self.cmod:].contiguous()
            self._add(dx, self.module.bwd(dy[..., :self.cmod].contiguous()))
            return dx
        return self.module.bwd(dy)


class _Head:
    """Dense(3) (train.py:198-202): fp32 output for the fp32 loss (train.py:262-263).  steps > 0: the per-timestep heads
    (train.py:199, 203, 211-214) - Dense(3 * steps) whose slice t_int - 1 is picked per image inside gct2_dense_steps_fwd / _bwd;
    net.t_int (device int32[B], set by the engine before the forward pass) holds the timesteps."""

    def __init__(self, net: _Net, cin: int, steps: int = 0):
        self.net, self.cin, self.steps = net, cin, steps
        units = 3 * steps if steps else 3
        self.w, self.b = net.declare("dense.w", (cin, units)), net.declare("dense.b", (units,))

    def fwd(self, x):
        n = self.net
        M = x.numel() // self.cin
        y = torch.empty(*x.shape[:-1], 3, dtype=torch.float32, device=x.device)
        if self.steps:
            B = x.shape[0]
            if n.t_int is None or n.t_int.numel() != B:
                raise _lib.Gct2Error(f"the per-timestep heads need one timestep per image: {0 if n.t_int is None else n.t_int.numel()} for a batch of {B}")
            call("gct2_dense_steps_fwd", n.ctx.handle, n.dtype, x.data_ptr(), self.cin, n.pptr(self.w), n.pptr(self.b), n.t_int.data_ptr(),
                 y.data_ptr(), B, M // B, self.cin, 3, self.steps, n.stream())
            self.x = x
            return y
        call("gct2_dense_fwd", n.dtype, x.data_ptr(), self.cin, n.pptr(self.w), n.pptr(self.b), y.data_ptr(), M, self.cin, 3, n.stream())
        self.x = x
        return y

    def bwd(self, dpred):
        """dpred: fp32 [B,H,W,3].  Kernel / bias gradients in fp32 from the fp32 gradient (gct2_dense_bwd with no masked input
        gradient); the input gradient through the 1 x 1 convolution entry point, since the head's input is not a ReLU output in
        every variant."""
        n, x = self.net, self.x
        B, H, W, C = x.shape
        M = B * H * W
        if self.steps:
            return self._bwd_steps(dpred)
        dummy = torch.empty(8, dtype=x.dtype, device=x.device)
        call("gct2_dense_bwd", n.dtype, x.data_ptr(), C, n.pptr(self.w), dpred.data_ptr(), dummy.data_ptr(), 0, n.gptr(self.w), n.gptr(self.b),
             M, C, 3, 0, 0, n.stream())
        dz = dpred.to(x.dtype)
        dx = torch.empty_like(x)
        call("gct2_conv2d_s1_dgrad", n.ctx.handle, n.dtype, dz.data_ptr(), 3, n.optr(self.w), None, 0, dx.data_ptr(), C, B, H, W, C, 3, 1, 0,
             n.stream())
        self.x = None
        return dx

    def _bwd_steps(self, dpred):
        """the gathered head: kernel / bias gradients of every slice from gct2_dense_steps_bwd (no input gradient there: its ReLU mask
        belongs to the planned engine's layout); the input gradient per image through the 1 x 1 convolution entry point on that
        image's slice of the operand copy (gathered on the device, t_int clamped as the kernels clamp it: memory movement only)."""
        n, x = self.net, self.x
        B, H, W, C = x.shape
        sc = n.steps_scratch(B, H * W, C)                       # (kept by the engine per shape)
        call("gct2_dense_steps_bwd", n.ctx.handle, n.dtype, x.data_ptr(), C, n.pptr(self.w), n.t_int.data_ptr(), dpred.data_ptr(), None, 0,
             n.gptr(self.w), n.gptr(self.b), sc.data_ptr(), sc.numel(), B, H * W, C, 3, self.steps, 0, 0, n.stream())
        dz = dpred.to(x.dtype)
        dx = torch.empty_like(x)
        s_idx = (n.t_int.long() - 1).clamp_(0, self.steps - 1)
        op = n.view(n.ema_op if n.read_ema else n.op, self.w).view(C, self.steps, 3)
        w_img = op.index_select(1, s_idx).permute(1, 0, 2).contiguous()                # [B, C, 3]: image i's slice
        for i in range(B):
            call("gct2_conv2d_s1_dgrad", n.ctx.handle, n.dtype, dz[i].data_ptr(), 3, w_img[i].data_ptr(), None, 0, dx[i].data_ptr(), C, 1, H, W,
                 C, 3, 1, 0, n.stream())
        self.x = None
        return dx


def build_structure(net: _Net, pixel_size: int, max_size: int, octaves: int, block_depth: int, residual: bool, concat: bool,
                    head_steps: int = 0, hidden_dense: bool = False):
    """Denoiser.__init__ (train.py:175-204) with every switch honoured; returns (top sequential, channel count fed to Dense(3)).
    hidden_dense: Dense(pixel_size, relu) in front of the head (train.py:195-197) - here the composition the fused pair
    gct2_dense2_* is defined by (a 1 x 1 convolution with ReLU, then the head): the head's input is not a ReLU output in every
    variant, so the masked input gradient of the fused backward kernel does not apply."""

    def block(name: str, cin: int, filters: int):
        """Block(filters) (train.py:123-143): block_depth x [Conv2D(filters, 3, 1, 'same', relu)]; identity at depth 0."""
        nodes, c = [], cin
        for d in range(block_depth):
            nodes.append(_Conv(net, f"{name}.{d}", "c3", c, filters))
            c = filters
        return (_Seq(nodes) if nodes else None), c

    def level(i: int, cin: int):
        """the Residual of level i (train.py:180-190) and its output channel count."""
        filters = min(pixel_size * 2 ** i, max_size)
        down = _Conv(net, f"D{i}", "down", cin, filters)
        ba, c = block(f"blkA{i}", filters, filters)
        if i + 1 < octaves:
            inner, c = level(i + 1, c)
        else:
            inner, c = block("blkMid", c, min(pixel_size * 2 ** octaves, max_size))          # train.py:179
        bb, c = block(f"blkB{i}", c, filters)
        fu = min(pixel_size * 2 ** i // 2, max_size)
        up = _Conv(net, f"U{i}", "up", c, fu)
        res = _Residual(net, f"res{i}", _Seq([down, ba, inner, bb, up]), cin, fu, residual, concat)
        return res, res.cout

    b0, c = block("blkTopA", 3, pixel_size)                                                   # train.py:192
    if octaves > 0:
        mid, c = level(0, c)
    else:
        mid, c = block("blkMid", c, min(pixel_size, max_size))
    b1, c = block("blkTopB", c, pixel_size)                                                   # train.py:194
    hid = None
    if hidden_dense:
        hid, c = _Conv(net, "dense_hidden", "d1", c, pixel_size), pixel_size
    head = _Head(net, c, head_steps)
    return _Seq([b0, mid, b1, hid, head]), c


class VariantEngine(TrainerState):
    """train step of a Denoiser built with block_depth > 0 / residual / concat=False (same surface as UNetEngine where it matters:
    train_step, predict, get/set_params, get_grads, iterations, loss_scale, the objective switches, f32_matrix)."""

    def __init__(self, pixel_size: int, max_size: int, octaves: int, block_depth: int, residual: bool, concat: bool, dtype: int = F32,
                 device: Optional[torch.device] = None, steps: int = 200, base_lr: float = 2e-5, warm_up: int = 2000, beta_1: float = 0.9,
                 beta_2: float = 0.999, epsilon: float = 1e-7, loss_scaling: bool = False, seed: int = 1234, rng_seed: int = 0,
                 predict_x: bool = True, predict_scaled_epsilon: bool = False, prediction_weighting: bool = False,
                 ordinary_differential_equation: bool = False, f32_matrix: bool = False, use_ema: bool = False,
                 ema_momentum: float = 0.99, timestep_heads: bool = False, hidden_dense: bool = False,
                 head_initializer: str = "glorot_uniform", predict_v: bool = False):
        check_head_options(type(self).__name__, hidden_dense, timestep_heads, head_initializer)
        super().__init__(dtype, device, steps, base_lr, warm_up, beta_1, beta_2, epsilon, loss_scaling, rng_seed, predict_x,
                         predict_scaled_epsilon, prediction_weighting, ordinary_differential_equation, f32_matrix, predict_v=predict_v)
        self.octaves = octaves
        self.timestep_heads = bool(timestep_heads)      # train.py:199, 203, 211-214; fixed here: it decides the shape of dense.w / dense.b
        self.hidden_dense = bool(hidden_dense)          # train.py:195-197; fixed here: it adds dense_hidden.w / .b and changes dense.w's shape
        self.head_initializer = head_initializer        # train.py:199
        # one call context for the train step and for predict (the sampler): with f32_matrix every fp32 convolution runs on the
        # matrix cores, and the workspace below doubles as their split-K and weight-gradient scratch
        self.net = _Net(dtype, self.device, self._new_ctx())
        self.workspace = torch.empty(16 << 18, dtype=torch.float32, device=self.device)
        self.net.ctx.set_workspace(self.workspace)
        self.top, self.head_cin = build_structure(self.net, pixel_size, max_size, octaves, block_depth, residual, concat,
                                                  steps if self.timestep_heads else 0, self.hidden_dense)
        self._steps_store: dict = {}
        self.net.steps_scratch = lambda B, HW, cin: self._steps_scratch(self._steps_store, B, HW, cin)
        self.net.allocate()
        self.glorot_init(seed)
        self.partials = torch.zeros(1024, dtype=torch.float32, device=self.device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._loss_store: dict = {}     # scratch (and the DCT basis) of the non-default training losses, by kind and shape
        self.last = {}
        if use_ema:
            self.enable_ema(ema_momentum)

    # ---- the parameter averages (TrainerState.enable_ema) -------------------------------------------------------------------
    def _ema_source(self):
        return self.net.p, (self.net.op if self.dtype != F32 else None)

    def _ema_tensors(self):
        return self.net.ema, (self.net.ema_op if self.dtype != F32 else None)

    def _ema_attach(self, ema, ema_shadow) -> None:
        self.net.ema, self.net.ema_op = ema, (ema_shadow if self.dtype != F32 else ema)

    def _ema_select(self, on: bool) -> None:
        self.net.read_ema = bool(on)

    def _ema_selected(self) -> bool:
        return self.net.read_ema

    # ---- gradient clipping (TrainerState.set_clipping) ----------------------------------------------------------------------
    def _clip_segments(self):
        return sorted((self.net.offsets[name], int(np.prod(shp))) for name, shp in self.net.specs)

    def _clip_device(self):
        return self.net.g.device

    def _l2_segments(self):
        """every kernel, bias and the head carry the regularizer; Residual's bias-free projection is built without one (train.py:107)"""
        return sorted((self.net.offsets[name], int(np.prod(shp))) for name, shp in self.net.specs if name not in self.net.unregularized)

    # ---- parameters ---------------------------------------------------------------------------------------------------------
    @property
    def shapes(self) -> Dict[str, Tuple[int, ...]]:
        return self.net.shapes

    def glorot_init(self, seed: int) -> None:
        """Keras glorot_uniform kernels, zero biases (train.py:134,149,162; Dense default [TF])."""
        gen = torch.Generator(device="cpu").manual_seed(seed)
        for name, shp in self.net.specs:
            if name.endswith(".b"):
                continue
            w = (torch.rand(shp, generator=gen) * 2 - 1) * glorot_limit(shp)
            if name == "dense.w" and self.head_initializer == "zeros":      # train.py:199 '#kernel_initializer='zeros'' (the draw is still made)
                w.zero_()
            self.net.view(self.net.p, name).copy_(w.to(self.device))
        self.refresh_operands()

    def refresh_operands(self) -> None:
        if self.dtype != F32:
            call("gct2_cast_from_f32", self.dtype, self.net.p.data_ptr(), self.net.op.data_ptr(), self.net.p.numel(), self.net.stream())

    def set_params(self, params) -> None:
        for k, v in params.items():
            self.net.view(self.net.p, k).copy_(torch.as_tensor(np.asarray(v, dtype=np.float32)).to(self.device))
        self.refresh_operands()

    def get_params(self):
        return {k: self.net.view(self.net.p, k).cpu().numpy().copy() for k in self.net.shapes}

    def get_grads(self):
        return {k: self.net.view(self.net.g, k).cpu().numpy().copy() for k in self.net.shapes}

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def _noised(self, x, t_int, eps):
        B, H, W, _ = x.shape
        s = self.net.stream()
        if t_int is None:
            t_int = torch.zeros(B, dtype=torch.int32, device=self.device)
            call("gct2_rng_uniform_int", self.rng_seed, 1, self.rng_offset_t, t_int.data_ptr(), B, 1, self.steps, s)
            self.rng_offset_t += B
        else:
            t_int = t_int.to(self.device, torch.int32).contiguous()
        if eps is None:
            eps = torch.zeros_like(x)
            call("gct2_rng_normal", self.rng_seed, 2, self.rng_offset_eps, eps.data_ptr(), eps.numel(), s)
            self.rng_offset_eps += eps.numel()
        else:
            eps = eps.to(self.device, torch.float32).contiguous()
        out = torch.empty(B, H, W, 3, dtype=TORCH_DTYPE[self.dtype], device=self.device)
        if self._default_schedule():
            call("gct2_noise_image", self.dtype, x.data_ptr(), t_int.data_ptr(), eps.data_ptr(), out.data_ptr(), 3, None, 0, B, H * W, 3,
                 self.steps, s)
        else:                                                  # another schedule (set_noise_schedule): the pair comes from the host's table
            call("gct2_noise_image_table", self.dtype, x.data_ptr(), t_int.data_ptr(), eps.data_ptr(), self._noise_coef_ptr(), out.data_ptr(), 3,
                 None, 0, B, H * W, 3, self.steps, s)
        return out, t_int, eps

    def _objective(self, x, t_int, eps):
        """(target fp32, prediction weights or None) of train.py:238-252."""
        if self.default_objective():
            return x, None
        a, c, w = self.objective_coefficients(t_int)
        if not self.objective_weighted():
            w = None
        target = torch.empty_like(x)
        call("gct2_mix_per_image", x.data_ptr(), eps.data_ptr(), a.data_ptr(), c.data_ptr(), target.data_ptr(), x.shape[0],
             x.numel() // x.shape[0], self.net.stream())
        self.last["coef"] = (a, c, w)
        return target, w

    def train_step(self, x, t_int=None, eps=None, apply: bool = True, backward: bool = True):
        """backward=False: Trainer.call (train.py:223-272), the loss of a freshly noised batch without gradients."""
        if x.dim() != 4 or x.shape[-1] != 3:
            raise ValueError(f"expected an NHWC batch [B,H,W,3], got {tuple(x.shape)}")
        self._refuse_training_on_averages()
        self.check_step_settings()
        x = x.to(self.device, torch.float32).contiguous()
        B, H, W, _ = x.shape
        if H % (2 ** self.octaves) or W % (2 ** self.octaves):
            raise ValueError(f"spatial size {H}x{W} is not divisible by 2**octaves (train.py:114-119)")
        s = self.net.stream()
        n = B * H * W * 3
        self.begin_step()
        regularized = backward and self.l2 > 0.0               # (Trainer.call reports the data term, as calling the Keras model does)
        if regularized:
            self._penalty_begin(s)
        noised, t_int, eps = self._noised(x, t_int, eps)
        self.net.t_int = t_int                                 # (the per-timestep heads read it inside their kernels)
        pred = self.top.fwd(noised)
        weights = self.loss_weighting is not None               # the target is then formed inside the loss kernel: no target plane
        target, w = (None, None) if weights else self._objective(x, t_int, eps)
        if w is not None:
            call("gct2_mix_per_image", pred.data_ptr(), None, w.data_ptr(), None, pred.data_ptr(), B, H * W * 3, s)
        dpred = torch.empty_like(pred)
        if weights:                                            # set_loss_weighting: loss and gradient in one launch
            self.last["coef"] = self._objective_loss_launch(self._loss_store, pred, x, eps, t_int, dpred if backward else None, self.loss, s)
        elif self.training_loss != "mse":                        # train.py:265-280 (no gradient when there is no reverse pass)
            self._loss_launch(self._loss_store, pred, target.data_ptr(), dpred if backward else None, self.loss, s)
        else:
            call("gct2_mse_fwd_bwd", pred.data_ptr(), target.data_ptr(), dpred.data_ptr(), self.loss.data_ptr(), self.partials.data_ptr(), n, self._ls_ptr(), s)
        if w is not None:
            call("gct2_mix_per_image", dpred.data_ptr(), None, w.data_ptr(), None, dpred.data_ptr(), B, H * W * 3, s)
        self.last.update(pred=pred, noised=noised)
        if not backward:
            return self.loss
        loss = self._penalty_finish(self.loss, s) if regularized else self.loss
        self.top.bwd(dpred)
        if apply:
            self.apply_adam()
        return loss

    # ---- evaluation (TrainerState.evaluate_batch): where the input goes and how the forward pass runs ------------------------------
    def _eval_buffers(self, B: int, H: int, W: int):
        if H % (2 ** self.octaves) or W % (2 ** self.octaves):
            raise ValueError(f"spatial size {H}x{W} is not divisible by 2**octaves (train.py:114-119)")
        sets = self.__dict__.setdefault("_eval_sets", {})
        if (B, H, W) not in sets:
            sets[(B, H, W)] = (torch.zeros(B, dtype=torch.int32, device=self.device),
                               torch.zeros(B, H, W, 3, dtype=torch.float32, device=self.device), {})
        return sets[(B, H, W)]

    def _eval_noise(self, x, t_int, eps, draw):
        B, H, W, _ = x.shape
        out = torch.empty(B, H, W, 3, dtype=TORCH_DTYPE[self.dtype], device=self.device)
        tail = (out.data_ptr(), 3, None, 0, B, H * W, 3, self.steps, self.net.stream())
        if draw is None:
            head, name = (self.dtype, x.data_ptr(), t_int.data_ptr(), eps.data_ptr()), "gct2_noise_image"
        else:
            seed, offset, keep = draw
            head = (self.dtype, x.data_ptr(), t_int.data_ptr(), seed, EVAL_STREAM_EPS, offset, eps.data_ptr() if keep else None)
            name = "gct2_noise_image_rng"
        if self._default_schedule():
            call(name, *head, *tail)
        else:
            call(name + "_table", *head, self._noise_coef_ptr(), *tail)
        return out

    def _eval_forward(self, noised, t_int):
        self.flush_deferred()
        self.net.t_int = t_int                                 # (the per-timestep heads read it inside their kernels)
        return self.top.fwd(noised)

    def apply_adam(self) -> None:
        N, s = self.net, self.net.stream()
        if self.clip_mode != _lib.CLIP_NONE or self.optimizer_kind != "adam" or self._regularized():
            if not self._clip_by_norm():                       # (a norm-clipped step: gct2_grad_sumsq sets found_inf in its one pass)
                self._check_finite(N.g.data_ptr(), N.g.numel(), s)
            self._update_launches(N.p, N.m, N.v, N.g, N.op if self.dtype != F32 else None, 0, N.p.numel(), 1.0, s)
            self.finish_step()
            return
        self._check_finite(N.g.data_ptr(), N.g.numel(), s)
        shadow = N.op.data_ptr() if self.dtype != F32 else None
        call("gct2_adam_keras_multi", N.p.data_ptr(), N.m.data_ptr(), N.v.data_ptr(), N.g.data_ptr(), shadow, self.dtype, N.p.numel(),
             0.0 if self.ls_state is not None else self.adam_alpha(), self.beta_1, self.beta_2, self.epsilon, 1.0, self._ls_ptr(), 0, s)
        self.finish_step()

    def predict(self, noised: torch.Tensor, t=None, use_ema: bool = False) -> torch.Tensor:
        """use_ema: evaluate the averaged weights (ema_weights()) instead of the raw iterate.  t: the timestep(s) of the batch, one int
        or B of them in 1..steps - required by the per-timestep heads, accepted and ignored without them (as UNetEngine.predict)"""
        if self.timestep_heads and t is None:
            raise ValueError("predict: an engine built with timestep_heads=True needs the timestep(s) t of the batch (1..steps)")
        if use_ema:
            with self.ema_weights():
                return self.predict(noised, t)
        if self.timestep_heads:
            self.net.t_int = torch.tensor(check_timesteps(t, noised.shape[0], self.steps), dtype=torch.int32).to(self.device)
        return self.top.fwd(noised.to(self.device, TORCH_DTYPE[self.dtype]).contiguous())
