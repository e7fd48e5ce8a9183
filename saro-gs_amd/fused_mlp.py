"""The deformation heads as one fused kernel each way: Linear -> ReLU -> Linear -> ReLU -> Linear [-> Sigmoid] on the HIP library
(csrc/gsrast_mlp.h: fp32 on the f32-input matrix instruction, hidden activations kept on chip, recomputed by the backward), or, with
precision="bf16", on the bf16 matrix instruction with fp32 accumulation (csrc/gsrast_mlp_bf16.h states what is rounded where).

Stands where the reference's four nn.Sequential heads stand (scene/saro_gaussian.py:104-110: motion_mlp, rot_mlp, shs_mlp: 32 + 9 -> 128
-> 128 -> 3 / 7 / 48; opacity_mlp: 32 -> 128 -> 64 -> 1 with a Sigmoid), which it evaluates over all Gaussians once or twice per view:

  fused_mlp3(x, w1, b1, w2, b2, w3, b3, x_tail=None, sigmoid_out=False, precision="fp32")      the autograd function
  FusedMLP3 / FusedMLP3.from_sequential(seq, precision="fp32")               a module holding the Sequential's own Linear layers
  convert_heads(model, precision="fp32")                                     swaps a model's four head attributes in place

`x_tail` [N, D_tail] is read behind x's columns without a cat and receives no gradient: the reference's
`torch.cat((hexplane_feature, time_emb.detach()), 1)`.  Supported: D_x + D_tail <= 64, hidden widths in {32, 64, 96, 128}, D_out <= 64,
fp32 tensors at either precision (the bf16 path converts inside its kernels and keeps no bf16 copy).  There is no CPU / PyTorch fallback: without libgsrast_hip.so and GPU tensors this raises, as do other shapes."""
import ctypes as C
from typing import Optional

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from diff_gaussian_rasterization_ch3 import _C as _lib

HEAD_NAMES = ("motion_mlp", "rot_mlp", "shs_mlp", "opacity_mlp")
HIDDEN_WIDTHS = (32, 64, 96, 128)
MAX_IO = 64
PRECISIONS = {"fp32": _lib.MLP_FP32, "bf16": _lib.MLP_BF16}


def _precision(precision) -> int:
    """include/gsrast.h's GSRAST_MLP_* of "fp32" / "bf16", or a ValueError (no device needed)."""
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"fused_mlp3: precision must be one of {tuple(PRECISIONS)}, got {precision!r}")
    return PRECISIONS[precision]


def _check_shapes(x, w1, b1, w2, b2, w3, b3, x_tail):
    """Dims of one call, or a ValueError naming what is unsupported (no device needed)."""
    if x.dim() != 2:
        raise ValueError("fused_mlp3: x must be [N, D_x]")
    N, d_x = int(x.shape[0]), int(x.shape[1])
    d_tail = 0
    if x_tail is not None:
        if x_tail.dim() != 2 or int(x_tail.shape[0]) != N:
            raise ValueError("fused_mlp3: x_tail must be [N, D_tail] with x's row count")
        d_tail = int(x_tail.shape[1])
    if any(w.dim() != 2 for w in (w1, w2, w3)) or any(b.dim() != 1 for b in (b1, b2, b3)):
        raise ValueError("fused_mlp3: weights must be [out, in] and biases [out], as nn.Linear holds them")
    h1, h2, d_out = int(w1.shape[0]), int(w2.shape[0]), int(w3.shape[0])
    if d_x < 1 or not 1 <= d_x + d_tail <= MAX_IO:
        raise ValueError(f"fused_mlp3: D_in = D_x + D_tail = {d_x} + {d_tail} must be in [1, {MAX_IO}] with D_x >= 1")
    if h1 not in HIDDEN_WIDTHS or h2 not in HIDDEN_WIDTHS:
        raise ValueError(f"fused_mlp3: hidden widths {h1}, {h2} must be in {HIDDEN_WIDTHS}")
    if not 1 <= d_out <= MAX_IO:
        raise ValueError(f"fused_mlp3: D_out = {d_out} must be in [1, {MAX_IO}]")
    if tuple(w1.shape) != (h1, d_x + d_tail) or tuple(w2.shape) != (h2, h1) or tuple(w3.shape) != (d_out, h2) \
            or tuple(b1.shape) != (h1,) or tuple(b2.shape) != (h2,) or tuple(b3.shape) != (d_out,):
        raise ValueError("fused_mlp3: the layers' shapes do not chain (w1 [H1, D_x + D_tail], w2 [H2, H1], w3 [D_out, H2])")
    for t in (x, w1, b1, w2, b2, w3, b3) + ((x_tail,) if x_tail is not None else ()):
        if t.dtype != torch.float32:
            raise ValueError("fused_mlp3: fp32 tensors only")
    return N, d_x, d_tail, h1, h2, d_out


def _desc(N, d_x, d_tail, h1, h2, d_out, sigmoid, **ptrs):
    d = _lib.Mlp3Struct(N, d_x, d_tail, h1, h2, d_out, int(sigmoid))
    for k, t in ptrs.items():
        if t is not None:
            setattr(d, k, t.data_ptr() if t.numel() else None)
    return d


class _FusedMLP3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x_tail, w1, b1, w2, b2, w3, b3, sigmoid_out, workgroups, precision):
        dims = _check_shapes(x, w1, b1, w2, b2, w3, b3, x_tail)
        if not x.is_cuda:
            raise RuntimeError("fused_mlp3: tensors must be on a GPU (HIP) device; there is no CPU fallback")
        for name, t in (("x_tail", x_tail), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("w3", w3), ("b3", b3)):
            if t is not None and t.device != x.device:      # (a model not yet moved with .to(device): an error text, not a device fault)
                raise RuntimeError(f"fused_mlp3: {name} is on {t.device}, x on {x.device}; all tensors must be on x's device")
        dev = x.device
        # made contiguous as fused_hexplane does with its inputs (parameters and the lookup's output are contiguous already: no copy)
        xs = x.detach().contiguous()
        ts = x_tail.detach().contiguous() if x_tail is not None and dims[2] else None
        ws = [p.detach().contiguous() for p in (w1, b1, w2, b2, w3, b3)]
        y = torch.empty((dims[0], dims[5]), dtype=torch.float32, device=dev)
        d = _desc(*dims, sigmoid_out, x=xs, x_tail=ts, w1=ws[0], b1=ws[1], w2=ws[2], b2=ws[3], w3=ws[4], b3=ws[5], y=y)
        _lib.launch("gsrast_mlp3_forward_p", dev, C.byref(d), int(precision), int(workgroups))
        ctx.dims, ctx.sigmoid, ctx.workgroups, ctx.has_tail, ctx.precision = dims, bool(sigmoid_out), int(workgroups), ts is not None, int(precision)
        # the hidden activations are not kept: x, the tail, the parameters, and y for the sigmoid's derivative
        ctx.save_for_backward(xs, ts if ts is not None else xs.new_empty(0), *ws, y if sigmoid_out else xs.new_empty(0))
        return y

    @staticmethod
    @once_differentiable      # (the kernels are not differentiable themselves: a double backward raises)
    def backward(ctx, dy):
        xs, ts, w1, b1, w2, b2, w3, b3, y = ctx.saved_tensors
        N, d_x, d_tail, h1, h2, d_out = ctx.dims
        dev = xs.device
        need = ctx.needs_input_grad
        if dy.device != dev:
            raise RuntimeError(f"fused_mlp3: the upstream gradient is on {dy.device}, x on {dev}")
        dy = dy.contiguous().float()
        g = {}
        if need[0]:
            g["dx"] = torch.empty_like(xs)
        for k, (name, ref) in enumerate((("dw1", w1), ("db1", b1), ("dw2", w2), ("db2", b2), ("dw3", w3), ("db3", b3))):
            if need[2 + k]:
                g[name] = torch.empty_like(ref)
        d = _desc(N, d_x, d_tail, h1, h2, d_out, ctx.sigmoid, x=xs, x_tail=ts if ctx.has_tail else None, w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3,
                  y=y if ctx.sigmoid else None, dy=dy, **g)
        scratch = None
        if any(k != "dx" for k in g):
            nbytes = _lib.scratch_bytes("gsrast_mlp3_scratch_bytes_p", C.byref(d), ctx.precision, ctx.workgroups)      # workgroups x parameters: independent of N
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if g:
            _lib.launch("gsrast_mlp3_backward_p", dev, C.byref(d), ctx.precision, ctx.workgroups, scratch.data_ptr() if scratch is not None else None)
        return (g.get("dx"), None, g.get("dw1"), g.get("db1"), g.get("dw2"), g.get("db2"), g.get("dw3"), g.get("db3"), None, None, None)


def fused_mlp3(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, *,
               x_tail: Optional[torch.Tensor] = None, sigmoid_out: bool = False, workgroups: int = 0, precision: str = "fp32") -> torch.Tensor:
    """[sigmoid](relu(relu([x | x_tail] w1^T + b1) w2^T + b2) w3^T + b3).  Gradients go to x and the six parameters (each only when it
    requires one), never to x_tail.  `workgroups` = 0 is the library's choice for the device; the weight gradients are bit-identical from run
    to run for the same count.  `precision` = "bf16" runs the products on the bf16 matrix instruction with fp32 accumulation (inputs, weights,
    hidden activations and back-propagated gradients rounded to bfloat16 where a product reads them); every tensor stays fp32 and the
    gradients are the fp32 parameters', as under autocast."""
    return _FusedMLP3Fn.apply(x, x_tail, w1, b1, w2, b2, w3, b3, bool(sigmoid_out), int(workgroups), _precision(precision))


class FusedMLP3(nn.Module):
    """Drop-in for nn.Sequential(Linear, ReLU, Linear, ReLU, Linear[, Sigmoid]).  The three Linear layers are children named "0", "2", "4"
    like the Sequential's, so the state_dict keys (0.weight, 0.bias, 2.weight, ...), the order of parameters() and -- through
    from_sequential -- the Parameter objects themselves are the Sequential's: checkpoints, optimizer groups and flat gradient buckets built
    from the Sequential keep working.  `precision` ("fp32" / "bf16") is a plain attribute: not a parameter, not a buffer, not in the state_dict."""

    def __init__(self, d_in: int, h1: int, h2: int, d_out: int, sigmoid_out: bool = False, precision: str = "fp32"):
        super().__init__()
        self._adopt(nn.Linear(d_in, h1), nn.Linear(h1, h2), nn.Linear(h2, d_out), sigmoid_out, precision)

    def _adopt(self, l1: nn.Linear, l2: nn.Linear, l3: nn.Linear, sigmoid_out: bool, precision: str = "fp32") -> None:
        _precision(precision)
        for l in (l1, l2, l3):
            if l.bias is None:
                raise ValueError("FusedMLP3: every Linear needs its bias")
        if l1.out_features not in HIDDEN_WIDTHS or l2.out_features not in HIDDEN_WIDTHS:
            raise ValueError(f"FusedMLP3: hidden widths {l1.out_features}, {l2.out_features} must be in {HIDDEN_WIDTHS}")
        if not 1 <= l1.in_features <= MAX_IO or not 1 <= l3.out_features <= MAX_IO:
            raise ValueError(f"FusedMLP3: input and output widths must be in [1, {MAX_IO}]")
        if l2.in_features != l1.out_features or l3.in_features != l2.out_features:
            raise ValueError("FusedMLP3: the layers' widths do not chain")
        self.add_module("0", l1)
        self.add_module("2", l2)
        self.add_module("4", l3)
        self.sigmoid_out = bool(sigmoid_out)
        self.precision = precision

    @classmethod
    def from_sequential(cls, seq: nn.Sequential, precision: str = "fp32") -> "FusedMLP3":
        """The fused module over `seq`'s own Linear layers (same Parameter objects).  Any other structure raises."""
        if not isinstance(seq, nn.Sequential):
            raise ValueError("FusedMLP3.from_sequential: not an nn.Sequential")
        mods = list(seq)
        sigmoid_out = len(mods) == 6 and type(mods[5]) is nn.Sigmoid
        if not (len(mods) == 5 or sigmoid_out) or [type(m) for m in mods[:5]] != [nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear]:
            raise ValueError("FusedMLP3.from_sequential: expected Linear, ReLU, Linear, ReLU, Linear[, Sigmoid], got "
                             + ", ".join(type(m).__name__ for m in mods))
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self._adopt(mods[0], mods[2], mods[4], sigmoid_out, precision)
        self.train(seq.training)
        return self

    def forward(self, x: torch.Tensor, x_tail: Optional[torch.Tensor] = None) -> torch.Tensor:
        l1, l2, l3 = self._modules["0"], self._modules["2"], self._modules["4"]
        return fused_mlp3(x, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias, x_tail=x_tail, sigmoid_out=self.sigmoid_out,
                          precision=self.precision)

    def extra_repr(self) -> str:
        return f"sigmoid_out={self.sigmoid_out}, precision={self.precision}"


def convert_heads(model, names=HEAD_NAMES, precision="fp32"):
    """Swap `model`'s deformation heads for FusedMLP3 in place, where the attribute exists and is a Sequential of the fused structure and
    widths; returns the names converted.  The parameters stay the same objects, so an optimizer built before the call stays valid.  `precision` is
    given to every head converted."""
    _precision(precision)
    done = []
    for name in names:
        seq = getattr(model, name, None)
        if not isinstance(seq, nn.Sequential):
            continue
        try:
            fused = FusedMLP3.from_sequential(seq, precision)
        except ValueError:
            continue
        setattr(model, name, fused)
        done.append(name)
    return done
