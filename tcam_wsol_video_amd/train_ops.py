"""The layer ops the three trainers share (:class:`~.training.DecoderTrainer`,
:class:`~.cl_training.ClassifierTrainer`, :class:`~.vgg_training.VGG16ClassifierTrainer`):
weight packing, BatchNorm forward / backward, the scaled MFMA copy of a gradient and the conv
weight gradient, as plain functions over the kernels of libtcam_hip.so.  No state: a function
that needs scratch takes the workspace tensor and has a ``*_ws_bytes`` helper, so each trainer
keeps its own allocation policy.  Which C entry runs depends only on the formats and the
geometry handed in:

  fmt    the convolutions' format: "x6" (S3 activations), "f16x3" (S2) or "amp" (S1)
  glay   the gradients' layout: "s3" (x6 and f16x3) or "s1" (AMP)

A gradient travels as :class:`Grad` ``(dy, op, scale)``: ``op`` is what the MFMA weight and
data gradients read — dy's per-channel scaled S2 copy on f16x3, ``dy`` itself on x6 and AMP —
``scale`` its per-channel powers of two (None off f16x3), and ``dy`` the gradient in ``glay``
(None when the fused f16x3 backward was not asked for it).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._lib import check, tcam_conv_src
from .flat_sgd import _stream


class Grad(NamedTuple):
    dy: Optional[torch.Tensor]
    op: torch.Tensor
    scale: Optional[torch.Tensor]


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------ weight pack
# parts per value and dtype of each format's operand (Kpad/32, 4, parts, Mpad, 8)
_OPERAND = {"x6": (3, torch.bfloat16), "amp": (1, torch.float16), "f16x3": (2, torch.float16)}


def pack_weight(w: torch.Tensor, fmt: str, mode: int, *, c0: int = 0, sel: int = 0,
                cin_pad: int = 0, kdiv: Optional[torch.Tensor] = None, out=None):
    """The MFMA operand of conv weight ``w`` (Cout, Cin, KH, KW), packed on the device: mode 0
    the forward's (inputs zero-padded to ``cin_pad`` channels), mode 1 the data gradient's
    (transposed, rotated, over input channels [c0, c0 + sel), dy zero-padded to ``cin_pad``
    channels); f16x3: divided by ``kdiv`` (dy's per-channel scales).  ``out``: a (wt, wscale)
    pair to pack into when it has the operand's shape.  Returns (wt, wscale or None)."""
    cout, ctot, kh, kw = w.shape
    if mode == 0:
        K, M = kh * kw * max(ctot, cin_pad), cout
    else:
        K, M = kh * kw * max(cout, cin_pad), sel
    kp, mp = ops.conv_x6_weight_dims(K, M)
    parts, dtype = _OPERAND[fmt]
    shape = (kp // 32, 4, parts, mp, 8)
    wt, sc = out if out is not None else (None, None)
    if wt is None or wt.dtype != dtype or tuple(wt.shape) != shape:
        wt = torch.empty(shape, device=w.device, dtype=dtype)
        sc = torch.empty(mp, device=w.device, dtype=torch.float32) if fmt == "f16x3" else None
    lib = _lib.load()
    if fmt == "f16x3":
        check(lib.tcam_pack_weight_f16x3(w.data_ptr(), wt.data_ptr(), sc.data_ptr(), mode, cout,
                                         ctot, kh, kw, c0, sel, cin_pad, _p(kdiv), _stream()),
              "tcam_pack_weight_f16x3")
        return wt, sc
    fn, name = (lib.tcam_pack_weight_f16, "tcam_pack_weight_f16") if fmt == "amp" else \
        (lib.tcam_pack_weight_x6, "tcam_pack_weight_x6")
    check(fn(w.data_ptr(), wt.data_ptr(), mode, cout, ctot, kh, kw, c0, sel, cin_pad, _stream()),
          name)
    return wt, None


# -------------------------------------------------------------------- BatchNorm
def bn_ws_bytes(y: torch.Tensor, scaled: bool = False) -> int:
    """Workspace of :func:`bn_stats` / :func:`bn_relu_bwd` on ``y``; ``scaled``: of the f16x3
    step's fused backward (the larger of the two)."""
    B, H, W, Cc = ops.s3_dims(y)
    lib = _lib.load()
    return int((lib.tcam_bn_bwd_scaled_ws_bytes if scaled else lib.tcam_bn_ws_bytes)(B * H * W,
                                                                                   Cc))


def bn_stats(y: torch.Tensor, bn, lay: str, ws: torch.Tensor):
    """(mean, invstd) of ``y`` over (B, H, W), ``bn``'s running statistics updated in place."""
    B, H, W, Cc = ops.s3_dims(y)
    mean = torch.empty(Cc, device=y.device)
    invstd = torch.empty(Cc, device=y.device)
    check(getattr(_lib.load(), f"tcam_bn_stats_{lay}")(
        y.data_ptr(), B * H * W, Cc, bn.eps, bn.momentum, mean.data_ptr(), invstd.data_ptr(),
        bn.running_mean.data_ptr(), bn.running_var.data_ptr(), ws.data_ptr(), _stream()),
        f"tcam_bn_stats_{lay}")
    return mean, invstd


def bn_relu(y: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, bn, lay: str):
    """relu(gamma (y - mean) invstd + beta), in y's layout."""
    B, H, W, Cc = ops.s3_dims(y)
    out = torch.empty_like(y)
    check(getattr(_lib.load(), f"tcam_bn_relu_{lay}")(
        y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), bn.weight.data_ptr(),
        bn.bias.data_ptr(), out.data_ptr(), B * H * W, Cc, _stream()), f"tcam_bn_relu_{lay}")
    return out


def bn_relu_bwd(dout, out, y, mean, invstd, bn, dgamma, dbeta, fmt: str, ws: torch.Tensor, *,
                scaled: bool = True, masky: bool = False, need_dy: bool = False) -> Grad:
    """The gradient of a BatchNorm whose output went through the ReLU that produced ``out``
    (the mask), dgamma / dbeta written.  f16x3: the fused backward, straight to the scaled S2
    copy (``need_dy``: the S3 dy too; ``scaled`` False: the unfused backward, the S3 dy alone);
    AMP: the fused two-pass backward; x6: the three-pass one.  ``masky``: a plain BN-ReLU, the
    mask recomputed from y instead of read from ``out`` (f16x3 and AMP).  ``ws``:
    :func:`bn_ws_bytes` of ``y`` (``scaled`` on f16x3)."""
    lib = _lib.load()
    B, H, W, Cc = ops.s3_dims(y)
    P = B * H * W
    head = (dout.data_ptr(), None if masky else out.data_ptr(), y.data_ptr(), mean.data_ptr(),
            invstd.data_ptr(), bn.weight.data_ptr())
    if fmt == "f16x3" and scaled:
        dy = ops.lay_empty("s3", B, H, W, Cc, y.device) if need_dy else None
        dy2 = ops.lay_empty("s2", B, H, W, Cc, y.device)
        scale = torch.empty(Cc, device=y.device, dtype=torch.float32)
        check(lib.tcam_bn_relu_bwd_scaled_s3s2(
            *head, bn.bias.data_ptr(), _p(dy), dy2.data_ptr(), scale.data_ptr(),
            dgamma.data_ptr(), dbeta.data_ptr(), P, Cc, ws.data_ptr(), _stream()),
            "tcam_bn_relu_bwd_scaled_s3s2")
        return Grad(dy, dy2, scale)
    if fmt == "amp":
        dy = ops.lay_empty("s1", B, H, W, Cc, y.device)
        check(lib.tcam_bn_relu_bwd_fused_s1(
            *head, bn.bias.data_ptr(), dy.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), P, Cc,
            ws.data_ptr(), _stream()), "tcam_bn_relu_bwd_fused_s1")
        return Grad(dy, dy, None)
    dy = ops.lay_empty("s3", B, H, W, Cc, y.device)
    tail = (dy.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), P, Cc, ws.data_ptr())
    if fmt == "f16x3":   # S3 gradients over S2 activations, no channel maxima
        check(lib.tcam_bn_relu_bwd_s3s2(*head, *tail, None, _stream()), "tcam_bn_relu_bwd_s3s2")
    else:
        check(lib.tcam_bn_relu_bwd_s3(*head, *tail, _stream()), "tcam_bn_relu_bwd_s3")
    return Grad(dy, dy, None)


def dy_scaled(dy: torch.Tensor, amax: Optional[torch.Tensor] = None) -> Grad:
    """An S3 gradient with its per-channel power-of-two scaled S2 copy (max |dy_c| scale_c in
    [2^14, 2^15)); the channel maxima ``amax`` are computed here when not given."""
    B, H, W, Cc = ops.s3_dims(dy)
    compute = amax is None
    if compute:
        amax = torch.empty(Cc, device=dy.device, dtype=torch.int32)
    scale = torch.empty(Cc, device=dy.device, dtype=torch.float32)
    dy2 = ops.lay_empty("s2", B, H, W, Cc, dy.device)
    check(_lib.load().tcam_dy_scaled_s2(dy.data_ptr(), B * H * W, Cc, amax.data_ptr(),
                                        1 if compute else 0, scale.data_ptr(), dy2.data_ptr(),
                                        _stream()), "tcam_dy_scaled_s2")
    return Grad(dy, dy2, scale)


# -------------------------------------------------------------- weight gradient
def conv_srcs(srcs: Sequence["ops.ConvSrc"]):
    """The ``tcam_conv_src[]`` of a conv's input sources."""
    arr = (tcam_conv_src * len(srcs))()
    for i, s in enumerate(srcs):
        _, H, W, Cc = ops.s3_dims(s.t)
        arr[i] = tcam_conv_src(s.t.data_ptr(), Cc, H, W, s.stride, 1 if s.up2 else 0)
    return arr


def _generic(arr, fmt: str, k: Tuple[int, int], pad: int) -> bool:
    """f16x3 off the 3x3 / stride-1 / pad-1 MFMA path: the fp32-MFMA general path on dy."""
    return fmt == "f16x3" and not (k == (3, 3) and arr[0].stride == 1 and pad == 1)


def conv_wgrad_ws_bytes(arr, g: Grad, fmt: str, k, pad: int) -> int:
    """Workspace of :func:`conv_wgrad` with the same arguments (0: unsupported geometry)."""
    k = (k, k) if isinstance(k, int) else k
    lib = _lib.load()
    gen = _generic(arr, fmt, k, pad)
    B, Ho, Wo, Cd = ops.s3_dims(g.dy if gen else g.op)
    query = lib.tcam_conv_wgrad_generic_ws_bytes if gen else lib.tcam_conv_wgrad_ws_bytes
    return int(query(arr, len(arr), B, Cd, Ho, Wo, k[0], k[1]))


def conv_wgrad(arr, g: Grad, dw: torch.Tensor, ws: torch.Tensor, fmt: str, k, pad: int, *,
               wgrad_prec: Optional[str] = None, cout_store: Optional[int] = None) -> None:
    """dW (Cout, Ctot, KH, KW) of a conv on the sources ``arr`` (:func:`conv_srcs`) from the
    gradient ``g`` of its output.  AMP: the fp16 product on ``g.op`` (S1); f16x3: the MFMA path
    on ``g.op`` / ``g.scale`` for 3x3 / stride 1 / pad 1, else the fp32-MFMA general path on
    ``g.dy`` (S3); x6: three fp16 products (``wgrad_prec`` "f16x3": an x beyond the fp16 range
    sets the overflow flag, raised by ops.check_f16_overflow) or the six bf16 ones.  ``ws``:
    :func:`conv_wgrad_ws_bytes`; ``cout_store``: rows of dW written (a padded dy)."""
    k = (k, k) if isinstance(k, int) else k
    lib = _lib.load()
    gen = _generic(arr, fmt, k, pad)
    dy = g.dy if gen else g.op
    B, Ho, Wo, Cd = ops.s3_dims(dy)
    tail = (Cd, Ho, Wo, k[0], k[1], pad, pad, cout_store or Cd, dw.data_ptr(), ws.data_ptr(),
            ws.numel())
    if fmt == "amp":
        check(lib.tcam_conv_wgrad_s1(arr, len(arr), B, dy.data_ptr(), *tail, _stream()),
              "tcam_conv_wgrad_s1")
    elif gen:
        check(lib.tcam_conv_wgrad_s3s2(arr, len(arr), B, dy.data_ptr(), *tail, _stream()),
              "tcam_conv_wgrad_s3s2")
    elif fmt == "f16x3":
        check(lib.tcam_conv_wgrad_s2_f16x3(arr, len(arr), B, dy.data_ptr(), g.scale.data_ptr(),
                                           *tail, _stream()), "tcam_conv_wgrad_s2_f16x3")
    elif wgrad_prec == "f16x3":
        check(lib.tcam_conv_wgrad_s3_f16x3(arr, len(arr), B, dy.data_ptr(), *tail,
                                           ops.f16_overflow_flag(dw.device).data_ptr(),
                                           _stream()), "tcam_conv_wgrad_s3_f16x3")
    else:
        check(lib.tcam_conv_wgrad_s3(arr, len(arr), B, dy.data_ptr(), *tail, _stream()),
              "tcam_conv_wgrad_s3")
