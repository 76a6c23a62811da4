"""Stage-1 training of the VGG16 (WSOL16) ``STDClassifier`` on the gfx950 kernels: the
reference's ``Trainer._wsol_training`` for task STD_CL with ``--encoder_name vgg16
--freeze_encoder False`` (learning/train_wsol.py:700-714; encoders/vgg.py:61-161), the run
whose best weights a VGG16-TCAM run starts from.

Forward (train mode = the eval forward with every conv output kept): conv3x3 + bias + ReLU
on the MFMA conv kernels (no BatchNorm), ``MaxPool2d(2, 2)``, ``conv6`` 512 -> 1024, WGAP's
pool + fc.  Loss: ``nn.CrossEntropyLoss``.  Backward, per conv in reverse: the 2x2 max-pool
adjoint where a pool follows (``tcam_maxpool2x2_bwd_*``), the ReLU backward with the bias
gradient and the channel maxima (``tcam_relu_bwd_*``), the per-channel scaled S2 copy
(``tcam_dy_scaled_s2``; a channel that is dead on the whole batch — there is no BatchNorm to
revive it — gets scale 2^126, so its weight and bias gradients are exactly 0), the 3x3
weight gradient (``tcam_conv_wgrad_s2_f16x3`` / ``_s1``) and, for every conv but the first,
the data gradient as the forward conv of dy with the packed transposed weights.  Update:
torch.optim.SGD with the reference's two VGG groups (process/instantiators.py:736-807:
``encoder.features.*`` at ``lr``; ``encoder.conv6.*`` and ``classification_head.*`` at ``lr *
lr_classifier_ratio``), gated on the device as the ResNet50 step is.

Precision: ``prec="f16x3"`` (activations S2, gradients S3) or ``amp=True`` (S1 tensors, the
device GradScaler), as :class:`~.cl_training.ClassifierTrainer`: both are a
:class:`~.cl_training.Stage1Trainer`, so checkpoints, the lr schedule and the runner work on
either.

Every launch goes to the current stream (no side stream).  Every scratch buffer belongs to
one kernel and one geometry, is sized by that kernel's own ``*_ws_bytes`` query and is never
regrown or shared between differently shaped calls.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
import torch.nn as nn

from . import _lib, ops, train_ops
from ._lib import check
from .cl_training import Stage1Trainer, _stream
from .models import STDClassifier
from .ops import ConvSrc
from .train_ops import Grad, _p, pack_weight

VGG16 = "vgg16"


class _VConv:
    """One conv3x3 (pad 1, with bias) + ReLU of the stack, ``pool``: a MaxPool2d(2, 2)
    follows; ``wt`` / ``wsc`` the forward's packed operand, ``dwt`` / ``dsc`` the data
    gradient's, ``cin_pad``: the input's stored channels (8 for the image)."""

    __slots__ = ("name", "conv", "cout", "cin", "cin_pad", "pool", "wt", "wsc", "dwt", "dsc",
                 "bias16", "dw_pad")

    def __init__(self, name: str, conv: nn.Conv2d):
        self.name, self.conv = name, conv
        self.cout, self.cin = conv.out_channels, conv.in_channels
        self.cin_pad = (self.cin + 7) // 8 * 8
        self.pool = False
        self.wt = self.wsc = self.dwt = self.dsc = self.bias16 = self.dw_pad = None


def _is_conv3x3(m) -> bool:
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (1, 1) and
            m.padding == (1, 1) and m.dilation == (1, 1) and m.groups == 1 and
            m.bias is not None and m.out_channels % 8 == 0)


def _is_pool2x2(m) -> bool:
    def two(v):
        return v == 2 or v == (2, 2)
    return (isinstance(m, nn.MaxPool2d) and two(m.kernel_size) and two(m.stride) and
            m.padding in (0, (0, 0)) and m.dilation in (1, (1, 1)) and not m.ceil_mode)


def vgg_stack(model) -> List[_VConv]:
    """The conv stack of a VGG16 ``STDClassifier`` in forward order (``encoder.features`` then
    ``encoder.conv6``); raises when ``encoder.features`` is not the conv3x3-pad1 / ReLU /
    MaxPool2d(2, 2) WSOL16 layout."""
    enc = model.encoder
    bad = NotImplementedError("VGG16 stage-1 training runs the WSOL16 stack: conv3x3 pad 1 + "
                              "ReLU and MaxPool2d(2, 2) (encoders/vgg.py:146-161)")
    mods = list(enc.features.named_children())
    out: List[_VConv] = []
    i = 0
    while i < len(mods):
        k, m = mods[i]
        if _is_conv3x3(m):
            if i + 1 >= len(mods) or not isinstance(mods[i + 1][1], nn.ReLU):
                raise bad
            if m.in_channels != (out[-1].cout if out else 3):
                raise bad
            out.append(_VConv(f"encoder.features.{k}", m))
            i += 2
        elif _is_pool2x2(m) and out and not out[-1].pool:
            out[-1].pool = True
            i += 1
        else:
            raise bad
    conv6 = getattr(enc, "conv6", None)
    if not out or not _is_conv3x3(conv6) or conv6.in_channels != out[-1].cout:
        raise bad
    out.append(_VConv("encoder.conv6", conv6))
    return out


class VGG16ClassifierTrainer(Stage1Trainer):
    """Trains every parameter of a VGG16 ``STDClassifier`` (encoder + WGAP head)."""

    ENCODER = VGG16

    @staticmethod
    def param_split(model) -> int:
        """Elements of the first SGD group (named_parameters order: encoder.features.*, then
        encoder.conv6.* and the head — the reference's second group — as the tail;
        encoder.full_features.* are the same Parameters under a second name, which
        named_parameters lists once)."""
        split, tail = 0, False
        for name, p in model.named_parameters():
            if name.startswith("encoder.features."):
                if tail:
                    raise NotImplementedError("encoder.features.* must precede conv6 / the head")
                split += p.numel()
            else:
                tail = True
        return split

    def _build(self, model: STDClassifier) -> None:
        self.convs = vgg_stack(model)
        # scratch: one buffer per (kernel, geometry), sized by the kernel's own query
        self._ws: Dict[Tuple, torch.Tensor] = {}

    def _scratch(self, kernel: str, geom: Tuple, nbytes: int) -> torch.Tensor:
        """The scratch buffer of ``kernel`` at ``geom``: exactly ``nbytes`` (its own size
        query's answer for that geometry), allocated once."""
        nbytes = int(nbytes)
        if nbytes <= 0:
            raise ValueError(f"{kernel}: unsupported geometry {geom}")
        key = (kernel,) + tuple(geom)
        cur = self._ws.get(key)
        if cur is None:
            cur = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            self._ws[key] = cur
        elif cur.numel() != nbytes:
            raise RuntimeError(f"{kernel}{geom}: workspace query changed "
                               f"({cur.numel()} -> {nbytes} bytes)")
        return cur

    def repack(self):
        """The forward operands of every conv from the flat fp32 weights (AMP: and the
        fp16-rounded biases autocast gives a conv)."""
        self._packed_version = self.param_version()
        for c in self.convs:
            c.wt, c.wsc = pack_weight(c.conv.weight.data, self.fmt, 0, cin_pad=c.cin_pad,
                                      out=(c.wt, c.wsc))
            if self.amp:
                if c.bias16 is None:
                    c.bias16 = torch.empty(c.cout, device=self.dev, dtype=torch.float32)
                c.bias16.copy_(c.conv.bias.data.half())

    # ------------------------------------------------------------ forward
    def forward(self, images: torch.Tensor):
        """Train-mode forward: (cl_logits (B, K) fp32, state for :meth:`backward`)."""
        lib = _lib.load()
        f = self._images_s3(images)
        saved = []
        for c in self.convs:
            _, H, W, _ = ops.s3_dims(f)
            bias = c.bias16 if self.amp else c.conv.bias.data
            a = ops.conv2d_x6([ConvSrc(f)], c.wt, bias, c.cout, H, W, 3, 1, True, wscale=c.wsc)
            saved.append((f, a))
            if c.pool:
                if H < 2 or W < 2:
                    raise ValueError("input too small for the VGG16 pools")
                f = ops.pool2d_s3(a, 2, 2, 0, "max")
            else:
                f = a
        B, _, _, Cf = ops.s3_dims(f)
        logits, pooled = self._head_fwd(
            f, self._scratch("cls_pool", (B, Cf), lib.tcam_cls_pool_ws_bytes(B, Cf)))
        self.model.x_in = images
        return logits, {"convs": saved, "pooled": pooled, "feat": f}

    # ----------------------------------------------------------- backward
    def _relu_bwd(self, dout: torch.Tensor, a: torch.Tensor, db: torch.Tensor) -> Grad:
        """The gradient of one conv's ReLU: dz = dout [a > 0] (S3 / S1), the bias gradient into
        ``db``; f16x3: with its per-channel scaled S2 copy for the MFMA."""
        lib = _lib.load()
        B, H, W, Cc = ops.s3_dims(a)
        P = B * H * W
        ws = self._scratch("relu_bwd", (P, Cc), lib.tcam_relu_bwd_ws_bytes(P, Cc))
        dz = ops.lay_empty(self.glay, B, H, W, Cc, self.dev)
        amax = None if self.amp else torch.empty(Cc, device=self.dev, dtype=torch.int32)
        name = "tcam_relu_bwd_s1" if self.amp else "tcam_relu_bwd_s3s2"
        check(getattr(lib, name)(dout.data_ptr(), a.data_ptr(), dz.data_ptr(), db.data_ptr(),
                                 _p(amax), P, Cc, ws.data_ptr(), ws.numel(), _stream()), name)
        return Grad(dz, dz, None) if self.amp else train_ops.dy_scaled(dz, amax)

    def _pool_bwd(self, gout: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
        lib = _lib.load()
        B, H, W, Cc = ops.s3_dims(a)
        _, Ho, Wo, _ = ops.s3_dims(gout)
        gin = ops.lay_empty(self.glay, B, H, W, Cc, self.dev)
        name = "tcam_maxpool2x2_bwd_s1" if self.amp else "tcam_maxpool2x2_bwd_s3s2"
        check(getattr(lib, name)(gout.data_ptr(), a.data_ptr(), gin.data_ptr(), B, Cc, H, W, Ho,
                                 Wo, _stream()), name)
        return gin

    def _wgrad(self, c: _VConv, x: torch.Tensor, g: Grad) -> None:
        """The 3x3 weight gradient of ``c`` on input ``x`` into the flat gradient buffer."""
        B, H, W, Cx = ops.s3_dims(x)
        arr = train_ops.conv_srcs([ConvSrc(x)])
        ws = self._scratch("conv_wgrad", (B, Cx, c.cout, H, W),
                           train_ops.conv_wgrad_ws_bytes(arr, g, self.fmt, 3, 1))
        gw = self.g(c.conv.weight)
        dw = gw
        if Cx != c.cin:   # the image padded to 8 channels: only the real ones are kept
            if c.dw_pad is None:
                c.dw_pad = torch.empty((c.cout, Cx, 3, 3), device=self.dev, dtype=torch.float32)
            dw = c.dw_pad
        train_ops.conv_wgrad(arr, g, dw, ws, self.fmt, 3, 1)
        if dw is not gw:
            gw.copy_(dw[:, :c.cin])

    def _dgrad(self, c: _VConv, g: Grad, H: int, W: int) -> torch.Tensor:
        """d loss / d (the input of ``c``): the stride-1 conv of dy's MFMA copy with the
        transposed, rotated weight (divided by dy's scales on the f16x3 path)."""
        c.dwt, c.dsc = pack_weight(c.conv.weight.data, self.fmt, 1, sel=c.cin, kdiv=g.scale,
                                   out=(c.dwt, c.dsc))
        zero = self._zeros(c.cin)
        if self.amp:
            return ops.conv2d_x6([ConvSrc(g.op)], c.dwt, zero, c.cin, H, W, 3, 1, False)
        return ops.conv2d_f16x3_s3out([ConvSrc(g.op)], c.dwt, c.dsc, zero, c.cin, H, W, 3, 1)

    def backward(self, dlogits: torch.Tensor, st) -> None:
        """Gradients of every parameter into the flat buffer from d loss / d logits."""
        dout = self._head_bwd(dlogits.contiguous().float(), st["feat"], st["pooled"])
        for i in range(len(self.convs) - 1, -1, -1):
            c = self.convs[i]
            x, a = st["convs"][i]
            if c.pool:
                dout = self._pool_bwd(dout, a)
            g = self._relu_bwd(dout, a, self.g(c.conv.bias))
            self._wgrad(c, x, g)
            if i == 0:
                break   # the image needs no gradient
            _, H, W, _ = ops.s3_dims(x)
            dout = self._dgrad(c, g, H, W)
