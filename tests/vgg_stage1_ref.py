"""TEST INFRASTRUCTURE ONLY (a helper, not collected) — plain-torch restatement of one
stage-1 STD_CL step of the VGG16 classifier (learning/train_wsol.py:700-714 with
``--encoder_name vgg16 --freeze_encoder False``): the WSOL16 stack (encoders/vgg.py:61-161:
``F.conv2d`` + bias, ReLU, ``MaxPool2d(2, 2)``; conv6 512 -> 1024), WGAP
(poolings/core.py:109-115), ``nn.CrossEntropyLoss`` and ``torch.optim.SGD`` over the
reference's two parameter groups (``encoder.features.*`` at lr, ``encoder.conv6.*`` and
``classification_head.*`` at lr * lr_classifier_ratio).  fp64 by default.

"Mask-exact" mode: ``masks`` fixes every ReLU's branch and ``pool_idx`` every pool window's
chosen element to what the device forward under test took, so the reference differentiates
the SAME piecewise-linear function (a pre-activation within fp32 rounding of 0, or two
window entries within rounding of each other, would otherwise move a gradient
discontinuously — not a kernel error).

``amp=True`` inserts autocast's fp16 rounding points (``oracle.train_ref.r16``: value and
gradient rounded to fp16): conv inputs / weights / biases / outputs, the pooled vector, the
fc operands and the logits; the loss is scaled by the GradScaler scale before the backward and
the gradients are divided by it.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle.train_ref import r16

# encoders/vgg.py:47-58
WSOL16 = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, 512, 512, 512]


def conv_names() -> List[Tuple[str, bool]]:
    """[(parameter prefix of a conv, a MaxPool2d(2, 2) follows it)] in forward order."""
    out, idx = [], 0
    for v in WSOL16:
        if v == "M":
            out[-1] = (out[-1][0], True)
            idx += 1
        else:
            out.append((f"encoder.features.{idx}", False))
            idx += 2   # conv, relu
    out.append(("encoder.conv6", False))
    return out


def param_keys(sd) -> List[str]:
    """The model's parameters in ``named_parameters`` order (``full_features`` re-registers
    the same modules: its state_dict keys are duplicates, not parameters)."""
    return [k for k in sd if not k.startswith("encoder.full_features.")]


def param_groups(keys) -> Tuple[List[str], List[str]]:
    feat = [k for k in keys if k.startswith("encoder.features.")]
    return feat, [k for k in keys if k not in feat]


def vgg16_features(p: Dict[str, torch.Tensor], x: torch.Tensor,
                   masks: Optional[Dict[str, torch.Tensor]] = None,
                   pool_idx: Optional[Dict[str, torch.Tensor]] = None,
                   amp: bool = False) -> torch.Tensor:
    """``masks`` {conv prefix: bool NCHW, the conv's output > 0}; ``pool_idx`` {conv prefix:
    int64 (B, C, H/2, W/2), ``max_pool2d(..., return_indices=True)``'s flat indices of the
    pool after that conv}."""
    q = r16 if amp else (lambda t: t)
    f = x
    for name, pool in conv_names():
        z = q(F.conv2d(q(f), q(p[name + ".weight"]), q(p[name + ".bias"]), padding=1))
        f = q(z * masks[name].to(z.dtype)) if masks is not None else q(F.relu(z))
        if pool:
            if pool_idx is not None:
                idx = pool_idx[name]
                f = f.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
            else:
                f = F.max_pool2d(f, 2, 2)
    return f


def vgg16_stdcl_step(sd: Dict[str, torch.Tensor], x: torch.Tensor, labels: torch.Tensor,
                     lr=0.001, lr_classifier_ratio=10.0, momentum=0.9, dampening=0.0,
                     weight_decay=1e-4, nesterov=True, cl_lambda=1.0, dtype=torch.float64,
                     masks=None, pool_idx=None, amp: bool = False, scale: float = 2.0 ** 16):
    """Returns (loss, logits, grads, new_params, (group-0 names, group-1 names), group lrs)."""
    keys = param_keys(sd)
    params = {k: sd[k].detach().clone().to(dtype).requires_grad_(True) for k in keys}
    q = r16 if amp else (lambda t: t)
    f = vgg16_features(params, x.to(dtype), masks, pool_idx, amp)
    pooled = q(F.adaptive_avg_pool2d(f, 1).flatten(1))
    logits = q(F.linear(q(pooled), q(params["classification_head.fc.weight"]),
                        q(params["classification_head.fc.bias"])))
    loss = cl_lambda * F.cross_entropy(logits, labels.long(), reduction="mean")
    if amp:   # scaler.scale(loss).backward(); scaler.unscale_(optimizer)
        (loss * scale).backward()
        for k in keys:
            params[k].grad /= scale
    else:
        loss.backward()
    grads = {k: params[k].grad.detach().clone() for k in keys}
    feat, cls = param_groups(keys)
    opt = torch.optim.SGD([{"params": [params[k] for k in feat], "lr": lr},
                           {"params": [params[k] for k in cls],
                            "lr": lr * lr_classifier_ratio}],
                          lr=lr, momentum=momentum, dampening=dampening,
                          weight_decay=weight_decay, nesterov=nesterov)
    opt.step()
    new = {k: params[k].detach().clone() for k in keys}
    return (float(loss.detach()), logits.detach(), grads, new, (feat, cls),
            [g["lr"] for g in opt.param_groups])
