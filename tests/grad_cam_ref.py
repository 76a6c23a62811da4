"""fp64 references, elementwise bounds, shapes and input builders of the gradient CAM family
(GradCam, GradCAMpp, XGradCAM, LayerCAM on the WGAP classifier): tests/test_grad_cam_ref.py on
the CPU, tests/test_x_grad_cam_gpu.py and tests/test_grad_cam_gpu_model.py on the device.

The method is written twice: :func:`autograd_low` literally after dlib/cams/gradcam.py (torch
autograd through AdaptiveAvgPool2d(1) + Linear on a given hooked activation, the hooked
gradient, each method's ``_get_weights``, core.py's nansum / ReLU / in-place normalisation),
and :func:`closed_weights` / :func:`closed_low`, the closed form the kernels compute: the
hooked gradient is g[k] = W[c, k] / hw at every position, so
    GradCam w = g;  GradCAMpp w = hw g^2 relu(g);  XGradCAM w = g S / S, S = sum_p A[p]
    (NaN where S is 0, NaN or infinite: nansum drops the channel);  LayerCAM w = relu(g).

:func:`grad_cam_ref` is the kernels' reference in the conventions of tests/infer_tail_ref.py
(whose helpers it uses): it takes the features as the device stored them and returns the fp64
maps and their per-element bounds, n 2^-24 (sum of the magnitudes of the terms) with n the
fp32 roundings on the kernel's longest path.  No bound is taken from a kernel's output.
Plain torch, CPU only."""
import numpy as np
import torch

import infer_tail_ref as R
from infer_tail_ref import FLT_MAX, U, _near, blend, taps

METHODS = ["GradCam", "GradCAMpp", "XGradCAM", "LayerCAM"]
METHOD_ID = {m: i for i, m in enumerate(METHODS)}        # TCAM_GRAD_* of include/tcam_hip.h
GOLDEN_TOL = 5e-6      # fp64 method vs the reference's fp32 maps (2048-channel fp32 sums)


def hook_gradient(wrow, hw):
    """fp32(W[c] / hw), the gradient the reference's backward hook sees at every position
    (bit-identical in the goldens), as fp64."""
    return (wrow.float() / np.float32(hw)).double()


# ------------------------------------------------------------ the method, written twice
def autograd_low(A64, W64, c, method, normalized=True):
    """gradcam.py on one frame's hooked activation A64 (C, h, w) in fp64: scores through
    AdaptiveAvgPool2d(1) + Linear (no bias: it has no gradient), ``scores[:, c].sum()``
    back-propagated to the hook, the method's ``_get_weights``, then core.py:177-193."""
    hook_a = A64[None].clone().requires_grad_(True)
    scores = torch.nn.functional.adaptive_avg_pool2d(hook_a, 1).flatten(1) @ W64.t()
    hook_g, = torch.autograd.grad(scores[:, c].sum(), hook_a)
    hook_a = hook_a.detach()
    if method == "GradCam":
        weights = hook_g.squeeze(0).flatten(1).mean(-1)
    elif method == "GradCAMpp":
        grad_2 = hook_g.pow(2)
        grad_3 = grad_2 * hook_g
        denom = 2 * grad_2 + (grad_3 * hook_a).flatten(2).sum(-1)[(...,) + (None,) * 2]
        nan_mask = grad_2 > 0
        alpha = grad_2
        alpha[nan_mask].div_(denom[nan_mask])        # acts on a copy, as in the reference
        weights = alpha.squeeze_(0).mul_(torch.relu(hook_g.squeeze(0))).flatten(1).sum(-1)
    elif method == "XGradCAM":
        weights = (hook_g * hook_a).squeeze(0).flatten(1).sum(-1) / \
            hook_a.squeeze(0).flatten(1).sum(-1)
    else:
        assert method == "LayerCAM", method
        weights = torch.relu(hook_g).squeeze(0)
    missing = hook_a.ndim - weights.ndim - 1
    weights = weights[(...,) + (None,) * missing]
    cam = torch.relu(torch.nansum(weights * hook_a.squeeze(0), dim=0))
    if normalized:
        cam = cam - cam.min()
        cam = cam / cam.max()
    return cam


def closed_weights(A64, g64, method):
    """The per-channel weights in closed form from the hooked gradient g64 (C,)."""
    hw = A64.shape[1] * A64.shape[2]
    if method == "GradCam":
        return g64
    if method == "GradCAMpp":
        return hw * g64 * g64 * torch.relu(g64)
    if method == "LayerCAM":
        return torch.relu(g64)
    assert method == "XGradCAM", method
    S = A64.flatten(1).sum(1)
    return (g64 * S) / S


def closed_low(A64, g64, method, normalized=True):
    cam = torch.relu(torch.nansum(closed_weights(A64, g64, method)[:, None, None] * A64, 0))
    if normalized:
        cam = cam - cam.min()
        cam = cam / cam.max()
    return cam


def final_low(low):
    """What the store keeps (inference_wsol.py:1093): nan_to_num(0, 1, 0) of the map."""
    return torch.nan_to_num(low, nan=0.0, posinf=1.0, neginf=0.0)


# ------------------------------------------------------------------- the kernels' reference
def _overflow(t):
    """fp32 overflow of a product formed in fp64."""
    return torch.where(t.abs() > FLT_MAX, torch.sign(t) * float("inf"), t)


def weights_ref(A64, wrow, method, lay, exps=None):
    """The device's channel weights of one frame from the stored features A64 (C, h, w) (times
    2^exps per channel when ``exps``) and the true fc row: the fp64 value (products beyond
    FLT_MAX as +-inf, like fp32) and its bound.  g = W / hw is one rounded division (1);
    GradCam and LayerCAM copy it: 1 2^-24 |w|; GradCAMpp squares, multiplies by relu(g) and by
    hw, each on a g within 2^-24: (3 + 3) 2^-24 |w|; XGradCAM (g S) / S: the product and the
    quotient (S itself cancels, whatever its own rounding): 3 2^-24 |w|, NaN where S is 0, NaN
    or infinite.  The 2^-exps factor is exact."""
    hw = A64.shape[1] * A64.shape[2]
    g = hook_gradient(wrow, hw)
    if method == "XGradCAM":
        S = _overflow(A64.flatten(1).sum(1))
        w = _overflow(g * S) / S
        n = 3
    elif method == "GradCAMpp":
        w = _overflow(hw * _overflow(_overflow(g * g) * torch.relu(g)))
        n = 6
    else:
        w = g if method == "GradCam" else torch.relu(g)
        n = 1
    if exps is not None:
        w = w * torch.pow(2.0, -exps.double())
    b_w = n * U * torch.nan_to_num(w, nan=0.0, posinf=0.0, neginf=0.0).abs()
    return w, b_w


def grad_cam_ref(A64, fc_w, cls, Ho, Wo, lay, method, exps=None):
    """Per frame: s = relu(nansum_k w_k A_k) with :func:`weights_ref`'s weights, then std_cam's
    tail (tests/infer_tail_ref.py std_cam_ref, whose accounting this repeats): low = (s - min)
    / max(s - min); nan_to_num; cam = bilinear(align_corners=False).
    s: the summation's roundings as std_cam's (layouts 16 ceil(G / 64) products and additions
    per lane and 6 wave levels; plain 2 per term that is not an exact zero) on sum |w A|, plus
    the weights' own bounds carried through, sum b_w |A|; the ReLU moves nothing further
    (|relu a - relu b| <= |a - b|).  A position whose sum is certainly <= 0 (sum + e_s <= 0)
    is clamped to exactly 0 on both sides; where there is one, 0 is the minimum on both sides
    and s - 0 rounds nothing.  A map clamped everywhere (a class row that is <= 0) is 0 / 0 ->
    0 exactly, as is one position; a NaN or infinite min / max zeroes the whole map."""
    B, C, h, w_ = A64.shape
    G = C // 8
    lows, b_lows = [], []
    for i in range(B):
        wk, b_wk = weights_ref(A64[i], fc_w[int(cls[i])], method, lay, exps)
        t = _overflow(wk[:, None, None] * A64[i])
        raw = torch.nansum(t, 0)
        s = torch.relu(raw)
        fin = torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0).abs()
        # (a NaN term — a dropped channel — is skipped, not added: it rounds nothing either)
        n = 2 * ((t != 0) & ~torch.isnan(t)).sum(0) if lay == "f32" else 16 * -(-G // 64) + 6
        a_fin = torch.nan_to_num(A64[i], nan=0.0, posinf=0.0, neginf=0.0).abs()
        e_s = n * U * fin.sum(0) + (b_wk[:, None, None] * a_fin).sum(0)
        clamped = torch.isfinite(raw) & (raw + e_s <= 0)
        e_s = torch.where(clamped, torch.zeros_like(e_s), e_s)
        mn = s.min()
        v = s - mn
        mx = v.max()
        if not bool(torch.isfinite(mn) & torch.isfinite(mx)) or h * w_ == 1 or \
                bool(clamped.all()):
            lows.append(torch.nan_to_num(v / mx, nan=0.0, posinf=1.0, neginf=0.0))
            b_lows.append(torch.zeros_like(s))
            continue
        assert float(mx) > 0, "a map that is zero in the reference but not certainly on the device"
        lo_set = _near(s, e_s, True)
        if bool(clamped.any()):
            e_v = e_s.clone()
        else:
            e_v = e_s + e_s[lo_set].max() + U * v.abs()
        hi_set = _near(v, e_v, False)
        e_mx = e_v[hi_set].max()
        low = v / mx
        b_low = (e_v + low * e_mx) / mx + U * low
        if int(lo_set.sum()) == 1:
            b_low[lo_set] = 0.0
        if int(hi_set.sum()) == 1:
            b_low[hi_set] = 0.0
        lows.append(low)
        b_lows.append(b_low)
    low, b_low = torch.stack(lows), torch.stack(b_lows)
    cam, mag, pos, e = blend(low, taps(h, Ho, False), taps(w_, Wo, False), b_low)
    return dict(low=low, b_low=b_low, cam=cam, b_cam=e + 5 * U * mag + pos, pos=pos)


# ------------------------------------------------------------------ shapes and inputs
# (C, h, w, Ho, Wo), B = 2 frames of classes (1, 3) of 5.  The weights kernel: a thread per
# (frame, channel); XGradCAM's sums: layouts a thread per group over chunks of 32 positions,
# plain a wave per plane; the map: std_cam's kernel (a block of 1024 threads per frame).
SHAPES = [
    (64, 7, 7, 28, 28),         # G 8: 56 idle lanes; two chunks, the second of 17 positions
    (520, 3, 5, 12, 20),        # G 65: one group past a wave; one chunk of 15
    (8, 1, 1, 5, 5),            # one position: 0 / 0 gives an all-zero map
    (2048, 7, 7, 224, 224),     # G 256, the ResNet50 hook at 224^2
    (8, 64, 64, 32, 32),        # h w = 4096, the LDS limit: 128 chunks, 64 per lane (plain)
]
REFUSED = R.STD_REFUSED         # h w = 4097
CLS = R.STD_CLS
KINDS = ["dead", "nonpos_row", "mixed_row", "negative_features"]


def gpu_input(C, h, w, kind, seed=None):
    """R.std_input's sparse post-ReLU features and mostly positive class rows, then:
    dead: every fourth channel of frame 0 and every fifth of frame 1 all zero (XGradCAM's 0 / 0
    is dropped); nonpos_row: frame 0's class row <= 0 everywhere, with exact zeros (LayerCAM and
    GradCAM++ give an all-zero map, GradCam and XGradCAM relu of a negative sum);
    mixed_row: both rows of mixed sign, half and half; negative_features: a tenth of the
    features negated, the channel sums staying well away from 0."""
    c = R.std_input(C, h, w, seed=(C + h) if seed is None else seed)
    A, fw = c["A"].clone(), c["w"].clone()
    g = torch.Generator().manual_seed(17 + C + h)
    if kind == "dead":
        A[0, ::4] = 0
        A[1, 1::5] = 0
    elif kind == "nonpos_row":
        fw[CLS[0]] = -fw[CLS[0]].abs()
        fw[CLS[0], ::3] = 0
    elif kind == "mixed_row":
        sign = torch.where(torch.rand(fw.shape, generator=g) < 0.5, -1.0, 1.0)
        fw = fw.abs() * sign
    else:
        assert kind == "negative_features", kind
        A = A * torch.where(torch.rand(A.shape, generator=g) < 0.1, -1.0, 1.0)
    return dict(A=A, w=fw, cls=c["cls"])


# every kind at the two small multi-group shapes; at the others the kinds that reach a new path
CASES = [(s, k) for s in SHAPES[:2] for k in KINDS] + [
    (SHAPES[2], "dead"), (SHAPES[3], "dead"), (SHAPES[3], "mixed_row"),
    (SHAPES[4], "dead"), (SHAPES[4], "negative_features")]


def nan_feature_input():
    """One NaN feature element in a live channel of frame 0 (dropped: by nansum, and under
    XGradCAM with its whole channel, whose sum is NaN)."""
    C, h, w, Ho, Wo = SHAPES[0]
    c = gpu_input(C, h, w, "dead")
    c["A"][0, 5, 3, 3] = float("nan")
    return c, (Ho, Wo)


def nan_position_input():
    """Two channels of frame 0 alive at one position only, with class weights +-3e38: the
    weighted sum there overflows fp32 to (+inf) + (-inf) = NaN (GradCam, XGradCAM) or to +inf
    (LayerCAM, GradCAM++, whose ReLU removes the negative weight), so the minimum or the
    maximum is not finite and the whole map is 0; the other frame is untouched."""
    C, h, w, Ho, Wo = SHAPES[0]
    c = gpu_input(C, h, w, "dead")
    k = int(c["cls"][0])
    c["w"][k, 9], c["w"][k, 10] = 3e38, -3e38
    c["A"][0, 9:11] = 0
    c["A"][0, 9:11, 2, 5] = 100.0
    return c, (Ho, Wo)


def exps_input(C):
    """Per-channel exponents as the f16x3 plans give them: 0 .. 6, a third of them 0."""
    e = (torch.arange(C) * 5) % 9 - 2
    return e.clamp(min=0).to(torch.int32)
