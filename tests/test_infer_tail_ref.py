"""CPU checks of tests/infer_tail_ref.py, the references and bounds of the inference tail's
kernel tests (tests/test_x_infer_tail_gpu.py): every reference pinned to torch's own fp64
operation or to oracle/model_ref.py; an emulation of each kernel in torch fp32, in the
kernel's order of operations, accepted at every case the GPU file runs; the checkers' teeth
(plausible wrong kernels must be rejected); and the conditions on the shared inputs: at most
0.5 % of the uint8 / argmax pixels undecided, no accidental ties, inputs representable in every
storage form.

One tooth the checker cannot have: heat applied with the 1e-6 omitted.  exp(t (c + 1e-6)) /
max exp(t (c + 1e-6)) = exp(t c) / max exp(t c): the constant cancels, and what is left of it
(the rounding of c + 1e-6) is rounding the bound has to allow.  The test below states that;
the heat's teeth are a missing t and a maximum taken over the wrong frame."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import infer_tail_ref as R
from oracle import model_ref as M

F32, F64 = torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")


def _ok(got, ref, bound):
    return R.nan_ratio(got, ref, bound) <= 1.0


def _tol(ref, scale=1.0):
    return 1e-13 * scale * (1.0 + ref.abs())


# -------------------------------------------------------------------------- pools
def emu_avgpool(x64, k, s, p, ceil, lay, clipped=False):
    """pool_s3_kernel mode 1: the in-frame taps added row-major in fp32, one division."""
    B, C, H, W = x64.shape
    x = x64.float()
    Ho, Wo = R.pool_out(H, k, s, p, ceil), R.pool_out(W, k, s, p, ceil)
    out = torch.zeros(B, C, Ho, Wo)
    for oy in range(Ho):
        hs = oy * s - p
        he = min(hs + k, H + p)
        for ox in range(Wo):
            ws = ox * s - p
            we = min(ws + k, W + p)
            acc = torch.zeros(B, C)
            n = 0
            for y in range(max(hs, 0), min(he, H)):
                for xx in range(max(ws, 0), min(we, W)):
                    acc = acc + x[:, :, y, xx]
                    n += 1
            out[:, :, oy, ox] = acc / np.float32(n if clipped else (he - hs) * (we - ws))
    return R.stored(out, lay)


@pytest.mark.parametrize("lay", R.LAYS[1:])
def test_pools_pinned_accepted_and_with_teeth(lay):
    seen_border = False
    for C, H, W, (k, s, p, mode, ceil) in R.pool_cases():
        x64 = R.stored(R.pool_input(2, C, H, W, seed=C + H + k), lay)
        if mode == "max":
            ref, bound = R.maxpool_ref(x64, k, s, p, ceil)
            # exact in fp32 too, and each window's largest tap by hand
            assert torch.equal(ref, F.max_pool2d(x64.float(), k, s, p, ceil_mode=ceil).double()
                               ) or lay == "s2"
            pad = F.pad(x64, (p, k, p, k), value=-INF)
            win = pad.unfold(2, k, s).unfold(3, k, s)[:, :, :ref.shape[2], :ref.shape[3]]
            assert torch.equal(ref, win.amax((4, 5))) and not bound.any()
            continue
        ref, bound = R.avgpool_ref(x64, k, s, p, ceil, lay)
        tor = F.avg_pool2d(x64, k, s, p, ceil_mode=ceil, count_include_pad=True)
        assert ref.shape == tor.shape and bool(((ref - tor).abs() <= _tol(ref)).all())
        assert _ok(emu_avgpool(x64, k, s, p, ceil, lay), ref, bound)
        wrong = emu_avgpool(x64, k, s, p, ceil, lay, clipped=True)
        if not torch.equal(wrong, emu_avgpool(x64, k, s, p, ceil, lay)):
            seen_border = True
            assert not _ok(wrong, ref, bound)
    assert seen_border


def test_maxpool_nan_reaches_exactly_its_windows():
    x = R.pool_input(2, 24, 13, 10, seed=3)
    x[1, 5, 6, 9] = NAN
    for k, s, p, ceil in [(3, 2, 1, False), (3, 1, 1, False), (2, 2, 0, False), (3, 2, 1, True)]:
        ref, _ = R.maxpool_ref(x.double(), k, s, p, ceil)
        hit = F.max_pool2d(torch.isnan(x).double(), k, s, p, ceil_mode=ceil) > 0
        assert torch.equal(torch.isnan(ref), hit) and 1 <= int(hit.sum()) <= 9
        clean = R.maxpool_ref(torch.nan_to_num(x, nan=-1e30).double(), k, s, p, ceil)[0]
        assert torch.equal(ref[~hit], clean[~hit])
        dropped = torch.where(hit, clean, ref)          # a maximum that drops NaN
        assert not _ok(dropped, ref, torch.zeros_like(ref))
        assert _ok(ref.clone(), ref, torch.zeros_like(ref))


# --------------------------------------------------------------------- resamplers
def _taps32(n_in, n_out, ac):
    i0, i1, l0, l1, _ = R.taps(n_in, n_out, ac)
    return i0, i1, l0.float(), l1.float()


def emu_blend(x, ty, tx, tap_err=0.0):
    """The four taps blended in fp32 in the kernels' order; tap_err: the wrong kernel (the
    weight of the second column tap off by that much)."""
    y0, y1, ly0, ly1 = ty
    x0, x1, lx0, lx1 = tx
    g = lambda yy, xx: x[..., yy[:, None], xx[None, :]]
    ly0, ly1 = ly0[:, None], ly1[:, None]
    lx1 = lx1 + np.float32(tap_err)
    return ly0 * (lx0 * g(y0, x0) + lx1 * g(y0, x1)) + ly1 * (lx0 * g(y1, x0) + lx1 * g(y1, x1))


def _torch_up2(x64, Ho, Wo):
    up = F.interpolate(x64, scale_factor=2, mode="nearest")
    return F.interpolate(up, size=(Ho, Wo), mode="bilinear", align_corners=True)


def _pos_tol(r, x64, extra=1.0):
    """What torch's fp64 positions may differ by from ATen's fp32 ones: the fp32 scale and the
    fp32 product (2 2^-24 r per axis) times the largest tap difference, 2 max |x|; the weights'
    own fp32 rounding, 2^-24 each."""
    return 2 * R.U * (2 * r + 4) * 2 * float(x64.abs().max()) * extra + 1e-13


@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("hw,out", R.UP2R_SHAPES)
def test_up2_resize_pinned_accepted_and_with_teeth(hw, out, lay):
    (H, W), (Ho, Wo) = hw, out
    for C in R.UP2R_C:
        x64 = R.stored(R.act_input(2, C, H, W, seed=C + H + Ho), lay)
        ref, bound, pos = R.up2_resize_ref(x64, Ho, Wo, lay)
        r = max(2 * H, 2 * W)
        assert bool(((ref - _torch_up2(x64, Ho, Wo)).abs() <= _pos_tol(r, x64)).all())
        up = x64.float().repeat_interleave(2, -2).repeat_interleave(2, -1)
        ty, tx = _taps32(2 * H, Ho, True), _taps32(2 * W, Wo, True)
        assert _ok(R.stored(emu_blend(up, ty, tx), lay), ref, bound)
        if W > 1 and lay in ("f32", "s3"):
            assert not _ok(R.stored(emu_blend(up, ty, tx, tap_err=1e-5), lay), ref, bound)
    if (hw, out) == ((7, 7), (14, 14)):
        assert torch.equal(ref, x64.repeat_interleave(2, -2).repeat_interleave(2, -1))
    if out == (1, 1):
        assert torch.equal(ref[..., 0, 0], x64[..., 0, 0])


def emu_up2_bwd(g64, H, W, lay):
    """up2_resize_bwd_kernel: acc += (wy wx) g over the outputs with a non-zero weight, fp32."""
    Ho, Wo = g64.shape[-2:]
    Wy, Wx = R.up2_matrix(H, Ho)[0].float(), R.up2_matrix(W, Wo)[0].float()
    g = g64.float()
    acc = torch.zeros(g.shape[0], g.shape[1], H, W)
    for oy in range(Ho):
        for ox in range(Wo):
            w = Wy[oy][:, None] * Wx[ox][None, :]
            acc = acc + w * g[:, :, oy, ox][:, :, None, None]
    return R.stored(acc, lay)


@pytest.mark.parametrize("lay", ["s3", "s1"])
@pytest.mark.parametrize("C", R.UP2R_C)
@pytest.mark.parametrize("hw,out", R.UP2R_BWD_SHAPES)
def test_up2_resize_bwd_is_the_adjoint_accepted_and_with_teeth(hw, out, C, lay):
    (H, W), (Ho, Wo) = hw, out
    g64 = R.stored(R.act_input(2, C, Ho, Wo, seed=C + H + Wo), lay)
    ref, bound, _ = R.up2_resize_bwd_ref(g64, H, W, lay)
    x = torch.randn(2, C, H, W, dtype=F64, requires_grad=True)
    (_torch_up2(x, Ho, Wo) * g64).sum().backward()
    n = Ho * Wo
    assert bool(((ref - x.grad).abs() <= _pos_tol(max(2 * H, 2 * W), g64, n)).all())
    # <up2(x), g> = <x, bwd(g)> with this module's own forward, to the weights' fp32 rounding
    fwd = R.up2_resize_ref(x.detach(), Ho, Wo, "s3")[0]
    lhs, rhs = (fwd * g64).sum(), (x.detach() * ref).sum()
    assert abs(float(lhs - rhs)) <= 4 * R.U * float((fwd.abs() * g64.abs()).sum()) + 1e-12
    assert _ok(emu_up2_bwd(g64, H, W, lay), ref, bound)
    if lay == "s3":
        short = g64.clone()
        short[..., -1, :] = 0            # the last output row not gathered
        assert not _ok(emu_up2_bwd(short, H, W, lay), ref, bound)


def emu_cam(a, argmax):
    """The CAM of fp32 fcams as the kernels compute it."""
    a0, a1 = a[:, 0], a[:, 1]
    if argmax:
        c = (a1 > a0).float()
    else:
        m = torch.maximum(a0, a1)
        e0, e1 = torch.exp(a0 - m), torch.exp(a1 - m)
        c = e1 / (e0 + e1)
    return torch.nan_to_num(c, nan=0.0, posinf=1.0, neginf=0.0)


def _u8_floor(cam):
    return (cam.double() * 255).floor().to(torch.uint8)


def _u8_round(cam):
    return (cam.double() * 255).round().to(torch.uint8)


def _check_u8(cam_emu, ref, bound, tag, teeth=True):
    """The 0.5 % cap from the reference alone; the emulation's floor passes, its round fails."""
    own, dec_ok, excl = R.u8_check(_u8_floor(cam_emu), cam_emu, ref, bound)
    assert excl <= R.U8_EXCLUDED_MAX, (tag, excl)
    assert own and dec_ok, tag
    if teeth:
        own, dec_ok, _ = R.u8_check(_u8_round(cam_emu), cam_emu, ref, bound)
        assert not own and not dec_ok, tag


@pytest.mark.parametrize("argmax", [False, True])
@pytest.mark.parametrize("hw,out", R.RESIZE_CAM_SHAPES)
def test_resize_cam_pinned_accepted_and_with_teeth(hw, out, argmax):
    (Hi, Wi), (Ho, Wo) = hw, out
    f = R.fcams_input(2, Hi, Wi, seed=Hi + Wo)
    ref = R.resize_cam_ref(f.double(), Ho, Wo, argmax)
    tor = F.interpolate(f.double(), size=(Ho, Wo), mode="bilinear", align_corners=True)
    assert bool(((ref["fcams"] - tor).abs() <= _pos_tol(max(Hi, Wi), f.double())).all())
    cam_t = M.segmentation_cam(ref["fcams"], argmax).double()
    assert bool(((ref["cam"] - cam_t).abs() <= 1e-15).all())
    a = emu_blend(f, _taps32(Hi, Ho, True), _taps32(Wi, Wo, True))
    assert _ok(a, ref["fcams"], ref["b_fcams"])
    cam = emu_cam(a, argmax)
    assert _ok(cam, ref["cam"], ref["b_cam"])
    _check_u8(cam, ref["cam"], ref["b_cam"], (hw, out, argmax), teeth=not argmax)
    if Wi > 1 and Wo != Wi:
        assert not _ok(emu_blend(f, _taps32(Hi, Ho, True), _taps32(Wi, Wo, True), 1e-5),
                       ref["fcams"], ref["b_fcams"])
    if argmax:      # no accidental ties: the undecided pixels are within the cap
        assert float((ref["b_cam"] > 0).double().mean()) <= R.U8_EXCLUDED_MAX


# --------------------------------------------------------------------------- WGAP
def _lanes_sum(v, lanes=64):
    """Sum over the last axis as a wave does: lanes striding it, then the xor butterfly."""
    n = v.shape[-1]
    pad = torch.zeros(*v.shape[:-1], -(-n // lanes) * lanes)
    pad[..., :n] = v
    acc = torch.zeros(*v.shape[:-1], lanes)
    for part in pad.view(*v.shape[:-1], -1, lanes).unbind(-2):
        acc = acc + part
    while acc.shape[-1] > 1:
        h = acc.shape[-1] // 2
        acc = acc[..., :h] + acc[..., h:]
    return acc[..., 0]


def emu_wgap(x64, w, b, lay, drop=False):
    B, C = x64.shape[:2]
    v = x64.float().reshape(B, C, -1)
    HW = v.shape[2]
    if lay == "f32":
        mean = _lanes_sum(v) / np.float32(HW)
    else:
        tot = torch.zeros(B, C)
        for p0 in range(0, HW, 32):
            part = torch.zeros(B, C)
            for p in range(p0, min(HW, p0 + 32) - (1 if drop and p0 == 0 else 0)):
                part = part + v[:, :, p]
            tot = tot + part
        mean = tot / np.float32(HW)
    logits = _lanes_sum(mean[:, None, :] * w[None]) + b
    return mean, logits


@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("B,C,HW,K", R.WGAP_SHAPES)
def test_wgap_pinned_accepted_and_with_teeth(B, C, HW, K, lay):
    c = R.wgap_input(B, C, HW, K, seed=C + HW)
    x64 = R.stored(c["x"], lay)
    ref = R.wgap_ref(x64, c["w"], c["b"], lay)
    mean_t = F.adaptive_avg_pool2d(x64, 1).flatten(1)
    assert bool(((ref["mean"] - mean_t).abs() <= _tol(mean_t)).all())
    logit_t = F.linear(mean_t, c["w"].double(), c["b"].double())
    assert bool(((ref["logits"] - logit_t).abs() <= _tol(logit_t, C)).all())
    mean, logits = emu_wgap(x64, c["w"], c["b"], lay)
    assert _ok(mean, ref["mean"], ref["b_mean"]) and _ok(logits, ref["logits"], ref["b_logits"])
    if HW == 784 and lay != "f32":
        mean, logits = emu_wgap(x64, c["w"], c["b"], lay, drop=True)
        assert not _ok(mean, ref["mean"], ref["b_mean"])
        assert not _ok(logits, ref["logits"], ref["b_logits"])


# ------------------------------------------------------------------------ seghead
@pytest.mark.parametrize("argmax", [False, True])
@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("B,Cin,H,W", R.SEG_SHAPES)
def test_seghead_pinned_accepted_and_with_teeth(B, Cin, H, W, lay, argmax):
    c = R.seg_input(B, Cin, H, W, seed=Cin + H)
    x64 = R.stored(c["x"], lay)
    ref = R.seghead_ref(x64, c["w"], c["b"], argmax)
    cam_t = M.segmentation_cam(F.conv2d(x64, c["w"].double(), c["b"].double(), padding=1),
                               argmax).double()
    assert bool(((ref["cam"] - cam_t).abs() <= 1e-15).all())
    a = F.conv2d(x64.float(), c["w"], c["b"], padding=1)
    assert _ok(a, ref["fcams"], ref["b_fcams"])
    cam = emu_cam(a, argmax)
    assert _ok(cam, ref["cam"], ref["b_cam"])
    _check_u8(cam, ref["cam"], ref["b_cam"], (B, Cin, H, W, lay, argmax), teeth=not argmax)
    if argmax:
        assert float((ref["b_cam"] > 0).double().mean()) <= R.U8_EXCLUDED_MAX
    elif H > 1:
        w = c["w"].clone()
        w[1, 0, 0, 1] = 0                 # one tap of one channel not read
        assert not _ok(F.conv2d(x64.float(), w, c["b"], padding=1), ref["fcams"], ref["b_fcams"])


def test_seghead_nan_input_zeroes_the_pixels_that_read_it():
    c = R.seg_input(2, 16, 20, 24, seed=36)
    x = c["x"].clone()
    x[1, 3, 0, 5] = NAN            # a top-edge pixel: six readers
    x[0, 9, 7, 7] = NAN            # an interior pixel: nine
    for argmax in (False, True):
        ref = R.seghead_ref(x.double(), c["w"], c["b"], argmax)
        nan = torch.isnan(ref["fcams"][:, 0])
        assert int(nan[1].sum()) == 6 and int(nan[0].sum()) == 9
        assert torch.equal(nan, torch.isnan(ref["fcams"][:, 1]))
        assert not ref["cam"][nan].any() and not ref["b_cam"][nan].any()
        assert not R.u8_of(ref["cam"])[nan].any()
        ora = M.segmentation_cam(F.conv2d(x, c["w"], c["b"], padding=1), argmax)
        assert not ora[nan].any() and not torch.isnan(ora).any()


# ------------------------------------------------------------------------ std_cam
def emu_std_cam(A64, w, cls, Ho, Wo, lay, ac=False, drop_nan=False):
    """std_cam_kernel / std_cam_s3_kernel in fp32; drop_nan: the min / max that drop NaN."""
    B, C, h, w_ = A64.shape
    lows = []
    for i in range(B):
        t = w[int(cls[i])][:, None, None] * A64[i].float()
        t = torch.where(torch.isnan(t), torch.zeros_like(t), t).reshape(C, -1)
        if lay == "f32":
            s = torch.zeros(h * w_)
            for ch in range(C):
                s = s + t[ch]
        else:
            s = _lanes_sum(t.t().reshape(h * w_, C // 8, 8).sum(-1))     # a lane per group
        if drop_nan:
            fin = s[~torch.isnan(s)]
            mn = fin.min()
            v = s - mn
            mx = v[~torch.isnan(v)].max()
        else:
            mn = s.min()
            v = s - mn
            mx = v.max()
        lows.append(torch.nan_to_num(v / mx, nan=0.0, posinf=1.0, neginf=0.0).reshape(h, w_))
    low = torch.stack(lows)
    cam = emu_blend(low, _taps32(h, Ho, ac), _taps32(w_, Wo, ac))
    return low, cam


def _oracle_std(A, w, cls, Ho, Wo):
    sd = {"classification_head.fc.weight": w}
    res = [M.std_cam(sd, A[i], int(cls[i]), (Ho, Wo)) for i in range(A.shape[0])]
    return torch.stack([r[0] for r in res]), torch.from_numpy(np.stack([r[1] for r in res]))


@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("C,h,w,Ho,Wo", R.STD_SHAPES)
def test_std_cam_pinned_accepted_and_with_teeth(C, h, w, Ho, Wo, lay):
    c = R.std_input(C, h, w, seed=C + h)
    A64 = R.stored(c["A"], lay)
    assert bool(torch.isfinite(A64).all())
    assert bool(((A64 - c["A"].double()).abs() <= R.out_storage(c["A"].double(), lay)).all())
    ref = R.std_cam_ref(A64, c["w"], c["cls"], Ho, Wo, lay)
    low_o, cam_o = _oracle_std(A64, c["w"].double(), c["cls"], Ho, Wo)
    assert bool(((ref["low"] - low_o).abs() <= 1e-13).all())
    assert bool(((ref["cam"] - cam_o).abs() <= _pos_tol(max(h, w), ref["low"])).all())
    low, cam = emu_std_cam(A64, c["w"], c["cls"], Ho, Wo, lay)
    assert _ok(low, ref["low"], ref["b_low"]) and _ok(cam, ref["cam"], ref["b_cam"])
    _check_u8(cam, ref["cam"], ref["b_cam"], (C, h, w, lay), teeth=h * w > 1)
    if h * w == 1:
        assert not ref["low"].any() and not ref["cam"].any() and not ref["b_cam"].any()
        return
    # no accidental ties: one pixel can be the minimum, one the maximum
    for i in range(2):
        t = c["w"][int(c["cls"][i])].double()[:, None, None] * A64[i]
        s = t.sum(0)
        e = 2 * C * R.U * t.abs().sum(0)
        assert int(R._near(s, e, True).sum()) == 1 and int(R._near(s, e, False).sum()) == 1
    if (h, w) != (Ho, Wo):
        swapped = emu_std_cam(A64, c["w"], c["cls"], Ho, Wo, lay, ac=True)[1]
        assert not _ok(swapped, ref["cam"], ref["b_cam"])


@pytest.mark.parametrize("lay,how", [(lay, "overflow") for lay in R.LAYS] +
                         [("f32", "inf"), ("s1", "inf")])
def test_std_cam_non_finite_follow_the_oracle(lay, how):
    C, h, w, Ho, Wo = 64, 7, 7, 28, 28
    c = R.std_input(C, h, w, seed=C + h)
    # one NaN feature element: nansum drops it, the map is that of the other 63 channels
    A = c["A"].clone()
    A[0, 4, 3, 3] = NAN
    A64 = R.stored(A, lay)
    ref = R.std_cam_ref(A64, c["w"], c["cls"], Ho, Wo, lay)
    low_o, cam_o = _oracle_std(A64, c["w"].double(), c["cls"], Ho, Wo)
    assert bool(torch.isfinite(ref["low"]).all()) and float(ref["low"][0].max()) == 1.0
    assert bool(((ref["low"] - low_o).abs() <= 1e-13).all())
    low, cam = emu_std_cam(A64, c["w"], c["cls"], Ho, Wo, lay)
    assert _ok(low, ref["low"], ref["b_low"]) and _ok(cam, ref["cam"], ref["b_cam"])
    # a pixel whose weighted sum is (+inf) + (-inf), from finite features by fp32 overflow or
    # from inf features where the form holds one: low.min() is NaN, the whole map of that frame
    # 0; the other frame is untouched
    A, fw = c["A"].clone(), c["w"].clone()
    k = int(c["cls"][0])
    big, val = (3e38, 4.0) if how == "overflow" else (1.5, INF)
    fw[k, 8], fw[k, 9] = big, -big
    A[0, 8:10] = 0
    A[0, 8:10, 2, 5] = val
    A64 = R.stored(A, lay)
    assert bool(torch.isfinite(A64).all()) == (how == "overflow")
    assert float(A64[0, 8, 2, 5]) == val
    ref = R.std_cam_ref(A64, fw, c["cls"], Ho, Wo, lay)
    low_o, cam_o = _oracle_std(A64.float(), fw, c["cls"], Ho, Wo)       # the oracle in fp32
    assert not low_o[0].any() and not cam_o[0].any() and bool(low_o[1].any())
    assert not ref["low"][0].any() and not ref["cam"][0].any() and not ref["b_cam"][0].any()
    low, cam = emu_std_cam(A64, fw, c["cls"], Ho, Wo, lay)
    assert _ok(low, ref["low"], ref["b_low"]) and _ok(cam, ref["cam"], ref["b_cam"])
    low, cam = emu_std_cam(A64, fw, c["cls"], Ho, Wo, lay, drop_nan=True)
    assert not _ok(low, ref["low"], ref["b_low"]) and not _ok(cam, ref["cam"], ref["b_cam"])


# ----------------------------------------------------------------------- temporal
def emu_temporal(cams, idx, t, heat=True, own_max=True, drop_nan=False, eps=True):
    """temporal_max_kernel / temporal_cam_kernel in fp32."""
    t32, e32 = np.float32(t), np.float32(1e-6 if eps else 0.0)
    M_, hw = len(idx), cams.shape[1]
    out = torch.zeros(M_, hw)
    E = torch.exp((cams + e32) * t32)
    for i, row in enumerate(idx):
        acc = None
        for f in row:
            if f < 0:
                continue
            v = cams[f]
            if t > 0 and heat:
                e = E[f]
                pool = e if own_max else E[[g for g in row if g >= 0]]
                mx = pool[~torch.isnan(pool)].max() if drop_nan else pool.max()
                v = torch.nan_to_num(e / mx, nan=0.0, posinf=1.0, neginf=0.0)
            if acc is None:
                acc = v
            elif drop_nan:
                acc = torch.fmax(acc, v)
            else:
                acc = torch.maximum(acc, v)
        if acc is not None:
            out[i] = acc
    return out


def _oracle_temporal(cams, idx, t):
    out = torch.zeros(len(idx), cams.shape[1], dtype=cams.dtype)
    for i, row in enumerate(idx):
        fr = [cams[f] for f in row if f >= 0]
        if fr:
            out[i] = M.temporal_max(fr, t=R.f32(t))
    return out


@pytest.mark.parametrize("t", R.TMP_T)
@pytest.mark.parametrize("k1", [1, 3])
@pytest.mark.parametrize("hw", R.TMP_FRAMES)
def test_temporal_pinned_accepted_and_with_teeth(hw, k1, t):
    cams = R.tmp_input(*hw, seed=hw[0] + k1)
    idx = R.TMP_IDX[k1] + [R.TMP_ABSENT_ROW[:k1]]
    ref, bound = R.temporal_ref(cams.double(), idx, t)
    ora = _oracle_temporal(cams.double(), idx, t)
    assert bool(((ref - ora).abs() <= 1e-12 * (1 + t)).all())
    assert not ref[-1].any() and not bound[-1].any()
    got = emu_temporal(cams, idx, t)
    assert _ok(got, ref, bound)
    _check_u8(got, ref, bound, (hw, k1, t), teeth=hw[0] * hw[1] > 4)
    if t == 0:
        assert not bound.any() and torch.equal(got.double(), ref)
        return
    # no accidental ties: each frame's largest CAM clears the runner-up by far more than the
    # argument's roundings, so e / max e is exactly 1 at one pixel
    top = cams.double().topk(min(2, cams.shape[1]), 1).values
    if top.shape[1] == 2:
        assert bool(((top[:, 0] - top[:, 1]) * t > 64 * R.U * t).all())
    # the 1e-6 cancels in e / max e: a kernel without it cannot be told apart (module docstring)
    assert _ok(emu_temporal(cams, idx, t, eps=False), ref, bound)
    assert not _ok(emu_temporal(cams, idx, t, heat=False), ref, bound)
    if k1 > 1:
        assert not _ok(emu_temporal(cams, idx, t, own_max=False), ref, bound)


@pytest.mark.parametrize("t", R.TMP_T)
def test_temporal_nan_pixel_follows_the_oracle(t):
    hw = (33, 40)
    cams = R.tmp_input(*hw, seed=7)
    cams[3, 517] = NAN
    idx = R.TMP_IDX[3]
    ref, bound = R.temporal_ref(cams.double(), idx, t)
    ora = _oracle_temporal(cams, idx, t)               # the oracle in fp32
    assert torch.equal(torch.isnan(ref), torch.isnan(ora))
    if t == 0:
        # the output pixel of every row that reads frame 3 is NaN, its u8 0
        assert [int(torch.isnan(r).sum()) for r in ref] == [0, 1, 0, 0, 0]
        assert bool(torch.isnan(ref[1, 517])) and int(R.u8_of(ref)[1, 517]) == 0
    else:
        # frame 3 contributes zeros everywhere: row 1 is the maximum of frames 2 and 4 alone
        assert not torch.isnan(ref).any()
        two, _ = R.temporal_ref(cams.double(), [[2, 4]], t)
        assert torch.equal(ref[1], two[0])
        assert float((ref.float() - ora).abs().max()) < 1e-5
    good = emu_temporal(cams, idx, t)
    assert _ok(good, ref, bound)
    assert not _ok(emu_temporal(cams, idx, t, drop_nan=True), ref, bound)   # a max that drops NaN


# --------------------------------------------------------------------------- top-k
def _rank_flags(logits, target, nan_first=True):
    """The rank of the target counted as topk_kernel does; nan_first False: the comparison
    that ignores NaN."""
    B, C = logits.shape
    t1, t5 = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        l, t = logits[b].tolist(), int(target[b])
        rank = 0
        for c_ in range(C):
            v, lt = l[c_], l[t]
            if nan_first and v != v:
                rank += (lt == lt) or c_ < t
            elif nan_first and lt != lt:
                rank += 0
            else:
                rank += (v > lt) or (v == lt and c_ < t)
        t1[b], t5[b] = rank == 0, rank < 5
    return t1, t5


def test_topk_reference_ranks_nan_first_and_ties_by_index():
    for name, (logits, target) in R.topk_cases().items():
        assert int(target.min()) >= 0 and int(target.max()) < logits.shape[1]
        r1, r5 = R.topk_ref(logits, target)
        sub = slice(0, 40)
        e1, e5 = _rank_flags(logits[sub], target[sub])
        assert torch.equal(r1[sub], e1) and torch.equal(r5[sub], e5), name
        if name == "C3":
            assert bool(r5.all())
        if name == "C1000":
            assert logits.shape[0] > 256 and 0 < int(r5.sum()) < 300
            assert bool((target[:100:2] == 0).all() and (target[1:100:2] == 999).all())
        if name == "ties":
            assert r1.tolist() == [0, 0, 1, 1] and r5.tolist() == [1, 0, 1, 1]
        if name == "nan":
            assert r1.tolist() == [1, 0, 0, 0, 0, 0] and r5.tolist() == [1, 1, 1, 0, 1, 0]
            w1, w5 = _rank_flags(logits, target, nan_first=False)
            assert not (torch.equal(w1, r1) and torch.equal(w5, r5))


# ------------------------------------------------------------ the inputs' storage
@pytest.mark.parametrize("lay", R.LAYS)
def test_inputs_are_representable_in_every_storage_form(lay):
    xs = [R.pool_input(2, 24, 13, 10, 1), R.act_input(2, 24, 5, 6, 2),
          R.wgap_input(2, 520, 37, 10, 3)["x"], R.seg_input(1, 64, 17, 33, 4)["x"]]
    for x in xs:
        s = R.stored(x, lay)
        assert bool(torch.isfinite(s).all())
        assert bool(((s - x.double()).abs() <= R.out_storage(x.double(), lay)).all())
        assert torch.equal(R.stored(s.float(), lay), s)          # storing twice changes nothing
    nan = torch.tensor([NAN, 1.0])
    assert bool(torch.isnan(R.stored(nan, lay)[0])) and float(R.stored(nan, lay)[1]) == 1.0
