"""Direct fp64 checks of the gradient chain of the fp32-accurate (f16x3) training steps, kernel
by kernel: the BN-ReLU backward in every variant (unfused with / without the channel maxima,
fused with the bound-derived scale, the AMP form), the per-channel scaled S2 copy, the
data gradient (tcam_pack_weight_f16x3 mode 1 with kdiv + tcam_conv2d_f16x3_s3out) and the
weight gradients that read that copy, and the SGD / GradScaler kernels.  Every reference is
plain torch fp64 on the operands as the device stored them (activations read back with
ops.s3_to_nchw; mean, invstd, gamma, beta the same fp32 values on both sides), and every
bound is taken on the sum of magnitudes of the operation, so cancellation cannot hide an
error."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import train_ref as T
from tcam_wsol_video_amd import _lib, ops
from tcam_wsol_video_amd.ops import ConvSrc
from sgd_ref import LR, SGD_CFGS, sgd_ref, ulp
from test_gpu_enc_train import _act, _frames, _masks, _nchw, _norm_rel, _st

pytestmark = pytest.mark.gpu

EPS = 1e-5


# ---------------------------------------------------------------- BN-ReLU backward
def _bn_case(cuda, B, C, H, W, dmag, seed, lay="s2", outlier=False, dead=(), dead_how=None):
    """Inputs of one BN-ReLU backward, stored on the device: y and out = the forward kernel's
    relu(bn(y)) in the activation layout ``lay`` (S2, or S1 with an S1 dout), dout S3 with the
    per-channel spread logspace(-2, 2, C) * dmag.  ``outlier``: one pixel per channel at
    ~50 sigma.  ``dead`` channels get no gradient: every pixel masked (beta = -50), gamma = 0
    exactly, or a zero dout channel."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, C, H, W, generator=g) * (torch.rand(C, generator=g) + 0.5)[None, :, None, None] \
        + torch.randn(C, generator=g)[None, :, None, None]
    if outlier:
        idx = torch.randint(0, B * H * W, (C,), generator=g)
        yv = y.permute(1, 0, 2, 3).reshape(C, -1)
        yv[torch.arange(C), idx] += 50.0 * yv.std(dim=1)
        y = yv.view(C, B, H, W).permute(1, 0, 2, 3).contiguous()
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    dout = torch.randn(B, C, H, W, generator=g) * dmag * \
        torch.logspace(-2, 2, C)[None, :, None, None]
    dead = list(dead)
    if dead_how == "beta":
        beta[dead] = -50.0
    elif dead_how == "gamma":
        gamma[dead] = 0.0
        beta[dead] = beta[dead].abs() + 0.1   # the ReLU passes: only gamma = 0 kills dy
    elif dead_how == "dout":
        dout[:, dead] = 0.0
    afmt, gfmt = ("amp", "amp") if lay == "s1" else ("f16x3", "x6")
    ys, ds = _act(y, cuda, afmt), _act(dout, cuda, gfmt)
    y64 = _nchw(ys)
    mean = y64.mean((0, 2, 3)).float()
    invstd = (1.0 / torch.sqrt(y64.var((0, 2, 3), unbiased=False) + EPS)).float()
    c = dict(B=B, C=C, H=H, W=W, P=B * H * W, lay=lay, y=ys, dout=ds, y64=y64, d64=_nchw(ds))
    for k, v in (("mean", mean), ("invstd", invstd), ("gamma", gamma), ("beta", beta)):
        c[k] = v.to(cuda).contiguous()
    c["out"] = _bn_fwd(c)
    c["mask"] = _nchw(c["out"]) > 0
    return c


def _bn_fwd(c):
    out = torch.empty_like(c["y"])
    fn = getattr(_lib.load(), f"tcam_bn_relu_{c['lay']}")
    assert fn(c["y"].data_ptr(), c["mean"].data_ptr(), c["invstd"].data_ptr(),
              c["gamma"].data_ptr(), c["beta"].data_ptr(), out.data_ptr(), c["P"], c["C"],
              _st()) == 0
    return out


def _bn_ref(c):
    """fp64: g = dout mask, dbeta = sum g, dgamma = sum g xh, dy = gamma invstd (g - mean g -
    xh mean(g xh)), xh = (y - mean) invstd; with the magnitude sums of each."""
    v = lambda k: c[k].double().cpu()[None, :, None, None]
    xh = (c["y64"] - v("mean")) * v("invstd")
    g = c["d64"] * c["mask"]
    n = float(c["P"])
    db, dg = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    mg, mq = (db / n)[None, :, None, None], (dg / n)[None, :, None, None]
    k = v("gamma") * v("invstd")
    return dict(dy=k * (g - mg - xh * mq), dgamma=dg, dbeta=db, g=g, xh=xh, mg=mg, mq=mq, k=k,
                mag_dy=k.abs() * (g.abs() + mg.abs() + xh.abs() * mq.abs()),
                mag_dg=(g * xh).abs().sum((0, 2, 3)), mag_db=g.abs().sum((0, 2, 3)))


def _ratio(err, bound):
    """max err / bound (0 where both are 0; inf where only the bound is)."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def _check_sums(ref, dgamma, dbeta, tag):
    rg = _ratio((dgamma.double().cpu() - ref["dgamma"]).abs(), 1e-6 * ref["mag_dg"])
    rb = _ratio((dbeta.double().cpu() - ref["dbeta"]).abs(), 1e-6 * ref["mag_db"])
    print(f"{tag}: dgamma {rg:.3g} dbeta {rb:.3g} of the bound")
    assert rg <= 1.0 and rb <= 1.0, (tag, rg, rb)


def _check_dy(ref, dy64, tag, extra=None):
    bound = 1e-6 * ref["mag_dy"] + (0 if extra is None else extra)
    err = (dy64 - ref["dy"]).abs()
    r = _ratio(err, bound)
    print(f"{tag}: dy {r:.3g} of the bound")
    assert torch.isfinite(dy64).all(), tag
    if not r <= 1.0:   # the worst element's terms, for the failure message
        i = int(torch.where(err == 0, torch.zeros_like(err), err / bound).argmax())
        at = {k: float(ref[k].expand_as(err).flatten()[i]) for k in ("dy", "g", "xh", "mg", "mq", "k")}
        at.update(got=float(dy64.flatten()[i]), index=np.unravel_index(i, tuple(err.shape)))
        raise AssertionError((tag, r, at))


def _check_scaled(dy64, dy2, scale, tag):
    """scale an exact power of two, max |dy2_c| < 2^15, |dy2 / scale - dy| <= 2^-21 |dy| +
    2^-24 / scale (the S2 split leaves half an ulp of the low part: 2^-22 of the value while
    the low part is normal, 2^-25 absolute in scaled units below; one bit of margin each).
    Returns the largest 2^15 / max |dy2_c| over the channels with a gradient."""
    sc = scale.double().cpu()
    assert torch.equal(torch.frexp(sc)[0], torch.full_like(sc, 0.5)), tag
    d2 = _nchw(dy2)
    amax = d2.abs().amax((0, 2, 3))
    assert (amax < 2.0 ** 15).all(), (tag, float(amax.max()))
    s = sc[None, :, None, None]
    r = _ratio((d2 / s - dy64).abs(), 2.0 ** -21 * dy64.abs() + 2.0 ** -24 / s)
    assert r <= 1.0, (tag, r)
    live = amax > 0
    slack = float((2.0 ** 15 / amax[live]).max()) if live.any() else 0.0
    print(f"{tag}: scaled copy {r:.3g} of the bound, 2^15 / max|dy2_c| up to {slack:.3g}")
    return slack


def _bwd_unfused(c, want_amax):
    lib = _lib.load()
    P, C = c["P"], c["C"]
    ws = torch.empty(int(lib.tcam_bn_ws_bytes(P, C)), dtype=torch.uint8, device=c["y"].device)
    dy = torch.empty_like(c["dout"])
    dg, db = (torch.full((C,), float("nan"), device=dy.device) for _ in range(2))
    amax = torch.full((C,), -1, dtype=torch.int32, device=dy.device) if want_amax else None
    rc = lib.tcam_bn_relu_bwd_s3s2(c["dout"].data_ptr(), c["out"].data_ptr(), c["y"].data_ptr(),
                                   c["mean"].data_ptr(), c["invstd"].data_ptr(),
                                   c["gamma"].data_ptr(), dy.data_ptr(), dg.data_ptr(),
                                   db.data_ptr(), P, C, ws.data_ptr(),
                                   amax.data_ptr() if want_amax else None, _st())
    return rc, dy, dg, db, amax


def _dy_scaled(dy, amax, compute):
    lib = _lib.load()
    B, H, W, C = ops.s3_dims(dy)
    scale = torch.full((C,), float("nan"), device=dy.device)
    dy2 = ops.s2_empty(B, H, W, C, dy.device)
    rc = lib.tcam_dy_scaled_s2(dy.data_ptr(), B * H * W, C, amax.data_ptr(), compute,
                               scale.data_ptr(), dy2.data_ptr(), _st())
    return rc, dy2, scale


def _bwd_fused(c, use_out, want3):
    lib = _lib.load()
    P, C, dev = c["P"], c["C"], c["y"].device
    ws = torch.empty(int(lib.tcam_bn_bwd_scaled_ws_bytes(P, C)), dtype=torch.uint8, device=dev)
    dy3 = torch.empty_like(c["dout"]) if want3 else None
    dy2 = ops.s2_empty(c["B"], c["H"], c["W"], C, dev)
    scale, dg, db = (torch.full((C,), float("nan"), device=dev) for _ in range(3))
    rc = lib.tcam_bn_relu_bwd_scaled_s3s2(
        c["dout"].data_ptr(), c["out"].data_ptr() if use_out else None, c["y"].data_ptr(),
        c["mean"].data_ptr(), c["invstd"].data_ptr(), c["gamma"].data_ptr(),
        c["beta"].data_ptr(), dy3.data_ptr() if want3 else None, dy2.data_ptr(),
        scale.data_ptr(), dg.data_ptr(), db.data_ptr(), P, C, ws.data_ptr(), _st())
    return rc, dy3, dy2, scale, dg, db


def _bwd_fused_s1(c, use_out):
    lib = _lib.load()
    P, C, dev = c["P"], c["C"], c["y"].device
    ws = torch.empty(int(lib.tcam_bn_ws_bytes(P, C)), dtype=torch.uint8, device=dev)
    dy = torch.empty_like(c["dout"])
    dg, db = (torch.full((C,), float("nan"), device=dev) for _ in range(2))
    rc = lib.tcam_bn_relu_bwd_fused_s1(
        c["dout"].data_ptr(), c["out"].data_ptr() if use_out else None, c["y"].data_ptr(),
        c["mean"].data_ptr(), c["invstd"].data_ptr(), c["gamma"].data_ptr(),
        c["beta"].data_ptr(), dy.data_ptr(), dg.data_ptr(), db.data_ptr(), P, C, ws.data_ptr(),
        _st())
    return rc, dy, dg, db


def _same(what, *pairs):
    assert all(torch.equal(x, y) for x, y in pairs), what + ": not bit-identical"


def _check_bn_variants(c, s1c, tag):
    """Every variant of the backward on one input against the one fp64 reference; returns the
    largest 2^15 / max |dy2_c| of the fused (bound-derived) scale."""
    ref = _bn_ref(c)
    C = c["C"]
    # unfused, without and (C / 8 dividing 256) with the channel maxima
    rc, dy, dg, db, _ = _bwd_unfused(c, False)
    assert rc == 0
    _check_sums(ref, dg, db, tag + " unfused")
    _check_dy(ref, _nchw(dy), tag + " unfused")
    if 256 % (C // 8):   # the fused entries refuse such a C in their argument check
        assert _bwd_fused(c, True, True)[0] != 0 and _bwd_fused(c, False, False)[0] != 0
        assert _bwd_fused_s1(s1c, True)[0] != 0 and _bwd_fused_s1(s1c, False)[0] != 0
        torch.cuda.synchronize()
        return 0.0
    rc, dya, dga, dba, amax = _bwd_unfused(c, True)
    assert rc == 0
    _same(tag + " unfused amax: dgamma, dbeta", (dga, dg), (dba, db))
    _check_dy(ref, _nchw(dya), tag + " unfused amax")
    written = ops.s3_to_nchw(dya).abs().amax(dim=(0, 2, 3)).contiguous()
    _same(tag + " amax vs the written max |dy_c|", (amax, written.view(torch.int32)))
    # the scaled copy: the maxima computed by tcam_dy_scaled_s2 == those handed in
    rc0, dy2a, sca = _dy_scaled(dya, amax, 0)
    amax1 = torch.full_like(amax, -1)
    rc1, dy2b, scb = _dy_scaled(dya, amax1, 1)
    assert rc0 == 0 and rc1 == 0
    _same(tag + " dy_scaled compute=1 vs 0", (amax1, amax), (scb, sca), (dy2b, dy2a))
    _check_scaled(_nchw(dya), dy2a, sca, tag + " dy_scaled")
    wmax = written.double().cpu()
    top = (wmax * sca.double().cpu())[wmax > 0]
    assert ((top >= 2.0 ** 14) & (top < 2.0 ** 15)).all(), tag   # the max pass is tight
    # fused: out given / NULL, dy3 given / NULL
    slack = 0.0
    for use_out in (True, False):
        rc, dy3, dy2, sc, dg, db = _bwd_fused(c, use_out, True)
        assert rc == 0
        t = f"{tag} fused out={int(use_out)}"
        _check_sums(ref, dg, db, t)
        _check_dy(ref, _nchw(dy3), t)
        slack = max(slack, _check_scaled(_nchw(dy3), dy2, sc, t))
        rc, _, dy2n, scn, dgn, dbn = _bwd_fused(c, use_out, False)
        assert rc == 0
        _same(t + " dy3 NULL vs given", (dy2n, dy2), (scn, sc), (dgn, dg), (dbn, db))
    # AMP: S1 everywhere, dy rounded to fp16: 2^-11 |dy|, and below fp16's normal range
    # (|dy| < 2^-14), where the format has no relative precision to offer, half a subnormal
    # ulp, 2^-25
    ref1 = _bn_ref(s1c)
    a1 = ref1["dy"].abs()
    extra = 2.0 ** -11 * a1 + 2.0 ** -25 * (a1 < 2.0 ** -14)
    for use_out in (True, False):
        rc, dy1, dg, db = _bwd_fused_s1(s1c, use_out)
        assert rc == 0
        t = f"{tag} s1 out={int(use_out)}"
        _check_sums(ref1, dg, db, t)
        _check_dy(ref1, _nchw(dy1), t, extra=extra)
    return slack


@pytest.mark.parametrize("dmag", [1.0, 1e-7])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (3, 40, 37)])
@pytest.mark.parametrize("C", [8, 24, 64, 512, 2048])
def test_bn_relu_bwd_variants_match_fp64(cuda, C, B, H, W, dmag):
    """tcam_bn_relu_bwd_s3s2 (with / without amax), tcam_bn_relu_bwd_scaled_s3s2 (out and dy3
    given / NULL) and tcam_bn_relu_bwd_fused_s1 (out given / NULL) against one fp64 reference:
    dgamma, dbeta within 1e-6 of sum |g xh|, sum |g|; dy elementwise within 1e-6 |gamma invstd|
    (|g| + |mean g| + |xh| |mean g xh|) (+ fp16's rounding on S1); amax the bit pattern of the
    written max |dy_c|; the scaled copy's contract (_check_scaled).  C = 24: the unfused kernel's
    per-group path; the fused entries must refuse it.  The shapes reach one and many chunks of
    the partial sums, the tail iteration, GS = 1 .. 32 and both apply-loop branches.
    Measured on an MI355X, as fractions of the bounds: dy 0.29 (every S3 variant), dgamma 0.057,
    dbeta 0.044, the scaled copy 0.50; S1 dy 1.0 (fp16's half ulp is reached).  With sum g xh
    accumulated on an fp32 xh, dy reached 70.8 of its bound at 2048 x 70 (a channel whose sum
    g xh nearly cancels), and amax missed the written maximum by an ulp (the store's split
    contracted with dy's last product): both fixed in csrc/train.hip."""
    seed = C * 7 + H + (dmag < 1)
    c = _bn_case(cuda, B, C, H, W, dmag, seed)
    s1c = _bn_case(cuda, B, C, H, W, dmag, seed, lay="s1")
    _check_bn_variants(c, s1c, f"C{C} {B}x{H}x{W} dmag {dmag:g}")


@pytest.mark.parametrize("C,B,H,W", [(64, 2, 5, 7), (512, 3, 40, 37)])
def test_bn_relu_bwd_outlier_pixel_loose_scale(cuda, C, B, H, W):
    """One pixel per channel at ~50 sigma makes the bound behind the fused scale loose (max |xh|
    enters it): every assertion of the variants test still holds, dy2 keeps its accuracy.
    Measured on an MI355X: 2^15 / max |dy2_c| up to 83.8 here (C = 64; 2.86 at C = 512, and up
    to 3.33 on the plain inputs of test_bn_relu_bwd_variants_match_fp64), the scaled copy at
    0.50 of its bound; the max-pass scale keeps it within (1, 2]."""
    c = _bn_case(cuda, B, C, H, W, 1.0, C + 1, outlier=True)
    s1c = _bn_case(cuda, B, C, H, W, 1.0, C + 1, lay="s1", outlier=True)
    slack = _check_bn_variants(c, s1c, f"outlier C{C}")
    print(f"outlier C{C}: largest 2^15 / max|dy2_c| = {slack:.4g}")
    assert slack >= 1.0


def _f32_next(x, k):
    """x moved by k fp32 ulps."""
    return (x.contiguous().view(torch.int32) + k).view(torch.float32)


@pytest.mark.parametrize("lay", ["s2", "s1"])
@pytest.mark.parametrize("C", [64, 512])
def test_bn_relu_bwd_mask_from_y_equals_mask_from_out(cuda, lay, C):
    """out = NULL (the mask recomputed from y) == out given (the forward kernel's output), bit
    for bit, on pre-activations gamma xh + beta at 0, within +-1 fp32 ulp of it, and inside and
    below fp16's subnormal range (|z| from 1e-9 to 1e-4): y on a coarse grid, beta = -gamma
    xh(p0) for a grid value p0 per channel, moved by ulps and by small offsets channel by
    channel."""
    g = torch.Generator().manual_seed(C)
    B, H, W = 2, 9, 11
    grid = torch.randint(-6, 7, (B, C, H, W), generator=g).float() * 0.25
    c = _bn_case(cuda, B, C, H, W, 1.0, C, lay=lay)
    c["y"] = _act(grid, cuda, "amp" if lay == "s1" else "f16x3")
    c["y64"] = _nchw(c["y"])
    assert torch.equal(c["y64"], grid.double())      # the grid is exact in both layouts
    mean = c["y64"].mean((0, 2, 3)).float()
    invstd = (1.0 / torch.sqrt(c["y64"].var((0, 2, 3), unbiased=False) + EPS)).float()
    gamma = c["gamma"].cpu()
    p0 = torch.randint(-6, 7, (C,), generator=g).float() * 0.25
    xh0 = (p0 - mean) * invstd                        # fp32, as the kernels compute xh
    beta = -(gamma * xh0)
    ch = torch.arange(C)
    for k, ulps in ((1, 1), (2, -1), (3, 2), (4, -2)):
        beta[ch % 16 == k] = _f32_next(beta[ch % 16 == k], ulps)
    offs = torch.logspace(-9, -4, 10)
    for k in range(10):
        sel = ch % 16 == 5 + k % 11
        beta[sel] = beta[sel] + offs[k] * (1 if k % 2 else -1)
    for k, v in (("mean", mean), ("invstd", invstd), ("beta", beta)):
        c[k] = v.to(cuda).contiguous()
    c["out"] = _bn_fwd(c)
    o = _nchw(c["out"])
    hit = (c["y64"] == p0.double()[None, :, None, None])
    assert hit.any() and (o[hit] > 0).any() and (o[hit] == 0).any()   # both sides of the edge
    if lay == "s1":
        a, b = _bwd_fused_s1(c, True), _bwd_fused_s1(c, False)
    else:
        a, b = _bwd_fused(c, True, True), _bwd_fused(c, False, True)
    assert a[0] == 0 and b[0] == 0
    torch.cuda.synchronize()
    for ta, tb in zip(a[1:], b[1:]):
        assert torch.equal(ta.view(torch.int16) if ta.dtype != torch.float32 else
                           ta.view(torch.int32),
                           tb.view(torch.int16) if tb.dtype != torch.float32 else
                           tb.view(torch.int32))


# ------------------------------------ scaled copy -> data gradient and weight gradients
def _dead_set(C, dead):
    if dead == "none":
        return [], None
    n, how = dead.split("-")
    idx = [C // 3] if n == "one" else list(range(1, C, 4))
    return idx, how


def _producers(cuda, B, C, H, W, dmag, seed, dead, zero_dout=False, outlier=False):
    """(dy2, scale) of one BN-ReLU backward by both producers — the fused bound-derived scale
    and the unfused backward's amax + tcam_dy_scaled_s2 — with ``dead`` channels (every channel
    with ``zero_dout``), ``outlier``: one pixel per channel at ~50 sigma (a loose fused scale);
    each with the fp64 dy the device stored (dy2 / scale)."""
    idx, how = (list(range(C)), "dout") if zero_dout else _dead_set(C, dead)
    c = _bn_case(cuda, B, C, H, W, dmag, seed, outlier=outlier, dead=idx, dead_how=how)
    rc, _, dy2f, scf, _, _ = _bwd_fused(c, False, False)
    assert rc == 0
    rc, dy, _, _, amax = _bwd_unfused(c, True)
    assert rc == 0
    rc, dy2u, scu = _dy_scaled(dy, amax, 0)
    assert rc == 0
    res = []
    for name, dy2, sc in (("fused", dy2f, scf), ("amax", dy2u, scu)):
        d64 = _nchw(dy2) / sc.double().cpu()[None, :, None, None]
        if idx:
            assert (d64[:, idx] == 0).all() and (d64.abs().amax((0, 2, 3)) > 0).sum() == C - len(idx)
        res.append((name, dy2, sc, d64))
    return res


def _zero_up2(t, H, W):
    B, Hi, Wi, C = ops.s3_dims(t)
    out = ops.act_empty(t, B, H, W, C)
    assert _lib.load().tcam_zero_up2(t.data_ptr(), out.data_ptr(), 32, B, C, H, W, Hi, Wi,
                                     _st()) == 0
    return out


def _pack_dgrad(w, c0, sel, kdiv):
    """tcam_pack_weight_f16x3 mode 1: the data-gradient operand of conv weight ``w`` over its
    input channels [c0, c0 + sel), divided by kdiv per output channel of w."""
    cout, ctot, kh, kw = w.shape
    kp, mp = ops.conv_x6_weight_dims(kh * kw * cout, sel)
    wt = torch.empty((kp // 32, 4, 2, mp, 8), device=w.device, dtype=torch.float16)
    sc = torch.empty(mp, device=w.device, dtype=torch.float32)
    assert _lib.load().tcam_pack_weight_f16x3(w.data_ptr(), wt.data_ptr(), sc.data_ptr(), 1, cout,
                                              ctot, kh, kw, c0, sel, 0, kdiv.data_ptr(),
                                              _st()) == 0
    return wt, sc


def _dgrad(srcs, w, c0, sel, kdiv, H, W):
    k = w.shape[2]
    wt, sc = _pack_dgrad(w, c0, sel, kdiv)
    bias = torch.zeros(sel, device=w.device)
    return _nchw(ops.conv2d_f16x3_s3out([ConvSrc(s) for s in srcs], wt, sc, bias, sel, H, W, k,
                                        k - 1 - (k // 2)))


def _wgrad11(x, stride, dy2, sc):
    lib = _lib.load()
    B, Hin, Win, Cin = ops.s3_dims(x)
    _, Ho, Wo, Cout = ops.s3_dims(dy2)
    nb = lib.tcam_wgrad11_ws_bytes(B, Cin, Hin, Win, stride, Cout, Ho, Wo)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    dw = torch.full((Cout, Cin, 1, 1), float("nan"), device=x.device)
    assert lib.tcam_wgrad11_s2_f16x3(x.data_ptr(), B, Cin, Hin, Win, stride, dy2.data_ptr(),
                                     sc.data_ptr(), Cout, Ho, Wo, dw.data_ptr(), ws.data_ptr(),
                                     nb, _st()) == 0
    return dw.cpu().double()


def _wgrad33(x, dy2, sc):
    lib = _lib.load()
    B, H, W, Cin = ops.s3_dims(x)
    _, Ho, Wo, Cout = ops.s3_dims(dy2)
    arr = (_lib.tcam_conv_src * 1)()
    arr[0] = _lib.tcam_conv_src(x.data_ptr(), Cin, H, W, 1, 0)
    nb = int(lib.tcam_conv_wgrad_ws_bytes(arr, 1, B, Cout, Ho, Wo, 3, 3))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device=x.device)
    assert lib.tcam_conv_wgrad_s2_f16x3(arr, 1, B, dy2.data_ptr(), sc.data_ptr(), Cout, Ho, Wo, 3,
                                        3, 1, 1, Cout, dw.data_ptr(), ws.data_ptr(), nb,
                                        _st()) == 0
    return dw.cpu().double()


def _ref_grads(x64, w64, dy64, stride, pad):
    """fp64 dx = conv_transpose2d(dy, W) and dW = sum_p dy x of y = conv2d(x, W), and the same
    two operations on absolute values."""
    out = []
    for x, w, d in ((x64, w64, dy64), (x64.abs(), w64.abs(), dy64.abs())):
        H, W = x.shape[2:]
        k = w.shape[2]
        oph = H - ((d.shape[2] - 1) * stride - 2 * pad + k)
        opw = W - ((d.shape[3] - 1) * stride - 2 * pad + k)
        dx = F.conv_transpose2d(d, w, stride=stride, padding=pad, output_padding=(oph, opw))
        wr = w.clone().requires_grad_(True)
        F.conv2d(x, wr, stride=stride, padding=pad).backward(d)
        out += [dx, wr.grad]
    return out


# name: (Cout of the conv = dy's channels, Ctot its input channels, k, stride, c0, sel,
#        B, H, W of the conv's input)
GEOMS = {
    "1x1_64to256": (64, 256, 1, 1, 0, 256, 2, 9, 11),
    "1x1_2048to512": (2048, 512, 1, 1, 0, 512, 2, 4, 4),
    "3x3_64to64": (64, 64, 3, 1, 0, 64, 2, 9, 11),
    "3x3s2_zero_up2": (64, 32, 3, 2, 0, 32, 2, 9, 11),
    "3x3_slice": (32, 96, 3, 1, 16, 64, 2, 9, 11),
}
DEAD = ["none", "one-beta", "one-gamma", "one-dout", "quarter-beta", "quarter-gamma",
        "quarter-dout"]
DMAGS = [1.0, 1e-5, 1e-7]


def _check_geom(cuda, geom, dmag, dead, outlier=False):
    """One geometry's dx and dW from both producers' (scale, dy2) against fp64, within 1e-6 of
    the same operation on absolute values; returns each producer's largest 2^15 / max |dy2_c|."""
    cout, ctot, k, stride, c0, sel, B, H, W = GEOMS[geom]
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g = torch.Generator().manual_seed(cout + ctot + k)
    w = (torch.randn(cout, ctot, k, k, generator=g) / (ctot * k * k) ** 0.5).to(cuda)
    xs = _act(torch.randn(B, ctot, H, W, generator=g), cuda, "f16x3")
    x64, w64 = _nchw(xs), w.double().cpu()
    slack = {}
    for name, dy2, sc, d64 in _producers(cuda, B, cout, Ho, Wo, dmag, cout + k + stride, dead,
                                         outlier=outlier):
        src = dy2 if stride == 1 else _zero_up2(dy2, H, W)
        dx_ref, dw_ref, dx_mag, dw_mag = _ref_grads(x64, w64, d64, stride, pad)
        dx = _dgrad([src], w, c0, sel, sc, H, W)
        rx = _ratio((dx - dx_ref[:, c0:c0 + sel]).abs(), 1e-6 * dx_mag[:, c0:c0 + sel])
        dw = _wgrad11(xs, stride, dy2, sc) if k == 1 else _wgrad33(xs, src, sc)
        rw = _ratio((dw - dw_ref).abs(), 1e-6 * dw_mag)
        amax = _nchw(dy2).abs().amax((0, 2, 3))
        slack[name] = float((2.0 ** 15 / amax[amax > 0]).max())
        print(f"{geom} dmag {dmag:g} {dead} outlier={int(outlier)} {name}: dx {rx:.3g} dW "
              f"{rw:.3g} of 1e-6 mag, 2^15 / max|dy2_c| up to {slack[name]:.3g}")
        assert torch.isfinite(dx).all() and torch.isfinite(dw).all()
        assert rx <= 1.0 and rw <= 1.0, (geom, dmag, dead, name, rx, rw)
    return slack


@pytest.mark.parametrize("dead", DEAD)
@pytest.mark.parametrize("dmag", DMAGS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_dgrad_wgrad_of_scaled_copy_match_fp64(cuda, geom, dmag, dead):
    """dy -> (scale, dy2) by both producers -> dx = tcam_conv2d_f16x3_s3out(dy2, pack(W, mode 1,
    kdiv = scale)) against fp64 conv_transpose2d, dW (tcam_wgrad11_s2_f16x3 /
    tcam_conv_wgrad_s2_f16x3) against the fp64 sum: both within 1e-6 of the same operation on
    absolute values, for gradients down to 1e-7 and with dead channels in dy (all masked, gamma
    = 0, zero dout): a channel without a gradient must not set the fp16 range of the packed
    columns.  Measured on an MI355X (worst |err| / mag, bound 1e-6): dx 4.0e-7 and dW 3.0e-7
    over all cases; with scale 1 for such a channel dx reached 7.5e-4 (dout x 1e-5) and 6.4e-2
    (dout x 1e-7) — DESIGN.md "The f16x3 training step"."""
    _check_geom(cuda, geom, dmag, dead)


@pytest.mark.parametrize("dmag", [1.0, 1e-7])
@pytest.mark.parametrize("geom", ["1x1_64to256", "3x3_64to64"])
def test_dgrad_wgrad_with_loose_scale_match_fp64(cuda, geom, dmag):
    """The same checks on a dy whose BN input has one pixel per channel at ~50 sigma: the fused
    backward's bound-derived scale is then loose (max |dy2_c| well below 2^15; the max pass
    keeps 2^15 / max |dy2_c| within (1, 2]), and dx and dW must still hold 1e-6 of their
    magnitude sums.  Measured on an MI355X: 2^15 / max |dy2_c| 34 to 49 (fused), dx at most 0.35
    and dW at most 0.34 of the bound, the same as with the tight scale."""
    slack = _check_geom(cuda, geom, dmag, "none", outlier=True)
    assert slack["amax"] <= 2.0 and slack["fused"] > 2.0, slack


@pytest.mark.parametrize("dead", DEAD)
@pytest.mark.parametrize("dmag", DMAGS)
def test_dgrad_two_source_projection_matches_fp64(cuda, dmag, dead):
    """A projection block's input gradient: one K-concatenated 1x1 conv over [dy1 | dyd], the
    second source (the stride-2 shortcut's dy) zero-inserted onto the input grid, the weight
    cat(W1, Wd) packed with kdiv = cat(sc1, scd); and each conv's own 1x1 weight gradient."""
    B, cin, H, W, c1, cd = 2, 128, 8, 10, 64, 256
    g = torch.Generator().manual_seed(17)
    w1 = (torch.randn(c1, cin, 1, 1, generator=g) / cin ** 0.5).to(cuda)
    wd = (torch.randn(cd, cin, 1, 1, generator=g) / cin ** 0.5).to(cuda)
    xs = _act(torch.randn(B, cin, H, W, generator=g), cuda, "f16x3")
    x64 = _nchw(xs)
    p1 = _producers(cuda, B, c1, H, W, dmag, 31, dead)
    pd = _producers(cuda, B, cd, H // 2, W // 2, dmag, 32, dead)
    for (name, dy2a, sca, da), (_, dy2b, scb, dbb) in zip(p1, pd):
        ra = _ref_grads(x64, w1.double().cpu(), da, 1, 0)
        rb = _ref_grads(x64, wd.double().cpu(), dbb, 2, 0)
        dx = _dgrad([dy2a, _zero_up2(dy2b, H, W)], torch.cat([w1, wd], 0).contiguous(), 0, cin,
                    torch.cat([sca, scb]).contiguous(), H, W)
        rx = _ratio((dx - (ra[0] + rb[0])).abs(), 1e-6 * (ra[2] + rb[2]))
        rw1 = _ratio((_wgrad11(xs, 1, dy2a, sca) - ra[1]).abs(), 1e-6 * ra[3])
        rwd = _ratio((_wgrad11(xs, 2, dy2b, scb) - rb[1]).abs(), 1e-6 * rb[3])
        print(f"projection dmag {dmag:g} {dead} {name}: dx {rx:.3g} dW {rw1:.3g} {rwd:.3g}")
        assert rx <= 1.0 and rw1 <= 1.0 and rwd <= 1.0, (dmag, dead, name, rx, rw1, rwd)


@pytest.mark.parametrize("wmag", [1.0, 1e-4])
def test_dgrad_of_an_all_zero_dy_is_zero(cuda, wmag):
    """Every dy channel without a gradient (a zero dout): both producers give dy2 = 0 and the
    same scale for every channel, and the data / weight gradients are exactly 0 — the packed
    columns, now made of nothing but W / scale, keep a usable scale (no 0 / 0), small weights
    included."""
    B, cout, cin, H, W = 2, 64, 64, 5, 7
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * wmag / 24).to(cuda)
    xs = _act(torch.randn(B, cin, H, W, generator=g), cuda, "f16x3")
    for name, dy2, sc, d64 in _producers(cuda, B, cout, H, W, 1.0, 5, "none", zero_dout=True):
        assert (d64 == 0).all() and (sc == sc[0]).all() and float(sc[0]) >= 1.0, name
        dx = _dgrad([dy2], w, 0, cin, sc, H, W)
        dw = _wgrad33(xs, dy2, sc)
        assert (dx == 0).all() and (dw == 0).all(), name


# ------------------------------------------------- whole steps with dead BN channels
def test_stdcl_step_with_dead_channels_matches_fp64_oracle(cuda):
    """test_stdcl_step_matches_fp64_oracle at 2 x 64^2 on an encoder with BN channels that are
    masked on the whole batch (bn1 / bn2 biases of layer1.0 and layer3.1 at -50, as a trained
    encoder has them): every parameter gradient norm-relative <= 1e-4 of the mask-exact fp64
    oracle.  Measured on an MI355X: worst 6.5e-6; with scale 1 for a dead channel 6.9e-5
    (encoder.layer3.1.bn1.weight) — ten times worse but inside the bound, so this guard alone
    would not have caught that fault at this size; the kernel tests above do."""
    from tcam_wsol_video_amd.cl_training import ClassifierTrainer
    from tcam_wsol_video_amd.models import build_r50_stdcl
    torch.manual_seed(0)
    model = build_r50_stdcl(seed=21).to(cuda)
    with torch.no_grad():
        for blk in (model.encoder.layer1[0], model.encoder.layer3[1]):
            blk.bn1.bias[[1, 7, 20]] = -50.0
            blk.bn2.bias[[0, 13, 40, 41]] = -50.0
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    tr = ClassifierTrainer(model, lr=0.01)
    B = 2
    x = _frames(B, 64, 3)
    y = torch.tensor([(7 * i + 3) % 10 for i in range(B)], dtype=torch.int32)
    logits, st = tr.forward(x.to(cuda))
    loss, dl = tr.loss_and_grad(logits, y.to(cuda))
    tr.loss_gate.copy_(loss)
    tr.backward(dl, st)
    torch.cuda.synchronize()
    ops.check_f16_overflow(cuda, all_ranks=False)
    masks = _masks(tr, st)
    assert not masks["encoder.layer1.0.relu1"][:, [1, 7, 20]].any()
    assert not masks["encoder.layer3.1.relu2"][:, [0, 13, 40, 41]].any()
    gdev = {n: tr.g(p).detach().cpu().clone() for n, p in model.named_parameters()}
    lo, lg, grads, _, _ = T.stdcl_step(sd0, x, y, lr=0.01, masks=masks)
    assert abs(float(loss) - lo) <= 1e-5 * abs(lo)
    assert _norm_rel(logits, lg) <= 1e-5
    worst = max((_norm_rel(gdev[n], grads[n]), n) for n in gdev)
    print("stdcl step with dead channels: worst gradient", worst)
    assert worst[0] <= 1e-4, worst


def test_decoder_step_with_dead_channels_matches_autograd_oracle(cuda):
    """test_train_step_matches_autograd_oracle (build_r50_tcam at 64, f16x3, its 2e-5) on a
    decoder with BN channels masked on the whole batch (biases at -50).  Measured on an
    MI355X: worst 1.0e-5; with scale 1 for a dead channel 7.4e-4 (decoder.blocks.0.conv1.1.weight),
    which fails."""
    from tcam_wsol_video_amd.models import build_r50_tcam
    from tcam_wsol_video_amd.training import DecoderTrainer
    from test_gpu_train import _batch, _device_relu_masks, _rel
    model = build_r50_tcam(seed=21)
    with torch.no_grad():
        sd = model.state_dict()
        for i in (0, 2):
            for cv in ("conv1", "conv2"):
                b = sd[f"decoder.blocks.{i}.{cv}.1.bias"]
                b[[1, b.numel() // 2, b.numel() - 1]] = -50.0
    sd_cpu = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(cuda)
    x, raw, seeds = _batch(2, 64, seed=5)
    tr = DecoderTrainer(model, prec="f16x3")
    masks = _device_relu_masks(tr, x.to(cuda))
    assert not masks["decoder.blocks.0.conv1"][:, 1].any()
    losses_ref, grads, _, _ = T.train_step(sd_cpu, x, raw, seeds, masks=masks)
    losses = tr.step(x.to(cuda), raw.to(cuda), seeds.to(cuda)).cpu().numpy()
    torch.cuda.synchronize()
    for i, k in enumerate(("total", "sl", "crf", "size")):
        assert abs(losses[i] - losses_ref[k]) <= 1e-5 * max(abs(losses_ref[k]), 1e-3), k
    named = dict(model.named_parameters())
    errs = {k: _rel(tr.g(named[k]), gref) for k, gref in grads.items()}
    worst = max(errs, key=errs.get)
    print("decoder step with dead channels: worst gradient", worst, errs[worst])
    assert errs[worst] <= 2e-5, (worst, errs[worst])


# ------------------------------------------------------------- SGD and the GradScaler
NS = [1, 63, 257, 100003]
def _sgd_state(cuda, n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(cuda)
    buf = torch.full((n,), 7.0, device=cuda)     # stale: the first applied step must overwrite it
    grads = [(torch.randn(n, generator=g) * 10 ** float(e)).to(cuda) for e in (0, -3, 1, 0, -1, 0)]
    return p, buf, grads


def _check_sgd(p0, g, b0, first, cfg, p, buf, tag):
    rp, rb, bp, bb = sgd_ref(p0.double().cpu(), g.double().cpu(), b0.double().cpu(), first, cfg)
    ep = (p.double().cpu() - rp).abs()
    assert (ep <= bp).all(), (tag, _ratio(ep, bp))
    if cfg[0] != 0:
        eb = (buf.double().cpu() - rb).abs()
        assert (eb <= bb).all(), (tag, _ratio(eb, bb))
    else:
        assert torch.equal(buf, b0), tag


@pytest.mark.parametrize("cfg", SGD_CFGS)
@pytest.mark.parametrize("n", NS)
def test_sgd_step_matches_fp64(cuda, n, cfg):
    """tcam_sgd_step over three consecutive steps (first = 1, 0, 0), each against the fp64 step
    from the state the device held."""
    lib = _lib.load()
    m, damp, wd, nest, gs = cfg
    p, buf, grads = _sgd_state(cuda, n, n)
    for step in range(3):
        p0, b0, g = p.clone(), buf.clone(), grads[step]
        assert lib.tcam_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr(), n, LR, m, damp, wd,
                                 nest, int(step == 0), gs, _st()) == 0
        _check_sgd(p0, g, b0, step == 0, cfg, p, buf, (n, cfg, step))


@pytest.mark.parametrize("cfg", SGD_CFGS[1:4])
@pytest.mark.parametrize("n", NS)
def test_sgd_step_gated_matches_fp64(cuda, n, cfg):
    """tcam_sgd_step_gated: a NaN / inf gate leaves parameters and momentum bit-unchanged and
    counts a skip; the first APPLIED step (after a skipped one) initialises the buffer."""
    lib = _lib.load()
    m, damp, wd, nest, gs = cfg
    p, buf, grads = _sgd_state(cuda, n, n + 1)
    steps = torch.zeros(1, dtype=torch.int32, device=cuda)
    skipped = torch.zeros(1, dtype=torch.int32, device=cuda)
    applied = nskip = 0
    for step, gv in enumerate([float("nan"), 0.7, float("inf"), 2.5, 0.1, float("-inf")]):
        gate = torch.tensor([gv], device=cuda)
        p0, b0, g = p.clone(), buf.clone(), grads[step]
        assert lib.tcam_sgd_step_gated(p.data_ptr(), g.data_ptr(), buf.data_ptr(), n, LR, m, damp,
                                       wd, nest, gs, gate.data_ptr(), steps.data_ptr(),
                                       skipped.data_ptr(), _st()) == 0
        if np.isfinite(gv):
            _check_sgd(p0, g, b0, applied == 0, cfg, p, buf, (n, cfg, step))
            applied += 1
        else:
            assert torch.equal(p, p0) and torch.equal(buf, b0)
            nskip += 1
        assert int(steps) == applied and int(skipped) == nskip
    # skipped may be NULL
    assert lib.tcam_sgd_step_gated(p.data_ptr(), grads[0].data_ptr(), buf.data_ptr(), n, LR, m,
                                   damp, wd, nest, gs, torch.tensor([float("nan")],
                                                                    device=cuda).data_ptr(),
                                   steps.data_ptr(), None, _st()) == 0
    assert int(steps) == applied


@pytest.mark.parametrize("cfg", SGD_CFGS[2:4])
@pytest.mark.parametrize("n", NS)
def test_sgd_step_amp_matches_fp64_and_gradscaler(cuda, n, cfg):
    """tcam_sgd_step_amp: the step runs only on a finite loss without found_inf; found_inf backs
    the scale off and resets the tracker; growth_interval clean steps in a row grow it; a
    non-finite loss changes neither parameters, momentum, scale nor tracker."""
    lib = _lib.load()
    m, damp, wd, nest, gs = cfg
    p, buf, grads = _sgd_state(cuda, n, n + 2)
    steps = torch.zeros(1, dtype=torch.int32, device=cuda)
    skipped = torch.zeros(1, dtype=torch.int32, device=cuda)
    scale = torch.tensor([1024.0], device=cuda)
    tracker = torch.zeros(1, dtype=torch.int32, device=cuda)
    ex_scale, ex_tr, applied, nskip = 1024.0, 0, 0, 0
    seq = [(1.0, 1.0), (float("nan"), 0.0), (1.0, 0.0), (0.5, 0.0), (float("inf"), 1.0),
           (2.0, 0.0)]
    for step, (lossv, finf) in enumerate(seq):
        gate = torch.tensor([lossv, finf], device=cuda)
        p0, b0, g = p.clone(), buf.clone(), grads[step]
        assert lib.tcam_sgd_step_amp(p.data_ptr(), g.data_ptr(), buf.data_ptr(), n, LR, m, damp,
                                     wd, nest, gs, gate.data_ptr(), steps.data_ptr(),
                                     skipped.data_ptr(), scale.data_ptr(), tracker.data_ptr(),
                                     2.0, 0.5, 2, _st()) == 0
        if np.isfinite(lossv) and finf == 0:
            _check_sgd(p0, g, b0, applied == 0, cfg, p, buf, (n, cfg, step))
            applied += 1
            ex_tr += 1
            if ex_tr >= 2:
                ex_scale, ex_tr = ex_scale * 2.0, 0
        else:
            assert torch.equal(p, p0) and torch.equal(buf, b0)
            nskip += 1
            if np.isfinite(lossv):
                ex_scale, ex_tr = ex_scale * 0.5, 0
        assert float(scale) == ex_scale and int(tracker) == ex_tr, (step, float(scale))
        assert int(steps) == applied and int(skipped) == nskip
    assert applied == 3 and ex_scale == 1024.0


@pytest.mark.parametrize("n", NS)
def test_amp_unscale_exact_and_found_inf(cuda, n):
    """tcam_amp_unscale: g / scale exactly for a power-of-two scale; found_inf set by a single
    inf, and by a single NaN, in the last element, and left 0 otherwise."""
    lib = _lib.load()
    g0 = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 300.0).to(cuda)
    scale = torch.tensor([8192.0], device=cuda)
    for bad in (None, float("inf"), float("-inf"), float("nan")):
        g = g0.clone()
        if bad is not None:
            g[n - 1] = bad
        ref = g / 8192.0
        found = torch.zeros(1, device=cuda)
        assert lib.tcam_amp_unscale(g.data_ptr(), n, scale.data_ptr(), found.data_ptr(),
                                    _st()) == 0
        assert float(found) == (0.0 if bad is None else 1.0), bad
        assert torch.equal(g.view(torch.int32)[:n - 1], ref.view(torch.int32)[:n - 1])
        assert torch.equal(torch.isnan(g), torch.isnan(ref))
        assert torch.equal(g[~torch.isnan(g)], ref[~torch.isnan(ref)])
