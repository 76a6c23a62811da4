"""Direct fp64 checks of the inference tail, kernel by kernel through the C ABI, in every
storage form the kernel has (plain NCHW fp32, S3, S2, S1): tcam_maxpool3x3s2*, tcam_pool2d_*,
tcam_up2_resize*, tcam_up2_resize_bwd_*, tcam_resize_cam, tcam_wgap*, tcam_seghead_cam*,
tcam_std_cam*, tcam_temporal_max, tcam_temporal_cam and tcam_topk_flags.  References, bounds,
shapes and input builders: tests/infer_tail_ref.py (pinned to torch and the oracle, with
their teeth, by tests/test_infer_tail_ref.py).  Every operand is the value the device stored,
every bound is elementwise on the sum of magnitudes of the output's terms, every output is
filled with NaN (uint8: 0xA5) before the call, every call is made twice and compared bit for
bit, and no kernel's output feeds another's check.  A uint8 output must be floor(double(the
device's CAM) * 255) everywhere and floor(reference * 255) wherever the reference decides it.

Measured on an MI355X, worst error / bound per output (the whole file, 267 cases, runs in 3 s):
maxpool3x3s2 and pool2d max exact in every form; pool2d avg S3 0.50, S2 0.96, S1 1.00;
up2_resize plain 0.30, S3 0.31, S2 0.74, S1 1.00; up2_resize_bwd S3 0.25, S1 1.00 (fp16's half
ulp); resize_cam fcams 0.65, cam 0.40; wgap mean plain 0.34, S3 0.30, S2 0.33, S1 0.12, logits
0.06 - 0.08; seghead fcams 0.01, cam 0.05 (0.03 on S1) in every form; std_cam low 0.10, 0.10,
0.08, 0.07 and cam 0.10, 0.12, 0.10, 0.11 (plain, S3, S2, S1); temporal_max / temporal_cam 0.46,
exact at t = 0; uint8 pixels left undecided: resize_cam 0.06 %, seghead 0.36 %, std_cam 0.09 %,
temporal_cam 0.05 % at the most.  Before the kernels' NaN-propagating min / max and the NaN-first
rank, test_std_cam_nan_position_zeroes_the_map[s3 / s2 / s1-overflow, f32 / s1-inf],
test_temporal_nan_pixel_follows_the_oracle[0.7, 30.0] and
test_topk_flags_follow_the_stable_sort[nan] failed on the device; everything else passed
unchanged (f32-overflow too: the plain kernel's contracted fma(w, A, s) adds the unrounded
product to +inf and never forms the NaN, so its map was 0 already)."""
import pytest
import torch
import torch.nn.functional as F

import infer_tail_ref as R
from oracle import model_ref as M
from tcam_wsol_video_amd import _lib
from test_gpu_enc_train import _act, _nchw, _st
from test_x_train_fwd_gpu import FMT, NAN, _nan, _nan_act, _report, _twice

pytestmark = pytest.mark.gpu

E_ARG = -1      # TCAM_E_ARG


def _sym(name, lay):
    return getattr(_lib.load(), name if lay == "f32" else f"{name}_{lay}")


def _put(x, lay, cuda):
    """x (B, C, H, W) fp32 in the storage form on the device, and the fp64 values it holds."""
    if lay == "f32":
        xd = x.to(cuda).float().contiguous()
        return xd, xd.double().cpu()
    xs = _act(x, cuda, FMT[lay])
    return xs, _nchw(xs)


def _out(lay, B, C, H, W, cuda):
    return _nan(cuda, B, C, H, W) if lay == "f32" else _nan_act(lay, B, H, W, C, cuda)


def _get(t, lay):
    return t.double().cpu() if lay == "f32" else _nchw(t)


def _u8(cuda, *shape):
    return torch.full(shape, 0xA5, dtype=torch.uint8, device=cuda)


def _run(fn):
    """_twice for a call that also returns uint8 outputs (widened, losslessly, to int32)."""
    outs = fn()
    _twice(lambda: tuple(o if o.element_size() > 1 else o.int() for o in fn()))
    return outs


def _u8_ratios(tag, u8, cam, ref, bound):
    own, dec, excl = R.u8_check(u8.cpu(), cam.cpu() if cam is not None else None, ref, bound)
    print(f"{tag}: u8 excluded {excl:.4f}")
    assert own, f"{tag}: u8 is not floor(double(cam) * 255)"
    assert dec, f"{tag}: u8 differs from floor(ref * 255) at a decided pixel"
    assert excl <= R.U8_EXCLUDED_MAX


# -------------------------------------------------------------------------- pools
@pytest.mark.parametrize("with_nan", [False, True])
@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("C,H,W", R.POOL_SHAPES)
def test_maxpool3x3s2_is_exact(cuda, C, H, W, lay, with_nan):
    """tcam_maxpool3x3s2{,_s3,_s2,_s1} equals F.max_pool2d(3, 2, 1) in fp64 on the stored
    values, value for value; one NaN pixel makes exactly the windows that hold it NaN."""
    B = 2
    x = R.pool_input(B, C, H, W, seed=C + H)
    if with_nan:
        x[1, 5 % C, H // 2, W - 1] = NAN
    xs, x64 = _put(x, lay, cuda)
    Ho, Wo = R.pool_out(H, 3, 2, 1, False), R.pool_out(W, 3, 2, 1, False)

    def run():
        out = _out(lay, B, C, Ho, Wo, cuda)
        assert _sym("tcam_maxpool3x3s2", lay)(xs.data_ptr(), out.data_ptr(), B, C, H, W, Ho, Wo,
                                              _st()) == 0
        return (out,)
    (out,) = _twice(run)
    ref, _ = R.maxpool_ref(x64, 3, 2, 1)
    got = _get(out, lay)
    if with_nan:
        hit = F.max_pool2d(torch.isnan(x64).double(), 3, 2, 1) > 0
        assert torch.equal(torch.isnan(got), hit) and int(hit.sum()) >= 1
    _report(f"maxpool3x3s2 {lay} {C}x{H}x{W} nan {int(with_nan)}",
            {"out": R.nan_ratio(got, ref, 0.0)})


def _pool2d(lay, xs, B, C, H, W, cfg, cuda, out=None, cstride=0, coff=0):
    k, s, p, mode, ceil = cfg
    Ho, Wo = R.pool_out(H, k, s, p, ceil), R.pool_out(W, k, s, p, ceil)
    out = _nan_act(lay, B, Ho, Wo, C, cuda) if out is None else out.clone()
    assert getattr(_lib.load(), f"tcam_pool2d_{lay}")(
        xs.data_ptr(), out.data_ptr(), B, C, H, W, Ho, Wo, k, k, s, p, int(mode == "avg"),
        cstride, coff, _st()) == 0
    return (out,)


@pytest.mark.parametrize("lay", R.LAYS[1:])
def test_pool2d_matches_fp64(cuda, lay):
    """tcam_pool2d_{s3,s2,s1} at every case of infer_tail_ref.pool_cases(): max exact (with
    one NaN pixel in the input), avg within (taps + 1) 2^-24 sum |x| / divisor + storage."""
    B, worst = 2, {"max": 0.0, "avg": 0.0}
    for C, H, W, cfg in R.pool_cases():
        k, s, p, mode, ceil = cfg
        x = R.pool_input(B, C, H, W, seed=C + H + k)
        if mode == "max":
            x[0, C - 1, H - 1, W // 2] = NAN
        xs, x64 = _put(x, lay, cuda)
        (out,) = _twice(lambda: _pool2d(lay, xs, B, C, H, W, cfg, cuda))
        got = _get(out, lay)
        if mode == "max":
            ref, bound = R.maxpool_ref(x64, k, s, p, ceil)
            hit = F.max_pool2d(torch.isnan(x64).double(), k, s, p, ceil_mode=ceil) > 0
            assert torch.equal(torch.isnan(got), hit)
        else:
            ref, bound = R.avgpool_ref(x64, k, s, p, ceil, lay)
        r = R.nan_ratio(got, ref, bound)
        assert r <= 1.0, (C, H, W, cfg, r)
        worst[mode] = max(worst[mode], r)
    _report(f"pool2d {lay}", worst)


@pytest.mark.parametrize("lay", R.LAYS[1:])
def test_pool2d_concat_slice_leaves_the_other_channels_alone(cuda, lay):
    """out of 40 channels, the pool written at channel offset 16: channels [0, 16) and [32, 40)
    keep their byte pattern bit for bit."""
    q = R.POOL_CONCAT
    B, C, H, W, cs, co, cfg = 2, q["C"], q["H"], q["W"], q["cstride"], q["coff"], q["cfg"]
    xs, x64 = _put(R.pool_input(B, C, H, W, seed=9), lay, cuda)
    base = _nan_act(lay, B, H, W, cs, cuda)
    base.view(torch.uint8).copy_((torch.arange(base.view(torch.uint8).numel(), device=cuda)
                                  % 251).to(torch.uint8).view(base.view(torch.uint8).shape))
    (out,) = _twice(lambda: _pool2d(lay, xs, B, C, H, W, cfg, cuda, base, cs, co))
    g0, g1 = co // 8, (co + C) // 8
    ob, bb = out.view(torch.uint8), base.view(torch.uint8)
    assert torch.equal(ob[:, :, :, :g0], bb[:, :, :, :g0])
    assert torch.equal(ob[:, :, :, g1:], bb[:, :, :, g1:])
    ref, bound = R.avgpool_ref(x64, *cfg[:3], cfg[4], lay)
    _report(f"pool2d concat {lay}", {"out": R.ratio(_get(out, lay)[:, co:co + C], ref, bound)})


# --------------------------------------------------------------------- resamplers
@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("C", R.UP2R_C)
@pytest.mark.parametrize("hw,out", R.UP2R_SHAPES)
def test_up2_resize_matches_fp64(cuda, hw, out, C, lay):
    (H, W), (Ho, Wo), B = hw, out, 2
    xs, x64 = _put(R.act_input(B, C, H, W, seed=C + H + Ho), lay, cuda)

    def run():
        o = _out(lay, B, C, Ho, Wo, cuda)
        assert _sym("tcam_up2_resize", lay)(xs.data_ptr(), o.data_ptr(), B, C, H, W, Ho, Wo,
                                            _st()) == 0
        return (o,)
    (o,) = _twice(run)
    got = _get(o, lay)
    ref, bound, _ = R.up2_resize_ref(x64, Ho, Wo, lay)
    _report(f"up2_resize {lay} {C}x{H}x{W}->{Ho}x{Wo}", {"out": R.ratio(got, ref, bound)})
    if (Ho, Wo) == (2 * H, 2 * W):      # scale 1: the nearest map itself
        assert torch.equal(got, ref)


@pytest.mark.parametrize("lay", ["s3", "s1"])
@pytest.mark.parametrize("C", R.UP2R_C)
@pytest.mark.parametrize("hw,out", R.UP2R_BWD_SHAPES)
def test_up2_resize_bwd_matches_fp64(cuda, hw, out, C, lay):
    (H, W), (Ho, Wo), B = hw, out, 2
    gs, g64 = _put(R.act_input(B, C, Ho, Wo, seed=C + H + Wo), lay, cuda)

    def run():
        gx = _nan_act(lay, B, H, W, C, cuda)
        assert _sym("tcam_up2_resize_bwd", lay)(gs.data_ptr(), gx.data_ptr(), B, C, H, W, Ho, Wo,
                                                _st()) == 0
        return (gx,)
    (gx,) = _twice(run)
    ref, bound, _ = R.up2_resize_bwd_ref(g64, H, W, lay)
    _report(f"up2_resize_bwd {lay} {C}x{H}x{W}<-{Ho}x{Wo}",
            {"gx": R.ratio(_nchw(gx), ref, bound)})


@pytest.mark.parametrize("argmax", [0, 1])
@pytest.mark.parametrize("hw,out", R.RESIZE_CAM_SHAPES)
def test_resize_cam_matches_fp64(cuda, hw, out, argmax):
    (Hi, Wi), (Ho, Wo), B = hw, out, 2
    f = R.fcams_input(B, Hi, Wi, seed=Hi + Wo)
    fd = f.to(cuda)

    def run():
        fo, cam, u8 = _nan(cuda, B, 2, Ho, Wo), _nan(cuda, B, Ho, Wo), _u8(cuda, B, Ho, Wo)
        assert _lib.load().tcam_resize_cam(fd.data_ptr(), fo.data_ptr(), cam.data_ptr(),
                                           u8.data_ptr(), B, Hi, Wi, Ho, Wo, argmax, _st()) == 0
        return fo, cam, u8
    fo, cam, u8 = _run(run)
    ref = R.resize_cam_ref(f.double(), Ho, Wo, bool(argmax))
    tag = f"resize_cam {Hi}x{Wi}->{Ho}x{Wo} argmax {argmax}"
    _report(tag, {"fcams": R.ratio(fo.cpu(), ref["fcams"], ref["b_fcams"]),
                  "cam": R.ratio(cam.cpu(), ref["cam"], ref["b_cam"])})
    _u8_ratios(tag, u8, cam, ref["cam"], ref["b_cam"])


# --------------------------------------------------------------------------- WGAP
@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("B,C,HW,K", R.WGAP_SHAPES)
def test_wgap_matches_fp64(cuda, B, C, HW, K, lay):
    lib = _lib.load()
    c = R.wgap_input(B, C, HW, K, seed=C + HW)
    xs, x64 = _put(c["x"], lay, cuda)
    wd, bd = c["w"].to(cuda), c["b"].to(cuda)

    def run():
        logits, mean = _nan(cuda, B, K), _nan(cuda, B, C)
        if lay == "f32":
            rc = lib.tcam_wgap(xs.data_ptr(), wd.data_ptr(), bd.data_ptr(), logits.data_ptr(),
                               mean.data_ptr(), B, C, HW, K, _st())
        else:
            ws = _nan(cuda, int(lib.tcam_wgap_s3_ws_bytes(B, C, HW)) // 4)
            rc = _sym("tcam_wgap", lay)(xs.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                        logits.data_ptr(), mean.data_ptr(), ws.data_ptr(), B, C,
                                        HW, K, _st())
        assert rc == 0
        return logits, mean
    logits, mean = _twice(run)
    ref = R.wgap_ref(x64, c["w"], c["b"], lay)
    _report(f"wgap {lay} {B}x{C}x{HW}x{K}",
            {"mean": R.ratio(mean.cpu(), ref["mean"], ref["b_mean"]),
             "logits": R.ratio(logits.cpu(), ref["logits"], ref["b_logits"])})


# ------------------------------------------------------------------------ seghead
def _seghead(lay, xs, wd, bd, B, Cin, H, W, argmax, cuda):
    fc, cam, u8 = _nan(cuda, B, 2, H, W), _nan(cuda, B, H, W), _u8(cuda, B, H, W)
    assert _sym("tcam_seghead_cam", lay)(xs.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                         fc.data_ptr(), cam.data_ptr(), u8.data_ptr(), B, Cin, H,
                                         W, argmax, _st()) == 0
    return fc, cam, u8


@pytest.mark.parametrize("argmax", [0, 1])
@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("B,Cin,H,W", R.SEG_SHAPES)
def test_seghead_cam_matches_fp64(cuda, B, Cin, H, W, lay, argmax):
    c = R.seg_input(B, Cin, H, W, seed=Cin + H)
    xs, x64 = _put(c["x"], lay, cuda)
    wd, bd = c["w"].to(cuda), c["b"].to(cuda)
    fc, cam, u8 = _run(lambda: _seghead(lay, xs, wd, bd, B, Cin, H, W, argmax, cuda))
    ref = R.seghead_ref(x64, c["w"], c["b"], bool(argmax))
    tag = f"seghead {lay} {B}x{Cin}x{H}x{W} argmax {argmax}"
    _report(tag, {"fcams": R.ratio(fc.cpu(), ref["fcams"], ref["b_fcams"]),
                  "cam": R.ratio(cam.cpu(), ref["cam"], ref["b_cam"])})
    _u8_ratios(tag, u8, cam, ref["cam"], ref["b_cam"])


@pytest.mark.parametrize("argmax", [0, 1])
@pytest.mark.parametrize("lay", R.LAYS)
def test_seghead_cam_nan_input_gives_zero_cam(cuda, lay, argmax):
    """One NaN input element on an edge and one inside: fcams NaN, cam 0 and u8 0 on the six and
    nine pixels that read them (nan_to_num), everything else within its bound."""
    B, Cin, H, W = 2, 16, 20, 24
    c = R.seg_input(B, Cin, H, W, seed=36)
    x = c["x"].clone()
    x[1, 3, 0, 5] = NAN
    x[0, 9, 7, 7] = NAN
    xs, x64 = _put(x, lay, cuda)
    fc, cam, u8 = _run(lambda: _seghead(lay, xs, c["w"].to(cuda), c["b"].to(cuda), B, Cin, H, W,
                                        argmax, cuda))
    ref = R.seghead_ref(x64, c["w"], c["b"], bool(argmax))
    nan = torch.isnan(ref["fcams"][:, 0])
    assert int(nan.sum()) == 15
    assert not cam.cpu()[nan].any() and not u8.cpu()[nan].any()
    tag = f"seghead nan {lay} argmax {argmax}"
    _report(tag, {"fcams": R.nan_ratio(fc.cpu(), ref["fcams"], ref["b_fcams"]),
                  "cam": R.ratio(cam.cpu(), ref["cam"], ref["b_cam"])})
    _u8_ratios(tag, u8, cam, ref["cam"], ref["b_cam"])


# ------------------------------------------------------------------------ std_cam
def _std_cam(lay, As, wd, cd, B, C, h, w, Ho, Wo, cuda, expect=0):
    low, cam, u8 = _nan(cuda, B, h, w), _nan(cuda, B, Ho, Wo), _u8(cuda, B, Ho, Wo)
    rc = _sym("tcam_std_cam", lay)(As.data_ptr(), wd.data_ptr(), cd.data_ptr(), low.data_ptr(),
                                   cam.data_ptr(), u8.data_ptr(), B, C, h, w, Ho, Wo, _st())
    assert rc == expect
    return low, cam, u8


def _std_check(tag, lay, A, fw, cls, Ho, Wo, cuda):
    B, C, h, w = A.shape
    As, A64 = _put(A, lay, cuda)
    wd, cd = fw.to(cuda), cls.to(cuda)
    low, cam, u8 = _run(lambda: _std_cam(lay, As, wd, cd, B, C, h, w, Ho, Wo, cuda))
    ref = R.std_cam_ref(A64, fw, cls, Ho, Wo, lay)
    _report(tag, {"low": R.ratio(low.cpu(), ref["low"], ref["b_low"]),
                  "cam": R.ratio(cam.cpu(), ref["cam"], ref["b_cam"])})
    _u8_ratios(tag, u8, cam, ref["cam"], ref["b_cam"])
    return A64, ref, low.cpu(), cam.cpu()


@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("C,h,w,Ho,Wo", R.STD_SHAPES)
def test_std_cam_matches_fp64(cuda, C, h, w, Ho, Wo, lay):
    c = R.std_input(C, h, w, seed=C + h)
    _, ref, low, cam = _std_check(f"std_cam {lay} {C}x{h}x{w}->{Ho}x{Wo}", lay, c["A"], c["w"],
                                  c["cls"], Ho, Wo, cuda)
    if h * w == 1:
        assert not low.any() and not cam.any()


@pytest.mark.parametrize("lay", R.LAYS)
def test_std_cam_refuses_more_than_4096_positions(cuda, lay):
    """h w = 4097: TCAM_E_ARG before any launch, the filled outputs untouched."""
    C, h, w = R.STD_REFUSED
    c = R.std_input(C, 1, 1, seed=1)
    As, _ = _put(torch.zeros(2, C, h, w), lay, cuda)
    low, cam, u8 = _std_cam(lay, As, c["w"].to(cuda), c["cls"].to(cuda), 2, C, h, w, 5, 5, cuda,
                            expect=E_ARG)
    torch.cuda.synchronize()
    assert torch.isnan(low).all() and torch.isnan(cam).all() and bool((u8 == 0xA5).all())


@pytest.mark.parametrize("lay", R.LAYS)
def test_std_cam_drops_a_nan_feature(cuda, lay):
    """One NaN feature element: nansum drops that term, the map stays finite and bounded."""
    C, h, w, Ho, Wo = 64, 7, 7, 28, 28
    c = R.std_input(C, h, w, seed=C + h)
    A = c["A"].clone()
    A[0, 4, 3, 3] = NAN
    A64, ref, low, _ = _std_check(f"std_cam nan feature {lay}", lay, A, c["w"], c["cls"], Ho, Wo,
                                  cuda)
    assert bool(torch.isnan(A64[0, 4, 3, 3])) and float(low[0].max()) == 1.0
    sd = {"classification_head.fc.weight": c["w"]}
    assert float((M.std_cam(sd, A64[0].float(), int(c["cls"][0]), (Ho, Wo))[0] - low[0])
                 .abs().max()) < 1e-5


@pytest.mark.parametrize("lay,how", [(lay, "overflow") for lay in R.LAYS] +
                         [("f32", "inf"), ("s1", "inf")])
def test_std_cam_nan_position_zeroes_the_map(cuda, lay, how):
    """A position whose weighted sum is (+inf) + (-inf) — from finite features by fp32 overflow
    of the products (every form), or from inf features (the forms that can hold one): low.min()
    is NaN in the reference, so the frame's whole map, CAM and u8 are 0; the other frame of the
    batch is untouched."""
    C, h, w, Ho, Wo = 64, 7, 7, 28, 28
    c = R.std_input(C, h, w, seed=C + h)
    A, fw = c["A"].clone(), c["w"].clone()
    k = int(c["cls"][0])
    big, val = (3e38, 4.0) if how == "overflow" else (1.5, float("inf"))
    fw[k, 8], fw[k, 9] = big, -big
    A[0, 8:10] = 0
    A[0, 8:10, 2, 5] = val
    A64, ref, low, cam = _std_check(f"std_cam nan position {lay} {how}", lay, A, fw, c["cls"], Ho,
                                    Wo, cuda)
    sd = {"classification_head.fc.weight": fw}
    ora = M.std_cam(sd, A64[0].float(), k, (Ho, Wo))
    assert not ora[0].any() and not ora[1].any()
    assert not low[0].any() and not cam[0].any() and bool(low[1].any())


# ----------------------------------------------------------------------- temporal
def _temporal_max(cd, idd, M_, k1, hw, t, cuda):
    out = _nan(cuda, M_, hw)
    assert _lib.load().tcam_temporal_max(cd.data_ptr(), idd.data_ptr(), out.data_ptr(), M_, k1,
                                         hw, t, _st()) == 0
    return (out,)


def _temporal_cam(cd, idd, M_, k1, hw, t, cuda):
    out, u8, ws = _nan(cuda, M_, hw), _u8(cuda, M_, hw), _nan(cuda, R.TMP_N)
    assert _lib.load().tcam_temporal_cam(cd.data_ptr(), R.TMP_N, idd.data_ptr(), out.data_ptr(),
                                         u8.data_ptr(), M_, k1, hw, t, ws.data_ptr(), _st()) == 0
    return out, u8


def _temporal_both(tag, cams, idx, t, cuda):
    """tcam_temporal_max on the rows of idx and tcam_temporal_cam on those plus a row whose
    neighbours are all absent, against the same reference."""
    k1, hw = len(idx[0]), cams.shape[1]
    cd = cams.to(cuda)
    rows = idx + [R.TMP_ABSENT_ROW[:k1]]
    ref, bound = R.temporal_ref(cams.double(), rows, t)
    idd = torch.tensor(idx, dtype=torch.int32, device=cuda)
    (out,) = _twice(lambda: _temporal_max(cd, idd, len(idx), k1, hw, t, cuda))
    idr = torch.tensor(rows, dtype=torch.int32, device=cuda)
    full, u8 = _run(lambda: _temporal_cam(cd, idr, len(rows), k1, hw, t, cuda))
    _report(tag, {"max": R.nan_ratio(out.cpu(), ref[:-1], bound[:-1]),
                  "cam": R.nan_ratio(full.cpu(), ref, bound)})
    assert not full.cpu()[-1].any() and not u8.cpu()[-1].any()
    _u8_ratios(tag, u8, full, ref, bound)
    return ref, out.cpu(), full.cpu(), u8.cpu()


@pytest.mark.parametrize("t", R.TMP_T)
@pytest.mark.parametrize("k1", [1, 3])
@pytest.mark.parametrize("hw", R.TMP_FRAMES)
def test_temporal_max_and_cam_match_fp64(cuda, hw, k1, t):
    cams = R.tmp_input(*hw, seed=hw[0] + k1)
    ref, out, full, _ = _temporal_both(f"temporal {hw[0]}x{hw[1]} k1 {k1} t {t:g}", cams,
                                       R.TMP_IDX[k1], t, cuda)
    if t == 0:
        assert torch.equal(out.double(), ref[:-1]) and torch.equal(full.double(), ref)


@pytest.mark.parametrize("t", R.TMP_T)
def test_temporal_nan_pixel_follows_the_oracle(cuda, t):
    """A NaN pixel in one neighbour frame.  t = 0: that output pixel is NaN, its u8 0.  t > 0:
    re_normalize_cam divides by e.max() = NaN, so after nan_to_num the whole frame contributes
    zeros — the rows that read it are the maximum of their other frames."""
    cams = R.tmp_input(33, 40, seed=7)
    cams[3, 517] = NAN
    ref, out, full, u8 = _temporal_both(f"temporal nan t {t:g}", cams, R.TMP_IDX[3], t, cuda)
    if t == 0:
        assert bool(torch.isnan(out[1, 517])) and int(torch.isnan(out).sum()) == 1
        assert bool(torch.isnan(full[1, 517])) and int(u8[1, 517]) == 0
    else:
        assert not torch.isnan(out).any() and not torch.isnan(full).any()
        ora = M.temporal_max([cams[f] for f in R.TMP_IDX[3][1]], t=R.f32(t))
        assert float((ora - out[1]).abs().max()) < 1e-5


# --------------------------------------------------------------------------- top-k
@pytest.mark.parametrize("name", ["ties", "C3", "C1000", "nan"])
def test_topk_flags_follow_the_stable_sort(cuda, name):
    logits, target = R.topk_cases()[name]
    B, C = logits.shape
    ld, td = logits.to(cuda).contiguous(), target.int().to(cuda)

    def run():
        t1 = torch.full((B,), -7, dtype=torch.int32, device=cuda)
        t5 = torch.full((B,), -7, dtype=torch.int32, device=cuda)
        assert _lib.load().tcam_topk_flags(ld.data_ptr(), td.data_ptr(), t1.data_ptr(),
                                           t5.data_ptr(), B, C, _st()) == 0
        return t1, t5
    t1, t5 = _twice(run)
    r1, r5 = R.topk_ref(logits, target)
    assert torch.equal(t1.cpu(), r1), (name, "top1")
    assert torch.equal(t5.cpu(), r5), (name, "top5")
