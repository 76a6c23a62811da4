"""Direct fp64 checks of tcam_grad_cam{,_s3,_s2,_s1} through the C ABI: every method (GradCam,
GradCAMpp, XGradCAM, LayerCAM) in every storage form of the hooked features, B = 2 frames of
different classes.  References, bounds, shapes and inputs: tests/grad_cam_ref.py (pinned to
the reference's own maps by tests/test_grad_cam_ref.py, which also shows that the reference
alone decides all but 0.5 % of the uint8 pixels of every input used here).  The conventions
are those of tests/test_x_infer_tail_gpu.py: every operand is the value the device stored,
every bound is elementwise, every output is filled with NaN (uint8: 0xA5) before the call,
every call is made twice and compared bit for bit, the uint8 must be floor(double(the
device's CAM) * 255) everywhere and floor(reference * 255) wherever the reference decides.

Measured on an MI355X (the whole file, 252 cases, runs in 3 s), worst error / bound over all
methods and inputs: low 0.20, 0.13, 0.13, 0.11 and cam 0.15, 0.14, 0.14, 0.16 (plain, S3, S2,
S1); uint8 pixels left undecided: 0.21 % at the most."""
import pytest
import torch

import grad_cam_ref as G
import infer_tail_ref as R
from tcam_wsol_video_amd import _lib
from test_gpu_enc_train import _st
from test_x_infer_tail_gpu import E_ARG, _put, _run, _sym, _u8, _u8_ratios
from test_x_train_fwd_gpu import _nan, _report

pytestmark = pytest.mark.gpu


def _grad_cam(lay, As, wd, cd, ed, method, B, C, h, w, Ho, Wo, cuda, expect=0):
    lib = _lib.load()
    low, cam, u8 = _nan(cuda, B, h, w), _nan(cuda, B, Ho, Wo), _u8(cuda, B, Ho, Wo)
    ws = _nan(cuda, max(1, int(lib.tcam_grad_cam_ws_bytes(B, C, h * w)) // 4))
    rc = _sym("tcam_grad_cam", lay)(As.data_ptr(), wd.data_ptr(), cd.data_ptr(),
                                    ed.data_ptr() if ed is not None else None,
                                    G.METHOD_ID[method], ws.data_ptr(), low.data_ptr(),
                                    cam.data_ptr(), u8.data_ptr(), B, C, h, w, Ho, Wo, _st())
    assert rc == expect
    return low, cam, u8


def _check(tag, lay, method, A, fw, cls, Ho, Wo, cuda, exps=None):
    """A: the features the device stores (already times 2^exps when ``exps``)."""
    B, C, h, w = A.shape
    As, A64 = _put(A, lay, cuda)
    wd, cd = fw.to(cuda), cls.to(cuda)
    ed = exps.to(cuda) if exps is not None else None
    low, cam, u8 = _run(lambda: _grad_cam(lay, As, wd, cd, ed, method, B, C, h, w, Ho, Wo, cuda))
    ref = G.grad_cam_ref(A64, fw, cls, Ho, Wo, lay, method, exps)
    _report(tag, {"low": R.ratio(low.cpu(), ref["low"], ref["b_low"]),
                  "cam": R.ratio(cam.cpu(), ref["cam"], ref["b_cam"])})
    _u8_ratios(tag, u8, cam, ref["cam"], ref["b_cam"])
    return A64, ref, low.cpu(), cam.cpu()


@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("shape,kind", G.CASES)
def test_grad_cam_matches_fp64(cuda, shape, kind, method, lay):
    C, h, w, Ho, Wo = shape
    c = G.gpu_input(C, h, w, kind)
    _, ref, low, cam = _check(f"grad_cam {method} {lay} {kind} {C}x{h}x{w}->{Ho}x{Wo}", lay,
                              method, c["A"], c["w"], c["cls"], Ho, Wo, cuda)
    if h * w == 1 or kind == "nonpos_row":
        # one position, or a class row <= 0: 0 / 0, an all-zero map
        assert not low[0].any() and not cam[0].any()
    if h * w > 1:
        assert float(low[1].max()) == 1.0


@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("C,h,w,Ho,Wo", G.SHAPES[:2])
def test_grad_cam_s2_exponents(cuda, C, h, w, Ho, Wo, method):
    """S2 features stored times 2^e per channel with ``exps`` = e: the map of the unscaled
    features (the exponent cancels in XGradCAM's ratio and is taken out of every weight)."""
    c = G.gpu_input(C, h, w, "dead")
    e = G.exps_input(C)
    scaled = c["A"] * torch.pow(2.0, e.float())[None, :, None, None]
    tag = f"grad_cam exps {method} {C}x{h}x{w}"
    A64, ref, low, cam = _check(tag, "s2", method, scaled, c["w"], c["cls"], Ho, Wo, cuda, exps=e)
    plain = G.grad_cam_ref(A64 * torch.pow(2.0, -e.double())[None, :, None, None], c["w"],
                           c["cls"], Ho, Wo, "s2", method)
    assert torch.equal(plain["low"], ref["low"])
    # without the exponents the device computes another map
    As, _ = _put(scaled, "s2", cuda)
    other, _, _ = _grad_cam("s2", As, c["w"].to(cuda), c["cls"].to(cuda), None, method, 2, C, h, w,
                            Ho, Wo, cuda)
    assert not R.accept(other.cpu(), ref["low"], ref["b_low"])


@pytest.mark.parametrize("lay", R.LAYS)
def test_grad_cam_refuses_bad_geometry(cuda, lay):
    """h w = 4097, a method that does not exist and a missing workspace: TCAM_E_ARG before
    any launch, the filled outputs untouched."""
    C, h, w = G.REFUSED
    c = G.gpu_input(C, 1, 1, "dead")
    lib = _lib.load()
    As, _ = _put(torch.zeros(2, C, h, w), lay, cuda)
    wd, cd = c["w"].to(cuda), c["cls"].to(cuda)
    low, cam, u8 = _grad_cam(lay, As, wd, cd, None, "LayerCAM", 2, C, h, w, 5, 5, cuda,
                             expect=E_ARG)
    torch.cuda.synchronize()
    assert torch.isnan(low).all() and torch.isnan(cam).all() and bool((u8 == 0xA5).all())
    As, _ = _put(torch.zeros(2, C, 4, 4), lay, cuda)
    low, cam, u8 = _nan(cuda, 2, 4, 4), _nan(cuda, 2, 5, 5), _u8(cuda, 2, 5, 5)
    ws = _nan(cuda, int(lib.tcam_grad_cam_ws_bytes(2, C, 16)) // 4)
    fn = _sym("tcam_grad_cam", lay)
    for method, wsp, Ho in ((4, ws.data_ptr(), 5), (-1, ws.data_ptr(), 5), (3, None, 5),
                            (3, ws.data_ptr(), 0)):
        assert fn(As.data_ptr(), wd.data_ptr(), cd.data_ptr(), None, method, wsp,
                  low.data_ptr(), cam.data_ptr(), u8.data_ptr(), 2, C, 4, 4, Ho, 5,
                  _st()) == E_ARG
    if lay != "f32":
        assert fn(As.data_ptr(), wd.data_ptr(), cd.data_ptr(), None, 3, ws.data_ptr(),
                  low.data_ptr(), cam.data_ptr(), u8.data_ptr(), 2, C - 1, 4, 4, 5, 5,
                  _st()) == E_ARG
    torch.cuda.synchronize()
    assert torch.isnan(low).all() and torch.isnan(cam).all() and bool((u8 == 0xA5).all())


@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("method", G.METHODS)
def test_grad_cam_drops_a_nan_feature(cuda, lay, method):
    """One NaN feature element: nansum drops that term (XGradCAM: the channel's sum is NaN, so
    its weight is, and the whole channel is dropped); the map stays finite and bounded."""
    c, (Ho, Wo) = G.nan_feature_input()
    A64, ref, low, _ = _check(f"grad_cam nan feature {method} {lay}", lay, method, c["A"],
                              c["w"], c["cls"], Ho, Wo, cuda)
    assert bool(torch.isnan(A64[0, 5, 3, 3])) and float(low[0].max()) == 1.0
    assert bool(torch.isfinite(low).all())


@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("method", G.METHODS)
def test_grad_cam_nan_position_zeroes_the_map(cuda, lay, method):
    """A position whose weighted sum overflows fp32 — (+inf) + (-inf) = NaN under GradCam and
    XGradCAM, +inf under LayerCAM and GradCAM++, whose ReLU removes the negative weight: the
    minimum or the maximum is not finite, so the frame's whole map, CAM and u8 are 0, as the
    reference's normalisation followed by nan_to_num gives; the other frame is untouched."""
    c, (Ho, Wo) = G.nan_position_input()
    A64, ref, low, cam = _check(f"grad_cam nan position {method} {lay}", lay, method, c["A"],
                                c["w"], c["cls"], Ho, Wo, cuda)
    assert not ref["low"][0].any() and bool(ref["low"][1].any())
    assert not low[0].any() and not cam[0].any() and bool(low[1].any())
