"""The VGG16 stage-1 kernels (csrc/vgg_train.hip) one by one against fp64 on the operands as
the device stored them, in both forms (_s3s2: gradients S3, activations S2; _s1: the AMP
step's fp16 tensors): the MaxPool2d(2, 2) backward against torch's CPU backward, the ReLU
backward with its bias gradient and channel maxima, and the geometry refusals."""
import pytest
import torch
import torch.nn.functional as F

from tcam_wsol_video_amd import _lib, ops
from test_gpu_enc_train import _act, _nchw, _st

pytestmark = pytest.mark.gpu

FORMS = {"s3s2": ("f16x3", "x6", "s3"), "s1": ("amp", "amp", "s1")}   # act fmt, grad fmt, glay


# ------------------------------------------------------------------ pool backward
@pytest.mark.parametrize("form", ["s3s2", "s1"])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("H,W", [(6, 10), (9, 11)])
def test_maxpool2x2_bwd_equals_torch_cpu(cuda, form, C, H, W):
    """gin == torch.nn.functional.max_pool2d's CPU backward exactly: small integers force
    ties (the first maximum in (kh, kw) order takes the gradient), one window is all zero,
    one holds a NaN (NaN wins); with odd H / W the pool floors and the last row / column
    gets zero."""
    afmt, gfmt, glay = FORMS[form]
    B = 2
    g = torch.Generator().manual_seed(C + H * W)
    x = torch.randint(0, 3, (B, C, H, W), generator=g).float()
    x[0, :, 2:4, 4:6] = 0.0                 # an all-zero window
    x[1, 1, 3, 7] = float("nan")            # window (1, 3), tap (1, 1)
    x[1, 2, 0, 0] = float("nan")            # two NaNs in one window: the later one wins
    x[1, 2, 1, 1] = float("nan")
    Ho, Wo = H // 2, W // 2
    gout = torch.randn(B, C, Ho, Wo, generator=g)
    xs, gs = _act(x, cuda, afmt), _act(gout, cuda, gfmt)
    gin = ops.lay_empty(glay, B, H, W, C, cuda)
    gin.view(torch.int16).fill_(0x3c00 if glay == "s1" else 0x3f80)   # ones: every pixel is written
    fn = getattr(_lib.load(), f"tcam_maxpool2x2_bwd_{form}")
    assert fn(gs.data_ptr(), xs.data_ptr(), gin.data_ptr(), B, C, H, W, Ho, Wo, _st()) == 0
    xr = _nchw(xs).requires_grad_(True)
    assert torch.isnan(xr).sum() == 3
    F.max_pool2d(xr, 2, 2).backward(_nchw(gs))
    got = _nchw(gin)
    assert torch.equal(got, xr.grad)
    if H % 2:
        assert torch.equal(got[:, :, -1], torch.zeros_like(got[:, :, -1]))
    if W % 2:
        assert torch.equal(got[:, :, :, -1], torch.zeros_like(got[:, :, :, -1]))
    assert got[1, 1, 3, 7] == _nchw(gs)[1, 1, 1, 3] and got[1, 2, 1, 1] == _nchw(gs)[1, 2, 0, 0]


# ------------------------------------------------------------------ ReLU backward
def _relu_bwd(form, dout, out, want_amax=True):
    lib = _lib.load()
    B, H, W, C = ops.s3_dims(out)
    P = B * H * W
    nb = lib.tcam_relu_bwd_ws_bytes(P, C)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=out.device)
    dz = torch.empty_like(dout)
    db = torch.full((C,), float("nan"), device=out.device)
    amax = torch.full((C,), -1, dtype=torch.int32, device=out.device) if want_amax else None
    fn = getattr(lib, f"tcam_relu_bwd_{form}")
    assert fn(dout.data_ptr(), out.data_ptr(), dz.data_ptr(), db.data_ptr(),
              amax.data_ptr() if want_amax else None, P, C, ws.data_ptr(), nb, _st()) == 0
    return dz, db, amax


# C = 8: 256 pixel rows per block; 24: a group count that does not divide the block (idle
# threads); 64 / 512: the VGG widths; 2 x 8 x 384 x 384: more pixels than one pass of the
# fixed 1024-block grid covers (the grid-stride loop)
@pytest.mark.parametrize("form", ["s3s2", "s1"])
@pytest.mark.parametrize("B,C,H,W", [(2, 8, 9, 11), (2, 24, 9, 11), (2, 64, 36, 44),
                                     (3, 512, 5, 7), (2, 8, 384, 384)])
@pytest.mark.parametrize("dmag", [1.0, 1e-7])
def test_relu_bwd_matches_fp64(cuda, form, B, C, H, W, dmag):
    """dz is exact (a copy of dout or 0); db within the bound test_grad_chain_gpu.py holds
    dbeta to — 1e-6 of sum |dz|, the same per-channel fp32 sum (_s1: plus the fp16 rounding
    of the result the AMP form applies, half an ulp: 2^-11 |db|, 2^-25 below the normal
    range); amax equals the written max |dz| bit for bit; a channel with out <= 0 everywhere
    gives dz = 0, db = 0 and scale 2^126 after tcam_dy_scaled_s2."""
    afmt, gfmt, glay = FORMS[form]
    if form == "s1":   # fp16 gradients and an fp16 db: keep both inside fp16's range
        dmag = 1e-2 if dmag == 1.0 else 1e-3
    g = torch.Generator().manual_seed(B * C + H)
    out = torch.randn(B, C, H, W, generator=g).clamp(min=0)
    dead = 3 if C > 8 else 5
    out[:, dead] = 0.0
    dout = torch.randn(B, C, H, W, generator=g) * dmag * \
        torch.logspace(-2, 2, C)[None, :, None, None]
    outs, ds = _act(out, cuda, afmt), _act(dout, cuda, gfmt)
    dz, db, amax = _relu_bwd(form, ds, outs)
    d64, mask = _nchw(ds), _nchw(outs) > 0
    ref = d64 * mask
    got = _nchw(dz)
    assert torch.equal(got, ref)
    ref_db, mag = ref.sum((0, 2, 3)), ref.abs().sum((0, 2, 3))
    bound = 1e-6 * mag
    if form == "s1":
        bound = bound + 2.0 ** -11 * ref_db.abs() + 2.0 ** -25
    err = (db.double().cpu() - ref_db).abs()
    live = mag > 0
    worst = float((err[live] / bound[live]).max())
    print(f"{form} {B}x{C}x{H}x{W} dmag {dmag:g}: db {worst:.3g} of the bound")
    assert (err <= bound).all(), worst
    assert torch.equal(amax.view(torch.float32).cpu().double(), got.abs().amax((0, 2, 3)))
    assert float(db[dead]) == 0.0 and int(amax[dead]) == 0 and not got[:, dead].any()
    if form == "s3s2":
        scale = torch.empty(C, device=cuda)
        dy2 = ops.s2_empty(B, H, W, C, cuda)
        assert _lib.load().tcam_dy_scaled_s2(dz.data_ptr(), B * H * W, C, amax.data_ptr(), 0,
                                             scale.data_ptr(), dy2.data_ptr(), _st()) == 0
        assert float(scale[dead]) == 2.0 ** 126 and not _nchw(dy2)[:, dead].any()
        s = scale.double().cpu()
        top = _nchw(dy2).abs().amax((0, 2, 3))
        assert ((top[live] >= 2.0 ** 14 * (1 - 2.0 ** -20)) & (top[live] < 2.0 ** 15)).all()
        assert torch.equal(torch.frexp(s)[0], torch.full_like(s, 0.5))
    else:   # the AMP form needs no maxima: amax may be NULL
        dz2, db2, _ = _relu_bwd(form, ds, outs, want_amax=False)
        assert torch.equal(_nchw(dz2), got) and torch.equal(db2, db)


def test_relu_bwd_is_deterministic(cuda):
    g = torch.Generator().manual_seed(4)
    out = _act(torch.randn(2, 64, 36, 44, generator=g).clamp(min=0), cuda, "f16x3")
    ds = _act(torch.randn(2, 64, 36, 44, generator=g), cuda, "x6")
    a, b = _relu_bwd("s3s2", ds, out), _relu_bwd("s3s2", ds, out)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("form", ["s3s2", "s1"])
def test_geometry_refusals_return_an_error_without_launching(cuda, form):
    """A C that is no multiple of 8, a wrong Ho / Wo, a null pointer, aliased output and a
    short workspace return a non-zero status; the output buffers keep their sentinel."""
    lib = _lib.load()
    buf = lambda: torch.full((1 << 16,), 0x5a, dtype=torch.uint8, device=cuda)
    a, b, c, d, ws = buf(), buf(), buf(), buf(), buf()
    amax = buf()
    relu = getattr(lib, f"tcam_relu_bwd_{form}")
    pool = getattr(lib, f"tcam_maxpool2x2_bwd_{form}")
    P = 6 * 10
    nb = lib.tcam_relu_bwd_ws_bytes(P, 16)
    assert nb > 0 and lib.tcam_relu_bwd_ws_bytes(P, 12) == 0
    ok = (a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), amax.data_ptr())
    assert relu(*ok, P, 12, ws.data_ptr(), ws.numel(), _st()) != 0
    assert relu(*ok, 0, 16, ws.data_ptr(), ws.numel(), _st()) != 0
    assert relu(*ok, P, 16, ws.data_ptr(), nb - 1, _st()) != 0
    assert relu(*ok, P, 16, None, nb, _st()) != 0
    assert relu(a.data_ptr(), b.data_ptr(), a.data_ptr(), d.data_ptr(), None, P, 16,
                ws.data_ptr(), nb, _st()) != 0
    assert relu(None, b.data_ptr(), c.data_ptr(), d.data_ptr(), None, P, 16, ws.data_ptr(), nb,
                _st()) != 0
    for H, W, Ho, Wo, C in ((6, 10, 3, 5, 12), (6, 10, 4, 5, 8), (7, 10, 4, 5, 8),
                            (6, 11, 3, 6, 8), (1, 10, 0, 5, 8)):
        assert pool(a.data_ptr(), b.data_ptr(), c.data_ptr(), 1, C, H, W, Ho, Wo, _st()) != 0
    assert pool(a.data_ptr(), b.data_ptr(), None, 1, 8, 6, 10, 3, 5, _st()) != 0
    assert pool(a.data_ptr(), b.data_ptr(), b.data_ptr(), 1, 8, 6, 10, 3, 5, _st()) != 0
    torch.cuda.synchronize()
    for t in (c, d, amax, ws):
        assert bool((t == 0x5a).all())
