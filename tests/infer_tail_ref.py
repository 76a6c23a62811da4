"""fp64 references, elementwise bounds, shapes and input builders of the inference tail's
kernel tests (tests/test_infer_tail_ref.py on the CPU, tests/test_x_infer_tail_gpu.py on the
device): the pools, the decoder's nearest-x2 + bilinear resample and its adjoint, WGAP, the
segmentation head + CAM, the fcams resize + CAM, the STD_CL CAM, the temporal CAM maximum and
the top-k flags, in the four storage forms of the activations ("f32" = plain NCHW fp32, "s3",
"s2", "s1").

The conventions are those of tests/train_fwd_ref.py: every reference takes the operands as the
device stored them (:func:`stored`) and returns the fp64 result AND its per-element bound, n *
2^-24 * (sum of the magnitudes of the terms of that output) with n = the fp32 roundings on the
kernel's longest path (counted next to each bound) plus the rounding of the output's storage.
No bound is taken from a kernel's output; a scalar the ABI receives as float enters through
f32().  Non-finite inputs: S2 and S3 cannot hold an inf (the low parts become inf - inf), so
they get NaN only; the inf - inf of std_cam is made from finite features by fp32 overflow of
the products, which every form can hold.

std_cam, topk_flags and temporal_max index with the class, the target and the frame index
unchecked: no test here passes one out of range (left to a later change).
Plain torch, CPU only."""
import numpy as np
import torch
import torch.nn.functional as F

from train_fwd_ref import U, accept, f32, ratio, softmax2_ref, storage, store  # noqa: F401

LAYS = ["f32", "s3", "s2", "s1"]
FLT_MAX = float(np.finfo(np.float32).max)


def stored(x, lay):
    """fp32 in, the fp64 values the device holds in that storage form."""
    return store(x, "s3" if lay == "f32" else lay)


def out_storage(v, lay):
    return storage(v, "s3" if lay == "f32" else lay)


def nan_ratio(got, ref, bound):
    """ratio() of tensors that may hold NaN: the NaNs must sit at the same elements (NaN if
    not), the others are compared."""
    got, ref = got.double(), ref.double()
    if got.shape != ref.shape or not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return float("nan")
    keep = ~torch.isnan(ref)
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    return ratio(got[keep], ref[keep], bound.expand_as(ref)[keep])


# ------------------------------------------------------------------ uint8 and argmax
def u8_of(cam):
    """uint8(double(cam) * 255) of a CAM in [0, 1]; NaN gives 0."""
    v = torch.nan_to_num(cam.double(), nan=0.0) * 255.0
    return v.floor().to(torch.uint8)


def u8_decided(ref, bound):
    """The pixels whose uint8 the reference decides: ref * 255 farther than 255 bound from an
    integer, or a reference that is exact (bound 0)."""
    v = torch.nan_to_num(ref.double(), nan=0.0) * 255.0
    return ((v - v.round()).abs() > 255.0 * bound) | (bound == 0)


def u8_check(dev_u8, dev_cam, ref, bound):
    """(the device u8 is floor(double(device cam) * 255) everywhere, it is floor(ref * 255)
    at every decided pixel, the excluded fraction)."""
    dec = u8_decided(ref, bound)
    own = bool(torch.equal(dev_u8, u8_of(dev_cam))) if dev_cam is not None else True
    return own, bool((dev_u8 == u8_of(ref))[dec].all()), 1.0 - float(dec.double().mean())


U8_EXCLUDED_MAX = 0.005


# -------------------------------------------------------------------------- pools
# (C, H, W) with B = 2; maxpool3x3s2 and pool2d: a thread per (output pixel, 8-channel group)
POOL_SHAPES = [
    (8, 1, 1),       # one pixel: every window is one tap, eight of nine clamped / skipped
    (8, 2, 3),       # H 2: the window of row 1 hangs over the bottom edge
    (24, 13, 10),    # G 3, odd H: 2 x 7 x 5 x 3 = 210 threads, one partial block
    (16, 7, 8),      # G 2, even W: the last column's window holds one in-frame column
]
# (k, s, p, mode, ceil) of test_pool2d_s3_matches_torch, at these (H, W) with C = 24, B = 2
POOL2D_CFGS = [(2, 2, 0, "max", False), (3, 2, 1, "max", True), (3, 1, 1, "max", False),
               (3, 1, 1, "avg", False), (3, 2, 1, "avg", True), (3, 2, 0, "max", False)]
POOL2D_HW = [(8, 9), (29, 30)]
POOL_CONCAT = dict(C=16, H=11, W=13, cstride=40, coff=16, cfg=(3, 1, 1, "avg", False))


def pool_out(n, k, s, p, ceil):
    """torch's pooling output size (a last window that starts in the right padding is dropped)."""
    o = -(-(n + 2 * p - k) // s) + 1 if ceil else (n + 2 * p - k) // s + 1
    if ceil and (o - 1) * s >= n + p:
        o -= 1
    return o


def pool_cases():
    """(C, H, W, (k, s, p, mode, ceil)) of every pool2d case; windows larger than the frame
    only where torch accepts them (every window starts inside the padded input)."""
    for C, H, W in POOL_SHAPES:
        for cfg in POOL2D_CFGS:
            k, s, p = cfg[:3]
            if H + 2 * p >= k and W + 2 * p >= k:
                yield C, H, W, cfg
    for H, W in POOL2D_HW:
        for cfg in POOL2D_CFGS:
            yield 24, H, W, cfg


def pool_input(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=g) * 10.0 ** torch.randint(-1, 2, (1, C, 1, 1),
                                                                        generator=g)


def maxpool_ref(x64, k, s, p, ceil=False):
    """F.max_pool2d in fp64 on the stored values: a maximum rounds nothing and every stored
    value is representable in its own form, so the bound is 0 (torch.equal on the values); NaN
    propagates to exactly the windows that hold it."""
    r = F.max_pool2d(x64, k, s, p, ceil_mode=ceil)
    return r, torch.zeros_like(r)


def avgpool_ref(x64, k, s, p, ceil, lay, clipped_divisor=False):
    """avg_pool2d(count_include_pad=True): the in-frame taps summed row-major, divided by (hend
    - hstart)(wend - wstart) with hend = min(hstart + k, H + p) taken BEFORE clipping to the
    frame (ATen's ceil_mode rule: the padding counts, the overhang past it does not).
    taps additions (the first lands on 0) and the division: (taps + 1) 2^-24 sum |x| / div +
    storage.  clipped_divisor: the wrong kernel (divides by the in-frame count)."""
    B, C, H, W = x64.shape
    Ho, Wo = pool_out(H, k, s, p, ceil), pool_out(W, k, s, p, ceil)
    out = torch.zeros(B, C, Ho, Wo, dtype=torch.float64)
    bound = torch.zeros_like(out)
    for oy in range(Ho):
        hs = oy * s - p
        he = min(hs + k, H + p)
        for ox in range(Wo):
            ws = ox * s - p
            we = min(ws + k, W + p)
            win = x64[:, :, max(hs, 0):min(he, H), max(ws, 0):min(we, W)]
            taps = win.shape[2] * win.shape[3]
            div = taps if clipped_divisor else (he - hs) * (we - ws)
            out[:, :, oy, ox] = win.sum((2, 3)) / div
            bound[:, :, oy, ox] = (taps + 1) * U * win.abs().sum((2, 3)) / div
    return out, bound + out_storage(out, lay)


# --------------------------------------------------------------------- resamplers
def taps(n_in, n_out, align_corners):
    """ATen's fp32 source positions and weights of a bilinear resize along one axis, computed
    in numpy.float32: the scale as an fp32 quotient, r = fl32(scale * o) (align_corners) or
    max(fl32(fl32(scale * (o + 0.5)) - 0.5), 0), i0 = int(r), i1 = i0 + (i0 < n_in - 1), l1 =
    fl32(r - i0), l0 = fl32(1 - l1).  Returns i0, i1, l0, l1 (fp32 values as fp64) and what one
    rounding more or fewer of the product moves the position by: 2^-24 |product|, and 0 where
    the position is clamped to 0 from further below than that."""
    o = np.arange(n_out, dtype=np.float32)
    if align_corners:
        sc = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
        prod = sc * o
        r = prod
        da = U * np.abs(prod.astype(np.float64))
    else:
        sc = np.float32(n_in) / np.float32(n_out)
        prod = sc * (o + np.float32(0.5))
        r = np.maximum(prod - np.float32(0.5), np.float32(0))
        da = U * np.abs(prod.astype(np.float64))
        da = np.where(prod.astype(np.float64) - 0.5 < -da, 0.0, da)
    assert prod.dtype == np.float32 and r.dtype == np.float32
    i0 = r.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = r - i0.astype(np.float32)
    l0 = np.float32(1) - l1
    assert l0.dtype == np.float32
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    return (t(i0, torch.long), t(i1, torch.long), t(l0, torch.float64), t(l1, torch.float64),
            t(da, torch.float64))


def blend(x64, ty, tx, err=None):
    """The four-tap blend ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11) of (..., H, W) in
    fp64 with the fp32 weights of :func:`taps`.  Returns the value, the sum of the magnitudes
    of its terms, what 2^-24 relative on the two positions moves it by (2^-24 r |d v / d l1|
    per axis), and — with ``err``, a bound on x — that bound carried through (the weights are
    non-negative)."""
    y0, y1, ly0, ly1, py = ty
    x0, x1, lx0, lx1, px = tx
    ly0, ly1, py = ly0[:, None], ly1[:, None], py[:, None]
    g = lambda a, yy, xx: a[..., yy[:, None], xx[None, :]]

    def mix(a):
        v00, v01, v10, v11 = g(a, y0, x0), g(a, y0, x1), g(a, y1, x0), g(a, y1, x1)
        return ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
    v00, v01, v10, v11 = g(x64, y0, x0), g(x64, y0, x1), g(x64, y1, x0), g(x64, y1, x1)
    row0, row1 = lx0 * v00 + lx1 * v01, lx0 * v10 + lx1 * v11
    v = ly0 * row0 + ly1 * row1
    mag = mix(x64.abs())
    pos = py * (row1 - row0).abs() + px * (ly0 * (v01 - v00) + ly1 * (v11 - v10)).abs()
    return v, mag, pos, (mix(err) if err is not None else None)


# (H, W) -> (Ho, Wo) of tcam_up2_resize*, C in UP2R_C, B = 2: a thread per (output pixel, group)
UP2R_SHAPES = [
    ((7, 7), (14, 14)),    # scale 13 / 13 = 1: every weight 0 or 1, the nearest map itself
    ((5, 6), (9, 13)),     # non-integer positions on both axes, downsizing
    ((4, 4), (9, 9)),      # upsizing the nearest map: scale 7 / 8
    ((3, 5), (1, 1)),      # a one-pixel output: scale 0, every output reads in[0][0]
    ((6, 2), (12, 3)),     # scale 1 down, 3 / 2 across
    ((1, 1), (2, 2)),      # one input pixel: all four taps are the same pixel
]
UP2R_C = [8, 24]
UP2R_BWD_SHAPES = UP2R_SHAPES + [((14, 14), (13, 13))]     # scale 27 / 12 > 2: skipped rows


def act_input(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=g)


def up2_resize_ref(x64, Ho, Wo, lay):
    """nearest x2 (U[y][x] = x[y >> 1][x >> 1]) then bilinear(align_corners=True) to (Ho, Wo).
    Two products, two additions on the longest path (4) and one for l0 = fl32(1 - l1) when the
    compiler fuses the position (these kernels do not pin contraction off: fma(sh, oy, -y0)
    moves l1 by up to 2^-24 r): 5 2^-24 mag + the position allowance + storage."""
    H, W = x64.shape[-2:]
    up = x64.repeat_interleave(2, -2).repeat_interleave(2, -1)
    v, mag, pos, _ = blend(up, taps(2 * H, Ho, True), taps(2 * W, Wo, True))
    return v, 5 * U * mag + pos + out_storage(v, lay), pos


def up2_matrix(H, Ho):
    """(Ho, H) fp32 weights with which output row o reads input row y through the nearest
    map: w = 0; w += l0 if (i0 >> 1) == y; w += l1 if (i1 >> 1) == y, in fp32 as the adjoint
    kernel builds it; and what a fused position moves each weight by (as :func:`blend`)."""
    i0, i1, l0, l1, da = taps(2 * H, Ho, True)
    Wm = np.zeros((Ho, H), np.float32)
    o = np.arange(Ho)
    np.add.at(Wm, (o, i0.numpy() >> 1), l0.numpy().astype(np.float32))
    np.add.at(Wm, (o, i1.numpy() >> 1), l1.numpy().astype(np.float32))
    hit0 = F.one_hot(i0 >> 1, H).double()
    hit1 = F.one_hot(i1 >> 1, H).double()
    Am = da[:, None] * (hit1 - hit0).abs() + U * (hit0 * l0[:, None] + hit1 * l1[:, None])
    return torch.from_numpy(Wm).double(), Am


def up2_resize_bwd_ref(g64, H, W, lay):
    """The adjoint of up2_resize_ref: gx[y][x] = sum over (oy, ox) of (wy wx) g[oy][ox] with the
    fp32 weights of :func:`up2_matrix`, gathered in fp64.  The weight product, the product
    with g and N - 1 additions (the first lands on 0), N = the outputs with a non-zero weight:
    (N + 1) 2^-24 sum |w g| + the position allowance + storage."""
    Ho, Wo = g64.shape[-2:]
    Wy, Ay = up2_matrix(H, Ho)
    Wx, Ax = up2_matrix(W, Wo)
    e = lambda a, m, b: torch.einsum("oy,bcop,px->bcyx", a, m, b)
    v = e(Wy, g64, Wx)
    mag = e(Wy, g64.abs(), Wx)
    n = (Wy != 0).sum(0)[:, None] * (Wx != 0).sum(0)[None, :]
    pos = e(Ay, g64.abs(), Wx) + e(Wy, g64.abs(), Ax)
    return v, (n + 1) * U * mag + pos + out_storage(v, lay), pos


# (Hi, Wi) -> (Ho, Wo) of tcam_resize_cam, B = 2, argmax off and on: a thread per output pixel
RESIZE_CAM_SHAPES = [((30, 30), (29, 29)), ((10, 12), (7, 5)), ((5, 7), (11, 3)),
                     ((1, 5), (3, 5))]     # the last: one input row, an identity across


def fcams_input(B, H, W, seed):
    """Logit pairs of a few units with a smooth part, so that a resize has tap differences."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(B, 2, H, W, generator=g) * 2
    f[:, 1] += torch.linspace(-1, 1, W)[None, None, :]
    return f


def cam_of(a, b_a, argmax):
    """SegmentationCam of fcams a (B, 2, ...) known within b_a: cam = softmax(a, 1)[:, 1] with
    softmax2_ref's own bound (expf, the sum, the division, the rounded difference) plus S0 S1
    (b_a0 + b_a1) for the inputs (d S1 / d a = +-S0 S1); argmax: 1 where a1 > a0, decided
    (bound 0) where |a1 - a0| exceeds the two bounds' sum and undecided (bound 1) elsewhere.
    NaN logits give 0 (nan_to_num), exactly."""
    a0, a1 = a[:, 0], a[:, 1]
    nan = torch.isnan(a0) | torch.isnan(a1)
    if argmax:
        cam = (a1 > a0).double()
        bound = ((a1 - a0).abs() <= b_a[:, 0] + b_a[:, 1]).double()
    else:
        sh = a.shape
        S, bS = softmax2_ref(a.reshape(sh[0], 2, -1))
        S, bS = S.reshape(sh), bS.reshape(sh)
        cam = S[:, 1]
        bound = bS[:, 1] + S[:, 0] * S[:, 1] * (b_a[:, 0] + b_a[:, 1])
    zero = torch.zeros_like(cam)
    return torch.where(nan, zero, cam), torch.where(nan, zero, bound)


def resize_cam_ref(f64, Ho, Wo, argmax):
    """fcams (B, 2, Hi, Wi) -> bilinear(align_corners=True) -> cam.  The kernel pins
    contraction off, so its positions are ATen's: 4 2^-24 mag, no position allowance."""
    Hi, Wi = f64.shape[-2:]
    a, mag, pos, _ = blend(f64, taps(Hi, Ho, True), taps(Wi, Wo, True))
    b_a = 4 * U * mag
    cam, b_cam = cam_of(a, b_a, argmax)
    return dict(fcams=a, b_fcams=b_a, cam=cam, b_cam=b_cam, pos=pos)


# --------------------------------------------------------------------------- WGAP
# (B, C, HW, classes).  S3 / S2 / S1: pool_partial_kernel sums chunks of 32 pixels, a thread
# per group, blocks of max(64, G rounded up to 64) threads; pool_linear_kernel adds the chunks,
# divides and runs a wave per class.  Plain: a wave per plane, then a wave per (b, class).
WGAP_SHAPES = [
    (3, 64, 784, 10),      # 25 chunks, the last holds 16 pixels; G 8 in a block of 64
    (2, 2048, 63, 10),     # G 256; 2 chunks, the last 31 pixels; HW < 64 on the plain path
    (1, 8192, 15, 10),     # G 1024: 1024 threads, the widest the entry accepts; one chunk
    (2, 520, 37, 10),      # G 65: a second wave with one live lane
    (2, 8, 1, 10),         # one pixel, one group
    (2, 64, 784, 3),       # 3 classes: fewer classes than waves
]


def wgap_input(B, C, HW, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, HW, 1, generator=g).abs() * 0.5 - 0.1     # mostly positive, some < 0
    return dict(x=x, w=torch.randn(K, C, generator=g) * 0.05, b=torch.randn(K, generator=g) * 0.1)


def wgap_ref(x64, w, b, lay, drop_last_of_chunk=False):
    """mean over HW, then Linear, on the stored features (S1: the fp32-accurate mean and
    logits of the fp16 features, which is what the kernel computes — not autocast's fp16
    logits).  mean: layouts min(HW, 32) - 1 additions in a chunk, nchunks - 1 over the chunks,
    the division: (min(HW, 32) + nchunks - 1) 2^-24 sum |x| / HW; plain: ceil(HW / 64) per
    lane, 6 wave levels, the division.  logits: ceil(C / 64) products and additions per lane, 6
    wave levels, the bias: (2 ceil(C / 64) + 7) 2^-24 (sum |mean w| + |b|) + b_mean |w|.
    drop_last_of_chunk: the wrong kernel (the 32nd pixel of the first chunk is not read)."""
    B, C = x64.shape[:2]
    v = x64.reshape(B, C, -1)
    HW = v.shape[2]
    if drop_last_of_chunk:
        keep = torch.ones(HW, dtype=torch.bool)
        keep[31] = False
        v = v * keep
    n = (min(HW, 32) + -(-HW // 32) - 1) if lay != "f32" else (-(-HW // 64) + 7)
    mean = v.sum(2) / HW
    b_mean = n * U * v.abs().sum(2) / HW
    w64, b64 = w.double(), b.double()
    nl = 2 * -(-C // 64) + 7
    logits = mean @ w64.t() + b64
    b_logits = nl * U * (mean.abs() @ w64.abs().t() + b64.abs()) + b_mean @ w64.abs().t()
    return dict(mean=mean, b_mean=b_mean, logits=logits, b_logits=b_logits)


# ------------------------------------------------------------------- seghead + CAM
# (B, Cin, H, W), argmax off and on.  Layouts: a block per 16 x 16 tile with its 18 x 18 halo
# in LDS (Cin x 324 floats); plain: a thread per pixel.
SEG_SHAPES = [
    (2, 16, 20, 24),     # 2 x 2 tiles, ragged both ways
    (1, 64, 17, 33),     # Cin 64: the LDS limit (82944 B of halo); tiles of 1 row / 1 column
    (3, 8, 1, 1),        # one pixel: only the centre tap is inside the frame
    (1, 16, 16, 16),     # exactly one tile
    (1, 24, 2, 35),      # H 2: every pixel is on an edge row
]


def seg_input(B, Cin, H, W, seed):
    """Features of unit size and weights of 0.1 / (9 Cin), so that sum |w x| is about 0.06 at
    every Cin: with n = 9 Cin + 1 the CAM's bound then stays near 1e-6 and the uint8 of all but
    a pixel in a thousand is decided; the bias puts the CAM around 1 / 3."""
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn(B, Cin, H, W, generator=g),
                w=torch.randn(2, Cin, 3, 3, generator=g) * (0.1 / (9 * Cin)),
                b=torch.tensor([0.4, -0.3]))


def seghead_ref(x64, w, b, argmax):
    """fcams = conv3x3(x; w, b) (pad 1), cam, from the stored x.  A chain of 9 Cin fmaf and the
    bias: (9 Cin + 1) 2^-24 (sum |w x| + |b|).  A NaN x gives NaN fcams and cam 0 on the up to
    nine pixels that read it."""
    Cin = x64.shape[1]
    w64, b64 = w.double(), b.double()
    a = F.conv2d(x64, w64, b64, padding=1)
    fin = torch.nan_to_num(x64, nan=0.0)
    mag = F.conv2d(fin.abs(), w64.abs(), b64.abs(), padding=1)
    b_a = (9 * Cin + 1) * U * mag
    cam, b_cam = cam_of(a, b_a, argmax)
    return dict(fcams=a, b_fcams=b_a, cam=cam, b_cam=b_cam)


# ------------------------------------------------------------------------ std_cam
# (C, h, w, Ho, Wo), B = 2 with classes (1, 3) of 5: a block of 1024 threads per frame.
# Layouts: a wave per position, lanes over the G = C / 8 groups; plain: a thread per position.
STD_SHAPES = [
    (64, 7, 7, 28, 28),         # G 8: 56 idle lanes
    (2048, 7, 7, 224, 224),     # G 256: four passes per lane
    (24, 28, 28, 224, 224),     # G 3
    (8, 64, 64, 32, 32),        # h w = 4096: the LDS limit; downsizing by 2 (weights 1/2)
    (8, 1, 1, 5, 5),            # one position: low - min = 0, 0 / 0 -> 0: an all-zero map
    (520, 3, 5, 12, 20),        # G 65: one group past 64 lanes
    (512, 3, 5, 12, 20),        # G 64: every lane one group
]
STD_REFUSED = (8, 17, 241)      # h w = 4097
STD_CLS = (1, 3)


def std_input(C, h, w, seed, B=2):
    """Post-ReLU features under a smooth spatial gain, about 24 of the C channels alive per
    position (layer4's features are sparse), and class weights that are mostly positive: the
    map's range is then of the order of sum |w A| and the CAM's bound small enough to decide
    all but a few uint8 in a thousand (an exact zero term rounds nothing)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    cy, cx = torch.rand(B, generator=g) - 0.5, torch.rand(B, generator=g) - 0.5
    gain = 0.05 + 0.95 * torch.exp(-3 * ((yy - cy[:, None, None]) ** 2 +
                                         (xx - cx[:, None, None]) ** 2))
    A = torch.relu(torch.randn(B, C, h, w, generator=g)) + 0.1
    A = A * (torch.rand(B, C, h, w, generator=g) < min(1.0, 24.0 / C)) * gain[:, None]
    fw = torch.randn(5, C, generator=g).abs() + 0.1
    fw[:, 3::4] *= -0.25
    return dict(A=A, w=fw, cls=torch.tensor(STD_CLS[:B], dtype=torch.int32))


def _near(s, e, lowest):
    """The pixels that can be the minimum (maximum) of s known within e."""
    if lowest:
        return (s - e) <= (s + e).min()
    return (s + e) >= (s - e).max()


def std_cam_ref(A64, w, cls, Ho, Wo, lay, align_corners=False):
    """Per frame: low = nansum_c w[cls] A (the products as fp32: beyond FLT_MAX they are +-inf);
    low = (low - min) / max(low - min); nan_to_num; cam = bilinear(align_corners=False).
    s: layouts 16 ceil(G / 64) products and additions per lane and 6 wave levels; plain a
    product and an addition per term that is not an exact zero (those round nothing), 2 nnz: n
    2^-24 sum |w A|.  v = s - min: e_s + e_min + 2^-24 |v| with e_min the largest e_s among
    the pixels that can be the minimum; e_max likewise on v; low = v / max: (e_v + low e_max) /
    max + 2^-24 low.  cam: e_low through the blend + 5 2^-24 mag + the position allowance (as
    up2_resize_ref: the kernels do not pin contraction off).  A min or max that is NaN zeroes the whole map.
    align_corners: the wrong kernel."""
    B, C, h, w_ = A64.shape
    G = C // 8
    lows, b_lows = [], []
    for i in range(B):
        t = w[int(cls[i])].double()[:, None, None] * A64[i]
        t = torch.where(t.abs() > FLT_MAX, torch.sign(t) * float("inf"), t)
        s = torch.nansum(t, 0)
        n = 2 * (t != 0).sum(0) if lay == "f32" else 16 * -(-G // 64) + 6
        e_s = n * U * torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0).abs().sum(0)
        mn = s.min()
        v = s - mn
        mx = v.max()
        if not bool(torch.isfinite(mn) & torch.isfinite(mx)) or h * w_ == 1:
            # NaN / inf anywhere: (x - nan), x / inf, inf / inf -> 0 everywhere; one pixel: 0 / 0
            lows.append(torch.nan_to_num(v / mx, nan=0.0, posinf=1.0, neginf=0.0))
            b_lows.append(torch.zeros_like(s))
            continue
        lo_set = _near(s, e_s, True)
        e_v = e_s + e_s[lo_set].max() + U * v.abs()
        hi_set = _near(v, e_v, False)
        e_mx = e_v[hi_set].max()
        low = v / mx
        b_low = (e_v + low * e_mx) / mx + U * low
        # the only pixel that can be the minimum is s - s = 0, the only one that can be the
        # maximum v / v = 1: both exact
        if int(lo_set.sum()) == 1:
            b_low[lo_set] = 0.0
        if int(hi_set.sum()) == 1:
            b_low[hi_set] = 0.0
        lows.append(low)
        b_lows.append(b_low)
    low, b_low = torch.stack(lows), torch.stack(b_lows)
    cam, mag, pos, e = blend(low, taps(h, Ho, align_corners), taps(w_, Wo, align_corners), b_low)
    return dict(low=low, b_low=b_low, cam=cam, b_cam=e + 5 * U * mag + pos, pos=pos)


# ----------------------------------------------------------------------- temporal
# frames (h, w) of N = 7 CAMs in [0, 1]; idx (M, k1) with -1 = absent.  temporal_max: a block of
# 256 threads per output, the frame in strides of 256; temporal_cam: 4 pixels per thread as a
# float4 when hw % 4 == 0, pixel by pixel otherwise.
TMP_FRAMES = [(28, 28),    # hw 784 = 4 x 196: the vector path, one block
              (57, 61),    # hw 3477, odd: the scalar path, 4 blocks, the last thread 1 pixel
              (1, 3),      # hw 3 < 4: one thread, three live pixels
              (33, 40)]    # hw 1320 = 4 x 330: the vector path, two blocks
TMP_N = 7
TMP_T = [0.0, 0.7, 30.0]
TMP_IDX = {1: [[0], [3], [6]],
           3: [[0, 1, -1], [2, 3, 4], [-1, 5, -1], [6, 5, 4], [-1, -1, 6]]}
TMP_ABSENT_ROW = [-1, -1, -1]       # temporal_cam only: yields 0


def tmp_input(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(TMP_N, h * w, generator=g)


def renorm_ref(c64, t):
    """re_normalize_cam of one frame (hw,): e = exp((c + 1e-6) t), e / max e, nan_to_num, with
    the fp32 values of t and 1e-6.  The argument's two roundings move it by 2 2^-24 |arg|, expf
    is within an ulp (2), at the pixel and at the maximum, and the division: v (2 2^-24 (|arg|
    + |arg_max|) + 5 2^-24).  The pixel of the maximum is 1 exactly (e / e, bound 0).  A NaN
    pixel makes the maximum NaN: the whole frame is 0."""
    arg = (c64 + f32(1e-6)) * f32(t)
    e = torch.exp(arg)
    mx = e.max()
    v = torch.nan_to_num(e / mx, nan=0.0, posinf=1.0, neginf=0.0)
    if not bool(torch.isfinite(mx)):
        return v, torch.zeros_like(v)
    bound = v * U * (2 * (arg.abs() + arg.abs().max()) + 5)
    return v, torch.where(e == mx, torch.zeros_like(v), bound)


def temporal_ref(cams64, idx, t):
    """out[i] = the NaN-propagating maximum over the present frames of row i (t = 0: the CAMs
    themselves, exact; t > 0: re-normalised first), 0 for a row with none.  |max a' - max a| <=
    max |a' - a|; where one of the frames is exactly 1 so is the maximum."""
    M, hw = len(idx), cams64.shape[1]
    t = f32(t)
    out = torch.zeros(M, hw, dtype=torch.float64)
    bound = torch.zeros_like(out)
    for i, row in enumerate(idx):
        acc = None
        for f in row:
            if f < 0:
                continue
            if t > 0:
                v, b = renorm_ref(cams64[f], t)
            else:
                v, b = cams64[f], torch.zeros(hw, dtype=torch.float64)
            if acc is None:
                acc, bacc, one = v, b, (v == 1) & (b == 0)
            else:
                acc, bacc = torch.maximum(acc, v), torch.maximum(bacc, b)
                one = one | ((v == 1) & (b == 0))
        if acc is not None:
            out[i] = acc
            bound[i] = torch.where(one | torch.isnan(acc), torch.zeros_like(bacc), bacc)
    return out, bound


# --------------------------------------------------------------------------- top-k
def topk_ref(logits, target):
    """top1 = target == order[0], top5 = target in order[:5], order = torch.sort(descending,
    stable): NaN sorts first, equal values (and NaNs) in index order."""
    order = torch.sort(logits.double(), dim=1, descending=True, stable=True).indices
    t = target.long()[:, None]
    return (order[:, :1] == t).any(1).int(), (order[:, :5] == t).any(1).int()


def topk_cases():
    """name -> (logits, target): the tie cases of test_topk_flags; C = 3 (top-5 always true);
    C = 1000 with B = 300 (two blocks of 256 threads) and targets at 0 and C - 1; NaN logits."""
    g = torch.Generator().manual_seed(5)
    nan = float("nan")
    ties = torch.tensor([[0.1, 0.5, 0.5, 0.2, 0.0, -1.0, 0.3], [1.0] * 7, [1.0] * 7,
                         [0.1, 0.5, 0.5, 0.2, 0.0, -1.0, 0.3]])
    big = torch.randn(300, 1000, generator=g)
    big[:, ::7] = big[:, 1::7][:, :143]                        # ties everywhere
    tb = torch.randint(0, 1000, (300,), generator=g)
    tb[:100:2], tb[1:100:2] = 0, 999
    nans = torch.tensor([[0.3, nan, 2.0, nan, 1.0, 0.5, 0.1, 0.2],     # target a NaN: rank 0
                         [0.3, nan, 2.0, nan, 1.0, 0.5, 0.1, 0.2],     # the second NaN: rank 1
                         [0.3, nan, 2.0, nan, 1.0, 0.5, 0.1, 0.2],     # the largest finite: 2
                         [nan, nan, 2.0, nan, nan, nan, 0.1, 0.2],     # five NaNs first: 5
                         [nan, nan, 2.0, nan, nan, nan, 0.1, 0.2],     # the fifth NaN: 4
                         [nan] * 8])
    return {"ties": (ties, torch.tensor([2, 5, 0, 1])),
            "C3": (torch.randn(9, 3, generator=g), torch.arange(9) % 3),
            "C1000": (big, tb),
            "nan": (nans, torch.tensor([1, 3, 2, 2, 5, 6]))}
