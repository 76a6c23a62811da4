"""fp64 references, elementwise bounds and shared input builders of the training forward's
kernel tests (tests/test_train_fwd_ref.py on the CPU, tests/test_x_train_fwd_gpu.py on the
device): BN statistics and BN-ReLU, the 2-way softmax, channel sums, the TCAM losses and their
gradient, the CRF energy, the classifier head and the nearest-x2 adjoint.

Every reference takes the operands as the device stored them and returns the fp64 result AND
its per-element bound.  Bound rule: n * 2^-24 * (sum of the magnitudes of the terms of that
output), n = the fp32 roundings on the kernel's path (counted next to each bound), plus the
rounding of the output's storage (:func:`storage`).  No bound is taken from a kernel's output.
Plain torch, CPU only."""
import math

import numpy as np
import torch

from oracle.train_ref import r16

U = 2.0 ** -24          # one fp32 rounding, relative


def f32(v):
    """The fp32 value of a scalar the C ABI receives as float, as a Python float."""
    return float(np.float32(v))


def storage(v, lay):
    """Rounding of the output's storage: S3 / plain fp32 none; S2 (fp16 high + fp16 low part)
    2^-22 |v| + 2^-25; S1 or an fp16-rounded fp32 ("r16") 2^-11 |v| + 2^-25."""
    if lay in ("s3", "f32"):
        return torch.zeros_like(v)
    if lay == "s2":
        return 2.0 ** -22 * v.abs() + 2.0 ** -25
    assert lay in ("s1", "r16"), lay
    return 2.0 ** -11 * v.abs() + 2.0 ** -25


def store(x, lay):
    """CPU emulation of an activation layout's storage (fp32 in, fp64 out): what
    ops.s3_to_nchw(ops.s3_from_nchw(x)) gives on the device."""
    x = x.float()
    if lay == "s3":
        return x.double()
    h = x.half()
    if lay == "s1":
        return h.double()
    lo = (x - h.float()).half()
    return h.double() + lo.double()


def ratio(got, ref, bound):
    """max |got - ref| / bound (0 where the error is 0); NaN when a NaN / inf is on one side
    only or the error is not finite."""
    got, ref = got.double(), ref.double()
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    bound = bound.expand_as(ref)
    if got.shape != ref.shape:
        return float("nan")
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def accept(got, ref, bound):
    r = ratio(got, ref, bound)
    return r <= 1.0    # False for NaN


# ------------------------------------------------------------------------------ BN
# (C, (B, H, W)) and the path of bn_plan / bn_stats_co_kernel each reaches (kB = 256 threads,
# G = C / 8 groups, GS groups side by side, NL = 256 / GS pixel lanes, cp pixels per chunk =
# max(ceil(P slices / 1024), 4 NL) rounded up to NL):
BN_SHAPES = [
    (8, (1, 25, 41)),     # GS 1, NL 256, cp 1024, P 1025: two chunks, the last holds one pixel
    (8, (2, 5, 7)),       # GS 1: P 70 < NL, idle lanes, no unrolled pair
    (24, (2, 5, 7)),      # G 3: GS 1 with 3 slices (grid.y = 3)
    (48, (2, 5, 7)),      # G 6: GS 2, NL 128, 3 slices
    (64, (2, 5, 7)),      # G 8: GS 8, NL 32: one pair (p, p + 32) + the tail pixels 64..69
    (320, (2, 5, 7)),     # G 40: GS 8 with 5 slices
    (64, (3, 40, 37)),    # P 4440, cp 128 = 4 NL: 35 chunks of two unrolled pairs, last 88 px
    (512, (3, 40, 37)),   # G 64: GS 32, NL 8, 2 slices, cp 32: 139 chunks, the last 24 px
    (2048, (2, 5, 7)),    # GS 32, NL 8, 8 slices, cp 32: three chunks, the last with 6 pixels
]
BN_EPS = [1e-5, 1e-3]
BN_MOMENTUM = 0.1
CONST_CH, ZERO_GAMMA_CH, DEAD_CH, LIVE_CH = 1, 3, 5, 6


def bn_input(C, B, H, W, seed):
    """y with per-channel std in [0.5, 1.5], every fourth channel at |mean| ~ 1e3 std, one
    constant channel; random running statistics; gamma with negative and one exactly zero
    channel; beta -50 (every pixel masked) and +50 (none masked) on one channel each."""
    g = torch.Generator().manual_seed(seed)
    std = torch.rand(C, generator=g) + 0.5
    mean = torch.randn(C, generator=g)
    sign = torch.where(torch.arange(C) % 8 == 0, 1.0, -1.0)
    mean[::4] = (sign * 1e3 * std)[::4]
    y = torch.randn(B, C, H, W, generator=g) * std[None, :, None, None] + mean[None, :, None, None]
    y[:, CONST_CH] = 0.75
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[2::5] *= -1.0
    gamma[ZERO_GAMMA_CH] = 0.0
    beta = torch.randn(C, generator=g) * 0.3
    beta[DEAD_CH], beta[LIVE_CH] = -50.0, 50.0
    return dict(y=y, gamma=gamma, beta=beta, run_mean=torch.randn(C, generator=g),
                run_var=torch.rand(C, generator=g) + 0.5)


def bn_stats_ref(y64, eps, momentum, run_mean=None, run_var=None):
    """Two-pass fp64 mean m and biased variance of y64 (B, C, H, W), invstd i = (var +
    eps)^-1/2, the running statistics (momentum mu = its fp32 value), and the bounds:
      |mean - m| <= 2^-23 |m| + P 2^-52 mean|y|
      |invstd - i| <= i (2^-23 + P 2^-52 E[y^2] / (var + eps))
    (one fp32 store each with a bit of margin; the second terms are the worst case of the
    kernel's one-pass fp64 sums and of q / P - m^2), hence |var_kernel - var| <= 2 P 2^-52
    E[y^2] (d i / i = -1/2 d var / (var + eps)); running statistics: 2^-23 of the two terms'
    magnitudes (the fp64 blend stored as fp32) plus mu times the propagated bound of m or of
    var P / (P - 1)."""
    P = y64.shape[0] * y64.shape[2] * y64.shape[3]
    eps, mu = f32(eps), f32(momentum)
    m = y64.mean((0, 2, 3))
    var = ((y64 - m[None, :, None, None]) ** 2).mean((0, 2, 3))
    ey2 = (y64 ** 2).mean((0, 2, 3))
    i = 1.0 / torch.sqrt(var + eps)
    sums = P * 2.0 ** -52
    out = dict(P=P, mean=m, var=var, invstd=i,
               b_mean=2.0 ** -23 * m.abs() + sums * y64.abs().mean((0, 2, 3)),
               b_invstd=i * (2.0 ** -23 + sums * ey2 / (var + eps)))
    if run_mean is not None:
        rm, rv = run_mean.double(), run_var.double()
        unb = var * P / (P - 1)
        out["run_mean"] = (1 - mu) * rm + mu * m
        out["run_var"] = (1 - mu) * rv + mu * unb
        out["b_run_mean"] = 2.0 ** -23 * ((1 - mu) * rm.abs() + mu * m.abs()) + \
            mu * sums * y64.abs().mean((0, 2, 3))
        out["b_run_var"] = 2.0 ** -23 * ((1 - mu) * rv.abs() + mu * unb) + \
            mu * 2 * sums * ey2 * P / (P - 1)
    return out


def bn_relu_ref(y64, mean, invstd, gamma, beta, lay):
    """relu(z), z = gamma ((y - mean) invstd) + beta on the fp32 mean / invstd / gamma / beta,
    and 4 2^-24 (|gamma| (|y| + |mean|) invstd + |beta|) + storage: the subtraction, the product
    with invstd and the fma (3 roundings) and one of margin.  ReLU is 1-Lipschitz: no special
    case at 0."""
    v = lambda t: t.double()[None, :, None, None]
    z = v(gamma) * ((y64 - v(mean)) * v(invstd)) + v(beta)
    out = torch.where(z < 0, torch.zeros_like(z), z)      # NaN passes, as torch's relu
    mag = v(gamma).abs() * (y64.abs() + v(mean).abs()) * v(invstd) + v(beta).abs()
    return out, 4 * U * mag + storage(out, lay)


# ------------------------------------------------------- softmax, channel sums, up2 bwd
SOFTMAX_SHAPES = [(1, 1), (3, 4095), (2, 4097)]     # one thread; a partial last block; > 4096
SOFTMAX_GAPS = [0.0, 1e-3, 20.0, 90.0, 120.0]


def softmax_input(B, HW, seed):
    """Logit pairs with equal pairs, a common offset of +-1e4 and the gaps of SOFTMAX_GAPS
    (both signs), random pairs elsewhere."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(B, 2, HW, generator=g) * 3
    j = torch.arange(HW)
    for k, gap in enumerate(SOFTMAX_GAPS):
        sel = j % 16 == k
        f[:, 1, sel] = f[:, 0, sel] + (gap if k % 2 else -gap)
        sel = j % 16 == 5 + k
        f[:, 0, sel] = f[:, 1, sel] + gap
    f[:, :, j % 16 == 11] += 1e4
    f[:, :, j % 16 == 12] -= 1e4
    if HW == 1:
        f[0, 0, 0], f[0, 1, 0] = 0.3, -0.8
    return f


def softmax2_ref(f64):
    """softmax over dim 1 of (B, 2, HW) and (4 + |f0 - f1|) 2^-24 S + 2^-126: expf within one
    ulp (2 roundings), the sum and the division, and |f0 - f1| 2^-24 for the rounding of the
    subtraction before expf; the floor allows a flushed denormal."""
    S = torch.softmax(f64, 1)
    gap = (f64[:, :1] - f64[:, 1:]).abs()
    return S, (4 + gap) * U * S + 2.0 ** -126


CHANSUM_SHAPES = [(2, 2, 4095), (3, 2, 16385), (1, 65, 7), (257, 2, 5)]   # chunk 16384; C > 64


def chansum_input(B, C, HW, seed):
    """Mixed signs, several magnitudes, every channel summing to about zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, HW, generator=g) * 10.0 ** torch.randint(-2, 3, (B, C, HW), generator=g)
    x -= x.mean((0, 2), keepdim=True)
    return x


def chansum_ref(x64):
    """sum over (b, hw) of (B, C, HW); 2^-24 |sum| (the fp32 store) + 2^-40 sum |x| (the fp64
    partial sums, with a wide margin)."""
    s = x64.sum((0, 2))
    return s, U * s.abs() + 2.0 ** -40 * x64.abs().sum((0, 2))


UP2_SHAPES = [(1, 8, 1, 1), (2, 24, 5, 7), (2, 64, 14, 14)]


def up2_bwd_ref(gu64, lay):
    """Adjoint of nearest x2: the sum of each 2x2 block of (B, C, 2H, 2W); three fp32 additions
    (the first lands on 0): 3 2^-24 sum |terms| + storage."""
    B, C, H2, W2 = gu64.shape
    blk = gu64.view(B, C, H2 // 2, 2, W2 // 2, 2)
    s = blk.sum((3, 5))
    return s, 3 * U * blk.abs().sum((3, 5)) + storage(s, lay)


# ----------------------------------------------------------------------- TCAM losses
# kLossPix = 4096 pixels per chunk, kFinBlock = 256 frames per pass of loss_finalize_kernel
LOSS_SHAPES = [(1, 1), (2, 16), (3, 4095), (2, 4097), (257, 5), (2, 50176)]
LOSS_T = [1.0, 2.5, 10.0]
LAM_ALL = (0.7, 0.3, 0.2)
LAM_DEFAULT = (1.0, 2e-9, 0.01)
IGNORE = -255


def loss_seed(B, HW):
    return 7 * B + HW


def loss_input(B, HW, seed):
    """fcams whose class-1 plane sum is far below 1/t^2 in the odd frames (f0 - f1 ~ 25) and
    not in the even ones; seeds of 0 / 1 / -255 with frame 0 all valid and, for B >= 2, the
    last frame all ignored; a synthetic AS over several magnitudes; gx / extra of a fifth
    term."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(B, 2, HW, generator=g) * 2
    f[1::2, 0] += 25.0
    seeds = torch.randint(-1, 2, (B, HW), generator=g).int()
    seeds[seeds < 0] = IGNORE
    seeds[0] = torch.randint(0, 2, (HW,), generator=g).int()
    if B >= 2:
        seeds[B - 1] = IGNORE
    AS = torch.randn(B, 2, HW, generator=g) * 10.0 ** torch.randint(-3, 4, (B, 2, HW), generator=g)
    gx = torch.randn(B, 2, HW, generator=g) * 0.1
    extra = torch.tensor([0.37 + 0.01 * seed])
    return dict(f=f, seeds=seeds, AS=AS, gx=gx, extra=extra)


def loss_runs(c):
    """(name, seeds, AS, gx, extra, lam) of the runs on one input: each term alone, all three
    with lambdas of one order (no term hides under another), the defaults, and the five-term
    entry."""
    return [("sl", c["seeds"], None, None, None, (1.0, 0.0, 0.0)),
            ("crf", None, c["AS"], None, None, (0.0, 0.3, 0.0)),
            ("size", None, None, None, None, (0.0, 0.0, 0.2)),
            ("all", c["seeds"], c["AS"], None, None, LAM_ALL),
            ("default", c["seeds"], c["AS"], None, None, LAM_DEFAULT),
            ("ex", c["seeds"], c["AS"], c["gx"], c["extra"], LAM_ALL)]


def _elb_terms(bl, t):
    """ELB (oracle/train_ref._elb, elementwise) of fx = -bl per plane, d ELB / d fx, the branch
    taken (True: log) and the fp32 error bounds of value and derivative.
    log branch l = -(1/t) log(bl): bl cast to fp32 (2^-24 absolute in the log), 1/t, logf within
    an ulp (2), the product: 2^-24 / t + 4 2^-24 |log bl| / t; dl = (1/t) / bl: 1/t, the cast,
    the division: 3 2^-24.  linear branch l = t fx - (1/t) log(1/t^2) + 1/t: the cast, three
    products, t t, two divisions, logf (2 absolute in its argument's two roundings + 2 relative),
    two additions: 8 2^-24 (t bl + |log(1/t^2)| / t + 1/t) + 2 2^-24 / t; dl = t exact."""
    ct = 1.0 / (t * t)
    is_log = bl >= ct                      # fx = -bl <= -1/t^2
    safe = bl.clamp(min=ct)
    l_log = -(1.0 / t) * torch.log(safe)
    l_lin = -t * bl - (1.0 / t) * math.log(ct) + 1.0 / t
    l = torch.where(is_log, l_log, l_lin)
    dl = torch.where(is_log, (1.0 / t) / safe, torch.full_like(bl, t))     # d l / d fx
    b_log = U / t + 4 * U * l_log.abs()
    b_lin = 8 * U * (t * bl + abs(math.log(ct)) / t + 1.0 / t) + 2 * U / t
    return l, dl, is_log, torch.where(is_log, b_log, b_lin), \
        torch.where(is_log, 3 * U * dl, torch.zeros_like(dl))


def tcam_loss_ref(f, S, seeds, AS, gx, extra, lam, t):
    """The TCAM loss terms and d total / d fcams of tcam_tcam_losses(_ex) in fp64 on fcams f
    (B, 2, HW), the softmax S the device stored, seeds (0 / 1 / -255, or None), AS (or None),
    the fifth term's gx / extra (or None); lam = (sl, crf, size), ELB's t.

      sl   = lam0 mean over valid seeds of CE(f, seed)          (NaN without a valid seed)
      crf  = lam1 -sum(S AS) / B, gradient -2 lam1 AS / B w.r.t. S (the doubled surrogate)
      size = lam2 / 2 sum_c mean_b ELB_t(-sum_hw S[b, c])
      gS_c = size'[b, c] - 2 lam1 AS_c / B + gx_c
      df_c = S_c (gS_c - sum_j S_j gS_j) + lam0 / n_valid (S_c - [seed == c])

    Returns losses (5: total, sl, crf, size, extra), their bounds, dF and its bound, and per
    (b, c) plane the ELB branch taken (True = log) and the relative distance of the plane sum
    from the breakpoint 1/t^2."""
    f, S = f.double(), S.double()
    B, _, HW = f.shape
    l0, l1, l2 = (f32(v) for v in lam)
    t = f32(t)
    use_sl, use_crf, use_size = seeds is not None, AS is not None, l2 != 0.0
    zero = torch.zeros((), dtype=torch.float64)
    # --- size: plane sums in fp64 on the device (no fp32 rounding before the cast)
    bl = S.sum(2)
    l, dl, is_log, b_l, b_dl = _elb_terms(bl, t)
    dist = (bl - 1 / t ** 2).abs() * t ** 2
    size = l2 * 0.5 * l.sum() / B if use_size else zero
    b_size = (l2 * 0.5 * b_l.sum() / B + U * size.abs()) if use_size else zero   # + the store
    # d size / d S[b, c] = -lam2 / 2 dl / B: dl's roundings, the two products, the division
    cs = -l2 * 0.5 * dl / B if use_size else torch.zeros_like(dl)
    b_cs = (b_dl / dl + 3 * U) * cs.abs()
    # --- CE: per valid pixel lse - f[seed] in fp32: the subtraction before expf and expf
    # ((|d| + 2) e / (1 + e) <= 1.4), 1 + e, logf (2 relative, log <= 0.7), m + log, the last
    # subtraction: below 6 2^-24 (1 + |f0| + |f1|); summed in fp64, one store
    sl, b_sl, c0 = zero, zero, 0.0
    valid = None
    if use_sl:
        valid = (seeds == 0) | (seeds == 1)
        nv = int(valid.sum())
        if nv > 0:
            lse = torch.logsumexp(f, 1)
            pick = torch.where(seeds == 1, f[:, 1], f[:, 0])
            sl = l0 * ((lse - pick) * valid).sum() / nv
            b_sl = l0 * (6 * U * (1 + f.abs().sum(1)) * valid).sum() / nv + U * sl.abs()
            c0 = l0 / nv
        elif l0 != 0.0:
            sl = b_sl = torch.tensor(float("nan"), dtype=torch.float64)
    # --- CRF value: fp64 products and sums, one store
    crf, b_crf, c1 = zero, zero, 0.0
    if use_crf:
        AS = AS.double()
        crf = l1 * -(S * AS).sum() / B
        b_crf = U * crf.abs() + 2.0 ** -50 * l1 * (S * AS).abs().sum() / B
        c1 = -2.0 * l1 / B
    ex = extra.double().reshape(()) if extra is not None else zero
    total = sl + crf + size + ex
    # the components' bounds + the three fp32 additions of the total
    b_total = b_sl + b_crf + b_size + 3 * U * (sl.abs() + crf.abs() + size.abs() + ex.abs())
    losses = torch.stack([total, sl, crf, size, ex])
    bounds = torch.stack([b_total, b_sl, b_crf, b_size, zero])
    # --- gradient
    gS = cs[:, :, None].expand(B, 2, HW).clone()
    mag = cs.abs()[:, :, None].expand(B, 2, HW).clone()
    if use_crf:
        gS += c1 * AS
        mag += (c1 * AS).abs()
    if gx is not None:
        gS += gx.double()
        mag += gx.double().abs()
    # cs's own roundings; coef1 (one division), its product with AS, the two additions: 4
    eg = b_cs[:, :, None] + 4 * U * mag
    dot = (S * gS).sum(1, keepdim=True)
    dot_mag = (S * gS.abs()).sum(1, keepdim=True)
    e_dot = (S * eg).sum(1, keepdim=True) + 3 * U * dot_mag      # two products, one addition
    dF = S * (gS - dot)
    # g - dot, its product with S, the final addition: 3 2^-24 S (|g| + sum S |g|)
    b_dF = S * (eg + e_dot) + 3 * U * S * (gS.abs() + dot_mag)
    if use_sl and c0 != 0.0:
        onehot = torch.stack([(seeds == 0), (seeds == 1)], 1).double()
        term = c0 * (S - onehot) * valid[:, None].double()
        dF = dF + term
        b_dF = b_dF + 4 * U * term.abs()      # coef0's store, S - 1, the product, the addition
    return dict(losses=losses, bounds=bounds, dF=dF, b_dF=b_dF, is_log=is_log, dist=dist)


# ------------------------------------------------------------------------ CRF energy
CRF_SHAPES = [(1, 1, 1, 1), (2, 2, 9, 7), (2, 2, 363, 361)]   # n = 524164 > 262144: 2 terms/thread


def crf_input(N, K, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    seg = torch.rand(N, K, H, W, generator=g)
    AS = torch.randn(N, K, H, W, generator=g) * 10.0 ** torch.randint(-2, 3, (N, K, H, W), generator=g)
    return seg, AS


def crf_energy_ref(seg64, as64, N):
    """-sum(seg AS) / N; an fp32 tree: T = ceil(n / 262144) product-sums per thread (2 T), the
    wave (6) and block (4) levels, the same over the 1024 partials (4 + 6 + 4), -1/N and its
    product (2): (2 T + 26) 2^-24 sum |seg AS| / N."""
    n = seg64.numel()
    T = -(-n // 262144)
    e = -(seg64 * as64).sum() / N
    return e, (2 * T + 26) * U * (seg64 * as64).abs().sum() / N


def crf_grad_ref(as64, gout, N):
    """-2 g AS / N: -2/N, its product with g, the product with AS: 3 2^-24 |grad|."""
    g = -2.0 * float(gout) * as64 / N
    return g, 3 * U * g.abs()


# -------------------------------------------------------------------- classifier head
# An fp16 output is compared with the UNROUNDED fp64 value under the storage bound (a rounded
# reference would charge a full fp16 ulp wherever the two sides round apart); the fp16 points
# of the operands are the device's own previous stage, or r16 of the fp32 parameters.
# kPoolSlices = 32 pixel slices of ceil(HW / 32); fc: a wave per logit, 64 lanes; tcam_cls_bwd
# refuses K > 256; ce_loss_kernel strides B over 256 threads.
HEAD_SHAPES = [
    (1, 8, 1, 1),          # one pixel: 31 empty slices; K 1: p = 1, dz = 0
    (6, 24, 31, 10),       # HW < 32: one pixel per slice, one slice empty; C < 64: idle lanes
    (3, 1024, 784, 10),    # VGG16: 25 pixels per slice, the last slice 9
    (6, 2048, 49, 200),    # ResNet50 at 224: 2 pixels per slice, slices 25.. empty
    (257, 8, 4, 3),        # B > 256: the strided frame loop of ce_loss_kernel
    (2, 64, 33, 256),      # K = 256, the largest tcam_cls_bwd takes; HW 33: 2 per slice, 17 used
]
HEAD_SPREAD = (6, 24, 31, 10)        # this shape also runs with logits spread over +-1e4
HEAD_LAM = [1.0, 0.3]
HEAD_GSCALE = {"f16x3": 2.0 ** 12, "amp": 2.0 ** 16}


def head_gscales(fmt, spread):
    """gscale NULL and the format's loss scale; the spread logits run AMP unscaled only (with
    weights of ~5e3, 2^16 dz w leaves the fp16 range: the case the GradScaler backs off from)."""
    return (None,) if (spread and fmt == "amp") else (None, HEAD_GSCALE[fmt])


def head_input(B, C, HW, K, seed, spread=False):
    """Post-ReLU features (B, C, HW, 1), fc weight / bias, labels."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, HW, 1, generator=g).abs() * 0.5
    w = torch.randn(K, C, generator=g) * (1e4 / (0.4 * C ** 0.5) if spread else 0.02)
    b = torch.randn(K, generator=g) * 0.1
    y = torch.randint(0, K, (B,), generator=g).int()
    return dict(x=x, w=w, b=b, y=y)


def _q(amp):
    return (lambda v: r16(v.double())) if amp else (lambda v: v.double())


def pool_ref(x64, amp):
    """pooled = mean over the pixels of (B, C, H, W): ceil(HW / 32) terms in order, the 32
    slices in order, the division: (ceil(HW / 32) + 32) 2^-24 sum |x| / HW (+ fp16 on AMP)."""
    HW = x64.shape[2] * x64.shape[3]
    n = -(-HW // 32) + 32
    p = x64.sum((2, 3)) / HW
    return p, n * U * x64.abs().sum((2, 3)) / HW + (storage(p, "r16") if amp else 0)


def fc_ref(pooled64, w, b, amp):
    """logits = pooled w^T + bias (AMP: the fp16 copies of w and bias, fp16 logits): ceil(C /
    64) products and additions per lane, 6 wave levels, the bias: (2 ceil(C / 64) + 7) 2^-24
    (sum |pooled w| + |bias|)."""
    q = _q(amp)
    wq, bq = q(w), q(b)
    C = w.shape[1]
    n = 2 * -(-C // 64) + 7
    z = pooled64 @ wq.t() + bq
    mag = pooled64.abs() @ wq.abs().t() + bq.abs()
    return z, n * U * mag + (storage(z, "r16") if amp else 0)


def ce_ref(z64, y, lam, gscale):
    """loss = lam mean_b (logsumexp z_b - z_b[y_b]) and dz = lam gscale (softmax(z) - onehot) /
    B (the target's entry as -sum of the others: no cancellation in the reference).  The kernel
    works in fp64: both within 2^-23 relative + 2^-149.  A label outside [0, K) gives a NaN
    loss (dz is then not compared)."""
    B, K = z64.shape
    lam, gs = f32(lam), (1.0 if gscale is None else f32(gscale))
    y = y.long()
    if bool(((y < 0) | (y >= K)).any()):
        nan = torch.tensor(float("nan"), dtype=torch.float64)
        return nan, nan, None, None
    lse = torch.logsumexp(z64, 1)
    loss = lam * (lse - z64.gather(1, y[:, None])[:, 0]).mean()
    p = torch.exp(z64 - lse[:, None])
    onehot = torch.zeros_like(p).scatter_(1, y[:, None], 1.0)
    others = (p * (1 - onehot)).sum(1, keepdim=True)
    dz = torch.where(onehot > 0, -others, p) * lam * gs / B
    return loss, 2.0 ** -23 * loss.abs() + 2.0 ** -149, dz, 2.0 ** -23 * dz.abs() + 2.0 ** -149


def cls_bwd_ref(dz64, pooled64, w, amp):
    """dW[k][c] = sum_b dz pooled (B products and additions: 2 B), db[k] = sum_b dz (B),
    dpooled[b][c] = sum_k dz w (2 K); AMP: dz rounded to fp16 as it enters, the fp16 copy of w,
    every result fp16."""
    q = _q(amp)
    B, K = dz64.shape
    dz, wq = q(dz64), q(w)
    st = (lambda v: storage(v, "r16")) if amp else (lambda v: 0)
    dw = dz.t() @ pooled64
    db = dz.sum(0)
    dp = dz @ wq
    return (dw, 2 * B * U * (dz.abs().t() @ pooled64.abs()) + st(dw),
            db, B * U * dz.abs().sum(0) + st(db),
            dp, 2 * K * U * (dz.abs() @ wq.abs()) + st(dp))


def pool_bwd_ref(dp64, HW, lay):
    """dout[b][c][p] = dpooled[b][c] / HW as 1/HW and a product: 2 2^-24 + storage."""
    v = dp64 / HW
    return v, 2 * U * v.abs() + storage(v, lay)
