"""fp64 reference, bounds, launch-plan restatements and the case table of the conv weight
gradients' kernel tests (tests/test_wgrad_ref.py on the CPU, tests/test_x_wgrad_plans_gpu.py
on the device): csrc/train.hip's wgrad33x6_kernel / wgrad33_kernel (3x3, stride 1, pad 1), the
generic wgrad_kernel and their split reductions, and csrc/enc_train.hip's wgrad11_kernel.

The planners make_w33 / make_wg / make_w11 choose, from the shape alone, how many patches or
pixels a block loops over, how many splits there are, how long the last one is and whether the
reduction runs in one pass or two.  w33_plan / wg_plan / w11_plan restate them in Python (tied
to the C++ through the workspace sizes, tests/test_wgrad_ref.py), so that every case below can
assert the plan it was chosen for: editing a planner constant then fails a case's assertion
instead of quietly moving it onto another path.

The reference takes the operands as the device stored them and returns the fp64 sum and the
same sum on absolute values; the bounds are elementwise on that magnitude sum and are the ones
the project's tests already hold these kernels to at one patch per block.  No bound is taken
from a kernel's output.  Plain torch, CPU only."""
import torch
import torch.nn.functional as F

from train_fwd_ref import accept, ratio   # noqa: F401  (re-exported: the shared checkers)

# ------------------------------------------------------------------ planner restatements
K_PR, K_PC = 2, 32      # make_w33: a patch is 2 rows x 32 columns
K_BLOCKS33 = 1536       # make_w33: blocks aimed at
K_RED_CHUNK = 16        # reduce33: splits per pass-1 chunk; one pass up to this many splits
K_WT, K_WK = 64, 16     # make_wg: tile edge, pixels per K-step
K_BLOCKS_G = 2048       # make_wg: blocks aimed at
K_KSTEPS_G = 64         # make_wg: K-steps per split at least
K_KP = 32               # make_w11: pixels per chunk
K_BLOCKS11 = 1024       # make_w11: blocks aimed at


def _cdiv(a, b):
    return -(-a // b)


def _up256(n):
    return _cdiv(n, 256) * 256


def w33_plan(B, Cout, srcs, H, W):
    """make_w33 for sources ``srcs`` = [(C, h, w, up2), ...] and a (B, Cout, H, W) dy: None when
    the geometry is not the 3x3 fast path's, else the fields wgrad33x6_kernel / wgrad33_kernel
    and reduce33 branch on —
      msub      32-row M subtiles per block (1: Cout <= 32);  ntiles = ntm * ncb blocks per split
      npatch    patches of the batch;  ppb patches per split (a block's patch loop)
      splits    partial slabs;  last = patches of the last split (ppb when it is full)
      nchunk    chunk sums of the two-pass reduction (0: one pass), last_chunk = splits in the
                last chunk
      ws_bytes  w33_ws_bytes: the slabs, the dy channel maxima and scales with the scaled S2
                copy of dy, the chunk sums."""
    if not 1 <= len(srcs) <= 2 or B <= 0 or Cout <= 0 or Cout % 8:
        return None
    for (C, h, w, up2) in srcs:
        if C <= 0 or C % 8 or ((2 * h, 2 * w) if up2 else (h, w)) != (H, W):
            return None
    if len(srcs) == 2 and srcs[0][0] % 32:
        return None
    ctot = sum(s[0] for s in srcs)
    prow, pcol = _cdiv(H, K_PR), _cdiv(W, K_PC)
    npatch = B * prow * pcol
    msub = 1 if Cout <= 32 else 2
    MT = 32 * msub
    ntm, ncb = _cdiv(Cout, MT), _cdiv(ctot, 32)
    ntiles = ntm * ncb
    slab = ntiles * MT * 288 * 4
    s = max(1, min(_cdiv(K_BLOCKS33, ntiles), npatch, (256 << 20) // slab))
    ppb = _cdiv(npatch, s)
    splits = _cdiv(npatch, ppb)
    nchunk = _cdiv(splits, K_RED_CHUNK) if splits > K_RED_CHUNK else 0
    chunk_off = _up256(_up256(splits * slab) + Cout * 2 * 4 + B * H * W * Cout * 4)
    return dict(msub=msub, ntm=ntm, ncb=ncb, ntiles=ntiles, prow=prow, pcol=pcol, npatch=npatch,
                ppb=ppb, splits=splits, last=npatch - (splits - 1) * ppb, nchunk=nchunk,
                last_chunk=splits - (nchunk - 1) * K_RED_CHUNK if nchunk else splits,
                ws_bytes=chunk_off + nchunk * slab)


def w33_split_pixels(plan, B, H, W):
    """Per split, the flat pixel indices (b H W + y W + x) its patches cover, in the kernel's
    patch order (frame, patch row, patch column)."""
    per_frame = plan["prow"] * plan["pcol"]
    out = []
    for k in range(plan["splits"]):
        idx = []
        for q in range(k * plan["ppb"], min(plan["npatch"], (k + 1) * plan["ppb"])):
            b, r = divmod(q, per_frame)
            y0, x0 = (r // plan["pcol"]) * K_PR, (r % plan["pcol"]) * K_PC
            ys = torch.arange(y0, min(H, y0 + K_PR))
            xs = torch.arange(x0, min(W, x0 + K_PC))
            idx.append(((b * H + ys)[:, None] * W + xs[None, :]).flatten())
        out.append(torch.cat(idx))
    return out


def wg_plan(B, Cout, Ctot, Hout, Wout, KH, KW):
    """make_wg (the generic wgrad_kernel: one 64 x 64 tile of one tap per block, 16 pixels per
    K-step): P pixels, ``chunk`` pixels per split (a multiple of 16), ``splits``, ``last`` =
    pixels of the last split, ``tail`` = pixels of its last K-step (0: the step is full), and
    the workspace of the partial tiles."""
    if B <= 0 or Cout <= 0 or Cout % 8 or Ctot <= 0 or Ctot % 8:
        return None
    if not (1 <= KH <= 7 and 1 <= KW <= 7):
        return None
    P = B * Hout * Wout
    ntm, nct = _cdiv(Cout, K_WT), _cdiv(Ctot, K_WT)
    ntiles = ntm * nct * KH * KW
    s = max(1, min(_cdiv(K_BLOCKS_G, ntiles), _cdiv(P, K_KSTEPS_G * K_WK)))
    chunk = _cdiv(_cdiv(P, s), K_WK) * K_WK
    splits = _cdiv(P, chunk)
    last = P - (splits - 1) * chunk
    return dict(P=P, ntm=ntm, nct=nct, ntiles=ntiles, chunk=chunk, splits=splits, last=last,
                tail=last % K_WK, ws_bytes=splits * ntiles * K_WT * K_WT * 4)


def wg_split_pixels(plan):
    return [torch.arange(k * plan["chunk"], min(plan["P"], (k + 1) * plan["chunk"]))
            for k in range(plan["splits"])]


def conv_wgrad_ws_bytes(B, Cout, srcs, Hout, Wout, KH, KW):
    """tcam_conv_wgrad_ws_bytes: the 3x3 fast path's workspace when make_w33 takes the geometry
    (every source at stride 1 and at the output size), else the generic one."""
    if KH == 3 and KW == 3:
        p = w33_plan(B, Cout, srcs, Hout, Wout)
        if p:
            return p["ws_bytes"]
    p = wg_plan(B, Cout, sum(s[0] for s in srcs), Hout, Wout, KH, KW)
    return p["ws_bytes"] if p else 0


def w11_plan(B, Cin, Hin, Win, stride, Cout, Ho, Wo):
    """make_w11 (wgrad11_kernel<F, wm, wn>: a 64 wm x 64 wn tile per block, 32 pixels per
    chunk): ``nchunk`` pixel chunks, ``cps`` chunks per split, ``splits``, ``last`` = chunks of
    the last split, ``tail`` = pixels of the last chunk (0: full), the workspace."""
    if B <= 0 or Cin <= 0 or Cin % 8 or Cout <= 0 or Cout % 8 or stride < 1:
        return None
    if Ho <= 0 or Wo <= 0 or (Ho - 1) * stride >= Hin or (Wo - 1) * stride >= Win:
        return None
    P = B * Ho * Wo
    nchunk = _cdiv(P, K_KP)
    wm, wn = (2 if Cout > 64 else 1), (2 if Cin > 64 else 1)
    MT, NT = 64 * wm, 64 * wn
    ntm, ntn = _cdiv(Cout, MT), _cdiv(Cin, NT)
    ntiles = ntm * ntn
    s = max(1, min(_cdiv(K_BLOCKS11, ntiles), 64, nchunk // 8))
    cps = _cdiv(nchunk, s)
    splits = _cdiv(nchunk, cps)
    return dict(P=P, wm=wm, wn=wn, ntm=ntm, ntn=ntn, ntiles=ntiles, nchunk=nchunk, cps=cps,
                splits=splits, last=nchunk - (splits - 1) * cps, tail=P % K_KP,
                ws_bytes=splits * ntiles * MT * NT * 4 + 256)


def w11_split_pixels(plan):
    n = plan["cps"] * K_KP
    return [torch.arange(k * n, min(plan["P"], (k + 1) * n)) for k in range(plan["splits"])]


# ------------------------------------------------------------------ reference and bounds
def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def cat_sources(xs64):
    """[(x, up2), ...] -> the conv's input: the sources concatenated over channels, nearest x2
    where up2 is set."""
    return torch.cat([F.interpolate(x, scale_factor=2, mode="nearest") if up2 else x
                      for x, up2 in xs64], 1)


def tap_rows(x64, dy_shape, k, stride, pad):
    """For each tap (kh, kw) in PyTorch's weight order, the (P, C) matrix of the input pixels
    that tap multiplies with the (P, Cout) rows of dy (P = B Ho Wo, zero outside the image)."""
    (KH, KW), (ph, pw) = _pair(k), _pair(pad)
    B, _, Ho, Wo = dy_shape
    C = x64.shape[1]
    # enough zero rows / columns below and right for the last tap of the last output pixel
    need_h, need_w = (Ho - 1) * stride + KH, (Wo - 1) * stride + KW
    xp = F.pad(x64, (pw, max(0, need_w - pw - x64.shape[3]), ph,
                     max(0, need_h - ph - x64.shape[2])))
    for kh in range(KH):
        for kw in range(KW):
            v = xp[:, :, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride]
            yield v.permute(0, 2, 3, 1).reshape(B * Ho * Wo, C)


def dy_rows(dy64):
    return dy64.permute(0, 2, 3, 1).reshape(-1, dy64.shape[1])


def wgrad_ref(xs64, dy64, k, stride, pad):
    """fp64 dW[co][c][kh][kw] = sum_p dy[p][co] x[tap(p, kh, kw)][c] of y = conv2d(x, W, stride,
    pad) over x = cat_sources(xs64), and ``mag``, the same sum on absolute values."""
    x = cat_sources(xs64)
    KH, KW = _pair(k)
    d = dy_rows(dy64)
    dt, da = d.t().contiguous(), d.abs().t().contiguous()
    ref, mag = [], []
    for xt in tap_rows(x, dy64.shape, k, stride, pad):
        ref.append(dt @ xt)
        mag.append(da @ xt.abs())
    shape = (dy64.shape[1], x.shape[1], KH, KW)
    return torch.stack(ref, 2).view(shape), torch.stack(mag, 2).view(shape)


def bound_f32(mag):
    """f16x3, x6, fp32-MFMA and the generic kernel (fp32 sums of products kept to ~2^-22):
    1e-6 of the magnitude sum, as tests/test_grad_chain_gpu.py and test_wgrad11_f16x3_matches_fp64
    hold them."""
    return 1e-6 * mag


def bound_s1(ref, mag):
    """The AMP (S1) gradients: exact fp16 products, fp32 sums, dW rounded to fp16
    (tests/test_gpu_amp.py)."""
    return 2.0 ** -11 * ref.abs() + 2e-6 * (mag + 1e-3)


def is_fp16(v):
    return torch.equal(v.double(), v.half().double())


# ------------------------------------------------------------------ inputs
ZERO_DY_CH, ZERO_X_CH = 2, 5


def wgrad_inputs(B, Cout, src_shapes, dy_hw, dmag, seed):
    """fp32 sources [(B, C, h, w), ...] ~ N(0, 1) with one all-zero channel (ZERO_X_CH of source
    0), and a (B, Cout, Ho, Wo) dy ~ N(0, 1) dmag logspace(-2, 2, Cout)[co] with channel
    ZERO_DY_CH all zero (Cout > ZERO_DY_CH + 1)."""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, C, h, w, generator=g) for (C, h, w) in src_shapes]
    if xs[0].shape[1] > ZERO_X_CH:   # (the stem's image has its zero channels from the padding)
        xs[0][:, ZERO_X_CH] = 0.0
    dy =torch.randn(B, Cout, *dy_hw, generator=g) * dmag * \
        torch.logspace(-2, 2, Cout)[None, :, None, None]
    dy[:, ZERO_DY_CH] = 0.0
    return xs, dy


# ------------------------------------------------------------------ the case table
# 3x3 / stride 1 / pad 1.  srcs: (C, h, w, up2) per source; ``plan``: the fields of w33_plan
# the case was chosen for (asserted by w33_case_plan).  ntiles = ceil(Cout / 32 msub) *
# ceil(Ctot / 32), s = min(ceil(1536 / ntiles), npatch), ppb = ceil(npatch / s).
W33_CASES = {
    # msub 2, 48 tiles, s 32 of 35 patches: a block loops over 2 patches, the 18th split holds
    # one; 18 splits > 16: chunk sums of 16 + 2 splits; source 0 read at half resolution
    "up2_skip_two_pass": dict(B=5, cout=64, srcs=[(1024, 7, 10, 1), (512, 14, 20, 0)],
                              plan=dict(msub=2, npatch=35, ppb=2, splits=18, last=1, nchunk=2,
                                        last_chunk=2)),
    # 128 tiles, s 12 of 70 patches (W 40: a patch column of 8): ppb 6, the last split 4
    "ppb6_one_pass": dict(B=5, cout=256, srcs=[(1024, 13, 40, 0)],
                          plan=dict(msub=2, npatch=70, ppb=6, splits=12, last=4, nchunk=0)),
    # msub 1 (Cout <= 32), 32 tiles, s 48 of 65 patches: ppb 2, 33 splits = 16 + 16 + 1
    "thin8_33_splits": dict(B=5, cout=8, srcs=[(1024, 25, 20, 0)],
                            plan=dict(msub=1, npatch=65, ppb=2, splits=33, last=1, nchunk=3,
                                      last_chunk=1)),
    # the same with 52 patches: 26 splits of exactly 2 (a full last split behind a patch loop)
    "thin8_exact_last": dict(B=4, cout=8, srcs=[(1024, 25, 20, 0)],
                             plan=dict(msub=1, npatch=52, ppb=2, splits=26, last=2, nchunk=2,
                                       last_chunk=10)),
    "thin32_33_splits": dict(B=5, cout=32, srcs=[(1024, 25, 20, 0)],
                             plan=dict(msub=1, npatch=65, ppb=2, splits=33, last=1, nchunk=3,
                                       last_chunk=1)),
    # both sides of kRedChunk: 16 splits reduce in one pass, 17 through chunk sums of 16 + 1
    "splits_16": dict(B=1, cout=64, srcs=[(64, 32, 20, 0)],
                      plan=dict(msub=2, npatch=16, ppb=1, splits=16, last=1, nchunk=0)),
    "splits_17": dict(B=1, cout=64, srcs=[(64, 34, 20, 0)],
                      plan=dict(msub=2, npatch=17, ppb=1, splits=17, last=1, nchunk=2,
                                last_chunk=1)),
    # the seg head's form: 8 dy channels computed, 2 stored
    "seg_head_store2": dict(B=2, cout=8, srcs=[(16, 9, 40, 0)], cout_store=2,
                            plan=dict(msub=1, npatch=20, ppb=1, splits=20, last=1, nchunk=2,
                                      last_chunk=4)),
    # Cout 40: the M tile's rows 40..63 are padding; channel block 1 = 8 channels of source 1
    # and 24 of padding; W 33: the second patch column holds one pixel column
    "ragged_40_32p8": dict(B=3, cout=40, srcs=[(32, 7, 33, 0), (8, 7, 33, 0)],
                           plan=dict(msub=2, npatch=24, ppb=1, splits=24, last=1, nchunk=2,
                                     last_chunk=8)),
}

# The generic path.  (B, cin, cpad, cout, H, W, (KH, KW), stride, (pad_h, pad_w)); s =
# min(ceil(2048 / ntiles), ceil(P / 1024)), chunk = ceil(P / s) rounded up to 16.
WG_CASES = {
    # the stem's form: the 3-channel image padded to 8 channels, 7x7 / 2, 49 tiles
    "stem_7x7s2": dict(B=3, cin=3, cpad=8, cout=64, H=65, W=69, k=(7, 7), stride=2, pad=(3, 3),
                       plan=dict(P=3465, splits=4, chunk=880, last=825, tail=9)),
    "conv_3x3s2": dict(B=3, cin=32, cpad=32, cout=48, H=57, W=61, k=(3, 3), stride=2, pad=(1, 1),
                       plan=dict(P=2697, splits=3, chunk=912, last=873, tail=9)),
    # rectangular taps (the Inception 1x7 form)
    "conv_1x7": dict(B=2, cin=24, cpad=24, cout=16, H=41, W=43, k=(1, 7), stride=1, pad=(0, 3),
                     plan=dict(P=3526, splits=4, chunk=896, last=838, tail=6)),
}

# wgrad11: (B, cin, cout, H, W, stride) as tests/test_gpu_enc_train.py lists them.  P = 969:
# 31 chunks of 32 pixels, 3 splits of 11 / 11 / 9 chunks, the last chunk holds 9 pixels.  With
# Cout > 64 wm = 2 and with Cin > 64 wn = 2, so (72, 136) runs the <2, 2> variant on ragged
# tiles; (40, 136) and (136, 40) reach <2, 1> and <1, 2>.
W11_NEW = dict(nchunk=31, cps=11, splits=3, last=9, tail=9)
W11_CASES = [
    ((3, 64, 64, 19, 17, 1), dict(wm=1, wn=1, **W11_NEW)),
    ((3, 72, 136, 19, 17, 1), dict(wm=2, wn=2, ntm=2, ntn=1, **W11_NEW)),
    ((3, 40, 136, 19, 17, 1), dict(wm=2, wn=1, ntm=2, ntn=1, **W11_NEW)),
    ((3, 136, 40, 19, 17, 1), dict(wm=1, wn=2, ntm=1, ntn=2, **W11_NEW)),
]
# the cases the suite had before: the only one with several splits has a full last chunk
W11_OLD = [(2, 64, 256, 14, 14, 1), (2, 256, 64, 14, 14, 1), (3, 256, 512, 16, 16, 2),
           (1, 1024, 2048, 7, 7, 1), (2, 8, 8, 5, 7, 1), (2, 72, 136, 9, 11, 1),
           (2, 64, 64, 9, 9, 2), (4, 512, 128, 28, 28, 1)]

# 3x3 geometries of the direct tests the suite had before (B, cout, srcs): every one has ppb 1
# (their (3, 32, [(16, 5, 6, 1), (8, 10, 12, 0)]) is not the fast path's: source 0 does not end
# on a 32-channel block)
W33_OLD = [(3, 40, [(24, 9, 11, 0)]), (3, 16, [(32, 7, 20, 1), (16, 14, 40, 0)]), (3, 72, [(64, 9, 9, 1), (32, 18, 18, 0)]),
           (3, 8, [(16, 37, 35, 0)]), (3, 64, [(64, 14, 14, 1), (64, 28, 28, 0)]),
           (2, 64, [(64, 9, 11, 0)]), (2, 64, [(32, 9, 11, 0)]), (2, 32, [(96, 9, 11, 0)])]
# generic geometries of those tests: (B, cout, ctot, Hout, Wout, KH, KW); every one has 1 split
WG_OLD = [(3, 16, 32, 6, 6, 3, 3), (2, 64, 8, 20, 18, 7, 7), (2, 48, 32, 7, 8, 3, 3)]


def _assert_plan(name, plan, want):
    got = {k: plan[k] for k in want}
    assert got == want, f"{name}: the planner gives {got}, the case was chosen for {want}"


def w33_dims(case):
    """(H, W, Ctot) of a 3x3 case."""
    C, h, w, up2 = case["srcs"][0]
    return (2 * h if up2 else h), (2 * w if up2 else w), sum(s[0] for s in case["srcs"])


def w33_case_plan(name):
    c = W33_CASES[name]
    H, W, _ = w33_dims(c)
    plan = w33_plan(c["B"], c["cout"], c["srcs"], H, W)
    assert plan is not None, name
    _assert_plan(name, plan, c["plan"])
    return plan


def wg_dims(case):
    """(Ho, Wo) of a generic case."""
    (KH, KW), (ph, pw), s = case["k"], case["pad"], case["stride"]
    return (case["H"] + 2 * ph - KH) // s + 1, (case["W"] + 2 * pw - KW) // s + 1


def wg_case_plan(name):
    c = WG_CASES[name]
    Ho, Wo = wg_dims(c)
    plan = wg_plan(c["B"], c["cout"], c["cpad"], Ho, Wo, *c["k"])
    _assert_plan(name, plan, c["plan"])
    return plan


def w11_case_plan(shape, want):
    B, cin, cout, H, W, stride = shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    plan = w11_plan(B, cin, H, W, stride, cout, Ho, Wo)
    _assert_plan(str(shape), plan, want)
    return plan


def coverage():
    """What the table reaches, for the assertion that nothing in it went missing."""
    p33 = {n: w33_case_plan(n) for n in W33_CASES}
    pg = {n: wg_case_plan(n) for n in WG_CASES}
    p11 = [w11_case_plan(s, w) for s, w in W11_CASES]
    return dict(
        ppb={min(p["ppb"], 3) for p in p33.values()},
        last={"short" if p["last"] < p["ppb"] else "exact" for p in p33.values()
              if p["ppb"] > 1},
        splits={p["splits"] for p in p33.values()},
        msub={p["msub"] for p in p33.values()},
        passes={p["nchunk"] > 0 for p in p33.values()},
        generic_tail=all(p["splits"] > 1 and p["tail"] for p in pg.values()),
        w11={(p["wm"], p["wn"]) for p in p11})
