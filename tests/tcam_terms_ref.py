"""fp64 reference, elementwise bounds and input builders of tcam_tcam_losses_terms: the terms
of tests/train_fwd_ref.tcam_loss_ref plus BgSizeGreatSizeFgTcams, FgSizeTcams and
EmptyOutsideBboxTcams (losses/tcam.py:281-430), and the teacher-statistics kernel.  Pinned to
the reference's own classes by tests/golden/tcam_terms.npz (tests/golden/make_terms_golden.py)
in tests/test_tcam_terms_ref.py; used on the device by tests/test_x_tcam_terms_gpu.py.

Bound rule as in train_fwd_ref: n 2^-24 (sum of the magnitudes of the terms of the output), n =
the fp32 roundings on the kernel's path; no bound comes from a kernel's output.  Plain torch,
CPU only."""
import math

import torch

from train_fwd_ref import U, f32, _elb_terms, loss_input, tcam_loss_ref

KEYS = ("bgfg", "fgsz", "eob")            # slots 5, 6, 7 of the entry's losses[8]
LAM3 = (0.5, 0.8, 0.3)                    # one order, no term hides under another
T_MIXED = (2.5, 10.0, 1.0)                # the run with a different t per term
EPS = 0.003
LAM_BASE = (0.7, 0.3, 0.2)


def elb64(fx, mag, t):
    """ELB_t elementwise on the barrier argument fx (fp64): value l, d l / d fx, the branch
    (True: log, fx <= -1/t^2), the fp32 bounds of both, and the error bound e_fx of fx itself.
    fx reaches the fp32 formula as one cast of an fp64 expression whose terms' magnitudes sum
    to ``mag``: e_fx = 2^-24 mag (for bg - fg, which cancels, mag = bg + fg, not |bg - fg|).
    The formula's own roundings are train_fwd_ref._elb_terms' counts on |fx|: log branch
    4 2^-24 |l| (1/t, logf within an ulp: 2, the product) and 3 2^-24 dl; linear branch
    8 2^-24 (t |fx| + |log(1/t^2)| / t + 1/t) + 2 2^-24 / t, dl = t exact.  e_fx enters the value
    through |dl| and, in the log branch, the derivative through dl / |fx|."""
    ct = -1.0 / (t * t)
    is_log = fx <= ct
    safe = (-fx).clamp(min=-ct)
    l_log = -(1.0 / t) * torch.log(safe)
    l_lin = t * fx - (1.0 / t) * math.log(-ct) + 1.0 / t
    l = torch.where(is_log, l_log, l_lin)
    dl = torch.where(is_log, (1.0 / t) / safe, torch.full_like(fx, t))
    e_fx = U * mag
    b_log = 4 * U * l_log.abs()
    b_lin = 8 * U * (t * fx.abs() + abs(math.log(-ct)) / t + 1.0 / t) + 2 * U / t
    b_l = torch.where(is_log, b_log, b_lin) + dl * e_fx
    b_dl = torch.where(is_log, 3 * U * dl + dl / safe * e_fx, torch.zeros_like(dl))
    return dict(l=l, dl=dl, is_log=is_log, b_l=b_l, b_dl=b_dl, e_fx=e_fx, fx=fx,
                ambiguous=(fx - ct).abs() <= e_fx)


def terms_ref(f, S, seeds, AS, gx, extra, lam, t, fg_size, msk, lam3, t3, eps):
    """tcam_tcam_losses_terms in fp64 on fcams f (B, 2, HW), the softmax S the device stored,
    the inputs of tcam_loss_ref, fg_size (B,) or None, msk (B, HW) or None; lam3 / t3 = the
    lambdas / ELB t of (bgfg, fgsz, eob), eps.

      bgfg = lam / B sum_b ELB(-(bg_b - fg_b)),   bg / fg = sum_hw S[b, 0 / 1]
      fgsz = lam / 2 / B sum_b (ELB(fs_b - eps - fg_b / HW) + ELB(fg_b / HW - fs_b - eps))
      eob  = lam / B sum_b ELB(a_b),   a_b = sum_hw S[b, 1] (1 - msk[b])
      gS_0 = size' - bgfg',  gS_1 = size' + bgfg' + lam / (2 B HW) (ELB'_2 - ELB'_1)
             + lam / B ELB'(a_b) (1 - msk)      (+ the CRF and extra terms of tcam_loss_ref)

    Returns losses (8: total, sl, crf, size, extra, bgfg, fgsz, eob) and bounds, dF and b_dF,
    and ``elb``: per term the list of its elb64 dicts (branch, ambiguity band)."""
    base = tcam_loss_ref(f, S, seeds, AS, gx, extra, lam, t)
    f, S = f.double(), S.double()
    B, _, HW = f.shape
    lb, lf, le = (f32(v) for v in lam3)
    tb, tf, te = (f32(v) for v in t3)
    eps = f32(eps)
    on_b, on_f, on_e = lb != 0.0, fg_size is not None and lf != 0.0, \
        msk is not None and le != 0.0
    zero = torch.zeros((), dtype=torch.float64)
    bg, fg = S[:, 0].sum(1), S[:, 1].sum(1)
    elbs = {}
    vals, b_vals = [zero] * 3, [zero] * 3
    # per-plane constants of d loss / d S and their bounds / magnitudes, then the pixel term
    cc = torch.zeros(B, 2, dtype=torch.float64)
    b_cc = torch.zeros(B, 2, dtype=torch.float64)
    m_cc = torch.zeros(B, 2, dtype=torch.float64)
    if on_b:
        e = elb64(-(bg - fg), bg + fg, tb)
        elbs["bgfg"] = [e]
        vals[0] = lb * e["l"].sum() / B
        b_vals[0] = lb * e["b_l"].sum() / B + U * vals[0].abs()
        c = lb * e["dl"] / B                      # the product and the division: 2
        b_c = (e["b_dl"] / e["dl"] + 2 * U) * c
        cc += torch.stack([-c, c], 1)
        b_cc += torch.stack([b_c, b_c], 1)
        m_cc += torch.stack([c, c], 1)
    if on_f:
        fs = fg_size.double()
        fgn = fg / HW
        mag = fs.abs() + eps + fgn
        e1, e2 = elb64(fs - eps - fgn, mag, tf), elb64(fgn - fs - eps, mag, tf)
        elbs["fgsz"] = [e1, e2]
        vals[1] = lf * 0.5 * (e1["l"].sum() + e2["l"].sum()) / B
        b_vals[1] = lf * 0.5 * (e1["b_l"].sum() + e2["b_l"].sum()) / B + U * vals[1].abs()
        # lam 0.5 (dl2 - dl1) / (B HW): the subtraction, B HW, the product, the division: 4,
        # on the magnitude dl1 + dl2
        k = lf * 0.5 / (B * HW)
        cc[:, 1] += k * (e2["dl"] - e1["dl"])
        b_cc[:, 1] += k * (e1["b_dl"] + e2["b_dl"]) + 4 * U * k * (e1["dl"] + e2["dl"])
        m_cc[:, 1] += k * (e1["dl"] + e2["dl"])
    pix = b_pix = m_pix = None
    if on_e:
        w = 1.0 - msk.double()
        e = elb64((S[:, 1] * w).sum(1), (S[:, 1] * w.abs()).sum(1), te)
        elbs["eob"] = [e]
        vals[2] = le * e["l"].sum() / B
        b_vals[2] = le * e["b_l"].sum() / B + U * vals[2].abs()
        cm = le * e["dl"] / B
        b_cm = (e["b_dl"] / e["dl"] + 2 * U) * cm
        pix = cm[:, None] * w
        # 1 - msk in fp32 (on 1 + |msk|) and the product
        b_pix = b_cm[:, None] * w.abs() + cm[:, None] * U * (1 + msk.double().abs() + w.abs())
        m_pix = pix.abs()
    v_new = torch.stack(vals)
    total = base["losses"][0] + v_new.sum()
    mags = base["losses"][1:].abs().sum() + v_new.abs().sum()
    b_total = base["bounds"][0] + torch.stack(b_vals).sum() + 3 * U * mags
    losses = torch.cat([total[None], base["losses"][1:], v_new])
    bounds = torch.cat([b_total[None], base["bounds"][1:], torch.stack(b_vals)])
    # ---- gradient: tcam_loss_ref's, with the constants and the pixel term added to gS
    l0, l1, l2 = (f32(v) for v in lam)
    t = f32(t)
    use_sl, use_crf, use_size = seeds is not None, AS is not None, l2 != 0.0
    _, dl, _, _, b_dl = _elb_terms(S.sum(2), t)
    cs = -l2 * 0.5 * dl / B if use_size else torch.zeros_like(dl)
    b_cs = (b_dl / dl + 3 * U) * cs.abs()
    gS = (cs + cc)[:, :, None].expand(B, 2, HW).clone()
    mag = (cs.abs() + m_cc)[:, :, None].expand(B, 2, HW).clone()
    eg = (b_cs + b_cc)[:, :, None].expand(B, 2, HW).clone()
    if use_crf:
        c1 = -2.0 * l1 / B
        gS += c1 * AS.double()
        mag += (c1 * AS.double()).abs()
    if gx is not None:
        gS += gx.double()
        mag += gx.double().abs()
    if pix is not None:
        gS[:, 1] += pix
        mag[:, 1] += m_pix
        eg[:, 1] += b_pix
    # tcam_loss_ref's four (coef1, its product, two additions) + the three further additions
    eg = eg + 7 * U * mag
    dot = (S * gS).sum(1, keepdim=True)
    dot_mag = (S * gS.abs()).sum(1, keepdim=True)
    e_dot = (S * eg).sum(1, keepdim=True) + 3 * U * dot_mag
    dF = S * (gS - dot)
    b_dF = S * (eg + e_dot) + 3 * U * S * (gS.abs() + dot_mag)
    if use_sl:
        valid = (seeds == 0) | (seeds == 1)
        nv = int(valid.sum())
        if nv > 0 and l0 != 0.0:
            onehot = torch.stack([(seeds == 0), (seeds == 1)], 1).double()
            term = l0 / nv * (S - onehot) * valid[:, None].double()
            dF = dF + term
            b_dF = b_dF + 4 * U * term.abs()
    return dict(losses=losses, bounds=bounds, dF=dF, b_dF=b_dF, elb=elbs)


# ---------------------------------------------------------------------------- inputs
MASK_KINDS = ("box", "real", "ones", "zeros")


def mask_kind(b, HW):
    return MASK_KINDS[(b + HW) % 4]


def terms_input(B, HW, seed):
    """loss_input(B, HW, seed) with: every fourth frame's foreground raised (fg > bg; the odd
    frames have bg >> fg, the others bg ~ fg); fg_size ~ the frame's own fg / HW (+ 0.004), 0
    and 0.9 in turn (~, <<, >>); msk per frame, in turn from (b + HW) % 4: a 0/1 box (the
    middle half of the pixels), real values in [0.5, 2] (a negative outside area; on a frame
    with bg ~ fg wherever HW is odd), all ones, all zeros (an empty box)."""
    c = loss_input(B, HW, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    f = c["f"].clone()
    f[2::4, 1] += 4.0
    fgn = torch.softmax(f.double(), 1)[:, 1].sum(1) / HW
    fs = torch.zeros(B, dtype=torch.float64)
    fs[0::3] = fgn[0::3] + 0.004
    fs[2::3] = 0.9
    msk = torch.zeros(B, HW)
    j = torch.arange(HW)
    for b in range(B):
        k = mask_kind(b, HW)
        if k == "box":
            msk[b] = ((j >= HW // 4) & (j < HW - HW // 4)).float()
        elif k == "ones":
            msk[b] = 1.0
        elif k == "real":
            msk[b] = 0.5 + 1.5 * torch.rand(HW, generator=g)
    c.update(f=f, fg_size=fs.float(), msk=msk)
    return c


def terms_runs(c):
    """(name, seeds, AS, gx, extra, lam, fg_size, msk, lam3) of the runs on one input: each
    new term alone, the three together, and all seven slots with seeds, AS and the extra
    term."""
    n = (None,) * 4
    z = (0.0, 0.0, 0.0)
    return [("bgfg", *n, z, None, None, (LAM3[0], 0.0, 0.0)),
            ("fgsz", *n, z, c["fg_size"], None, (0.0, LAM3[1], 0.0)),
            ("eob", *n, z, None, c["msk"], (0.0, 0.0, LAM3[2])),
            ("three", *n, z, c["fg_size"], c["msk"], LAM3),
            ("seven", c["seeds"], c["AS"], c["gx"], c["extra"], LAM_BASE, c["fg_size"],
             c["msk"], LAM3)]


def t_cases():
    from train_fwd_ref import LOSS_T
    return [(t, t, t) for t in LOSS_T] + [T_MIXED]


# ---------------------------------------------------------------- teacher statistics
STATS_SHAPES = [(1, 1, 1), (3, 7, 9), (2, 64, 65)]


def stats_input(B, H, W, seed):
    """CAMs in [0, 1], a random 0/1 roi, boxes (x0, y0, x1, y1): frame 0 the whole frame (it
    touches every border), the last frame (B >= 2) empty, the others random."""
    g = torch.Generator().manual_seed(seed)
    cams = torch.rand(B, H, W, generator=g)
    roi = (torch.rand(B, H, W, generator=g) < 0.4).to(torch.uint8)
    bbox = torch.zeros(B, 4, dtype=torch.int32)
    for b in range(B):
        x0, y0 = int(torch.randint(0, W, (1,), generator=g)), int(torch.randint(0, H, (1,), generator=g))
        bbox[b] = torch.tensor([x0, y0, int(torch.randint(x0, W + 1, (1,), generator=g)),
                                int(torch.randint(y0, H + 1, (1,), generator=g))])
    bbox[0] = torch.tensor([0, 0, W, H])
    if B >= 2:
        bbox[B - 1] = torch.tensor([W // 2, H // 2, W // 2, H // 2])
    return cams, roi, bbox


def stats_ref(cams, roi, bbox):
    """mask[b, 0, y0:y1, x0:x1] = 1 (exact) and fg_size = sum(cam roi) / (H W) in fp64 with the
    bound 2 2^-24 sum |cam roi| / (H W) (the fp32 store, with margin for the fp64 sums)."""
    B, H, W = cams.shape
    msk = torch.zeros(B, 1, H, W)
    for b in range(B):
        x0, y0, x1, y1 = (int(v) for v in bbox[b])
        msk[b, 0, y0:y1, x0:x1] = 1.0
    prod = cams.double() * roi.double()
    return msk, prod.sum((1, 2)) / (H * W), 2 * U * prod.abs().sum((1, 2)) / (H * W)
