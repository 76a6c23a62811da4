"""CPU checks of tests/train_fwd_ref.py, the references and bounds of the training forward's
kernel tests (tests/test_x_train_fwd_gpu.py): every reference pinned to torch's own fp64
operation; every checker's teeth (plausible wrong kernels, emulated in torch, must be
rejected); and an emulation of each kernel's own formula — the one-pass fp64 sums for the BN
statistics, fp32 arithmetic elsewhere — must be accepted at every case the GPU file runs, so
the bounds are safe to state before any device run.  The conditions on the shared input
builders are asserted here too."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_fwd_ref as R
from oracle import train_ref as T

F32, F64 = torch.float32, torch.float64


# ----------------------------------------------------------------------- emulations
def sum_rows(v, acc):
    """Row sums of (C, n) accumulated in ``acc`` the way a block of 256 threads would: each
    lane strides the row, then a tree over the lanes (torch's own fp32 sums accumulate wider)."""
    C, n = v.shape
    pad = torch.zeros(C, -(-n // 256) * 256, dtype=acc)
    pad[:, :n] = v.to(acc)
    lanes = torch.zeros(C, 256, dtype=acc)
    for row in pad.view(C, -1, 256).unbind(1):
        lanes = lanes + row
    while lanes.shape[1] > 1:
        lanes = lanes[:, ::2] + lanes[:, 1::2]
    return lanes[:, 0].double()


def emu_bn_stats(y64, eps, mom, rm, rv, acc=F64, invstd_unbiased=False, run_biased=False,
                 drop=False, mom_swapped=False):
    """bn_stats_co_kernel + bn_finalize_kernel: one-pass sums (in ``acc``), m = s / P, var =
    max(q / P - m^2, 0), fp32 outputs; the keyword variants are the wrong kernels."""
    B, C, H, W = y64.shape
    P = B * H * W
    v = y64.permute(1, 0, 2, 3).reshape(C, P)
    if drop:
        v = v[:, :-1]
    s, q = sum_rows(v, acc), sum_rows(v.to(acc) * v.to(acc), acc)
    m = s / P
    var = (q / P - m * m).clamp(min=0)
    unb = var * P / (P - 1)
    mu = R.f32(mom)
    a, b = (mu, 1 - mu) if mom_swapped else (1 - mu, mu)
    return dict(mean=m.float(),
                invstd=(1 / torch.sqrt((unb if invstd_unbiased else var) + R.f32(eps))).float(),
                run_mean=(a * rm.double() + b * m).float(),
                run_var=(a * rv.double() + b * (var if run_biased else unb)).float())


def emu_bn_relu(y64, mean, invstd, gamma, beta, lay):
    v = lambda t: t.float()[None, :, None, None]
    z = v(gamma) * ((y64.float() - v(mean)) * v(invstd)) + v(beta)
    return R.store(torch.where(z < 0, torch.zeros_like(z), z), lay)


def emu_softmax2(f):
    m = f.max(1, keepdim=True).values
    e = torch.exp(f - m)
    return e / e.sum(1, keepdim=True)


def emu_losses(f, S, seeds, AS, gx, extra, lam, t, wrong=None):
    """loss_partial_kernel + loss_finalize_kernel + loss_grad_kernel: fp32 per-pixel
    arithmetic, fp64 sums.  ``wrong``: one of the teeth."""
    B, _, HW = f.shape
    l0, l1, l2, t = (np.float32(v) for v in (*lam, t))
    one = np.float32(1)
    Sd = S.double()
    bl = Sd.sum(2)
    fx = (-bl).float()
    ct = torch.tensor(-1.0 / (float(t) * float(t))).float()
    is_log = fx <= ct
    if wrong == "always_log":
        is_log = torch.ones_like(is_log)
    it = one / t
    l_log = -it * torch.log(-fx)
    l_lin = t * fx - it * np.log(one / (t * t)) + it
    l = torch.where(is_log, l_log, l_lin)
    dl = torch.where(is_log, -it / fx, torch.full_like(fx, float(t)))
    half = np.float32(1.0 if wrong == "no_half" else 0.5)
    nv, ce = 0, 0.0
    if seeds is not None:
        valid = (seeds == 0) | (seeds == 1)
        nv = int(valid.sum())
        m = f.max(1).values
        lse = m + torch.log(torch.exp(f[:, 0] - m) + torch.exp(f[:, 1] - m))
        ce = ((lse - torch.where(seeds == 1, f[:, 1], f[:, 0])).double() * valid).sum()
    n_ce = B * HW if wrong == "ce_all_pixels" else nv
    n_size = nv if (wrong == "size_div_nv" and nv) else B
    sl = np.float32(float(l0) * float(ce) / n_ce) if nv else \
        np.float32("nan" if (seeds is not None and l0 != 0) else 0)
    crf = np.float32(float(l1) * -float((Sd * AS.double()).sum()) / B) if AS is not None \
        else np.float32(0)
    sz = np.float32(float(l2) * float(half) * float(l.double().sum()) / n_size) if l2 != 0 \
        else np.float32(0)
    ex = np.float32(float(extra)) if extra is not None else np.float32(0)
    total = ((sl + crf) + sz) + ex if extra is not None else (sl + crf) + sz
    cs = (-l2 * half * dl / np.float32(n_size)) if l2 != 0 else torch.zeros_like(dl)
    g = cs[:, :, None].expand(B, 2, HW).clone()
    if AS is not None:
        c1 = np.float32(-1.0 if wrong == "crf_grad_1" else -2.0) * l1 / np.float32(B)
        g = g + c1 * AS
    if gx is not None:
        g = g + gx
    dot = S[:, 0] * g[:, 0] + S[:, 1] * g[:, 1]
    r = S * (g - dot[:, None])
    if nv:
        c0 = np.float32(float(l0) / n_ce)
        onehot = torch.stack([seeds == 0, seeds == 1], 1).float()
        r = r + c0 * (S - onehot) * valid[:, None].float()
    return torch.tensor([total, sl, crf, sz, ex], dtype=F32), r


def emu_pool(x64, amp, wrong_div=False):
    B, C, H, W = x64.shape
    HW, per = H * W, -(-H * W // 32)
    v = torch.zeros(B, C, 32 * per)
    v[:, :, :HW] = x64.float().reshape(B, C, HW)
    s = v.view(B, C, 32, per).sum(3).sum(2)
    p = s / np.float32(32 * per if wrong_div else HW)
    return p.half().float() if amp else p


def emu_fc(pooled, w, b, amp):
    h = (lambda v: v.half().float()) if amp else (lambda v: v)
    return h(pooled @ h(w).t() + h(b))


def emu_ce(z, y, lam, gscale, no_b=False, no_lam=False, no_gs=False):
    B, K = z.shape
    lam, gs = R.f32(lam), (1.0 if gscale is None else R.f32(gscale))
    z64 = z.double()
    lse = torch.logsumexp(z64, 1)
    ok = (y >= 0) & (y < K)
    pick = z64.gather(1, y.long().clamp(0, K - 1)[:, None])[:, 0]
    loss = (torch.where(ok, lse - pick, torch.full_like(lse, float("nan"))).sum() / B * lam).float()
    p = torch.exp(z64 - lse[:, None])
    onehot = torch.zeros_like(p).scatter_(1, y.long().clamp(0, K - 1)[:, None], 1.0)
    dz = (p - onehot) / (1 if no_b else B) * (1 if no_lam else lam) * (1 if no_gs else gs)
    return loss, dz.float()


def emu_cls_bwd(dz, pooled, w, amp):
    h = (lambda v: v.half().float()) if amp else (lambda v: v)
    dz = h(dz)
    return h(dz.t() @ pooled), h(dz.sum(0)), h(dz @ h(w))


def emu_pool_bwd(dp, HW, lay):
    return R.store(dp * (np.float32(1) / np.float32(HW)), lay)


# ------------------------------------------------------------------------------ BN
def _bn_ratios(got, ref):
    return {k: R.ratio(got[k].double(), ref[k], ref["b_" + k])
            for k in ("mean", "invstd", "run_mean", "run_var")}


@pytest.mark.parametrize("C,bhw", [(2048, (2, 5, 7)), (512, (3, 40, 37)), (8, (1, 25, 41))])
def test_bn_stats_ref_matches_torch_batch_norm(C, bhw):
    """Mean / invstd / running statistics of the reference == F.batch_norm(training=True) in
    fp64 (momentum the fp32 value), and relu(BN) == bn_relu_ref on them."""
    c = R.bn_input(C, *bhw, seed=C)
    y = c["y"].double()
    mu = R.f32(R.BN_MOMENTUM)
    for eps in R.BN_EPS:
        ref = R.bn_stats_ref(y, eps, R.BN_MOMENTUM, c["run_mean"], c["run_var"])
        rm, rv = c["run_mean"].double().clone(), c["run_var"].double().clone()
        out = F.relu(F.batch_norm(y, rm, rv, c["gamma"].double(), c["beta"].double(), True, mu,
                                  R.f32(eps)))
        assert torch.allclose(rm, ref["run_mean"], rtol=1e-13, atol=1e-13)
        assert torch.allclose(rv, ref["run_var"], rtol=1e-12, atol=1e-13)
        mine, _ = R.bn_relu_ref(y, ref["mean"], ref["invstd"], c["gamma"], c["beta"], "s3")
        scale = (y.abs() + ref["mean"].abs()[None, :, None, None]) * \
            ref["invstd"][None, :, None, None] + 50
        assert ((mine - out).abs() <= 1e-12 * scale).all()


@pytest.mark.parametrize("lay", ["s3", "s2", "s1"])
@pytest.mark.parametrize("C,bhw", R.BN_SHAPES)
def test_bn_stats_checker_accepts_one_pass_fp64_and_rejects_wrong_kernels(C, bhw, lay):
    c = R.bn_input(C, *bhw, seed=C + bhw[1])
    y = R.store(c["y"], lay)
    P = bhw[0] * bhw[1] * bhw[2]
    for eps in R.BN_EPS:
        ref = R.bn_stats_ref(y, eps, R.BN_MOMENTUM, c["run_mean"], c["run_var"])
        args = (y, eps, R.BN_MOMENTUM, c["run_mean"], c["run_var"])
        good = _bn_ratios(emu_bn_stats(*args), ref)
        assert max(good.values()) <= 0.5, good
        bad = _bn_ratios(emu_bn_stats(*args, acc=F32), ref)
        assert not bad["mean"] <= 1 or not bad["invstd"] <= 1, bad
        assert not _bn_ratios(emu_bn_stats(*args, invstd_unbiased=True), ref)["invstd"] <= 1
        assert not _bn_ratios(emu_bn_stats(*args, run_biased=True), ref)["run_var"] <= 1
        bad = _bn_ratios(emu_bn_stats(*args, drop=True), ref)
        assert not bad["mean"] <= 1 and not bad["invstd"] <= 1, bad
        bad = _bn_ratios(emu_bn_stats(*args, mom_swapped=True), ref)
        assert not bad["run_mean"] <= 1 and not bad["run_var"] <= 1, bad
        # the control of the GPU test: the other eps
        other = emu_bn_stats(y, 1e-3 if eps == 1e-5 else 1e-5, *args[2:])
        assert not _bn_ratios(other, ref)["invstd"] <= 1


@pytest.mark.parametrize("lay", ["s3", "s2", "s1"])
@pytest.mark.parametrize("C,bhw", R.BN_SHAPES)
def test_bn_relu_checker_accepts_fp32_and_rejects_wrong_kernels(C, bhw, lay):
    c = R.bn_input(C, *bhw, seed=C + bhw[1] + 1)
    y = R.store(c["y"], lay)
    st = R.bn_stats_ref(y, 1e-5, R.BN_MOMENTUM)
    mean, invstd = st["mean"].float(), st["invstd"].float()
    ref, bound = R.bn_relu_ref(y, mean, invstd, c["gamma"], c["beta"], lay)
    assert (ref[:, R.DEAD_CH] == 0).all() and (ref[:, R.LIVE_CH] > 0).all()
    assert (ref[:, R.ZERO_GAMMA_CH] == c["beta"][R.ZERO_GAMMA_CH].double().clamp(min=0)).all()
    r = R.ratio(emu_bn_relu(y, mean, invstd, c["gamma"], c["beta"], lay), ref, bound)
    assert r <= 1.0, r
    no_eps = (1 / torch.sqrt(st["var"])).float()        # eps forgotten (inf on the constant channel)
    assert not R.accept(emu_bn_relu(y, mean, no_eps, c["gamma"], c["beta"], lay), ref, bound)
    gam, bet = c["gamma"].clone(), c["beta"].clone()
    gam[7], bet[7] = c["beta"][7], c["gamma"][7]        # gamma and beta swapped for one channel
    assert not R.accept(emu_bn_relu(y, mean, invstd, gam, bet, lay), ref, bound)


# ---------------------------------------------------- softmax, channel sums, up2 bwd
@pytest.mark.parametrize("B,HW", R.SOFTMAX_SHAPES)
def test_softmax2_ref(B, HW):
    f = R.softmax_input(B, HW, seed=HW)
    ref, bound = R.softmax2_ref(f.double())
    assert torch.equal(ref, F.softmax(f.double(), 1))
    if HW > 1:
        gaps = (f[:, 0] - f[:, 1]).abs()
        assert (gaps == 0).any() and (gaps > 100).any() and (f.abs() > 9e3).any()
    r = R.ratio(emu_softmax2(f), ref, bound)
    assert r <= 1.0, r
    # a softmax that skips the max subtraction overflows on the +1e4 offsets; one computed in
    # fp16-rounded logits misses the bound
    e = torch.exp(f)
    assert HW == 1 or not R.accept(e / e.sum(1, keepdim=True), ref, bound)
    assert not R.accept(emu_softmax2(f.half().float() + 2.0 ** -12), ref, bound)


@pytest.mark.parametrize("B,C,HW", R.CHANSUM_SHAPES)
def test_chansum_ref(B, C, HW):
    x = R.chansum_input(B, C, HW, seed=HW)
    ref, bound = R.chansum_ref(x.double())
    assert torch.equal(ref, x.double().sum((0, 2)))
    assert (ref.abs() <= 1e-3 * x.abs().sum((0, 2))).all()      # the sums nearly cancel
    assert R.accept(x.double().sum(2).sum(0).float(), ref, bound)
    seq = sum_rows(x.permute(1, 0, 2).reshape(C, -1), F32).float()     # fp32 accumulation
    assert not R.accept(seq, ref, bound) or B * HW < 4096
    assert not R.accept((x.double().sum((0, 2)) - x[B - 1, :, HW - 1].double()).float(), ref, bound)


@pytest.mark.parametrize("lay", ["s3", "s1"])
@pytest.mark.parametrize("B,C,H,W", R.UP2_SHAPES)
def test_up2_bwd_ref(B, C, H, W, lay):
    g = torch.Generator().manual_seed(C + H)
    gu = R.store(torch.randn(B, C, 2 * H, 2 * W, generator=g), lay)
    ref, bound = R.up2_bwd_ref(gu, lay)
    x = torch.zeros(B, C, H, W, dtype=F64, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode="nearest").backward(gu)
    assert torch.allclose(ref, x.grad, rtol=1e-15, atol=1e-15)
    v = gu.float().view(B, C, H, 2, W, 2)
    emu = ((v[:, :, :, 0, :, 0] + v[:, :, :, 0, :, 1]) + v[:, :, :, 1, :, 0]) + v[:, :, :, 1, :, 1]
    assert R.accept(R.store(emu, lay), ref, bound)
    wrong = v[:, :, :, 0].sum(-1) * 2            # the upper row twice
    assert not R.accept(R.store(wrong, lay), ref, bound)


# ----------------------------------------------------------------------- TCAM losses
G = os.path.join(os.path.dirname(__file__), "golden", "tcam_losses.npz")


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_tcam_loss_ref_matches_the_loss_oracle(case):
    """tcam_loss_ref with the CRF off == oracle/train_ref.tcam_losses (pinned to the
    reference's goldens) and its autograd gradient, on the three golden inputs."""
    d = np.load(G)
    d = {k[2:]: d[k] for k in d.files if k.startswith(case + "_")}
    f = torch.from_numpy(d["fcams"]).double().requires_grad_(True)
    seeds = torch.from_numpy(d["seeds"])
    t = R.f32(float(d["elb_t"]))
    total, sl, crf, size = T.tcam_losses(f, None, seeds, lam_sl=1.0, lam_crf=0.0,
                                         lam_size=R.f32(0.01), elb_t=t)
    total.backward()
    B = f.shape[0]
    fd = f.detach().reshape(B, 2, -1)
    ref = R.tcam_loss_ref(fd, torch.softmax(fd, 1), seeds.reshape(B, -1).int(), None, None, None,
                          (1.0, 0.0, 0.01), t)
    for i, v in enumerate((total, sl, crf, size)):
        assert abs(float(ref["losses"][i]) - float(v.detach())) <= 1e-12 * max(1.0, abs(float(v.detach())))
    g = f.grad.reshape(B, 2, -1)
    assert (ref["dF"] - g).abs().max() <= 1e-12 * g.abs().max()


def test_tcam_loss_ref_crf_gradient_is_the_doubled_surrogate():
    """d / dS of the surrogate 2 lam -sum(S AS) / B with AS constant, through the softmax,
    == the reference's dF with only the CRF term on."""
    c = R.loss_input(3, 40, seed=3)
    f = c["f"].double().requires_grad_(True)
    S = torch.softmax(f, 1)
    (2 * R.f32(0.3) * -(S * c["AS"].double()).sum() / 3).backward()
    ref = R.tcam_loss_ref(c["f"], S.detach(), None, c["AS"], None, None, (0.0, 0.3, 0.0), 1.0)
    assert (ref["dF"] - f.grad).abs().max() <= 1e-12 * f.grad.abs().max()
    assert abs(float(ref["losses"][2]) - R.f32(0.3) * -float((S.detach() * c["AS"]).sum()) / 3) < 1e-12


def _loss_ratios(got_l, got_d, ref, five):
    n = 5 if five else 4
    out = {k: R.ratio(got_l[i:i + 1], ref["losses"][i:i + 1], ref["bounds"][i:i + 1])
           for i, k in enumerate(("total", "sl", "crf", "size", "extra")[:n])}
    out["dF"] = R.ratio(got_d, ref["dF"], ref["b_dF"])
    return out


@pytest.mark.parametrize("B,HW", R.LOSS_SHAPES)
def test_loss_inputs_and_checker(B, HW):
    """The conditions on the shared loss inputs; the fp32 emulation of the kernels is accepted
    on every run of the GPU file; the wrong kernels are rejected."""
    c = R.loss_input(B, HW, seed=R.loss_seed(B, HW))
    f = c["f"]
    S = emu_softmax2(f)
    valid = (c["seeds"] == 0) | (c["seeds"] == 1)
    assert valid[0].all() and (B == 1 or not valid[B - 1].any())
    mixed = valid.any(1) & ~valid.all(1)
    assert B < 3 or HW < 16 or mixed.any()
    branches, even_log = set(), B < 2
    for t in R.LOSS_T:
        for name, seeds, AS, gx, extra, lam in R.loss_runs(c):
            ref = R.tcam_loss_ref(f, S, seeds, AS, gx, extra, lam, t)
            assert (ref["dist"] > 1e-3).all(), (t, float(ref["dist"].min()))
            branches |= set(ref["is_log"].flatten().tolist())
            if B >= 2:     # one class's plane sum below 1/t^2 in some frames, not in others
                assert not ref["is_log"][1::2, 1].any()
                even_log |= bool(ref["is_log"][0::2, 1].any())
            gl, gd = emu_losses(f, S, seeds, AS, gx, extra, lam, t)
            r = _loss_ratios(gl, gd, ref, extra is not None)
            assert max(r.values()) <= 1.0, (t, name, r)
            if name != "all" or HW == 1:
                continue
            for wrong, key in (("no_half", "size"), ("size_div_nv", "size"),
                               ("ce_all_pixels", "sl"), ("crf_grad_1", "dF"),
                               ("always_log", "size")):
                gl, gd = emu_losses(f, S, seeds, AS, gx, extra, lam, t, wrong=wrong)
                r = _loss_ratios(gl, gd, ref, False)
                assert not r[key] <= 1.0 and not r["total" if key != "dF" else "dF"] <= 1.0, \
                    (t, wrong, r)
                if key in ("size", "sl"):
                    assert not r["dF"] <= 1.0, (t, wrong, r)
    assert even_log and branches == {True, False}     # both ELB branches somewhere in the parametrisation


def test_loss_ref_without_a_valid_seed_is_nan():
    c = R.loss_input(2, 16, seed=1)
    seeds = torch.full_like(c["seeds"], R.IGNORE)
    S = emu_softmax2(c["f"])
    ref = R.tcam_loss_ref(c["f"], S, seeds, c["AS"], None, None, R.LAM_ALL, 1.0)
    assert torch.isnan(ref["losses"][:2]).all() and torch.isfinite(ref["losses"][2:]).all()
    lo = F.cross_entropy(c["f"].double(), seeds.long(), ignore_index=R.IGNORE)
    assert torch.isnan(lo)
    off = R.tcam_loss_ref(c["f"], S, None, c["AS"], None, None, R.LAM_ALL, 1.0)
    assert torch.equal(ref["dF"], off["dF"])     # the gradient keeps the other terms only
    gl, gd = emu_losses(c["f"], S, seeds, c["AS"], None, None, R.LAM_ALL, 1.0)
    assert torch.isnan(gl[:2]).all() and R.accept(gd, ref["dF"], ref["b_dF"])
    zero = R.tcam_loss_ref(c["f"], S, seeds, c["AS"], None, None, (0.0, 0.3, 0.2), 1.0)
    assert torch.isfinite(zero["losses"]).all() and float(zero["losses"][1]) == 0.0


# ------------------------------------------------------------------------ CRF energy
@pytest.mark.parametrize("N,K,H,W", R.CRF_SHAPES)
def test_crf_energy_and_grad_ref(N, K, H, W):
    seg, AS = R.crf_input(N, K, H, W, seed=H)
    e, be = R.crf_energy_ref(seg.double(), AS.double(), N)
    assert abs(float(e) + float((seg.double() * AS.double()).sum()) / N) <= 1e-12 * abs(float(e))
    emu = (seg * AS).sum() * (np.float32(-1) / np.float32(N))
    assert R.accept(emu.reshape(1), e.reshape(1), be.reshape(1))
    assert not R.accept(-emu.reshape(1) * (N + 1) / N, e.reshape(1), be.reshape(1))
    gout = 0.37
    g, bg = R.crf_grad_ref(AS.double(), np.float32(gout), N)
    assert R.accept(np.float32(-2) / np.float32(N) * np.float32(gout) * AS, g, bg)
    assert not R.accept(np.float32(-1) / np.float32(N) * np.float32(gout) * AS, g, bg)
    assert not R.accept(np.float32(-2) / np.float32(N) * AS, g, bg)       # grad_out ignored


# -------------------------------------------------------------------- classifier head
def _head_cases():
    for shape in R.HEAD_SHAPES:
        yield shape, False
    yield R.HEAD_SPREAD, True


@pytest.mark.parametrize("shape,spread", list(_head_cases()))
def test_head_ref_matches_torch_autograd(shape, spread):
    B, C, HW, K = shape
    c = R.head_input(B, C, HW, K, seed=C + K, spread=spread)
    lam, gs = 0.3, 2.0 ** 12
    x = c["x"].double().requires_grad_(True)
    w, b = c["w"].double().requires_grad_(True), c["b"].double().requires_grad_(True)
    pooled = F.adaptive_avg_pool2d(x, 1).flatten(1)
    z = F.linear(pooled, w, b)
    loss = R.f32(lam) * F.cross_entropy(z, c["y"].long())
    (loss * gs).backward()
    p, _ = R.pool_ref(c["x"].double(), False)
    zr, _ = R.fc_ref(p, c["w"], c["b"], False)
    lr, _, dz, _ = R.ce_ref(zr, c["y"], lam, gs)
    dw, _, db, _, dp, _ = R.cls_bwd_ref(dz, p, c["w"], False)
    dx, _ = R.pool_bwd_ref(dp, HW, "s3")
    close = lambda a, r: (a - r).abs().max() <= 1e-11 * max(float(r.abs().max()), 1e-300)
    assert close(p, pooled.detach()) and close(zr, z.detach()) and close(lr, loss.detach())
    assert close(dw, w.grad) and close(db, b.grad)
    assert close(dx[:, :, None, None].expand_as(x), x.grad)


@pytest.mark.parametrize("fmt", ["f16x3", "amp"])
@pytest.mark.parametrize("shape,spread", list(_head_cases()))
def test_head_checker_accepts_fp32_and_rejects_wrong_kernels(shape, spread, fmt):
    B, C, HW, K = shape
    amp = fmt == "amp"
    lay, glay = ("s1", "s1") if amp else ("s2", "s3")
    c = R.head_input(B, C, HW, K, seed=C + K, spread=spread)
    x = R.store(c["x"], lay)
    pooled = emu_pool(x, amp)
    ref, bound = R.pool_ref(x, amp)
    assert R.accept(pooled, ref, bound)
    if 32 * -(-HW // 32) != HW:
        assert not R.accept(emu_pool(x, amp, wrong_div=True), ref, bound)
    logits = emu_fc(pooled, c["w"], c["b"], amp)
    ref, bound = R.fc_ref(pooled.double(), c["w"], c["b"], amp)
    assert R.accept(logits, ref, bound)
    if spread:
        assert float(logits.abs().max()) > 5e3
    for lam in R.HEAD_LAM:
        for gs in R.head_gscales(fmt, spread):
            loss, dz = emu_ce(logits, c["y"], lam, gs)
            rl, bl, rdz, bdz = R.ce_ref(logits.double(), c["y"], lam, gs)
            assert R.accept(loss.reshape(1), rl.reshape(1), bl.reshape(1))
            assert R.accept(dz, rdz, bdz)
            live = bool((rdz != 0).any())
            if B > 1 and live:
                assert not R.accept(emu_ce(logits, c["y"], lam, gs, no_b=True)[1], rdz, bdz)
            if lam != 1.0 and live:
                assert not R.accept(emu_ce(logits, c["y"], lam, gs, no_lam=True)[1], rdz, bdz)
            if gs is not None and live:
                assert not R.accept(emu_ce(logits, c["y"], lam, gs, no_gs=True)[1], rdz, bdz)
            dw, db, dp = emu_cls_bwd(dz, pooled, c["w"], amp)
            assert torch.isfinite(dw).all() and torch.isfinite(dp).all()
            rw, bw, rb, bb, rp, bp = R.cls_bwd_ref(dz.double(), pooled.double(), c["w"], amp)
            assert R.accept(dw, rw, bw) and R.accept(db, rb, bb) and R.accept(dp, rp, bp)
            ro, bo = R.pool_bwd_ref(dp.double(), HW, glay)
            assert R.accept(emu_pool_bwd(dp, HW, glay), ro, bo)
    bad = c["y"].clone()
    bad[0] = K
    assert torch.isnan(emu_ce(logits, bad, 1.0, None)[0]) and torch.isnan(
        R.ce_ref(logits.double(), bad, 1.0, None)[0])
