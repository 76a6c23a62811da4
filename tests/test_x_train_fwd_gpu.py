"""Direct fp64 checks of the training forward, kernel by kernel through the C ABI: the BN
statistics and BN-ReLU in the three activation layouts, tcam_softmax2, tcam_chansum_nchw,
tcam_tcam_losses(_ex), tcam_crf_energy / tcam_crf_grad, the classifier head (tcam_cls_fwd,
tcam_ce_loss, tcam_cls_bwd, tcam_pool_bwd) and tcam_up2_bwd.  References, bounds, shapes and
input builders: tests/train_fwd_ref.py (pinned to torch, with their teeth, by
tests/test_train_fwd_ref.py).  Every operand is the value the device stored, every bound is
elementwise on the sum of magnitudes of the output's terms, every output is filled with NaN
before the call, and every call is made twice and compared bit for bit.

Measured on an MI355X, worst error / bound per output (the whole file runs in 5 s): BN
statistics mean 0.50, invstd 0.49, run_mean 0.49, run_var 0.49 in every layout; bn_relu S3
0.63, S2 0.75, S1 1.00; softmax2 0.80; chansum 0 (the nearly cancelling sums are
representable in fp32); tcam_losses total 0.38, sl 0.05, crf 0.56, size 0.23, dfcams 0.62;
crf energy 0.02, grad 0.33; up2_bwd S3 0.76, S1 1.00; head f16x3 pooled 0.17, logits 0.11,
loss 0.33, dlogits 0.49, dW 0.37, db 0.50, dpooled 0.30, dout 0.81; head AMP pooled 0.99,
logits 0.99, loss 0.36, dlogits 0.49, dW / db / dpooled / dout 1.00 (fp16's half ulp)."""
import numpy as np
import pytest
import torch

import train_fwd_ref as R
from tcam_wsol_video_amd import _lib, ops
from test_gpu_enc_train import _act, _nchw, _st

pytestmark = pytest.mark.gpu

NAN = float("nan")
FMT = {"s3": "x6", "s2": "f16x3", "s1": "amp"}


def _nan(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _nan_act(lay, B, H, W, C, dev):
    """An activation tensor whose every stored part is NaN."""
    t = ops.lay_empty(lay, B, H, W, C, dev)
    t.fill_(NAN)
    return t


def _twice(fn):
    """fn() -> tuple of fresh output tensors; run twice, bit-identical (NaN == NaN)."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        bits = torch.int16 if x.element_size() == 2 else torch.int32
        assert torch.equal(x.view(bits), y.view(bits)), "not deterministic"
    return a


def _report(tag, ratios):
    print(f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + " of the bound")
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------ BN
def _bn_stats(lay, ys, P, C, eps, rm, rv):
    lib = _lib.load()
    dev = ys.device
    ws = torch.empty(int(lib.tcam_bn_ws_bytes(P, C)), dtype=torch.uint8, device=dev)
    mean, invstd = _nan(dev, C), _nan(dev, C)
    rm = rm.clone() if rm is not None else None
    rv = rv.clone() if rv is not None else None
    rc = getattr(lib, f"tcam_bn_stats_{lay}")(
        ys.data_ptr(), P, C, eps, R.BN_MOMENTUM, mean.data_ptr(), invstd.data_ptr(),
        rm.data_ptr() if rm is not None else None, rv.data_ptr() if rv is not None else None,
        ws.data_ptr(), _st())
    assert rc == 0
    return (mean, invstd) + ((rm, rv) if rm is not None else ())


@pytest.mark.parametrize("eps", R.BN_EPS)
@pytest.mark.parametrize("lay", ["s3", "s2", "s1"])
@pytest.mark.parametrize("C,bhw", R.BN_SHAPES)
def test_bn_stats_match_fp64(cuda, C, bhw, lay, eps):
    """tcam_bn_stats_{s3,s2,s1}: mean, invstd, run_mean, run_var against the two-pass fp64
    statistics of the stored y (train_fwd_ref.bn_stats_ref's bounds; the path each shape
    reaches: train_fwd_ref.BN_SHAPES); run_mean = run_var = NULL gives the same mean / invstd
    bit for bit; the device's result for the other eps fails the checker (control)."""
    B, H, W = bhw
    P = B * H * W
    c = R.bn_input(C, B, H, W, seed=C + H)
    ys = _act(c["y"], cuda, FMT[lay])
    y64 = _nchw(ys)
    rm0, rv0 = c["run_mean"].to(cuda), c["run_var"].to(cuda)
    ref = R.bn_stats_ref(y64, eps, R.BN_MOMENTUM, c["run_mean"], c["run_var"])
    mean, invstd, rm, rv = _twice(lambda: _bn_stats(lay, ys, P, C, eps, rm0, rv0))
    got = dict(mean=mean, invstd=invstd, run_mean=rm, run_var=rv)
    _report(f"bn_stats_{lay} C{C} {B}x{H}x{W} eps {eps:g}",
            {k: R.ratio(got[k].cpu(), ref[k], ref["b_" + k]) for k in got})
    m2, i2 = _twice(lambda: _bn_stats(lay, ys, P, C, eps, None, None))
    assert torch.equal(m2, mean) and torch.equal(i2, invstd)
    other = _bn_stats(lay, ys, P, C, 1e-3 if eps == 1e-5 else 1e-5, None, None)[1]
    assert not R.accept(other.cpu(), ref["invstd"], ref["b_invstd"])


def _bn_relu(lay, ys, dims, mean, invstd, gamma, beta):
    B, H, W, C = dims
    out = _nan_act(lay, B, H, W, C, ys.device)
    assert getattr(_lib.load(), f"tcam_bn_relu_{lay}")(
        ys.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
        out.data_ptr(), B * H * W, C, _st()) == 0
    return (out,)


@pytest.mark.parametrize("lay", ["s3", "s2", "s1"])
@pytest.mark.parametrize("C,bhw", R.BN_SHAPES)
def test_bn_relu_matches_fp64(cuda, C, bhw, lay):
    """tcam_bn_relu_{s3,s2,s1} with the fp64 reference's mean / invstd rounded to fp32: gamma
    negative and exactly zero, a channel with every pixel masked (beta -50) and one with none
    (+50); on S3 and S1 one NaN pixel must come out NaN (torch's relu)."""
    B, H, W = bhw
    c = R.bn_input(C, B, H, W, seed=C + H + 1)
    y = c["y"].clone()
    nan_at = (B - 1, 9 % C, H // 2, W // 3)
    if lay != "s2":
        y[nan_at] = NAN
    ys = _act(y, cuda, FMT[lay])
    y64 = _nchw(ys)
    st = R.bn_stats_ref(_nchw(_act(c["y"], cuda, FMT[lay])), 1e-5, R.BN_MOMENTUM)
    mean, invstd = st["mean"].float(), st["invstd"].float()
    dev = [t.to(cuda).contiguous() for t in (mean, invstd, c["gamma"], c["beta"])]
    (out,) = _twice(lambda: _bn_relu(lay, ys, (B, H, W, C), *dev))
    got = _nchw(out)
    ref, bound = R.bn_relu_ref(y64, mean, invstd, c["gamma"], c["beta"], lay)
    if lay != "s2":
        assert torch.isnan(ref[nan_at]) and torch.isnan(got[nan_at])
        assert int(torch.isnan(got).sum()) == 1
        got[nan_at] = ref[nan_at] = 0.0
    assert (got[:, R.DEAD_CH] == 0).all() and (got[:, R.LIVE_CH] > 0).all()
    _report(f"bn_relu_{lay} C{C} {B}x{H}x{W}", {"out": R.ratio(got, ref, bound)})


# ------------------------------------------------ softmax, channel sums, up2 bwd, CRF
def _softmax(f):
    B, _, HW = f.shape
    S = _nan(f.device, B, 2, HW)
    assert _lib.load().tcam_softmax2(f.data_ptr(), S.data_ptr(), B, HW, _st()) == 0
    return (S,)


@pytest.mark.parametrize("B,HW", R.SOFTMAX_SHAPES)
def test_softmax2_matches_fp64(cuda, B, HW):
    f = R.softmax_input(B, HW, seed=HW)
    fd = f.to(cuda)
    (S,) = _twice(lambda: _softmax(fd))
    ref, bound = R.softmax2_ref(f.double())
    _report(f"softmax2 {B}x{HW}", {"S": R.ratio(S.cpu(), ref, bound)})
    same = f[:, 0] == f[:, 1]
    assert (S.cpu()[:, 0][same] == 0.5).all()


@pytest.mark.parametrize("B,C,HW", R.CHANSUM_SHAPES)
def test_chansum_matches_fp64(cuda, B, C, HW):
    lib = _lib.load()
    x = R.chansum_input(B, C, HW, seed=HW)
    xd = x.to(cuda)
    ws = torch.empty(int(lib.tcam_chansum_ws_bytes(B, C, HW)), dtype=torch.uint8, device=cuda)

    def run():
        out = _nan(cuda, C)
        assert lib.tcam_chansum_nchw(xd.data_ptr(), B, C, HW, out.data_ptr(), ws.data_ptr(),
                                     _st()) == 0
        return (out,)
    (out,) = _twice(run)
    ref, bound = R.chansum_ref(x.double())
    _report(f"chansum {B}x{C}x{HW}", {"sum": R.ratio(out.cpu(), ref, bound)})


@pytest.mark.parametrize("lay", ["s3", "s1"])
@pytest.mark.parametrize("B,C,H,W", R.UP2_SHAPES)
def test_up2_bwd_matches_fp64(cuda, B, C, H, W, lay):
    g = torch.Generator().manual_seed(C + H)
    gus = _act(torch.randn(B, C, 2 * H, 2 * W, generator=g), cuda, FMT[lay])

    def run():
        gx = _nan_act(lay, B, H, W, C, cuda)
        assert getattr(_lib.load(), f"tcam_up2_bwd_{lay}")(gus.data_ptr(), gx.data_ptr(), B, C, H,
                                                           W, _st()) == 0
        return (gx,)
    (gx,) = _twice(run)
    ref, bound = R.up2_bwd_ref(_nchw(gus), lay)
    _report(f"up2_bwd_{lay} {B}x{C}x{H}x{W}", {"gx": R.ratio(_nchw(gx), ref, bound)})


@pytest.mark.parametrize("N,K,H,W", R.CRF_SHAPES)
def test_crf_energy_and_grad_match_fp64(cuda, N, K, H, W):
    """tcam_crf_energy (one and two terms per thread of the fp32 tree) and tcam_crf_grad with
    grad_out != 1."""
    lib = _lib.load()
    seg, AS = R.crf_input(N, K, H, W, seed=H)
    sd, ad = seg.to(cuda), AS.to(cuda)
    gout = torch.tensor([0.37], device=cuda)
    ws = torch.empty(int(lib.tcam_crf_energy_ws_bytes()) // 4, device=cuda)

    def run():
        e, g = _nan(cuda, 1), _nan(cuda, N, K, H, W)
        assert lib.tcam_crf_energy(sd.data_ptr(), ad.data_ptr(), sd.numel(), N, e.data_ptr(),
                                   ws.data_ptr(), _st()) == 0
        assert lib.tcam_crf_grad(ad.data_ptr(), gout.data_ptr(), ad.numel(), N, g.data_ptr(),
                                 _st()) == 0
        return e, g
    e, g = _twice(run)
    re, be = R.crf_energy_ref(seg.double(), AS.double(), N)
    rg, bg = R.crf_grad_ref(AS.double(), gout.cpu()[0], N)
    _report(f"crf {N}x{K}x{H}x{W}", {"energy": R.ratio(e.cpu(), re.reshape(1), be.reshape(1)),
                                     "grad": R.ratio(g.cpu(), rg, bg)})


# ----------------------------------------------------------------------- TCAM losses
def _losses(fd, Sd, seeds, AS, gx, extra, lam, t):
    lib = _lib.load()
    B, _, HW = fd.shape
    dev = fd.device
    ws = torch.empty(int(lib.tcam_tcam_loss_ws_bytes(B, HW)), dtype=torch.uint8, device=dev)
    losses, dF = _nan(dev, 5), _nan(dev, B, 2, HW)
    p = lambda v: v.data_ptr() if v is not None else None
    if gx is None:
        rc = lib.tcam_tcam_losses(fd.data_ptr(), Sd.data_ptr(), p(seeds), p(AS), B, HW, *lam, t,
                                  losses.data_ptr(), dF.data_ptr(), ws.data_ptr(), _st())
    else:
        rc = lib.tcam_tcam_losses_ex(fd.data_ptr(), Sd.data_ptr(), p(seeds), p(AS), p(gx),
                                     p(extra), B, HW, *lam, t, losses.data_ptr(), dF.data_ptr(),
                                     ws.data_ptr(), _st())
    assert rc == 0
    return losses, dF


def _loss_ratios(losses, dF, ref, five):
    n = 5 if five else 4
    lo = losses.cpu()
    assert five or torch.isnan(lo[4])          # the four-term entry leaves losses[4] alone
    out = {k: R.ratio(lo[i:i + 1], ref["losses"][i:i + 1], ref["bounds"][i:i + 1])
           for i, k in enumerate(("total", "sl", "crf", "size", "extra")[:n])}
    out["dF"] = R.ratio(dF.cpu(), ref["dF"], ref["b_dF"])
    return out


@pytest.mark.parametrize("t", R.LOSS_T)
@pytest.mark.parametrize("B,HW", R.LOSS_SHAPES)
def test_tcam_losses_match_fp64(cuda, B, HW, t):
    """tcam_tcam_losses / _ex: each term alone, all three with lambdas of one order, the
    defaults, and the five-term entry; every loss value and every element of dfcams.  HW <=
    4096 one chunk, 4097 and 50176 several (kLossPix); B = 257 the second pass of
    loss_finalize_kernel's frame loop (kFinBlock); both ELB branches and t != 1 (the inputs'
    conditions: tests/test_train_fwd_ref.py)."""
    c = R.loss_input(B, HW, seed=R.loss_seed(B, HW))
    d = {k: v.to(cuda) for k, v in c.items()}
    (Sd,) = _twice(lambda: _softmax(d["f"]))
    S = Sd.cpu()
    on_dev = lambda v: None if v is None else [x for k, x in d.items() if c[k] is v][0]
    for name, seeds, AS, gx, extra, lam in R.loss_runs(c):
        args = (d["f"], Sd, on_dev(seeds), on_dev(AS), on_dev(gx), on_dev(extra), lam, t)
        losses, dF = _twice(lambda: _losses(*args))
        ref = R.tcam_loss_ref(c["f"], S, seeds, AS, gx, extra, lam, t)
        _report(f"tcam_losses {B}x{HW} t {t:g} {name}",
                _loss_ratios(losses, dF, ref, extra is not None))


@pytest.mark.parametrize("ex", [False, True])
def test_tcam_losses_without_a_valid_seed_are_nan(cuda, ex):
    """Seeds given, lam_sl != 0, no seed 0 or 1 in the whole batch: sl and the total are NaN
    (nn.CrossEntropyLoss's mean over no element; the reference then skips the step), the other
    terms and dfcams (= the gradient without the CE term) keep their bounds.  lam_sl = 0, or
    one valid seed anywhere in the batch, stays finite."""
    B, HW = 3, 40
    c = R.loss_input(B, HW, seed=11)
    d = {k: v.to(cuda) for k, v in c.items()}
    (Sd,) = _softmax(d["f"])
    S = Sd.cpu()
    none = torch.full_like(c["seeds"], R.IGNORE)
    gx, extra, gxd, exd = (c["gx"], c["extra"], d["gx"], d["extra"]) if ex else (None,) * 4
    losses, dF = _twice(lambda: _losses(d["f"], Sd, none.to(cuda), d["AS"], gxd, exd, R.LAM_ALL,
                                        1.0))
    lo = losses.cpu()
    assert torch.isnan(lo[0]) and torch.isnan(lo[1])
    ref = R.tcam_loss_ref(c["f"], S, None, c["AS"], gx, extra, R.LAM_ALL, 1.0)
    r = {k: R.ratio(lo[i:i + 1], ref["losses"][i:i + 1], ref["bounds"][i:i + 1])
         for i, k in ((2, "crf"), (3, "size")) + (((4, "extra"),) if ex else ())}
    r["dF"] = R.ratio(dF.cpu(), ref["dF"], ref["b_dF"])
    _report(f"tcam_losses no valid seed ex={int(ex)}", r)
    # lam_sl = 0 with the same seeds; and one valid seed in one frame
    lam0 = (0.0,) + R.LAM_ALL[1:]
    losses, dF = _losses(d["f"], Sd, none.to(cuda), d["AS"], gxd, exd, lam0, 1.0)
    ref = R.tcam_loss_ref(c["f"], S, none, c["AS"], gx, extra, lam0, 1.0)
    assert float(losses[1]) == 0.0
    _report("tcam_losses no valid seed, lam_sl 0", _loss_ratios(losses, dF, ref, ex))
    one = none.clone()
    one[1, 7] = 1
    losses, dF = _losses(d["f"], Sd, one.to(cuda), d["AS"], gxd, exd, R.LAM_ALL, 1.0)
    ref = R.tcam_loss_ref(c["f"], S, one, c["AS"], gx, extra, R.LAM_ALL, 1.0)
    _report("tcam_losses one valid seed", _loss_ratios(losses, dF, ref, ex))


def test_decoder_step_without_a_valid_seed_is_skipped(cuda):
    """One DecoderTrainer.step on a batch whose seeds are all ignored: the total is NaN, the
    gated SGD leaves parameters and momentum bit-identical and counts a skipped step — what the
    reference's isfinite(loss) check does; the next batch, with seeds, is applied."""
    from tcam_wsol_video_amd.models import build_r50_tcam
    from tcam_wsol_video_amd.training import DecoderTrainer
    from test_gpu_train import _batch
    model = build_r50_tcam(seed=21).to(cuda)
    tr = DecoderTrainer(model, lr=0.01)
    x, raw, seeds = _batch(2, 64, seed=5)
    tr.step(x.to(cuda), raw.to(cuda), seeds.to(cuda))      # a first step: momentum is non-zero
    torch.cuda.synchronize()
    assert tr.applied_steps == 1 and tr.skipped_steps == 0 and bool((tr.mom != 0).any())
    p0, m0 = tr.flat.clone(), tr.mom.clone()
    losses = tr.step(x.to(cuda), raw.to(cuda), torch.full_like(seeds, R.IGNORE).to(cuda)).cpu()
    torch.cuda.synchronize()
    assert torch.isnan(losses[0]) and torch.isnan(losses[1]) and torch.isfinite(losses[2:]).all()
    assert torch.equal(tr.flat, p0) and torch.equal(tr.mom, m0)
    assert tr.applied_steps == 1 and tr.skipped_steps == 1
    some = torch.full_like(seeds, R.IGNORE)
    some[1] = seeds[1]                  # frame 0 all ignored, frame 1 with seeds: a normal step
    losses = tr.step(x.to(cuda), raw.to(cuda), some.to(cuda)).cpu()
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and not torch.equal(tr.flat, p0)
    assert tr.applied_steps == 2 and tr.skipped_steps == 1


# -------------------------------------------------------------------- classifier head
def _head_cases():
    for shape in R.HEAD_SHAPES:
        yield shape, False
    yield R.HEAD_SPREAD, True


def _cls_fwd(lay, xs, B, HW, C, K, wd, bd):
    lib = _lib.load()
    dev = xs.device
    pooled, logits = _nan(dev, B, C), _nan(dev, B, K)
    ws = torch.empty(int(lib.tcam_cls_pool_ws_bytes(B, C)), dtype=torch.uint8, device=dev)
    assert getattr(lib, f"tcam_cls_fwd_{lay}")(xs.data_ptr(), B, HW, C, wd.data_ptr(),
                                               bd.data_ptr(), K, pooled.data_ptr(),
                                               logits.data_ptr(), ws.data_ptr(), _st()) == 0
    return pooled, logits


def _ce(logits, yd, lam, gs):
    B, K = logits.shape
    loss, dz = _nan(logits.device, 1), _nan(logits.device, B, K)
    gsd = torch.tensor([gs], device=logits.device) if gs is not None else None
    assert _lib.load().tcam_ce_loss(logits.data_ptr(), yd.data_ptr(), B, K, lam,
                                    gsd.data_ptr() if gs is not None else None, loss.data_ptr(),
                                    dz.data_ptr(), _st()) == 0
    torch.cuda.synchronize()      # gsd lives until the kernel has read it
    return loss, dz


def _cls_bwd(dz, pooled, wd, amp):
    B, K = dz.shape
    C = pooled.shape[1]
    dev = dz.device
    dw, db, dp = _nan(dev, K, C), _nan(dev, K), _nan(dev, B, C)
    rc = _lib.load().tcam_cls_bwd(dz.data_ptr(), pooled.data_ptr(), wd.data_ptr(), B, K, C,
                                  int(amp), dw.data_ptr(), db.data_ptr(), dp.data_ptr(), _st())
    return rc, dw, db, dp


@pytest.mark.parametrize("fmt", ["f16x3", "amp"])
@pytest.mark.parametrize("shape,spread", list(_head_cases()))
def test_cls_head_matches_fp64_elementwise(cuda, shape, spread, fmt):
    """tcam_cls_fwd_{s2,s1}, tcam_ce_loss, tcam_cls_bwd, tcam_pool_bwd_{s3,s1}: pooled, logits,
    loss, dlogits, dW, db, dpooled and dout elementwise, each stage on the device's own previous
    stage, lam 1 and 0.3, gscale NULL and the format's loss scale (the paths of the shapes:
    train_fwd_ref.HEAD_SHAPES)."""
    B, C, HW, K = shape
    amp = fmt == "amp"
    lay, glay = ("s1", "s1") if amp else ("s2", "s3")
    c = R.head_input(B, C, HW, K, seed=C + K, spread=spread)
    xs = _act(c["x"], cuda, fmt)
    wd, bd, yd = c["w"].to(cuda), c["b"].to(cuda), c["y"].to(cuda)
    tag = f"head {fmt} {B}x{C}x{HW}x{K}{' spread' if spread else ''}"
    pooled, logits = _twice(lambda: _cls_fwd(lay, xs, B, HW, C, K, wd, bd))
    rp, bp = R.pool_ref(_nchw(xs), amp)
    rz, bz = R.fc_ref(pooled.cpu().double(), c["w"], c["b"], amp)
    _report(tag, {"pooled": R.ratio(pooled.cpu(), rp, bp), "logits": R.ratio(logits.cpu(), rz, bz)})
    if spread:
        assert float(logits.abs().max()) > 5e3
    for lam in R.HEAD_LAM:
        for gs in R.head_gscales(fmt, spread):
            loss, dz = _twice(lambda: _ce(logits, yd, lam, gs))
            rl, bl, rdz, bdz = R.ce_ref(logits.cpu().double(), c["y"], lam, gs)
            rc, dw, db, dp = _cls_bwd(dz, pooled, wd, amp)
            assert rc == 0
            _twice(lambda: _cls_bwd(dz, pooled, wd, amp)[1:])
            rw, bw, rb, bb, rdp, bdp = R.cls_bwd_ref(dz.cpu().double(), pooled.cpu().double(),
                                                     c["w"], amp)

            def pool_bwd():
                dout = _nan_act(glay, B, HW, 1, C, cuda)
                assert getattr(_lib.load(), f"tcam_pool_bwd_{glay}")(
                    dp.data_ptr(), B, HW, C, dout.data_ptr(), _st()) == 0
                return (dout,)
            (dout,) = _twice(pool_bwd)
            ro, bo = R.pool_bwd_ref(dp.cpu().double(), HW, glay)
            ro = ro[:, :, None, None].expand(B, C, HW, 1)
            bo = bo[:, :, None, None].expand(B, C, HW, 1)
            _report(f"{tag} lam {lam:g} gscale {gs}", {
                "loss": R.ratio(loss.cpu(), rl.reshape(1), bl.reshape(1)),
                "dlogits": R.ratio(dz.cpu(), rdz, bdz), "dW": R.ratio(dw.cpu(), rw, bw),
                "db": R.ratio(db.cpu(), rb, bb), "dpooled": R.ratio(dp.cpu(), rdp, bdp),
                "dout": R.ratio(_nchw(dout), ro, bo)})


def test_cls_bwd_refuses_more_than_256_classes(cuda):
    """K = 257: TCAM_E_ARG before any launch, the NaN-filled outputs untouched."""
    B, K, C = 2, 257, 16
    dz, pooled, w = (torch.randn(s, device=cuda) for s in ((B, K), (B, C), (K, C)))
    rc, dw, db, dp = _cls_bwd(dz, pooled, w, False)
    torch.cuda.synchronize()
    assert rc == -1      # TCAM_E_ARG
    assert torch.isnan(dw).all() and torch.isnan(db).all() and torch.isnan(dp).all()


@pytest.mark.parametrize("bad", [-1, "K"])
def test_ce_loss_of_a_label_out_of_range_is_nan(cuda, bad):
    B, K = 5, 7
    z = torch.randn(B, K, device=cuda)
    y = torch.arange(B, dtype=torch.int32)
    y[3] = K if bad == "K" else bad
    loss, _ = _twice(lambda: _ce(z, y.to(cuda), 1.0, None))
    assert torch.isnan(loss).all()
    assert torch.isnan(R.ce_ref(z.cpu().double(), y, 1.0, None)[0])
