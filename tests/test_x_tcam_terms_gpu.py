"""tcam_tcam_losses_terms (the fg-size, bg > fg and empty-outside-box TCAM terms) and
tcam_teacher_stats on the device, through the C ABI, against tests/tcam_terms_ref.py (pinned to
the reference's classes by tests/test_tcam_terms_ref.py); then the terms through MasterLoss,
DecoderTrainer.step and main.py.  Every output is filled with NaN before the call, every call
is made twice and compared bit for bit, every loss slot and every element of dfcams must lie
within the fp64 reference's bound; no case is skipped (the CPU test asserts that no barrier
argument sits within its own error of a breakpoint).

Without the feature the C-ABI tests fail on the missing symbols (AttributeError in _lib.load)
and the MasterLoss / trainer / main.py tests on MasterLoss.add's NotImplementedError, the
unknown DecoderTrainer arguments and the unknown flags.

Measured on an MI355X (the whole file runs in 10 s), worst error / bound over LOSS_SHAPES x
t in {1, 2.5, 10, (2.5, 10, 1)} x the five runs: total 0.28, sl 0.05, crf 0.68, size 0.18, bgfg
0.20, fgsz 0.12, eob 0.12, dfcams 0.42; tcam_teacher_stats: mask exact, fg_size 0.34.  With the
terms off every loss_runs case is bit-equal to tcam_tcam_losses_ex."""
import os

import numpy as np
import pytest
import torch

import tcam_terms_ref as T
import train_fwd_ref as R
from tcam_wsol_video_amd import _lib
from test_gpu_enc_train import _st

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = os.path.join(os.path.dirname(__file__), "golden", "tcam_terms.npz")


def _nan(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "not deterministic"
    return a


def _softmax(fd):
    B, _, HW = fd.shape
    S = _nan(fd.device, B, 2, HW)
    assert _lib.load().tcam_softmax2(fd.data_ptr(), S.data_ptr(), B, HW, _st()) == 0
    return S


def _terms(fd, Sd, seeds, AS, gx, extra, lam, t, fs, msk, lam3, t3, eps):
    lib = _lib.load()
    B, _, HW = fd.shape
    dev = fd.device
    ws = torch.empty(int(lib.tcam_tcam_loss_terms_ws_bytes(B, HW)), dtype=torch.uint8,
                     device=dev)
    losses, dF = _nan(dev, 8), _nan(dev, B, 2, HW)
    p = lambda v: v.data_ptr() if v is not None else None
    rc = lib.tcam_tcam_losses_terms(fd.data_ptr(), Sd.data_ptr(), p(seeds), p(AS), p(gx),
                                    p(extra), p(fs), p(msk), B, HW, *lam, t, *lam3, *t3, eps,
                                    losses.data_ptr(), dF.data_ptr(), ws.data_ptr(), _st())
    assert rc == 0
    return losses, dF


WORST = {}


def _report(tag, ratios):
    print(f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + " of the bound")
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("t3", T.t_cases(), ids=lambda t: "t" + "-".join(f"{v:g}" for v in t))
@pytest.mark.parametrize("B,HW", R.LOSS_SHAPES)
def test_terms_match_fp64(cuda, B, HW, t3):
    """Each new term alone, the three together, and all seven slots with seeds, AS and the
    extra term.  (1, 1) one thread; 4095 / 4097 either side of a kLossPix chunk; (257, 5) the
    second pass of the 256-wide finalize; 50176 many chunks; t = 1, 2.5, 10 and a different t
    per term; the inputs take every ELB branch of every term (tests/test_tcam_terms_ref.py)."""
    c = T.terms_input(B, HW, seed=R.loss_seed(B, HW))
    d = {k: v.to(cuda) for k, v in c.items()}
    (Sd,) = _twice(lambda: (_softmax(d["f"]),))
    S = Sd.cpu()
    on_dev = lambda v: None if v is None else [x for k, x in d.items() if c[k] is v][0]
    t = R.LOSS_T[1]
    for run in T.terms_runs(c):
        name, seeds, AS, gx, extra, lam, fs, msk, lam3 = run
        args = (d["f"], Sd, on_dev(seeds), on_dev(AS), on_dev(gx), on_dev(extra), lam, t,
                on_dev(fs), on_dev(msk), lam3, t3, T.EPS)
        losses, dF = _twice(lambda: _terms(*args))
        ref = T.terms_ref(c["f"], S, seeds, AS, gx, extra, lam, t, fs, msk, lam3, t3, T.EPS)
        lo = losses.cpu()
        r = {k: R.ratio(lo[i:i + 1], ref["losses"][i:i + 1], ref["bounds"][i:i + 1])
             for i, k in enumerate(("total", "sl", "crf", "size", "extra", "bgfg", "fgsz", "eob"))}
        r["dF"] = R.ratio(dF.cpu(), ref["dF"], ref["b_dF"])
        _report(f"tcam_losses_terms {B}x{HW} t {t3} {name}", r)
    print("worst so far:", {k: round(v, 3) for k, v in WORST.items()})


@pytest.mark.parametrize("t", R.LOSS_T)
@pytest.mark.parametrize("B,HW", R.LOSS_SHAPES)
def test_terms_off_equals_ex_bit_for_bit(cuda, B, HW, t):
    """With the three terms off (zero lambdas, NULL fg_size / msk — and also with inputs given
    but zero lambdas) losses[0:4|5] and dfcams hold tcam_tcam_losses_ex's bits on every
    loss_runs case."""
    lib = _lib.load()
    c = T.terms_input(B, HW, seed=R.loss_seed(B, HW))
    d = {k: v.to(cuda) for k, v in c.items()}
    Sd = _softmax(d["f"])
    on_dev = lambda v: None if v is None else [x for k, x in d.items() if c[k] is v][0]
    p = lambda v: v.data_ptr() if v is not None else None
    bits = lambda v: v.view(torch.int32)
    for name, seeds, AS, gx, extra, lam in R.loss_runs(c):
        a = [on_dev(v) for v in (seeds, AS, gx, extra)]
        ws = torch.empty(int(lib.tcam_tcam_loss_ws_bytes(B, HW)), dtype=torch.uint8, device=cuda)
        lo0, dF0 = _nan(cuda, 5), _nan(cuda, B, 2, HW)
        assert lib.tcam_tcam_losses_ex(d["f"].data_ptr(), Sd.data_ptr(), *(p(v) for v in a), B,
                                       HW, *lam, t, lo0.data_ptr(), dF0.data_ptr(),
                                       ws.data_ptr(), _st()) == 0
        n = 5 if extra is not None else 4
        for fs, msk in ((None, None), (d["fg_size"], d["msk"])):
            lo1, dF1 = _terms(d["f"], Sd, *a, lam, t, fs, msk, (0.0, 0.0, 0.0), (1.0, 2.5, 10.0),
                              T.EPS)
            torch.cuda.synchronize()
            assert torch.equal(bits(lo0[:n]), bits(lo1[:n])), (name, lo0, lo1)
            assert torch.equal(bits(dF0), bits(dF1)), name
            assert lo1[5:].tolist() == [0.0, 0.0, 0.0]


def test_nan_fg_size_gives_nan_total_and_finite_gradient(cuda):
    B, HW = 3, 40
    c = T.terms_input(B, HW, seed=3)
    d = {k: v.to(cuda) for k, v in c.items()}
    Sd = _softmax(d["f"])
    fs = d["fg_size"].clone()
    fs[1] = NAN
    lo, dF = _terms(d["f"], Sd, None, None, None, None, (0.0, 0.0, 0.2), 1.0, fs, d["msk"],
                    T.LAM3, T.T_MIXED, T.EPS)
    assert torch.isnan(lo[0]) and torch.isnan(lo[6]) and torch.isfinite(lo[[3, 5, 7]]).all()
    assert torch.isfinite(dF).all()


@pytest.mark.parametrize("B,H,W", T.STATS_SHAPES)
def test_teacher_stats_match(cuda, B, H, W):
    """tcam_teacher_stats: the box mask exactly, fg_size within 2 2^-24 sum |cam roi| / (HW) of
    fp64; a box touching every border (frame 0) and an empty box (the last frame)."""
    from tcam_wsol_video_amd.training import teacher_stats
    cams, roi, bbox = T.stats_input(B, H, W, seed=B + H)
    msk_ref, fg_ref, bound = T.stats_ref(cams, roi, bbox)

    def run():
        return teacher_stats(cams.to(cuda), roi.to(cuda), bbox.to(cuda))

    msk, fg = _twice(run)
    assert msk.shape == (B, 1, H, W) and torch.equal(msk.cpu(), msk_ref)
    _report(f"teacher_stats {B}x{H}x{W}", {"fg_size": R.ratio(fg.cpu(), fg_ref, bound)})


def test_teacher_stats_follow_get_roi(cuda):
    """On tcam_get_roi's own outputs: the mask is GetRoiSingleCam.__call__'s box mask."""
    from tcam_wsol_video_amd.seeding import GetRoiSingleCam
    from tcam_wsol_video_amd.training import teacher_stats
    g = torch.Generator().manual_seed(5)
    cams = torch.rand(2, 24, 20, generator=g) * 0.2
    cams[0, 4:15, 3:9] += 0.7
    cams[1, 10:20, 8:19] += 0.6
    getter = GetRoiSingleCam("largest", 0.05)
    roi, bbox, _ = getter.batch(cams.to(cuda))
    msk, fg = teacher_stats(cams.to(cuda), roi, bbox)
    for b in range(2):
        r1, m1, _ = getter(cams[b].to(cuda))
        assert torch.equal(msk[b, 0], m1) and float(m1.sum()) > 0
        want = float((cams[b].double() * r1.cpu().double()).sum() / (24 * 20))
        assert abs(float(fg[b]) - want) <= 2 * R.U * want


# ------------------------------------------------------------------------ MasterLoss
def _master(gold, dev):
    from tcam_wsol_video_amd import losses as L

    def elb(k):
        e = L.ELB(init_t=1.0, max_t=10.1)
        e.set_t(float(gold[f"t_{k}"]))
        return e

    lam = {k: float(gold[f"lam_{k}"]) for k in ("crf", "rgb", "size", "fgsz", "bgfg", "eob", "sl")}
    fg = L.FgSizeTcams(lambda_=lam["fgsz"], elb=elb("fgsz"))
    fg.set_eps(float(gold["eps"]))
    m = L.MasterLoss()
    for x in (L.ConRanFieldTcams(lambda_=lam["crf"], sigma_rgb=15., sigma_xy=100., scale_factor=1.),
              L.RgbJointConRanFieldTcams(lambda_=lam["rgb"], sigma_rgb=15., scale_factor=1.),
              L.MaxSizePositiveTcams(lambda_=lam["size"], elb=elb("size")), fg,
              L.BgSizeGreatSizeFgTcams(lambda_=lam["bgfg"], elb=elb("bgfg")),
              L.EmptyOutsideBboxTcams(lambda_=lam["eob"], elb=elb("eob")),
              L.SelfLearningTcams(lambda_=lam["sl"])):
        m.add(x)
    return m


def test_master_loss_seven_terms_match_the_reference(cuda):
    """All seven terms of get_loss_tcam through MasterLoss at 2 x 2 x 16 x 16 against the
    reference's values and autograd gradient; the tolerances of
    test_gpu_train.test_loss_kernel_matches_reference_goldens."""
    gold = np.load(G)
    m = _master(gold, cuda)
    t = lambda k: torch.from_numpy(gold[k]).to(cuda)
    f = t("fcams").requires_grad_(True)
    kw = dict(fcams=f, raw_img=t("raw").float(), seeds=t("seeds"), seq_iter=t("seq"),
              frm_iter=t("frm"), fg_size=t("fg_size"), msk_bbox=t("msk"))
    total = m(epoch=0, **kw)
    total.sum().backward()
    assert m.n_holder[1:] == ["con_ran_field_tcams", "rgb_joint_con_ran_field_tcams",
                              "max_size_positive_tcams", "fg_size_tcams",
                              "bg_size_great_size_fg_tcams", "empty_outside_bbox_tcams",
                              "self_learning_tcams"]
    got = [float(v.detach()) for v in m.l_holder]
    for k, a, ref in zip(["total"] + m.n_holder[1:], got,
                         [float(gold["seven_total"])] + gold["seven_terms"].tolist()):
        print(k, a, ref)
        assert abs(a - ref) <= 1e-5 * max(abs(ref), 1e-3), (k, a, ref)
    g = gold["seven_grad"]
    assert np.abs(f.grad.cpu().numpy() - g).max() <= 1e-5 * np.abs(g).max()
    # a missing or mis-shaped input of an active term
    for bad in (dict(fg_size=None), dict(fg_size=t("fg_size")[:1]), dict(msk_bbox=None),
                dict(msk_bbox=t("msk")[:, 0]), dict(msk_bbox=t("msk")[:, :, :8])):
        with pytest.raises(ValueError):
            m(epoch=0, **{**kw, **bad})


# --------------------------------------------------------------------------- trainer
def _trainer(cuda, **kw):
    from tcam_wsol_video_amd.models import build_r50_tcam
    from tcam_wsol_video_amd.training import DecoderTrainer
    return DecoderTrainer(build_r50_tcam(seed=21).to(cuda), lr=0.01, **kw)


def _teacher_inputs(n, size, cuda):
    g = torch.Generator().manual_seed(8)
    fs = (torch.rand(n, generator=g) * 0.5 + 0.1).to(cuda)
    msk = torch.zeros(n, 1, size, size)
    msk[:, :, size // 4:size // 2, size // 8:size // 2] = 1.0
    return fs, msk.to(cuda)


THREE = dict(use_bgfg=True, bgfg_lambda=0.5, use_fgsz=True, fgsz_lambda=0.8, fgsz_eps=0.003,
             use_eob=True, eob_lambda=0.3)


def test_decoder_step_with_the_three_terms(cuda):
    """One step at the trainer tests' smallest batch with the three terms on: 7 slots (total,
    sl, crf, size, bg > fg, fg size, empty outside), each equal to the fused entry's value on
    the step's own fcams; outside its window a configured term keeps a zero slot; a NaN
    fg_size leaves parameters and momentum bit-identical and counts a skipped step."""
    from test_gpu_train import _batch
    from tcam_wsol_video_amd.training import tcam_losses
    x, raw, seeds = (v.to(cuda) for v in _batch(2, 64, seed=5))
    fs, msk = _teacher_inputs(2, 64, cuda)
    tr = _trainer(cuda, windows={"eob": (2, -1)}, **THREE)
    assert tr.loss_names()[4:] == ["bg_size_great_size_fg_tcams", "fg_size_tcams",
                                   "empty_outside_bbox_tcams"]
    for e, t in zip(("bgfg", "fgsz", "eob"), (2.5, 10.0, 1.25)):
        tr.term_elbs[e].set_t(t)
    tr.set_epoch(1)
    _, fcams, _ = _trainer(cuda).forward(x)          # the same seeded model: the step's fcams
    want, _ = tcam_losses(fcams, raw, seeds, tr.lam, tr.elb.t, tr.sigma,
                          terms={"bgfg": (0.5, 2.5), "fgsz": (0.8, 10.0, 0.003, fs)})
    lo = tr.step(x, raw, seeds, fg_size=fs, msk_bbox=None).cpu()    # eob is off: no mask needed
    torch.cuda.synchronize()
    assert lo.shape == (7,) and torch.isfinite(lo).all() and float(lo[6]) == 0.0
    assert torch.allclose(lo[:6], want.cpu(), rtol=1e-5, atol=1e-7), (lo, want)
    assert float(lo[4]) != 0.0 and float(lo[5]) != 0.0
    assert tr.applied_steps == 1 and tr.skipped_steps == 0
    tr.set_epoch(2)
    with pytest.raises(ValueError):
        tr.step(x, raw, seeds, fg_size=fs, msk_bbox=None)
    lo = tr.step(x, raw, seeds, fg_size=fs, msk_bbox=msk).cpu()
    assert lo.shape == (7,) and torch.isfinite(lo).all() and float(lo[6]) != 0.0
    torch.cuda.synchronize()
    assert tr.applied_steps == 2
    p0, m0 = tr.flat.clone(), tr.mom.clone()
    bad = fs.clone()
    bad[1] = NAN
    lo = tr.step(x, raw, seeds, fg_size=bad, msk_bbox=msk).cpu()
    torch.cuda.synchronize()
    assert torch.isnan(lo[0]) and torch.isnan(lo[5])
    assert tr.skipped_steps == 1 and tr.applied_steps == 2
    assert torch.equal(tr.flat.view(torch.int32), p0.view(torch.int32))
    assert torch.equal(tr.mom.view(torch.int32), m0.view(torch.int32))


def test_decoder_step_amp_with_the_three_terms(cuda):
    """The AMP path (dF scale -> half) with the three terms.  The plane-sum barriers push every
    pixel the same way (lambda t / B each), so their weight gradients are far larger than the
    CE's: at the GradScaler's first scale 2^16 the step overflows fp16 and is skipped, as the
    reference's would be; small lambdas and a scale of 2^10 keep this one step inside fp16."""
    from test_gpu_train import _batch
    x, raw, seeds = (v.to(cuda) for v in _batch(2, 64, seed=5))
    fs, msk = _teacher_inputs(2, 64, cuda)
    tr = _trainer(cuda, amp=True, init_scale=2.0 ** 10,
                  **{**THREE, "bgfg_lambda": 1e-3, "eob_lambda": 1e-3})
    lo = tr.step(x, raw, seeds, fg_size=fs, msk_bbox=msk).cpu()
    torch.cuda.synchronize()
    assert lo.shape == (7,) and torch.isfinite(lo).all() and all(float(v) != 0 for v in lo[4:])
    assert (tr.applied_steps, tr.skipped_steps) == (1, 0) and float(tr.found_inf.item()) == 0.0


def test_decoder_step_without_new_terms_is_the_old_entry(cuda, monkeypatch):
    """No new term configured: the step calls tcam_tcam_losses_ex (never the new entry) and
    its losses and parameters are bit-identical to a step whose loss call is forced through
    the parent's code path (terms=None)."""
    from test_gpu_train import _batch
    from tcam_wsol_video_amd import training
    x, raw, seeds = (v.to(cuda) for v in _batch(2, 64, seed=5))
    called = []
    real = training.tcam_losses

    def spy(*a, **k):
        called.append(k.get("terms"))
        k["terms"] = None
        return real(*a, **k)

    lib = _lib.load()
    monkeypatch.setattr(lib, "tcam_tcam_losses_terms",
                        lambda *a: pytest.fail("the new entry ran with no new term configured"))
    a = _trainer(cuda)
    la = a.step(x, raw, seeds).cpu()
    monkeypatch.setattr(training, "tcam_losses", spy)
    b = _trainer(cuda)
    lb = b.step(x, raw, seeds).cpu()
    torch.cuda.synchronize()
    assert called == [None] and la.shape == (4,)
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert torch.equal(a.flat.view(torch.int32), b.flat.view(torch.int32))


# ------------------------------------------------------------------------ entry point
def test_main_trains_with_the_three_terms(cuda, tmp_path):
    """main.py --task TCAM with the three constraints and the teacher from epoch 0 on, two
    epochs of the tiny synthetic dataset: finite losses, every term named, best_loc written."""
    from test_gpu_entrypoints import _train
    from tcam_wsol_video_amd import checkpoints as CK
    exp = str(tmp_path / "exp")
    logs = _train(["--task", "TCAM", "--synthetic", "1", "--max_epochs", "2", "--batch_size",
                   "16", "--exp_path", exp, "--checkpoint_save", "100", "--sl_tc_knn", "1",
                   "--sl_tc_knn_mode", "before", "--cam_curve_interval", "0.05",
                   "--empty_out_bb_tc", "True", "--sizefg_tmp_tc", "True",
                   "--size_bg_g_fg_tc", "True", "--sl_tc_epoch_switch_to_sl", "0",
                   "--final_test_eval", "False"])
    assert [lg["epoch"] for lg in logs] == [0, 1, 2]
    for lg in logs[1:]:
        assert len(lg["losses"]) == 7 and np.isfinite(lg["losses"]).all(), lg["losses"]
        assert lg["loss_names"] == ["total", "self_learning_tcams", "con_ran_field_tcams",
                                    "max_size_positive_tcams", "bg_size_great_size_fg_tcams",
                                    "fg_size_tcams", "empty_outside_bbox_tcams"]
        assert all(v != 0.0 for v in lg["losses"][4:])
    assert any(f.endswith("_best_model.pth") for f in os.listdir(os.path.join(exp, "best_loc")))
    _, cpt = CK.find_last_checkpoint(os.path.join(exp, "checkpoints"), CK.CHP_CP)
    names = [n for n, _ in cpt[CK.CHP_T]]
    assert names == ["con_ran_field_tcams", "max_size_positive_tcams", "fg_size_tcams",
                     "bg_size_great_size_fg_tcams", "empty_outside_bbox_tcams",
                     "self_learning_tcams"]
    assert [t for _, t in cpt[CK.CHP_T]][2:5] == pytest.approx([1.01 ** 2] * 3, rel=1e-6)
