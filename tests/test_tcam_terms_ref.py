"""tests/tcam_terms_ref.py pinned on the CPU: its fp64 terms and gradient against the
reference's own classes (tests/golden/tcam_terms.npz), the inputs' conditions (every ELB branch
of every term, no barrier argument inside the ambiguity band of its breakpoint), an fp32
emulation of the kernel's formula accepted at every GPU case, plausible wrong kernels rejected,
and the host logic of the three loss classes (names, set_eps, l_holder, t round trips)."""
import os

import numpy as np
import pytest
import torch

import tcam_terms_ref as T
import train_fwd_ref as R

G = os.path.join(os.path.dirname(__file__), "golden", "tcam_terms.npz")
F32 = torch.float32


@pytest.fixture(scope="module")
def gold():
    d = np.load(G)
    return {k: d[k] for k in d.files}


# ------------------------------------------------------------------ against the golden
def _gold_args(gold):
    f = torch.from_numpy(gold["fcams"]).double().flatten(2)
    S = torch.softmax(f, 1)
    fs = torch.from_numpy(gold["fg_size"])
    msk = torch.from_numpy(gold["msk"]).flatten(1)
    lam3 = tuple(float(gold[f"lam_{k}"]) for k in T.KEYS)
    t3 = tuple(float(gold[f"t_{k}"]) for k in T.KEYS)
    return f, S, fs, msk, lam3, t3, float(gold["eps"])


@pytest.mark.parametrize("i,key", list(enumerate(T.KEYS)))
def test_each_term_alone_matches_the_reference(gold, i, key):
    """Value and autograd gradient of each term alone.  1e-6, not fp64's 1e-12: the
    reference's ELB keeps t in an fp32 buffer and forms 1/t, 1/t^2 and log(1/t^2) from it in
    fp32 (elb.py:118-132) even on fp64 inputs, a few 2^-24 of the barrier's constants."""
    f, S, fs, msk, lam3, t3, eps = _gold_args(gold)
    only = tuple(v if j == i else 0.0 for j, v in enumerate(lam3))
    r = T.terms_ref(f, S, None, None, None, None, (0.0, 0.0, 0.0), 1.0, fs, msk, only, t3, eps)
    ref = float(gold[f"{key}_total"])
    assert abs(float(r["losses"][5 + i]) - ref) <= 1e-6 * max(1.0, abs(ref))
    assert abs(float(r["losses"][0]) - ref) <= 1e-6 * max(1.0, abs(ref))
    g = torch.from_numpy(gold[f"{key}_grad"]).flatten(2)
    assert float((r["dF"] - g).abs().max()) <= 1e-6 * float(g.abs().max())
    assert float(g.abs().max()) > 0


def test_seven_terms_slots_match_the_reference(gold):
    """All seven through the reference MasterLoss: the slots this module computes without the
    CRF filters (size, the three new terms, self-learning), in get_loss_tcam's order; size's
    lambda 0.01 is not an fp32 value, hence 1e-6."""
    f, S, fs, msk, lam3, t3, eps = _gold_args(gold)
    seeds = torch.from_numpy(gold["seeds"]).flatten(1)
    lam = (float(gold["lam_sl"]), 0.0, float(gold["lam_size"]))
    r = T.terms_ref(f, S, seeds, None, None, None, lam, float(gold["t_size"]), fs, msk, lam3,
                    t3, eps)
    order = [str(k) for k in gold["order"]]
    assert order == ["crf", "rgb", "size", "fgsz", "bgfg", "eob", "sl"]
    ref = dict(zip(order, gold["seven_terms"]))
    slot = dict(sl=1, size=3, bgfg=5, fgsz=6, eob=7)
    for k, i in slot.items():
        assert abs(float(r["losses"][i]) - ref[k]) <= 1e-6 * abs(ref[k]), k
    assert abs(gold["seven_total"] - gold["seven_terms"].sum()) <= 1e-12 * abs(gold["seven_total"])


# -------------------------------------------------------- the GPU cases' conditions
def _cases():
    for B, HW in R.LOSS_SHAPES:
        c = T.terms_input(B, HW, seed=R.loss_seed(B, HW))
        S = torch.softmax(c["f"].float(), 1)       # the device's softmax within its own bound
        for t3 in T.t_cases():
            yield B, HW, c, S, t3


def test_no_barrier_argument_is_ambiguous_and_every_branch_is_taken():
    """The fp64 reference alone puts no frame's barrier argument within its fp32 error of the
    breakpoint -1/t^2 at any GPU case (so the GPU test needs no skip), and over the cases
    every barrier of every term takes both branches; at t = 1 both fg-size barriers are
    linear, as for any sizes in [0, 1]."""
    seen = {}
    for B, HW, c, S, t3 in _cases():
        run = T.terms_runs(c)[-1]
        r = T.terms_ref(c["f"], S, *run[1:6], R.LOSS_T[0], *run[6:9], t3, T.EPS)
        for k, es in r["elb"].items():
            for n, e in enumerate(es):
                assert not bool(e["ambiguous"].any()), (B, HW, t3, k, n)
                seen.setdefault((k, n), set()).update(e["is_log"].tolist())
                if k == "fgsz" and t3[1] == 1.0:
                    assert not bool(e["is_log"].any())
    assert seen == {(k, n): {True, False}
                    for k, n in (("bgfg", 0), ("fgsz", 0), ("fgsz", 1), ("eob", 0))}, seen


def test_inputs_hold_every_mask_kind_and_size_relation():
    kinds = {T.mask_kind(b, HW) for B, HW in R.LOSS_SHAPES for b in range(B)}
    assert kinds == set(T.MASK_KINDS)
    c = T.terms_input(257, 5, seed=R.loss_seed(257, 5))
    assert float(c["msk"].max()) > 1.5 and float(c["msk"].min()) == 0.0
    S = torch.softmax(c["f"].double(), 1)
    d = S[:, 0].sum(1) - S[:, 1].sum(1)
    assert bool((d > 4).any()) and bool((d < -1).any()) and bool((d.abs() < 1).any())
    fgn = S[:, 1].sum(1) / 5
    rel = c["fg_size"].double() - fgn
    assert bool((rel > 0.3).any()) and bool((rel < -0.3).any()) and bool((rel.abs() < 0.01).any())


# ---------------------------------------------------------- the kernel's fp32 formula
def _elb32(fx64, t, B_):
    fx = fx64.to(F32)
    t = torch.tensor(t, dtype=F32)
    ct = -1.0 / (t * t)
    is_log = fx <= ct
    safe = torch.minimum(fx, ct)
    l = torch.where(is_log, -(1.0 / t) * torch.log(-safe),
                    t * fx - (1.0 / t) * torch.log(1.0 / (t * t)) + 1.0 / t)
    dl = torch.where(is_log, -(1.0 / t) / safe, t.expand_as(fx))
    return l, dl


def emulate(c, S, run, t, t3, eps, mut=""):
    """tcam_tcam_losses_terms' arithmetic in torch: fp64 plane sums, one cast of each barrier
    argument, the fp32 ELB formula, fp32 coefficients and gradient.  The four earlier slots are
    the fp64 reference's values (their kernel is tested by test_train_fwd_ref.py).  ``mut``:
    one of the wrong kernels of test_wrong_kernels_are_rejected."""
    name, seeds, AS, gx, extra, lam, fs, msk, lam3 = run
    base = R.tcam_loss_ref(c["f"], S, seeds, AS, gx, extra, lam, t)
    B, _, HW = S.shape
    S32 = S.to(F32)
    bl = S.double().sum(2)
    if mut == "shared_t":
        t3 = (t3[0],) * 3
    if mut == "no_eps":
        eps = 0.0
    nb = 1.0 if mut == "sum" else float(B)
    f_ = lambda v: torch.tensor(v, dtype=F32)
    vals = torch.zeros(3, dtype=F32)
    # the size term's constants
    _, dls = _elb32(-bl, t, B)
    cc = (-f_(lam[2]) * 0.5 * dls / float(B)) if lam[2] else torch.zeros(B, 2, dtype=F32)
    cc = cc.clone()
    cm = None
    if lam3[0]:
        d = bl[:, 0] - bl[:, 1]
        l, dl = _elb32(d if mut == "sign" else -d, t3[0], B)
        vals[0] = (R.f32(lam3[0]) * l.double().sum() / nb).to(F32)
        g = f_(lam3[0]) * dl / nb * (-1.0 if mut == "sign" else 1.0)
        cc[:, 0] -= g
        cc[:, 1] += g
    if lam3[1] and fs is not None:
        hw = 1.0 if mut == "no_hw" else float(HW)
        half = 1.0 if mut == "no_half" else 0.5
        fgn, e = bl[:, 1] / hw, float(np.float32(eps))
        l1, dl1 = _elb32(fs.double() - e - fgn, t3[1], B)
        l2, dl2 = _elb32(fgn - fs.double() - e, t3[1], B)
        vals[1] = (R.f32(lam3[1]) * half * (l1.double().sum() + l2.double().sum()) / nb).to(F32)
        cc[:, 1] += f_(lam3[1]) * half * (dl2 - dl1) / (f_(nb) * f_(hw))
    if lam3[2] and msk is not None:
        w64 = msk.double() if mut == "msk" else 1.0 - msk.double()
        l, dl = _elb32((S[:, 1].double() * w64).sum(1), t3[2], B)
        vals[2] = (R.f32(lam3[2]) * l.double().sum() / nb).to(F32)
        cm = f_(lam3[2]) * dl / nb
    total = base["losses"][0].to(F32)
    for v in vals:
        total = total + v
    losses = torch.cat([total[None], base["losses"][1:].to(F32), vals])
    g = cc[:, :, None].expand(B, 2, HW).clone()
    if AS is not None:
        g += (-2.0 * f_(lam[1]) / float(B)) * AS
    if gx is not None:
        g += gx
    if cm is not None:
        w = msk if mut == "msk" else 1.0 - msk
        if mut == "const_grad":
            w = torch.ones_like(msk)
        g[:, 1] += cm[:, None] * w
    dot = (S32 * g).sum(1, keepdim=True)
    dF = S32 * (g - dot)
    if seeds is not None and lam[0]:
        valid = (seeds == 0) | (seeds == 1)
        onehot = torch.stack([(seeds == 0), (seeds == 1)], 1).to(F32)
        dF = dF + (f_(lam[0]) / float(valid.sum())) * (S32 - onehot) * valid[:, None].to(F32)
    return losses, dF


def _accepted(c, S, run, t, t3, mut=""):
    ref = T.terms_ref(c["f"], S, *run[1:6], t, *run[6:9], t3, T.EPS)
    lo, dF = emulate(c, S, run, t, t3, T.EPS, mut)
    ok = {f"l{i}": R.accept(lo[i:i + 1], ref["losses"][i:i + 1], ref["bounds"][i:i + 1])
          for i in (0, 5, 6, 7)}
    ok["dF"] = R.accept(dF, ref["dF"], ref["b_dF"])
    return ok


def test_fp32_emulation_is_accepted_at_every_gpu_case():
    for B, HW, c, S, t3 in _cases():
        for run in T.terms_runs(c):
            ok = _accepted(c, S, run, R.LOSS_T[1], t3)
            assert all(ok.values()), (B, HW, t3, run[0], ok)


@pytest.mark.parametrize("mut", ["sum", "no_half", "no_hw", "msk", "sign", "no_eps", "shared_t",
                                 "const_grad"])
def test_wrong_kernels_are_rejected(mut):
    """ELB summed instead of averaged over b; fg size without / 2, without / (HW), without eps;
    msk in place of 1 - msk; the sign of bg - fg flipped; one t for the three terms (the mixed-t
    case); the mask-weighted gradient as a per-plane constant.  Each must miss a bound at (3,
    4095) in the three-term run — the value, the gradient, or both."""
    B, HW = 3, 4095
    c = T.terms_input(B, HW, seed=R.loss_seed(B, HW))
    S = torch.softmax(c["f"].float(), 1)
    run = T.terms_runs(c)[3]
    assert all(_accepted(c, S, run, 1.0, T.T_MIXED).values())
    ok = _accepted(c, S, run, 1.0, T.T_MIXED, mut)
    assert not all(ok.values()), (mut, ok)
    if mut != "const_grad":
        assert not ok["l0"], (mut, ok)
    assert not ok["dF"], (mut, ok)


def test_teacher_stats_reference():
    for B, H, W in T.STATS_SHAPES:
        cams, roi, bbox = T.stats_input(B, H, W, seed=B + H)
        msk, fg, b = T.stats_ref(cams, roi, bbox)
        assert float(msk[0].min()) == 1.0                  # the whole frame
        if B >= 2:
            assert float(msk[B - 1].max()) == 0.0          # the empty box
        x0, y0, x1, y1 = (int(v) for v in bbox[B // 2])
        assert float(msk[B // 2].sum()) == (x1 - x0) * (y1 - y0)
        want = torch.stack([(cams[i].double() * roi[i]).sum() / (H * W) for i in range(B)])
        assert torch.equal(fg, want) and bool((b >= 0).all())


# ------------------------------------------------------------------------- host logic
def _three(elbs=None, windows=None):
    from tcam_wsol_video_amd import losses as L
    elbs = elbs or [L.ELB(init_t=1.0) for _ in range(3)]
    windows = windows or {}
    fg = L.FgSizeTcams(lambda_=0.8, elb=elbs[0], **windows.get("fgsz", {}))
    bg = L.BgSizeGreatSizeFgTcams(lambda_=0.5, elb=elbs[1], **windows.get("bgfg", {}))
    eo = L.EmptyOutsideBboxTcams(lambda_=0.3, elb=elbs[2], **windows.get("eob", {}))
    return fg, bg, eo


def test_class_names_and_exports():
    import tcam_wsol_video_amd as P
    from tcam_wsol_video_amd import losses as L
    fg, bg, eo = _three()
    assert [x.__name__ for x in (fg, bg, eo)] == [
        "fg_size_tcams", "bg_size_great_size_fg_tcams", "empty_outside_bbox_tcams"]
    for n in ("FgSizeTcams", "BgSizeGreatSizeFgTcams", "EmptyOutsideBboxTcams"):
        assert n in L.__all__ and n in P.__all__ and getattr(P, n) is getattr(L, n)
        with pytest.raises(AssertionError):
            getattr(L, n)(lambda_=1.0)                      # elb must be an ELB
    assert fg.eps == 0.0 and not fg.eps_already_set
    with pytest.raises(AssertionError):
        fg.set_eps(1)                                       # a float, as the reference
    with pytest.raises(AssertionError):
        fg.set_eps(-0.1)
    fg.set_eps(0.25)
    assert fg.eps == 0.25 and fg.eps_already_set
    m = L.MasterLoss()
    for x in (fg, bg, eo):
        m.add(x)                                            # NotImplementedError on the parent
    assert m.n_holder == ["master_loss", "fg_size_tcams", "bg_size_great_size_fg_tcams",
                          "empty_outside_bbox_tcams"]


def test_forward_before_set_eps_is_an_assertion():
    from tcam_wsol_video_amd import losses as L
    fg, _, _ = _three()
    m = L.MasterLoss()
    m.add(fg)
    with pytest.raises(AssertionError, match="set it first"):
        m(epoch=0, fcams=torch.zeros(2, 2, 4, 4), fg_size=torch.zeros(2))


def test_l_holder_order_windows_and_term_arguments(monkeypatch):
    """MasterLoss.forward hands the active terms, each with its own t, to the one fused call
    and fills l_holder in self.losses order, zero for a term outside its window (the fused
    call is replaced by a recorder: no device)."""
    from tcam_wsol_video_amd import losses as L
    from tcam_wsol_video_amd import training
    elbs = [L.ELB(init_t=1.0) for _ in range(4)]
    for e, t in zip(elbs, (10.0, 2.5, 1.25, 1.75)):
        e.set_t(t)
    fg, bg, eo = _three(elbs, {"eob": dict(start_epoch=2, end_epoch=-1),
                               "bgfg": dict(start_epoch=0, end_epoch=1)})
    fg.set_eps(0.125)
    size = L.MaxSizePositiveTcams(lambda_=0.01, elb=elbs[3])
    m = L.MasterLoss()
    for x in (size, fg, bg, eo):             # get_loss_tcam's order
        m.add(x)
    seen = {}

    def fake(fcams, raw, seeds, lam, t, sigma, rgb=None, crf_scale=1.0, terms=None):
        seen.update(lam=lam, t=t, terms=terms)
        n = 4 + len(terms or {})
        # slot i holds i: total 0, sl 1, crf 2, size 3, then bgfg / fgsz / eob in TERM_KEYS order
        return torch.arange(n, dtype=F32), torch.zeros_like(fcams)

    monkeypatch.setattr(training, "tcam_losses", fake)
    f = torch.zeros(2, 2, 4, 4, requires_grad=True)
    fs, msk = torch.rand(2), torch.ones(2, 1, 4, 4)
    m(epoch=0, fcams=f, fg_size=fs, msk_bbox=msk)
    assert set(seen["terms"]) == {"bgfg", "fgsz"} and seen["t"] == 1.75
    assert seen["terms"]["bgfg"] == (0.5, 2.5)
    assert seen["terms"]["fgsz"][:3] == (0.8, 10.0, 0.125) and seen["terms"]["fgsz"][3] is fs
    # l_holder: total, size (3), fgsz (slot 5 of the two configured: bgfg 4, fgsz 5), bgfg, 0
    assert [float(v.detach()) for v in m.l_holder] == [0.0, 3.0, 5.0, 4.0, 0.0]
    m(epoch=2, fcams=f, fg_size=fs, msk_bbox=msk)
    assert set(seen["terms"]) == {"fgsz", "eob"} and seen["terms"]["eob"][:2] == (0.3, 1.25)
    assert seen["terms"]["eob"][2] is msk
    assert [float(v.detach()) for v in m.l_holder] == [0.0, 3.0, 4.0, 0.0, 5.0]


def test_t_round_trip_with_differing_t():
    from tcam_wsol_video_amd import losses as L
    from tcam_wsol_video_amd import checkpoints as CK

    def master(ts):
        elbs = [L.ELB(init_t=1.0, max_t=10.0, mulcoef=1.01) for _ in range(4)]
        for e, t in zip(elbs, ts):
            e.set_t(t)
        m = L.MasterLoss()
        m.add(L.MaxSizePositiveTcams(elb=elbs[3]))
        for x in _three(elbs[:3]):
            m.add(x)
        m.add(L.SelfLearningTcams())
        return m

    a = master((1.5, 2.5, 3.5, 4.5))
    a.update_t()
    t = a.get_t()
    assert [n for n, _ in t] == ["max_size_positive_tcams", "fg_size_tcams",
                                 "bg_size_great_size_fg_tcams", "empty_outside_bbox_tcams",
                                 "self_learning_tcams"]
    want = [float(np.float32(v) * np.float32(1.01)) for v in (4.5, 1.5, 2.5, 3.5)]
    assert [v for _, v in t[:4]] == pytest.approx(want, rel=1e-7) and t[4][1] == 0.0
    b = master((1.0, 1.0, 1.0, 1.0))
    b.set_t(t)
    assert b.get_t() == t
    # the trainer's checkpoint entry: the same names, in get_loss_tcam's order
    ck = CK._loss_t(4.5, (True, False, True), False, {"bgfg": 2.5, "eob": 3.5, "fgsz": 1.5})
    assert ck == [["max_size_positive_tcams", 4.5], ["fg_size_tcams", 1.5],
                  ["bg_size_great_size_fg_tcams", 2.5], ["empty_outside_bbox_tcams", 3.5],
                  ["self_learning_tcams", 0.0]]
    assert CK._loss_t(1.0) == [["con_ran_field_tcams", 0.0], ["max_size_positive_tcams", 1.0],
                               ["self_learning_tcams", 0.0]]
