"""Generate tests/golden/tcam_terms.npz from the REFERENCE's FgSizeTcams,
BgSizeGreatSizeFgTcams and EmptyOutsideBboxTcams (dlib/losses/tcam.py:281-430): each term
alone, and all seven TCAM terms of get_loss_tcam (process/instantiators.py:147-252) together
through the reference MasterLoss, at 2 x 2 x 16 x 16.

Run in the build container only (needs /root/reference and oracle/_ref; never on the GPU box):

    make -C oracle && python tests/golden/make_terms_golden.py

The reference is imported the way make_train_golden.py imports it (read-only, nothing copied;
``cuda_id="cpu"`` and the two torch.cuda shims).  Stored: the inputs and, per case, the term
values, the total and d total / d fcams from the reference's autograd with the inputs cast to
fp64.  Each term has its own ELB t, as get_loss_tcam's deep copies do.

One more environment patch for the fp64 run: ELB.forward allocates its result with
``.type(torch.float32)`` (elb.py:115) and then index-assigns the branch values, which torch
refuses for fp64 values; while the reference runs, ``Tensor.type(torch.float32)`` of an fp64
tensor returns it unchanged, so the barrier is evaluated in fp64 on the fp32 ``t`` buffers.
(The filter shims of make_train_golden.py take the fp64 softmax as fp32, as the SWIG filters do.)
"""
from __future__ import annotations

import os
import sys
sys.dont_write_bytecode = True  # nothing may be written under /root/reference

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_train_golden as M  # noqa: E402

# the new terms' lambdas, every t and eps are exact in fp32 (the C ABI takes floats), so the
# fp64 reference of the tests can be held to the golden far below one fp32 rounding
LAM = dict(crf=2e-9, rgb=2e-9, size=0.01, fgsz=0.75, bgfg=0.5, eob=0.25, sl=1.0)
T = dict(size=1.75, fgsz=10.0, bgfg=2.5, eob=1.25)
EPS = 2.0 ** -8
ORDER = ("crf", "rgb", "size", "fgsz", "bgfg", "eob", "sl")     # get_loss_tcam's order


def build(mods, which):
    master, tcam, elb_mod = mods
    kw = dict(cuda_id="cpu", support_background=False, multi_label_flag=False)

    def elb(t):
        e = elb_mod.ELB(init_t=1., max_t=10.1, mulcoef=1.01)
        e.set_t(float(t))
        return e

    mk = dict(
        crf=lambda: tcam.ConRanFieldTcams(lambda_=LAM["crf"], sigma_rgb=15., sigma_xy=100.,
                                          scale_factor=1., **kw),
        rgb=lambda: tcam.RgbJointConRanFieldTcams(lambda_=LAM["rgb"], sigma_rgb=15.,
                                                  scale_factor=1., **kw),
        size=lambda: tcam.MaxSizePositiveTcams(lambda_=LAM["size"], elb=elb(T["size"]), **kw),
        fgsz=lambda: tcam.FgSizeTcams(lambda_=LAM["fgsz"], elb=elb(T["fgsz"]), **kw),
        bgfg=lambda: tcam.BgSizeGreatSizeFgTcams(lambda_=LAM["bgfg"], elb=elb(T["bgfg"]), **kw),
        eob=lambda: tcam.EmptyOutsideBboxTcams(lambda_=LAM["eob"], elb=elb(T["eob"]), **kw),
        sl=lambda: tcam.SelfLearningTcams(lambda_=LAM["sl"], seg_ignore_idx=-255, **kw))
    ml = master.MasterLoss(cuda_id="cpu")
    for k in ORDER:
        if k in which:
            term = mk[k]()
            if k == "fgsz":
                term.set_eps(eps=EPS)
            ml.add(term)
    return ml


def main():
    from oracle import crf_ref
    if not (crf_ref.ref_available("xy") and crf_ref.ref_available("color")):
        raise SystemExit("build oracle/_ref first: make -C oracle")
    torch.set_num_threads(8)
    mods = M._install()
    _type = torch.Tensor.type
    torch.Tensor.type = lambda self, dtype=None, **k: self if (
        dtype is torch.float32 and self.dtype == torch.float64) else _type(self, dtype, **k)
    n, h, w = 2, 16, 16
    g = torch.Generator().manual_seed(31)
    fcams = torch.randn(n, 2, h, w, generator=g) * 2.0
    fcams[1, 0] += 1.5                      # frame 1: bg > fg
    raw = (torch.rand(n, 3, h, w, generator=g) * 255).round()
    seeds = torch.randint(-1, 2, (n, h, w), generator=g)
    seeds[seeds < 0] = -255
    seq, frm = torch.tensor([4., 4.]), torch.tensor([1., 0.])
    fg_size = torch.tensor([0.30, 0.55])
    msk = torch.zeros(n, 1, h, w)
    msk[0, 0, 3:12, 2:9] = 1.0
    msk[1, 0, 0:16, 5:16] = 1.0
    out = dict(fcams=fcams.numpy(), raw=raw.numpy().astype(np.uint8),
               seeds=seeds.numpy().astype(np.int32), seq=seq.numpy(), frm=frm.numpy(),
               fg_size=fg_size.numpy(), msk=msk.numpy(), eps=np.float64(EPS),
               order=np.array(ORDER))
    for k, v in LAM.items():
        out[f"lam_{k}"] = np.float64(v)
    for k, v in T.items():
        out[f"t_{k}"] = np.float64(v)
    for case, which in (("fgsz", ("fgsz",)), ("bgfg", ("bgfg",)), ("eob", ("eob",)),
                        ("seven", ORDER)):
        ml = build(mods, which)
        f = fcams.double().requires_grad_(True)
        total = ml(epoch=0, fcams=f, raw_img=raw.double() if case != "seven" else raw,
                   seeds=seeds, seq_iter=seq, frm_iter=frm, fg_size=fg_size.double(),
                   msk_bbox=msk.double())
        total.sum().backward()
        out[f"{case}_total"] = np.float64(float(total.detach().sum()))
        out[f"{case}_terms"] = np.array([float(t.detach().sum()) for t in ml.l_holder[1:]])
        out[f"{case}_grad"] = f.grad.numpy()
        print(case, out[f"{case}_total"], out[f"{case}_terms"])
    np.savez_compressed(os.path.join(HERE, "tcam_terms.npz"), **out)
    print("wrote tcam_terms.npz")


if __name__ == "__main__":
    main()
