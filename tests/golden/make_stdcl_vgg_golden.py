"""Generate tests/golden/stdcl_vgg16_train.npz from the REFERENCE stage-1 (task STD_CL) step
of the VGG16 classifier.

Run where the reference checkout is present (make_golden.py's REF), on the CPU only:

    python tests/golden/make_stdcl_vgg_golden.py

Imported from the reference (read-only, not copied) through make_golden.py's stubs, as
make_stdcl_golden.py does: dlib/stdcl/classifier.py (STDClassifier: the WSOL16 VGG encoder +
WGAP), dlib/losses/{master,std}.py (MasterLoss + ClLoss) and dlib/process/instantiators.py
(get_optimizer: SGD over the two parameter groups of _get_model_params_for_opt — for vgg16
``encoder.features.*`` at lr, everything else at lr * lr_classifier_ratio).

One step of train_wsol.py:700-714 + 1162-1184 (amp off) on a seeded model in train mode.
Stored: the inputs, labels, logits, loss, every parameter gradient's squared norm (fp64
sums), the groups' lrs and sizes, and the full gradient / post-step value of a few small
tensors, at two sizes (4 x 64^2, 2 x 96^2 with a repeated label).
"""
from __future__ import annotations

import os
import sys
sys.dont_write_bytecode = True  # nothing may be written into the reference checkout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import make_stdcl_golden as SG  # noqa: E402
from tcam_wsol_video_amd.utils.seeding import seeded_state_dict  # noqa: E402

FULL = ("encoder.features.0.weight", "encoder.features.0.bias", "encoder.conv6.bias",
        "classification_head.fc.weight", "classification_head.fc.bias")
OPT = SG.OPT
CASES = SG.CASES


class _Args(SG._Args):
    def __init__(self, const):
        super().__init__(const)
        self.model = {"encoder_name": "vgg16"}


def make_case(refs, n, size, labels, seed):
    MG, stdcl, const, master, std, inst = refs
    model = stdcl.STDClassifier(
        task=const.STD_CL, encoder_name="vgg16", encoder_depth=3, encoder_weights=None,
        in_channels=3, scale_in=1.,
        aux_params=dict(pooling_head="WGAP", classes=10, support_background=False))
    model.load_state_dict(seeded_state_dict(model, 1234), strict=True)
    model.train()
    x, _ = MG.normalized_frames(n, size, seed=seed)
    y = torch.tensor(labels, dtype=torch.long)
    ml = master.MasterLoss(cuda_id="cpu")
    ml.add(std.ClLoss(cuda_id="cpu", support_background=False, multi_label_flag=False))
    opt, _ = inst.get_optimizer(_Args(const), model)
    opt.zero_grad()
    logits = model(x)
    loss = ml(epoch=0, cl_logits=logits, glabel=y)
    loss.backward()
    named = dict(model.named_parameters())
    out = dict(x=x.numpy(), labels=np.array(labels, dtype=np.int32),
               logits=logits.detach().numpy(), loss=np.float64(float(loss.detach())),
               names=np.array(list(named)),
               gsq=np.array([float((p.grad.double() ** 2).sum()) for p in named.values()]),
               lrs=np.array([g["lr"] for g in opt.param_groups]),
               group_sizes=np.array([len(g["params"]) for g in opt.param_groups]))
    for k in FULL:
        out["grad/" + k] = named[k].grad.detach().numpy().copy()
    opt.step()
    for k in FULL:
        out["new/" + k] = named[k].detach().numpy().copy()
    return out


def main():
    torch.set_num_threads(8)
    refs = SG._reference()
    res = {}
    for name, (n, size, labels, seed) in CASES.items():
        for k, v in make_case(refs, n, size, labels, seed).items():
            res[f"{name}:{k}"] = v
    res["seed"] = np.int64(1234)
    res["opt"] = np.array([OPT["opt__lr"], OPT["opt__momentum"], OPT["opt__dampening"],
                           OPT["opt__weight_decay"], float(OPT["opt__nesterov"]),
                           OPT["opt__lr_classifier_ratio"]])
    np.savez_compressed(os.path.join(HERE, "stdcl_vgg16_train.npz"), **res)
    print("wrote stdcl_vgg16_train.npz", sorted(CASES))


if __name__ == "__main__":
    main()
