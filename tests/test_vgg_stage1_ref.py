"""tests/vgg_stage1_ref.py (the fp64 reference a device VGG16 stage-1 step is to be checked
against; the device step itself is not in the tree yet) against the REFERENCE's own step (tests/golden/make_stdcl_vgg_golden.py: STDClassifier(vgg16) in train
mode, MasterLoss + ClLoss, instantiators.get_optimizer's two SGD groups)."""
import os

import numpy as np
import pytest
import torch

import vgg_stage1_ref as V

GOLD = os.path.join(os.path.dirname(__file__), "golden", "stdcl_vgg16_train.npz")


@pytest.mark.parametrize("case", ("a", "b"))
def test_vgg_step_helper_matches_reference_golden(case):
    """Run in fp32 — the reference's CPU arithmetic, with the golden's 8 intra-op threads —
    the helper reproduces the reference to 1e-5 relative (the figure test_train_oracle.py
    holds the ResNet50 oracle to against the same kind of golden): loss, logits, every
    parameter gradient's squared norm, the stored gradients and post-step values; the two
    groups' lrs are [lr, 10 lr] and their sizes the reference's."""
    from tcam_wsol_video_amd.models import build_stdcl
    d = np.load(GOLD)
    g = {k[len(case) + 1:]: d[k] for k in d.files if k.startswith(case + ":")}
    sd = build_stdcl("vgg16", seed=int(d["seed"])).state_dict()
    lr, mom, damp, wd, nest, ratio = [float(v) for v in d["opt"]]
    nt = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        loss, logits, grads, new, groups, lrs = V.vgg16_stdcl_step(
            sd, torch.from_numpy(g["x"]), torch.from_numpy(g["labels"]), lr=lr,
            lr_classifier_ratio=ratio, momentum=mom, dampening=damp, weight_decay=wd,
            nesterov=bool(nest), dtype=torch.float32)
    finally:
        torch.set_num_threads(nt)
    assert abs(loss - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    assert np.abs(logits.numpy() - g["logits"]).max() <= 1e-5 * np.abs(g["logits"]).max()
    names = list(g["names"])
    assert names == list(grads), "parameter order / names differ from the reference"
    gsq = np.array([float((grads[k].double() ** 2).sum()) for k in names])
    np.testing.assert_allclose(gsq, g["gsq"], rtol=1e-5)
    stored = [n[5:] for n in g if n.startswith("grad/")]
    assert len(stored) == 5
    for k in stored:
        ref = g["grad/" + k]
        assert np.abs(grads[k].numpy() - ref).max() <= 1e-5 * np.abs(ref).max(), k
        refn = g["new/" + k]
        assert np.abs(new[k].numpy() - refn).max() <= 1e-5 * max(np.abs(refn).max(), 1e-3), k
    np.testing.assert_allclose(lrs, [lr, 10 * lr], rtol=1e-12)
    np.testing.assert_allclose(g["lrs"], [lr, 10 * lr], rtol=1e-12)
    assert [len(groups[0]), len(groups[1])] == list(g["group_sizes"]) == [26, 4]


def test_helper_groups_are_the_checkpoint_layout():
    """The helper's groups are checkpoints.reference_param_groups' (what a saved optimiser
    state uses), and group 1 is the tail of named_parameters."""
    from tcam_wsol_video_amd import checkpoints as CK
    from tcam_wsol_video_amd.models import build_stdcl
    m = build_stdcl("vgg16", seed=0)
    names = [n for n, _ in m.named_parameters()]
    assert names == V.param_keys(m.state_dict())
    g0, g1 = CK.reference_param_groups(m)
    assert (g0, g1) == V.param_groups(names)
    assert names == g0 + g1
    feats = list(m.encoder.features.named_children())
    convs = [(f"encoder.features.{k}", isinstance(feats[i + 2][1], torch.nn.MaxPool2d)
              if i + 2 < len(feats) else False)
             for i, (k, mod) in enumerate(feats) if isinstance(mod, torch.nn.Conv2d)]
    assert V.conv_names() == convs + [("encoder.conv6", False)]
