"""The gradient CAM extractors (inference.GradCAM, GradCAMpp, XGradCAM, LayerCAM) on the three
STD_CL classifiers at the inputs of tests/golden/grad_cams.npz (the reference's own
extractors on its STDClassifier, seeded weights 1234), in every precision of the forward, and
CAMComputer's ``method`` argument."""
import os

import numpy as np
import pytest
import torch

import grad_cam_ref as G
import infer_tail_ref as R
from tcam_wsol_video_amd import inference, ops
from tcam_wsol_video_amd.inference import CAMComputer
from tcam_wsol_video_amd.models import TRG_LAYERS, build_r50_stdcl, build_stdcl
from tcam_wsol_video_amd.utils.seeding import synthetic_clip

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "grad_cams.npz")
CAM_TOL = 1e-4          # the project's CAM-vs-golden bound (tests/test_gpu_entrypoints.py:96)
EXTRACTORS = {"GradCam": inference.GradCAM, "GradCAMpp": inference.GradCAMpp,
              "XGradCAM": inference.XGradCAM, "LayerCAM": inference.LayerCAM}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module", params=["resnet50", "vgg16", "inceptionv3"])
def classifier(request, cuda, golden):
    name = request.param
    seed = int(golden["seed"])
    m = build_r50_stdcl(seed=seed) if name == "resnet50" else build_stdcl(name, seed=seed)
    return name, m.to(cuda)


@pytest.mark.parametrize("prec", ["f16x3", "x6", "amp"])
def test_extractors_match_the_reference_goldens(cuda, golden, classifier, prec):
    """Both golden classes as one batch of two frames (one class per frame).  f16x3 and x6:
    within 1e-4 of the reference's map.  amp: the features are fp16 (S1) and the method's
    arithmetic fp32, so the map is held to the fp64 method on the device's own S1 features,
    within the host module's bound."""
    name, m = classifier
    m.conv_precision = prec
    x = torch.from_numpy(golden[f"{name}:x"]).to(cuda)
    classes = [int(c) for c in golden[f"{name}:classes"]]
    with torch.no_grad():
        scores = m(x.repeat(2, 1, 1, 1).contiguous())
    feats = ops.s3_to_nchw(m.features).double().cpu()
    fw = m.classification_head.fc.weight.detach().cpu()
    for method, cls in EXTRACTORS.items():
        ext = cls(m, target_layer=TRG_LAYERS[name])
        low = ext(classes, scores, normalized=True, reshape=None).cpu()
        assert low.shape == (2,) + golden[f"{name}:low0/{method}"].shape
        one = ext(classes[1], scores, reshape=None)      # one class: every frame gets it
        for j in range(2):
            ref = G.final_low(torch.from_numpy(golden[f"{name}:low{j}/{method}"]).double())
            err = float((low[j].double() - ref).abs().max())
            if prec == "amp":
                kr = G.grad_cam_ref(feats[j:j + 1], fw, [classes[j]], 5, 5, "s1", method,
                                    exps=m.features_exp)
                r = R.ratio(low[j], kr["low"][0], kr["b_low"][0])
                print(f"{name} {prec} {method} class {classes[j]}: {r:.3g} of the bound on "
                      f"the S1 features ({err:.3g} from the golden)")
                assert r <= 1.0
            else:
                print(f"{name} {prec} {method} class {classes[j]}: {err:.3g} from the golden")
                assert err <= CAM_TOL
        # a single class index goes to every frame of the batch, as inference.CAM's does
        assert one.shape == low.shape
        assert torch.equal(one[1].cpu().view(torch.int32), low[1].view(torch.int32))


def test_extractor_reshape_and_builder(cuda, golden, classifier):
    """reshape=(H, W) returns the bilinear map of the low one; build_std_cam_extractor picks
    the class from ``args.method`` (cams/__init__.py:53-117)."""
    import argparse
    name, m = classifier
    m.conv_precision = "f16x3"
    x = torch.from_numpy(golden[f"{name}:x"]).to(cuda)
    with torch.no_grad():
        scores = m(x)
    H = x.shape[2]
    for method, cls in EXTRACTORS.items():
        args = argparse.Namespace(method=method, encoder_name=name)
        ext = inference.build_std_cam_extractor(m, args)
        assert type(ext) is cls and ext.target_layer == TRG_LAYERS[name]
        low = ext(3, scores)
        cam = ext(3, scores, reshape=(H, H))
        want = torch.nn.functional.interpolate(low[None, None], (H, H), mode="bilinear",
                                               align_corners=False)[0, 0]
        assert cam.shape == (H, H) and float((cam - want).abs().max()) < 1e-6
    assert type(inference.build_std_cam_extractor(
        m, argparse.Namespace(method="CAM", encoder_name=name))) is inference.CAM
    with pytest.raises(ValueError, match="ScoreCAM"):
        inference.build_std_cam_extractor(m, argparse.Namespace(method="ScoreCAM",
                                                                encoder_name=name))


def _clip(cuda):
    clip = synthetic_clip(3, seed=5, height=224, width=224)
    x = ((torch.from_numpy(clip).float().permute(0, 3, 1, 2) / 255.0 - 0.45) / 0.225).contiguous()
    gt = torch.tensor([[[30, 40, 150, 170]], [[10, 10, 200, 120]], [[60, 60, 100, 100]]],
                      dtype=torch.int32)
    return x.to(cuda), torch.tensor([3, 0, 7], device=cuda), gt.to(cuda)


def _evaluate(m, cuda, **kw):
    x, y, gt = _clip(cuda)
    comp = CAMComputer(m, cam_curve_interval=0.01, device=cuda, **kw)
    u8 = comp.evaluate_batch(x, y, gt)
    acc = comp.compute_and_evaluate()
    ev = comp.evaluator
    counts = [np.asarray(ev.num_correct[t]).tolist() + np.asarray(ev.num_correct_top1[t]).tolist()
              for t in (30, 50, 70)]
    return u8.clone(), comp.last_cam.clone(), (acc, counts, ev.best_tau_list, int(ev.cnt))


def test_camcomputer_method_cam_is_the_default_path(cuda):
    """CAMComputer(method="CAM") is CAMComputer(): CAMs and counters bit-identical; another
    method changes the CAMs and equals that method's extractor."""
    m = build_r50_stdcl(seed=21).to(cuda)
    u8_a, cam_a, cnt_a = _evaluate(m, cuda)
    u8_b, cam_b, cnt_b = _evaluate(m, cuda, method="CAM")
    assert torch.equal(u8_a, u8_b) and torch.equal(cam_a.view(torch.int32),
                                                    cam_b.view(torch.int32))
    assert cnt_a == cnt_b and cnt_a[-1] == 3
    u8_c, cam_c, _ = _evaluate(m, cuda, method="LayerCAM")
    assert not torch.equal(u8_a, u8_c)
    x, y, _ = _clip(cuda)
    with torch.no_grad():
        scores = m(x)
    want = inference.LayerCAM(m)(y, scores, reshape=tuple(x.shape[2:]))
    assert torch.equal(want.view(torch.int32), cam_c.view(torch.int32))
    with pytest.raises(ValueError, match="SSCAM"):
        CAMComputer(m, device=cuda, method="SSCAM")
