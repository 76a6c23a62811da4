"""Generate tests/golden/grad_cams.npz from the REFERENCE gradient CAM extractors.

Run in the build container only (needs /root/reference; never on the GPU box):

    python tests/golden/make_gradcam_golden.py

Imported from the reference (read-only, not copied), with make_golden.py's stubs for the
absent third-party modules: dlib/stdcl/classifier.py (STDClassifier: the WSOL encoder +
WGAP) and dlib/cams/gradcam.py (GradCAM, GradCAMpp, XGradCAM, LayerCAM over cams/core.py's
_CAM), hooked at constants.TRG_LAYERS[encoder] as cams/__init__.py:93-115 builds them.

Per encoder (ResNet50 and VGG16 at 1 x 64^2, InceptionV3 at 1 x 96^2, seeded weights 1234,
eval mode) and per class (3, and the first other class whose fc row has both signs):
``scores = model(x)``, ``low = extractor(class_idx, scores, normalized=True)``
(core.py:139-193).  Stored, numbers only: the input, the classes, hw, the two fc rows, the
hooked activations (fp32), the hooked gradient at position (0, 0) per channel and the four
low-resolution maps.
"""
from __future__ import annotations

import importlib
import os
import sys
sys.dont_write_bytecode = True  # nothing may be written under /root/reference

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from tcam_wsol_video_amd.utils.seeding import seeded_state_dict  # noqa: E402

SEED = 1234
ENCODERS = {"resnet50": (5, 64), "vgg16": (3, 64), "inceptionv3": (5, 96)}
METHODS = {"GradCam": "GradCAM", "GradCAMpp": "GradCAMpp", "XGradCAM": "XGradCAM",
           "LayerCAM": "LayerCAM"}   # constants.py:38-42 -> the class in gradcam.py
FIRST_CLASS = 3


def make_encoder(MG, stdcl, const, gradcam, name, depth, size):
    model = stdcl.STDClassifier(
        task=const.STD_CL, encoder_name=name, encoder_depth=depth, encoder_weights=None,
        in_channels=3, scale_in=1.,
        aux_params=dict(pooling_head="WGAP", classes=10, support_background=False))
    model.load_state_dict(seeded_state_dict(model, SEED), strict=True)
    model.eval()
    x, _ = MG.normalized_frames(1, size, seed=11 + size)
    fc = model.classification_head.fc.weight.detach()
    second = next(c for c in range(fc.shape[0])
                  if c != FIRST_CLASS and bool((fc[c] > 0).any()) and bool((fc[c] < 0).any()))
    classes = [FIRST_CLASS, second]
    out = {"x": x.numpy(), "classes": np.array(classes, dtype=np.int32),
           "fc_rows": fc[classes].numpy().copy()}
    for j, c in enumerate(classes):
        for mname, cname in METHODS.items():
            ext = getattr(gradcam, cname)(model=model, target_layer=const.TRG_LAYERS[name])
            scores = model(x)
            low = ext(class_idx=int(c), scores=scores, normalized=True)
            out[f"low{j}/{mname}"] = low.detach().numpy().astype(np.float32).copy()
            A, g = ext.hook_a[0], ext.hook_g[0]
            ext.clear_hooks()
            if "A" not in out:
                out["A"] = A.numpy().copy()
                out["hw"] = np.int64(A.shape[1] * A.shape[2])
            assert np.array_equal(out["A"], A.numpy())
            # the gradient is the same at every position: one value per channel is kept
            assert bool((g == g[:, :1, :1]).all())
            out.setdefault(f"hook_g{j}", g[:, 0, 0].numpy().copy())
            assert np.array_equal(out[f"hook_g{j}"], g[:, 0, 0].numpy())
    return out


def main():
    torch.set_num_threads(8)
    import make_golden as MG
    _, stdcl, const = MG.reference_models()
    gradcam = importlib.import_module("dlib.cams.gradcam")
    res = {"seed": np.int64(SEED), "methods": np.array(list(METHODS))}
    for name, (depth, size) in ENCODERS.items():
        for k, v in make_encoder(MG, stdcl, const, gradcam, name, depth, size).items():
            res[f"{name}:{k}"] = v
    path = os.path.join(HERE, "grad_cams.npz")
    np.savez_compressed(path, **res)
    print("wrote grad_cams.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
