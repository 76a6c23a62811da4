"""main.py --task STD_CL --arch STDClassifier --encoder_name vgg16 end to end on the GPU
(tcam_wsol_video_amd/runner.py train_stdcl_main over vgg_training.VGG16ClassifierTrainer),
mirroring test_gpu_entrypoints.test_main_stage1_std_cl_trains_and_feeds_tcam."""
import os

import numpy as np
import pytest
import torch

from tcam_wsol_video_amd import checkpoints as CK
from tcam_wsol_video_amd.models import build_vgg16_tcam
from test_gpu_entrypoints import _train

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("amp", [False, True])
def test_main_stage1_vgg16_trains_and_feeds_tcam(cuda, tmp_path, amp):
    """Stage 1 with the VGG16 encoder: the classifier trains end to end on the device (finite
    losses, both groups' lrs decayed per epoch), the checkpoint's optimiser holds the
    reference's two VGG groups ([26, 4]: encoder.features.* | conv6 + head), validation
    writes best_loc / best_cl, the best model loads bit-equal as a VGG16-TCAM's
    --pretrained_classifier, and a resume trains nothing more."""
    exp = str(tmp_path / "exp")
    argv = ["--task", "STD_CL", "--arch", "STDClassifier", "--encoder_name", "vgg16",
            "--freeze_cl", "False", "--freeze_encoder", "False", "--support_background", "True",
            "--synthetic", "1", "--max_epochs", "2", "--batch_size", "8", "--exp_path", exp,
            "--checkpoint_save", "3", "--cam_curve_interval", "0.01", "--opt__lr", "0.001",
            "--opt__step_size", "1", "--opt__gamma", "0.9", "--amp", str(amp)]
    final = []
    logs = _train(argv, final)
    assert [lg["epoch"] for lg in logs] == [0, 1, 2]
    assert all(np.isfinite(lg["loss"]) for lg in logs[1:])
    assert logs[1]["lr"] == pytest.approx([0.0009, 0.009], rel=1e-6)
    assert logs[2]["lr"] == pytest.approx([0.00081, 0.0081], rel=1e-6)
    if not amp:   # (AMP: GradScaler may back off on its first steps, as torch's does)
        assert all(lg["skipped_steps"] == 0 for lg in logs[1:])
    it, cpt = CK.find_last_checkpoint(os.path.join(exp, "checkpoints"), CK.CHP_CP)
    assert it == 8 and len(cpt[CK.CHP_O]["param_groups"]) == 2
    assert [len(g["params"]) for g in cpt[CK.CHP_O]["param_groups"]] == [26, 4]
    assert [g["lr"] for g in cpt[CK.CHP_O]["param_groups"]] == \
        pytest.approx([0.00081, 0.0081], rel=1e-6)
    assert cpt[CK.CHP_T] == [["cl_loss", 0.0]]
    assert final and set(final[0]) == {"best_loc", "best_cl"}
    for key in ("best_loc", "best_cl"):
        assert os.path.isdir(os.path.join(exp, key))
    # TCAM stage 2 reads the stage-1 classifier
    tcam = build_vgg16_tcam(seed=1)
    CK.load_pretrained_classifier(tcam, os.path.join(exp, "best_loc"))
    _, best = CK.find_last_checkpoint(os.path.join(exp, "best_loc"), CK.CHP_BEST_M)
    assert any(k.startswith("conv6.") for k in best["encoder"])
    for k, v in best["encoder"].items():
        assert torch.equal(tcam.encoder.state_dict()[k].cpu(), v.cpu()), k
    # resume: the last checkpoint (epoch floor(8 / 4) = 2) is evaluated, nothing more trained
    logs2 = _train(argv[:-2] + ["--checkpoint_save", "100", "--amp", str(amp)])
    assert len(logs2) == 1 and logs2[0]["epoch"] == 2
