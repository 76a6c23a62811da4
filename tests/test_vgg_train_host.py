"""CPU checks of the VGG16 stage-1 step: the stand-alone address-check program of its
kernels' index arithmetic (tests/host/vgg_addr_check.cpp over csrc/vgg_train_addr.h: every
access of every thread of each kernel's whole launch grid stays inside its buffer, over the
VGG16 layer ladder at 36x44, 64x64 and 224x224), and the trainer factory."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "vgg_addr_check.cpp")


def _compile(cxx, exe, sanitize):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", SRC, "-o", exe]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_vgg_kernel_addresses_stay_in_bounds(tmp_path):
    """Built with the host compiler and -fsanitize=address,undefined (without them when the
    sanitizer runtimes are not installed: the program's own assertions remain), run as a plain
    executable."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or \
        shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "vgg_addr_check")
    r = _compile(cxx, exe, True)
    sanitized = r.returncode == 0
    if not sanitized:
        r = _compile(cxx, exe, False)
    assert r.returncode == 0, r.stderr
    print("sanitizers:", "address,undefined" if sanitized else "not available")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "vgg_addr_check: ok" in run.stdout, run.stdout


def test_factory_picks_the_trainer_by_encoder_name():
    from tcam_wsol_video_amd import cl_training as CT
    from tcam_wsol_video_amd.vgg_training import VGG16ClassifierTrainer
    assert CT.classifier_trainer_class("resnet50") is CT.ClassifierTrainer
    assert CT.classifier_trainer_class("vgg16") is VGG16ClassifierTrainer
    with pytest.raises(NotImplementedError, match="InceptionV3"):
        CT.classifier_trainer_class("inceptionv3")


def test_trainers_refuse_the_other_encoder_and_a_foreign_stack():
    """ClassifierTrainer(vgg model) keeps raising; the VGG trainer refuses a ResNet50 model,
    and ``vgg_stack`` a features stack that is not conv3x3-pad1 / ReLU / MaxPool2d(2, 2)."""
    import torch.nn as nn
    from tcam_wsol_video_amd import cl_training as CT
    from tcam_wsol_video_amd.models import build_r50_stdcl, build_stdcl
    from tcam_wsol_video_amd.vgg_training import VGG16ClassifierTrainer, vgg_stack
    vgg = build_stdcl("vgg16", seed=0)
    with pytest.raises(NotImplementedError):
        CT.ClassifierTrainer(vgg)
    with pytest.raises(NotImplementedError):
        VGG16ClassifierTrainer(build_r50_stdcl(seed=0))
    with pytest.raises(RuntimeError, match="HIP path"):
        VGG16ClassifierTrainer(vgg)          # a CPU model: no device is touched
    stack = vgg_stack(vgg)
    assert [c.name for c in stack][-1] == "encoder.conv6" and len(stack) == 14
    assert [c.pool for c in stack] == [False, True, False, True, False, False, True] + [False] * 7
    assert stack[0].cin == 3 and stack[0].cin_pad == 8
    vgg.encoder.features[4] = nn.MaxPool2d(3, 2, 1)
    with pytest.raises(NotImplementedError, match="WSOL16"):
        vgg_stack(vgg)
    vgg = build_stdcl("vgg16", seed=0)
    vgg.encoder.features[2] = nn.Conv2d(64, 64, 5, padding=2)
    with pytest.raises(NotImplementedError, match="WSOL16"):
        vgg_stack(vgg)
