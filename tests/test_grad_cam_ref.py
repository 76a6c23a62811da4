"""The gradient CAM family's host references (tests/grad_cam_ref.py) pinned to the reference's
own maps (tests/golden/grad_cams.npz, written by tests/golden/make_gradcam_golden.py from
dlib/cams/gradcam.py on its STDClassifier for ResNet50, VGG16 and InceptionV3), the uint8
decision rule on every input of the device tests, and the entry points' --method checks.
No GPU."""
import os

import numpy as np
import pytest
import torch

import grad_cam_ref as G
import infer_tail_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "grad_cams.npz")
ENCODERS = ["resnet50", "vgg16", "inceptionv3"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _case(golden, enc, j):
    A = torch.from_numpy(golden[f"{enc}:A"]).double()
    row = torch.from_numpy(golden[f"{enc}:fc_rows"][j])
    return A, row, int(golden[f"{enc}:hw"])


@pytest.mark.parametrize("enc", ENCODERS)
def test_golden_hooked_gradient_is_the_fc_row_over_hw(golden, enc):
    """The hooked gradient is fp32(W[c] / hw), bit for bit, at every position."""
    A = golden[f"{enc}:A"]
    assert A.shape[1] * A.shape[2] == int(golden[f"{enc}:hw"])
    classes = golden[f"{enc}:classes"]
    assert classes[0] == 3 and classes[1] != 3
    row1 = golden[f"{enc}:fc_rows"][1]
    assert (row1 > 0).any() and (row1 < 0).any()
    for j in range(2):
        g = golden[f"{enc}:hook_g{j}"]
        want = golden[f"{enc}:fc_rows"][j] / np.float32(golden[f"{enc}:hw"])
        assert want.dtype == np.float32 and np.array_equal(g, want)
        assert np.array_equal(G.hook_gradient(torch.from_numpy(golden[f"{enc}:fc_rows"][j]),
                                              int(golden[f"{enc}:hw"])).numpy(),
                              g.astype(np.float64))


@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("enc", ENCODERS)
def test_both_fp64_forms_agree_and_reproduce_the_golden_maps(golden, enc, method):
    """autograd through avgpool + Linear (gradcam.py literally) == the closed form, and both
    are within 5e-6 of the reference's fp32 map; real features have dead channels, so
    XGradCAM's 0 / 0 is exercised."""
    for j in range(2):
        A, row, hw = _case(golden, enc, j)
        W = torch.zeros(4, A.shape[0], dtype=torch.float64)
        W[2] = G.hook_gradient(row, hw) * hw     # the fc row whose gradient is the golden's
        lit = G.final_low(G.autograd_low(A, W, 2, method))
        clo = G.final_low(G.closed_low(A, G.hook_gradient(row, hw), method))
        ref = torch.from_numpy(golden[f"{enc}:low{j}/{method}"]).double()
        assert ref.shape == clo.shape
        d_forms = float((lit - clo).abs().max())
        d_lit = float((lit - G.final_low(ref)).abs().max())
        d_clo = float((clo - G.final_low(ref)).abs().max())
        dead = int((A.flatten(1).sum(1) == 0).sum())
        print(f"{enc} {method} class {j}: forms {d_forms:.3g} literal {d_lit:.3g} "
              f"closed {d_clo:.3g} dead channels {dead}")
        assert d_forms <= 1e-12
        assert d_lit <= G.GOLDEN_TOL and d_clo <= G.GOLDEN_TOL
        # ResNet50's class 3 has a negative sum everywhere under GradCam / XGradCAM: the
        # reference's map is 0 / 0 = NaN at every position, which the store turns into zeros
        zero = bool(torch.isnan(ref).all())
        assert zero == (enc == "resnet50" and j == 0 and method in ("GradCam", "XGradCAM"))
        assert dead > 0 and float(clo.max()) == (0.0 if zero else 1.0)
        # the kernels' reference is the closed form, and its bound covers the golden
        kr = G.grad_cam_ref(A[None], row[None], [0], 5, 5, "f32", method)
        assert float((kr["low"][0] - clo).abs().max()) <= 1e-12


def test_the_methods_differ_on_the_goldens(golden):
    """GradCam, GradCAMpp, LayerCAM and plain CAM give different maps (a kernel that ignored
    ``method`` would not pass).  XGradCAM's weight g S / S is g wherever S is not 0, and a
    channel whose S is 0 without being dead does not occur in post-ReLU features: on this
    classifier XGradCAM's map is GradCam's unless a feature is NaN."""
    A, row, hw = _case(golden, "resnet50", 1)
    g = G.hook_gradient(row, hw)
    maps = {m: G.closed_low(A, g, m) for m in G.METHODS}
    cam = torch.nansum(row.double()[:, None, None] * A, 0)      # plain CAM: no ReLU
    maps["CAM"] = (cam - cam.min()) / (cam - cam.min()).max()
    assert float((maps["GradCam"] - maps.pop("XGradCAM")).abs().max()) <= 1e-12
    names = list(maps)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert float((maps[a] - maps[b]).abs().max()) > 1e-3, (a, b)
    # a NaN feature separates them: XGradCAM drops the whole channel, GradCam one term
    k = int(A.flatten(1).sum(1).argmax())
    A = A.clone()
    A[k, 0, 0] = float("nan")
    assert float((G.closed_low(A, g, "GradCam") - G.closed_low(A, g, "XGradCAM")).abs().max()) > 1e-3


def _stored(c, lay):
    return R.stored(c["A"], lay)


@pytest.mark.parametrize("lay", R.LAYS)
@pytest.mark.parametrize("shape,kind", G.CASES + [(None, "nan_feature"), (None, "nan_position")])
def test_reference_alone_decides_the_uint8_of_every_device_input(shape, kind, lay):
    """On every input of tests/test_x_grad_cam_gpu.py, in every storage form and method, the
    reference and its bound leave at most 0.5 % of the uint8 pixels undecided."""
    if shape is None:
        c, (Ho, Wo) = G.nan_feature_input() if kind == "nan_feature" else G.nan_position_input()
        h, w = c["A"].shape[2:]
    else:
        C, h, w, Ho, Wo = shape
        c = G.gpu_input(C, h, w, kind)
    A64 = _stored(c, lay)
    for method in G.METHODS:
        ref = G.grad_cam_ref(A64, c["w"], c["cls"], Ho, Wo, lay, method)
        excl = 1.0 - float(R.u8_decided(ref["cam"], ref["b_cam"]).double().mean())
        assert excl <= R.U8_EXCLUDED_MAX, (method, excl)
        assert bool(torch.isfinite(ref["b_low"]).all()) and bool(torch.isfinite(ref["cam"]).all())
        print(f"{method} {lay} {kind} {shape}: u8 excluded {excl:.4f}")
        if kind in ("nonpos_row", "nan_position"):
            # frame 0's row is <= 0: every method's map is clamped to zero everywhere; a sum
            # that is not finite: the normalisation zeroes the map
            assert not ref["low"][0].any() and not ref["b_low"][0].any()
            assert bool(ref["low"][1].any()) == (h * w > 1)


def test_exps_cancel_in_the_reference():
    """Features stored times 2^e with the weights times 2^-e: the same maps, exactly."""
    C, h, w, Ho, Wo = G.SHAPES[0]
    c = G.gpu_input(C, h, w, "dead")
    e = G.exps_input(C)
    assert int(e.max()) > 0 and int((e == 0).sum()) > 0
    A64 = R.stored(c["A"], "s2")
    scaled = A64 * torch.pow(2.0, e.double())[None, :, None, None]
    for method in G.METHODS:
        a = G.grad_cam_ref(A64, c["w"], c["cls"], Ho, Wo, "s2", method)
        b = G.grad_cam_ref(scaled, c["w"], c["cls"], Ho, Wo, "s2", method, exps=e)
        assert torch.equal(a["low"], b["low"]) and torch.equal(a["cam"], b["cam"])
        excl = 1.0 - float(R.u8_decided(b["cam"], b["b_cam"]).double().mean())
        assert excl <= R.U8_EXCLUDED_MAX


def test_the_bounds_have_teeth():
    """A map without the ReLU, one with the wrong method and one from the pre-scaled CAM
    weight all leave the bound by orders of magnitude."""
    C, h, w, Ho, Wo = G.SHAPES[0]
    c = G.gpu_input(C, h, w, "mixed_row")
    A64 = R.stored(c["A"], "s3")
    ref = G.grad_cam_ref(A64, c["w"], c["cls"], Ho, Wo, "s3", "GradCam")
    other = G.grad_cam_ref(A64, c["w"], c["cls"], Ho, Wo, "s3", "LayerCAM")
    assert not R.accept(other["low"], ref["low"], ref["b_low"])
    k = int(c["cls"][0])
    raw = torch.nansum(G.hook_gradient(c["w"][k], h * w)[:, None, None] * A64[0], 0)
    no_relu = (raw - raw.min()) / (raw - raw.min()).max()
    assert not R.accept(no_relu, ref["low"][0], ref["b_low"][0])
    assert R.accept(ref["low"].float(), ref["low"], ref["b_low"] + 2.0 ** -24)


# ------------------------------------------------------------------ entry points
def test_the_extractors_are_exported():
    import tcam_wsol_video_amd as T
    from tcam_wsol_video_amd import inference
    for name in ("GradCAM", "GradCAMpp", "XGradCAM", "LayerCAM"):
        assert getattr(T, name) is getattr(inference, name)
    assert [inference.STD_CAM_METHODS[m].method for m in G.METHODS] == G.METHODS
    assert callable(T.build_std_cam_extractor)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("method", ["ScoreCAM", "SmoothGradCAMpp", "SSCAM", "ISCAM", "WILDCAT",
                                    "GAP", "MaxPOL", "LogSumExp"])
def test_std_cl_refuses_the_methods_that_are_not_built(method, train):
    from tcam_wsol_video_amd import runner
    with pytest.raises(SystemExit) as e:
        runner.parser(train=train).parse_args(["--task", "STD_CL", "--method", method])
    assert method in str(e.value) and "not built" in str(e.value)


def test_std_cl_refuses_an_unknown_method_by_name():
    from tcam_wsol_video_amd import runner
    with pytest.raises(SystemExit) as e:
        runner.parser(train=False).parse_args(["--task", "STD_CL", "--method", "gradcam"])
    assert "gradcam" in str(e.value) and "not built" not in str(e.value)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("method", ["CAM"] + G.METHODS)
def test_std_cl_parses_the_built_methods(method, train):
    from tcam_wsol_video_amd import runner
    args = runner.parser(train=train).parse_args(["--task", "STD_CL", "--method", method])
    assert args.method == method


def test_tcam_task_and_the_default_are_unaffected():
    from tcam_wsol_video_amd import runner
    for train in (False, True):
        assert runner.parser(train=train).parse_args([]).method == "CAM"
        assert runner.parser(train=train).parse_args(["--task", "STD_CL"]).method == "CAM"
        # --task TCAM never reads --method: any value parses, as before
        a = runner.parser(train=train).parse_args(["--task", "TCAM", "--method", "ScoreCAM"])
        assert a.method == "ScoreCAM"
    a = runner.parser(train=False).parse_args(["--task", "STD_CL", "--store_std_cams", "d",
                                               "--std_cams_roi_file", "f"])
    assert (a.store_std_cams, a.std_cams_roi_file) == ("d", "f")
    with pytest.raises(SystemExit):
        runner.parser(train=False).parse_args(["--task", "STD_CL", "--std_cams_roi_file", "f"])


def test_camcomputer_refuses_a_method_it_does_not_have():
    from tcam_wsol_video_amd.inference import check_std_cam_method
    assert check_std_cam_method("LayerCAM") == "LayerCAM"
    with pytest.raises(ValueError, match="ScoreCAM"):
        check_std_cam_method("ScoreCAM")
