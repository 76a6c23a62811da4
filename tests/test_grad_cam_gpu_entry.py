"""The stage-1 CAM methods through the entry points (tcam_wsol_video_amd/runner.py) on an
on-disk JPEG dataset of 12 frames per split (train, val, test) in the reference's WSOL
metadata layout: ``eval.py --task STD_CL --method X`` against the oracle's CPU pipeline,
``main.py --task STD_CL --method X`` validating with the same method, ``eval.py
--store_std_cams`` writing the CAM store, and ``main.py --task TCAM --std_cams_folder``
training on it."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grad_cam_ref as G
from oracle import model_ref as R
from tcam_wsol_video_amd import camstore, runner
from tcam_wsol_video_amd import checkpoints as CK
from tcam_wsol_video_amd import frames as FR
from tcam_wsol_video_amd.inference import build_std_cam_extractor
from tcam_wsol_video_amd.models import build_r50_stdcl
from tcam_wsol_video_amd.runner import eval_main, train_main
from tcam_wsol_video_amd.utils.seeding import synthetic_boxes, synthetic_clip
from test_gpu_entrypoints import _oracle_vs_device, _run, _run_collect, _train

pytestmark = pytest.mark.gpu

SPLITS = {"train": 30, "val": 50, "test": 70}      # split -> first clip seed


def _write_split(root, split, seed0, n_shots=2, n_frames=6):
    """As test_gpu_entrypoints._write_dataset, one split with its own shots."""
    from PIL import Image
    meta = os.path.join(root, "meta", split)
    os.makedirs(meta)
    lines = {"image_ids": [], "class_labels": [], "image_sizes": [], "localization": []}
    for s in range(n_shots):
        clip = synthetic_clip(n_frames, seed=seed0 + s)
        boxes = synthetic_boxes(clip, 480)
        for t in range(n_frames):
            i = f"car/data/{split}{s:04d}/shots/001/frame{t:04d}.jpg"
            path = os.path.join(root, "frames", i)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            Image.fromarray(clip[t]).save(path, quality=95)
            x0, y0, x1, y1 = boxes[t]
            lines["image_ids"].append(i)
            lines["class_labels"].append(f"{i},{3 + s}")
            lines["image_sizes"].append(f"{i},480,360")
            lines["localization"].append(f"{i},{x0 + 0.25},{y0 * 360 / 480 + 0.5},"
                                         f"{x1 - 0.25},{y1 * 360 / 480}")
    for k, v in lines.items():
        with open(os.path.join(meta, k + ".txt"), "w") as f:
            f.write("\n".join(v) + "\n")
    return lines["image_ids"]


@pytest.fixture(scope="module")
def data(tmp_path_factory, cuda):
    root = str(tmp_path_factory.mktemp("gradcam_entry"))
    ids = {s: _write_split(root, s, seed0) for s, seed0 in SPLITS.items()}
    model = build_r50_stdcl(seed=13)
    best = os.path.join(root, "best")
    CK.save_best_model(model, "STD_CL", best, 4)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    return dict(root=root, meta=os.path.join(root, "meta"), frames=os.path.join(root, "frames"),
                ids=ids, best=best, sd=sd, feats={})


def _base(d, *more):
    return ["--task", "STD_CL", "--metadata_root", d["meta"], "--data_root", d["frames"],
            "--batch_size", "5"] + list(more)


def _metrics(r):
    return {k: v for k, v in r.items() if not k.startswith("frames_per_s")}


@pytest.mark.parametrize("method", ["LayerCAM", "GradCam"])
def test_eval_std_cl_method_matches_oracle(cuda, data, method):
    """eval.py --task STD_CL --method X: every fp32 CAM within 1e-4 of the fp64 method
    (tests/grad_cam_ref.py) on the oracle's features of the same file, resized as
    inference_wsol.py:342-346; the oracle evaluator fed the device's uint8 CAMs reproduces
    the counters exactly."""
    outs, got = _run_collect(eval_main, _base(data, "--splits", "test", "--checkpoint",
                                              data["best"], "--cam_curve_interval", "0.01",
                                              "--method", method))
    res = outs[0]["results"]["test"]
    assert outs[0]["task"] == "STD_CL" and res["frames"] == 12
    sd, feats = data["sd"], data["feats"]
    fw = sd["classification_head.fc.weight"]

    def cam_fn(x, label):
        key = hash(x.numpy().tobytes())
        if key not in feats:                      # one oracle forward per frame, both methods
            feats[key] = R.stdcl_forward(sd, x)[1][0].double()
        A = feats[key]
        g = G.hook_gradient(fw[label], A.shape[1] * A.shape[2])
        low = G.final_low(G.closed_low(A, g, method))
        return F.interpolate(low[None, None], (224, 224), mode="bilinear",
                             align_corners=False)[0, 0].numpy()
    _oracle_vs_device(data["meta"], data["frames"], got, res, cam_fn)


def test_main_std_cl_validates_with_the_method(cuda, data, tmp_path):
    """main.py --task STD_CL --method LayerCAM --max_epochs 0: the validation that selects
    best_loc is eval.py's with the same method on the same seeded model, and not CAM's."""
    common = ["--arch", "STDClassifier", "--freeze_cl", "False", "--max_epochs", "0",
              "--final_test_eval", "False"]
    val = {}
    for method in ("LayerCAM", "CAM"):
        logs = _train(_base(data, "--method", method, "--exp_path",
                            str(tmp_path / method), *common))
        assert len(logs) == 1 and logs[0]["epoch"] == 0
        val[method] = _metrics(logs[0]["val"])
    assert val["LayerCAM"]["frames"] == 12 and val["LayerCAM"]["cam_curve_interval"] == 0.004
    ev = _run(eval_main, _base(data, "--splits", "val", "--method", "LayerCAM",
                               "--cam_curve_interval", "0.004"))[0]["results"]["val"]
    assert _metrics(ev) == val["LayerCAM"]
    assert val["LayerCAM"] != val["CAM"]


def test_store_std_cams_feeds_tcam(cuda, data, tmp_path):
    """eval.py --store_std_cams DIR --std_cams_roi_file FILE: one 2-D fp32 CPU tensor per
    frame of every split, bit-equal to the extractor's low-resolution map of the frame's
    label, readable by camstore.load_std_cams, one ROI line per id; then one epoch of main.py
    --task TCAM --std_cams_folder DIR ends with finite losses."""
    store, roi = str(tmp_path / "cams"), str(tmp_path / "roi.txt")
    out = _run(eval_main, _base(data, "--splits", "train,val,test", "--checkpoint", data["best"],
                                "--method", "LayerCAM", "--store_std_cams", store,
                                "--std_cams_roi_file", roi))
    assert len(out) == 1 and out[0]["frames"] == 36 and out[0]["method"] == "LayerCAM"
    assert out[0]["frames_per_split"] == {"train": 12, "val": 12, "test": 12}
    all_ids = [i for s in SPLITS for i in data["ids"][s]]
    assert sorted(os.listdir(store)) == sorted(camstore.reformat_id(i) + ".pt" for i in all_ids)
    th = camstore.load_roi_thresholds(roi)
    assert list(th) == all_ids and all(0.0 <= v <= 1.0 for v in th.values())
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("roi.txt.")]
    # the same batches through the extractor
    args = runner.parser(train=False).parse_args(_base(data, "--method", "LayerCAM"))
    model = build_r50_stdcl()
    CK.load_best_model(model, "STD_CL", data["best"])
    model = model.to(cuda).eval()
    ext = build_std_cam_extractor(model, args)
    split = runner.Split.from_metadata(os.path.join(data["meta"], "val"), data["frames"], 224)
    tf = FR.get_eval_tranforms(224)
    for k in range(0, 12, 5):
        ids = split.ids[k:k + 5]
        x, _ = runner.device_frames(split, ids, cuda, tf)
        with torch.no_grad():
            scores = model(x)
        low = ext([split.labels[i] for i in ids], scores).cpu()
        cams = camstore.load_std_cams(store, ids)
        assert cams.shape == (len(ids), 1, 28, 28) and cams.dtype == torch.float32
        assert torch.equal(cams[:, 0].view(torch.int32), low.view(torch.int32))
        one = torch.load(camstore.get_cams_paths(store, ids)[ids[0]], weights_only=True)
        assert one.ndim == 2 and one.dtype == torch.float32 and one.device.type == "cpu"
        assert float(one.max()) == 1.0 and float(one.min()) == 0.0
    # stage 2 on the store
    logs = _train(["--metadata_root", data["meta"], "--data_root", data["frames"],
                   "--batch_size", "6", "--max_epochs", "1", "--exp_path", str(tmp_path / "exp"),
                   "--checkpoint_save", "100", "--std_cams_folder", store,
                   "--std_cams_thresh_file", roi, "--final_test_eval", "False",
                   "--cam_curve_interval", "0.01"])
    assert [lg["epoch"] for lg in logs] == [0, 1]
    assert len(logs[1]["losses"]) >= 3 and bool(np.isfinite(logs[1]["losses"]).all())
