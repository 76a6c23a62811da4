"""bench.dump_outputs on the CPU: what --dump-outputs writes for a clip held by a stand-in
CAMComputer — names, dtypes, the 64 MB bound and the fixed, seeded frame choice of a clip too
large for it."""
import os
from types import SimpleNamespace

import numpy as np
import torch

import bench


def _comp(b, h=224, w=224, classes=10):
    g = torch.Generator().manual_seed(b)
    cam = torch.rand(b, h, w, generator=g)
    ev = SimpleNamespace(counters=torch.arange(3 * 3 * 7, dtype=torch.int32).view(3, 3, 7),
                         cls_correct=torch.tensor([b], dtype=torch.int32))
    comp = SimpleNamespace(evaluator=ev, last_cam=cam,
                           last_logits=torch.randn(b, classes, generator=g))
    return comp, (cam * 255).to(torch.uint8)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_clip_is_written_whole(tmp_path):
    comp, u8 = _comp(5, 32, 24)
    bench.dump_outputs(str(tmp_path / "o"), comp, u8)
    got = _load(str(tmp_path / "o"))
    assert sorted(got) == ["box_counters", "cam", "cam_u8", "cls_correct", "frames", "logits"]
    assert {k: v.dtype for k, v in got.items()} == {
        "box_counters": np.float64, "cls_correct": np.float64, "frames": np.float64,
        "cam": np.float32, "cam_u8": np.float32, "logits": np.float32}
    np.testing.assert_array_equal(got["frames"], np.arange(5))
    np.testing.assert_array_equal(got["cam"], comp.last_cam.numpy())
    np.testing.assert_array_equal(got["cam_u8"], u8.numpy().astype(np.float32))
    np.testing.assert_array_equal(got["logits"], comp.last_logits.numpy())
    np.testing.assert_array_equal(got["box_counters"], comp.evaluator.counters.numpy())
    np.testing.assert_array_equal(got["cls_correct"], [5.0])


def test_large_clip_is_cut_to_a_fixed_sample_within_64_mb(tmp_path):
    comp, u8 = _comp(300)                      # 2 x 300 x 224 x 224 x 4 B = 120 MB whole
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), comp, u8)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    size = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert size <= 64 << 20
    idx = a["frames"].astype(np.int64)
    assert 1 <= len(idx) < 300 and np.all(np.diff(idx) > 0) and idx[-1] < 300
    np.testing.assert_array_equal(a["cam"], comp.last_cam.numpy()[idx])
    np.testing.assert_array_equal(a["cam_u8"], u8.numpy()[idx].astype(np.float32))
    np.testing.assert_array_equal(a["logits"], comp.last_logits.numpy()[idx])
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
