"""Time the stage-1 CAM methods on the device, in one run:

* the four gradient methods (tcam_grad_cam_s2) and CAM (tcam_std_cam_s2) on S2 features of
  32 x 2048 x 28 x 28 (the ResNet50 hook at 224^2, one clip) resized to 224^2, fp32 CAM and
  uint8 out: device events around ``reps`` calls after a warm-up, the calls alternating
  between the methods so that each sees the same machine state;
* STD_CL evaluation (CAMComputer: forward + CAM + bbox sweep + counters) in frames / s per
  method on seeded ResNet50 weights and synthetic clips.

Prints one JSON line.  Needs an MI355X; reported, not gated."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tcam_wsol_video_amd import ops  # noqa: E402
from tcam_wsol_video_amd.inference import STD_CAM_METHODS, CAMComputer  # noqa: E402
from tcam_wsol_video_amd.models import build_r50_stdcl  # noqa: E402
from tcam_wsol_video_amd.utils.seeding import synthetic_clip  # noqa: E402


def kernel_times(dev, B, C, hw, out, reps, rounds):
    g = torch.Generator().manual_seed(0)
    A = torch.relu(torch.randn(B, C, hw, hw, generator=g))
    A = A * (torch.rand(B, C, hw, hw, generator=g) < 0.05)      # sparse, as layer4's features
    As = ops.s3_from_nchw(A.to(dev).contiguous(), None, "f16x3")
    fw = (torch.randn(10, C, generator=g) * 0.05).to(dev)
    cls = torch.arange(B, device=dev, dtype=torch.int32) % 10

    def call(m):
        if m == "CAM":
            return ops.std_cam(As, fw, cls, (out, out))
        return ops.grad_cam(As, fw, cls, (out, out), m)
    methods = list(STD_CAM_METHODS)
    for m in methods:
        for _ in range(3):
            call(m)
    torch.cuda.synchronize()
    ms = {m: [] for m in methods}
    for _ in range(rounds):
        for m in methods:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call(m)
            e1.record()
            torch.cuda.synchronize()
            ms[m].append(e0.elapsed_time(e1) / reps)
    feat_bytes = B * C * hw * hw * 4          # S2: 32 B per 8-channel group
    res = {}
    for m in methods:
        best = min(ms[m])
        passes = 2 if m == "XGradCAM" else 1
        res[m] = {"ms_min": round(best, 4), "ms_max": round(max(ms[m]), 4),
                  "feature_GB_per_s": round(passes * feat_bytes / best / 1e6, 1)}
    return res


def eval_rates(dev, clips, frames, size):
    model = build_r50_stdcl(seed=1234).to(dev)
    data = []
    for k in range(clips):
        clip = synthetic_clip(frames, seed=40 + k, height=size, width=size)
        x = ((torch.from_numpy(clip).float().permute(0, 3, 1, 2) / 255.0 - 0.45) / 0.225)
        gen = torch.Generator().manual_seed(k)
        lo = torch.randint(0, size // 2, (frames, 1, 2), generator=gen)
        gt = torch.cat([lo, lo + torch.randint(20, size // 2, (frames, 1, 2), generator=gen)], 2)
        data.append((x.contiguous().to(dev), torch.randint(0, 10, (frames,), generator=gen).to(dev),
                     gt.to(torch.int32).to(dev)))
    res = {}
    for m in STD_CAM_METHODS:
        for timed in (False, True):            # the first pass warms every shape up
            comp = CAMComputer(model, cam_curve_interval=0.001, device=dev, fwd_streams=2,
                               method=m)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for x, y, gt in data:
                comp.evaluate_batch(x, y, gt)
            comp.compute_and_evaluate()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        res[m] = round(clips * frames / dt, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--channels", type=int, default=2048)
    ap.add_argument("--hw", type=int, default=28)
    ap.add_argument("--out", type=int, default=224)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clips", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cam_methods.py measures on the GPU only")
    dev = torch.device("cuda:0")
    out = {"shape": [a.batch, a.channels, a.hw, a.hw, a.out],
           "kernels": kernel_times(dev, a.batch, a.channels, a.hw, a.out, a.reps, a.rounds),
           "eval_frames_per_s": eval_rates(dev, a.clips, a.batch, a.out)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
