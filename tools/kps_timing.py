"""The time of dtc_kps_heatmaps_to_keypoints at the workload shape, on the device (tests/README_keypoints.md records the numbers;
none is a threshold of a test):

    python tools/kps_timing.py [--launches 200]

  B = 8 images x 100 live rows (max_out = 128), K = 17 keypoints, S = 56, boxes drawn like person detections on an 800 x 1333 image:
  heights 60 .. 700, widths 0.3 .. 0.6 of the height, every row of the person class.

The figure is the mean over --launches back-to-back calls (three kernels each) between two device events, after a warm-up of 20, so it
includes the launch gaps of an eager stream; the pixel rate is the number of resized values the rule defines (sum over the live rows
of K Hr Wr, computed from the boxes) over that time -- each is evaluated twice, once for the maximum and once for the sum.  Prints one
JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectorch_amd import hip_kps  # noqa: E402

B, LIVE, MAX_OUT, K, S = 8, 100, 128, 17, 56
IM_H, IM_W = 800, 1333


def person_boxes(rs):
    dets = np.zeros((B, MAX_OUT, 6), np.float32)
    h = rs.uniform(60, 700, (B, LIVE))
    w = h * rs.uniform(0.3, 0.6, (B, LIVE))
    x1, y1 = rs.uniform(0, IM_W - w), rs.uniform(0, IM_H - h)
    dets[:, :LIVE, 0], dets[:, :LIVE, 1], dets[:, :LIVE, 2], dets[:, :LIVE, 3] = x1, y1, x1 + w, y1 + h
    dets[:, :LIVE, 4], dets[:, :LIVE, 5] = 0.9, 1
    return dets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kps_timing needs the GPU: a time taken anywhere else says nothing")
    dets = person_boxes(np.random.RandomState(0))
    wr = np.ceil(np.maximum(dets[:, :LIVE, 2] - dets[:, :LIVE, 0], 1))
    hr = np.ceil(np.maximum(dets[:, :LIVE, 3] - dets[:, :LIVE, 1], 1))
    pixels = int((wr * hr).sum()) * K
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    heat = torch.randn((B * MAX_OUT, K, S, S), generator=g, device="cuda") * 3
    d, cnt = torch.from_numpy(dets).cuda(), torch.full((B,), LIVE, dtype=torch.int32, device="cuda")
    out, ws = hip_kps.keypoint_outputs(B, MAX_OUT, K, "cuda"), hip_kps.workspace(B, MAX_OUT, K, "cuda")
    fn = lambda: hip_kps.heatmaps_to_keypoints(heat, d, cnt, person_class=1, out=out, ws=ws)
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / args.launches
    assert int((out["kp_status"] == 1).sum()) == B * LIVE
    print(json.dumps(dict(shape=dict(B=B, live_rows=LIVE, max_out=MAX_OUT, K=K, S=S), launches=args.launches, resized_pixels=pixels,
                          call_us=round(us, 1), Gpixel_per_s=round(pixels / us / 1e3, 2))))


if __name__ == "__main__":
    main()
