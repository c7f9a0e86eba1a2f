"""The time of the two test-time-augmentation kernels at the workload shape, on the device (tests/README_tta.md records the numbers;
neither is a threshold of a test):

    python tools/tta_timing.py [--launches 200]

  merge    dtc_aug_merge_boxes, B = 8 images, T = 4 views (flags 1, 0, 1, 0), R = 1000 rois, 81 classes, logits in, UNION
  combine  dtc_aug_combine_masks, 8 x 128 rows of 81 x 28 x 28, T = 4 views, every row live; with mask_class (one channel of a row is
           combined, the others are written as zeros) and without (every channel), SOFT_AVG and LOGIT_AVG

Each figure is the mean over --launches back-to-back launches between two device events, after a warm-up of 20, so it includes the
launch gap of an eager stream; the bytes are the ones the rule needs (read once, written once), computed from the shapes.  Prints one
JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectorch_amd import hip_aug  # noqa: E402

B, T, R, N_CLS, MAX_OUT, M = 8, 4, 1000, 81, 128, 28


def timed(fn, launches):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches                       # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tta_timing needs the GPU: a time taken anywhere else says nothing")
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    rn = lambda *s: torch.randn(s, generator=g, device="cuda")
    im_size = torch.tensor([[500.0, 833.0]] * B, device="cuda")
    views = []
    for t in range(T):
        xy = torch.rand((B, R, 2), generator=g, device="cuda") * torch.tensor([700.0, 400.0], device="cuda")
        wh = torch.rand((B, R, 2), generator=g, device="cuda") * 300 + 8
        rois5 = torch.cat([torch.arange(B, device="cuda", dtype=torch.float32)[:, None, None].expand(B, R, 1), xy, xy + wh], 2).contiguous()
        views.append(dict(rois5=rois5, n_rois=torch.full((B,), R, dtype=torch.int32, device="cuda"), cls_score=rn(B, R, N_CLS) * 2,
                          bbox_pred=rn(B, R, 4 * N_CLS) * 0.1, scale=torch.full((B,), 1.6, device="cuda"), flipped=t % 2 == 0))
    out = hip_aug.merge_outputs(B, T * R, N_CLS, "cuda")
    res = {}
    us = timed(lambda: hip_aug.merge_boxes(views, im_size, scores_are_logits=True, out=out), args.launches)
    nbytes = B * T * R * ((5 + N_CLS + 4 * N_CLS) * 4 + (N_CLS + 4 * N_CLS + 1) * 4)
    res["merge_us"], res["merge_GBps"] = round(us, 1), round(nbytes / us / 1e3, 1)
    masks = [torch.rand((B * MAX_OUT, N_CLS, M, M), generator=g, device="cuda") for _ in range(T)]
    cnt = torch.full((B,), MAX_OUT, dtype=torch.int32, device="cuda")
    mc = torch.randint(1, N_CLS, (B * MAX_OUT,), generator=g, device="cuda", dtype=torch.int32)
    mo = torch.empty_like(masks[0])
    flips = [t % 2 == 0 for t in range(T)]
    plane = B * MAX_OUT * M * M * 4
    for heur in ("SOFT_AVG", "LOGIT_AVG"):
        us = timed(lambda: hip_aug.combine_masks(masks, flips, cnt, mc, heur, out=mo), args.launches)
        res["combine_class_%s_us" % heur], res["combine_class_%s_GBps" % heur] = round(us, 1), round((T * plane + N_CLS * plane) / us / 1e3, 1)
        us = timed(lambda: hip_aug.combine_masks(masks, flips, cnt, None, heur, out=mo), args.launches)
        res["combine_all_%s_us" % heur], res["combine_all_%s_GBps" % heur] = round(us, 1), round((T + 1) * N_CLS * plane / us / 1e3, 1)
    print(json.dumps(dict(shape=dict(B=B, T=T, R=R, n_cls=N_CLS, mask_rows=B * MAX_OUT, M=M), launches=args.launches, **res)))


if __name__ == "__main__":
    main()
