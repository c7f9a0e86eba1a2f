"""The wall time of scoring a synthetic set of instance masks on the device, next to the numpy restatement's
(tests/README_segm_eval.md records both; neither is a threshold of a test):

    python tools/segm_eval_timing.py [--images 5000] [--batch 50] [--ref-images 200]

The set: --images images of 800 x 1333 with 100 detections over 81 classes and 2 to 12 gt; boxes are synth's (log-uniform sides
16-600 px), six detections in ten are a gt's box moved by a few pixels; every mask, detections and gt alike, is one of synth's 28 x 28
blobs pasted into its box and run-length-encoded by the project's own kernels (hip.mask_paste, hip.mask_rle), so the run lists are
what the inference path leaves on the device.  Device: MaskEvaluator.update over all batches plus accumulate(), inputs already on
the device, after one warm-up pass.  Restatement: tests/segm_eval_ref.py (bitmaps) on the first --ref-images images, scaled to the
whole set; the same slice on the device must give the same bits.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from detectorch_amd import hip, synth  # noqa: E402
from detectorch_amd.utils.evaluator import MaskEvaluator  # noqa: E402

M, NUM_CLASSES, N_DET, G = 28, 81, 100, 16
CAPACITY, RUNS_STRIDE = 40 << 20, 8192                       # crop bytes per image (100 boxes of up to 600 x 600), runs per mask at first


def encode(rs, boxes, classes, counts, im_size):
    """boxes [B,D,4], classes [B,D], counts [B] -> (run lengths int32 [B,D,stride'], n_runs int32 [B,D]) on the device: a blob per box,
    pasted and encoded by the project's kernels; stride': the longest list of the batch"""
    B, D = boxes.shape[:2]
    dets = np.zeros((B, D, 6), np.float32)
    dets[:, :, :4], dets[:, :, 5] = boxes, classes
    masks = torch.from_numpy(synth.make_masks(rs, B * D, 1, M)).cuda()
    count = torch.from_numpy(counts).cuda()
    paste = hip.mask_paste(masks, torch.from_numpy(dets).cuda(), count, im_size, M, CAPACITY, cls_specific=False)
    if int(paste["bytes"].max()) > CAPACITY:                                     # paste again with the capacity it asks for
        paste = hip.mask_paste(masks, torch.from_numpy(dets).cuda(), count, im_size, M, int(paste["bytes"].max()), cls_specific=False)
    rle = hip.mask_rle(paste, count, im_size, runs_stride=RUNS_STRIDE, str_stride=16)      # the strings are not needed
    if int(rle["n_runs"].min()) < 0:                                             # a noisy tall mask: encode again with the stride it asks for
        rle = hip.mask_rle(paste, count, im_size, runs_stride=8 - int(rle["n_runs"].min()), str_stride=16)
    n_runs = rle["n_runs"]
    longest = max(int(n_runs.max()), 1)
    return rle["counts"][:, :, :longest].contiguous(), n_runs


def make_set(n_images, batch):
    """-> the batches, each a dict of device tensors: dets, det_count, rle (counts, n_runs), im_size, gt"""
    rs = synth.rng(10, 0)
    out = []
    for i0 in range(0, n_images, batch):
        B = min(batch, n_images - i0)
        im_size = torch.tensor([[float(synth.IM_H), float(synth.IM_W)]] * B, device="cuda")
        gt_boxes, gt_classes = np.zeros((B, G, 4), np.float32), np.zeros((B, G), np.int32)
        gt_is_crowd, gt_counts = np.zeros((B, G), np.int32), rs.randint(2, 13, B).astype(np.int32)
        dets = np.zeros((B, N_DET, 6), np.float32)
        for n in range(B):
            g = int(gt_counts[n])
            gt_boxes[n, :g] = synth.make_rois(rs, g)
            gt_classes[n, :g] = rs.randint(1, NUM_CLASSES, g)
            gt_is_crowd[n, :g] = rs.rand(g) < 0.05
            near = rs.rand(N_DET) < 0.6
            src = rs.randint(0, g, N_DET)
            boxes = np.where(near[:, None], gt_boxes[n, src] + rs.randint(-8, 9, (N_DET, 4)), synth.make_rois(rs, N_DET))
            boxes[:, 0::2], boxes[:, 1::2] = np.clip(boxes[:, 0::2], 0, synth.IM_W - 1), np.clip(boxes[:, 1::2], 0, synth.IM_H - 1)
            cls = np.where(near & (rs.rand(N_DET) < 0.85), gt_classes[n, src], rs.randint(1, NUM_CLASSES, N_DET))
            order = np.argsort(cls, kind="stable")                               # class-major rows, as the detection stage writes them
            dets[n, :, :4], dets[n, :, 5] = boxes[order], cls[order]
            dets[n, :, 4] = rs.rand(N_DET).astype(np.float32)
        det_count = np.full(B, N_DET, np.int32)
        gt_runs, gt_n_runs = encode(rs, gt_boxes, gt_classes, gt_counts, im_size)
        counts, n_runs = encode(rs, dets[:, :, :4], dets[:, :, 5], det_count, im_size)
        t = lambda a: torch.from_numpy(a).cuda()
        out.append(dict(dets=t(dets), det_count=t(det_count), rle=dict(counts=counts, n_runs=n_runs), im_size=im_size,
                        gt=dict(gt_runs=gt_runs, gt_n_runs=gt_n_runs, gt_classes=t(gt_classes), gt_is_crowd=t(gt_is_crowd),
                                gt_counts=t(gt_counts))))
    return out


def device_pass(batches):
    ev = MaskEvaluator(num_classes=NUM_CLASSES)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in batches:
        ev.update(b["dets"], b["det_count"], b["rle"], b["im_size"], b["gt"])
    res = ev.accumulate()
    return time.perf_counter() - t0, res


def host_case(batches, n):
    """the first n images as a case of tests/segm_eval_ref.py"""
    import coco_eval_ref as cr
    take, left = [], n
    for b in batches:
        if left <= 0:
            break
        take.append((b, min(left, b["dets"].shape[0])))
        left -= take[-1][1]
    cat = lambda f: np.concatenate([f(b)[:k].cpu().numpy() for b, k in take])

    def cat_runs(f):                                                             # the batches have strides of their own: pad to the longest
        parts = [f(b)[:k].cpu().numpy() for b, k in take]
        stride = max(p.shape[2] for p in parts)
        return np.concatenate([np.pad(p, ((0, 0), (0, 0), (0, stride - p.shape[2]))) for p in parts]).view(np.uint32)

    iou_thrs, rec_thrs, max_dets, area_rngs = cr.coco_params()
    return dict(dets=cat(lambda b: b["dets"]), det_count=cat(lambda b: b["det_count"]), im_size=cat(lambda b: b["im_size"]),
                det_runs=cat_runs(lambda b: b["rle"]["counts"]), det_n_runs=cat(lambda b: b["rle"]["n_runs"]),
                gt_runs=cat_runs(lambda b: b["gt"]["gt_runs"]), gt_n_runs=cat(lambda b: b["gt"]["gt_n_runs"]),
                gt_classes=cat(lambda b: b["gt"]["gt_classes"]), gt_is_crowd=cat(lambda b: b["gt"]["gt_is_crowd"]),
                gt_counts=cat(lambda b: b["gt"]["gt_counts"]), num_classes=NUM_CLASSES, iou_thrs=iou_thrs, rec_thrs=rec_thrs,
                max_dets=max_dets, area_rngs=area_rngs), take


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--ref-images", type=int, default=200)
    args = ap.parse_args()
    t0 = time.perf_counter()
    batches = make_set(args.images, args.batch)
    torch.cuda.synchronize()
    made = time.perf_counter() - t0
    n_runs = torch.cat([b["rle"]["n_runs"].reshape(-1) for b in batches])
    device_pass(batches)                                                         # warm-up: library load, allocator
    times = [device_pass(batches) for _ in range(3)]
    out = dict(images=args.images, batch=args.batch, make_set_seconds=round(made, 1), device_seconds=[round(t, 4) for t, _ in times],
               AP=float(times[0][1]["stats"][0]), det_runs_mean=round(float(n_runs.float().mean()), 1), det_runs_max=int(n_runs.max()),
               masks_that_did_not_fit=int((n_runs < 0).sum()))
    if args.ref_images:
        import segm_eval_ref as sr
        case, take = host_case(batches, min(args.ref_images, args.images))
        n = len(case["dets"])
        t0 = time.perf_counter()
        ref = sr.run(case)
        dt = time.perf_counter() - t0
        ev = MaskEvaluator(num_classes=NUM_CLASSES)                               # the same slice on the device: the same bits
        for b, k in take:
            ev.update(b["dets"][:k], b["det_count"][:k], {x: v[:k] for x, v in b["rle"].items()}, b["im_size"][:k],
                      {x: v[:k] for x, v in b["gt"].items()})
        dev = ev.accumulate()
        same = all(dev[k].tobytes() == ref[k].tobytes() for k in ("precision", "recall", "stats"))
        iou = np.concatenate([r["iou"].cpu().numpy() for r in ev._records])
        out.update(ref_images=n, ref_seconds=round(dt, 2), ref_seconds_scaled=round(dt * args.images / n, 1), ref_AP=float(ref["stats"][0]),
                   slice_bit_equal=bool(same), slice_iou_bit_equal=bool(iou.tobytes() == ref["iou"].tobytes()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
