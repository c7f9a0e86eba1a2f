"""Times the detection post-processing (dtc_postprocess_detections_ex2) per option set at the bench's shape: pipeline.synthetic_batch
(B = 8, R = 1000, 81 classes), its class probabilities handed over as LOGITS (log p: the kernel's softmax gives p back, so the
candidates are the bench's), rois drawn like the proposals.

    python tools/bench_det_options.py [--iters 100] [--warmup 20] [--host-images 8]

One JSON line per mode (hard, hard+vote, linear, gaussian, linear+vote, and hard+vote / linear+vote with each scoring other than 'ID':
the vote-scoring launch ahead of the limit): the median of --iters launches of the whole entry (HIP events around each), plus the
candidates per (class, image) segment (mean / max: the Soft-NMS walk is O(n^2) per segment).  Last lines: the host-loop baselines --
what result_utils.box_results_with_nms_and_limit ran before the batched path, the reference's 80-iteration per-class loop on the
single-segment kernels (one launch and one copy back per class), reproduced below, over the same images' decoded boxes: with
do_soft_nms=True, and with hard NMS + a vote scored IOU_AVG."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectorch_amd import hip, synth  # noqa: E402
from detectorch_amd.pipeline import synthetic_batch  # noqa: E402
from detectorch_amd.utils import boxes as box_utils  # noqa: E402

MODES = [("hard", {}), ("hard+vote", dict(do_bbox_vote=True)), ("linear", dict(do_soft_nms=True, soft_nms_method="linear")),
         ("gaussian", dict(do_soft_nms=True, soft_nms_method="gaussian")),
         ("linear+vote", dict(do_soft_nms=True, soft_nms_method="linear", do_bbox_vote=True))]
MODES += [("%s:%s" % (name, m), dict(kw, bbox_vote_method=m)) for m in ("TEMP_AVG", "AVG", "IOU_AVG", "GENERALIZED_AVG", "QUASI_SUM")
          for name, kw in MODES if name.endswith("+vote")]


def host_loop(scores, boxes, num_classes=81, score_thresh=0.05, overlap_thresh=0.5, vote_method=None):
    """the per-class loop box_results_with_nms_and_limit ran before the batched path (result_utils.py:126-165): do_soft_nms=True,
    or (vote_method) hard NMS + box_voting(scoring_method=vote_method) at 0.8"""
    cls_boxes = [[] for _ in range(num_classes)]
    for j in range(1, num_classes):
        inds = np.where(scores[:, j] > score_thresh)[0]
        dets_j = np.hstack((boxes[inds, j * 4:(j + 1) * 4], scores[inds, j][:, np.newaxis])).astype(np.float32, copy=False)
        if vote_method is None:
            nms_dets, _ = box_utils.soft_nms(dets_j, sigma=0.5, overlap_thresh=overlap_thresh, score_thresh=0.0001, method="linear")
        else:
            nms_dets = dets_j[box_utils.nms(dets_j, overlap_thresh), :]
            if len(nms_dets):
                nms_dets = box_utils.box_voting(nms_dets, dets_j, 0.8, scoring_method=vote_method)
        cls_boxes[j] = nms_dets
    image_scores = np.hstack([cls_boxes[j][:, -1] for j in range(1, num_classes)])
    if len(image_scores) > 100:
        th = np.sort(image_scores)[-100]
        for j in range(1, num_classes):
            cls_boxes[j] = cls_boxes[j][cls_boxes[j][:, -1] >= th]
    return np.vstack([cls_boxes[j] for j in range(1, num_classes)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = 8
    _, _, _, probs, bbox, _, sf, im = synthetic_batch(B, dev, seed=4000)
    logits = torch.log(probs).contiguous()
    R, ncls = logits.shape[1], logits.shape[2]
    rs = synth.rng(40, 0)
    rois = torch.from_numpy(np.stack([np.hstack([np.full((R, 1), b, np.float32), synth.make_rois(rs, R)]) for b in range(B)])).to(dev)
    cand = (probs[:, :, 1:] > 0.05).sum(1).float()                          # [B, 80] candidates per segment
    seg = dict(cand_mean=round(float(cand.mean()), 1), cand_max=int(cand.max()))
    for name, kw in MODES:
        kw = dict(kw)
        scoring = hip.vote_scoring(kw.pop("bbox_vote_method", "ID"))
        opt = hip.det_options(**kw)
        ws = hip.workspace(hip.det_workspace_bytes(B, R, ncls, opt, scoring=scoring), dev)
        out = hip.det_outputs(B, 128, dev)
        st = hip.stream_ptr(dev)

        def launch():
            hip.call("dtc_postprocess_detections_ex2", name, rois5=rois, n_rois=None, cls_score=logits, scores_are_logits=1, bbox_pred=bbox,
                     decoded_boxes=None, scaling_factor=sf, im_size=im, batch=B, max_rois=R, n_cls=ncls, wx=10., wy=10., ww=5., wh=5.,
                     score_thresh=.05, nms_thresh=.5, max_det=100, opt=opt, scoring=scoring, workspace=ws, workspace_bytes=ws.numel(),
                     max_out=128, fpn=None, stream=st, **out)
        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        print(json.dumps(dict(mode=name, median_us=round(statistics.median(ts), 1), min_us=round(min(ts), 1), iters=a.iters, batch=B,
                              rois=R, classes=ncls, dets_per_image=out["det_count"].tolist(), **seg)), flush=True)
    # host-loop baseline: decoded boxes of the same images, the old per-class loop (one single-segment launch + sync per class)
    n = min(a.host_images, B)
    dec = [hip.bbox_transform(rois[b, :, 1:] / sf[b], bbox[b], (10., 10., 5., 5.), clip_to=(float(im[b, 0]), float(im[b, 1])))
           for b in range(n)]
    host = [(probs[b].cpu().numpy(), dec[b].cpu().numpy()) for b in range(n)]
    for mode, vm in (("host_loop_linear", None), ("host_loop_hard+vote:IOU_AVG", "IOU_AVG")):
        host_loop(*host[0], vote_method=vm)                                 # warm-up
        t0 = time.perf_counter()
        for s, bx in host:
            host_loop(s, bx, vote_method=vm)
        t_host = (time.perf_counter() - t0) * 1e6
        print(json.dumps(dict(mode=mode, images=n, total_us=round(t_host, 1), per_batch_of_8_us=round(t_host * 8 / n, 1))), flush=True)


if __name__ == "__main__":
    main()
