"""The wall time of mask NMS and mask voting on a synthetic set of instance masks on the device, next to the numpy restatement's on a
small slice (tests/README_mask_post.md records both; neither is a threshold of a test):

    python tools/mask_post_timing.py [--images 500] [--batch 50] [--ref-dets 20]

The set: --images images of 800 x 1333 with 100 detections over 81 classes -- boxes are synth's (log-uniform sides 16-600 px), six in
ten crowd around a dozen centres --, plus, per detection, its duplicate from a second (mirrored and mapped back) pass: the same blob
in the box moved by up to 4 pixels, the score scaled by 0.9.  Every mask is one of synth's 28 x 28 blobs pasted into its box and
run-length-encoded by the project's own kernels (hip.mask_paste, hip.mask_rle): the run lists are what the inference path leaves on
the device.  Per batch, on the device and without a sync: the overlaps of the pool of A = 200 masks with itself and the IOU walk at
0.5 (utils.segms.rle_mask_nms_batched), the first T = 100 kept rows gathered as tops, their overlaps with the pool and the AVG vote
at iou_thresh 0.5, binarize_thresh 0.5 (rle_mask_voting_batched).  Wall time over all batches, three passes after a warm-up.
Restatement: tests/mask_post_ref.py (bitmaps) on the first --ref-dets detections of the first image and their duplicates; the same
slice on the device must give the same bits.
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
from detectorch_amd.utils import segms  # noqa: E402

M, NUM_CLASSES, N_DET, T = 28, 81, 100, 100
CAPACITY, RUNS_STRIDE = 80 << 20, 8192                       # crop bytes per image (200 boxes of up to 600 x 600), runs per mask at first
NMS_THRESH, IOU_THRESH, BINARIZE_THRESH = 0.5, 0.5, 0.5


def encode(masks, dets, im_size):
    """dets [B,A,6] -> (run lengths int32 [B,A,stride'], n_runs int32 [B,A]) on the device: blob k pasted into box k and encoded by
    the project's kernels; stride': the longest list of the batch"""
    B, A = dets.shape[:2]
    count = torch.full((B,), A, dtype=torch.int32, device="cuda")
    d = torch.from_numpy(dets).cuda()
    paste = hip.mask_paste(masks, d, count, im_size, M, CAPACITY, cls_specific=False)
    if int(paste["bytes"].max()) > CAPACITY:                                     # paste again with the capacity it asks for
        paste = hip.mask_paste(masks, d, count, im_size, M, int(paste["bytes"].max()), cls_specific=False)
    rle = hip.mask_rle(paste, count, im_size, runs_stride=RUNS_STRIDE, str_stride=16)      # the strings are not needed
    if int(rle["n_runs"].min()) < 0:                                             # a noisy tall mask: encode again with the stride it asks for
        rle = hip.mask_rle(paste, count, im_size, runs_stride=8 - int(rle["n_runs"].min()), str_stride=16)
    longest = max(int(rle["n_runs"].max()), 1)
    return rle["counts"][:, :, :longest].contiguous(), rle["n_runs"]


def make_set(n_images, batch):
    """-> the batches, each a dict of device tensors: runs, n_runs, dets [B,200,6], count, im_size"""
    rs = synth.rng(12, 0)
    out = []
    for i0 in range(0, n_images, batch):
        B = min(batch, n_images - i0)
        im_size = torch.tensor([[float(synth.IM_H), float(synth.IM_W)]] * B, device="cuda")
        dets = np.zeros((B, 2 * N_DET, 6), np.float32)
        for n in range(B):
            centres = synth.make_rois(rs, 12)
            near = rs.rand(N_DET) < 0.6
            boxes = np.where(near[:, None], centres[rs.randint(0, 12, N_DET)] + rs.randint(-12, 13, (N_DET, 4)), synth.make_rois(rs, N_DET))
            cls = np.sort(rs.randint(1, NUM_CLASSES, N_DET))                     # class-major rows, as the detection stage writes them
            score = rs.rand(N_DET).astype(np.float32)
            twin = boxes + rs.randint(-4, 5, (N_DET, 4))
            for k, b in ((0, boxes), (N_DET, twin)):
                b[:, 0::2], b[:, 1::2] = np.clip(b[:, 0::2], 0, synth.IM_W - 1), np.clip(b[:, 1::2], 0, synth.IM_H - 1)
                b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 4)
                dets[n, k:k + N_DET, :4], dets[n, k:k + N_DET, 5] = b, cls
            dets[n, :N_DET, 4], dets[n, N_DET:, 4] = score, score * np.float32(0.9)
        blobs = synth.make_masks(rs, B * N_DET, 1, M).reshape(B, N_DET, 1, M, M)
        masks = torch.from_numpy(np.concatenate([blobs, blobs], 1).reshape(B * 2 * N_DET, 1, M, M)).cuda()
        runs, n_runs = encode(masks, dets, im_size)
        out.append(dict(runs=runs, n_runs=n_runs, dets=torch.from_numpy(dets).cuda(),
                        count=torch.full((B,), 2 * N_DET, dtype=torch.int32, device="cuda"), im_size=im_size))
    return out


def chain(b, n_top=T):
    """overlaps + NMS on the pool, the first n_top kept rows as tops, overlaps + AVG vote; no sync"""
    kept = segms.rle_mask_nms_batched(b["runs"], b["n_runs"], b["dets"], b["count"], b["im_size"], NMS_THRESH, 'IOU')
    B, A, S = b["runs"].shape
    keep = torch.clamp(kept["keep"][:, :n_top], min=0).to(torch.int64)
    top_runs = torch.gather(b["runs"], 1, keep[:, :, None].expand(B, n_top, S))
    top_n = torch.gather(b["n_runs"], 1, keep)
    top_count = torch.clamp(kept["keep_count"], max=n_top)
    voted = segms.rle_mask_voting_batched(top_runs, top_n, top_count, b["runs"], b["n_runs"], b["dets"], b["count"], b["im_size"],
                                          IOU_THRESH, BINARIZE_THRESH, 'AVG', out_stride=2 * S)
    return kept, dict(top_runs=top_runs, top_n_runs=top_n, top_count=top_count), voted


def device_pass(batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for b in batches:
        last = chain(b)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, last


def stage_seconds(batches):
    """the same pass with a sync after each stage: where the time goes (the syncs cost a little)"""
    t = dict(nms=0.0, vote=0.0)
    for b in batches:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kept = segms.rle_mask_nms_batched(b["runs"], b["n_runs"], b["dets"], b["count"], b["im_size"], NMS_THRESH, 'IOU')
        torch.cuda.synchronize()
        t["nms"] += time.perf_counter() - t0
    total, _ = device_pass(batches)
    t["vote"] = total - t["nms"]
    return {k: round(v, 4) for k, v in t.items()}


def walked(b, voted, live):
    """how much of what the vote kernel walks can be set at all: per voted row, the pixels between the first and the last column of any
    voter (what the kernel walks, to within a column) against the largest voter's area and the sum of the voters' areas: the pixels
    some voter has lie between the two"""
    box = segms.rle_masks_to_boxes_batched(b["runs"], b["n_runs"], b["im_size"], b["count"])
    votes = voted["ovr"] >= IOU_THRESH                                           # [B,T,A]
    rows = live & (votes.sum(2) >= 2)
    x0 = torch.where(votes, box["boxes"][:, None, :, 0], torch.full_like(box["boxes"][:, None, :, 0], 1 << 30)).amin(2)
    x1 = torch.where(votes, box["boxes"][:, None, :, 2], torch.full_like(box["boxes"][:, None, :, 2], -1)).amax(2)
    span = ((x1 - x0 + 1).double() * b["im_size"][:, :1].double())[rows]
    areas = votes * box["area"][:, None, :].double()
    area, largest = areas.sum(2)[rows], areas.amax(2)[rows]                      # the voters' union lies between the two
    return dict(walked_pixels_mean=round(float(span.mean())), voter_area_sum_mean=round(float(area.mean())),
                largest_voter_area_mean=round(float(largest.mean())),
                share_set_at_least=round(float(largest.sum() / span.sum()), 3), share_set_at_most=round(float(torch.minimum(area, span).sum() / span.sum()), 3))


def ref_slice(b, k):
    """the first k detections of the first image and their duplicates: the restatement against the device, and both times"""
    import mask_post_ref as mr
    rows = list(range(k)) + list(range(N_DET, N_DET + k))
    sub = dict(runs=b["runs"][:1, rows].contiguous(), n_runs=b["n_runs"][:1, rows].contiguous(), dets=b["dets"][:1, rows].contiguous(),
               count=torch.full((1,), 2 * k, dtype=torch.int32, device="cuda"), im_size=b["im_size"][:1])
    chain(sub, n_top=k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kept, tops, voted = chain(sub, n_top=k)
    torch.cuda.synchronize()
    dev_seconds = time.perf_counter() - t0
    h = {k_: v.cpu().numpy() for k_, v in sub.items()}
    runs = h["runs"].view(np.uint32)
    t0 = time.perf_counter()
    iou = mr.overlaps(runs, h["n_runs"], h["count"], runs, h["n_runs"], h["count"], h["im_size"], False)
    want_keep = mr.nms(h["dets"], h["count"], iou["ovr"], NMS_THRESH, 'IOU')
    keep = np.maximum(want_keep["keep"][:, :k], 0)
    case = dict(top_runs=np.take_along_axis(runs, keep[:, :, None], 1), top_n_runs=np.take_along_axis(h["n_runs"], keep, 1),
                top_count=np.minimum(want_keep["keep_count"], k), all_runs=runs, all_n_runs=h["n_runs"], all_dets=h["dets"],
                all_count=h["count"], im_size=h["im_size"], out_stride=voted["out_runs"].shape[2], iou_thresh=IOU_THRESH,
                binarize_thresh=BINARIZE_THRESH)
    ovr = mr.overlaps(case["top_runs"], case["top_n_runs"], case["top_count"], runs, h["n_runs"], h["count"], h["im_size"], False)["ovr"]
    want = mr.vote(case, ovr, 'AVG')
    ref_seconds = time.perf_counter() - t0
    got_n, got_runs = voted["out_n_runs"].cpu().numpy(), voted["out_runs"].cpu().numpy().view(np.uint32)
    nt = int(case["top_count"][0])
    same = (kept["ovr"].cpu().numpy().tobytes() == iou["ovr"].tobytes() and np.array_equal(kept["keep"].cpu().numpy(), want_keep["keep"]) and
            voted["ovr"].cpu().numpy().tobytes() == ovr.tobytes() and np.array_equal(got_n[0, :nt], want["out_n_runs"][0, :nt]) and
            all(got_runs[0, t, :got_n[0, t]].tolist() == want["lists"][0][t] for t in range(nt) if got_n[0, t] >= 0))
    return dict(ref_masks=2 * k, ref_tops=nt, ref_voted=int((~want["copied"][0, :nt]).sum()), ref_seconds=round(ref_seconds, 2),
                slice_device_seconds=round(dev_seconds, 4), slice_bit_equal=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--ref-dets", type=int, default=20)
    args = ap.parse_args()
    t0 = time.perf_counter()
    batches = make_set(args.images, args.batch)
    torch.cuda.synchronize()
    made = time.perf_counter() - t0
    n_runs = torch.cat([b["n_runs"].reshape(-1) for b in batches])
    _, (kept, tops, voted) = device_pass(batches)                                # warm-up: library load, allocator
    times = [device_pass(batches)[0] for _ in range(3)]
    need, n_out = voted["need"], voted["out_n_runs"]
    nt = tops["top_count"]
    live = torch.arange(T, device="cuda")[None, :] < nt[:, None]
    voters = ((voted["ovr"] >= IOU_THRESH).sum(2))[live].float()
    out = dict(images=args.images, batch=args.batch, make_set_seconds=round(made, 1), device_seconds=[round(t, 4) for t in times],
               images_per_second=round(args.images / min(times), 1), stage_seconds=stage_seconds(batches),
               runs_mean=round(float(n_runs.float().mean()), 1), runs_max=int(n_runs.max()),
               last_batch=dict(kept_mean=round(float(kept["keep_count"].float().mean()), 1), voters_mean=round(float(voters.mean()), 2),
                               voted_rows=int((voters >= 2).sum()), rows=int(live.sum()), did_not_fit=int((n_out[live] < 0).sum()),
                               need_max=int(need[live].max())))
    out["last_batch"].update(walked(batches[-1], voted, live))
    if args.ref_dets:
        out.update(ref_slice(batches[0], args.ref_dets))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
