"""Times mask training for B = 8 images with 128 foreground rows each (Rm = 1024), K = 81, at the FPN shape (M = 28) and the C4 shape
(M = 14):

  targets  dtc_mask_targets on a minibatch of 512 rows per image, 128 of them foreground, against 20 gt of one 40-point polygon each
           (no torch side: the host form is a Python loop over the RoIs through pycocotools);
  native   ONE dtc_mask_loss: the loss and the dense [Rm, K, M, M] gradient;
  torch    the same loss in plain torch ops on the same GPU: gather of the class channel, binary_cross_entropy_with_logits with a
           weight for the ignored targets, autograd for the gradient (which scatters into zeros of the logits' shape).

    python tools/mask_train_timing.py [--window 0.5] [--rounds 5] [--out FILE]

HIP events around windows of back-to-back calls; every window lasts at least --window seconds (the call count is set from a trial);
the sides alternate, --rounds windows each, in one process, after a warm-up of all.  One JSON line per shape: the median time per
call of each side in microseconds, the spread (min .. max over the rounds), torch / native, and the byte floor of the gradient store
(Rm K M^2 4 bytes, at 8 TB/s).  Both loss sides are checked against each other before they are timed.  Needs the GPU: without one it
fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectorch_amd import hip_mask  # noqa: E402
from detectorch_amd.utils.mask_rcnn_targets import pack_polygons  # noqa: E402

SHAPES = {"fpn": 28, "c4": 14}


def inputs(B, G, R, F, seed, dev):
    rs = np.random.RandomState(seed)
    polys, boxes = [], np.zeros((B, G, 4), np.float32)
    for b in range(B):
        per = []
        for g in range(G):
            cx, cy, r = rs.uniform(100, 1200), rs.uniform(100, 700), rs.uniform(20, 200)
            a = np.sort(rs.uniform(0, 2 * np.pi, 40))
            rad = r * rs.uniform(0.5, 1.0, 40)
            p = np.stack([cx + rad * np.cos(a), cy + rad * np.sin(a)], 1).astype(np.float32)
            per.append([p.reshape(-1).tolist()])
            boxes[b, g] = [p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()]
        polys.append(per)
    src = rs.randint(0, G, (B, F))
    gtb = np.take_along_axis(boxes, src[..., None].repeat(4, 2), 1)
    size = np.tile(gtb[..., 2:] - gtb[..., :2], 2)
    props = (gtb + rs.uniform(-0.15, 0.15, gtb.shape) * size).astype(np.float32)
    labels = np.full((B, R), -1, np.int32)
    labels[:, :F] = rs.randint(1, 81, (B, F))
    labels[:, F:R - 7] = 0
    keep = np.full((B, R), -1, np.int32)
    keep[:, :F] = G + np.arange(F)
    keep[:, F:R - 7] = G
    d = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(dev, dt)
    i32, f32 = torch.int32, torch.float32
    return dict(labels=d(labels, i32), keep=d(keep, i32), n_rois=d(np.full(B, R - 7), i32), gt=d(boxes, f32),
                cls=d(rs.randint(1, 81, (B, G)), i32), crowd=torch.zeros((B, G), dtype=i32, device=dev),
                counts=d(np.full(B, G), i32), props=d(props, f32), scale=torch.ones(B, device=dev),
                polys=pack_polygons(polys, G, device=dev))


def window(fn, calls):
    """milliseconds of `calls` back-to-back calls, by HIP events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_train_timing needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    B, G, R, F, K = 8, 20, 512, 128, 81
    lines = []
    for name, M in SHAPES.items():
        x = inputs(B, G, R, F, 60 + M, dev)
        tout = hip_mask.targets_outputs(B, R, F, M, dev)

        def targets():
            hip_mask.mask_targets(x["labels"], x["keep"], x["n_rois"], x["gt"], x["cls"], x["crowd"], x["counts"], x["props"], x["scale"],
                                  *x["polys"], M=M, k_min=2, k_max=5, out=tout)
        targets()
        torch.cuda.synchronize()
        masks, mcls = tout["masks"].reshape(B * F, M * M).clone(), tout["mask_class"].reshape(B * F).clone()
        assert tout["n_mask"].tolist() == [F] * B and int((masks == 1).sum()) > 0 and int((masks < 0).sum()) == 0
        masks[::7, ::5] = -1                                                  # some ignored targets, as rows without a polygon have
        logits = torch.randn((B * F, K, M, M), device=dev, generator=torch.Generator(device=dev).manual_seed(M)) * 2
        lout = hip_mask.loss_outputs(B * F, K, M, dev)
        ref = logits.clone().requires_grad_()
        rows, state = torch.arange(B * F, device=dev), {}
        weight, target = (masks >= 0).float(), (masks == 1).float()

        def native():
            hip_mask.mask_loss(logits, masks, mcls, out=lout)

        def plain():
            ref.grad = None
            sel = ref.reshape(B * F, K, M * M)[rows, mcls.long()]
            loss = torch.nn.functional.binary_cross_entropy_with_logits(sel, target, weight=weight, reduction="sum") / weight.sum()
            loss.backward()
            state["loss"] = loss.detach()
        native()
        plain()
        torch.cuda.synchronize()
        L = float(lout["loss"][0])
        assert abs(L - float(state["loss"])) <= 1e-5 * max(1.0, L), "the two sides disagree on the loss"
        assert float((lout["grad_mask_logits"] - ref.grad).abs().max()) <= 1e-9 + 1e-5 / int(lout["n_valid"][0])
        sides = {"targets": targets, "native": native, "torch": plain}
        calls = {}
        for side, fn in sides.items():                                       # warm-up, then the call count of a window
            window(fn, 5)
            ms = window(fn, 10) / 10.0
            calls[side] = max(10, int(args.window * 1e3 / ms) + 1)
        us = {side: [] for side in sides}
        for _ in range(args.rounds):
            for side, fn in sides.items():                                   # alternating
                us[side].append(window(fn, calls[side]) / calls[side] * 1e3)
        med = {side: statistics.median(v) for side, v in us.items()}
        floor_bytes = B * F * K * M * M * 4
        mm = lambda side: [round(min(us[side]), 2), round(max(us[side]), 2)]
        lines.append(json.dumps(dict(
            shape=name, M=M, batch=B, fg_rows=F, K=K, n_valid=int(lout["n_valid"][0]), window_s=args.window, rounds=args.rounds,
            calls_per_window=calls, targets_us=round(med["targets"], 2), targets_us_min_max=mm("targets"),
            native_us=round(med["native"], 2), native_us_min_max=mm("native"), torch_us=round(med["torch"], 2),
            torch_us_min_max=mm("torch"), torch_over_native=round(med["torch"] / med["native"], 2), grad_store_bytes=floor_bytes,
            floor_us_at_8TBs=round(floor_bytes / 8e12 * 1e6, 2))))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
