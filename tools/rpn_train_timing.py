"""Times the RPN training minibatch + losses for B = 8 images of 20 gt boxes at the C4 shape (38 x 50 x 15 anchors, N = 28 500) and
the FPN shape (200 x 336 and four coarser levels x 3 anchors, N = 268 569):

  native  dtc_rpn_targets (labels, sample, box targets) + ONE dtc_rpn_loss (both losses and the dense gradient maps);
  torch   the same contract in plain torch ops on the same GPU, per image: the hip.bbox_overlaps matrix, max / argmax, the masks of
          the three groups, topk of the (rand_key, index) keys for the two samples, bbox_transform_inv, then
          binary_cross_entropy_with_logits and smooth-L1 over the batch and autograd for the gradient maps.  The shifted anchors and
          the inside mask are built beforehand and not timed.

    python tools/rpn_train_timing.py [--window 0.5] [--rounds 5] [--out FILE]

HIP events around windows of back-to-back calls; every window lasts at least --window seconds (the call count is set from a trial);
the two sides alternate, --rounds windows each, in one process, after a warm-up of both.  One JSON line per shape: the median time
per call of each side in microseconds, the spread (min .. max over the rounds), torch / native, and the byte floor of the native side
(labels, keys and logits read once, the gradient maps written once) at 8 TB/s.  Both sides are checked against each other before they
are timed.  Needs the GPU: without one it fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectorch_amd import hip, hip_rpn  # noqa: E402
from detectorch_amd.utils.generate_anchors import generate_anchors  # noqa: E402

BETA = 1.0 / 9.0
SHAPES = {"c4": [(15, 38, 50, 16.0, generate_anchors(16))],
          "fpn": [(3, h, w, 4.0 * 2 ** l, generate_anchors(4 * 2 ** l, (32 * 2 ** l,)))
                  for l, (h, w) in enumerate(((200, 336), (100, 168), (50, 84), (25, 42), (13, 21)))]}
IMAGE = {"c4": (608.0, 800.0), "fpn": (800.0, 1344.0)}


def all_anchors(spec, dev):
    out = []
    for A, H, W, stride, base in spec:
        base = torch.tensor(np.asarray(base, np.float32), device=dev)
        sx = torch.arange(W, dtype=torch.float32, device=dev) * stride
        sy = torch.arange(H, dtype=torch.float32, device=dev) * stride
        shift = torch.stack([sx[None, :].expand(H, W), sy[:, None].expand(H, W)] * 2, -1)
        out.append((base[:, None, None, :] + shift[None]).reshape(-1, 4))
    return torch.cat(out).contiguous()


def inputs(name, B, G, seed, dev):
    spec = SHAPES[name]
    rs = np.random.RandomState(seed)
    anchors = all_anchors(spec, dev)
    N = anchors.shape[0]
    h, w = IMAGE[name]
    a = anchors.cpu().numpy()
    ok = np.where((a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] < w) & (a[:, 3] < h))[0]
    src = a[rs.choice(ok, (B, G))].astype(np.float64)
    size = np.tile(src[..., 2:] - src[..., :2] + 1.0, 2)
    gt = (src + rs.uniform(-0.1, 0.1, src.shape) * size).astype(np.float32)
    d = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(dev, dt)
    cls = [d(rs.standard_normal((B, A, H, W)) * 2.0, torch.float32) for A, H, W, _, _ in spec]
    box = [d(rs.standard_normal((B, 4 * A, H, W)) * 0.3, torch.float32) for A, H, W, _, _ in spec]
    return dict(spec=spec, anchors=anchors, N=N, gt=d(gt, torch.float32), crowd=torch.zeros((B, G), dtype=torch.int32, device=dev),
                counts=torch.full((B,), G, dtype=torch.int32, device=dev), scale=torch.ones(B, device=dev),
                im_hw=d([[h, w]] * B, torch.float32), keys=d(rs.randint(-2 ** 31, 2 ** 31, (B, N)), torch.int32), cls=cls, box=box)


def native_side(x, R=256):
    spec, B = x["spec"], x["gt"].shape[0]
    prm = hip_rpn.rpn_train_params(batch_size_per_im=R)
    tl, _ = hip_rpn.make_levels([s[:3] for s in spec], [s[4] for s in spec], [s[3] for s in spec])
    tout = hip_rpn.targets_outputs(tl, B, x["N"], x["gt"].shape[1], prm, x["gt"].device)
    gc, gb = [torch.empty_like(t) for t in x["cls"]], [torch.empty_like(t) for t in x["box"]]
    ll, _, _ = hip_rpn.map_levels(x["cls"], x["box"], gc, gb)
    lout = hip_rpn.loss_outputs(ll, B, x["gt"].device)

    def step():
        hip_rpn.rpn_targets(tl, x["gt"], x["crowd"], x["counts"], x["scale"], x["im_hw"], x["keys"], prm, out=tout)
        hip_rpn.rpn_loss(ll, tout["labels"], tout["fg_index"], tout["fg_targets"], tout["n_fg"], tout["n_bg"], beta=BETA, out=lout)
    return step, tout, lout, gc, gb


def torch_side(x, R=256, pos=0.7, neg=0.3):
    spec, B, N, anchors = x["spec"], x["gt"].shape[0], x["N"], x["anchors"]
    F = R // 2
    dev = anchors.device
    cls = [t.clone().requires_grad_() for t in x["cls"]]
    box = [t.clone().requires_grad_() for t in x["box"]]
    idx = torch.arange(N, device=dev)
    big = torch.tensor(1 << 62, device=dev)
    aw, ah = anchors[:, 2] - anchors[:, 0] + 1.0, anchors[:, 3] - anchors[:, 1] + 1.0
    acx, acy = anchors[:, 0] + 0.5 * aw, anchors[:, 1] + 0.5 * ah
    state = {}

    def step():
        for t in cls + box:
            t.grad = None
        flat_cls = torch.cat([t.reshape(B, -1) for t in cls], 1)
        flat_box = torch.cat([t.reshape(B, t.shape[1] // 4, 4, -1).permute(0, 1, 3, 2).reshape(B, -1, 4) for t in box], 1)
        labels = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        loss_bbox = 0.0
        n_valid = 0
        for b in range(B):
            h, w = x["im_hw"][b, 0], x["im_hw"][b, 1]
            inside = (anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] < w) & (anchors[:, 3] < h)
            gt = x["gt"][b] * x["scale"][b]
            ov = hip.bbox_overlaps(anchors, gt) * inside[:, None]
            mx, arg = ov.max(1)
            gmax = ov.max(0)[0]
            fg = inside & ((mx >= pos) | ((ov == gmax[None]) & (gmax[None] > 0)).any(1))
            bg = inside & ~fg & (mx < neg)
            key = ((x["keys"][b].long() & 0xFFFFFFFF) << 20) | idx
            fv, fi = torch.topk(torch.where(fg, key, big), F, largest=False)
            n_fg = (fv < big).sum()
            bv, bi = torch.topk(torch.where(bg, key, big), R, largest=False)
            take_bg = (bv < big) & (torch.arange(R, device=dev) < R - n_fg)
            n_bg = take_bg.sum()
            lab = labels[b]
            lab[bi[take_bg]] = 0
            lab[fi[fv < big]] = 1
            g = gt[arg[fi]]
            gw, gh = g[:, 2] - g[:, 0] + 1.0, g[:, 3] - g[:, 1] + 1.0
            t = torch.stack([(g[:, 0] + 0.5 * gw - acx[fi]) / aw[fi], (g[:, 1] + 0.5 * gh - acy[fi]) / ah[fi], torch.log(gw / aw[fi]),
                             torch.log(gh / ah[fi])], 1)
            dlt = flat_box[b, fi] - t
            a = dlt.abs()
            sl1 = torch.where(a <= BETA, 0.5 * dlt * dlt / BETA, a - 0.5 * BETA) * (fv < big)[:, None]
            loss_bbox = loss_bbox + sl1.sum() / (n_fg + n_bg).clamp(min=1) / B
            n_valid = n_valid + n_fg + n_bg
        valid = labels >= 0
        loss_cls = torch.nn.functional.binary_cross_entropy_with_logits(flat_cls, (labels == 1).float(), weight=valid.float(),
                                                                        reduction="sum") / n_valid.clamp(min=1)
        (loss_cls + loss_bbox).backward()
        state.update(labels=labels, loss_cls=loss_cls.detach(), loss_bbox=loss_bbox.detach())
    return step, state, cls, box


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
        raise SystemExit("rpn_train_timing needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    lines = []
    for name in ("c4", "fpn"):
        B, G = 8, 20
        x = inputs(name, B, G, 50 + len(name), dev)
        native, tout, lout, gc, gb = native_side(x)
        step, state, cls, box = torch_side(x)
        # both sides compute the same thing
        native()
        step()
        torch.cuda.synchronize()
        L = lout["losses"].cpu().numpy()
        assert torch.equal(tout["labels"], state["labels"]), "the two sides sampled different anchors"
        assert abs(L[0] - float(state["loss_cls"])) <= 1e-5 * max(1.0, L[0]) and abs(L[1] - float(state["loss_bbox"])) <= 1e-4 * max(1.0, L[1])
        assert max(float((a - b.grad).abs().max()) for a, b in zip(gc + gb, cls + box)) <= 1e-6
        sides = {"native": native, "torch": step}
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
        floor_bytes = B * x["N"] * (4 + 4 + 4) + B * x["N"] * (4 + 16)
        lines.append(json.dumps(dict(
            shape=name, batch=B, anchors=x["N"], gt=G, n_valid=int(lout["n_valid"][0]), window_s=args.window, rounds=args.rounds,
            calls_per_window=calls, native_us=round(med["native"], 2),
            native_us_min_max=[round(min(us["native"]), 2), round(max(us["native"]), 2)], torch_us=round(med["torch"], 2),
            torch_us_min_max=[round(min(us["torch"]), 2), round(max(us["torch"]), 2)],
            torch_over_native=round(med["torch"] / med["native"], 2), floor_bytes=floor_bytes,
            floor_us_at_8TBs=round(floor_bytes / 8e12 * 1e6, 2))))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
