"""Times RoIAlign backward (dtc_roi_align_backward, one call for all levels) at two training shapes:

  box head   8 images x 512 RoIs, 256 channels, 7 x 7 bins, sampling ratio 2, the four FPN levels of an 800 x 1333 batch
  C4 head    2 images x 256 RoIs, 1024 channels, 14 x 14 bins, adaptive sampling, one 50 x 84 map

against a plain-torch formulation on the same GPU -- the tap indices and weights of every sample are computed beforehand (not
timed); timed is, per level, gathering grad_output at the taps' bins, scaling by the weights and one index_add_ into the map, which
torch performs with float atomics into a zeroed [B*H*W, C] map (channels last; no transpose back is charged) -- and against the
memory floor: (bytes of the maps written once + bytes of grad_output read once) / 8 TB/s.

    python tools/roi_align_backward_timing.py [--window 0.5] [--rounds 5] [--out FILE]

HIP events around windows of back-to-back calls; every window lasts at least --window seconds (the call count is set from a trial);
the two sides alternate, --rounds windows each, in one process, after a warm-up of both.  One JSON line per shape: the median time
per call of each side in microseconds, the spread (min .. max over the rounds), torch / native and native / floor.  Both sides
are checked against each other before they are timed.  Needs the GPU: without one it fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectorch_amd import hip_grad  # noqa: E402

HBM_BYTES_PER_S = 8e12


def make_rois(rs, batch, per_image, im_h, im_w, lo, hi):
    """boxes with log-uniform sides lo .. hi pixels inside an im_h x im_w image -> float32 [batch * per_image, 5]"""
    n = batch * per_image
    bw, bh = np.exp(rs.uniform(np.log(lo), np.log(hi), n)), np.exp(rs.uniform(np.log(lo), np.log(hi), n))
    bw, bh = np.minimum(bw, im_w - 1.0), np.minimum(bh, im_h - 1.0)
    x1, y1 = rs.uniform(0, im_w - bw), rs.uniform(0, im_h - bh)
    return np.stack([np.repeat(np.arange(batch), per_image), x1, y1, x1 + bw, y1 + bh], 1).astype(np.float32)


def fpn_levels(rois, k_min=2, k_max=5):
    """the FPN heuristic: level floor(4 + log2(sqrt(area) / 224)) clipped to k_min .. k_max, as an index from 0"""
    s = np.sqrt((rois[:, 3] - rois[:, 1] + 1) * (rois[:, 4] - rois[:, 2] + 1))
    return (np.clip(np.floor(4 + np.log2(s / 224.0 + 1e-6)), k_min, k_max) - k_min).astype(np.int32)


def taps(rois, shape, scale, ph, pw, ratio):
    """(bin index into grad_output viewed [R*PH*PW, C], pixel index into the map viewed [B*H*W, C], weight / count) of every tap
    of every valid sample of `rois` (float32 [R, 5], on the device), by torch ops"""
    B, _, H, W = shape
    R = rois.shape[0]
    dev = rois.device
    b = rois[:, 0].long()
    x1, y1, x2, y2 = (rois[:, k] * scale for k in range(1, 5))
    rw, rh = (x2 - x1).clamp(min=1.0), (y2 - y1).clamp(min=1.0)
    gh = torch.full((R,), ratio, device=dev) if ratio > 0 else torch.ceil(rh / ph).long()
    gw = torch.full((R,), ratio, device=dev) if ratio > 0 else torch.ceil(rw / pw).long()
    G = int(max(gh.max(), gw.max()))

    def axis(start, size, n_bins, grid, extent):
        p = torch.arange(n_bins, device=dev).view(1, -1, 1).float()
        i = torch.arange(G, device=dev).view(1, 1, -1).float()
        binsz = (size / n_bins).view(-1, 1, 1)
        v = start.view(-1, 1, 1) + p * binsz + (i + 0.5) * binsz / grid.view(-1, 1, 1).float()
        ok = (i < grid.view(-1, 1, 1)) & (v >= -1.0) & (v <= extent)
        v = v.clamp(min=0.0)
        lo = v.floor().long().clamp(max=extent - 1)
        hi = (lo + 1).clamp(max=extent - 1)
        v = torch.where(lo >= extent - 1, lo.float(), v)
        frac = v - lo.float()
        return ok, lo, hi, frac                                   # each [R, n_bins, G]

    oky, ylo, yhi, ly = axis(y1, rh, ph, gh, H)
    okx, xlo, xhi, lx = axis(x1, rw, pw, gw, W)
    full = (R, ph, G, pw, G)
    e = lambda t, y: (t.view(R, ph, G, 1, 1) if y else t.view(R, 1, 1, pw, G)).expand(full)
    ok = e(oky, 1) & e(okx, 0)
    inv = (1.0 / (gh * gw).float()).view(R, 1, 1, 1, 1).expand(full)
    bins = ((torch.arange(R, device=dev).view(R, 1, 1, 1, 1) * ph + torch.arange(ph, device=dev).view(1, ph, 1, 1, 1)) * pw +
            torch.arange(pw, device=dev).view(1, 1, 1, pw, 1)).expand(full)
    img = b.view(R, 1, 1, 1, 1).expand(full)
    out = []
    for yy, wy in ((ylo, 1 - ly), (yhi, ly)):
        for xx, wx in ((xlo, 1 - lx), (xhi, lx)):
            out.append((bins[ok], ((img * H + e(yy, 1)) * W + e(xx, 0))[ok], (e(wy, 1) * e(wx, 0) * inv)[ok]))
    return tuple(torch.cat([o[k] for o in out]) for k in range(3))


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
        raise SystemExit("roi_align_backward_timing needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    shapes = {
        "box head": dict(batch=8, per_image=512, channels=256, pooled=7, ratio=2, maps=[(200, 336), (100, 168), (50, 84), (25, 42)],
                         scales=[1 / 4., 1 / 8., 1 / 16., 1 / 32.], sides=(24.0, 640.0)),
        "C4 head": dict(batch=2, per_image=256, channels=1024, pooled=14, ratio=0, maps=[(50, 84)], scales=[1 / 16.], sides=(32.0, 500.0)),
    }
    lines = []
    for name, s in shapes.items():
        rs = np.random.RandomState(len(name))
        B, C, P = s["batch"], s["channels"], s["pooled"]
        rois_h = make_rois(rs, B, s["per_image"], 800, 1333, *s["sides"])
        levels_h = fpn_levels(rois_h) if len(s["maps"]) > 1 else np.zeros(len(rois_h), np.int32)
        rois, levels = torch.from_numpy(rois_h).to(dev), torch.from_numpy(levels_h).to(dev)
        R = rois.shape[0]
        top = torch.randn(R, C, P, P, device=dev)
        feature_shapes = [(B, C, h, w) for h, w in s["maps"]]
        out = hip_grad.backward_outputs(feature_shapes, R, dev)
        native = lambda: hip_grad.roi_align_backward(top, rois, feature_shapes, s["scales"], P, P, s["ratio"], roi_levels=levels, out=out)

        per_level = []
        for l, (shape, scale) in enumerate(zip(feature_shapes, s["scales"])):
            rows = torch.nonzero(levels == l).flatten()
            if rows.numel() == 0:
                raise SystemExit("level %d has no RoI: choose other sides" % l)
            bins, pix, w = taps(rois[rows], shape, scale, P, P, s["ratio"])
            bins = (rows[bins // (P * P)] * (P * P) + bins % (P * P))
            per_level.append((bins, pix, w.view(-1, 1), torch.empty((B * shape[2] * shape[3], C), device=dev)))
        top_rows = top.permute(0, 2, 3, 1).reshape(R * P * P, C).contiguous()            # [bin, C], prepared once (not timed)

        def torch_side():
            for bins, pix, w, grad in per_level:
                grad.zero_()
                grad.index_add_(0, pix, top_rows[bins] * w)

        native()
        torch_side()
        torch.cuda.synchronize()
        for l, (shape, (_, _, _, grad)) in enumerate(zip(feature_shapes, per_level)):       # both sides compute the same thing
            want = grad.view(B, shape[2], shape[3], C).permute(0, 3, 1, 2)
            scale_l = float(want.abs().max()) + 1e-30
            assert float((out["grads"][l] - want).abs().max()) <= 1e-4 * scale_l, (name, l)
        sides = {"native": native, "torch": torch_side}
        calls = {}
        for side, fn in sides.items():                                       # warm-up, then the call count of a window
            window(fn, 3)
            ms = window(fn, 5) / 5.0
            calls[side] = max(3, int(args.window * 1e3 / ms) + 1)
        us = {side: [] for side in sides}
        for _ in range(args.rounds):
            for side, fn in sides.items():                                   # alternating
                us[side].append(window(fn, calls[side]) / calls[side] * 1e3)
        med = {side: statistics.median(v) for side, v in us.items()}
        map_bytes = sum(4 * B * C * h * w for h, w in s["maps"])
        floor_us = (map_bytes + top.numel() * 4) / HBM_BYTES_PER_S * 1e6
        lines.append(json.dumps(dict(
            shape=name, rois=R, channels=C, pooled=P, sampling_ratio=s["ratio"], rois_per_level=np.bincount(levels_h).tolist(),
            map_mbytes=round(map_bytes / 1e6, 1), grad_output_mbytes=round(top.numel() * 4 / 1e6, 1), window_s=args.window,
            rounds=args.rounds, calls_per_window=calls, native_us=round(med["native"], 1),
            native_us_min_max=[round(min(us["native"]), 1), round(max(us["native"]), 1)], torch_us=round(med["torch"], 1),
            torch_us_min_max=[round(min(us["torch"]), 1), round(max(us["torch"]), 1)], floor_us=round(floor_us, 1),
            torch_over_native=round(med["torch"] / med["native"], 2), native_over_floor=round(med["native"] / floor_us, 1))))
        print(lines[-1], flush=True)
        del per_level, top_rows, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
