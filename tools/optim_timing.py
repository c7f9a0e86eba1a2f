"""Times the optimizer tail of the training step on the trainable parameters of freeze_stem(detector()) (Fast R-CNN R-50-C4: the
shapes are taken from the model, built on the CPU):

  fused    ONE call of dtc_sgd_step (norm pass + update pass; the gradients are not written);
  foreach  the reference's formulation (train_fast.py:165-166) with torch's multi-tensor kernels on the same GPU:
           clip_grad_norm_(foreach=True) + torch.optim.SGD(momentum=0.9, weight_decay=1e-4, foreach=True).step();
  tfused   the same with torch.optim.SGD(fused=True), where this torch offers it ("not measured" otherwise).

    python tools/optim_timing.py [--window 0.5] [--rounds 5] [--out FILE]

HIP events around windows of back-to-back calls; every window lasts at least --window seconds (the call count is set from a trial);
the sides alternate, --rounds windows each, in one process, after a warm-up of all.  One JSON line: the median time per call of
each side in microseconds with the spread (min .. max over the rounds), the ratios, and beside them the floor of the algorithm:
24 bytes per element (4 read by the norm pass, 12 read and 8 written by the update pass) at the 8.0 TB/s of the HBM's data sheet and
at the 6.3 TB/s a float4 copy reaches on this GPU.  The parameter set (about 100 MB) fits the 256 MiB Infinity Cache three times
over, so a side may well run below the HBM floor: the floor is for orientation, not a bound on these numbers.  All sides are
checked against each other after one step from equal states before they are timed.  Needs the GPU: without one it fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectorch_amd import hip_optim  # noqa: E402

LR, MOMENTUM, WD, MAX_NORM = 1e-4, 0.9, 1e-4, 35.0


def shapes():
    """the trainable parameter shapes of the model the reference trains, in model.parameters() order"""
    from detectorch_amd.model.detector import detector
    from detectorch_amd.train import freeze_stem
    return [tuple(p.shape) for p in freeze_stem(detector())]


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
        raise SystemExit("optim_timing needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    shp = shapes()
    rs = np.random.RandomState(90)
    p0 = [torch.from_numpy((rs.standard_normal(s) * 0.05).astype(np.float32)).to(dev) for s in shp]
    g0 = [torch.from_numpy((rs.standard_normal(s) * 0.01).astype(np.float32)).to(dev) for s in shp]
    n = sum(t.numel() for t in p0)

    def state():
        params = [torch.nn.Parameter(t.clone()) for t in p0]
        for p, g in zip(params, g0):
            p.grad = g.clone()
        return params

    # fused: the raw entry on its own table (what ClippedSGD.step() makes once the table exists)
    mine = state()
    bufs = [torch.zeros_like(p) for p in mine]
    plan = hip_optim.make_plan(mine, [p.grad for p in mine], bufs, [0] * len(mine), 1)
    hyper = torch.tensor([[LR, WD]], dtype=torch.float32, device=dev)
    stats = torch.zeros(4, dtype=torch.float32, device=dev)
    sides = {"fused": lambda: hip_optim.sgd_step(plan, hyper, MOMENTUM, MAX_NORM, stats)}
    models = {"fused": mine}

    def torch_side(**kw):
        params = state()
        opt = torch.optim.SGD(params, lr=LR, momentum=MOMENTUM, weight_decay=WD, **kw)

        def step():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
            opt.step()
        return params, step
    models["foreach"], sides["foreach"] = torch_side(foreach=True)
    try:
        models["tfused"], sides["tfused"] = torch_side(fused=True)
    except (RuntimeError, TypeError, ValueError) as e:
        print("SGD(fused=True) is not offered here: %s" % e, file=sys.stderr)

    # all sides compute the same step (the first one, from equal states; afterwards clip_grad_norm_ has rescaled torch's gradients)
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    scale = max(float(t.abs().max()) for t in p0)
    for name in list(sides)[1:]:
        worst = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(models["fused"], models[name]))
        assert worst <= 16 * np.finfo(np.float32).eps * scale, (name, worst)
    calls = {}
    for name, fn in sides.items():                                           # warm-up, then the call count of a window
        window(fn, 10)
        ms = window(fn, 20) / 20.0
        calls[name] = max(20, int(args.window * 1e3 / ms) + 1)
    us = {name: [] for name in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():                                       # alternating
            us[name].append(window(fn, calls[name]) / calls[name] * 1e3)
    med = {name: statistics.median(v) for name, v in us.items()}
    out = dict(tensors=len(shp), elements=n, bytes_per_element=24, window_s=args.window, rounds=args.rounds, calls_per_window=calls,
               n_chunks=plan.n_chunks, floor_us_at_8_0_TBps=round(24.0 * n / 8.0e12 * 1e6, 2),
               floor_us_at_6_3_TBps=round(24.0 * n / 6.3e12 * 1e6, 2))
    for name in ("fused", "foreach", "tfused"):
        if name in med:
            out[name + "_us"] = round(med[name], 2)
            out[name + "_us_min_max"] = [round(min(us[name]), 2), round(max(us[name]), 2)]
            if name != "fused":
                out[name + "_over_fused"] = round(med[name] / med["fused"], 2)
        else:
            out[name + "_us"] = "not measured"
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
