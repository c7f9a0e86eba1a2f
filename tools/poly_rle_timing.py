"""The wall time of converting a synthetic val2017-sized set of polygon annotations to run lists on the device, next to the numpy
restatement's (tests/README_poly_rle.md records both; neither is a threshold of a test):

    python tools/poly_rle_timing.py [--images 5000] [--batch 250] [--ref-images 100] [--timeout 600]

The set: --images images of about 600 x 800 (each side within 25 % of that) with 2 to 12 instances (mean 7) of 1 to 3 polygons each;
a polygon is a noisy closed curve of 8 to 60 vertices around a centre inside the image, radius log-uniform in 6 .. 260 px, so some
reach outside the image; coordinates have two decimals, as COCO's.  Device: utils.segms.pack_gt_segms over all batches -- packing on
the host, dtc_poly_rle, the sync that sizes the buffers, the second conversion where the first guess was too small -- after one
warm-up pass.  Restatement: tests/poly_rle_ref.py on the first --ref-images images, scaled to the whole set; the same slice on the
device must give the same run lists (a digest of n_runs, runs and area is compared).

The process that prints the result never opens the GPU: the device step runs in a child process of its own under --timeout seconds
and is killed when it runs over; nothing else is started on the GPU after that.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_set(n_images, seed=0):
    """-> (segms_per_image: per image, per instance a list of COCO polygons [x0, y0, ...]; im_sizes int [n, 2] = (h, w))"""
    rs = np.random.RandomState(20261120 + seed)
    segms, sizes = [], np.zeros((n_images, 2), np.int64)
    for i in range(n_images):
        h, w = int(600 * rs.uniform(0.75, 1.25)), int(800 * rs.uniform(0.75, 1.25))
        sizes[i] = (h, w)
        inst = []
        for _ in range(rs.randint(2, 13)):
            cx, cy, r = rs.uniform(0, w), rs.uniform(0, h), float(np.exp(rs.uniform(np.log(6.0), np.log(260.0))))
            polys = []
            for k in range(rs.randint(1, 4)):
                n = rs.randint(8, 61)
                a = np.sort(rs.uniform(0, 2 * np.pi, n))
                rad = (r if k == 0 else 0.4 * r) * rs.uniform(0.6, 1.0, n)
                ox, oy = (0.0, 0.0) if k == 0 else rs.uniform(-r, r, 2)
                xy = np.stack([cx + ox + rad * np.cos(a), cy + oy + rad * np.sin(a)], 1)
                polys.append(np.round(xy, 2).reshape(-1).tolist())
            inst.append(polys)
        segms.append(inst)
    return segms, sizes


def digest(n_runs, runs_of_row, area):
    """sha256 over the rows in order: n_runs, the runs, the area"""
    h = hashlib.sha256()
    for i in range(n_runs.shape[0]):
        for j in range(n_runs.shape[1]):
            h.update(np.asarray([n_runs[i, j], area[i, j]], np.int64).tobytes())
            h.update(np.asarray(runs_of_row(i, j), np.uint32).tobytes())
    return h.hexdigest()


def device_step(args):
    import torch
    from detectorch_amd.utils import segms
    segm, sizes = make_set(args.images)
    G = max(len(s) for s in segm)

    def one_pass():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [segms.pack_gt_segms(segm[i0:i0 + args.batch], sizes[i0:i0 + args.batch], "cuda", G) for i0 in range(0, args.images, args.batch)]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    one_pass()                                                                   # warm-up: library load, allocator
    times = [one_pass() for _ in range(3)]
    out = times[0][1]
    n_runs = np.concatenate([o["gt_n_runs"].cpu().numpy() for o in out])
    area = np.concatenate([o["area"].cpu().numpy() for o in out])
    res = dict(images=args.images, batch=args.batch, instances=int(sum(len(s) for s in segm)), polygons=int(sum(len(p) for s in segm for p in s)),
               device_seconds=[round(t, 4) for t, _ in times], runs_mean=round(float(n_runs[n_runs > 0].mean()), 1), runs_max=int(n_runs.max()),
               runs_strides=sorted({int(o["gt_runs"].shape[2]) for o in out}), pixels_on_mean=round(float(area[n_runs > 0].mean()), 1))
    k = min(args.ref_images, args.images)
    if k:
        runs = np.concatenate([np.pad(o["gt_runs"].cpu().numpy(), ((0, 0), (0, 0), (0, res["runs_strides"][-1] - o["gt_runs"].shape[2])))
                               for o in out[:(k + args.batch - 1) // args.batch]]).view(np.uint32)
        res["slice_digest"] = digest(n_runs[:k], lambda i, j: runs[i, j, :max(n_runs[i, j], 0)], area[:k])
    print(json.dumps(res))


def ref_step(args):
    import poly_rle_ref as pr
    segm, sizes = make_set(args.images)
    G = max(len(s) for s in segm)
    k = min(args.ref_images, args.images)
    t0 = time.perf_counter()
    case = pr.make_case([[[np.asarray(p, np.float64).reshape(-1, 2) for p in polys] for polys in s] for s in segm[:k]], sizes[:k], G=G)
    want = pr.run(case, 1 << 20, 1 << 20)
    dt = time.perf_counter() - t0
    return dict(ref_images=k, ref_seconds=round(dt, 2), ref_seconds_scaled=round(dt * args.images / k, 1),
                slice_digest=digest(want["n_runs"], lambda i, j: want["runs"][i][j] or [], want["area"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--ref-images", type=int, default=100)
    ap.add_argument("--timeout", type=int, default=600, help="seconds the device step may take")
    ap.add_argument("--step", choices=("all", "device"), default="all")
    args = ap.parse_args()
    if args.step == "device":
        return device_step(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "device", "--images", str(args.images), "--batch", str(args.batch),
           "--ref-images", str(args.ref_images)]
    try:
        child = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        sys.exit("the device step ran over %d s and was killed" % args.timeout)
    if child.returncode != 0:
        sys.exit("the device step ended with status %d" % child.returncode)
    out = json.loads(child.stdout.decode().strip().splitlines()[-1])
    if args.ref_images:
        ref = ref_step(args)
        out["slice_equal"] = ref.pop("slice_digest") == out.pop("slice_digest")
        out.update(ref)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
