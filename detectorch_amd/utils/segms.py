"""COCO segmentations for the batched path: polygons at image size to run lists on the device (hip_poly.py,
include/detectorch_poly_hip.h), and the reference's polygon helpers (lib/utils/segms.py) on top of that.

The reference converts polygons with pycocotools (frPyObjects / decode / annToRLE), which this project never assumes.  Here the
conversion is dtc_poly_rle, written from the published algorithm (common/maskApi.c: rleFrPoly, rleMerge); parity with pycocotools
itself is unpinned (tests/README_poly_rle.md).

    gt = pack_gt(roidb, device)
    gt.update(pack_gt_segms(segms_per_image, im_sizes, device))      # polygons, crowd RLEs, bitmaps, None -- as the file has them
    mask_evaluator.update(dets, det_count, rle, im_size, gt)

flip_segms is the reference's (segms.py:35-61): polygon lists are mirrored in Python doubles -- a list is loader data, and it is the
arithmetic of dtc_flip_polygons --, RLE dicts go through dtc_flip_rle (hip_flip.py), which mirrors the run list without a bitmap.

There is no CPU fallback: a polygon to convert, or an RLE to flip, needs a GPU.  polys_to_mask_wrt_box is csrc/mask_train's
(mask_rcnn_targets.py); the rle_mask_* functions of the reference are out of scope.
"""
import numpy as np
import torch

from .. import hip_flip, hip_poly
from . import result_utils
from .evaluator import pack_gt_masks
from .mask_rcnn_targets import pack_polygons

WORKSPACE_BUDGET = 1 << 28                                    # bytes of event keys in flight: pack_gt_segms converts in chunks of images


def pack_polygons64(polys_per_image, G, device=None, points=None, polys=None):
    """mask_rcnn_targets.pack_polygons with the points kept as float64 (COCO's coordinates are JSON doubles, and the conversion at
    image size rounds 5 x + 0.5 in double).  polys_per_image: per image, per gt row (at most G), a list of COCO polygons [x0, y0, x1,
    y1, ...] (a gt without polygons: an empty list or None).  -> (poly_xy f64 [B,PTS,2], poly_ptr i32 [B,NP+1], gt_poly_ptr i32
    [B,G+1]); `points` / `polys` fix PTS / NP (default: the largest image's, at least 1).  Rows past an image's own counts repeat the
    last offset (empty ranges)."""
    xy32, poly_ptr, gt_poly_ptr = pack_polygons(polys_per_image, G, None, points, polys)      # the layout, and its checks
    poly_xy = np.zeros(tuple(xy32.shape), np.float64)
    for b, im in enumerate(polys_per_image):
        pts = [np.asarray(poly, np.float64).reshape(-1, 2) for gt in im for poly in (gt if isinstance(gt, (list, tuple)) else [])]
        if pts:
            pts = np.concatenate(pts, 0)
            poly_xy[b, :len(pts)] = pts
    out = (torch.from_numpy(poly_xy), poly_ptr, gt_poly_ptr)
    return out if device is None else tuple(t.to(device) for t in out)


def polys_to_rle_batched(poly_xy, poly_ptr, gt_poly_ptr, gt_counts, im_size, runs_stride, events_stride, out=None, ws=None):
    """The thin, sync-free call of dtc_poly_rle on device tensors (hip_poly.poly_rle has the shapes).  -> dict(gt_runs i32
    [N,G,runs_stride] holding the uint32 run lengths, gt_n_runs i32 [N,G], area i32 [N,G], need i32 [N,G,2] = (events, runs) the row
    needs); the first two merge into the gt dict of MaskEvaluator.update.  A row with gt_n_runs = -1 did not fit runs_stride or
    events_stride: `need` says what it takes.  `out`: the dict of an earlier call, written in place (graph capture)."""
    raw = None if out is None else dict(runs=out["gt_runs"], n_runs=out["gt_n_runs"], area=out["area"], need=out["need"])
    raw = hip_poly.poly_rle(poly_xy, poly_ptr, gt_poly_ptr, gt_counts, im_size, runs_stride, events_stride, out=raw, ws=ws)
    return dict(gt_runs=raw["runs"], gt_n_runs=raw["n_runs"], area=raw["area"], need=raw["need"])


def is_polygons(segm):
    """a COCO `segmentation` field that is a list of polygons (not a bitmap, an RLE dict or None)"""
    return isinstance(segm, (list, tuple))


def _events_capacity(n):
    return next((c for c in hip_poly.SORT_CAPACITIES if c >= n), hip_poly.MAX_EVENTS)


def _convert(polys_per_image, sizes, dev, G, runs_stride, first):
    """the polygon rows of a chunk of images -> (the dict of polys_to_rle_batched, its need as numpy); first: the strides (events,
    runs) of the first attempt"""
    N = len(polys_per_image)
    xy, ptr, gptr = pack_polygons64(polys_per_image, G, dev)
    counts = torch.tensor([len(im) for im in polys_per_image], dtype=torch.int32, device=dev)
    im_size = torch.from_numpy(np.asarray(sizes, np.float32).reshape(N, 2)).to(dev)
    ev, rs = first
    res = polys_to_rle_batched(xy, ptr, gptr, counts, im_size, rs, ev)
    need = res["need"].cpu().numpy()                          # the one sync
    want_ev, want_rs = int(need[..., 0].max(initial=0)), int(need[..., 1].max(initial=0))
    fixed = runs_stride is not None
    if (want_ev > ev and ev < hip_poly.MAX_EVENTS) or (want_rs > rs and not fixed):
        ev = _events_capacity(want_ev)
        if not fixed:                                         # a row whose events did not fit: at most one run more than events
            unknown = bool((need[..., 1] < 0).any())
            rs = min(hip_poly.MAX_RUNS, max(rs, want_rs, min(want_ev, ev) + 1 if unknown else 0))
        res = polys_to_rle_batched(xy, ptr, gptr, counts, im_size, rs, ev)
        need = res["need"].cpu().numpy()
    return res, need


def pack_gt_segms(segms_per_image, im_sizes, device, G=None, runs_stride=None):
    """segms_per_image[i][j]: the COCO `segmentation` of gt row j of image i (the rows of pack_gt, in its order) in any form: a list
    of polygons [x0, y0, x1, y1, ...], converted on the device by dtc_poly_rle (annToRLE: the union of the polygons), or a form
    pack_gt_masks takes -- a binary [h, w] array, an uncompressed or compressed RLE dict (a crowd region), None --, converted on the
    host by pack_gt_masks itself; im_sizes [N, 2] = (h, w).  -> the dict of pack_gt_masks (gt_runs int32 [N, G, runs_stride], gt_n_runs
    int32 [N, G]) plus area int32 [N, G], the pixel count of every mask, on `device`.  Loader code: with polygons it syncs, sizes the
    buffers from what the rows need and converts again when the first guess was too small.  ValueError, naming the image and the
    row, when a row does not fit runs_stride (if given) or DTC_POLY_MAX_EVENTS."""
    N = len(segms_per_image)
    im_sizes = np.asarray(im_sizes).reshape(N, 2)
    host = [[None if is_polygons(m) else m for m in ms] for ms in segms_per_image]
    base = pack_gt_masks(host, im_sizes, "cpu", G, runs_stride)
    h_runs, h_n = base["gt_runs"].numpy().view(np.uint32), base["gt_n_runs"].numpy()
    G = h_n.shape[1]
    h_area = np.zeros((N, G), np.int64)
    for i in range(N):
        for j in range(G):
            h_area[i, j] = h_runs[i, j, 1:h_n[i, j]:2].astype(np.int64).sum()
    h_area = np.minimum(h_area, np.iinfo(np.int32).max).astype(np.int32)
    poly_rows = [(i, j) for i, ms in enumerate(segms_per_image) for j, m in enumerate(ms) if is_polygons(m)]
    if not poly_rows:
        return dict(gt_runs=base["gt_runs"].to(device), gt_n_runs=base["gt_n_runs"].to(device), area=torch.from_numpy(h_area).to(device))

    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("detectorch_amd converts polygons on the GPU only (got device %s); there is no CPU fallback" % dev)
    polys = [[m if is_polygons(m) else None for m in ms] for ms in segms_per_image]
    first = (hip_poly.SORT_CAPACITIES[0], 2048 if runs_stride is None else int(runs_stride))
    chunk = max(1, min(hip_poly.MAX_BATCH, WORKSPACE_BUDGET // (8 * hip_poly.MAX_EVENTS * G)))
    parts = []
    for i0 in range(0, N, chunk):
        res, need = _convert(polys[i0:i0 + chunk], im_sizes[i0:i0 + chunk], dev, G, runs_stride, first)
        n_runs = res["gt_n_runs"].cpu().numpy()
        for i, j in zip(*np.nonzero(n_runs < 0)):
            raise ValueError("pack_gt_segms: image %d gt %d: its polygons give %d events and %s runs: more than %s" % (
                i0 + i, j, need[i, j, 0], "an unknown number of" if need[i, j, 1] < 0 else need[i, j, 1],
                "DTC_POLY_MAX_EVENTS = %d" % hip_poly.MAX_EVENTS if need[i, j, 1] < 0 else "runs_stride = %d" % res["gt_runs"].shape[2]))
        parts.append((res, int(n_runs.max(initial=1))))
    stride = int(runs_stride) if runs_stride is not None else max([h_runs.shape[2]] + [s for _, s in parts])
    if stride > h_runs.shape[2]:
        h_runs = np.concatenate([h_runs, np.zeros((N, G, stride - h_runs.shape[2]), np.uint32)], 2)
    is_poly = np.zeros((N, G), bool)
    for i, j in poly_rows:
        is_poly[i, j] = True
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    col = torch.arange(stride, device=dev)
    d_runs, d_n, d_area = [], [], []
    for res, _ in parts:
        r = res["gt_runs"][:, :, :stride]
        if r.shape[2] < stride:
            r = torch.cat([r, r.new_zeros(r.shape[0], G, stride - r.shape[2])], 2)
        d_runs.append(torch.where(col[None, None, :] < res["gt_n_runs"][:, :, None], r, torch.zeros_like(r)))   # past n_runs: zeros, as the host rows
        d_n.append(res["gt_n_runs"])
        d_area.append(res["area"])
    sel = t(is_poly)
    return dict(gt_runs=torch.where(sel[:, :, None], torch.cat(d_runs), t(h_runs.view(np.int32))).contiguous(),
                gt_n_runs=torch.where(sel, torch.cat(d_n), t(h_n)), area=torch.where(sel, torch.cat(d_area), t(h_area)))


def polys_to_rle(polygons, height, width, device="cuda"):
    """One instance's list of COCO polygons -> its COCO RLE dict(size=[height, width], counts=<the compressed string>): annToRLE
    for a polygon annotation."""
    out = pack_gt_segms([[list(polygons)]], [(height, width)], device)
    n = int(out["gt_n_runs"][0, 0])
    counts = out["gt_runs"][0, 0, :n].cpu().numpy().view(np.uint32).astype(np.int64).tolist()
    return dict(size=[int(height), int(width)], counts=result_utils._rle_counts_to_string(counts))


def polys_to_mask(polygons, height, width):
    """The reference's segms.polys_to_mask: a list of COCO polygons -> the float32 [height, width] mask of their union, decoded from
    polys_to_rle."""
    counts = result_utils.rle_string_to_counts(polys_to_rle(polygons, height, width)["counts"])
    flat = np.zeros(int(height) * int(width), np.float32)
    ends = np.cumsum(counts)
    for k in range(1, len(counts), 2):
        flat[ends[k - 1]:ends[k]] = 1
    return flat.reshape(int(width), int(height)).T.copy()      # column-major: position x * h + y


def polys_to_boxes(polys):
    """The reference's segms.polys_to_boxes: per instance a list of polygons -> float32 [n, 4], the tight (x0, y0, x1, y1)."""
    boxes = np.zeros((len(polys), 4), np.float32)
    for i, poly in enumerate(polys):
        xs = np.concatenate([np.asarray(p, np.float64)[0::2] for p in poly])
        ys = np.concatenate([np.asarray(p, np.float64)[1::2] for p in poly])
        boxes[i] = [xs.min(), ys.min(), xs.max(), ys.max()]
    return boxes


def _flip_poly(poly, width):
    """segms.py:37-40: np.array(poly) is float64; x' = width - x - 1 in double, one rounding per subtraction"""
    out = [float(v) for v in poly]
    out[0::2] = [float(width) - x - 1.0 for x in out[0::2]]
    return out


def flip_rles(rles, height, width, device="cuda"):
    """RLE dicts (counts: an uncompressed list or a compressed str / bytes, as pack_gt_masks takes them) of one height x width image
    -> their left/right mirror images as dict(size=[height, width], counts=<the compressed string>), by dtc_flip_rle.  Loader code:
    it syncs for `need`, and calls again when a mirrored list is longer than the first guess."""
    if not rles:
        return []
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("detectorch_amd flips run lists on the GPU only (got device %s); there is no CPU fallback" % dev)
    height, width = int(height), int(width)
    packed = pack_gt_masks([list(rles)], [(height, width)], dev)
    runs, n_runs = packed["gt_runs"], packed["gt_n_runs"]
    im_size = torch.tensor([[height, width]], dtype=torch.float32, device=dev)
    res = hip_flip.flip_rle(runs, n_runs, im_size, [1])
    need = res["need"].cpu().numpy()                           # the one sync
    if int(need.max(initial=0)) > res["out_runs"].shape[2]:
        res = hip_flip.flip_rle(runs, n_runs, im_size, [1], out_stride=int(need.max()))
    n = res["out_n_runs"][0].cpu().numpy()
    out_runs = res["out_runs"][0].cpu().numpy().view(np.uint32)
    out = []
    for j in range(len(rles)):
        if n[j] < 0:
            raise ValueError("flip_segms: RLE %d does not describe a %d x %d mask (its runs must sum to height * width <= 2^30)" % (
                j, height, width))
        out.append(dict(size=[height, width], counts=result_utils._rle_counts_to_string(out_runs[j, :n[j]].astype(np.int64).tolist())))
    return out


def flip_segms(segms, height, width, device="cuda"):
    """The reference's segms.flip_segms: left/right flip each segmentation of a list, all of one height x width image.  A list of
    polygons is mirrored in Python doubles (no GPU needed); an RLE dict -- `counts` an uncompressed list or a compressed string --
    is mirrored on the device and comes back as dict(size, counts=<compressed string>), what the reference's encode returns."""
    rle_at = [i for i, segm in enumerate(segms) if not is_polygons(segm)]
    for i in rle_at:
        assert isinstance(segms[i], dict), "a segmentation is a list of polygons or an RLE dict"
    rles = iter(flip_rles([segms[i] for i in rle_at], height, width, device))
    return [[_flip_poly(poly, width) for poly in segm] if is_polygons(segm) else next(rles) for segm in segms]
