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

rle_mask_nms, rle_mask_voting and rle_masks_to_boxes are the reference's (segms.py:134-268) on dtc_mpost_* (hip_mpost.py,
include/detectorch_mpost_hip.h): overlaps, the greedy walk, the vote and the boxes are computed on the run lists, without a bitmap.
The *_batched forms take the device tensors of hip.mask_rle as they are and do not sync.

There is no CPU fallback: a polygon to convert, an RLE to flip, masks to suppress, vote or box need a GPU.  polys_to_mask_wrt_box is
csrc/mask_train's (mask_rcnn_targets.py).
"""
import numpy as np
import torch

from .. import hip_flip, hip_mpost, hip_poly
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


# ---- mask NMS, mask voting, mask boxes (the reference's segms.py:134-268) on run lists ----------------------------------------------------
def rle_masks_to_boxes_batched(runs, n_runs, im_size, counts=None, out=None):
    """rle_masks_to_boxes on device tensors in hip.mask_rle's layout: runs i32 [N,R,stride] (the uint32 run lengths), n_runs i32
    [N,R], im_size f32 [N,2] = (h, w), counts i32 [N] or None.  -> dict(boxes i32 [N,R,4] = the inclusive (x0, y0, x1, y1), zeros for
    an empty mask; area i32 [N,R]; nonempty i32 [N,R], the reference's `keep`).  `out`: the dict of an earlier call.  No host sync."""
    return hip_mpost.mask_boxes(runs, n_runs, im_size, counts, out=out)


def _pick(out, keys):
    return None if out is None else {k: out[k] for k in keys}


def rle_mask_nms_batched(runs, n_runs, dets, count, im_size, thresh, mode='IOU', out=None, ws=None):
    """rle_mask_nms on device tensors: runs i32 [N,R,stride] / n_runs i32 [N,R] (hip.mask_rle's), dets f32 [N,R,6] (score in column
    4, class in column 5: rows suppress rows of their own class only), count i32 [N], im_size f32 [N,2].  -> dict(keep i32 [N,R]: the
    kept rows in the order kept, then -1; keep_count i32 [N]; ovr f64 [N,R,R]: maskUtils.iou of the masks with themselves, with crowd
    for IOMA and CONTAINMENT; a_area, b_area i32 [N,R]: the masks' areas).  `out`: the dict of an earlier call, written in place;
    `ws`: a uint8 workspace (hip_mpost.overlaps_workspace_bytes).  No host sync."""
    if mode not in hip_mpost.NMS_MODES:
        raise NotImplementedError('Mode {} is unknown'.format(mode))
    pairs = hip_mpost.mask_overlaps(runs, n_runs, count, runs, n_runs, count, im_size, crowd=mode != 'IOU',
                                    out=_pick(out, ("ovr", "a_area", "b_area")), ws=ws)
    kept = hip_mpost.mask_nms(dets, count, pairs["ovr"], thresh, mode, out=_pick(out, ("keep", "keep_count")))
    return dict(kept, **pairs)


def rle_mask_voting_batched(top_runs, top_n_runs, top_count, all_runs, all_n_runs, all_dets, all_count, im_size, iou_thresh,
                            binarize_thresh, method='AVG', out_stride=None, out=None, ws=None):
    """rle_mask_voting on device tensors: the top masks (top_runs i32 [N,T,stride], top_n_runs i32 [N,T], top_count i32 [N]) are
    replaced by the vote of the masks of the pool (all_runs i32 [N,A,stride'], all_n_runs i32 [N,A], all_dets f32 [N,A,5 or more]:
    box and score, all_count i32 [N]) that overlap them by iou_thresh or more.  -> dict(out_runs i32 [N,T,out_stride], out_n_runs i32
    [N,T]: -1 where a list did not fit, need i32 [N,T]: what it takes; ovr f64 [N,T,A], a_area i32 [N,T], b_area i32 [N,A]: the
    overlaps and areas of tops and pool).  `out`: the dict of an earlier call, written in place; `ws`: a uint8 workspace of at least
    rle_mask_voting_workspace_bytes(...).  No host sync."""
    if method not in hip_mpost.VOTE_METHODS:
        raise NotImplementedError('Method {} is unknown'.format(method))
    pairs = hip_mpost.mask_overlaps(top_runs, top_n_runs, top_count, all_runs, all_n_runs, all_count, im_size, crowd=False,
                                    out=_pick(out, ("ovr", "a_area", "b_area")), ws=ws)
    voted = hip_mpost.mask_vote(top_runs, top_n_runs, top_count, all_runs, all_n_runs, all_dets, all_count, pairs["ovr"], im_size,
                                iou_thresh, binarize_thresh, method, out_stride=out_stride,
                                out=_pick(out, ("out_runs", "out_n_runs", "need")), ws=ws)
    return dict(voted, **pairs)


def rle_mask_voting_workspace_bytes(N, T, top_stride, A, all_stride):
    """the bytes of the `ws` that serves both stages of rle_mask_voting_batched (they run one after the other on one stream)"""
    return max(hip_mpost.overlaps_workspace_bytes(N, T, top_stride, A, all_stride), hip_mpost.vote_workspace_bytes(N, A, all_stride))


def _pack_one_image(masks, dev, what):
    """RLE dicts of one image -> (runs i32 [1,n,stride], n_runs i32 [1,n], count i32 [1], im_size f32 [1,2], [h, w])"""
    if dev.type != "cuda":
        raise RuntimeError("detectorch_amd runs %s on the GPU only (got device %s); there is no CPU fallback" % (what, dev))
    size = [int(v) for v in masks[0]['size']]
    for j, m in enumerate(masks):
        if [int(v) for v in m['size']] != size:
            raise ValueError("%s: mask %d is %s, mask 0 is %s: the masks of one call are of one image" % (what, j, list(m['size']), size))
    if len(masks) > hip_mpost.MAX_ROWS:
        raise ValueError("%s: at most %d masks in one call, got %d" % (what, hip_mpost.MAX_ROWS, len(masks)))
    packed = pack_gt_masks([list(masks)], [size], dev)
    count = torch.tensor([len(masks)], dtype=torch.int32, device=dev)
    return packed["gt_runs"], packed["gt_n_runs"], count, torch.tensor([size], dtype=torch.float32, device=dev), size


def rle_mask_nms(masks, dets, thresh, mode='IOU', device="cuda"):
    """The reference's segms.rle_mask_nms: greedy non-maximum suppression by mask overlap.  masks: RLE dicts (counts: an uncompressed
    list or a compressed str / bytes) of one image; dets [n, 5 or more], the score in column 4; mode 'IOU', 'IOMA' (intersection over
    the smaller area) or 'CONTAINMENT' (ious[m1, m2] = |m1 & m2| / area(m1)).  -> the list of kept indices by descending score;
    equal scores go by index (the reference's unstable argsort leaves them unspecified)."""
    if len(masks) == 0:
        return []
    if len(masks) == 1:
        return [0]
    if mode not in hip_mpost.NMS_MODES:
        raise NotImplementedError('Mode {} is unknown'.format(mode))
    dev = torch.device(device)
    runs, n_runs, count, im_size, _ = _pack_one_image(masks, dev, "rle_mask_nms")
    rows = np.zeros((1, len(masks), 6), np.float32)
    rows[0, :, 4] = np.asarray(dets, np.float32).reshape(len(masks), -1)[:, 4]
    rows[0, :, 5] = 1.0
    res = rle_mask_nms_batched(runs, n_runs, torch.from_numpy(rows).to(dev), count, im_size, float(thresh), mode)
    k = int(res["keep_count"][0])
    return [int(v) for v in res["keep"][0, :k].cpu().numpy()]


def rle_mask_voting(top_masks, all_masks, all_dets, iou_thresh, binarize_thresh, method='AVG', device="cuda"):
    """The reference's segms.rle_mask_voting: new masks, in correspondence with top_masks, from the masks of all_masks that overlap
    them by iou_thresh or more: 'AVG' binarizes their average, weighted by the score inside each voter's box and 1e-5 outside,
    'UNION' joins them.  Masks are RLE dicts of one image; all_dets [n, 5 or more]: box and score.  -> a list of RLE dicts: a voted
    mask as dict(size, counts=<compressed string>); a top mask that is empty or has fewer than two voters comes back as the caller's
    own dict, as in the reference.  No top masks: None, as in the reference.  Loader code: it syncs, and votes again when a voted
    list is longer than the first guess."""
    if method not in hip_mpost.VOTE_METHODS:
        raise NotImplementedError('Method {} is unknown'.format(method))
    if len(top_masks) == 0:
        return None
    if len(all_masks) == 0:                                    # nobody votes (the reference fails here)
        return list(top_masks)
    dev = torch.device(device)
    t_runs, t_n, t_count, im_size, size = _pack_one_image(top_masks, dev, "rle_mask_voting")
    a_runs, a_n, a_count, _, a_size = _pack_one_image(all_masks, dev, "rle_mask_voting")
    if a_size != size:
        raise ValueError("rle_mask_voting: top masks of %s and a pool of %s" % (size, a_size))
    d = np.asarray(all_dets, np.float32).reshape(len(all_masks), -1)
    if d.shape[1] < 5:
        raise ValueError("rle_mask_voting: all_dets [n, 5 or more], got %s" % (d.shape,))
    d = torch.from_numpy(np.ascontiguousarray(d[None])).to(dev)
    args = (t_runs, t_n, t_count, a_runs, a_n, d, a_count, im_size, float(iou_thresh), float(binarize_thresh), method)
    res = rle_mask_voting_batched(*args, out_stride=max(t_runs.shape[2], a_runs.shape[2]))
    need = res["need"].cpu().numpy()                           # the one sync
    if int(need.max(initial=0)) > res["out_runs"].shape[2]:
        res = rle_mask_voting_batched(*args, out_stride=int(need.max()))
    n = res["out_n_runs"][0].cpu().numpy()
    out_runs = res["out_runs"][0].cpu().numpy().view(np.uint32)
    ovr, area = res["ovr"][0].cpu().numpy(), res["a_area"][0].cpu().numpy()
    out = []
    for j, top in enumerate(top_masks):
        if n[j] < 0:
            raise ValueError("rle_mask_voting: top mask %d does not describe a %d x %d mask of at most 2^30 pixels" % (j, size[0], size[1]))
        if area[j] == 0 or int((ovr[j, :len(all_masks)] >= float(iou_thresh)).sum()) < 2:
            out.append(top)                                   # copied as it is: the caller's own dict
        else:
            out.append(dict(size=list(size), counts=result_utils._rle_counts_to_string(out_runs[j, :n[j]].astype(np.int64).tolist())))
    return out


def rle_masks_to_boxes(masks, device="cuda"):
    """The reference's segms.rle_masks_to_boxes: masks: RLE dicts of one image -> (boxes float64 [n, 4], the inclusive (x0, y0, x1,
    y1) of every mask, zeros for an empty one; the indices of the masks that are not empty).  No masks: []."""
    if len(masks) == 0:
        return []
    runs, n_runs, count, im_size, _ = _pack_one_image(masks, torch.device(device), "rle_masks_to_boxes")
    res = rle_masks_to_boxes_batched(runs, n_runs, im_size, count)
    return res["boxes"][0].cpu().numpy().astype(np.float64), np.where(res["nonempty"][0].cpu().numpy() != 0)[0]
