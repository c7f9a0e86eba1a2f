"""Box AP, mask AP and proposal recall, scored on the device (hip_eval.py, include/detectorch_eval_hip.h; hip_segm.py,
include/detectorch_segm_hip.h).

The reference scores its detections with pycocotools' COCOeval (lib/utils/json_dataset_evaluator.py:193-235 for boxes, :40-64 and
:116-124 for masks) and its proposals with evaluate_box_proposals (:238-319).  Here they run as HIP kernels on the fixed-shape
tensors of the batched path:

    ev = BoxEvaluator(num_classes=81)
    for batch in loader:
        dets, det_count = ...                      # RegionPath / forward_batched, or dist.ResultGatherer.finish()
        ev.update(dets, det_count, gt)             # gt: the dict the train steps take (+ optional gt_area); no host sync
    stats, per_class_ap = ev.summarize()           # COCO's twelve numbers, and the per-class AP the reference logs

    mv = MaskEvaluator(num_classes=81)             # the same for iouType 'segm'
    ...
        rle = hip.mask_rle(hip.mask_paste(...), det_count, im_size)
        mv.update(dets, det_count, rle, im_size, dict(gt, **pack_gt_masks(gt_masks, im_sizes, device)))
    stats, per_class_ap = mv.summarize()

Ground-truth polygons go through utils/segms.py:pack_gt_segms (polygon -> RLE at image size on the device, hip_poly.py;
pack_gt_masks itself takes bitmaps and RLEs); evaluate_masks takes either.
Out of scope: keypoint evaluation (OKS), json files and category ids (result_utils.coco_bbox_results / coco_segm_results stay the way
to an external scorer), reducing the records across ranks (gather the detections first, as dist.py does), non-finite scores.
"""
import warnings

import numpy as np
import torch

from .. import hip_eval
from .. import hip_segm
from . import result_utils

# the reference's eight named area ranges (json_dataset_evaluator.py:247-264)
PROPOSAL_AREAS = {'all': (0 ** 2, 1e5 ** 2), 'small': (0 ** 2, 32 ** 2), 'medium': (32 ** 2, 96 ** 2), 'large': (96 ** 2, 1e5 ** 2),
                  '96-128': (96 ** 2, 128 ** 2), '128-256': (128 ** 2, 256 ** 2), '256-512': (256 ** 2, 512 ** 2),
                  '512-inf': (512 ** 2, 1e5 ** 2)}


def coco_defaults():
    """COCOeval's Params for 'bbox': (iouThrs, recThrs, maxDets, areaRng)"""
    iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    area_rngs = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64)
    return iou_thrs, rec_thrs, (1, 10, 100), area_rngs


def summarize_stats(precision, recall, iou_thrs):
    """COCOeval.summarize for 'bbox' from precision [T,R,K,A,M] and recall [T,K,A,M]: the mean over the entries > -1 (numpy's own
    summation), -1 without any.  Defined for COCO's shape (A = 4 area ranges all / small / medium / large, M = 3 max_dets) only: any
    other shape leaves the twelve numbers -1."""
    stats = np.full(12, -1.0)
    if precision.shape[3] != 4 or precision.shape[4] != 3 or len(iou_thrs) != 10:
        return stats

    def one(ap, iou_thr=None, a=0, m=2):
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[..., [a], [m]]
        s = s[s > -1]
        return -1.0 if len(s) == 0 else np.mean(s)

    stats[0] = one(1)
    stats[1] = one(1, iou_thr=.5)
    stats[2] = one(1, iou_thr=.75)
    stats[3], stats[4], stats[5] = one(1, a=1), one(1, a=2), one(1, a=3)
    stats[6], stats[7], stats[8] = one(0, m=0), one(0, m=1), one(0, m=2)
    stats[9], stats[10], stats[11] = one(0, a=1), one(0, a=2), one(0, a=3)
    return stats


def per_class_ap(precision, iou_thrs, lo=0.5, hi=0.95):
    """the mean and per-category AP @ IoU=[lo, hi] the reference logs (json_dataset_evaluator.py:205-233): area range 0, the last
    max_dets.  -> (mean, [K]); nan where a class has no entry > -1 (np.mean of nothing, as there)."""
    ind = lambda thr: np.where((iou_thrs > thr - 1e-5) & (iou_thrs < thr + 1e-5))[0][0]
    p = precision[ind(lo):ind(hi) + 1, :, :, 0, -1]
    mean = lambda s: float(np.mean(s[s > -1])) if (s > -1).any() else float('nan')
    return mean(p), np.array([mean(p[:, :, k]) for k in range(p.shape[2])])


class BoxEvaluator:
    """Streaming COCO box AP.  update() runs dtc_eval_match on one batch and keeps its records on the device without a host sync;
    accumulate() sorts the keys of the whole run once (torch.sort, stable), runs dtc_eval_accumulate and makes the one sync.
    update() can be captured in a torch.cuda.graph after one eager call: a replay rewrites the records of the captured call in place
    (with the image_base it was captured with)."""

    def __init__(self, num_classes=81, iou_thrs=None, rec_thrs=None, max_dets=(1, 10, 100), area_rngs=None, device="cuda",
                 on_overflow="raise"):
        if on_overflow not in ("raise", "truncate"):
            raise ValueError("on_overflow must be 'raise' or 'truncate'")
        d_iou, d_rec, _, d_area = coco_defaults()
        self.num_classes = int(num_classes)
        self.iou_thrs = np.ascontiguousarray(d_iou if iou_thrs is None else iou_thrs, np.float64).reshape(-1)
        self.rec_thrs = np.ascontiguousarray(d_rec if rec_thrs is None else rec_thrs, np.float64).reshape(-1)
        self.area_rngs = np.ascontiguousarray(d_area if area_rngs is None else area_rngs, np.float64).reshape(-1, 2)
        self.max_dets = tuple(int(m) for m in max_dets)        # used as given, like COCOeval's: summarize indexes it by position
        if any(b < a for a, b in zip(self.max_dets, self.max_dets[1:])):
            raise ValueError("max_dets must be non-decreasing (the last one cuts the detections of an image), got %s" % (self.max_dets,))
        if np.any(np.diff(self.rec_thrs) < 0):
            raise ValueError("rec_thrs must be non-decreasing")
        T, A = len(self.iou_thrs), len(self.area_rngs)
        if not (T >= 1 and 1 <= A <= hip_eval.MAX_AREAS and T * A <= hip_eval.MAX_PAIRS and
                1 <= len(self.rec_thrs) <= hip_eval.MAX_REC_THRS and 1 <= len(self.max_dets) <= hip_eval.MAX_MAX_DETS and
                self.max_dets[0] >= 1 and 2 <= self.num_classes <= hip_eval.MAX_CLASSES):
            raise ValueError("BoxEvaluator: unsupported parameters: %d thresholds x %d area ranges (at most %d pairs, %d ranges), %d "
                             "recall thresholds (at most %d), max_dets %s (at most %d, each >= 1), %d classes (2 .. %d)" %
                             (T, A, hip_eval.MAX_PAIRS, hip_eval.MAX_AREAS, len(self.rec_thrs), hip_eval.MAX_REC_THRS, self.max_dets,
                              hip_eval.MAX_MAX_DETS, self.num_classes, hip_eval.MAX_CLASSES))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("detectorch_amd runs the evaluation on the GPU only (got device %s); there is no CPU fallback" % self.device)
        self.on_overflow = on_overflow
        dev = self.device
        self._iou_thrs, self._rec_thrs = torch.from_numpy(self.iou_thrs).to(dev), torch.from_numpy(self.rec_thrs).to(dev)
        self._area_rngs = torch.from_numpy(self.area_rngs).to(dev)
        self._max_dets = torch.tensor(self.max_dets, dtype=torch.int32, device=dev)
        self.reset()

    def reset(self):
        self._records, self._counts, self.n_images, self._result = [], [], 0, None

    def update(self, dets, det_count, gt):
        """dets f32 [N,max_out,6] and det_count i32 [N] on the device; gt: gt_boxes f32 [N,G,4] (original image coordinates),
        gt_classes / gt_is_crowd i32 [N,G], gt_counts i32 [N], optional gt_area f32 [N,G] (None: the box area).  Every call must
        have the same max_out.  -> the records of this call (the dict of hip_eval.match_outputs).  No host sync: an image with
        det_count > max_out is reported by accumulate(), as on_overflow says."""
        if self._records and dets.shape[1] != self._records[0]["dt_rank"].shape[1]:
            raise ValueError("update: max_out changed from %d to %d" % (self._records[0]["dt_rank"].shape[1], dets.shape[1]))
        rec = hip_eval.eval_match(dets, det_count, gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"], gt.get("gt_area"),
                                  self.num_classes, self._iou_thrs, self._area_rngs, self.max_dets[-1], image_base=self.n_images)
        self._records.append(rec)
        self._counts.append((det_count.clone(), dets.shape[1]))      # the caller may reuse its buffer for the next batch
        self.n_images += dets.shape[0]
        self._result = None
        return rec

    def accumulate(self):
        """-> dict(precision [T,R,K,A,M], recall [T,K,A,M], stats [12], counts [K,A]) as numpy; one host sync"""
        if not self._records:
            raise RuntimeError("accumulate: no update() yet")
        cat = lambda k: torch.cat([r[k].reshape(-1) for r in self._records])
        out = hip_eval.eval_accumulate(cat("dt_rank"), cat("dt_match"), cat("dt_ignore"), cat("sort_key"),
                                       torch.cat([r["npig"] for r in self._records]), self.num_classes, len(self.iou_thrs),
                                       len(self.area_rngs), self._rec_thrs, self._max_dets)
        det_count = torch.cat([c.reshape(-1) for c, _ in self._counts])
        precision, recall, counts, det_count = (t.cpu().numpy() for t in (out["precision"], out["recall"], out["counts"], det_count))
        max_out = self._counts[0][1]
        over = np.flatnonzero(det_count > max_out)
        if len(over):      # ties at the image threshold beyond the fixed rows (result_utils.assemble_results)
            msg = "image %d: %d detections but only %d rows were kept: raise the path's max_out" % (over[0], det_count[over[0]], max_out)
            if self.on_overflow == "raise":
                raise RuntimeError(msg)
            warnings.warn(msg + " -- truncated", RuntimeWarning)
        self._result = dict(precision=precision, recall=recall, stats=summarize_stats(precision, recall, self.iou_thrs), counts=counts)
        return self._result

    def summarize(self):
        """-> (stats [12]: AP, AP50, AP75, AP small / medium / large, AR at max_dets[0..2], AR small / medium / large;
        dict(mean=, per_class=[K]): the AP @ IoU=[.5,.95] of all classes and of each class, as the reference logs them)"""
        res = self._result or self.accumulate()
        try:
            mean, per_class = per_class_ap(res["precision"], self.iou_thrs)
        except IndexError:                                   # thresholds without .5 or .95
            mean, per_class = float('nan'), np.full(self.num_classes - 1, np.nan)
        return res["stats"], dict(mean=mean, per_class=per_class)


class MaskEvaluator(BoxEvaluator):
    """Streaming COCO mask AP (COCOeval's iouType 'segm'): BoxEvaluator with the IoU of a pair taken between the masks
    (dtc_segm_iou: maskApi.c's rleIou on the run lists) and the area of a detection being its mask's pixel count; the records, the
    accumulation and the summary are the box protocol's.  update() makes no host sync and can be captured like BoxEvaluator's."""

    def reset(self):
        super().reset()
        self._bad = []

    def update(self, dets, det_count, det_rle, im_size, gt):
        """dets f32 [N,max_out,6] and det_count i32 [N] on the device; det_rle: the dict hip.mask_rle returns (counts [N,max_out,
        runs_stride], n_runs i32 [N,max_out]; the strings are not read); im_size [N,2] = (h, w) of the original images; gt: the dict
        of BoxEvaluator.update (gt_boxes is not read) plus gt_runs [N,G,runs_stride'] / gt_n_runs i32 [N,G] (pack_gt_masks);
        gt_area f32 [N,G] is the area of a gt when given (COCO's annotation area), else its mask's pixel count.  Every call must
        have the same max_out.  -> the records of this call (hip_eval.match_outputs) plus iou, det_area, gt_mask_area and n_bad.
        No host sync: a mask that did not fit hip.mask_rle's buffers (n_runs < 0) is scored as empty and reported by accumulate(),
        as on_overflow says, like an image with det_count > max_out."""
        if self._records and dets.shape[1] != self._records[0]["dt_rank"].shape[1]:
            raise ValueError("update: max_out changed from %d to %d" % (self._records[0]["dt_rank"].shape[1], dets.shape[1]))
        pairs = hip_segm.segm_iou(dets, det_count, det_rle["counts"], det_rle["n_runs"], im_size.to(torch.float32).contiguous(),
                                  gt["gt_runs"], gt["gt_n_runs"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"], self.num_classes)
        rec = hip_segm.segm_match(dets, det_count, pairs["iou"], pairs["det_area"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"],
                                  gt.get("gt_area"), pairs["gt_mask_area"], self.num_classes, self._iou_thrs, self._area_rngs,
                                  self.max_dets[-1], image_base=self.n_images)
        rec.update(pairs)
        self._records.append(rec)
        self._counts.append((det_count.clone(), dets.shape[1]))
        self._bad.append(pairs["n_bad"])
        self.n_images += dets.shape[0]
        self._result = None
        return rec

    def accumulate(self):
        res = super().accumulate()
        n_bad = torch.cat(self._bad).cpu().numpy()
        bad = np.flatnonzero(n_bad > 0)
        if len(bad):
            msg = ("image %d: %d masks did not fit the RLE buffers (negative n_runs), %d in the run: encode them again with a larger "
                   "runs_stride / crop capacity" % (bad[0], n_bad[bad[0]], int(n_bad.sum())))
            if self.on_overflow == "raise":
                self._result = None
                raise RuntimeError(msg)
            warnings.warn(msg + " -- scored as empty masks", RuntimeWarning)
        return res


def pack_gt(roidb, device, G=None):
    """roidb-style dicts (boxes, gt_classes, is_crowd, seg_areas; rows with gt_classes == 0 are proposals and left out) -> the gt dict
    of BoxEvaluator.update on `device`"""
    rows = [np.flatnonzero(np.asarray(e['gt_classes']) > 0) for e in roidb]
    N, G = len(roidb), max([1] + [len(r) for r in rows]) if G is None else G
    boxes, cls, crowd = np.zeros((N, G, 4), np.float32), np.zeros((N, G), np.int32), np.zeros((N, G), np.int32)
    area, counts = np.zeros((N, G), np.float32), np.zeros(N, np.int32)
    for i, (e, r) in enumerate(zip(roidb, rows)):
        n = counts[i] = len(r)
        boxes[i, :n] = np.asarray(e['boxes'], np.float32).reshape(-1, 4)[r]
        cls[i, :n], crowd[i, :n] = np.asarray(e['gt_classes'])[r], np.asarray(e['is_crowd'])[r]
        area[i, :n] = np.asarray(e['seg_areas'], np.float32)[r]
    t = lambda a: torch.from_numpy(a).to(device)
    return dict(gt_boxes=t(boxes), gt_classes=t(cls), gt_is_crowd=t(crowd), gt_counts=t(counts), gt_area=t(area))


def evaluate_boxes(all_boxes, roidb, device="cuda", batch=256, **evaluator_args):
    """The reference-shaped convenience: all_boxes[cls][image] = [k,5] (x1,y1,x2,y2,score) as result_utils.assemble_results leaves
    them, roidb: a list of dicts (boxes, gt_classes, is_crowd, seg_areas).  -> the BoxEvaluator after accumulate()."""
    num_classes, N = len(all_boxes), len(roidb)
    per_image = [[(j, np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5)) for j in range(1, num_classes) if len(all_boxes[j][i])]
                 for i in range(N)]
    count = [sum(len(d) for _, d in p) for p in per_image]
    max_out = max([1] + count)
    if max_out > hip_eval.MAX_OUT:
        raise ValueError("evaluate_boxes: an image has %d detections, at most %d" % (max_out, hip_eval.MAX_OUT))
    G = max([1] + [int((np.asarray(e['gt_classes']) > 0).sum()) for e in roidb])
    ev = BoxEvaluator(num_classes=num_classes, device=device, **evaluator_args)
    for i0 in range(0, N, batch):
        i1 = min(N, i0 + batch)
        dets = np.zeros((i1 - i0, max_out, 6), np.float32)
        for i in range(i0, i1):
            at = 0
            for j, d in per_image[i]:
                dets[i - i0, at:at + len(d), :5], dets[i - i0, at:at + len(d), 5] = d, j
                at += len(d)
        ev.update(torch.from_numpy(dets).to(ev.device), torch.tensor(count[i0:i1], dtype=torch.int32, device=ev.device),
                  pack_gt(roidb[i0:i1], ev.device, G))
    ev.accumulate()
    return ev


def _gt_runs(m, h, w, where):
    """one gt mask in any accepted form -> its run lengths as int64, or None"""
    if m is None:
        return None
    if isinstance(m, dict):
        if [int(v) for v in m['size']] != [h, w]:
            raise ValueError("%s: an RLE of size %s in an image of size %s" % (where, list(m['size']), [h, w]))
        c = m['counts']
        runs = np.asarray(result_utils.rle_string_to_counts(c) if isinstance(c, (str, bytes)) else c, np.int64).reshape(-1)
    else:
        m = np.asarray(m)
        if m.shape != (h, w):
            raise ValueError("%s: a bitmap of shape %s in an image of size %s" % (where, m.shape, (h, w)))
        runs = np.asarray(result_utils.rle_counts(m), np.int64)
    if len(runs) and (runs.min() < 0 or runs.max() > 0xffffffff):
        raise ValueError("%s: run lengths must be in 0 .. 2^32 - 1" % where)
    return runs


def pack_gt_masks(masks_per_image, im_sizes, device, G=None, runs_stride=None):
    """masks_per_image[i][j]: the mask of gt row j of image i (the rows of pack_gt, in its order) as a binary [h, w] array, an
    uncompressed RLE (dict(size=[h, w], counts=list)), a compressed RLE (counts as str / bytes) or None (no segmentation: an empty
    mask); im_sizes [N, 2] = (h, w).  -> dict(gt_runs int32 [N, G, runs_stride] holding the uint32 run lengths, gt_n_runs int32
    [N, G]) on `device`, to be merged into the gt dict of MaskEvaluator.update.  Polygons are not taken here:
    utils/segms.py:pack_gt_segms converts them at image size on the device (annToRLE) and hands every other form to this function."""
    im_sizes = np.asarray(im_sizes).reshape(len(masks_per_image), 2)
    runs = [[_gt_runs(m, int(im_sizes[i, 0]), int(im_sizes[i, 1]), "image %d gt %d" % (i, j)) for j, m in enumerate(ms)]
            for i, ms in enumerate(masks_per_image)]
    N = len(runs)
    need_G, need_stride = max([1] + [len(r) for r in runs]), max([1] + [len(x) for r in runs for x in r if x is not None])
    G, runs_stride = need_G if G is None else int(G), need_stride if runs_stride is None else int(runs_stride)
    if need_G > G or need_stride > runs_stride:
        raise ValueError("pack_gt_masks: %d gt of up to %d runs do not fit G = %d, runs_stride = %d" % (need_G, need_stride, G, runs_stride))
    out, n_runs = np.zeros((N, G, runs_stride), np.uint32), np.zeros((N, G), np.int32)
    for i, r in enumerate(runs):
        for j, x in enumerate(r):
            if x is not None:
                out[i, j, :len(x)], n_runs[i, j] = x, len(x)
    return dict(gt_runs=torch.from_numpy(out.view(np.int32)).to(device), gt_n_runs=torch.from_numpy(n_runs).to(device))


def evaluate_masks(all_boxes, all_segms, roidb, gt_masks, device="cuda", batch=64, **evaluator_args):
    """The reference-shaped convenience (json_dataset_evaluator.py:evaluate_masks without the json files): all_boxes[cls][image] =
    [k,5] and all_segms[cls][image] = k RLE dicts (size, compressed counts) as result_utils.assemble_results leaves them; roidb: a
    list of dicts (boxes, gt_classes, is_crowd, seg_areas as for evaluate_boxes; height and width, or the sizes are read off the RLEs); gt_masks[image][j]: the
    mask of the j-th row with gt_classes > 0, in any form pack_gt_masks takes, or a list of COCO polygons (the annotation's
    `segmentation` as it is: converted at image size on the device, utils/segms.py:pack_gt_segms; the roidb entry must then carry
    height and width unless another mask of the image tells them).  -> the MaskEvaluator after accumulate().
    Out of scope: json files, category ids, keypoints."""
    num_classes, N = len(all_boxes), len(roidb)
    per_image, sizes = [], np.zeros((N, 2), np.int64)
    for i in range(N):
        rows = []
        for j in range(1, num_classes):
            b = np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5)
            if len(b) != len(all_segms[j][i]):
                raise ValueError("evaluate_masks: image %d class %d: %d boxes and %d masks" % (i, j, len(b), len(all_segms[j][i])))
            rows += [(j, b[k], all_segms[j][i][k]) for k in range(len(b))]
        per_image.append(rows)
        e = roidb[i]
        known = [s['size'] for _, _, s in rows] + [m['size'] for m in gt_masks[i] if isinstance(m, dict)] + \
                [np.asarray(m).shape for m in gt_masks[i] if m is not None and not isinstance(m, (dict, list, tuple))]
        if 'height' in e and 'width' in e:
            sizes[i] = (e['height'], e['width'])
        elif known:
            sizes[i] = known[0]
        elif any(isinstance(m, (list, tuple)) for m in gt_masks[i]):
            raise ValueError("evaluate_masks: image %d has polygons and nothing tells its size: give height and width in the roidb" % i)
        for _, _, s in rows:
            if [int(v) for v in s['size']] != sizes[i].tolist():
                raise ValueError("evaluate_masks: image %d: a mask of size %s in an image of size %s" % (i, list(s['size']), sizes[i].tolist()))
    det_runs = [[np.asarray(result_utils.rle_string_to_counts(s['counts']) if isinstance(s['counts'], (str, bytes)) else s['counts'],
                            np.int64) for _, _, s in rows] for rows in per_image]
    max_out, stride = max([1] + [len(r) for r in per_image]), max([1] + [len(x) for r in det_runs for x in r])
    if max_out > hip_eval.MAX_OUT:
        raise ValueError("evaluate_masks: an image has %d detections, at most %d" % (max_out, hip_eval.MAX_OUT))
    n_gt = [int((np.asarray(e['gt_classes']) > 0).sum()) for e in roidb]
    G = max([1] + n_gt)
    gt_stride = None
    ev = MaskEvaluator(num_classes=num_classes, device=device, **evaluator_args)
    dev = ev.device
    for i0 in range(0, N, batch):
        i1 = min(N, i0 + batch)
        dets, counts = np.zeros((i1 - i0, max_out, 6), np.float32), np.zeros((i1 - i0, max_out, stride), np.uint32)
        n_runs = np.zeros((i1 - i0, max_out), np.int32)
        for i in range(i0, i1):
            for at, (j, b, _) in enumerate(per_image[i]):
                dets[i - i0, at, :5], dets[i - i0, at, 5] = b, j
                x = det_runs[i][at]
                counts[i - i0, at, :len(x)], n_runs[i - i0, at] = x, len(x)
        gt = pack_gt(roidb[i0:i1], dev, G)                      # gt_boxes is not read
        if any(isinstance(m, (list, tuple)) for ms in gt_masks[i0:i1] for m in ms):
            from . import segms                                # (segms imports this module)
            packed = segms.pack_gt_segms(gt_masks[i0:i1], sizes[i0:i1], dev, G, gt_stride)
            gt.update(gt_runs=packed["gt_runs"], gt_n_runs=packed["gt_n_runs"])
        else:
            gt.update(pack_gt_masks(gt_masks[i0:i1], sizes[i0:i1], dev, G, gt_stride))
        t = lambda a: torch.from_numpy(a).to(dev)
        ev.update(t(dets), torch.tensor([len(r) for r in per_image[i0:i1]], dtype=torch.int32, device=dev),
                  dict(counts=t(counts.view(np.int32)), n_runs=t(n_runs)), t(sizes[i0:i1].astype(np.float32)), gt)
    ev.accumulate()
    return ev


# the IoU thresholds of the recall summary when none are given: .5 to .95 in steps of .05, as the reference builds them
# (json_dataset_evaluator.py:309-311), so that the recalls compare bit for bit
DEFAULT_RECALL_THRESHOLDS = np.arange(0.5, 0.95 + 1e-5, 0.05)


def _recall_summary(gt_overlaps, num_pos, thresholds):
    """The summary of json_dataset_evaluator.py:308-319 on the recorded overlaps: per threshold the share of the num_pos gt whose
    overlap reaches it, and the mean of those shares.  num_pos == 0 gives nan, as there."""
    overlaps = np.sort(gt_overlaps)
    thresholds = DEFAULT_RECALL_THRESHOLDS.copy() if thresholds is None else np.asarray(thresholds)
    reached = (overlaps[None, :] >= thresholds.reshape(-1, 1)).sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        recalls = (reached / float(num_pos)).astype(thresholds.dtype).reshape(thresholds.shape)
    return dict(ar=recalls.mean(), recalls=recalls, thresholds=thresholds, gt_overlaps=overlaps, num_pos=num_pos)


def evaluate_box_proposals_batched(proposals, prop_counts, gt, thresholds=None, area='all', limit=None):
    """evaluate_box_proposals on device tensors: proposals f32 [N,P,4] in score order, prop_counts i32 [N], gt: the dict of
    BoxEvaluator.update (gt_area: the roidb's seg_areas; None: the box area).  One kernel, one host sync, then the reference's
    tiny summary on the host.  -> the reference's dict: ar, recalls, thresholds, gt_overlaps (sorted), num_pos.
    limit: None keeps every proposal, n >= 1 the first n of an image; 0 keeps none, as the reference's boxes[:0] does: an image
    that has proposals then still records a zero for each of its gt (the library's own limit = 0 means "no limit")."""
    if area not in PROPOSAL_AREAS:
        raise ValueError("area must be one of %s, got %r" % (sorted(PROPOSAL_AREAS), area))
    if limit is not None and int(limit) < 0:
        raise ValueError("limit must be None or >= 0, got %r" % (limit,))
    rng = torch.tensor(PROPOSAL_AREAS[area], dtype=torch.float64, device=proposals.device)
    out = hip_eval.proposal_recall(proposals, prop_counts, gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"],
                                   gt.get("gt_area"), rng, limit=0 if limit is None else int(limit))
    ov, n_pos, n_ov = (out[k].cpu().numpy() for k in ("gt_overlaps", "n_pos", "n_overlaps"))
    if limit is not None and int(limit) == 0:
        ov = np.zeros_like(ov)                     # no proposal is kept: no round is run, the entries of n_overlaps stay
    gt_overlaps = np.concatenate([np.zeros(0)] + [ov[i, :n_ov[i]] for i in range(len(n_ov))])
    return _recall_summary(gt_overlaps, int(n_pos.sum()), thresholds)


def evaluate_box_proposals(roidb, thresholds=None, area='all', limit=None, device="cuda"):
    """The reference's evaluate_box_proposals (json_dataset_evaluator.py:238-319) without json_dataset: in every roidb entry the rows
    with gt_classes == 0 are the proposals, in score order, the others the gt.  Same dict."""
    props = [np.asarray(e['boxes'], np.float32).reshape(-1, 4)[np.flatnonzero(np.asarray(e['gt_classes']) == 0)] for e in roidb]
    N, P = len(roidb), max([1] + [len(p) for p in props])
    boxes, counts = np.zeros((N, P, 4), np.float32), np.zeros(N, np.int32)
    for i, p in enumerate(props):
        boxes[i, :len(p)], counts[i] = p, len(p)
    dev = torch.device(device)
    return evaluate_box_proposals_batched(torch.from_numpy(boxes).to(dev), torch.from_numpy(counts).to(dev), pack_gt(roidb, dev),
                                          thresholds, area, limit)
