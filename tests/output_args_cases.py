"""Inputs and oracle-side expectations of the output-stage argument tests (test support, not a test module): shared by
tests/test_hip_mask_output_args.py, tests/test_hip_det_args.py (GPU) and tests/test_output_args_host.py, which pins on the oracle
alone the conditions the GPU tests rely on (so that none of them can pass emptily).  Everything here is numpy + the oracle."""
import numpy as np

from detectorch_amd import synth

BAND_PIXELS = 4096                 # mask_paste.hip: kBandPixels (a larger paste rectangle is cut into bands, helpers take bands 1..)
MASK_SIDES = (1, 2, 7, 14, 28, 56, 62)


# ---- mask paste / RLE ----------------------------------------------------------------------------------------------------------
def paste_ref(orc, mask, ref_box, im_h, im_w, thresh=0.5):
    """result_utils.py:182-214 for one detection from the oracle -> (expanded int box [4], paste rect (x0, y0, x1, y1) as
    dtc_mask_paste publishes it, crop uint8 [y1 - y0, x1 - x0] = the frame's content inside the rect)"""
    box, crop = orc.mask_resize_binarize(mask, ref_box, thresh)
    x0, x1 = max(int(box[0]), 0), min(int(box[2]) + 1, im_w)
    y0, y1 = max(int(box[1]), 0), min(int(box[3]) + 1, im_h)
    x1, y1 = max(x1, x0), max(y1, y0)
    if x1 > x0 and y1 > y0:
        sub = np.ascontiguousarray(crop[y0 - box[1]:y1 - box[1], x0 - box[0]:x1 - box[0]])
    else:
        sub = np.zeros((y1 - y0, x1 - x0), np.uint8)
    assert sub.shape == (y1 - y0, x1 - x0)
    return box, (x0, y0, x1, y1), sub


def frame_of(sub, rect, im_h, im_w):
    x0, y0, x1, y1 = rect
    fr = np.zeros((im_h, im_w), np.uint8)
    fr[y0:y1, x0:x1] = sub
    return fr


def paste_expectation(orc, masks_of, boxes, im_sizes, thresh=0.5):
    """boxes: per image [n_b, 4] reference boxes; masks_of(b, d) -> the [M, M] mask the detection must use; im_sizes [(h, w)] ints.
    -> per image dict(box [n,4], rect [n,4], area [n], off [n] (exclusive prefix of the areas), bytes, crop list)"""
    out = []
    for b, rb in enumerate(boxes):
        im_h, im_w = im_sizes[b]
        bx, rc, cr = [], [], []
        for d in range(len(rb)):
            box, rect, sub = paste_ref(orc, masks_of(b, d), rb[d], im_h, im_w, thresh)
            bx.append(box); rc.append(rect); cr.append(sub)
        area = np.array([c.size for c in cr], np.int64)
        off = np.concatenate([[0], np.cumsum(area)[:-1]]).astype(np.int64) if len(rb) else np.zeros(0, np.int64)
        out.append(dict(box=np.array(bx, np.int32).reshape(-1, 4), rect=np.array(rc, np.int32).reshape(-1, 4), area=area, off=off,
                        bytes=int(area.sum()), crop=cr))
    return out


OVERFLOW_SIZES = [(120, 160), (97, 131), (61, 83)]
OVERFLOW_K, OVERFLOW_Z = 3, 4      # image 1: the multi-band detection and the zero-area rectangle behind it


def overflow_batch(M=28):
    """1a: three images of different sizes with 9, 7 and 0 detections; image 1 holds a multi-band box mid-list (row OVERFLOW_K)
    and, right behind it, a box fully outside the image (row OVERFLOW_Z: zero-area paste rectangle).
    -> (boxes per image, classes per image, masks [3 * 16, 3, M, M] in (b * 16 + d) order)"""
    rs = synth.rng(41, M)
    b0 = synth.make_rois(rs, 9, im_h=120, im_w=160, min_side=4, max_side=110)
    b0[2] = [-12, 30, 70, 140]                                     # clipped left and bottom
    b1 = np.array([[5, 5, 30, 25], [40, 10, 70, 60], [-10, -10, 50, 40], [10, 5, 120, 90], [200, 200, 230, 240],
                   [60, 30, 100, 80], [1, 50, 20, 96]], np.float32)
    boxes = [b0.astype(np.float32), b1, np.zeros((0, 4), np.float32)]
    cls = [rs.randint(1, 3, len(rb)) for rb in boxes]
    masks = synth.make_masks(rs, 3 * 16, 3, M)
    return boxes, cls, masks


def overflow_capacities(exp):
    """the per_image_capacity values of 1a from the oracle geometry: everything fits (one image exactly); one byte short of
    image 1; one byte short of the multi-band detection; exactly its offset; exactly the zero-area rectangle's offset (the
    multi-band detection fits to the byte and the rectangle sits AT the capacity); nothing"""
    e1 = exp[1]
    k, z = OVERFLOW_K, OVERFLOW_Z
    return [max(e["bytes"] for e in exp), e1["bytes"] - 1, int(e1["off"][k] + e1["area"][k] - 1), int(e1["off"][k]),
            int(e1["off"][z]), 0]


def tie_case():
    """1c: M = 28, mask values on the 1/8 grid, expanded box exactly 60 x 60 -> (mask [28,28], ref box, values [60,60] float32 by a
    numpy restatement of the resize rule (mask_paste.hip header): every fraction is 0, 0.25 or 0.75, every product exact)"""
    M, S, n = 28, 30, 60
    mask = (np.random.RandomState(0).randint(0, 9, (M, M)) / 8.0).astype(np.float32)
    ref_box = np.array([100, 100, 155.25, 155.25], np.float32)
    pm = np.zeros((S, S), np.float32)
    pm[1:M + 1, 1:M + 1] = mask
    f = ((np.arange(n) + 0.5) * (S / float(n)) - 0.5).astype(np.float32)
    s0 = np.floor(f).astype(np.int64)
    fr = (f - s0.astype(np.float32)).astype(np.float32)
    lo, hi = s0 < 0, s0 >= S - 1
    s0[lo], fr[lo] = 0, 0
    s0[hi], fr[hi] = S - 1, 0
    s1 = np.minimum(s0 + 1, S - 1)
    one = np.float32(1)
    hor = pm[:, s0] * (one - fr)[None, :] + pm[:, s1] * fr[None, :]
    val = hor[s0, :] * (one - fr)[:, None] + hor[s1, :] * fr[:, None]
    assert val.dtype == np.float32
    return mask, ref_box, val


SIZE_FRAME = (200, 320)


def size_boxes():
    """1d: reference boxes on a 200 x 320 frame: 3 x 3, 20 x 50, 150 x 40, 300 x 5 pixels (up- and down-scaling on either axis), a
    tall narrow one and one that sticks out of the frame"""
    return np.array([[50, 60, 52, 62], [100, 20, 119, 69], [30, 100, 179, 139], [10, 150, 309, 154], [200, 5, 204, 194],
                     [250, 120, 400, 260]], np.float32)


def geometry_boxes():
    """the boxes of tests/golden/mask_geometry_sizes.npz: size_boxes() + 40 seeded ones"""
    rs = synth.rng(42, 0)
    return np.vstack([size_boxes(), synth.make_rois(rs, 40, im_h=200, im_w=320, min_side=2, max_side=300)]).astype(np.float32)


def noise_frame():
    """1f: a 61 x 83 frame of noise, rect = the whole frame"""
    return (synth.rng(43, 0).rand(61, 83) < 0.5).astype(np.uint8)


CHECKER_FRAME = (500, 833)
CHECKER_BOX = np.array([100, 50, 700, 450], np.float32)


def checker_mask(M=28):
    return (np.indices((M, M)).sum(0) % 2).astype(np.float32)


def segm_first_guess(im_w):
    """result_utils.segm_results' first runs_stride / str_stride"""
    return 2 * int(im_w) + 8, 4 * int(im_w) + 64


# ---- detection post-processing --------------------------------------------------------------------------------------------------
DET_SF = np.array([1.6, 1.25], np.float32)
DET_IM = np.array([[500.0, 833.0], [640.0, 480.0]], np.float32)
DET_N_ROIS = np.array([300, 173], np.int32)
N_DUP = 12


def det_batch():
    """B = 2, R = 300, 81 classes.  Rows DUP_DST[b] of image b repeat the roi and the deltas of rows DUP_SRC[b] (decoded boxes equal
    bit for bit: IoU = 1 pairs) with every foreground score scaled by 0.97, so a pair's lower-scoring row is always the copy.
    -> (rois5 [B,R,5], cls [B,R,81], deltas [B,R,324], dup_src [B,N_DUP], dup_dst [B,N_DUP])"""
    B, R = 2, 300
    rs = synth.rng(44, 0)
    rois = np.stack([synth.make_rois(rs, R) for _ in range(B)])
    cls, deltas = zip(*[synth.make_head_outputs(rs, R) for _ in range(B)])
    cls, deltas = np.stack(cls).copy(), np.stack(deltas).copy()
    src = np.stack([np.arange(5, 5 + 13 * N_DUP, 13) for _ in range(B)])              # all below n_rois = 173
    dst = src + 6
    for b in range(B):
        rois[b, dst[b]] = rois[b, src[b]]
        deltas[b, dst[b]] = deltas[b, src[b]]
        cls[b, dst[b], 1:] = cls[b, src[b], 1:] * np.float32(0.97)
        cls[b, dst[b], 0] = 1.0 - cls[b, dst[b], 1:].sum(1)
    rois5 = np.concatenate([np.zeros((B, R, 1), np.float32), rois], 2).astype(np.float32)
    return rois5, cls.astype(np.float32), deltas.astype(np.float32), src, dst


def as_logits(cls):
    return np.log(np.maximum(cls, 1e-30)).astype(np.float32)


def signed_score_batch():
    """Decoded-boxes entry with scores of both signs: B = 2, R = 300, 5 classes, scores N(-1.1, 0.5) with exact zeros on rows whose
    boxes are small, disjoint cells (so that tied zeros never meet in the NMS).  -> (scores [B,R,5], boxes [B,R,20], zero rows)"""
    B, R, ncls = 2, 300, 5
    rs = synth.rng(45, 0)
    scores = (rs.standard_normal((B, R, ncls)) * 0.5 - 1.1).astype(np.float32)
    scores = synth.dedupe_scores(scores.reshape(-1)).reshape(B, R, ncls)
    boxes = np.stack([np.hstack([synth.make_rois(rs, R, min_side=30, max_side=200) for _ in range(ncls)]) for _ in range(B)])
    zero_rows = np.arange(7, 7 + 9 * 16, 9)                                           # 16 rows
    for b in range(B):
        for i, r in enumerate(zero_rows):
            for j in range(1, ncls):
                x, y = 1200.0 + 20.0 * i, 900.0 + 20.0 * j                              # outside every other box (make_rois: 1333 x 800)
                boxes[b, r, 4 * j:4 * j + 4] = [x, y, x + 9, y + 9]
            scores[b, r, 1:] = 0.0
    return scores, boxes.astype(np.float32), zero_rows


def overflowing_union_batch():
    """Decoded-boxes entry, 3 classes, R = 40: ordinary boxes, and in each foreground class ONE row (not the best-scoring one) whose
    box is 2e20 wide and high -- its float32 area, and so every union with it, is +inf.  inter / inf = 0 >= thresh holds for
    thresh <= 0 only through the division: inter - thresh * union is NaN at thresh = 0 (0 * inf).
    -> (scores [1, 40, 3], boxes [1, 40, 12], huge rows {class: row})"""
    R, ncls = 40, 3
    rs = synth.rng(51, 0)
    scores = synth.dedupe_scores(rs.uniform(0.1, 0.9, R * ncls).astype(np.float32)).reshape(1, R, ncls)
    boxes = np.hstack([synth.make_rois(rs, R, min_side=30, max_side=300) for _ in range(ncls)])[None].astype(np.float32)
    huge = {1: 5, 2: 9}
    for j, r in huge.items():
        boxes[0, r, 4 * j:4 * j + 4] = [-1e20, -1e20, 1e20, 1e20]
        scores[0, r, j] = 0.5
    return scores, boxes, huge


def check_image(out, b, ref_dets, ref_roi, max_out, sf=None):
    """image b of (dets, det_roi, det_rois_scaled or None, det_count) == the oracle's rows (as tests/test_hip_det_options.py)"""
    dets, det_roi, det_scaled, det_count = out
    D = ref_dets.shape[0]
    assert int(det_count[b]) == D, (b, int(det_count[b]), D)
    n = min(D, max_out)
    got = dets[b, :n].cpu().numpy()
    assert np.array_equal(got, ref_dets[:n]), (b, np.argwhere(got != ref_dets[:n])[:5])
    assert np.array_equal(det_roi[b, :n].cpu().numpy(), ref_roi[:n])
    assert not dets[b, n:].any()
    if det_scaled is not None:
        assert np.array_equal(det_scaled[b, :n].cpu().numpy(), (ref_dets[:n, :4] * np.float32(sf)).astype(np.float32))
