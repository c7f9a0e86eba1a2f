"""Numpy restatements of the reference's horizontal flip, the yardsticks of tests/test_flip_host.py and tests/test_hip_flip.py
(tests/README_flip.md).  Each cites the reference lines it restates; none imports the package under test.

    flip_boxes       lib/utils/boxes.py:264-269, lib/data/roidb.py:112-117            float32
    flip_poly        lib/utils/segms.py:37-40                                          float64
    flip_rle_runs    lib/utils/segms.py:42-50 (decode, mask[:, ::-1], encode)          written from COCO's format definition
    flip_rle_sparse  the same on intervals, no bitmap (images of up to 2^30 pixels)    held to flip_rle_runs by tests/test_flip_limits_host.py
    flip_image       lib/data/coco_dataset.py:51-53                                    image[:, ::-1, :]

pycocotools is not installed where this is tested: the run-list coding is written from the format definition (column-major, runs
alternate zeros and ones and start with zeros), and parity with the package itself is unpinned, as everywhere else in this project."""
import numpy as np


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------------
def flip_boxes(boxes, im_width):
    """boxes.py:264-269: float32 boxes [n, 4k] against a Python-int width: numpy keeps float32, and evaluates (w - x2) - 1"""
    boxes = np.asarray(boxes, np.float32)
    out = boxes.copy()
    out[:, 0::4] = int(im_width) - boxes[:, 2::4] - 1
    out[:, 2::4] = int(im_width) - boxes[:, 0::4] - 1
    return out


def flip_boxes_batched(boxes, im_width, flipped, counts=None):
    """the batched form of the kernel: boxes f32 [B, R, cols]; rows past counts[b] and images with flipped[b] == 0 are copied"""
    boxes = np.asarray(boxes, np.float32)
    out = boxes.copy()
    for b in range(boxes.shape[0]):
        n = boxes.shape[1] if counts is None else min(max(int(counts[b]), 0), boxes.shape[1])
        if flipped[b]:
            out[b, :n] = flip_boxes(boxes[b, :n], int(im_width[b]))
    return out


# ---- polygons ---------------------------------------------------------------------------------------------------------------------------------
def flip_poly(poly, width):
    """segms.py:37-40: np.array(poly) is float64; x' = width - x - 1"""
    out = np.array(poly, np.float64)
    out[0::2] = width - np.array(poly, np.float64)[0::2] - 1
    return out.tolist()


def flip_polys_per_image(polys_per_image, widths, flipped):
    """lists as pack_polygons / pack_polygons64 take them: per image, per gt row, a list of polygons (or None)"""
    return [[([flip_poly(p, int(w)) for p in gt] if f else [list(p) for p in gt]) if isinstance(gt, (list, tuple)) else gt for gt in im]
            for im, w, f in zip(polys_per_image, widths, flipped)]


# ---- run lists --------------------------------------------------------------------------------------------------------------------------------
def decode(runs, h, w):
    """uncompressed COCO RLE -> bool [h, w]; the runs must sum to h w (zero-length runs anywhere are fine)"""
    runs = np.asarray(runs, np.int64)
    assert runs.sum() == h * w, (runs.sum(), h, w)
    flat = np.repeat(np.arange(len(runs)) & 1, runs).astype(bool)
    return flat.reshape(w, h).T                                # column-major: position x * h + y


def encode(mask):
    """bool [h, w] -> the canonical run list: the first run counts zeros and may be 0, no other run is 0"""
    flat = np.asarray(mask, bool).T.reshape(-1)
    if flat.size == 0:
        return [0]
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    runs = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return ([0] if flat[0] else []) + runs


def flip_rle_runs(runs, h, w):
    """segms.py:42-50: decode, mask[:, ::-1], encode"""
    return encode(decode(runs, h, w)[:, ::-1])


def cut(runs, h, w):
    """the runs cut at the column boundaries -> [(value, start, end)] in input order: of every run of at least one pixel its head (up
    to the end of its first column), the whole columns in its middle as ONE piece, and its tail; a piece starts at a multiple of h or
    is the head of a run that starts inside a column"""
    out, s = [], 0
    for k, n in enumerate(int(v) for v in runs):
        e = s + n
        if n > 0:
            c0, c1 = s // h, (e - 1) // h
            out.append((k & 1, s, min(e, (c0 + 1) * h)))
            if c1 > c0 + 1:
                out.append((k & 1, (c0 + 1) * h, c1 * h))
            if c1 > c0:
                out.append((k & 1, c1 * h, e))
        s = e
    return out


def flip_rle_sparse(runs, h, w):
    """flip_rle_runs without a bitmap: the pieces of the one-runs, [c h + y0, c h + y1) -> [(w - 1 - c) h + y0, (w - 1 - c) h + y1)
    (the whole columns c0 .. c1 - 1 of a piece to w - c1 .. w - 1 - c0), sorted, touching pieces merged, canonical runs out"""
    hw = h * w
    assert sum(int(v) for v in runs) == hw, (sum(int(v) for v in runs), h, w)
    if hw == 0:
        return [0]
    mapped = []
    for v, s, e in cut(runs, h, w):
        if v:
            c0, c1 = s // h, (e - 1) // h                      # c1 > c0: whole columns only
            mapped.append(((w - 1 - c1) * h + s - c0 * h, (w - 1 - c1) * h + e - c0 * h))
    merged = []
    for a, b in sorted(mapped):
        if merged and a == merged[-1][1]:
            merged[-1][1] = b
        else:
            merged.append([a, b])
    bounds = [x for ab in merged for x in ab]
    if bounds and bounds[-1] == hw:
        bounds.pop()
    edges = [0] + bounds + [hw]
    return [q - p for p, q in zip(edges[:-1], edges[1:])]


def side(v):
    """one side of im_size as the kernels read it: truncated; below 1, NaN: 0; above 2^30: 2^30"""
    v = np.float32(v)
    if not v >= 1:
        return 0
    return 1 << 30 if v >= np.float32(1 << 30) else int(v)


def flip_rle_batched(runs, n_runs, im_size, flipped, out_stride, counts=None, flip=None):
    """the batched entry: runs uint32-valued [N, R, S], n_runs [N, R] -> (lists per row or None where nothing is written, out_n_runs
    [N, R], need [N, R]); rows past counts are None / left 0 in the arrays; `flip`: flip_rle_runs (the default) or flip_rle_sparse"""
    flip = flip or flip_rle_runs
    N, R, S = np.asarray(runs).shape
    runs = np.asarray(runs).astype(np.int64) & 0xffffffff
    lists = [[None] * R for _ in range(N)]
    out_n, need = np.zeros((N, R), np.int32), np.zeros((N, R), np.int32)
    for n in range(N):
        cnt = R if counts is None else min(max(int(counts[n]), 0), R)
        h, w = side(im_size[n][0]), side(im_size[n][1])
        for r in range(cnt):
            m = int(n_runs[n][r])
            if m < 0 or m > S:
                out_n[n, r], need[n, r] = -1, 0
                continue
            row = runs[n, r, :m].tolist()
            if not flipped[n]:
                res = row
            elif m == 0:
                res = []
            elif h * w > 1 << 30 or sum(row) != h * w:
                out_n[n, r], need[n, r] = -1, 0
                continue
            else:
                res = flip(row, h, w)
            need[n, r] = len(res)
            if len(res) <= out_stride:
                out_n[n, r], lists[n][r] = len(res), res
            else:
                out_n[n, r] = -1
    return lists, out_n, need


# ---- the image --------------------------------------------------------------------------------------------------------------------------------
def flip_image(image):
    """coco_dataset.py:51-53"""
    return np.ascontiguousarray(np.asarray(image)[:, ::-1, :])


def blob_mask(rs, h, w, blobs=4):
    """a mask of a few random discs and boxes: the 427 x 640 case of the tests"""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(blobs):
        cy, cx, ry, rx = rs.randint(0, h), rs.randint(0, w), rs.randint(8, h // 4), rs.randint(8, w // 4)
        if rs.randint(2):
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        else:
            m |= (abs(yy - cy) <= ry) & (abs(xx - cx) <= rx)
    return m
