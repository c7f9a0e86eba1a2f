"""The inputs the flip tests share (tests/README_flip.md): built once, never modified by a test."""
import numpy as np

import flip_ref as fr

# ---- boxes: B = 3 images of widths 1, 640 and 1333 -----------------------------------------------------------------------------------------
BOX_WIDTHS = (1, 640, 1333)
BOX_R = 6


def box_rows(w):
    """integer and fractional coordinates, x1 == x2, boxes touching both borders"""
    return np.array([[0, 0, w - 1, 9],                          # touches both borders
                     [0, 2.5, 0, 7.25],                         # x1 == x2 on the left border
                     [w - 1, 1, w - 1, 3],                      # x1 == x2 on the right border
                     [0.3 * w, 4, 0.7 * w, 11.125],             # fractional
                     [17.05 % w, 3.5, (17.05 % w + 333.33) % w if w > 1 else 0.0, 8],
                     [(w - 1) / 3.0, 0.1, (w - 1) / 1.5, 639.49]], np.float32)


def box_case(cols):
    """boxes f32 [3, 6, cols]: the four columns above, tiled with a per-group offset for cols = 8"""
    per = []
    for w in BOX_WIDTHS:
        rows = box_rows(w)
        per.append(np.concatenate([rows + np.float32(0.125 * k) * np.array([1, 0, 1, 0], np.float32) if k else rows
                                   for k in range(cols // 4)], 1))
    return np.ascontiguousarray(np.stack(per), np.float32)


BOX_COUNTS = (0, 2, BOX_R)
BOX_FLAGS = ((1, 1, 1), (1, 0, 1), (0, 0, 0))

# ---- polygons: doubles; the point where a float32 flip of the float32 point differs from the rounding of the double flip ---------
POLY_WIDTHS = (640, 640, 333)
POLYS = [
    [[[639.49, 10.0, 100.1, 20.5, 0.3, 333.33]], [[12.7, 1.0, 17.05, 2.0, 333.33, 3.0, 100.1, 99.9], [0.0, 0.0, 639.0, 0.0, 320.5, 479.0]]],
    [],                                                         # an image without gt
    [[[1.5, 2.5, 300.25, 2.5, 150.0, 200.0]], None, [[332.0, 0.0, 0.0, 0.0, 5.0, 5.0], [10.1, 10.2, 20.3, 10.4, 15.5, 30.6]]],
]
POLY_G, POLY_PTS, POLY_NP = 3, 16, 5                            # PTS and NP leave padding behind every image's own
POLY_FLAGS = ((1, 1, 1), (1, 0, 0), (0, 1, 1))


# ---- run lists ----------------------------------------------------------------------------------------------------------------------------
def _mask(h, w, pixels):
    m = np.zeros((h, w), bool)
    for y, x in pixels:
        m[y, x] = True
    return m


def rle_rows():
    """[(name, h, w, runs or None, n_runs override)]: each a single mask; the expected answers come from flip_ref"""
    checker = np.indices((4, 5)).sum(0) % 2 == 1
    rs = np.random.RandomState(20261020)
    rows = [
        ("1x1 empty", 1, 1, [1]), ("1x1 full", 1, 1, [0, 1]),
        ("1x6 single row", 1, 6, fr.encode(_mask(1, 6, [(0, 0), (0, 3), (0, 4)]))),
        ("6x1 single column", 6, 1, fr.encode(_mask(6, 1, [(1, 0), (2, 0), (5, 0)]))),
        ("3x4 growth", 3, 4, [5, 2, 5]),
        ("full", 5, 7, [0, 35]), ("empty", 5, 7, [35]),
        ("first pixel set", 5, 7, fr.encode(_mask(5, 7, [(0, 0), (4, 6)]))),
        ("4x5 checkerboard", 4, 5, fr.encode(checker)),          # 16 runs: with an even h two equal pixels meet at every column boundary
        ("5x4 checkerboard, h w + 1 runs", 5, 4, fr.encode(np.indices((5, 4)).sum(0) % 2 == 0)),
        ("4x5 stripes, h w + 1 runs", 4, 5, fr.encode(np.indices((4, 5))[0] % 2 == 0)),
        ("7x1333 two pixels", 7, 1333, fr.encode(_mask(7, 1333, [(3, 2), (6, 1200)]))),
        ("interior zero runs", 5, 7, [0, 0, 4, 0, 0, 3, 0, 2, 6, 0, 20, 0]),
        ("leading zeros then ones", 3, 4, [0, 0, 0, 12]),
        ("random 9x13", 9, 13, fr.encode(rs.rand(9, 13) < 0.4)),
        ("random 13x9", 13, 9, fr.encode(rs.rand(13, 9) < 0.6)),
        ("300 runs, more than one chunk", 20, 40, fr.encode(rs.rand(20, 40) < 0.5)),
    ]
    return rows


BLOB_SEED, BLOB_HW = 20261020, (427, 640)


def blob_runs():
    """the 427 x 640 mask of a few random blobs: 889 runs (checked when the case was written: within 65 .. 4096)"""
    return fr.encode(fr.blob_mask(np.random.RandomState(BLOB_SEED), *BLOB_HW))


def pack_runs(lists, stride, n_override=None):
    """[R] lists -> (runs int32 [1, R, stride] holding uint32 bits, n_runs int32 [1, R]); rows shorter than stride are padded with a
    poison value that no kernel may read"""
    R = len(lists)
    runs = np.full((1, R, stride), 0xdeadbeef, np.uint32)
    n = np.zeros((1, R), np.int32)
    for r, row in enumerate(lists):
        runs[0, r, :len(row)] = row
        n[0, r] = len(row)
    if n_override:
        for r, v in n_override.items():
            n[0, r] = v
    return runs.view(np.int32), n
