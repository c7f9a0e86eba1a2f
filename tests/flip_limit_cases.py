"""The four flip entries past where tests/test_hip_flip.py stops (test support, not a test module): the "Limits" section of
tests/README_flip.md lists the cases.  Every builder is seeded, runs once (lru_cache) and returns the INPUTS only, read-only; the run-list
answers that are written out by hand stand beside their inputs.  tests/test_flip_limits_host.py pins on the CPU the condition every
case is named for; tests/test_hip_flip_limits.py launches them.

The kernel arithmetic the conditions speak of (detectorch_amd/csrc/flip/): dtc_flip_rle walks a row's runs in chunks of CHUNK runs
(pass 1) and its pieces -- flip_ref.cut -- in chunks of CHUNK pieces in OUTPUT order (pass 2), carrying the last group start (pass 1)
and the nearest group start behind (pass 2) from chunk to chunk; a group is the pieces of one column, or of a block of whole columns.
A piece is recorded as start << 2 | flags in 32 bits.  The box and polygon kernels run 256 threads per block, one per group of four
box columns / per point.
"""
import functools

import numpy as np

import flip_ref as fr

BASE_SEED = 20261020 + 6000
CHUNK = 256                                                   # csrc/flip/flip_rle.hip: kFlipThreads
POISON = 0xdeadbeef                                           # flip_cases.pack_runs' padding
DENSE_PIXELS = 1 << 22                                        # run lists of images up to this size are also decoded (flip_rle_runs)
U32 = 1 << 32


def _ro(a):
    a.setflags(write=False)
    return a


def pack(images, stride, counts=None, rows=None):
    """images: [((h, w), flag, [run list, ...] or [(run list, n_runs override), ...])] -> dict(runs i32 [N, R, stride] holding uint32
    bits with POISON behind every row's runs, n_runs, im_size f32 [N, 2], flipped, counts or None); an image with fewer than R rows is
    padded with rows of n_runs = 0"""
    N, R = len(images), rows or max(len(im[2]) for im in images)
    runs, n = np.full((N, R, stride), POISON, np.uint32), np.zeros((N, R), np.int32)
    for b, (_, _, lists) in enumerate(images):
        for r, row in enumerate(lists):
            row, override = row if isinstance(row, tuple) else (row, None)
            runs[b, r, :len(row)] = np.asarray(row, np.uint64).astype(np.uint32)
            n[b, r] = len(row) if override is None else override
    return dict(runs=_ro(runs.view(np.int32)), n_runs=_ro(n), im_size=_ro(np.array([im[0] for im in images], np.float32)),
                flipped=tuple(int(im[1]) for im in images), counts=None if counts is None else _ro(np.asarray(counts, np.int32)))


def mask_runs(h, w, pixels):
    m = np.zeros((h, w), bool)
    for y, x in pixels:
        m[y, x] = True
    return fr.encode(m)


# ---- 1. tall_column -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tall_column_rows():
    """[(h, w, runs)]: 600 x 3 with every other pixel of the middle column and one pixel in each outer column; 1100 x 2 with the
    alternating column first, and with it last"""
    a = np.zeros((600, 3), bool)
    a[0::2, 1], a[5, 0], a[7, 2] = True, True, True
    b = np.zeros((1100, 2), bool)
    b[0::2, 0], b[9, 1] = True, True
    c = np.zeros((1100, 2), bool)
    c[1::2, 1], c[9, 0] = True, True
    return ((600, 3, fr.encode(a)), (1100, 2, fr.encode(b)), (1100, 2, fr.encode(c)))


# ---- 2. zero_run_chunk ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zero_run_rows():
    """[(h, w, spliced runs, the runs they were made of)]: a random 9 x 13 mask with 600 zero-length runs behind run 3; a random 20 x 40
    mask (more than 256 runs: the 9 x 13 one has too few to fill chunk 0) with 256 zero-length runs as runs 256 .. 511, chunk 1"""
    rs = np.random.RandomState(BASE_SEED + 2)
    small, large = fr.encode(rs.rand(9, 13) < 0.4), fr.encode(rs.rand(20, 40) < 0.5)
    return ((9, 13, small[:4] + [0] * 600 + small[4:], small), (20, 40, large[:CHUNK] + [0] * CHUNK + large[CHUNK:], large))


# ---- 3. growth ------------------------------------------------------------------------------------------------------------------------------
GROWTH_ROWS = ((5, 720, [3] + [12] * 299 + [9]), (7, 1000, [3] + [23] * 304 + [5]))
GROWTH_STRIDES = (512, 1024)                                  # runs_stride, out_stride: the output chunks outnumber the input chunks


# ---- 4. chunk_edges -------------------------------------------------------------------------------------------------------------------------
def _three_rows(n):
    """n runs of 2 pixels (the last one longer) in a 3-row image: most runs cross a column boundary"""
    w = (2 * n + 2) // 3 + 1
    return (3, w, [2] * (n - 1) + [3 * w - 2 * (n - 1)])


EDGE_COUNTS = (255, 256, 257, 512, 513)
EDGE_ROWS = (tuple((1, n, [1] * n) for n in EDGE_COUNTS) + tuple(_three_rows(n) for n in EDGE_COUNTS) +
             ((3, 128, [2] * 192), (3, 256, [2] * 384)))      # the last two: exactly 256 and 512 pieces (4 pieces to 3 runs)
EDGE_PIECES = (256, 512)


# ---- 5. pixels_2_30: the answers are written out by hand ----------------------------------------------------------------------------------
S = 32768
P30 = S * S
PIXELS_2_30 = (
    ("pixel at row 5, column 0", [5, 1, P30 - 6], [32767 * 32768 + 5, 1, 32762]),
    ("pixel at row 32767, column 32767", [P30 - 1, 1], [32767, 1, P30 - 32768]),
    ("pixel at row 0, column 32767: a leading zero run", [32767 * 32768, 1, 32767], [0, 1, P30 - 1]),
    ("columns 1 .. 3 and rows 10 .. 19 of column 4", [32768, 3 * 32768, 10, 10, P30 - 4 * 32768 - 20],
     [32763 * 32768 + 10, 10, 32748, 3 * 32768, 32768]),
    ("empty", [P30], [P30]),
    ("full", [0, P30], [0, P30]),
)

# ---- 6. too_many_pixels / 7. im_sizes / 8. wrapped_sum --------------------------------------------------------------------------------------
# (im_size, [run lists]): the sums are the clipped product of the sides (2^30) and the true one
TOO_MANY = (((65536, 32768), [[P30], [1 << 31], [0, P30]]),
            ((3e9, 1.5), [[P30], [3000000000], [5, P30 - 5]]),      # the sides are 2^30 and 1: 2^30 pixels, NOT too many
            ((32768, 32769), [[P30], [P30 + 32768], [P30 + 32767, 1]]))

IM_SIZE_ROWS = (((7.9, 5.2), [mask_runs(7, 5, [(0, 0), (3, 1), (6, 4)]), [35], [36]]),
                ((0.5, 9), [[0], [5], [0, 0]]),
                ((np.nan, 9), [[0], [5], [0, 0]]),
                ((1, 1), [[1], [0, 1], [2]]))

WRAPPED_HW = (5, 7)
WRAPPED_ROWS = ([U32 - 1, 36], [4, U32 - 4, 35], [U32 - 1] * 300, [10, 5, 20])      # the last one is sound


# ---- 9. counts ------------------------------------------------------------------------------------------------------------------------------
COUNTS = (-3, 0, 2, 5, 9)
COUNTS_FLAGS = (1, 0, 1, 0, 1)


@functools.lru_cache(maxsize=None)
def counts_case():
    """R = 5 rows in each of five 6 x 8 images, counts (-3, 0, 2, 5, 9), flags mixed"""
    rs = np.random.RandomState(BASE_SEED + 9)
    return pack([((6, 8), f, [fr.encode(rs.rand(6, 8) < 0.5) for _ in range(5)]) for f in COUNTS_FLAGS], 64, counts=COUNTS)


# ---- the batches of dtc_flip_rle: name -> (inputs of pack(), [out_stride, ...]) ---------------------------------------------------------------
def _single(rows, stride, flag=1):
    return pack([((h, w), flag, [runs]) for h, w, runs in rows], stride)


@functools.lru_cache(maxsize=None)
def rle_batches():
    growth = _single(GROWTH_ROWS, GROWTH_STRIDES[0])
    need = [len(fr.flip_rle_sparse(r, h, w)) for h, w, r in GROWTH_ROWS]
    return {
        "tall_column": (_single(tall_column_rows(), 1200), [1200]),
        "zero_run_chunk": (_single([z[:3] for z in zero_run_rows()], 1024), [1024]),
        "growth": (growth, [GROWTH_STRIDES[1]] + [v - d for v in need for d in (0, 1)]),
        "chunk_edges": (_single(EDGE_ROWS, 520), [1100]),
        "pixels_2_30": (pack([((S, S), 1, [p[1] for p in PIXELS_2_30]), ((S, S), 0, [p[1] for p in PIXELS_2_30])], 8), [8]),
        "too_many_pixels": (pack([(size, 1, lists) for size, lists in TOO_MANY], 4), [4]),
        "im_sizes": (pack([(size, 1, lists) for size, lists in IM_SIZE_ROWS], 12), [12]),
        "wrapped_sum": (pack([(WRAPPED_HW, 1, list(WRAPPED_ROWS)), (WRAPPED_HW, 0, list(WRAPPED_ROWS))], 300), [300]),
        "counts": (counts_case(), [64]),
    }


@functools.lru_cache(maxsize=None)
def rle_expected(name, out_stride):
    """flip_ref.flip_rle_batched on the batch: by decoding where every image has at most DENSE_PIXELS, else by the sparse form"""
    b = rle_batches()[name][0]
    dense = max(fr.side(h) * fr.side(w) for h, w in b["im_size"]) <= DENSE_PIXELS
    return fr.flip_rle_batched(b["runs"], b["n_runs"], b["im_size"], b["flipped"], out_stride, b["counts"], flip=None if dense else fr.flip_rle_sparse)


# ---- boxes ----------------------------------------------------------------------------------------------------------------------------------
NAN_PAYLOAD = 0x7fc12345                                      # a quiet NaN with a payload; 0xffc00001: a negative one
BOX_SPECIALS = np.array([NAN_PAYLOAD, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00000000], np.uint32).view(np.float32)
# (shape, im_width, [(flags, counts)])
BOX_CASES = (((2, 300, 12), (2 ** 24 + 1, 640), [((1, 1), None), ((1, 1), (-1, 301)), ((0, 1), (150, 300)), ((1, 0), (299, 1))]),
             ((1, 1, 4096), (0,), [((1,), None), ((1,), (0,)), ((0,), (1,))]),
             ((2, 70000, 4), (1, 1333), [((1, 1), (70001, 65536)), ((1, 0), None)]))


@functools.lru_cache(maxsize=None)
def boxes(k):
    """seeded coordinates, and in every seventh box a special value in one of its four places: x and y alike"""
    shape = BOX_CASES[k][0]
    rs = np.random.RandomState(BASE_SEED + 20 + k)
    b = rs.uniform(-50, 1400, shape).astype(np.float32)
    flat = b.reshape(-1, 4)
    rows = np.arange(0, len(flat), 7)
    flat[rows, rows // 7 % 4] = BOX_SPECIALS[rows // 28 % len(BOX_SPECIALS)]
    return _ro(b)


# ---- polygons -------------------------------------------------------------------------------------------------------------------------------
POLY_PTS, POLY_NP, POLY_WIDTHS = 1000, 7, (640, 640, 333)
POLY_X_AT = (255, 256, 999)                                   # 639.49 at w = 640: float32(w - x - 1) is not the float32 flip
# (poly_ptr[b][NP] per image, flags)
POLY_CALLS = (((1000, 257, -5), (1, 1, 1)), ((2000, 1000, 257), (1, 0, 1)), ((256, 2 ** 31 - 1, -2 ** 31), (1, 1, 1)))


@functools.lru_cache(maxsize=None)
def polygon_points():
    """poly_xy f64 [3, 1000, 2]: seeded doubles, every point in use (no zero padding: what lies behind the last offset is data too)"""
    rs = np.random.RandomState(BASE_SEED + 30)
    xy = rs.uniform(0, 1, (3, POLY_PTS, 2)) * np.array([[[w, 480.0]] for w in POLY_WIDTHS])
    xy[:2, POLY_X_AT, 0] = 639.49
    return _ro(xy)


def polygon_ptr(last):
    """poly_ptr i32 [3, NP + 1]: the offsets in front of the last one are not read by the flip"""
    ptr = np.tile(np.array([0, 3, 6, 9, 12, 15, 18, 0], np.int32), (3, 1))
    ptr[:, POLY_NP] = last
    return ptr


def polygons_expected(xy, last, flags):
    """flip_ref.flip_poly on the points below the clamped last offset of a flipped image, a copy behind it -> (f64, its f32 cast)"""
    out = np.array(xy, np.float64)
    for b, (n, f, w) in enumerate(zip(last, flags, POLY_WIDTHS)):
        n = min(max(int(n), 0), POLY_PTS)
        if f and n:
            out[b, :n] = np.asarray(fr.flip_poly(xy[b, :n].reshape(-1).tolist(), w), np.float64).reshape(n, 2)
    return out, out.astype(np.float32)


# ---- prep -----------------------------------------------------------------------------------------------------------------------------------
PREP_HW = (40, 301)
PREP_TARGETS = ((40, 400), (20, 400), (80, 700))              # scale 1; downscale; upscale: blob widths 301, 151 (320 padded), 602


@functools.lru_cache(maxsize=None)
def prep_images():
    rs = np.random.RandomState(BASE_SEED + 40)
    return (_ro(rs.randint(0, 256, PREP_HW + (3,)).astype(np.uint8)), _ro(rs.uniform(0, 255, PREP_HW + (3,)).astype(np.float32)))
