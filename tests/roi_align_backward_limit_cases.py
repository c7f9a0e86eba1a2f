"""dtc_roi_align_backward off its default point (test support, not a test module): the cases that
tests/golden/make_roi_align_backward_limits_golden.py runs through the reference's own loop (tests/golden/roi_align_backward_limits.npz),
that tests/test_roi_align_backward_limits_host.py pins on the CPU and that tests/test_hip_roi_align_backward_limits.py launches.

A CASE is a dict like roi_align_backward_ref._case's (top, rois, batch, shapes, scales, ratio, levels), made by case(name), cached and
never modified; "bad_rows" lists the rows that include/detectorch_grad_hip.h calls bad.  restatement(name) is
roi_align_backward_ref.reference on it, computed once per process.  tests/README_roi_align_backward.md says what each group is
there for.  Every case uses the smallest maps and channel counts that still reach its branch.
"""
import functools

import numpy as np

import roi_align_backward_ref as rb

F = np.float32
A29 = float(2 ** 29 - 32)                            # the largest float32 below the 2^29 limit of a scaled coordinate
SAMPLED_CHANNELS = 4


def _case(top, rois, batch, shapes, scales, ratio, levels=None, bad_rows=()):
    c = rb._case(top, rois, batch, shapes, scales, ratio, levels)
    c["bad_rows"] = sorted(bad_rows)
    return c


def _grid_rois(rs, pairs, pooled, h, w, image=None):
    """one box per (gh, gw) of pairs whose adaptive grid at scale 1 is that pair: a side of pooled * (g - 0.5) map pixels"""
    rois = []
    for k, (gh, gw) in enumerate(pairs):
        bh, bw = pooled[0] * (gh - 0.5), pooled[1] * (gw - 0.5)
        x1, y1 = rs.uniform(min(w - bw, 0) - 1, max(w - bw, 0) + 1), rs.uniform(min(h - bh, 0) - 1, max(h - bh, 0) + 1)
        rois.append([k % 2 if image is None else image, x1, y1, x1 + bw, y1 + bh])
    return np.array(rois, F)


# ---- pooled: PH != PW ------------------------------------------------------------------------------------------------------------
POOLED = [(1, 1), (1, 7), (7, 1), (3, 5), (5, 3), (2, 14), (14, 7)]
POOLED_ADAPTIVE = {(3, 5): [(1, 2), (2, 1), (3, 1), (1, 3), (2, 3), (4, 2)] * 2, (14, 7): [(1, 2), (1, 3), (2, 1), (2, 3), (1, 2), (2, 1)] * 2}


def _pooled(ph, pw, ratio):
    rs = rb._rs(12, 1, ph, pw, ratio)
    if ratio == 0:
        rois = _grid_rois(rs, POOLED_ADAPTIVE[(ph, pw)], (ph, pw), 13, 17)
        rois[:, 1:] *= F(4)                          # sides and corners are multiples of 2^-k after rounding: * 4 / 4 is exact
    else:
        rois = rb._rois(rs, 12, 2, 13, 17, 0.25)
    return _case(rb._top(rs, 12, 3, ph, pw), rois, 2, [(13, 17)], [0.25], ratio)


# ---- ratio -----------------------------------------------------------------------------------------------------------------------
RATIOS = (1, 3, 4, 5, 7, 8, 0, -1, -3)


def _ratio(ratio):
    rs = rb._rs(12, 2)                               # the same inputs for every ratio: -1 and -3 are ratio 0
    return _case(rb._top(rs, 8, 2, 3, 3), rb._rois(rs, 8, 2, 13, 17, 0.25), 2, [(13, 17)], [0.25], ratio)


def _ratio_64():                                     # 4096 samples of ONE RoI two pixels wide, summed into at most 9 pixels
    return _case(rb._top(rb._rs(12, 3), 1, 2, 1, 1), [[0, 3.0, 2.0, 5.0, 4.0]], 1, [(5, 7)], [1.0], 64)


def _ratio_1024():                                   # DTC_GRAD_MAX_SAMPLING: a 160 x 160 box, samples 5 / 32 apart
    return _case(rb._top(rb._rs(12, 4), 1, 2, 1, 1), [[0, -76.5, -78.25, 83.5, 81.75]], 1, [(5, 7)], [1.0], 1024)


# ---- grid: adaptive grids up to DTC_GRAD_MAX_GRID and one float32 step past it -----------------------------------------------------
GRIDS = [(6, 7), (9, 5), (16, 16), (31, 33)]
G = 32768.0
G1 = float(np.nextafter(F(G), F(np.inf)))            # 32768 + 2^-8: the adaptive grid is 32769


def _grid_small():
    rs = rb._rs(12, 5)
    return _case(rb._top(rs, len(GRIDS), 2, 2, 2), _grid_rois(rs, GRIDS, (2, 2), 13, 17, image=0), 1, [(13, 17)], [1.0], 0)


def _grid_limit(which):
    """1 x 1 bins on a 5 x 7 map at scale 1; the long side runs from -16382 to 16386 (samples 1 apart, six of them on the map) or,
    one float32 step longer, from 0 to 32768 + 2^-8"""
    rs = rb._rs(12, 6)
    y, x = (-16382.0, 16386.0), (-16381.0, 16387.0)
    long_ = {"32768_y": [0, 1.0, y[0], 4.5, y[1]], "32768_x": [0, x[0], 1.0, x[1], 3.5], "32768_yx": [0, x[0], y[0], x[1], y[1]],
             "32769_y": [0, 1.0, 0.0, 4.5, G1], "32769_x": [0, 0.0, 1.0, G1, 3.5]}[which]
    rois = [[0, 0.5, 0.25, 5.0, 3.75], long_, [0, 2.0, 1.0, 6.5, 4.5]]
    return _case(rb._top(rs, 3, 1, 1, 1), rois, 1, [(5, 7)], [1.0], 0, bad_rows=[1] if which.startswith("32769") else [])


# ---- huge: RoIs far larger than the map, far corners, tile corners, the 2^29 limit, coinciding positions ----------------------------
HUGE_MAP = (9, 33)                                   # 3 x 3 tiles
TILE_CORNERS = [(3.0, 15.0), (3.0, 31.0), (7.0, 15.0), (7.0, 31.0)]     # (y, x): the pixel above and left of an interior tile corner


def _huge_rois(adaptive):
    h, w = HUGE_MAP
    rois = []
    for k in (2, 10, 100) if adaptive else (2, 10, 100, 10000):
        for dy, dx in ((0.0, 0.0), (-0.21, 0.37)):   # centred on the map, and off-centre by a fraction of the RoI
            cy, cx = (h - 1) / 2.0 + dy * k * h, (w - 1) / 2.0 + dx * k * w
            rois.append([0, cx - k * w / 2.0, cy - k * h / 2.0, cx + k * w / 2.0, cy + k * h / 2.0])
    if not adaptive:                                 # one corner inside the map, the opposite one 1e6 away
        rois += [[0, 5.0, 3.0, 1e6, 1e6], [0, -1e6, -1e6, 20.0, 6.0], [0, 5.0, -1e6, 1e6, 6.0], [0, -1e6, 2.5, 28.25, 1e6]]
    rois += [[0, x, y, x, y] for y, x in TILE_CORNERS]   # forced 1 x 1: every sample has its four taps in four tiles
    return np.array(rois, F)


def _huge(ph, pw, ratio):
    rois = _huge_rois(ratio <= 0)
    return _case(rb._top(rb._rs(12, 7, ph, pw), len(rois), 2, ph, pw), rois, 1, [HUGE_MAP], [1.0], ratio)


# x2 and y2 were searched, one float32 step at a time, for a sample that lands on the map (tests/README_roi_align_backward.md);
# the host module asserts that one does
ROI_2P29_X = [0, -A29, 1.0, 19884032.0, 7.0]         # 7 x 7 bins, ratio 2: the 14th sample column lies on the map
ROI_2P29_Y = [0, 2.0, -A29, 30.0, 48806400.0]        # 3 x 5 bins, ratio 2: the 6th sample row lies on the map


def _huge_limit(ph, pw):
    """two levels on the same 9 x 33 map, scales 1 and 0.25: scaled coordinates of 2^29 - 32 (valid) and of 2^29 (bad)"""
    rs = rb._rs(12, 8, ph, pw)
    rois = [[0, 3.0, 1.0, 25.0, 7.5], ROI_2P29_X, ROI_2P29_Y, [0, -A29, -A29, A29, A29],
            [0, 1.0, 1.0, 2.0 ** 29, 5.0], [0, -2.0 ** 29, 1.0, 8.0, 5.0], [0, 1.0, 1.0, 5.0, -2.0 ** 29],    # bad: 2^29 at scale 1
            [0, 12.0, 4.0, 100.0, 30.0], [0, 4.0, 4.0, 2.0 ** 31, 20.0], [0, 4.0, -2.0 ** 31, 40.0, 20.0],    # bad: 2^31 at scale 0.25
            [0, -4 * A29, 4.0, 4 * A29, 20.0]]                                                                  # 2^29 - 32 at scale 0.25
    levels = [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1]
    return _case(rb._top(rs, len(rois), 2, ph, pw), rois, 1, [HUGE_MAP, HUGE_MAP], [1.0, 0.25], 2, levels, bad_rows=[4, 5, 6, 8, 9])


def _huge_coincide():
    """x = 40000.3 on a 1 x 65536 map, pooled_w 1024, width forced to 1: bin_w = 2^-10 is a quarter of the float32 spacing (2^-8) of
    the positions, so neighbouring samples coincide"""
    rs = rb._rs(12, 9)
    return _case(rb._top(rs, 1, 1, 1, 1024), [[0, 40000.3, 0.0, 40000.3, 0.0]], 1, [(1, 65536)], [1.0], 2)


# ---- scale -----------------------------------------------------------------------------------------------------------------------
def _scale(which):
    rs = rb._rs(12, 10)
    s = {"third": 1.0 / 3.0, "2": 2.0, "0": 0.0, "neg": -0.25}[which]
    rois = rb._rois(rs, 8, 2, 13, 17, abs(s) if s else 0.25)
    if s < 0:
        rois[:6, 1:] *= F(-1)                        # negative coordinates at a negative scale: the boxes of scale 0.25; two stay off the map
    return _case(rb._top(rs, 8, 2, 7, 7), rois, 2, [(13, 17)], [s], 2)


# ---- groups: the preparation kernel's compaction -----------------------------------------------------------------------------------
GROUP_SHAPES, GROUP_SCALES = [(16, 20), (8, 10), (4, 5)], [0.25, 0.125, 0.0625]
BAD_AT = (0, 254, 255, 256, 257, 511, 512)           # chunk borders of the 256-wide compaction, and the last row


def _plant(rois, levels, rows, n_levels, batch):
    """one bad row of each kind, in turn, at `rows`"""
    kinds = [(0, -1.0), (2, np.nan), ("level", n_levels), (3, np.inf), ("level", -1), (0, float(batch)), (4, -np.inf), (0, np.nan)]
    for k, r in enumerate(rows):
        col, v = kinds[k % len(kinds)]
        if col == "level":
            levels[r] = v
        else:
            rois[r, col] = v
    return sorted(rows)


def _interleaved(rs, n, shapes, scales, batch):
    levels = (np.arange(n) % len(shapes)).astype(np.int32)
    per = [rb._rois(rs, n, batch, h, w, s, lo=1.5) for (h, w), s in zip(shapes, scales)]
    rois = np.stack([per[l][r] for r, l in enumerate(levels)])
    rois[:, 0] = (np.arange(n) // len(shapes)) % batch
    return rois, levels


def _groups(n):
    rs = rb._rs(12, 11, n)
    rois, levels = _interleaved(rs, n, GROUP_SHAPES, GROUP_SCALES, 2)
    bad = _plant(rois, levels, sorted({r for r in BAD_AT if r < n} | {n - 1}), 3, 2)
    return _case(rb._top(rs, n, 2, 2, 2), rois, 2, GROUP_SHAPES, GROUP_SCALES, 2, levels, bad)


def _groups_one():                                   # all 513 RoIs in ONE group (level 1, image 1), the other five empty
    rs = rb._rs(12, 12)
    rois = rb._rois(rs, 513, 2, 8, 10, 0.125, lo=1.5)
    rois[:, 0] = 1
    levels = np.ones(513, np.int32)
    bad = _plant(rois, levels, [256], 3, 2)
    return _case(rb._top(rs, 513, 2, 2, 2), rois, 2, GROUP_SHAPES, GROUP_SCALES, 2, levels, bad)


SHAPES_8 = [(16, 20), (8, 10), (4, 5), (1, 1), (2, 3), (1, 17), (1, 1), (3, 2)]
SCALES_8 = [0.25, 0.125, 0.0625, 0.015625, 0.03125, 0.25, 0.0078125, 0.03125]


def _groups_8x3():                                   # DTC_MAX_LEVELS levels x 3 images, 40 RoIs: every one of the 24 groups has one
    rs = rb._rs(12, 13)
    rois, levels = _interleaved(rs, 40, SHAPES_8, SCALES_8, 3)
    return _case(rb._top(rs, 40, 2, 2, 2), rois, 3, SHAPES_8, SCALES_8, 2, levels)


def _groups_null():                                  # roi_levels NULL with two levels: everything on level 0, level 1 all +0.0
    rs = rb._rs(12, 14)
    return _case(rb._top(rs, 20, 2, 2, 2), rb._rois(rs, 20, 2, 16, 20, 0.25), 2, GROUP_SHAPES[:2], GROUP_SCALES[:2], 2)


# ---- batch_index -------------------------------------------------------------------------------------------------------------------
BATCH_INDICES = [(-0.5, 0), (-0.999, 0), (0.0, 0), (0.9, 0), (1.0, 1), (1.5, 1), (1.999, 1), (-1.0, None), (2.0, None)]


def _batch_index():
    rs = rb._rs(12, 15)
    rois = rb._rois(rs, len(BATCH_INDICES), 2, 13, 17, 0.25)
    rois[:, 0] = [v for v, _ in BATCH_INDICES]
    return _case(rb._top(rs, len(rois), 2, 2, 2), rois, 2, [(13, 17)], [0.25], 2, bad_rows=[7, 8])


# ---- nonfinite_top -----------------------------------------------------------------------------------------------------------------
def _nonfinite_top():
    """box (0, 0, 4, 4), 2 x 2 bins, ratio 1: the samples are the pixel centres (1, 1), (1, 3), (3, 1), (3, 3), so three taps of
    each have weight 0.  Image 0: +inf, -inf, NaN and 1.5; image 1: -0.0, -tiny, 1.0 and -0.0.  Channel 1 is finite."""
    tiny = np.finfo(F).tiny
    top = np.zeros((2, 2, 2, 2), F)
    top[0, 0] = [[np.inf, -np.inf], [np.nan, 1.5]]
    top[1, 0] = [[-0.0, -tiny], [1.0, -0.0]]
    top[:, 1] = rb._top(rb._rs(12, 16), 2, 1, 2, 2)[:, 0]
    return _case(top, [[0, 0.0, 0.0, 4.0, 4.0], [1, 0.0, 0.0, 4.0, 4.0]], 2, [(5, 7)], [1.0], 1)


# ---- channels: blockIdx.y >= 2 -----------------------------------------------------------------------------------------------------
CHANNELS = (511, 512, 513, 769)
CHANNEL_MAPS = ((4, 16), (5, 17))


def _channels(ch, h, w):
    rs = rb._rs(12, 17, ch, h, w)
    return _case(rb._top(rs, 1, ch, 3, 3), [[0, 1.25, 0.5, w - 2.5, h - 0.75]], 1, [(h, w)], [1.0], 2)


def sample_channels(name, channels):
    """the channels of a `channels` case that the fixture holds: the first, the last and seeded ones between"""
    if not name.startswith("channels_"):
        return np.arange(channels)
    rs = rb._rs(12, 99, channels)
    return np.unique(np.concatenate([[0, channels - 1], rs.choice(np.arange(1, channels - 1), SAMPLED_CHANNELS - 2, replace=False)]))


# ---- extents -----------------------------------------------------------------------------------------------------------------------
EXTENTS = ((257, 1), (1, 1024), (1, 1025))


def _extent_rois(rs, h, w):
    rois = rb._rois(rs, 6, 1, h, w, 1.0, lo=1.0, hi=max(h, w) * 0.6)
    rois[2, 1:] = [0.0, 0.0, 2.0, 2.0]               # the first tile and the last
    rois[3, 1:] = [w - 2.5, h - 2.5, w - 0.5, h - 0.5]
    rois[4, 1:] = [-3.0, -3.0, w + 4.5, h + 4.5]     # longer than the map, both ways
    rois[5, 1:] = [0.25, 0.25, 2.0 * w, 2.0 * h]
    return rois


def _extents(h, w):
    rs = rb._rs(12, 18, h, w)
    return _case(rb._top(rs, 6, 1, 3, 3), _extent_rois(rs, h, w), 1, [(h, w)], [1.0], 2)


def _extents_two():
    rs = rb._rs(12, 19)
    rois = np.vstack([_extent_rois(rs, 257, 1), _extent_rois(rs, 3, 5)])
    return _case(rb._top(rs, 12, 1, 3, 3), rois, 1, [(257, 1), (3, 5)], [1.0, 1.0], 2, [0] * 6 + [1] * 6)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
BUILDERS = {}
for _ph, _pw in POOLED:
    BUILDERS["pooled_%dx%d" % (_ph, _pw)] = functools.partial(_pooled, _ph, _pw, 2)
for _ph, _pw in POOLED_ADAPTIVE:
    BUILDERS["pooled_%dx%d_adaptive" % (_ph, _pw)] = functools.partial(_pooled, _ph, _pw, 0)
for _r in RATIOS:
    BUILDERS["ratio_%d" % _r] = functools.partial(_ratio, _r)
BUILDERS["ratio_64_one_roi"] = _ratio_64
BUILDERS["ratio_1024"] = _ratio_1024
BUILDERS["grid_small"] = _grid_small
GRID_LIMIT = ("32768_y", "32768_x", "32768_yx", "32769_y", "32769_x")
for _w in GRID_LIMIT:
    BUILDERS["grid_" + _w] = functools.partial(_grid_limit, _w)
BUILDERS["huge_7x7"] = functools.partial(_huge, 7, 7, 2)
BUILDERS["huge_3x5"] = functools.partial(_huge, 3, 5, 2)
BUILDERS["huge_3x5_adaptive"] = functools.partial(_huge, 3, 5, 0)
BUILDERS["huge_limit_7x7"] = functools.partial(_huge_limit, 7, 7)
BUILDERS["huge_limit_3x5"] = functools.partial(_huge_limit, 3, 5)
BUILDERS["huge_coincide"] = _huge_coincide
for _w in ("third", "2", "0", "neg"):
    BUILDERS["scale_" + _w] = functools.partial(_scale, _w)
GROUP_SIZES = (255, 256, 257, 513)
for _n in GROUP_SIZES:
    BUILDERS["groups_%d" % _n] = functools.partial(_groups, _n)
BUILDERS["groups_one"] = _groups_one
BUILDERS["groups_8x3"] = _groups_8x3
BUILDERS["groups_null"] = _groups_null
BUILDERS["batch_index"] = _batch_index
BUILDERS["nonfinite_top"] = _nonfinite_top
for _c in CHANNELS:
    for _h, _w in CHANNEL_MAPS:
        BUILDERS["channels_%d_%dx%d" % (_c, _h, _w)] = functools.partial(_channels, _c, _h, _w)
for _h, _w in EXTENTS:
    BUILDERS["extents_%dx%d" % (_h, _w)] = functools.partial(_extents, _h, _w)
BUILDERS["extents_two_levels"] = _extents_two

CASES = list(BUILDERS)
# what the fixture records: everything the reference runs with defined behaviour (on the valid rows of each level) -- not the
# non-finite grad_output, whose NaN payloads are the compiler's choice
GOLDEN_CASES = [n for n in CASES if n != "nonfinite_top"]


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


BAD_ROW_CASES = [n for n in CASES if case(n)["bad_rows"]]


def pooled(c):
    return c["top"].shape[2:]


def levels_of(c):
    return np.zeros(len(c["rois"]), np.int64) if c["levels"] is None else c["levels"].astype(np.int64)


def bad_rows_by_rule(c):
    """the rows rb.is_bad names, each with its own level's scale"""
    lv = levels_of(c)
    n = len(c["shapes"])
    return [r for r in range(len(c["rois"]))
            if rb.is_bad(c["rois"][r], int(lv[r]), c["batch"], n, c["scales"][min(max(int(lv[r]), 0), n - 1)], pooled(c), c["ratio"])]


def without_bad_rows(c):
    good = [r for r in range(len(c["rois"])) if r not in c["bad_rows"]]
    return dict(c, top=np.ascontiguousarray(c["top"][good]), rois=np.ascontiguousarray(c["rois"][good]),
                levels=None if c["levels"] is None else np.ascontiguousarray(c["levels"][good]), bad_rows=[])


@functools.lru_cache(maxsize=None)
def restatement(name):
    """[(float32, float64, sum |terms|)] per level: computed once, shared, never modified"""
    with np.errstate(invalid="ignore", over="ignore"):
        res = rb.reference(case(name))
    for r in res:
        for a in r:
            a.setflags(write=False)
    return res


def reach(start, binsz, p, i, grid, extent):
    """(low, high) index of a sample along one axis as the kernel's pruning sees it, for an empty sample too: an empty sample
    below the map counts as (0, min(1, extent - 1)), one above it as (extent - 1, extent - 1).  From rb.axis alone: a sample
    that is empty on this map but not on one of extent 2^30 lies above the map."""
    ok, lo, hi, _, _ = rb.axis(start, binsz, p, i, grid, extent)
    if ok:
        return lo, hi
    if rb.axis(start, binsz, p, i, grid, 1 << 30)[0]:
        return extent - 1, extent - 1
    return 0, min(1, extent - 1)


def same_bits_or_nan(got, want):
    """bit patterns equal, except that a NaN equals a NaN of any payload (tests/README_optim.md): the SET of NaN elements is equal"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
