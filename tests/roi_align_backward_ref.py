"""RoIAlign backward as the reference computes it, restated in numpy float32, and the seeded cases of the RoIAlign-backward tests.

backward() restates roi_align_backward_loop of the reference's lib/cppcuda/roi_align_backward_cpu.cpp (cited below as :line)
operation for operation in float32: one rounding per operation, the terms added to each element in the loop's order n, ph, pw, iy,
ix, taps 1-4.  The loop over c is vectorised (the channels of one (n, ph, pw) are independent elements, so every element still
receives its terms in the serial order).  tests/test_roi_align_backward_host.py holds it to the reference's own output, bit for
bit (tests/golden/roi_align_backward.npz, made by tests/golden/make_roi_align_backward_golden.py from the reference's source).
Beside the float32 result it gives the float64 yardstick (the same taps, every product and sum in float64) and, per element,
the sum of |terms|: the scale of the rounding error of a float32 sum.

backward_levels() is the multi-level call of include/detectorch_grad_hip.h: the loop per level on the RoIs of that level, bad
RoIs (batch or level out of range, non-finite coordinates) left out.
"""
import hashlib
import math

import numpy as np

F = np.float32
EPS = float(np.finfo(np.float32).eps)

# the kernel's tile and channel block (detectorch_amd/csrc/grad/roi_align_backward.hip: kTileH, kTileW, kBwdThreads), tied to the
# source text by tests/test_roi_align_backward_host.py
TILE_H, TILE_W, CH_BLOCK = 4, 16, 256
LDS_BYTES = TILE_H * TILE_W * (CH_BLOCK + 1) * 4
REC_BYTES, GROUP_BYTES = 48, 8


def workspace_bytes(n_levels, batch, n_rois):
    """dtc_roi_align_backward_workspace_bytes: (offset, count) per (level, image), one record per RoI, blocks rounded up to 16"""
    up = lambda v: (v + 15) // 16 * 16
    return up(n_levels * batch * GROUP_BYTES) + up(max(n_rois, 1) * REC_BYTES)


def n_tiles(shapes, batch):
    """work items of the tile kernel over the levels' (height, width)"""
    return sum(batch * (-(-h // TILE_H)) * (-(-w // TILE_W)) for h, w in shapes)


def axis(start, binsz, p, i, grid, extent):
    """One axis of a sample: position (:145-151) and bilinear_interpolate_gradient (:26-59) -> (valid, low, high, l, h)."""
    v = F(F(start + F(F(p) * binsz)) + F(F(F(F(i) + F(.5)) * binsz) / F(grid)))      # :145-147 / :149-151, left to right
    if v < F(-1.0) or v > F(extent):                                                  # :26
        return False, -1, -1, F(0), F(0)                                              # :28-30
    if v <= F(0):                                                                     # :33-38
        v = F(0)
    lo = int(v)                                                                       # :40-41
    if lo >= extent - 1:                                                              # :43-45 / :50-52
        hi = lo = extent - 1
        v = F(lo)
    else:
        hi = lo + 1                                                                   # :47 / :54
    l = F(v - F(lo))                                                                  # :57-58
    h = F(1.0 - float(l))                                                             # :59  "1. - ly": double, rounded once
    return True, lo, hi, l, h


def roi_geometry(roi4, scale, pooled_h, pooled_w, sampling_ratio):
    """:112-142 -> (start_w, start_h, bin_w, bin_h, grid_h, grid_w, count)"""
    s = F(scale)
    sw, sh, ew, eh = F(roi4[0] * s), F(roi4[1] * s), F(roi4[2] * s), F(roi4[3] * s)  # :112-115
    rw, rh = max(F(ew - sw), F(1.)), max(F(eh - sh), F(1.))                           # :122-123
    bin_h, bin_w = F(rh / F(pooled_h)), F(rw / F(pooled_w))                           # :124-125
    gh = sampling_ratio if sampling_ratio > 0 else int(math.ceil(F(rh / F(pooled_h))))   # :135-137
    gw = sampling_ratio if sampling_ratio > 0 else int(math.ceil(F(rw / F(pooled_w))))   # :138-139
    return sw, sh, bin_w, bin_h, gh, gw, F(gh * gw)                                   # :142


def backward(top, rois, batch, height, width, scale, sampling_ratio, rows=None):
    """roi_align_backward_cpu (:189-234) on top [R, C, PH, PW] float32 and rois [R, 4 | 5] float32 -> (float32 result, float64
    yardstick, sum of |terms|), each [batch, C, height, width].  rows: the RoIs to run, in this order (default: all)."""
    R, C, PH, PW = top.shape
    out = np.zeros((batch, C, height, width), F)                                      # :214
    y64 = np.zeros((batch, C, height, width), np.float64)
    mag = np.zeros((batch, C, height, width), np.float64)
    top64 = top.astype(np.float64)
    cols = rois.shape[1]
    for n in (range(R) if rows is None else rows):                                    # :97, :102
        b = int(rois[n, 0]) if cols == 5 else 0                                       # :105-109
        sw, sh, bin_w, bin_h, gh, gw, count = roi_geometry(rois[n, cols - 4:], scale, PH, PW, sampling_ratio)
        for ph in range(PH):                                                          # :100
            # an empty sample (:26-31, :176) adds nothing: dropped here, before the product of the two axes, in the loops' order
            ys = [a for a in (axis(sh, bin_h, ph, iy, gh, height) for iy in range(gh)) if a[0]]
            if not ys:
                continue
            for pw in range(PW):                                                      # :99
                t, t64 = top[n, :, ph, pw], top64[n, :, ph, pw]                       # :130-132
                xs = [a for a in (axis(sw, bin_w, pw, ix, gw, width) for ix in range(gw)) if a[0]]
                for vy, y_lo, y_hi, ly, hy in ys:                                     # :144
                    for vx, x_lo, x_hi, lx, hx in xs:                                 # :148
                        ws = (F(hy * hx), F(hy * lx), F(ly * hx), F(ly * lx))         # :68
                        w64 = (float(hy) * float(hx), float(hy) * float(lx), float(ly) * float(hx), float(ly) * float(lx))
                        at = ((y_lo, x_lo), (y_lo, x_hi), (y_hi, x_lo), (y_hi, x_hi))  # :178-181
                        for (yy, xx), w, wd in zip(at, ws, w64):
                            g = (t * w) / count                                       # :171-174  top * w / count in float32
                            out[b, :, yy, xx] = out[b, :, yy, xx] + g                 # :75
                            g64 = t64 * wd / float(count)
                            y64[b, :, yy, xx] += g64
                            mag[b, :, yy, xx] += np.abs(g64)
    return out, y64, mag


def is_bad(roi, level, batch, n_levels, scale=1.0, pooled=(7, 7), sampling_ratio=2):
    """the RoIs that contribute nothing (include/detectorch_grad_hip.h)"""
    if not 0 <= level < n_levels:
        return True
    if len(roi) == 5:
        if not (roi[0] > -1 and roi[0] < batch):
            return True
    c = np.asarray(roi[-4:], F)
    if not np.all(np.isfinite(c)):
        return True
    with np.errstate(over="ignore"):
        s = c * F(scale)
    if not np.all(np.abs(s) < F(2.0 ** 29)):
        return True
    if sampling_ratio <= 0:
        g = roi_geometry(c, scale, pooled[0], pooled[1], sampling_ratio)
        return g[4] > 32768 or g[5] > 32768
    return False


def backward_levels(top, rois, roi_levels, batch, shapes, scales, sampling_ratio):
    """dtc_roi_align_backward: per level l, backward() on the valid RoIs of that level in ascending index
    -> [(float32, float64, sum |terms|)] per level.  roi_levels None: level 0."""
    R = top.shape[0]
    lv = np.zeros(R, np.int64) if roi_levels is None else np.asarray(roi_levels, np.int64)
    res = []
    for l, ((h, w), s) in enumerate(zip(shapes, scales)):
        rows = [n for n in range(R) if lv[n] == l and
                not is_bad(rois[n], int(lv[n]), batch, len(shapes), s, top.shape[2:], sampling_ratio)]
        res.append(backward(top, rois, batch, h, w, s, sampling_ratio, rows))
    return res


def forward_tables(rois, batch, height, width, scale, pooled_h, pooled_w, sampling_ratio):
    """The taps of the forward pass in the reference's float32 geometry, for a float64 restatement of the forward:
    (roi, ph, pw, image, y, x, weight as float64, 1 / count as float64), one row per tap of every valid sample."""
    rows = []
    cols = rois.shape[1]
    for n in range(rois.shape[0]):
        b = int(rois[n, 0]) if cols == 5 else 0
        sw, sh, bin_w, bin_h, gh, gw, count = roi_geometry(rois[n, cols - 4:], scale, pooled_h, pooled_w, sampling_ratio)
        for ph in range(pooled_h):
            for pw in range(pooled_w):
                for iy in range(gh):
                    vy, y_lo, y_hi, ly, hy = axis(sh, bin_h, ph, iy, gh, height)
                    for ix in range(gw):
                        vx, x_lo, x_hi, lx, hx = axis(sw, bin_w, pw, ix, gw, width)
                        if not (vy and vx):
                            continue
                        for yy, xx, w in ((y_lo, x_lo, float(hy) * float(hx)), (y_lo, x_hi, float(hy) * float(lx)),
                                          (y_hi, x_lo, float(ly) * float(hx)), (y_hi, x_hi, float(ly) * float(lx))):
                            rows.append((n, ph, pw, b, yy, xx, w, 1.0 / float(count)))
    return np.array(rows, np.float64).reshape(-1, 8)


# ---- the seeded cases --------------------------------------------------------------------------------------------------------------
def _rs(*seed):
    return np.random.RandomState(list(seed))


def _rois(rs, n, batch, h, w, scale, lo=2.0, hi=None, cols=5):
    """n boxes inside a [h, w] map at `scale`, sides lo .. hi map pixels, rounded to float32"""
    hi = hi or max(h, w) * 0.8
    x1 = rs.uniform(-1.0, w - 1.0, n)
    y1 = rs.uniform(-1.0, h - 1.0, n)
    bw, bh = rs.uniform(lo, hi, n), rs.uniform(lo, hi, n)
    r = np.stack([x1, y1, np.minimum(x1 + bw, w + 1.5), np.minimum(y1 + bh, h + 1.5)], 1) / scale
    if cols == 5:
        r = np.hstack([rs.randint(0, batch, (n, 1)).astype(np.float64), r])
    return np.ascontiguousarray(r, F)


def _top(rs, n, c, ph, pw):
    return rs.standard_normal((n, c, ph, pw)).astype(F)


def _case(top, rois, batch, shapes, scales, ratio, levels=None):
    return dict(top=np.ascontiguousarray(top, F), rois=np.ascontiguousarray(rois, F), batch=batch, shapes=list(shapes),
                scales=[float(F(s)) for s in scales], ratio=ratio, levels=None if levels is None else np.asarray(levels, np.int32))


CHANNEL_WIDTHS = (1, 3, 64, 65, 256, 257)           # (b): 257 is one past the kernel's channel block
TILE_EXTENTS_H = (1, TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1)
TILE_EXTENTS_W = (1, TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W + 1)
SAMPLED_CHANNELS = 4                                # channels of the larger cases that the fixture records


def make_case(name):
    if name == "a":                                  # one RoI, C = 1, 5 x 7 map, 2 x 2 bins, ratio 2
        rs = _rs(11, 1)
        return _case(_top(rs, 1, 1, 2, 2), [[0, 1.25, 0.5, 5.0, 3.75]], 1, [(5, 7)], [1.0], 2)
    if name.startswith("b"):                         # channel widths: B = 2, 13 x 17, 40 RoIs, 7 x 7, ratio 2
        c = int(name[1:])
        rois = _rois(_rs(11, 2), 40, 2, 13, 17, 0.25)
        return _case(_top(_rs(11, 2, c), 40, c, 7, 7), rois, 2, [(13, 17)], [0.25], 2)
    if name == "c":                                  # adaptive sampling: 14 x 14 bins, grids 1 x 1 .. 5 x 3
        rs = _rs(11, 3)
        grids = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (2, 3), (3, 3), (4, 2), (4, 3), (5, 3), (5, 1), (1, 3)]
        rois = []
        for gh, gw in grids:                         # a side of 14 * (g - 0.5) map pixels gives grid g
            bh, bw = 14.0 * (gh - 0.5), 14.0 * (gw - 0.5)
            x1, y1 = rs.uniform(0, 60 - bw), rs.uniform(0, 80 - bh)
            rois.append([0, x1 * 8, y1 * 8, (x1 + bw) * 8, (y1 + bh) * 8])
        c = _case(_top(rs, len(grids), 2, 14, 14), rois, 1, [(80, 60)], [0.125], 0)
        c["grids"] = grids
        return c
    if name == "d":                                  # map edges and degenerate boxes, 13 x 17 map at scale 1
        rs = _rs(11, 4)
        rois = [[0, -6.0, -5.0, 4.0, 3.0], [1, 12.0, 8.0, 25.0, 20.0],            # partly off: top left, bottom right
                [0, -40.0, -40.0, -20.0, -20.0], [1, 30.0, 30.0, 50.0, 50.0],      # wholly off
                [0, 18.5, 2.0, 30.0, 6.0], [1, 2.0, 14.5, 9.0, 22.0],              # wholly off on one axis only
                [0, -0.9, -0.9, 6.1, 6.1], [1, -1.0, -1.0, 2.5, 2.5],              # samples in [-1, 0]
                [0, 10.0, 7.0, 17.0, 13.0], [1, 15.5, 11.5, 17.0, 13.0],           # samples at >= H - 1 / W - 1 (collapsed taps)
                [0, 9.0, 5.0, 16.0, 12.0], [1, 16.0, 12.0, 16.0, 12.0],
                [0, 8.0, 4.0, 3.0, 9.0], [1, 8.0, 9.0, 12.0, 2.0], [0, 9.0, 9.0, 2.0, 2.0],   # x2 < x1, y2 < y1, both
                [0, 5.0, 5.0, 5.0, 5.0], [1, 3.5, 7.25, 3.5, 7.25], [0, 0.0, 0.0, 0.0, 0.0]]  # zero size (forced 1 x 1)
        return _case(_top(rs, len(rois), 3, 7, 7), rois, 2, [(13, 17)], [1.0], 2)
    if name.startswith("e"):                         # tile boundaries: e<H>x<W>
        h, w = (int(v) for v in name[1:].split("x"))
        rs = _rs(11, 5, h, w)
        rois = _rois(rs, 6, 1, h, w, 1.0, lo=1.0, hi=max(h, w) + 2.0)
        return _case(_top(rs, 6, 2, 7, 7), rois, 1, [(h, w)], [1.0], 2)
    if name in ("f", "fsmall", "fbig"):              # 300 RoIs piled on one pixel neighbourhood of a 9 x 9 map
        rs = _rs(11, 6)
        c0 = rs.uniform(3.8, 4.2, (300, 2))
        half = rs.uniform(0.6, 1.4, (300, 2))
        rois = np.hstack([np.zeros((300, 1)), c0 - half, c0 + half])
        top = _top(rs, 300, 2, 7, 7)
        if name == "fsmall":
            top = top * F(1e-40)                     # denormal terms
        if name == "fbig":
            top = top * F(1e30)
        return _case(top, rois, 1, [(9, 9)], [1.0], 2)
    if name in ("g", "g4"):
        rs = _rs(11, 7)
        if name == "g4":                             # 4-column RoIs: image 0 of two
            return _case(_top(rs, 12, 3, 7, 7), _rois(rs, 12, 1, 13, 17, 0.5, cols=4), 2, [(13, 17)], [0.5], 2)
        shapes, scales = [(32, 40), (16, 20), (8, 10), (4, 5)], [0.25, 0.125, 0.0625, 0.03125]
        levels = rs.choice([0, 1, 3], 30)            # level 2 has no RoI
        rois = np.vstack([_rois(rs, 1, 2, shapes[l][0], shapes[l][1], scales[l], lo=1.5) for l in levels])
        rois[levels == 3, 0] = 0                     # image 1 of level 3 has none either
        return _case(_top(rs, 30, 3, 7, 7), rois, 2, shapes, scales, 2, levels)
    if name == "h":                                  # bad RoIs among good ones (two levels, two images)
        rs = _rs(11, 8)
        shapes, scales = [(13, 17), (7, 9)], [0.25, 0.125]
        levels = rs.randint(0, 2, 24)
        rois = np.vstack([_rois(rs, 1, 2, shapes[l][0], shapes[l][1], scales[l], lo=1.5) for l in levels])
        bad = {1: (0, -1.0), 4: (0, 2.0), 6: (1, np.nan), 9: (3, np.inf), 11: (2, -np.inf), 13: (4, np.nan), 15: (0, np.nan),
               17: (0, -7.0), 19: (0, 1e9)}
        for r, (col, v) in bad.items():
            rois[r, col] = v
        levels[[2, 20]] = -1, 2                      # level -1 and level n_levels
        c = _case(_top(rs, 24, 3, 7, 7), rois, 2, shapes, scales, 2, levels)
        c["bad_rows"] = sorted(list(bad) + [2, 20])
        return c
    if name == "i":                                  # middle-sized: B = 2, C = 256, 50 x 84, 512 RoIs
        rs = _rs(11, 9)
        return _case(_top(rs, 512, 256, 7, 7), _rois(rs, 512, 2, 50, 84, 0.0625, lo=2.0, hi=30.0), 2, [(50, 84)], [0.0625], 2)
    if name == "k":                                  # autograd: two levels, two images
        rs = _rs(11, 10)
        shapes, scales = [(13, 17), (7, 9)], [0.25, 0.125]
        levels = rs.randint(0, 2, 16)
        rois = np.vstack([_rois(rs, 1, 2, shapes[l][0], shapes[l][1], scales[l], lo=1.5) for l in levels])
        return _case(_top(rs, 16, 8, 7, 7), rois, 2, shapes, scales, 2, levels)
    raise KeyError(name)


TILE_CASES = ["e%dx%d" % (h, w) for h in TILE_EXTENTS_H for w in TILE_EXTENTS_W]
# what the fixture records: every channel of the small cases, sample_channels() of the wide ones
GOLDEN_CASES = ["a", "b1", "b3", "b64", "b65", "b256", "b257", "c", "d", "e3x17", "e9x33", "f", "fsmall", "fbig", "g", "g4", "i"]
SAMPLED_CASES = ("b64", "b65", "b256", "b257", "i")


def sample_channels(name, channels):
    """the channels of a SAMPLED_CASES case that the fixture holds: the first, the last and seeded ones between"""
    if name not in SAMPLED_CASES:
        return np.arange(channels)
    rs = _rs(11, 99, channels)
    return np.unique(np.concatenate([[0, channels - 1], rs.choice(np.arange(1, channels - 1), SAMPLED_CHANNELS - 2, replace=False)]))


def digest(c):
    h = hashlib.sha1()
    for a in (c["top"], c["rois"], np.zeros(0, np.int32) if c["levels"] is None else c["levels"]):
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def reference(c, channels=None):
    """backward_levels on a case (optionally on some channels only: the channels are independent)"""
    top = c["top"] if channels is None else np.ascontiguousarray(c["top"][:, channels])
    return backward_levels(top, c["rois"], c["levels"], c["batch"], c["shapes"], c["scales"], c["ratio"])
