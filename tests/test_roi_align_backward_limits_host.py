"""RoIAlign backward off its default point, without a GPU (tests/roi_align_backward_limit_cases.py):
  * the numpy restatement against the reference's own output on every recorded case, BIT FOR BIT
    (tests/golden/roi_align_backward_limits.npz, made by tests/golden/make_roi_align_backward_limits_golden.py), inputs by digest;
  * every condition the cases are there for, asserted on the cases themselves, so that no GPU test passes emptily;
  * the monotonicity the tile kernel's range pruning rests on, restated over the `huge` and `grid` cases;
  * the passing side of the limits whose failing side tests/test_roi_align_backward_host.py holds, from a child process that sees
    no device.
Run as a script with --codes the module prints the return-code table as JSON (the child process of the test)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden
import roi_align_backward_limit_cases as lc
import roi_align_backward_ref as rb

F = np.float32


@pytest.fixture(scope="module")
def g():
    return golden("roi_align_backward_limits")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", lc.GOLDEN_CASES)
def test_restatement_equals_reference(g, name):
    c = lc.case(name)
    assert np.array_equal(rb.digest(c), g[name + "_digest"])
    ch = lc.sample_channels(name, c["top"].shape[1])
    assert (len(ch) == lc.SAMPLED_CHANNELS) == name.startswith("channels_")
    for l, (r32, _, _) in enumerate(lc.restatement(name)):
        want = g["%s_L%d" % (name, l)]
        assert want.shape == r32[:, ch].shape and np.array_equal(bits(r32[:, ch]), bits(want)), (name, l)


def test_the_fixture_holds_what_the_cases_name(g):
    want = {n + "_digest" for n in lc.GOLDEN_CASES} | {"%s_L%d" % (n, l) for n in lc.GOLDEN_CASES for l in range(len(lc.case(n)["shapes"]))}
    assert set(g.files) == want and "nonfinite_top" not in lc.GOLDEN_CASES and len(lc.CASES) == len(lc.GOLDEN_CASES) + 1


def geometry(c, r):
    s = c["scales"][int(lc.levels_of(c)[r])]
    return rb.roi_geometry(c["rois"][r, 1:], s, *lc.pooled(c), c["ratio"])


def samples(c, r):
    """(ph, pw, iy, ix, axis entry of y, axis entry of x) of every sample of RoI r"""
    l = int(lc.levels_of(c)[r])
    (h, w), (ph_n, pw_n) = c["shapes"][l], lc.pooled(c)
    sw, sh, bin_w, bin_h, gh, gw, _ = geometry(c, r)
    for ph in range(ph_n):
        for iy in range(gh):
            ay = rb.axis(sh, bin_h, ph, iy, gh, h)
            for pw in range(pw_n):
                for ix in range(gw):
                    yield ph, pw, iy, ix, ay, rb.axis(sw, bin_w, pw, ix, gw, w)


@pytest.mark.parametrize("name", lc.CASES)
def test_bad_rows_are_the_ones_the_rule_names(name):
    c = lc.case(name)
    assert lc.bad_rows_by_rule(c) == c["bad_rows"]
    assert (name in lc.BAD_ROW_CASES) == bool(c["bad_rows"])
    if c["bad_rows"]:                                # ... and the restatement of the call without them has the same bits
        with np.errstate(invalid="ignore", over="ignore"):
            clean = rb.reference(lc.without_bad_rows(c))
        assert len(lc.without_bad_rows(c)["rois"]) == len(c["rois"]) - len(c["bad_rows"])
        assert all(np.array_equal(bits(a[0]), bits(b[0])) for a, b in zip(clean, lc.restatement(name)))


def test_pooled_cases():
    assert lc.POOLED == [(1, 1), (1, 7), (7, 1), (3, 5), (5, 3), (2, 14), (14, 7)]
    for ph, pw in lc.POOLED:
        c = lc.case("pooled_%dx%d" % (ph, pw))
        assert c["top"].shape == (12, 3, ph, pw) and c["shapes"] == [(13, 17)] and c["batch"] == 2 and c["ratio"] == 2
        assert c["scales"] == [0.25] and lc.restatement("pooled_%dx%d" % (ph, pw))[0][0].any()
    for (ph, pw), pairs in lc.POOLED_ADAPTIVE.items():
        c = lc.case("pooled_%dx%d_adaptive" % (ph, pw))
        assert c["ratio"] == 0 and c["top"].shape == (12, 3, ph, pw)
        grids = [tuple(geometry(c, r)[4:6]) for r in range(12)]
        assert grids == pairs and all(gh != gw for gh, gw in grids)
    # a transposed read of top, or bins swapped, changes the result: the transposed case is another case
    a, b = lc.restatement("pooled_3x5")[0][0], lc.restatement("pooled_5x3")[0][0]
    assert not np.array_equal(a, b)


def test_ratio_cases():
    pow2 = lambda n: n & (n - 1) == 0
    fixed = [r for r in lc.RATIOS if r > 0]
    assert fixed == [1, 3, 4, 5, 7, 8] and [r * r for r in fixed] == [1, 9, 16, 25, 49, 64]
    assert {pow2(r * r) for r in fixed} == {True, False}
    base = lc.case("ratio_0")
    for r in lc.RATIOS:
        c = lc.case("ratio_%d" % r)
        assert c["top"].shape == (8, 2, 3, 3) and c["ratio"] == r
        assert np.array_equal(c["rois"], base["rois"]) and np.array_equal(c["top"], base["top"])
        assert [geometry(c, k)[4:6] for k in range(8)] == ([(r, r)] * 8 if r > 0 else [geometry(base, k)[4:6] for k in range(8)])
    counts = {int(geometry(base, k)[6]) for k in range(8)}
    assert {pow2(n) for n in counts} == {True, False}                          # adaptive: both ways to the quotient
    for r in (-1, -3):                                                          # <= 0 is adaptive
        assert np.array_equal(bits(lc.restatement("ratio_%d" % r)[0][0]), bits(lc.restatement("ratio_0")[0][0]))
    assert not np.array_equal(lc.restatement("ratio_1")[0][0], lc.restatement("ratio_0")[0][0])
    # ratio 64: 4096 samples of one RoI, every one valid, on at most 9 pixels
    c = lc.case("ratio_64_one_roi")
    assert len(c["rois"]) == 1 and lc.pooled(c) == (1, 1) and c["rois"][0, 3] - c["rois"][0, 1] == 2
    assert sum(1 for s in samples(c, 0) if s[4][0] and s[5][0]) == 4096
    assert 0 < np.count_nonzero(lc.restatement("ratio_64_one_roi")[0][0][0, 0]) <= 9
    # ratio 1024 = DTC_GRAD_MAX_SAMPLING: a few thousand valid samples of 2^20
    c = lc.case("ratio_1024")
    sw, sh, bin_w, bin_h, gh, gw, count = geometry(c, 0)
    assert (gh, gw, count) == (1024, 1024, F(2 ** 20)) and c["shapes"] == [(5, 7)]
    ny = sum(rb.axis(sh, bin_h, 0, i, gh, 5)[0] for i in range(gh))
    nx = sum(rb.axis(sw, bin_w, 0, i, gw, 7)[0] for i in range(gw))
    assert 500 < ny * nx <= 4000 and np.count_nonzero(lc.restatement("ratio_1024")[0][0]) == 2 * 35


def test_grid_cases():
    c = lc.case("grid_small")
    assert [tuple(geometry(c, r)[4:6]) for r in range(4)] == lc.GRIDS == [(6, 7), (9, 5), (16, 16), (31, 33)] and lc.pooled(c) == (2, 2)
    want = {"32768_y": (32768, 4), "32768_x": (3, 32768), "32768_yx": (32768, 32768), "32769_y": (32769, 4), "32769_x": (3, 32769)}
    for which in lc.GRID_LIMIT:
        c = lc.case("grid_" + which)
        assert c["shapes"] == [(5, 7)] and lc.pooled(c) == (1, 1) and c["scales"] == [1.0] and c["ratio"] == 0
        assert tuple(geometry(c, 1)[4:6]) == want[which]
        assert c["bad_rows"] == ([1] if "32769" in which else [])
        if "32769" in which:                         # ONE float32 step past the side that gives 32768
            side = max(c["rois"][1, 3] - c["rois"][1, 1], c["rois"][1, 4] - c["rois"][1, 2])
            assert side == np.nextafter(F(32768), F(np.inf)) and not rb.is_bad([0, 0, 0, 32768, 32768], 0, 1, 1, 1.0, (1, 1), 0)
        else:                                        # valid, and it contributes
            alone = dict(c, top=c["top"][1:2], rois=c["rois"][1:2])
            assert np.count_nonzero(rb.reference(alone)[0][0]) >= 10
    assert sum(1 for i in range(32768) if rb.axis(F(-16382), F(32768), 0, i, 32768, 5)[0]) == 6    # six samples of 32768 on the map


def test_huge_cases():
    h, w = lc.HUGE_MAP
    assert (h, w) == (9, 33) and rb.n_tiles([lc.HUGE_MAP], 1) == 9
    for name in ("huge_7x7", "huge_3x5", "huge_3x5_adaptive"):
        c = lc.case(name)
        ph, pw = lc.pooled(c)
        sizes = sorted({round(float(r[3] - r[1]) / w) for r in c["rois"] if r[3] - r[1] > w and np.abs(r[1:]).max() < F(1e6)})
        assert sizes == ([2, 10, 100] if name.endswith("adaptive") else [2, 10, 100, 10000])
        geo = [geometry(c, r) for r in range(len(c["rois"]))]
        assert sum(1 for q in geo if q[2] > w and q[3] > h) >= 4               # bins larger than the whole map
        assert sum(1 for q in geo if 1 < q[2] < w and 1 < q[3] < h) >= 2           # bin borders inside tiles, on both axes
        if not name.endswith("adaptive"):
            far = [r for r in c["rois"] if np.abs(r[1:]).max() == F(1e6)]
            assert len(far) == 4 and all(np.abs(r[1:]).min() < 33 for r in far)
        # the 1 x 1 boxes on the interior tile corners: the four taps of EVERY sample lie in four different tiles
        corners = [r for r in range(len(c["rois"])) if c["rois"][r, 1] == c["rois"][r, 3] and c["rois"][r, 2] == c["rois"][r, 4]]
        assert [(c["rois"][r, 2], c["rois"][r, 1]) for r in corners] == lc.TILE_CORNERS and len(corners) == 4
        for r in corners:
            n = 0
            for _, _, _, _, (vy, y0, y1, ly, hy), (vx, x0, x1, lx, hx) in samples(c, r):
                assert vy and vx
                assert len({(y // rb.TILE_H, x // rb.TILE_W) for y in (y0, y1) for x in (x0, x1)}) == 4
                n += 1
            assert n == ph * pw * geo[r][4] * geo[r][5]
    # the 2^29 limit: 2^29 - 32 is the float32 below it; valid there, with a sample on the map; bad at 2^29
    assert F(lc.A29) == np.nextafter(F(2.0 ** 29), F(0)) and lc.A29 == 2 ** 29 - 32
    for name, row in (("huge_limit_7x7", 1), ("huge_limit_3x5", 2)):
        c = lc.case(name)
        assert c["scales"] == [1.0, 0.25] and c["bad_rows"] == [4, 5, 6, 8, 9]
        assert np.abs(c["rois"][row, 1:]).max() == F(lc.A29)
        assert any(s[4][0] and s[5][0] for s in samples(c, row))               # a valid sample on the 2^29 - 32 RoI
        assert all(np.abs(c["rois"][r, 1:]).max() == F(2.0 ** 29) for r in (4, 5, 6))
        assert all(np.abs(c["rois"][r, 1:]).max() == F(2.0 ** 31) for r in (8, 9))
        assert np.abs(c["rois"][10, 1:]).max() * F(0.25) == F(lc.A29) and 10 not in c["bad_rows"]
    # coinciding float32 positions: 2048 sample columns on fewer than a third as many distinct positions
    c = lc.case("huge_coincide")
    sw, sh, bin_w, bin_h, gh, gw, _ = geometry(c, 0)
    assert c["shapes"] == [(1, 65536)] and lc.pooled(c) == (1, 1024) and bin_w == F(2.0 ** -10) and bin_w < np.spacing(sw) == F(2.0 ** -8)
    pos = [rb.axis(sw, bin_w, p, i, gw, 65536) for p in range(1024) for i in range(gw)]
    assert all(a[0] for a in pos)
    distinct = {(a[1], float(a[3])) for a in pos}
    assert 200 < len(distinct) < len(pos) // 3
    assert np.flatnonzero(lc.restatement("huge_coincide")[0][0]).tolist() == [40000, 40001, 40002]


def test_scale_cases():
    assert [lc.case("scale_" + k)["scales"][0] for k in ("third", "2", "0", "neg")] == [float(F(1.0 / 3.0)), 2.0, 0.0, -0.25]
    for k in ("third", "2", "0", "neg"):
        c = lc.case("scale_" + k)
        assert len(c["rois"]) == 8 and c["shapes"] == [(13, 17)] and not c["bad_rows"] and lc.restatement("scale_" + k)[0][0].any()
    c = lc.case("scale_0")                           # every RoI is the 1 x 1 box at the origin
    for r in range(8):
        sw, sh, bin_w, bin_h = geometry(c, r)[:4]
        assert sw == 0 and sh == 0 and bin_w == bin_h == F(1) / F(7)
    res = lc.restatement("scale_0")[0][0]
    assert res[:, :, 2:, :].any() == False and res[:, :, :, 2:].any() == False and res[:, :, :2, :2].all()    # noqa: E712
    c = lc.case("scale_neg")
    assert (c["rois"][:6, 1:] < 0).any() and sum(1 for r in range(8) if geometry(c, r)[2] > F(1) / F(7)) >= 5   # proper boxes at a negative scale


def test_groups_cases():
    assert lc.GROUP_SIZES == (255, 256, 257, 513) and rb.CH_BLOCK == 256       # the compaction's chunk is the block's 256 threads
    for n in lc.GROUP_SIZES:
        c = lc.case("groups_%d" % n)
        assert len(c["rois"]) == n and c["shapes"] == lc.GROUP_SHAPES and c["batch"] == 2
        assert c["bad_rows"] == sorted({r for r in lc.BAD_AT if r < n} | {n - 1})
        good = [r for r in range(n) if r not in c["bad_rows"]]
        key = c["levels"][good] * 2 + c["rois"][good, 0].astype(np.int64)
        assert set(key.tolist()) == set(range(6))
        assert np.all(key[1:] != key[:-1])                                      # interleaved row by row
        if n == 513:                                 # every group is populated in at least two chunks
            for k in range(6):
                assert len({good[i] // 256 for i in np.where(key == k)[0]}) >= 2
    c = lc.case("groups_513")
    kinds = c["rois"][c["bad_rows"]]
    assert np.isnan(kinds).any() and np.isinf(kinds).any() and (kinds[:, 0] == -1).any() and (kinds[:, 0] == 2).any()
    assert {-1, 3} <= set(c["levels"][c["bad_rows"]].tolist())
    c = lc.case("groups_one")
    assert len(c["rois"]) == 513 and set(c["levels"].tolist()) == {1} and set(c["rois"][:, 0].tolist()) - {1.0} <= {-1.0}
    res = lc.restatement("groups_one")
    assert res[1][0][1].all() and not res[1][0][0].any() and not res[0][0].any() and not res[2][0].any()
    c = lc.case("groups_8x3")
    assert len(c["shapes"]) == 8 and c["batch"] == 3 and len(c["rois"]) == 40 and sorted(c["shapes"]).count((1, 1)) == 2
    assert (1, 17) in c["shapes"]
    assert {(int(l), int(b)) for l, b in zip(c["levels"], c["rois"][:, 0])} == {(l, b) for l in range(8) for b in range(3)}
    assert all(r[0].any() for r in lc.restatement("groups_8x3"))
    c = lc.case("groups_null")
    res = lc.restatement("groups_null")
    assert c["levels"] is None and len(c["shapes"]) == 2 and res[0][0].any()
    assert np.array_equal(bits(res[1][0]), np.zeros_like(bits(res[1][0])))      # +0.0


def test_batch_index_case():
    c = lc.case("batch_index")
    assert [float(v) for v in c["rois"][:, 0]] == [float(F(v)) for v, _ in lc.BATCH_INDICES] and c["batch"] == 2
    assert F(-0.999) > -1 and F(1.999) < 2
    for r, (_, image) in enumerate(lc.BATCH_INDICES):
        alone = dict(c, top=c["top"][r:r + 1], rois=c["rois"][r:r + 1])
        res = rb.reference(alone)[0][0]
        assert [bool(res[b].any()) for b in range(2)] == [image == 0, image == 1], r
    assert c["bad_rows"] == [7, 8]


def test_nonfinite_top_case():
    c = lc.case("nonfinite_top")
    # the samples are pixel centres: l == 0 on both axes, so three of the four taps have weight 0
    for r in range(2):
        got = [(ay[1], ax[1], float(ay[3]), float(ax[3])) for _, _, _, _, ay, ax in samples(c, r)]
        assert got == [(1, 1, 0.0, 0.0), (1, 3, 0.0, 0.0), (3, 1, 0.0, 0.0), (3, 3, 0.0, 0.0)]
    res = lc.restatement("nonfinite_top")[0][0]
    ch0 = res[0, 0]
    assert ch0[1, 1] == np.inf and ch0[1, 3] == -np.inf and ch0[3, 3] == 1.5
    # inf * 0 and NaN * 0: the zero-weight taps put a NaN on the three neighbours of each; none next to the finite bin
    nan = np.zeros((5, 7), bool)
    for y, x in ((1, 1), (1, 3), (3, 1)):
        nan[y:y + 2, x:x + 2] = True
    nan[1, 1] = nan[1, 3] = False
    assert np.array_equal(np.isnan(ch0), nan) and nan.sum() == 10
    # image 1: -0.0 and -tiny bins; a pixel whose only terms are -0.0 holds 0.f + -0.0 = +0.0
    ch1 = res[1, 0]
    tiny = np.finfo(F).tiny
    assert bits(c["top"][1, 0, 0, 0]) == 0x80000000 and bits(ch1[1, 1]) == 0 and ch1[1, 3] == -tiny and ch1[3, 1] == 1.0
    assert np.count_nonzero(bits(ch1)) == 2 and np.isfinite(res[:, 1]).all() and res[:, 1].any()
    assert lc.same_bits_or_nan(res, res.copy()) and not lc.same_bits_or_nan(np.where(nan, 0, res[0, 0]), res[0, 0])
    other = res[0, 0].copy()
    other[2, 2] = -np.nan                            # a NaN of another sign or payload is the same NaN
    assert lc.same_bits_or_nan(other, res[0, 0])


def test_channels_and_extents_cases():
    assert lc.CHANNELS == (511, 512, 513, 769) and [-(-ch // rb.CH_BLOCK) for ch in lc.CHANNELS] == [2, 2, 3, 4]
    for ch in lc.CHANNELS:
        for h, w in lc.CHANNEL_MAPS:                 # both store paths
            c = lc.case("channels_%d_%dx%d" % (ch, h, w))
            assert c["top"].shape == (1, ch, 3, 3) and c["shapes"] == [(h, w)]
            res = lc.restatement("channels_%d_%dx%d" % (ch, h, w))[0][0]
            assert res[0, 0].any() and res[0, ch - 1].any()
    assert [w % 4 for _, w in lc.CHANNEL_MAPS] == [0, 1]
    assert lc.EXTENTS == ((257, 1), (1, 1024), (1, 1025))
    for h, w in lc.EXTENTS:
        c = lc.case("extents_%dx%d" % (h, w))
        assert c["top"].shape == (6, 1, 3, 3) and c["shapes"] == [(h, w)]
        longer = [r for r in c["rois"] if r[3] - r[1] > w and r[4] - r[2] > h]
        assert len(longer) == 2 and rb.n_tiles(c["shapes"], 1) == {257: 65, 1024: 64, 1025: 65}[max(h, w)]
        res = lc.restatement("extents_%dx%d" % (h, w))[0][0]
        assert len({(y // rb.TILE_H, x // rb.TILE_W) for y, x in zip(*np.nonzero(res[0, 0]))}) >= 8
        assert res[0, 0, 0, 0] != 0 and res[0, 0, -1, -1] != 0                   # from the first tile to the last
    c = lc.case("extents_two_levels")
    assert c["shapes"] == [(257, 1), (3, 5)] and all(r[0].any() for r in lc.restatement("extents_two_levels"))


@pytest.mark.parametrize("name", [n for n in lc.CASES if n.startswith(("huge", "grid"))])
def test_sample_reach_is_monotone(name):
    """What the kernel's `continue` / `break` on make_axis(...).lo / .hi rest on: along each axis the low and high index of a
    sample, an empty one included, do not decrease when the bin p or the sample i grows.  (Nothing is claimed, or needed, between
    the last sample of one bin and the first of the next: in float32 those can change places, as in huge_coincide.)"""
    c = lc.case(name)
    ph, pw = lc.pooled(c)
    for r in range(len(c["rois"])):
        if r in c["bad_rows"]:
            continue
        h, w = c["shapes"][int(lc.levels_of(c)[r])]
        sw, sh, bin_w, bin_h, gh, gw, _ = geometry(c, r)
        for start, binsz, n, grid, extent in ((sh, bin_h, ph, gh, h), (sw, bin_w, pw, gw, w)):
            m = np.array([[lc.reach(start, binsz, p, i, grid, extent) for i in range(grid)] for p in range(n)])   # [p, i, (lo, hi)]
            assert np.all(m[:, 1:] >= m[:, :-1]) and np.all(m[1:] >= m[:-1]), (name, r)
            assert np.all(m[..., 0] <= m[..., 1]) and m.min() >= 0 and m.max() <= extent - 1


# ---- return codes: the passing side of each limit ----------------------------------------------------------------------------------
# label -> (keyword overrides of test_roi_align_backward_host._call, expected code).  With the workspace NULL a call that passes the
# limits and the pointer checks ends in DTC_EWORKSPACE (-3), before anything touches a device; one past the limit is
# DTC_EUNSUPPORTED (-4) whatever the workspace is.  The failing sides with a workspace are in tests/test_roi_align_backward_host.py.
CODES = {
    "ratio 1024, workspace NULL": (dict(sampling_ratio=1024, workspace=None), -3), "ratio 1025, workspace NULL": (dict(sampling_ratio=1025, workspace=None), -4),
    "ratio -1024, workspace NULL": (dict(sampling_ratio=-1024, workspace=None), -3),
    "pooled_h 1024, workspace NULL": (dict(pooled_h=1024, workspace=None), -3), "pooled_w 1024, workspace NULL": (dict(pooled_w=1024, workspace=None), -3),
    "pooled_w 1025, workspace NULL": (dict(pooled_w=1025, workspace=None), -4),
    "n_levels 8, workspace NULL": (dict(n_levels=8, workspace=None), -3), "n_levels 9, workspace NULL": (dict(n_levels=9, workspace=None), -4),
    "scale 0, workspace NULL": (dict(scale=0.0, workspace=None), -3), "scale -0.25, workspace NULL": (dict(scale=-0.25, workspace=None), -3),
    "channels 769, workspace NULL": (dict(channels=769, workspace=None), -3),
    "width 65536, workspace NULL": (dict(height=1, width=65536, workspace=None), -3),
}


def test_return_codes_at_the_limits():
    import test_roi_align_backward_host as th
    assert not set(CODES) & set(th.CODES)                                        # those the other module already holds are not repeated
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--codes"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert json.loads(out.stdout.decode()) == {k: v[1] for k, v in CODES.items()}


if __name__ == "__main__" and "--codes" in sys.argv:
    import test_roi_align_backward_host as th
    from detectorch_amd import hip_grad as hg
    print(json.dumps({k: th._call(hg, **kw) for k, (kw, _) in CODES.items()}))
