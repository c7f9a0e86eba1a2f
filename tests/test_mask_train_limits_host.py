"""Mask training past the sizes of its first tests, without a GPU (cases: tests/mask_train_limit_cases.py):
  * the numpy restatement against the reference's own building blocks on every new case (tests/golden/mask_train_limits.npz, made by
    tests/golden/make_mask_train_limits_golden.py): poly-boxes and the sampled overlaps as float32 bits, the first maximum, mask_gt
    and the masks reproducible; the float64 loss yardstick against torch's, the recorded e_ref inside the bounds;
    polys_to_mask_wrt_box itself where the second golden exists;
  * one test per case of the condition that case is there for, on the restatement alone: a case that drifts off its condition fails
    here, not by passing emptily on the GPU;
  * the rectangle known answer at every M from 1 to 56; the kernel's event form against the trace on the new polygons.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden
import mask_train_limit_cases as lc
import mask_train_ref as mr
from test_mask_train_host import rect_answer, same_bits

SINGLE = sorted(n for n in lc.TARGETS if not n.startswith("all_m"))


@pytest.fixture(scope="module")
def g():
    return golden("mask_train_limits")


# ---- the restatement against the reference's building blocks ------------------------------------------------------------------------
def restatement_equals_reference(g, name, tag):
    img, M, k_min, k_max, Fm = lc.case(name)
    o = lc.want(name)
    elig = lc.eligible(img)
    pb = mr.poly_boxes([mr.valid_polys(img, q) for q in elig]) if elig else np.zeros((0, 4), np.float32)
    assert same_bits(pb, g[tag + "_poly_boxes"])
    rows = lc.sample_rows(name)
    want = g[tag + "_overlaps"]
    assert want.shape == (len(rows), len(elig) if rows else len(pb))
    boxes = lc.row_boxes(name, rows)
    for k, t in enumerate(rows):
        ov = mr.bbox_overlaps(boxes[k][None], pb)[0]
        assert same_bits(ov, want[k]) and elig[int(np.argmax(want[k]))] == o["mask_gt"][t]
    assert same_bits(o["mask_gt"], g[tag + "_mask_gt"])
    return o, rows


@pytest.mark.parametrize("case", SINGLE)
def test_restatement_equals_reference(g, case):
    o, _ = restatement_equals_reference(g, case, case)
    assert same_bits(o["masks"].astype(np.int8), g[case + "_masks"])


def test_restatement_equals_reference_at_every_m(g):
    masks = []
    for M in lc.ALL_M:
        o, rows = restatement_equals_reference(g, "all_m%d" % M, "all_m")
        assert rows == [0, 1]
        masks.append(o["masks"][rows].astype(np.int8).reshape(-1))
    assert same_bits(np.concatenate(masks), g["all_m_masks"])


def test_polys_to_mask_wrt_box_where_recorded():
    """pin-when-available: the generator records pycocotools' own rasterisation only where pycocotools imports"""
    path = os.path.join(GOLDEN, "mask_train_limits_coco.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/mask_train_limits_coco.npz is absent: pycocotools was not available to the generator (parity unpinned)")
    coco = np.load(path)
    for name in SINGLE:
        assert np.array_equal(lc.want(name)["masks"][lc.sample_rows(name)].astype(np.int8), coco[name + "_masks"]), name
    mine = np.concatenate([lc.want("all_m%d" % M)["masks"][:2].astype(np.int8).reshape(-1) for M in lc.ALL_M])
    assert np.array_equal(mine, coco["all_m_masks"])


def test_the_golden_is_small_and_holds_data_only(g):
    size = lambda n: os.path.getsize(os.path.join(GOLDEN, n))
    assert size("mask_train_limits.npz") <= size("mask_train.npz")
    assert all(g[k].dtype.kind in "fiu" for k in g.files)


LOSS_TAGS = [(n, False) for n in lc.LOSS] + [(n, True) for n in lc.MULTI_ROW]


@pytest.mark.parametrize("case,extremes", LOSS_TAGS)
def test_loss_yardstick_equals_reference(g, case, extremes):
    tag = case + ("_x" if extremes else "")
    y = lc.loss_want(case, extremes)
    want = float(g["loss_" + tag])
    assert abs(y["loss"] - want) <= 1e-12 * max(1.0, abs(want))                  # two float64 sums in different orders
    mine, ref = y["grad"].ravel()[lc.grad_sample(case, extremes)], g["loss_" + tag + "_grad"]
    assert np.array_equal(mine == 0, ref == 0) and np.allclose(mine, ref, rtol=1e-12, atol=0) and (ref != 0).sum() >= 2
    b = mr.loss_bounds(y)
    # as on the first cases: the float32 CPU reference stays within a quarter of every bound, so the 32 eps arm governs
    assert float(g["loss_" + tag + "_e_ref"]) <= b["loss"] / 4 and float(g["loss_" + tag + "_e_grad"]) <= 0.25


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------
def test_rows700_fm512_reaches_three_rounds_and_cuts_in_the_third():
    img, M, _, _, Fm = lc.case("rows700_fm512")
    o = lc.want("rows700_fm512")
    R = len(img["labels"])
    assert (R, img["n_rois"], len(img["gt_boxes"]), len(img["proposals"]), Fm, M) == (700, 650, 37, 300, 512, 7) and Fm == mr.MAX_ROWS
    assert -(-R // lc.BLOCK) == 3 and 0.8 < (img["labels"] > 0).mean() < 0.9
    groups = lc.wave_groups(img)
    assert len(groups) == 11 and all(1 <= len(q) <= min(63, min(64, 650 - 64 * i) - 1) for i, q in enumerate(groups))
    fg = lc.fg_rows(img)
    cut = fg[Fm - 1]                                                             # the 512th foreground row
    mine = groups[cut // 64]
    assert len(fg) > Fm and 2 * lc.BLOCK <= cut < 650 and mine[0] < cut < mine[-1] and fg[Fm] // 64 == cut // 64
    assert (img["labels"][650:] > 0).sum() >= 30 and not o["roi_has_mask"][650:].any()
    assert int(o["n_mask"]) == Fm and np.flatnonzero(o["roi_has_mask"]).tolist() == fg[:Fm] and np.all(o["mask_gt"] >= 0)
    assert [len(range(w, 37, lc.WAVES)) for w in range(lc.WAVES)] == [10, 9, 9, 9] and img["gt_count"] == 37
    keep = img["keep_inds"][fg[:Fm]]
    assert (keep < 37).sum() >= 20 and (keep >= 37).sum() >= 400
    assert img["gt_is_crowd"][5] == 1 and img["gt_classes"][11] == 0 and not set(o["mask_gt"].tolist()) & {5, 11}
    assert len(set(o["mask_gt"].tolist())) >= 30 and len(set(o["mask_roi_levels"].tolist())) >= 2


def test_rows700_fm300_cuts_in_the_second_round():
    img, _, _, _, Fm = lc.case("rows700_fm300")
    o = lc.want("rows700_fm300")
    fg = lc.fg_rows(img)
    assert Fm == 300 and lc.BLOCK <= fg[Fm - 1] < 2 * lc.BLOCK and int(o["n_mask"]) == Fm
    assert -(-Fm // lc.BLOCK) == 2 and Fm % lc.BLOCK == 44                       # section 4: a second, partial round
    assert np.all(o["roi_has_mask"][fg[:Fm]] == 1) and len(fg[Fm:]) > 200 and not o["roi_has_mask"][fg[Fm:]].any()
    full = lc.want("rows700_fm512")
    for k in ("mask_rois", "masks", "mask_class", "mask_roi_levels", "mask_gt"):
        assert same_bits(o[k], full[k][:Fm])


def test_rows700_fm5_cuts_inside_the_first_wavefront():
    img, _, _, _, Fm = lc.case("rows700_fm5")
    o = lc.want("rows700_fm5")
    fg = lc.fg_rows(img)
    assert Fm == 5 and fg[Fm - 1] < 64 and fg[Fm] < 64 and int(o["n_mask"]) == 5 and np.flatnonzero(o["roi_has_mask"]).tolist() == fg[:5]


def test_rows4096_is_the_limit_and_leaves_rows_past_n_mask():
    from detectorch_amd import hip_mask
    img, M, _, _, Fm = lc.case("rows4096")
    o = lc.want("rows4096")
    R = len(img["labels"])
    assert R == img["n_rois"] == hip_mask.MAX_ROIS == 4096 and R // lc.BLOCK == 16 and Fm == 512
    groups = lc.wave_groups(img)
    assert all(any(groups[4 * b + w] for w in range(4)) for b in range(16)) and 0.02 < (img["labels"] > 0).mean() < 0.04
    n = int(o["n_mask"])
    assert 64 < n < Fm and n == len(lc.fg_rows(img)) == o["roi_has_mask"].sum()
    assert not o["mask_rois"][n:].any() and not o["mask_class"][n:].any() and not o["mask_roi_levels"][n:].any()
    assert np.all(o["masks"][n:] == -1) and np.all(o["mask_gt"][n:] == -1) and np.all(o["mask_gt"][:n] >= 0)
    assert o["mask_rois"][n:].view(np.uint32).max() == 0                         # +0.0


def test_late_bg_finds_the_fallback_row_in_the_second_round():
    img = lc.case("late_bg")[0]
    o = lc.want("late_bg")
    assert len(img["labels"]) == 600 == img["n_rois"] and np.flatnonzero(img["labels"] == 0).tolist() == [403, 590]
    assert not (img["labels"] > 0).any() and np.all(np.delete(img["labels"], [403, 590]) == -1) and lc.BLOCK <= 403 < 2 * lc.BLOCK
    assert int(o["n_mask"]) == 1 and np.flatnonzero(o["roi_has_mask"]).tolist() == [403] and o["roi_has_mask"][403] == 1
    assert o["mask_class"][0] == 0 and np.all(o["masks"] == -1) and np.all(o["mask_gt"] == -1)
    assert o["mask_rois"][0].tolist() == [0, 2, 4, 60, 80] and not o["mask_rois"][1:].any()


def test_late_bg_past_has_its_background_rows_past_n_rois():
    img = lc.case("late_bg_past")[0]
    o = lc.want("late_bg_past")
    assert img["n_rois"] == 403 == min(np.flatnonzero(img["labels"] == 0)) and not (img["labels"] > 0).any()
    assert int(o["n_mask"]) == 0 and not o["roi_has_mask"].any() and not o["mask_rois"].any() and np.all(o["masks"] == -1)


# ---- the gt -----------------------------------------------------------------------------------------------------------------------------
def test_gt256_has_stale_rows_that_would_win_and_ties_across_wavefronts():
    from detectorch_amd import hip_mask
    img, M, _, _, Fm = lc.case("gt256")
    o = lc.want("gt256")
    G, n_g = len(img["gt_boxes"]), img["gt_count"]
    assert G == hip_mask.MAX_GT == 256 and n_g == 250 and len(img["labels"]) == Fm == 300 and M == 14 and int(o["n_mask"]) == 300
    ar = np.arange(G)
    assert np.all(img["gt_is_crowd"][:n_g] == (ar % 7 == 0)[:n_g]) and np.all((img["gt_classes"] == 0)[:n_g] == (ar % 11 == 0)[:n_g])
    two = [q for q in range(n_g) if q % 13 == 5]
    assert all(img["poly_ptr"][img["gt_poly_ptr"][q] + 1] - img["poly_ptr"][img["gt_poly_ptr"][q]] == 2 for q in two) and len(two) == 19
    elig = lc.eligible(img)
    skipped = set(range(n_g)) - set(elig)
    assert skipped == {q for q in range(n_g) if q % 7 == 0 or q % 11 == 0 or q % 13 == 5} and len(elig) == 180
    matched = set(o["mask_gt"].tolist())
    assert matched <= set(elig) and len(matched) >= 100 and max(matched) < n_g
    assert max(len([q for q in elig if q % 4 == w]) for w in range(4)) > 40   # every wavefront takes many gt
    pb = mr.poly_boxes([mr.valid_polys(img, q) for q in elig])
    # the ties: duplicate gt on different wavefronts, both above 64; the lower index wins whichever of the two boxes the row has
    for a, b in lc.GT256_TIES:
        assert 64 < a < b < n_g and a % 4 != b % 4 and a in elig and b in elig and same_bits(pb[elig.index(a)], pb[elig.index(b)])
    assert sorted(img["keep_inds"][:4].tolist()) == sorted(sum(lc.GT256_TIES, ()))
    for t, want in lc.GT256_TIE_ROWS.items():
        ov = mr.bbox_overlaps(lc.row_boxes("gt256", [t]), pb)[0]
        a, b = next(p for p in lc.GT256_TIES if p[0] == want)
        assert ov[elig.index(a)] == ov[elig.index(b)] == ov.max() == 1 and (ov == ov.max()).sum() == 2 and o["mask_gt"][t] == a
    # the stale rows: a gt row past gt_counts that equals the row's box, with a valid polygon, class > 0 and no crowd
    for k, t in enumerate(lc.GT256_STALE_ROWS):
        stale = n_g + k
        box = lc.row_boxes("gt256", [t])
        assert img["keep_inds"][t] == stale and same_bits(box[0], img["proposals"][k]) and same_bits(box[0], img["gt_boxes"][stale])
        assert img["gt_classes"][stale] > 0 and img["gt_is_crowd"][stale] == 0
        ps = mr.valid_polys(img, stale)
        assert len(ps) == 1 and same_bits(mr.poly_boxes([ps])[0], box[0])
        assert mr.bbox_overlaps(box, mr.poly_boxes([ps]))[0, 0] == 1 > mr.bbox_overlaps(box, pb)[0].max() > 0
        assert 0 <= o["mask_gt"][t] < n_g
    assert set(lc.sample_rows("gt256")[:10]) == set(range(10))                   # the golden keeps the overlaps of those ten rows


def test_points_edges_needs_the_last_point_of_every_polygon():
    img, M, k_min, k_max, Fm = lc.case("points_edges")
    o = lc.want("points_edges")
    n = np.diff(img["poly_ptr"])
    assert tuple(n) == lc.POINT_COUNTS == (3, 63, 64, 65, 128, 129, 255, 256, 257, 513) and int(o["n_mask"]) == 10 and M == 14
    assert o["mask_gt"][:10].tolist() == list(range(10)) and same_bits(img["gt_boxes"], mr.poly_boxes([[lc.points_polygon(k)] for k in range(10)]))
    for k in range(10):
        p = lc.points_polygon(k)
        assert p[-1, 0] > p[:-1, 0].max() and p[-1, 1] > p[:-1, 1].max()         # the last point alone carries the largest x and y
        # without it the poly-box shrinks and the row matches another gt (with 2 points left, gt 0 is no gt any more)
        cut = mr.targets(lc.points_edges(k), M, k_min, k_max, Fm)
        assert cut["mask_gt"][k] != k and cut["mask_gt"][k] >= 0
        # the closing edge toggles pixels: traced alone (as a 2-point loop it is walked twice), and in the mask
        nv = mr.normalise(p, img["gt_boxes"][k], M)
        ev = mr.trace_events(nv[[-1, 0]], M)
        assert len(ev) >= 2 and len(ev) % 2 == 0
        opened = np.zeros(M * M, np.int64)
        for pos in mr.trace_events(nv, M):
            opened[pos] ^= 1
        for pos in ev[:len(ev) // 2]:
            opened[pos] ^= 1                                                     # the polygon's events without the closing edge's
        assert not np.array_equal((np.cumsum(opened) % 2).reshape(M, M).T.reshape(-1), o["masks"][k])
    assert 0 < (o["masks"][:10] == 1).sum() < 10 * M * M and np.all(o["masks"][10:] == -1)


def test_many_polys_runs_38_passes_and_ors_them():
    img, M, _, _, _ = lc.case("many_polys")
    o = lc.want("many_polys")
    assert img["gt_poly_ptr"].tolist() == [0, lc.MANY_POLYS, lc.MANY_POLYS + 1] and M == 28
    n = np.diff(img["poly_ptr"])
    assert n[lc.MANY_TWO_POINT] == 2 and np.isnan(img["poly_xy"][img["poly_ptr"][lc.MANY_NAN]:img["poly_ptr"][lc.MANY_NAN + 1]]).sum() == 1
    ps = mr.valid_polys(img, 0)
    assert len(ps) == 38 and o["mask_gt"][:2].tolist() == [0, 1]
    each = [mr.raster(mr.normalise(p, img["gt_boxes"][0], M), M).reshape(-1) for p in ps]
    assert all(e.any() for e in each)
    assert np.array_equal(np.bitwise_or.reduce(each), o["masks"][0]) and not np.array_equal(np.bitwise_xor.reduce(each), o["masks"][0])
    assert 0 < o["masks"][0].sum() < M * M
    alone = mr.targets(lc.many_polys(True), M, 2, 5, 4)
    assert same_bits(alone["masks"][0], o["masks"][1]) and 0 < o["masks"][1].sum() < M * M


def test_all_m_reaches_every_chunk_size():
    chunk = {M: -(-M * M // lc.BLOCK) for M in lc.ALL_M}
    assert lc.ALL_M == tuple(range(1, 57)) and set(chunk.values()) == set(range(1, 14)) and 16 * 16 == lc.BLOCK and chunk[16] == 1
    assert chunk[17] == 2 and lc.BLOCK - -(-17 * 17 // 2) == 111                 # idle tail threads
    assert sum(1 for M in lc.ALL_M if (M * M) % chunk[M]) >= 20                   # the last owning thread gets a short chunk
    quad = mr.hand_cases()["m28"][0]
    img = lc.all_m()
    assert same_bits(img["poly_xy"][:4], quad["poly_xy"][:4]) and same_bits(img["gt_boxes"][0], quad["gt_boxes"][0])
    assert np.diff(img["gt_poly_ptr"]).tolist() == [1, 3]
    for M in lc.ALL_M:
        o = lc.want("all_m%d" % M)
        assert lc.case("all_m%d" % M)[1:] == (M, 2, 5, 4) and int(o["n_mask"]) == 2 and o["mask_gt"].tolist() == [0, 1, -1, -1]
        assert o["masks"].shape == (4, M * M) and np.all(o["masks"][2:] == -1) and (M < 3 or 0 < o["masks"][0].sum() < M * M)
    for M in (1, 2, 7, 14, 28, 56):
        assert same_bits(lc.want("all_m%d" % M)["masks"][0], mr.targets(*mr.hand_cases()["m%d" % M])["masks"][0])


def test_levels_reach_both_clamps_and_the_single_level_shortcut():
    img, M, k_min, k_max, Fm = lc.case("levels")
    o, single = lc.want("levels"), lc.want("levels_single")
    assert (k_min, k_max) == (0, 15) and lc.case("levels_single")[2:4] == (3, 3) and int(o["n_mask"]) == 8 == len(img["labels"])
    size = o["mask_rois"][:, 3] - o["mask_rois"][:, 1]
    assert size.min() == 2 and size.max() == 4000 * 256
    raw = [mr.fpn_level(r[1:], -100, 100) for r in o["mask_rois"]]
    assert min(raw) < 0 and max(raw) > 15 and o["mask_roi_levels"].tolist() == [min(max(t, 0), 15) for t in raw]
    assert o["mask_roi_levels"].min() == 0 and o["mask_roi_levels"].max() == 15 and len(set(o["mask_roi_levels"].tolist())) >= 6
    assert not single["mask_roi_levels"].any()
    for k in ("mask_rois", "masks", "mask_class", "mask_gt"):
        assert same_bits(o[k], single[k])


def test_batch2_pads_to_common_strides_and_keeps_each_image():
    names = lc.BATCH2
    cs = [lc.case(n) for n in names]
    assert cs[0][1:] == cs[1][1:] == (7, 2, 5, 512)
    batch, padded = mr.stack([c[0] for c in cs], 512)
    assert batch["labels"].shape == (2, 4096) and batch["gt_boxes"].shape == (2, 37, 4) and batch["proposals"].shape == (2, 300, 4)
    for b, name in enumerate(names):
        one, both = lc.want(name), mr.targets(padded[b], 7, 2, 5, 512, b=b)
        R = len(one["roi_has_mask"])
        assert same_bits(both["roi_has_mask"][:R], one["roi_has_mask"]) and not both["roi_has_mask"][R:].any()
        assert np.all(both["mask_rois"][:int(one["n_mask"]), 0] == b) and same_bits(both["mask_rois"][:, 1:], one["mask_rois"][:, 1:])
        for k in ("masks", "mask_class", "mask_roi_levels", "n_mask", "mask_gt"):
            assert same_bits(both[k], one[k]), k


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------
def test_loss_cases_share_workgroups_as_planned():
    from detectorch_amd import hip_mask
    assert lc.LOSS_BLOCKS == hip_mask.LOSS_MAX_BLOCKS and min(lc.LOSS[n][0] for n in lc.MULTI_ROW) > lc.LOSS_BLOCKS > max(mr.LOSS_ROWS)
    count = lambda name: np.bincount(lc.rows_per_workgroup(lc.LOSS[name][0])).tolist()      # [0, one row, two rows, ...]
    assert count("r1025m7k2") == count("r1025m28k3") == [0, 1023, 1] and count("r2047") == [0, 1, 1023] and count("r2048") == [0, 0, 1024]
    assert count("r2049") == [0, 0, 1023, 1] and count("r3077m7k3") == [0, 0, 0, 1019, 5]
    assert set(lc.MULTI_ROW) == {"r1025m7k2", "r2047", "r2048", "r2049", "r3077m7k3", "r1025m28k3"}
    Rm, M, K = lc.LOSS["r3077m7k3"]
    assert K * M * M == 147 and {(r * K * M * M) % 4 for r in range(Rm)} == {0, 1, 2, 3}    # every row at another 16-byte phase
    assert lc.LOSS["r3m56k2"][1] == mr.MAX_M == 56 and -(-56 * 56 // hip_mask.LOSS_BLOCK) == 13
    assert lc.LOSS["r5m55k3"][1] == 55 and (55 * 55) % 2 == 1 and -(-55 * 55 // hip_mask.LOSS_BLOCK) == 12
    for name, (Rm, M, K) in lc.LOSS.items():
        assert Rm * K * M * M * 4 < 10e6, name                                   # the gradient arena stays below 10 MB
        assert (K == hip_mask.MAX_CLASSES == 1024) == (name in lc.FIXED_CLASSES)
    for name, cls in lc.FIXED_CLASSES.items():
        c = lc.loss_case(name)
        assert c["cls"].tolist() == list(cls) and {0, 1023} <= set(cls) and lc.loss_want(name)["n_valid"] >= 2
        for r in (0, 1):                                                         # the last and the first channel carry valid elements
            assert ((c["masks"][r] == 0) | (c["masks"][r] == 1)).any()


@pytest.mark.parametrize("case", lc.MULTI_ROW)
def test_loss_rows_that_share_a_workgroup(case):
    c = lc.loss_case(case, extremes=True)
    pairs = lc.shared_pairs(c)
    ignored = ("neg", "K", "pad")
    if case in lc.PLANTED_SINGLE:
        assert pairs == {lc.PLANTED_SINGLE[case]}
    else:
        assert set(lc.PLANTED.values()) <= pairs
        for kind in ignored:                                                     # valid first and ignored second, and the reverse
            assert ("valid", kind) in pairs and (kind, "valid") in pairs
        assert any(a == "ext" and b in ignored for a, b in pairs) and any(b == "ext" and a in ignored for a, b in pairs)
        for x, kinds in lc.PLANTED.items():
            assert (lc.row_kind(c, x), lc.row_kind(c, x + lc.LOSS_BLOCKS)) == kinds and x % lc.LOSS_BLOCKS == (x + lc.LOSS_BLOCKS) % lc.LOSS_BLOCKS
    plain = lc.loss_case(case)
    assert "ext" not in {k for p in lc.shared_pairs(plain) for k in p} and same_bits(plain["cls"], c["cls"])
    y, yx = lc.loss_want(case), lc.loss_want(case, True)
    assert y["scale"] < 20 and yx["scale"] > 1e38 and y["n_valid"] > 40000
    assert np.isfinite(yx["loss"]) and np.isfinite(yx["grad"]).all()


def test_single_shared_workgroups_cover_both_orders():
    a, b = lc.PLANTED_SINGLE["r1025m7k2"], lc.PLANTED_SINGLE["r1025m28k3"]
    assert a[0] == "ext" and a[1] in ("neg", "K", "pad") and b[1] == "ext" and b[0] in ("neg", "K", "pad")


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", lc.ALL_M)
def test_rect_fifth_scaled_to_every_m(M):
    """the rectangle of `rect_fifth` (corners 12, 16, 49, 103 on the 5x grid at M = 28) scaled to M and rounded onto the 5x grid"""
    xs, ys, xe, ye = (int(round(v * M / 28.0)) for v in (12, 16, 49, 103))
    poly = mr.rect(xs / 5.0, ys / 5.0, xe / 5.0, ye / 5.0).astype(np.float64)
    assert [int(5 * v + 0.5) for v in poly[:, 0]] == [xs, xe, xe, xs] and [int(5 * v + 0.5) for v in poly[:, 1]] == [ys, ys, ye, ye]
    want = rect_answer(xs, ys, xe, ye, M)
    assert np.array_equal(mr.raster(poly, M), want) and np.array_equal(mr.raster(poly[::-1], M), want)
    if M == 28:
        assert want.sum() == 8 * 18
    assert M < 3 or 0 < want.sum() < M * M


def test_kernel_event_form_equals_the_trace_on_the_new_polygons():
    polys = []
    img = lc.case("points_edges")[0]
    for k in range(10):
        polys.append((mr.normalise(lc.points_polygon(k), img["gt_boxes"][k], 14), 14))
    img = lc.case("many_polys")[0]
    polys += [(mr.normalise(p, img["gt_boxes"][0], 28), 28) for p in mr.valid_polys(img, 0)]
    img = lc.all_m()
    for M in lc.ALL_M:
        polys += [(mr.normalise(p, img["gt_boxes"][q], M), M) for q in (0, 1) for p in mr.valid_polys(img, q)]
    img = lc.case("levels")[0]
    polys += [(mr.normalise(mr.valid_polys(img, 0)[0], b, 7), 7) for b in img["proposals"]]
    for p, M in polys:
        assert sorted(mr.kernel_events(p, M)) == sorted(mr.trace_events(p, M))
