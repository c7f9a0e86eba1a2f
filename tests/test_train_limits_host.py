"""The cases of tests/train_limit_cases.py without a GPU:
  * the numpy restatement (tests/train_targets_ref.py) against the reference's own chain on every recorded case
    (tests/golden/train_targets_limits.npz, made by tests/golden/make_train_limits_golden.py): everything but dw / dh bit for bit
    (through the fixture's digests, and its arrays where it holds them), dw / dh within the fixture's e_ref of
    w * log(float64(ratio)); the seeded inputs and parameter sets by digest;
  * what keeps tests/test_hip_train_limits.py from passing emptily, asserted on the restatement alone: every case reaches the
    branch, the pattern or the boundary its row in the table of tests/README.md names."""
import numpy as np
import pytest

from conftest import golden
import train_limit_cases as tl
import train_targets_ref as tr


@pytest.fixture(scope="module")
def g():
    return dict(golden("train_targets_limits"))


def _groups(cid):
    """(fg mask, bg mask) of a case's candidates"""
    _, p = tl.case(cid)
    mo = tl.want(cid)["max_overlaps"]
    return mo >= np.float32(p["fg_thresh"]), (mo < np.float32(p["bg_thresh_hi"])) & (mo >= np.float32(p["bg_thresh_lo"]))


def test_the_table_is_recorded(g):
    assert set(tl.RECORDED) | set(tl.REFERENCE_RAISES) == set(tl.CASES) and tl.REFERENCE_RAISES == ("classes_1204",)
    assert sorted(k[:-4] for k in g if k.endswith("_sha")) == sorted(tl.RECORDED)
    assert 2.0 < float(g["e_ref"]) < 4.0                                     # the reference's np.log: a few float32 ulps


@pytest.mark.parametrize("cid", tl.RECORDED)
def test_restatement_equals_reference(g, cid):
    im, params = tl.case(cid)
    assert tr.same_bits(tl.input_digest(cid), tl.fixture_sha(g, cid, "inputs"))
    m = tl.want(cid)
    keep, labels = g[cid + "_kept"]
    assert tr.same_bits(m["keep_inds"], keep) and m["n_fg"] == int(g[cid + "_n_fg"]) and tr.same_bits(m["labels"], labels)
    assert tr.same_bits(tl.assign_digest(m["max_overlaps"], m["max_classes"], m["targets5"]), tl.fixture_sha(g, cid, "assign"))
    assert tr.same_bits(tl.sha(m["max_overlaps"], m["max_classes"]), tl.fixture_sha(g, cid, "overlap"))
    assert tr.same_bits(tl.kept_digest(m["rois"], m["bbox_targets5"]), tl.fixture_sha(g, cid, "kept"))
    e_ref = float(g["e_ref"])
    assert tr.ulps_from(m["targets5"][:, 3:], m["want64"]).max(initial=0.0) <= e_ref
    if cid + "_rois" in g:
        assert tr.same_bits(m["max_overlaps"], g[cid + "_max_overlaps"]) and tr.same_bits(m["max_classes"], g[cid + "_max_classes"])
        assert tr.same_bits(m["rois"], g[cid + "_rois"])
        want5 = g[cid + "_targets5"]
        assert tr.same_bits(m["targets5"][:, :3], want5[:, :3])
        assert tr.ulps_from(want5[:, 3:], m["want64"]).max(initial=0.0) <= e_ref
    if cid in tl.EXPANDED_IDS:
        bt, want = m["bbox_targets"], g[cid + "_bbox_targets"]
        assert bt.shape == want.shape == (len(keep), 8 if params["cls_agnostic_bbox_reg"] else 4 * params["num_classes"])
        dwdh = np.zeros(bt.shape, bool)
        dwdh[:, 2::4] = dwdh[:, 3::4] = True
        assert tr.same_bits(np.where(dwdh, 0, bt), np.where(dwdh, 0, want)) and np.array_equal(bt != 0, want != 0)
        assert tr.same_bits(m["bbox_inside_weights"], g[cid + "_bbox_inside_weights"])
        assert tr.same_bits(m["bbox_outside_weights"], g[cid + "_bbox_outside_weights"])


def test_inputs_stay_inside_the_contract():
    for cid in tl.CASES:
        im, p = tl.case(cid)
        for k in ("gt_boxes", "proposals"):
            b = im[k]
            assert b.dtype == np.float32 and np.all(np.isfinite(b)) and np.all(b[:, 2] >= b[:, 0]) and np.all(b[:, 3] >= b[:, 1]), cid
        assert np.all(im["gt_classes"] > 0) and np.all(im["gt_classes"] < p["num_classes"]), cid
        assert len(im["gt_boxes"]) <= 256 and len(im["proposals"]) <= 2048 and im["rand_keys"].dtype == np.uint32
        assert len(im["rand_keys"]) == len(im["gt_boxes"]) + len(im["proposals"]) >= 1


def test_every_sweep_image_reaches_its_key_count_and_branch():
    assert [sum(tl.SWEEP[n]) for n in tl.SWEEP] == [1, 1, 2, 3, 4, 64, 65, 128, 129, 255, 256, 257, 512, 513, 1024, 1025, 2048, 2049,
                                                    2304]
    reached = set()
    for n, (G, n_prop) in tl.SWEEP.items():
        im = tl.image(n)
        assert (len(im["gt_boxes"]), len(im["proposals"])) == (G, n_prop) and G <= 256 and n_prop <= 2048
        np2 = tl.next_pow2(G + n_prop)
        assert (np2, tl.sort_branch(np2)) == tl.SWEEP_REACHES[n], n
        reached.add((np2, tl.sort_branch(np2)))
        fg, bg = _groups("sweep_" + n)
        assert (int(fg.sum() + bg.sum()) == np2) == (n in tl.SWEEP_FULL), n   # a full list: every one of the np2 keys a candidate's
        if G + n_prop >= 3:
            assert fg.any() and bg.any(), n
    # 2 ... 4096 keys, the merge sort from its first size to its last, the network on both sides of it
    assert reached == {(2, "regs1"), (4, "regs1"), (64, "regs1"), (128, "regs1"), (256, "merge"), (512, "merge"), (1024, "merge"),
                       (2048, "regs2"), (4096, "regs4")}
    assert {"n256", "n1024", "n2048"} <= set(tl.SWEEP_FULL)
    assert tl.sort_branch(128) == "regs1" and tl.sort_branch(2048) == "regs2" and [tl.next_pow2(n) for n in (0, 1, 2, 3)] == [2, 2, 2, 4]


@pytest.mark.parametrize("name", sorted(tl.GROUPS))
def test_every_group_boundary_image_has_its_pattern(name):
    fg, bg = _groups("group_" + name)
    n_pad = tl.next_pow2(len(fg)) - int(fg.sum()) - int(bg.sum())
    assert (bool(fg.any()), bool(bg.any()), n_pad > 0) == tl.GROUPS[name]
    assert not np.any(fg & bg)
    w = tl.want("group_" + name)
    if name == "neither":                                                    # candidates present, none sampled: every row padding
        assert len(fg) == 7 and w["n_rois"] == 0 and w["n_fg"] == 0
    else:
        assert w["n_rois"] == int(fg.sum() + bg.sum()) and w["n_fg"] == int(fg.sum())


def _assigned(im, w):
    """per kept row: the ORIGINAL index of the gt its targets were computed against (roidb.py:193-195), -1 without targets"""
    boxes = np.vstack([im["gt_boxes"], im["proposals"]])
    real = np.where(im["is_crowd"] == 0)[0]
    ov = tr.bbox_overlaps(boxes[w["keep_inds"]], im["gt_boxes"][real])
    return np.where(w["max_overlaps"][w["keep_inds"]] >= np.float32(0.5), real[ov.argmax(axis=1)], -1), ov


def test_many_gt_image_visits_every_lane_more_than_once():
    im, p = tl.case("many_gt")
    w = tl.want("many_gt")
    assert len(im["gt_boxes"]) == 200 and p == tr.DEFAULTS
    a, ov = _assigned(im, w)
    assert np.sum(a >= 64) >= 20 and np.sum(a >= 128) >= 10
    real = np.where(im["is_crowd"] == 0)[0]
    for lo, hi in tl.DUP_SAME_LANE + tl.DUP_OTHER_LANE:
        assert tr.same_bits(im["gt_boxes"][lo], im["gt_boxes"][hi]) and ((hi - lo) % 64 == 0) == ((lo, hi) in tl.DUP_SAME_LANE)
        rows = np.where(a == lo)[0]                                          # the first of the pair is the assigned one ...
        assert len(rows) >= 1 and not np.any(a == hi)
        col_lo, col_hi = list(real).index(lo), list(real).index(hi)
        assert np.all(ov[rows, col_lo] == ov[rows, col_hi]) and np.all(ov[rows, col_lo] == ov[rows].max(axis=1))   # ... on an exact tie
    # kept rows whose largest IoU is with a crowd gt: labelled with its class, targets against the best non-crowd gt
    boxes = np.vstack([im["gt_boxes"], im["proposals"]])
    crowd = np.array(tl.MANY_CROWD)
    assert np.all(im["is_crowd"][crowd] == 1) and im["is_crowd"].sum() == 2
    ovc = tr.bbox_overlaps(boxes[w["keep_inds"]], im["gt_boxes"][crowd]).max(axis=1)
    out = (w["keep_inds"] >= 200) & (ovc > ov.max(axis=1)) & (w["max_overlaps"][w["keep_inds"]] == ovc) & (w["bbox_targets5"][:, 0] > 0)
    assert out.sum() >= 4 and np.all(a[out] >= 0)
    # case h, recorded here too: lanes that visit four gt
    wh = tl.want("many_gt_h")
    ah, _ = _assigned(tl.image("h"), wh)
    assert np.sum(ah >= 64) >= 20 and np.sum(ah >= 128) >= 10 and np.sum(ah >= 192) >= 10


def test_bbox_thresh_at_and_below_zero_hands_out_deltas():
    w = tl.want("thresh_bbox0")
    t5 = w["bbox_targets5"]
    zero_class = (t5[:, 0] == 0) & np.all(t5[:, 1:3] != 0, axis=1)
    assert zero_class.sum() >= 20 and np.all(w["labels"][zero_class] == 0)
    wa = tl.want("thresh_bbox0_agnostic")                                   # class-agnostic: the same rows carry class 1 and a slot
    assert np.all(wa["bbox_targets5"][:, 0] == 1) and np.all(wa["bbox_inside_weights"][:, 4:] == 1)
    im, _ = tl.case("thresh_bbox_m1")
    wm = tl.want("thresh_bbox_m1")
    crowd_rows = np.where(im["is_crowd"] == 1)[0]
    kept_crowd = np.isin(wm["keep_inds"], crowd_rows)
    assert kept_crowd.sum() >= 1 and np.all(wm["bbox_targets5"][kept_crowd][:, 1:3] != 0)
    assert np.all(wm["bbox_targets5"][kept_crowd][:, 0] == 0) and np.all(wm["labels"][kept_crowd] == 0)
    filtered = wm["max_overlaps"][wm["keep_inds"]] == -1                     # ... and crowd-filtered proposals as background rows
    wl = tl.want("thresh_bg_lo_m1")                                          # at the default bbox_thresh they carry none
    neg = wl["max_overlaps"][wl["keep_inds"]] == -1
    assert filtered.sum() >= 3 and neg.sum() >= 3 and not wl["bbox_targets5"][neg].any() and np.all(wl["labels"][neg] == 0)


def test_threshold_cases_sit_on_their_comparisons():
    w = tl.want("thresh_ties")
    mo = w["max_overlaps"]
    for v in (0.125, 0.25, 0.375, 0.5, 1.0):                                 # exact: the IoU are quotients that float32 holds
        assert np.any(mo[3:] == np.float32(v)), v
    fg, bg = _groups("thresh_ties")
    assert np.all(bg[mo == np.float32(0.125)]) and not np.any(bg[mo == np.float32(0.25)]) and not np.any(fg[mo == np.float32(0.25)])
    assert np.all(fg[mo == np.float32(0.5)])
    at = np.where(mo == np.float32(0.375))[0]
    assert np.all(w["targets5"][at, 0] > 0) and not np.any(w["targets5"][(mo > 0) & (mo < np.float32(0.375)), 0] > 0)
    # the thresholds float32 does not hold: the comparison is made in float32 (a float64 comparison would differ on no row only
    # if no overlap fell between the two roundings; what is pinned is the parameter's one rounding)
    p = tl.THRESHOLDS["not_float32"]
    assert all(float(np.float32(p[k])) != p[k] for k in ("fg_thresh", "bg_thresh_hi", "bg_thresh_lo", "bbox_thresh"))
    w0, w1 = tl.want("thresh_fg_bg_0"), tl.want("thresh_fg_bg_1")
    assert w0["n_fg"] == 16 and w0["n_rois"] == 16 and np.any(w0["max_overlaps"][w0["keep_inds"]] == 0)       # overlap 0 is fg at 0
    assert w1["n_fg"] < 16 and np.all(w1["max_overlaps"][w1["keep_inds"][:w1["n_fg"]]] == 1) and w1["n_rois"] == 64
    assert np.any(w1["keep_inds"][:w1["n_fg"]] >= 6)                         # an exact copy of a gt among them


@pytest.mark.parametrize("R,f", tl.QUOTA_HALVES)
def test_quota_cases_show_the_rounding(R, f):
    x = f * R
    assert x - np.floor(x) == 0.5
    cid = "quota_R%d_f%s" % (R, f)
    fg, _ = _groups(cid)
    assert fg.sum() > np.ceil(x)                                             # more fg candidates than either rounding
    assert tl.want(cid)["n_fg"] == int(np.round(x)) == int(2 * round(x / 2))  # half to even


def test_quota_halves_tell_the_roundings_apart():
    differ = [(R, f) for R, f in tl.QUOTA_HALVES if int(np.floor(f * R + 0.5)) != int(np.round(f * R))]
    assert differ == [(1, 0.5), (2, 0.25), (10, 0.25), (17, 0.5)]
    w = tl.want("quota_R4096_f0.25_nc3")
    assert w["n_rois"] < 2304 and 4096 - w["n_rois"] >= 1792 and w["n_fg"] == 1024
    assert tl.want("quota_R4095_f0.5")["n_rois"] < 4095 and tl.want("quota_R17_f0.25")["n_rois"] == 17


@pytest.mark.parametrize("pattern", tl.KEY_PATTERNS)
def test_key_patterns_decide_the_sample(pattern):
    cid = "keys_" + pattern
    im, p = tl.case(cid)
    keys, w = im["rand_keys"], tl.want(cid)
    fg, bg = _groups(cid)
    fg_i, bg_i = np.where(fg)[0], np.where(bg)[0]
    nf = w["n_fg"]
    trunc = np.r_[tl.truncated_shift_order(fg_i, keys)[:nf], tl.truncated_shift_order(bg_i, keys)[:64 - nf]]
    if pattern in ("top_bits", "negative_int32"):
        # bits 20 ... 31 of the key decide: a shift by 12 inside 32 bits gives another sample
        assert not np.array_equal(trunc, w["keep_inds"])
        assert len(set((keys >> 20).tolist())) >= 7
    else:
        # keys below 2^20, or all equal: the truncated shift keeps the order; these pin the index tie-break (zeros, ones), the
        # all-ones key next to the pad key (ones) and the key's low bits against the index bits below them (low_bits)
        assert np.array_equal(trunc, w["keep_inds"])
        if pattern == "low_bits":
            assert set(keys.tolist()) == {0, 1, 2, 3, 4} and not np.array_equal(w["keep_inds"][:nf], fg_i[:nf])
        else:
            assert len(set(keys.tolist())) == 1 and np.array_equal(w["keep_inds"], np.r_[fg_i[:nf], bg_i[:64 - nf]])
    if pattern == "negative_int32":                                          # ... and a signed comparison another one
        signed = keys.view(np.int32).astype(np.int64)
        s = np.r_[fg_i[np.lexsort((fg_i, signed[fg_i]))][:nf], bg_i[np.lexsort((bg_i, signed[bg_i]))][:64 - nf]]
        assert np.sum(keys >= 2 ** 31) > 100 and not np.array_equal(s, w["keep_inds"])


@pytest.mark.parametrize("thresh", tl.CROWD_THRESH)
def test_crowd_threshold_cases_sit_on_the_threshold(thresh):
    im, p = tl.case("crowd_%s" % thresh)
    assert p["crowd_thresh"] == thresh and im["is_crowd"].tolist() == [1, 1, 0]
    ioa = tr.bb_iou_crowd(tr.xyxy_to_xywh(im["proposals"]), tr.xyxy_to_xywh(im["gt_boxes"][:2])).max(axis=1)
    assert np.sum(ioa == 1.0) >= 4 and np.sum(ioa == 0.5) == 1 and np.sum(ioa == 0.25) == 1 and np.sum(ioa == 0.05) == 1
    mo = tl.want("crowd_%s" % thresh)["max_overlaps"][3:]
    if thresh == 1e-9:
        assert np.any((ioa > 0) & (ioa <= 0.05)) and np.all(mo[ioa > 0] == -1) and np.all(mo[ioa == 0] >= 0)
    else:
        assert np.any(ioa == thresh)                                         # a proposal exactly at the threshold: not filtered (>)
        assert np.all(mo[ioa == thresh] >= 0)
        assert np.array_equal(mo == -1, (ioa > thresh) if thresh > 0 else np.zeros(len(ioa), bool))
    if thresh == 0.5:
        assert np.sum(mo == -1) >= 4


def test_weights_and_class_counts_reach_what_they_name():
    for cid in ("weights_odd", "weights_mixed"):
        ws = tl.case(cid)[1]["reg_weights"]
        assert len(set(ws)) == 4
    assert any(float(np.float32(v)) != v for v in tl.case("weights_odd")[1]["reg_weights"])
    for c in (2, 3, 64, 65, 1204):
        im, p = tl.case("classes_%d" % c)
        w = tl.want("classes_%d" % c)
        assert p["num_classes"] == c and im["gt_classes"].max() == c - 1 and w["bbox_targets"].shape[1] == 4 * c
        assert np.any(w["bbox_targets5"][:, 0] == c - 1)                      # the last slot of the expanded row is written
    # expansion rows narrower than, equal to and wider than a wavefront's 64 float4 slots
    assert 3 < 64 and 65 > 64 and tl.case("classes_1204")[1]["rois_per_image"] == 8


def test_small_images_fit_the_batch_strides():
    for n in tl.SMALL_IMAGES:
        im = tl.image(n)
        assert len(im["gt_boxes"]) <= 8 and len(im["proposals"]) <= 320
    assert len(tl.SMALL_IMAGES) == 11 and 300 % len(tl.SMALL_IMAGES) != 0
