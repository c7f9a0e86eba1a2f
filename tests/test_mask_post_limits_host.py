"""The limit cases of the mask post-processing library without a GPU and without the library (the "Limits" section of
tests/README_mask_post.md): every case of tests/mask_post_limit_cases.py holds the condition it is named for, the additions to the
restatement (trunc_box, vote_sparse) are pinned against what was there, and the cases tell the mutants of the README's table that
the restatement can state from the contract."""
import numpy as np
import pytest

import mask_post_cases as mc
import mask_post_limit_cases as lc
import mask_post_ref as mr
import segm_eval_ref as sr

P30 = 1 << 30


def ends_of(case, n, k):
    return mr.clipped_ends(case["all_runs"][n, k], case["all_n_runs"][n, k], sr.pixels(case["im_size"][n]))


def pixels_of(case, n, k, lo, hi):
    """the set positions of voter k inside [lo, hi)"""
    pos = np.arange(lo, hi)
    return pos[mr.on_at(ends_of(case, n, k), pos)]


def voters(case, ovr, n, t):
    with np.errstate(invalid='ignore'):
        return np.flatnonzero(ovr[n, t, :mr.clamp(case["all_count"][n], case["all_n_runs"].shape[1])] >= case["iou_thresh"])


def differs(a, b):
    return a["lists"] != b["lists"] or not np.array_equal(a["need"], b["need"])


def same(a, b):
    return a["lists"] == b["lists"] and all(np.array_equal(a[k], b[k]) for k in ("need", "out_n_runs", "copied"))


# ---- the additions to the restatement ------------------------------------------------------------------------------------------------------
def test_trunc_box_is_the_headers_cast_and_not_numpys():
    nan = np.nan
    got = mr.trunc_box(np.array([2.9, -2.9, -0.5, 0.99, nan, P30, -P30, 7.0, -0.0], np.float32))
    assert got.dtype == np.int32 and got.tolist() == [2, -2, 0, 0, 0, P30, -P30, 7, 0]
    with np.errstate(invalid='ignore'):
        own = np.array([nan], np.float32).astype(np.int32)      # C leaves it undefined, numpy to the platform: here -2^31
    assert own.tolist() == [-2 ** 31] and mr.trunc_box(np.array([nan], np.float32), nan_to=-2 ** 31).tolist() == own.tolist()
    rs = np.random.RandomState(0)
    v = (rs.rand(1000) * 200 - 100).astype(np.float32)          # on numbers the two casts are one
    assert np.array_equal(mr.trunc_box(v), v.astype(np.int32))


@pytest.mark.parametrize("name", ["tiny", "order", "chunks", "large"])
def test_vote_sparse_is_vote_on_the_existing_cases(name):
    case = mc.VOTE_CASES[name]()
    ovr = mc.real_ovr(case)
    for method in ("AVG", "UNION"):
        assert same(mr.vote_sparse(case, ovr, method, lc.full_windows(case)), mr.vote(case, ovr, method)), method
    if name == "large":                                         # windows: the columns the blobs lie in, not the image
        lo, hi = 700 * 800, 1100 * 800
        assert same(mr.vote_sparse(case, ovr, "AVG", [[(lo, hi)]]), mr.vote(case, ovr, "AVG"))
        with pytest.raises(AssertionError, match="outside the windows"):
            mr.vote_sparse(case, ovr, "AVG", [[(lo, lo + 4000)]])


def test_vote_sparse_is_vote_on_the_threshold_case():
    case, ovr = mc.threshold_vote()
    for bt in (0.5, np.nextafter(0.5, 0)):
        c = dict(case, binarize_thresh=bt)
        assert same(mr.vote_sparse(c, ovr, "AVG", lc.full_windows(c)), mr.vote(c, ovr, "AVG"))
    with pytest.raises(AssertionError, match="negative threshold"):
        mr.vote_sparse(dict(case, binarize_thresh=-0.1), ovr, "AVG", lc.full_windows(case))


@pytest.mark.parametrize("name", ["many_voters", "encoder_edges", "nan_box", "max_stride"])
def test_vote_sparse_is_vote_on_the_new_cases_small_enough_to_decode(name):
    case, ovr = lc.VOTE_LIMIT_CASES[name]()
    for method in ("AVG", "UNION"):
        assert same(lc.voted(name, method), mr.vote(case, ovr, method)), method


def test_vote_sparse_is_vote_on_the_small_images_of_im_size_rules():
    case, ovr = lc.im_size_rules()
    small = [0, 1, 2, 4, 5, 6]                                   # image 3 is 2^30 x 1; image 4 is refused before anything is decoded
    sub = {k: (v[small] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    for method in ("AVG", "UNION"):
        got, want = lc.voted("im_size_rules", method), mr.vote(sub, ovr[small], method)
        assert [got["lists"][n] for n in small] == want["lists"]
        assert all(np.array_equal(got[k][small], want[k]) for k in ("need", "out_n_runs", "copied"))


# ---- every case holds its condition --------------------------------------------------------------------------------------------------------------
def test_many_voters_holds_its_conditions():
    case, ovr = lc.many_voters()
    assert case["all_count"].tolist() == [512] and case["all_n_runs"].shape == (1, 512) and sr.pixels(case["im_size"][0]) == 768
    assert len(voters(case, ovr, 0, 0)) == 512 and voters(case, ovr, 0, 1).tolist() == lc.MANY_TOP1 and len(lc.MANY_TOP1) == 257
    has = lambda k, c: len(pixels_of(case, 0, k, 256 * c, 256 * c + 256)) > 0
    assert all(has(k, 0) for k in range(512)) and pixels_of(case, 0, 0, 0, 1).tolist() == [0]          # the walk starts at 0
    assert [k for k in range(512) if has(k, 1)] == [k for k in range(260, 512, 4) if k != 300] + [511]
    assert [k for k in range(512) if has(k, 2)] == [300, 511]
    only_511 = set(pixels_of(case, 0, 511, 512, 768)) - set(pixels_of(case, 0, 300, 512, 768))
    for method in ("AVG", "UNION"):
        lists = lc.voted("many_voters", method)["lists"][0]
        on = [mr.on_at(np.cumsum(l), np.arange(768)) for l in lists]
        # top 0: pixels in chunk 1 (only voters past the first 256 are there) and in chunk 0 from the first 256 voters alone
        assert on[0][256:512].any() and on[0][512:].any() and on[0][:256].any()
        # top 1: its chunks 1 and 2 hang on the voters at list places 255 and 256; some pixels on the one at place 256 alone
        assert on[1][256:512].any() and any(on[1][p] for p in only_511)
    low = {int(p) for k in range(256) for p in pixels_of(case, 0, k, 0, 256)} - {int(p) for k in range(256, 512) for p in pixels_of(case, 0, k, 0, 256)}
    assert any(mr.on_at(np.cumsum(lc.voted("many_voters", "UNION")["lists"][0][0]), np.array(sorted(low))))    # gone when the list starts over
    assert differs(lc.voted("many_voters", "AVG"), lc.voted("many_voters", "UNION"))


def test_negative_threshold_chunks_holds_its_conditions():
    case, ovr = lc.negative_threshold_chunks()
    assert [len(voters(case, ovr, 0, t)) for t in range(6)] == list(lc.NEG_VOTERS) and all(5 <= v <= 10 for v in lc.NEG_VOTERS)
    assert case["top_count"].tolist() == [6] and case["top_n_runs"].shape[1] <= 8 and sr.pixels(case["im_size"][0]) == 5 * 256
    scores = case["all_dets"][0, :12, 4]
    assert np.isnan(scores[1]) and np.isposinf(scores[2])
    for t in (0, 1):                                            # no voter of tops 0 and 1 in chunks 3 and 4
        assert not any(len(pixels_of(case, 0, k, 768, 1280)) for k in voters(case, ovr, 0, t))
    want = lc.voted("negative_threshold_chunks", "AVG")
    skipped = mr.vote(case, ovr, "AVG", "skip_chunks")
    assert want["lists"][0][0] != skipped["lists"][0][0] and want["lists"][0][1] != skipped["lists"][0][1]
    # the NaN score: off inside the support of voter 1, on outside it, where no voter has a pixel
    h, w = 32, 40
    top = mr.bitmap(np.array(want["lists"][0][1], np.uint32), 999, h, w)
    b = mr.trunc_box(case["all_dets"][0, 1, :4]).tolist()
    inside = np.zeros((h, w), bool)
    inside[max(b[1], 0):min(b[3] + 1, h), max(b[0], 0):min(b[2] + 1, w)] = True
    assert inside.any() and not top[inside].any() and top[:, 32:].all() and not inside[:, 32:].any()
    zero, minus = lc.voted("negative_threshold_chunks", "AVG", 0.0), lc.voted("negative_threshold_chunks", "AVG", -0.0)
    assert same(zero, minus) and differs(zero, want)


def test_encoder_edges_holds_its_conditions():
    case, ovr = lc.encoder_edges()
    avg = lc.voted("encoder_edges", "AVG")
    lists, need, out_n = avg["lists"][0], avg["need"][0], avg["out_n_runs"][0]
    assert case["out_stride"] == 257 and sr.pixels(case["im_size"][0]) == 4 * 256
    assert pixels_of(case, 0, 0, 0, 1024).tolist() == [0, 1023]                                  # every walk covers [0, h w)
    assert lists[0] == [0] + [1] * 255 + [769] and need[0] == out_n[0] == 257                    # 256 starts in chunk 0, fits exactly
    assert need[1] == 258 and out_n[1] == -1 and lists[1] is None                                # one more start
    assert lists[2] == [256, 256, 512] and not any(len(pixels_of(case, 0, k, 512, 768)) for k in voters(case, ovr, 0, 2))
    assert lists[3] == [1020, 4] and lists[4] == [0, 5, 1019]
    assert avg["copied"][0].tolist() == [False] * 5 + [True, False] and need[5] == 300 and out_n[5] == -1 and len(voters(case, ovr, 0, 5)) == 1
    uni = lc.voted("encoder_edges", "UNION")
    assert uni["lists"][0][3] == [0, 1, 1019, 4] and uni["need"][0, 0] == 258                    # the weak voter's pixels count in a union


def test_jumps_holds_its_conditions():
    case, ovr = lc.jumps()
    hw = sr.pixels(case["im_size"][0])
    assert hw == P30 and mr.sides(case["im_size"][0]) == (32768, 32768)
    ends = [ends_of(case, 0, k) for k in range(4)]
    ones = [mr.one_runs(e) for e in ends]
    in_a = lambda s, t: lc.CA - 1500 <= s and t <= lc.CA + 1500
    for s, t in zip(np.concatenate([o[0] for o in ones]), np.concatenate([o[1] for o in ones])):
        assert in_a(s, t) or lc.SB <= s, (s, t)                                                  # two clusters, nothing in between
        assert t <= lc.P0 + 8 or s >= lc.P0 + 300 or s >= lc.SB                                  # the hole
    assert any(s < lc.CA < t for s, t in zip(*[np.concatenate(x) for x in zip(*ones)]))          # a one-run across the column boundary
    assert ones[0][1][-1] == hw and ones[0][0][ones[0][0] >= lc.SB].min() == lc.SB               # voter 0: the last pixel; B starts at SB
    assert ends[1][-1] == lc.CA + 1200 < hw and len(ends[1]) % 2 == 0                            # voter 1 stops short, on a one-run
    raw = case["all_runs"][0, 2, :128].astype(np.int64)
    assert case["all_n_runs"][0, 2] == 128 and raw[:64].sum() > 1 << 32 and raw[:62].sum() < hw and (ends[2][62:] == hw).all()
    assert ones[2][0].tolist() == [lc.P0] and ones[2][1].tolist() == [lc.P0 + 7]
    wrapped = raw[:64].sum() % (1 << 32)                                                         # carried in 32 bits the tail lands in the hole
    assert lc.P0 + 8 <= wrapped + raw[64] and wrapped + raw[64:].sum() < lc.P0 + 300
    e3 = np.concatenate([[0], ends[3]])
    zero_len = [j for j in range(1, len(ends[3]), 2) if e3[j] == e3[j + 1] == lc.SB]
    assert len(zero_len) == 2                                                                    # voter 3: zero-length one-runs at SB
    after_a = max(t for o in ones for s, t in zip(*o) if t <= lc.CA + 1500)
    landing = min(int(e[np.searchsorted(e, after_a + 256, side='right')]) for e in (ends[0], ends[3]))
    assert landing == lc.SB                                                                      # where the jump over the gap lands
    win = sum(t - s for s, t in lc.JUMP_WINDOWS[0])
    assert win < 1 << 22
    avg, uni = lc.voted("jumps", "AVG"), lc.voted("jumps", "UNION")
    assert [len(voters(case, ovr, 0, t)) for t in range(4)] == [4, 2, 3, 1] and avg["copied"][0, 3] and not avg["copied"][0, :3].any()
    assert differs(avg, uni) and all(sum(l) == hw for l in avg["lists"][0][:3] + uni["lists"][0][:3])
    assert len(uni["lists"][0][0]) % 2 == 0                                                      # the closing run is ones
    b = mr.trunc_box(case["all_dets"][0, 2, :4]).tolist()
    assert b == [-P30, -P30, P30, P30]
    # the same lists through boxes and overlaps: the interval forms
    boxes = lc.interval_boxes(case["all_runs"], case["all_n_runs"], case["all_count"], case["im_size"])
    assert boxes["boxes"][0, 0].tolist() == [15258, 0, 32767, 32767] and boxes["boxes"][0, 2].tolist() == [15258, 32768 - 1000, 15258, 32768 - 994]
    assert boxes["area"][0, 2] == 7


def test_max_stride_holds_its_conditions():
    case, ovr = lc.max_stride()
    S = 1 << 20
    assert case["all_runs"].shape == (1, 4, S) and case["top_runs"].shape == (1, 3, S) and case["out_stride"] == S
    assert case["all_n_runs"][0, :3].tolist() == [S] * 3 and case["all_runs"][0, 1, 0] == 0 and (case["all_runs"][0, 0] == 1).all()
    avg, uni = lc.voted("max_stride", "AVG"), lc.voted("max_stride", "UNION")
    assert avg["need"][0].tolist() == [S, S + 1, S] and avg["out_n_runs"][0].tolist() == [S, -1, S] and avg["copied"][0].tolist() == [False, False, True]
    assert avg["lists"][0][0] == [1] * S and uni["lists"][0][:2] == [[0, S], [0, S]]
    for k, (box, area) in enumerate(lc.MAX_STRIDE_BOXES[:2] + lc.MAX_STRIDE_BOXES[3:]):          # the answers by hand against the intervals
        k = k if k < 2 else 3
        assert mr.interval_box(case["all_runs"][0, k], case["all_n_runs"][0, k], 1024, 1024) == (box, area)
    for crowd in (False, True):
        by_hand = lc.max_stride_pairs(crowd)
        for i, j in ((0, 3), (3, 1), (0, 1)):
            k, aa, ab = sr.interval_counts(case["all_runs"][0, i], case["all_n_runs"][0, i], case["all_runs"][0, j], case["all_n_runs"][0, j], S)
            assert by_hand["ovr"][0, i, j] == (0.0 if k == 0 else np.float64(k) / np.float64(aa if crowd else aa + ab - k))
            assert (by_hand["a_area"][0, i], by_hand["b_area"][0, j]) == (aa, ab)


def test_nan_box_holds_its_conditions():
    case, ovr = lc.nan_box()
    d = case["all_dets"][0, :9, :4]
    assert [np.flatnonzero(np.isnan(r)).tolist() for r in d[:4]] == [[0], [1], [2], [3]] and np.abs(d[4:7]).max() == P30
    assert mr.trunc_box(d[4]).tolist() == [-P30, -P30, P30, P30]
    want = lc.voted("nan_box", "AVG")
    numpys = mr.vote(case, ovr, "AVG", "nan_int_min")
    assert differs(want, numpys) and want["lists"][0][3] != numpys["lists"][0][3]
    wp, wn = mr.weight_planes(case["all_dets"][0, :9], 6, 8), mr.weight_planes(case["all_dets"][0, :9], 6, 8, "nan_int_min")
    assert (wp[:2] == 2.0).all() and (wn[:2] == 2.0).all()       # a NaN in column 0 or 1 is below the max(., 0) either way
    assert (wp[2, :, 0] == 2.0).all() and (wp[2, :, 1:] == 1e-5).all() and (wn[2] == 1e-5).all()
    assert (wp[3, 0, :] == 2.0).all() and (wp[3, 1:, :] == 1e-5).all() and (wn[3] == 1e-5).all()
    assert (wp[4] == 0.5).all() and (wp[5] == 1e-5).all() and (wp[6] == 1e-5).all()             # +/-2^30: whole, empty, empty


def test_im_size_rules_holds_its_conditions():
    case, ovr = lc.im_size_rules()
    assert [mr.sides(s) for s in case["im_size"]] == [(7, 5), (0, 5), (0, 5), (P30, 1), (65536, 32768), (1, 1), (1, 300)]
    assert [sr.pixels(s) for s in case["im_size"]] == [35, 0, 0, P30, P30, 1, 300]
    exact = dict(case, im_size=np.array([(7, 5)] + [tuple(s) for s in case["im_size"][1:]], np.float32))
    args = lambda c: (c["all_runs"], c["all_n_runs"], c["all_count"], c["im_size"])
    for method in ("AVG", "UNION"):
        v = lc.voted("im_size_rules", method)
        assert same(v, mr.vote_sparse(exact, ovr, method, lc.IM_WINDOWS))                         # (7.9, 5.2) is (7, 5)
        assert v["copied"][1:3, :4].all() and (v["need"][1:3, :4] == case["top_n_runs"][1:3, :4]).all()      # h w = 0: the vote copies
        assert (v["out_n_runs"][4, :4] == -1).all() and (v["need"][4, :4] == 0).all()            # h w = 2^31: refused
        assert not v["copied"][3, :4].any() and all(sum(l) == P30 for l in v["lists"][3][:4])    # 2^30 x 1 is voted
    b, be = lc.interval_boxes(*args(case)), lc.interval_boxes(*args(exact))
    assert all(np.array_equal(b[k], be[k]) for k in b)
    assert not b["boxes"][1:3, :4].any() and (b["area"][1:3, :4] == 0).all()
    assert b["boxes"][4, 0].tolist() == [0, 100, 0, 149] and b["boxes"][4, 1].tolist() == [16383, 65531, 16383, 65535]      # h = 65536 kept
    assert b["boxes"][3, 1].tolist() == [0, P30 - 5, 0, P30 - 1] and b["boxes"][6, 0].tolist() == [10, 0, 29, 0]            # h = 1: x is the position
    assert b["boxes"][5, :4].tolist() == [[0, 0, 0, 0]] * 4 and b["area"][5, :4].tolist() == [1, 0, 1, 1]
    small = [0, 1, 2, 5, 6]
    dec = mr.masks_to_boxes(case["all_runs"][small], case["all_n_runs"][small], case["all_count"][small], case["im_size"][small])
    assert all(np.array_equal(b[k][small], dec[k]) for k in b)
    for crowd in (False, True):
        p = mr.overlaps(*args(case)[:3], *args(case)[:3], case["im_size"], crowd, counts=sr.interval_counts)
        pe = mr.overlaps(*args(exact)[:3], *args(exact)[:3], exact["im_size"], crowd, counts=sr.interval_counts)
        assert all(np.array_equal(p[k], pe[k]) for k in p) and not p["ovr"][1:3].any() and p["ovr"][4, 0, 2] == (30 / 50 if crowd else 30 / 120)
        d = mr.overlaps(*[a[small] for a in args(case)[:3]] * 2, case["im_size"][small], crowd)
        assert all(np.array_equal(p[k][small], d[k]) for k in p)


def test_nms_limits_hold_their_conditions():
    cases = lc.nms_limits()
    keep = lambda c, variant=None: mr.nms(c["dets"], c["count"], c["ovr"], c["thresh"], c["mode"], variant)
    for name, want in lc.NMS_HAND.items():
        got = keep(cases[name])
        assert got["keep"][0, :got["keep_count"][0]].tolist() == want and (got["keep"][0, got["keep_count"][0]:] == -1).all(), name
    c = cases["r512_distinct"]
    got = keep(c)
    assert got["keep_count"][0] == 512 and np.array_equal(got["keep"][0], np.argsort(-c["dets"][0, :, 4], kind="stable"))
    assert len(set(c["dets"][0, :, 4].tolist())) == 512
    sets = {m: keep(cases["r512_seeded_" + m]) for m in ("IOU", "IOMA", "CONTAINMENT")}
    assert all(20 < s["keep_count"][0] < 500 for s in sets.values()) and not np.array_equal(sets["IOU"]["keep"], sets["IOMA"]["keep"])
    live = cases["r512_seeded_IOU"]["ovr"]
    assert np.isnan(live).any() and (live == 0.5).any() and (live == np.nextafter(0.5, 1)).any()
    for variant in ("lt", "reverse_ties"):
        assert not np.array_equal(keep(cases["r512_seeded_IOU"], variant)["keep"], sets["IOU"]["keep"]), variant
    assert keep(cases["nan_class"], "nan_class_equal")["keep"][0].tolist() == [0, 1, -1, -1, -1]    # two NaN classes as one class
    assert keep(cases["special_scores"], "reverse_ties")["keep"][0].tolist() != lc.NMS_HAND["special_scores"]


def test_the_batch_formulas_are_the_restatement_on_a_sample():
    case, keep, keep_count = lc.nms_batch()
    assert case["dets"].shape == (65535, 2, 6)
    rows = np.r_[0:210, 65535 - 210:65535]
    got = mr.nms(case["dets"][rows], case["count"][rows], case["ovr"][rows], case["thresh"], case["mode"])
    assert np.array_equal(got["keep"], keep[rows]) and np.array_equal(got["keep_count"], keep_count[rows])
    assert {tuple(k) for k in keep.tolist()} == {(0, 1), (1, 0), (0, -1), (1, -1)}               # the kept set differs by image
    b = lc.batch_limit()
    assert b["im_size"].shape == (65535, 2) and b["a"][0].shape == (65535, 1, 4)
    at = lambda x: x[rows]
    boxes = mr.masks_to_boxes(at(b["a"][0]), at(b["a"][1]), at(b["count"]), at(b["im_size"]))
    assert np.array_equal(boxes["boxes"], at(b["boxes"])) and np.array_equal(boxes["area"], at(b["area"])) and (boxes["nonempty"] == 1).all()
    assert len({tuple(r) for r in b["boxes"][:, 0].tolist()}) >= 12
    for crowd in (False, True):
        p = mr.overlaps(at(b["a"][0]), at(b["a"][1]), at(b["count"]), at(b["b"][0]), at(b["b"][1]), at(b["count"]), at(b["im_size"]), crowd)
        assert np.array_equal(p["ovr"], at(b["pairs"][crowd])) and (p["a_area"] == 2).all()
        assert {0.0, 1.0} < set(np.unique(b["pairs"][crowd]).tolist())


def test_far_offsets_sit_behind_4_gib_and_their_answers_are_the_restatement():
    runs, n_runs, im_size = lc.far_boxes()
    assert (lc.FAR_N - 1) * lc.FAR_R * runs.shape[2] * 4 == 1 << 32                              # image 2048 starts 4 GiB behind the base
    assert n_runs.min() >= 2 and n_runs.max() <= 10
    a, b, want = lc.far_overlaps()
    assert (lc.FAR_N - 1) * lc.FAR_R * lc.FAR_R * 8 == 1 << 32
    n2, cnt, size = np.full((1, 512), 2, np.int32), np.array([512], np.int32), np.array([(10, 10)], np.float32)
    rows = slice(0, 512, 37)
    for crowd in (False, True):
        got = mr.overlaps(a[:, rows], n2[:, rows], np.array([14], np.int32), b, n2, cnt, size, crowd, counts=sr.interval_counts)
        assert np.array_equal(got["ovr"], want[crowd]["ovr"][:, rows]) and np.array_equal(got["b_area"], want[crowd]["b_area"])
        assert 0 < np.count_nonzero(want[crowd]["ovr"]) < want[crowd]["ovr"].size
