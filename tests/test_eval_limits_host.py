"""The limit cases of the evaluation chain (tests/eval_limit_cases.py) without a GPU: for every case, THE CONDITION IT EXISTS FOR,
counted on the restatements' own walk (tests/coco_eval_ref.py, tests/segm_eval_ref.py), so that a case that drifts fails here and does
not pass vacuously on the GPU (tests/test_hip_eval_limits.py); and the greedy rounds of dtc_eval_proposal_recall's header, restated in
numpy on the pinned bbox_overlaps, against the reference's own evaluate_box_proposals on the new proposal cases
(tests/golden/eval_limits.npz).  None of these tests needs the libraries."""
import numpy as np
import pytest

from conftest import golden
import coco_eval_ref as cr
import eval_limit_cases as lc
import segm_eval_ref as sr

_RAN = {}


def ran(name):
    if name not in _RAN:
        case = lc.MATCH_CASES[name]()
        _RAN[name] = (case, cr.run(case))
    return _RAN[name]


def bit(word, a, t, T):
    return (int(word) >> (a * T + t)) & 1


def visiting_order(case, n, cls, a):
    """the positions of the class's gt in the order "not ignored first", stable: position -> place"""
    ng = min(max(int(case["gt_counts"][n]), 0), case["gt_boxes"].shape[1])
    rows = [g for g in range(ng) if case["gt_classes"][n, g] == cls]
    lo, hi = case["area_rngs"][a]
    ig = [bool(case["gt_is_crowd"][n, g]) or case["gt_area"][n, g] < lo or case["gt_area"][n, g] > hi for g in rows]
    return list(np.argsort(np.asarray(ig, np.uint8), kind="mergesort")), ig


# ---- the match cases --------------------------------------------------------------------------------------------------------------------
def test_full_gt_uses_every_word_and_the_last_byte():
    case, o = ran("full_gt")
    assert case["gt_boxes"].shape[1] == 256 and case["gt_counts"].tolist() == [256, 300, -4] and np.all(case["gt_classes"][0] == 1)
    for a in (0, 1):
        order, ig = visiting_order(case, 0, 1, a)
        assert len(order) == 256 and not ig[255] and any(ig) and order.index(255) < 255 and order[255] != 255
    m = o["gt_match"][0]                                          # [G, A, T]
    for pos in lc.EDGE_POS:
        assert (m[pos] >= 0).any(), pos
    assert {pos >> 6 for pos in range(256) if (m[pos] >= 0).any()} == {0, 1, 2, 3}
    # positions 64 apart matched at one (a, t): a mask word picked by too few bits of the position loses one of them
    assert all(m[p, 0, 0] >= 0 for p in (0, 64, 128, 192)) and all(m[p, 0, 0] >= 0 for p in (63, 127, 191, 255))
    # gt_counts = 300 counts 256 rows, -4 none
    for c in (1, 2):                                              # all 256 rows of image 1, the last one included
        rows = case["gt_classes"][1] == c
        assert rows.sum() == 128 == o["npig"][1, c - 1, 0] + int(case["gt_is_crowd"][1][rows].sum())
    assert case["gt_classes"][1, 255] == 2 and not case["gt_is_crowd"][1, 255] and o["gt_ignore"][1, 253] == 0b10
    assert not o["npig"][2].any() and not o["gt_ignore"][2].any() and np.all(o["gt_match"][2] == -1) and (o["dt_rank"][2] >= 0).sum() == 6


@pytest.mark.parametrize("name", sorted(lc.FULL_DETS))
def test_full_dets_fill_every_row(name):
    two, max_det = lc.FULL_DETS[name]
    case, o = ran("full_dets_" + name)
    cls, score = case["dets"][0, :, 5], case["dets"][0, :, 4]
    assert case["dets"].shape[1] == 512 == case["det_count"][0] and case["max_dets"][-1] == max_det and not np.isnan(case["dets"][0]).any()
    assert len(set(score.tolist())) == 10
    n1 = int((cls == 1).sum())
    assert n1 == (512 if not two else 512 - 171) and (o["dt_rank"][0][cls == 1] >= 0).sum() == min(n1, max_det)
    assert sorted(o["dt_rank"][0][(cls == 1) & (o["dt_rank"][0] >= 0)]) == list(range(min(n1, max_det)))
    for border in range(64, 512, 64):                           # equal scores on both sides of every 64-row border
        assert set(score[border - 64:border][cls[border - 64:border] == 1]) & set(score[border:border + 64][cls[border:border + 64] == 1])
        if two:                                                  # both classes in every chunk: the ballots are partial
            assert 0 < (cls[border - 64:border] == 2).sum() < 64 and 0 < (cls[border:border + 64] == 2).sum() < 64
    assert (max_det == 600) == (max_det > case["dets"].shape[1]) and (o["precision"] > 0).any()


@pytest.mark.parametrize("T,A", lc.ALL_LANES)
def test_all_lanes_use_the_last_bit(T, A):
    case, o = ran("all_lanes_%dx%d" % (T, A))
    assert len(case["iou_thrs"]) == T and len(case["area_rngs"]) == A and o["gt_match"].shape[2:] == (A, T)
    live = o["dt_rank"] >= 0
    top = T * A - 1
    for k in ("dt_match", "dt_ignore"):
        bits = (o[k][live] >> np.uint64(top)) & np.uint64(1)
        assert bits.any() and not bits.all(), k
        assert not (o[k] >> np.uint64(top) >> np.uint64(1)).any()
    if A == 16:
        ng = [(n, g) for n in range(6) for g in range(int(case["gt_counts"][n]))]
        b15 = [(o["gt_ignore"][n, g] >> 15) & 1 for n, g in ng]
        assert any(b15) and not all(b15)
    assert (T * A == 64) == ((T, A) != (1, 1))


def test_score_bits_order_every_finite_pattern():
    case, o = ran("score_bits")
    s = case["dets"][0, :, 4]
    key = lambda v: cr.score_key(lc.f32(v))
    assert np.signbit(s[[1, 4]]).all() and not np.signbit(s[[0, 5]]).any() and np.all(s[[0, 1, 4, 5]] == 0)
    assert key(0.0) == key(-0.0) and len({int(o["sort_key"][0, r]) for r in (0, 1, 4, 5)}) == 1
    assert o["dt_rank"][0, 0] + 1 == o["dt_rank"][0, 1] == o["dt_rank"][0, 4] - 1 == o["dt_rank"][0, 5] - 2     # equal keys: by row
    assert key(lc.FMAX) == 0x00800000 < key(1.0) < key(lc.TINY) == key(0.0) - 1 and key(-lc.TINY) == key(0.0) + 2 < key(-lc.FMAX) == 0xff7fffff
    assert key(lc.up(0.5)) + 1 == key(0.5) == key(lc.down(0.5)) - 1 and key(lc.down(-1.5)) == key(-1.5) + 1
    # every image ranks its class 1 rows as the keys order them, ties by row
    for n in range(4):
        rows = [d for d in range(24) if case["dets"][n, d, 5] == 1 and d < case["det_count"][n]]
        want = sorted(rows, key=lambda d: (key(case["dets"][n, d, 4]), d))
        assert [int(o["dt_rank"][n, d]) for d in want] == list(range(len(rows))) and len(rows) == len(lc.SCORES)
    # the last image_base of a run of four images
    base = (1 << 21) - 4
    top = lc.run_at(case, base)["sort_key"]
    live = top != cr.PAD_KEY
    assert np.array_equal(top[live] - o["sort_key"][live], np.full(live.sum(), base)) and (top[live] & ((1 << 21) - 1)).max() == (1 << 21) - 1


@pytest.mark.parametrize("name", sorted(lc.THRESHOLDS))
def test_threshold_edges_sit_on_the_edges(name):
    case, o = ran("threshold_edges_" + name)
    thr = list(case["iou_thrs"])
    T, t0, t5, t10, t15 = len(thr), thr.index(0.0), thr.index(0.5), thr.index(1.0), thr.index(1.5)
    assert (sorted(thr) != thr) == (name == "unsorted") and (len(set(thr)) < T) == (name == "unsorted")
    dm, di = o["dt_match"][0], o["dt_ignore"][0]
    assert case["dets"][0, 12, 5] == 2 and bit(dm[12], 0, t0, T) == 1 and [bit(dm[12], 0, t, T) for t in (t5, t10, t15)] == [0, 0, 0]
    assert [bit(dm[0], 0, t, T) for t in (t0, t5, t10, t15)] == [1, 1, 1, 1]        # the identical box: matched at t >= 1
    assert bit(dm[1], 0, t5, T) == 1 and bit(dm[1], 0, t10, T) == 0                  # IoU exactly 0.5
    # gt_area on lo, on hi and one float32 ulp outside: bit a of gt_ignore
    area = case["gt_area"][0, :6]
    assert area.tolist() == [400.0, 900.0, float(lc.down(400.0)), float(lc.up(400.0)), float(lc.down(900.0)), float(lc.up(900.0))]
    assert [int(v) for v in o["gt_ignore"][0, :6]] == [0b1000, 0b1010, 0b1110, 0b1010, 0b1010, 0b1110]
    assert not o["npig"][:, :, 3].any() and np.all(o["precision"][:, :, :, 3] == -1) and np.all(o["recall"][:, :, 3] == -1)
    # unmatched detections of area 399, 400, 401, 899, 900, 901 (rows 6 .. 11) at t = 0.5: ignored outside [lo, hi]
    assert [w * h for w, h in lc.UNMATCHED_SIDES] == [399, 400, 401, 899, 900, 901]
    assert all(bit(dm[r], a, t5, T) == 0 for r in range(6, 12) for a in range(4))
    assert [bit(di[r], 1, t5, T) for r in range(6, 12)] == [1, 0, 1, 1, 1, 1] and [bit(di[r], 2, t5, T) for r in range(6, 12)] == [1, 0, 0, 0, 0, 1]
    assert all(bit(dm[r], 0, t0, T) == 0 for r in range(6, 12))                       # t = 0: every gt is taken by then
    if name == "unsorted":
        i, j = [k for k, v in enumerate(thr) if v == 0.5]
        assert all(bit(w, a, i, T) == bit(w, a, j, T) for w in list(dm) + list(di) for a in range(4))


def test_area_fraction_sits_just_outside():
    case, o = ran("area_fraction")
    area = [float(np.prod(cr.xywh(case["dets"][0, r, :4])[2:])) for r in range(6)]
    assert area[0] == 400 and area[3] == 900 and 400 < area[1] < 400.0001 and 399.9999 < area[2] < 400 and 900 < area[4] < 900.0001 > 899.9999 < area[5] < 900
    assert not o["dt_match"][0, :6].any()
    assert [bit(o["dt_ignore"][0, r], 1, 0, 1) for r in range(6)] == [0, 1, 1, 1, 1, 1]
    assert [bit(o["dt_ignore"][0, r], 2, 0, 1) for r in range(6)] == [0, 0, 1, 0, 1, 0]


def test_degenerate_boxes_have_no_overlap():
    case, o = ran("degenerate_boxes")
    d, g = case["dets"][0], case["gt_boxes"][0]
    w, h = d[:11, 2] - d[:11, 0] + 1, d[:11, 3] - d[:11, 1] + 1
    assert w[:5].tolist() == [0, -4, 20, 20, -3] and h[:5].tolist() == [20, 20, 0, -4, -3]
    gw, gh = g[:6, 2] - g[:6, 0] + 1, g[:6, 3] - g[:6, 1] + 1
    assert gw[1:5].tolist() == [0, -4, 20, 20] and gh[1:5].tolist() == [20, 20, 0, -4]
    # each overlaps an ordinary box in the other axis, and no pair with a degenerate box has an IoU
    for i in range(5):
        assert cr.bb_iou(cr.xywh(d[i, :4]), cr.xywh(g[0]), False) == 0
    assert d[0, 1] == g[0, 1] and d[0, 3] == g[0, 3] and g[0, 0] < d[0, 0] < g[0, 2]
    T = 2
    assert all(bit(o["dt_match"][0, r], 0, 1, T) == 0 for r in (0, 1, 2, 3, 4, 8, 9)) and bit(o["dt_match"][0, 5], 0, 1, T) == 1
    assert bit(o["dt_match"][0, 0], 0, 0, T) == 1                                     # t = 0: IoU 0 matches
    assert [int(v) for v in o["gt_ignore"][0, 1:5]] == [0b100, 0b101, 0b100, 0b111]      # areas 0 and -80: inside [-100, 0]; the crowd one
    assert [bit(o["dt_ignore"][0, r], 1, 1, T) for r in (0, 1, 4)] == [0, 0, 1] and [bit(o["dt_ignore"][0, r], 2, 1, T) for r in (0, 1, 4)] == [1, 1, 0]


def test_class_column_rows_take_part_in_nothing():
    case, o = ran("class_column")
    assert case["num_classes"] == 4 and np.isnan(case["dets"][0, 7, 5]) and case["gt_classes"][0, 6] == -(1 << 31)
    assert case["det_count"][0] == 11 and case["gt_counts"][0] == 8
    none_d, none_g = [0, 4, 5, 6, 7], [1, 3, 5, 6]
    for r in none_d:
        assert o["dt_rank"][0, r] == -1 and o["sort_key"][0, r] == cr.PAD_KEY and o["dt_match"][0, r] == 0 and o["dt_ignore"][0, r] == 0
    for r in none_g:
        assert o["gt_ignore"][0, r] == 0 and np.all(o["gt_match"][0, r] == -1)
    keys = o["sort_key"][0]
    assert [int(keys[r]) >> 53 for r in (1, 2, 3, 8, 9, 10)] == [1, 2, 3, 2, 3, 1]     # 2.7 -> 2, 3.5 -> 3
    assert o["npig"][0, :, 0].tolist() == [2, 1, 1] and all((o["gt_match"][0, r] >= 0).any() for r in (0, 2, 4))


# ---- the accumulate cases ---------------------------------------------------------------------------------------------------------------
def segments(o, K):
    keys = np.sort(o["sort_key"].reshape(-1), kind="stable")
    return [cr.class_segment(keys, k) for k in range(K)]


def test_segment_lengths_are_the_tile_edges():
    case, o = ran("segment_lengths")
    seg = segments(o, 8)
    assert tuple(hi - lo for lo, hi in seg[:7]) == lc.SEG_LENGTHS == (0, 1, lc.TILE - 1, lc.TILE, lc.TILE + 1, 2 * lc.TILE, 2 * lc.TILE + 1)
    assert seg[7][1] - seg[7][0] > 0 and not o["counts"][7].any() and np.all(o["precision"][:, :, 7] == -1)
    assert o["counts"][0, 0] == 52 and np.all(o["recall"][:, 0, 0] == 0) and np.all(o["precision"][:, :, 0, 0] == 0)
    assert case["max_dets"] == (100, 1, 10) and case["dets"].shape[:2] == (52, 64)
    rank, cls = o["dt_rank"], np.nan_to_num(case["dets"][:, :, 5])
    cut = (rank < 0) & (cls >= 2) & (np.arange(64)[None] < case["det_count"][:, None])
    assert cut.sum() > 100 and all(((cls == c) & cut).any() for c in (3, 4, 5, 6, 7))
    # the rows of one class are spread over an image's rows, and rows of every rank lie between the rank-0 rows of a segment
    assert any(len(set(np.diff(np.flatnonzero(cls[n] == 5)))) > 1 for n in range(52))
    order = np.argsort(o["sort_key"].reshape(-1), kind="stable")
    r6 = rank.reshape(-1)[order[seg[5][0]:seg[5][1]]]
    assert set(r6.tolist()) == set(range(10)) and (np.diff(np.flatnonzero(r6 == 0)) > 1).any()
    assert all(o["precision"][0, 5, k, 0, 1] != o["precision"][0, 5, k, 0, 0] == o["precision"][0, 5, k, 0, 2] > 0 for k in range(2, 7))


def test_runs_of_padding_and_of_one_row():
    case, o = ran("all_padding")
    assert np.all(o["sort_key"] == cr.PAD_KEY) and np.all(o["dt_rank"] == -1) and o["counts"][:, 0].tolist() == [2, 2]
    assert np.all(o["recall"] == 0) and np.all(o["precision"] == 0)
    case, o = ran("one_row")
    assert o["sort_key"].size == 1 and o["dt_rank"][0, 0] == 0 and o["recall"][0, 0, 0, 2] == 1.0


@pytest.mark.parametrize("name", lc.RECALL_EDGES)
def test_recall_thresholds_equal_attained_recalls(name):
    case, o = ran("recall_edges_" + name)
    rec, T = case["rec_thrs"], 2
    assert len(rec) == {"r1": 1, "r1024": 1024, "m16": 36}[name] and len(case["max_dets"]) == (16 if name == "m16" else 3)
    assert np.all(np.diff(rec) >= 0) and o["counts"][0, 0] == 10 and o["counts"][1, 0] == 2
    lo, hi = segments(o, 2)[0]
    order = np.argsort(o["sort_key"].reshape(-1), kind="stable")[lo:hi]
    tp = np.cumsum([bit(w, 0, 0, T) for w in o["dt_match"].reshape(-1)[order]])
    attained = set((tp / 10.0).tolist())
    assert attained >= {j / 10.0 for j in range(1, 11)} and hi - lo == 20
    between = np.flatnonzero(np.diff(tp) == 0)                  # false positives between the true positives
    assert len(between) >= 5 and between.min() < 5
    if name == "r1":
        assert rec[0] in attained and rec[0] == 3 / 10.0
    else:
        for j in range(11):
            v = np.float64(j / 10.0)
            assert {np.nextafter(v, -1), v, np.nextafter(v, 2)} <= set(rec.tolist()), j
        assert (rec == 0.5).sum() == 2 and (rec > 1).sum() >= 2
        # a threshold met exactly is met AT that row: its precision differs from its upper neighbour's
        col = o["precision"][0, :, 0, 0, -1]
        at = lambda v: col[np.flatnonzero(rec == v)[0]]
        assert sum(at(np.float64(j / 10.0)) != at(np.nextafter(np.float64(j / 10.0), 2)) for j in range(1, 10)) >= 3
        assert all(at(np.float64(j / 10.0)) == at(np.nextafter(np.float64(j / 10.0), -1)) for j in range(1, 11))
        assert np.all(col[rec > 1] == 0)
    # class 2: every detection is ignored (inside the crowd gt), one gt counts
    d2 = (np.nan_to_num(case["dets"][:, :, 5]) == 2) & (o["dt_rank"] >= 0)
    assert d2.sum() == 6 and all(bit(w, 0, 0, T) and bit(w, 0, 1, T) for w in o["dt_ignore"][d2])
    assert np.all(o["recall"][:, 1, 0] == 0) and np.all(o["precision"][:, :, 1, 0] == 0)


# ---- proposal recall --------------------------------------------------------------------------------------------------------------------
def overlaps(e, n_gt):
    import mask_train_ref as mr
    props = e['boxes'][np.flatnonzero(e['gt_classes'] == 0)]
    return mr.bbox_overlaps(np.ascontiguousarray(props, np.float32), np.ascontiguousarray(e['boxes'][:n_gt], np.float32))


def taking_part(e, area):
    from test_eval_host import ec_area
    lo, hi = ec_area(area)
    return (e['gt_classes'] > 0) & (e['is_crowd'] == 0) & (e['seg_areas'] >= lo) & (e['seg_areas'] <= hi)


@pytest.mark.parametrize("name", sorted(lc.proposal_cases()))
def test_greedy_rounds_equal_the_reference(name):
    from test_eval_host import greedy_rounds, split_entry
    g, case = golden("eval_limits"), lc.proposal_cases()[name]
    rounds, meta, at = g[name + "_rounds"], g[name + "_meta"], 0
    for a, area in enumerate(lc.PROPOSAL_AREAS):
        for i, e in enumerate(case["roidb"]):
            props, gts, n_all = split_entry(e, area, case["limit"])
            n, n_pos = meta[a, i]
            assert n_pos == len(gts) and n == (len(gts) if n_all else 0)
            assert np.array_equal(greedy_rounds(props, gts)[:n], rounds[at:at + n])
            at += n
    assert at == len(rounds) and g[name + "_summary"].shape == (2, 12)


def test_proposal_conditions_occur():
    g, cases = golden("eval_limits"), lc.proposal_cases()
    meta = {k: g[k + "_meta"] for k in cases}
    n_props = lambda name, i: int((cases[name]["roidb"][i]['gt_classes'] == 0).sum())
    # G = 256 with G' = 256, 65, 128, 129, 255; the rows at the wavefront borders take no part; every wavefront holds some that do
    assert meta["g256"][0, :, 1].tolist() == [256, 65, 128, 129, 255] and all(0 < v < 120 for v in meta["g256"][1, :, 1])
    for i, e in enumerate(cases["g256"]["roidb"]):
        part = taking_part(e, "all")[:256]
        assert cases["g256"]["n_gt"][i] == 256 and part.sum() == meta["g256"][0, i, 1]
        if i in (1, 2, 3):
            assert not part[list(lc.SPLIT_ROWS)].any()
        assert i == 0 or not part[64]
        assert all(part[w * 64:(w + 1) * 64].any() for w in range(4))
    e = cases["g256"]["roidb"][0]
    assert np.array_equal(e['boxes'][11], e['boxes'][201]) and e['seg_areas'][1:5].tolist() == [1024.0, 9216.0, float(lc.down(1024.0)), float(lc.up(9216.0))]
    part = taking_part(e, "medium")
    assert part[1] and part[2] and not part[3] and not part[4]
    ov = overlaps(e, 256)
    best = ov.argmax(axis=0)
    assert best[10] == best[200] and ov[best[10], 10] == ov[best[10], 200] == ov[:, [10, 200]].max()
    second = lambda c: np.sort(ov[:, c])[-2]
    assert second(10) != second(200)                             # which of the two takes the shared proposal shows in the other's round
    # P = 65536: the best proposals at the ends of the strides
    e = cases["p65536"]["roidb"][0]
    assert n_props("p65536", 0) == 65536 and overlaps(e, 6).argmax(axis=0).tolist() == [0, 255, 256, 65535, 70, 40000]
    # equal overlaps 1, 64 and 256 apart; the later one is the better one for the gt next door
    e = cases["ties"]["roidb"][0]
    ov = overlaps(e, 9)
    for i, (q, dq) in enumerate(((10, 1), (30, 64), (120, 256))):
        a, b, c = 3 * i, 3 * i + 1, 3 * i + 2
        assert ov[q, a] == ov[q + dq, a] == ov[:, a].max() and ov[:, a].argmax() == q and ov[q + dq, b] == ov[:, b].max() > ov[q, b] > 0
        assert np.array_equal(e['boxes'][9 + 600 + q], e['boxes'][9 + 600 + q + dq]) and ov[:, c].argmax() == 600 + q
        assert ov[:, a].max() > ov[:, b].max()
    # G' = 200 with P' = 7; limit = 1 and limit = P; counts above P and negative
    assert meta["p7_g200"][0, 0].tolist() == [200, 200] and n_props("p7_g200", 0) == 7 and cases["p7_g200"]["n_gt"] == [256]
    assert cases["limit_1"]["limit"] == 1 and cases["limit_p"]["limit"] == 300 == n_props("limit_p", 0)
    assert np.count_nonzero(g["limit_1_rounds"][:40]) == 1 and np.count_nonzero(g["limit_p_rounds"][:40]) > 30
    boxes, counts = cases["counts"]["device"]
    assert counts.tolist() == [1050, -5] and boxes.shape == (2, 50, 4) and n_props("counts", 0) == 50 and n_props("counts", 1) == 0
    assert meta["counts"][0].tolist() == [[40, 40], [0, 12]]
    # the shared best proposal: every round retires the cached proposal of most columns left
    e = cases["shared_best"]["roidb"][0]
    ov = overlaps(e, 100)
    assert (ov.argmax(axis=0) == 0).sum() >= 60 and ov.shape == (1024, 100)
    # gt_area NULL: the float64 box area is the seg_area, on the ends of 'medium'
    e = cases["no_area"]["roidb"][0]
    b = e['boxes'][:8].astype(np.float64)
    assert np.array_equal((b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1), e['seg_areas'][:8]) and cases["no_area"]["no_area"]
    assert e['seg_areas'][:6].tolist() == [1024, 9216, 1056, 1023, 9312, 9215] and meta["no_area"][:, 0, 1].tolist() == [7, 4]


# ---- dtc_segm_iou -----------------------------------------------------------------------------------------------------------------------
def test_segm_full_gt_pairs_come_from_every_wavefront():
    case = lc.segm_full_gt()
    cls = case["gt_classes"][0]
    assert case["gt_counts"][0] == 256 and (cls == 1).sum() == 199 and (cls == 2).sum() == 57 and 199 % 4 and 57 % 4
    for c in (1, 2):
        assert all((cls[w * 64:(w + 1) * 64] == c).any() for w in range(4))
    assert case["dets"].shape[1] == 200 and case["det_count"][0] == 180
    assert all(case["det_n_runs"][0, r] < 0 for r in (63, 64, 130, 185)) and (case["det_n_runs"][0, :180] < 0).sum() == 3
    o = sr.iou_matrix(case)
    assert o["n_bad"].tolist() == [3] and (o["iou"] > 0).sum() > 5000 and (o["iou"][0, :, 192:] > 0).any() and (o["iou"] == 1).any()


def test_segm_chunk_lists_hold_their_conditions():
    case, lists = lc.segm_chunks(), lc.chunk_lists()
    ends = {k: sr.run_ends(np.asarray(v, np.uint32), len(v), lc.HW) for k, v in lists.items()}
    ones = lambda k: sum(1 for j in range(1, len(ends[k]), 2) if ends[k][j] > ends[k][j - 1])
    assert [ones("ones_%d" % k) for k in (64, 65, 128)] == [64, 65, 128]
    assert case["det_runs"].shape[2] == case["gt_runs"].shape[2] == 256 == len(lists["ones_128"])        # n_runs equal to the stride
    assert 256 in case["det_n_runs"][0] and 256 in case["gt_n_runs"][0]
    for k, v in lists.items():
        if k.startswith("reach"):
            n, r = (int(x) for x in k.split("_")[-2:])
            assert len(v) == n and ends[k][r] == lc.HW and (r == 0 or ends[k][r - 1] < lc.HW) and all(x > 0 for x in v[r + 1:])
            assert (sum(v[:r + 1]) == lc.HW) == ("exact" in k)
    assert {int(k.split("_")[-1]) % 64 for k in lists if k.startswith("reach")} == {63, 0}
    for r in (63, 64):
        for k in ("past_2_32_at_%d" % r, "past_2_32_summed_%d" % r):
            v = lists[k]
            assert sum(v[:r]) < 1 << 32 <= sum(v[:r + 1]) and sum(v[:r + 1]) % (1 << 32) + sum(v[r + 1:]) < lc.HW
    assert ends["gt_zero_runs"].count(8) == 4 and ends["on_the_ends"][:2] == [8, 12] and ends["on_the_ends_2"][:2] == [5, 8]
    # the interval form of the counts equals the bitmaps on every pair of these lists
    a, b = sr.iou_matrix(case), sr.iou_matrix(case, counts=sr.interval_counts)
    assert all(np.array_equal(a[k], b[k]) for k in a) and (a["iou"] > 0).sum() > 100
    names = sorted(lists)
    d, g = names.index("on_the_ends"), names.index("gt_zero_runs")
    assert a["iou"][0, d, g] == 10 / 13 and a["det_area"][0, d] == 10 and a["gt_mask_area"][0, g] == 13


def test_segm_im_sizes_truncate_and_clip():
    case = lc.segm_im_sizes()
    assert [sr.pixels(s) for s in case["im_size"]] == [35, 0, 0, 1 << 30, 1 << 30, 1 << 30]
    o = sr.iou_matrix(case, counts=sr.interval_counts)
    assert not o["det_area"][1:3].any() and not o["iou"][1:3].any() and (o["iou"][0] > 0).any() and (o["iou"][3:, :2, :3] > 0).all()
    assert o["det_area"][0].tolist()[:2] == [28, 20] and o["det_area"][3, 0] > 1 << 29 and np.array_equal(o["iou"][3], o["iou"][4])
