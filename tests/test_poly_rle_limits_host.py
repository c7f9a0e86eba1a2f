"""The limit cases of dtc_poly_rle (tests/poly_rle_limit_cases.py) without a GPU and without the library: for every case THE CONDITION
IT IS NAMED FOR, computed from the restatement alone (tests/poly_rle_ref.py), so that a case that drifts fails here and does not pass
vacuously on the GPU (tests/test_hip_poly_rle_limits.py); and the sparse form poly_rle_ref.run_sparse held to poly_rle_ref.run on every
case of tests/test_hip_poly_rle.py and on every new case that can be decoded."""
import numpy as np
import pytest

import poly_rle_limit_cases as lc
import poly_rle_ref as pr
import test_hip_poly_rle as old


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("n_runs", "area", "need")) and a["runs"] == b["runs"]


def positions(case, n, g):
    """every event position of the row, all polygons together"""
    ev = pr.row_events(case, n, g)
    return np.concatenate(ev) if ev else np.zeros(0, np.int64)


# ---- the sparse form -------------------------------------------------------------------------------------------------------------------------
OLD_CASES = [("small", old.small_case, [(2048, 2048)]), ("ragged", old.ragged_case, [(2048, 2048)]),
             ("garbage", old.garbage_past_counts_case, [(2048, 2048)]), ("bad_pointers", old.bad_pointers_case, [(2048, 2048)]),
             ("geometry", old.geometry_case, [(2048, 2048)]), ("star", old.star_case, [(2048, 2048), (2048, 4096), (2048, 8192)]),
             ("capacity", old.capacity_case, [(2048, 350), (2048, 349), (299, 2048), (298, 2048)]), ("large", old.large_case, [(4096, 8192)]),
             ("double", lambda: pr.make_case([[[old.double_polygon()]]], [(160, 200)]), [(2048, 2048)]),
             ("stream0", lambda: old.stream_case(0), [(2048, 2048)]), ("stream2", lambda: old.stream_case(2), [(2048, 2048)])]


@pytest.mark.parametrize("name,make,strides", OLD_CASES, ids=[c[0] for c in OLD_CASES])
def test_sparse_form_equals_the_bitmap_one_on_the_old_cases(name, make, strides):
    case = make()
    for rs, es in strides:
        assert same(pr.run(case, rs, es), pr.run_sparse(case, rs, es)), (rs, es)


@pytest.mark.parametrize("name", [n for n in lc.CASES if n not in ("big_image", "im_sizes")])
def test_sparse_form_equals_the_bitmap_one_on_the_new_cases(name):
    make, strides = lc.CASES[name]
    case = make()
    assert lc.decodable(case) or name == "mid_image"             # 9e6 pixels: decoded once all the same
    for rs, es in strides:
        assert same(pr.run(case, rs, es), lc.expected(name, rs, es)), (rs, es)


def test_sparse_form_on_the_decodable_images_of_im_sizes():
    case = {k: v[:4] for k, v in lc.im_sizes().items()}
    assert same(pr.run(case, 512, 2048), {k: v[:4] for k, v in lc.expected("im_sizes", 512, 2048).items()})


def test_union_of_spans_by_hand():
    assert pr.spans_of([7, 3, 3, 9, 12], 20) == [(7, 9), (12, 20)]            # sorted and paired; (3, 3) is empty; the odd last one runs to hw
    assert pr.union_runs([(2, 5), (5, 7), (6, 9), (12, 20)], 20) == ([2, 7, 3, 8], 15)
    assert pr.union_runs([(0, 4)], 20) == ([0, 4, 16], 4) and pr.union_runs([], 20) == ([20], 0) and pr.union_runs([(0, 20)], 20) == ([0, 20], 20)


# ---- the conditions --------------------------------------------------------------------------------------------------------------------------
def test_many_polygons_leave_the_lowest_digit_of_the_polygon():
    case = lc.many_polygons()
    assert case["gt_poly_ptr"][0].tolist() == [0, 300, 303] and case["poly_ptr"].shape[1] - 1 >= 300
    per_poly = pr.row_events(case, 0, 0)
    assert len(per_poly) == 300 and sum(len(e) > 0 for e in per_poly[256:]) >= 30      # polygon numbers >= 256 reach the keys: bits 40 and up
    mixed = 0                                                     # polygons j and 256 + j agree in the low 8 bits: do their events interleave?
    for j in range(300 - 256):
        a, b = np.sort(per_poly[j]), np.sort(per_poly[256 + j])
        mixed += bool(len(a) and len(b) and ((b > a[0]) & (b < a[-1])).any())
    assert mixed >= 30
    assert all(len(e) % 2 == 0 for e in per_poly)                # ... which is what it takes: whole blocks out of order keep the parities
    want = lc.expected("many_polygons", 4096, 8192)
    assert 2048 < want["need"][0, 0, 0] < 8192 and want["n_runs"][0, 0] > 256
    # row 1's polygons are 300 .. 302 of the image and 0 .. 2 of the row: alone in an image they give the same runs
    alone = pr.make_case([[[case["poly_xy"][0, s:e] for s, e in zip(case["poly_ptr"][0, 300:303], case["poly_ptr"][0, 301:304])]]], [lc.MANY_HW])
    assert pr.run_sparse(alone, 4096, 8192)["runs"][0][0] == want["runs"][0][1] and want["n_runs"][0, 1] > 3


def test_full_strides_meet_each_capacity_exactly():
    case = lc.full_strides()
    full = lc.expected("full_strides", 8200, 8192)
    assert full["need"][:, 1].tolist() == [[e, e + 1] for e in lc.SORT_CAPACITIES] and (full["need"][:, [0, 2], 0] < 64).all()
    for k, cap in enumerate(lc.SORT_CAPACITIES):
        met, missed = lc.expected("full_strides", 8200, cap), lc.expected("full_strides", 8200, cap - 1)
        assert met["n_runs"][k, 1] == cap + 1 and met["need"][k, 1].tolist() == [cap, cap + 1] and met["area"][k, 1] == 4 * 5 * cap // 8
        assert missed["n_runs"][k, 1] == -1 and missed["area"][k, 1] == 0 and missed["need"][k, 1].tolist() == [cap, -1]
        for w in (met, missed):                                   # the neighbours are intact, in every image
            assert (w["n_runs"][:, [0, 2]] == full["n_runs"][:, [0, 2]]).all() and (w["n_runs"][:, [0, 2]] > 1).all()
    met, missed = lc.expected("full_strides", 2049, 8192), lc.expected("full_strides", 2048, 8192)
    assert met["n_runs"][0, 1] == 2049 and missed["n_runs"][0, 1] == -1 and missed["need"][0, 1].tolist() == [2048, 2049] and missed["area"][0, 1] == 0
    strides = lc.CASES["full_strides"][1]
    assert {e for _, e in strides} >= {c - d for c in lc.SORT_CAPACITIES for d in (0, 1)} and {r for r, _ in strides} >= {2049, 2048}


def test_stacked_positions_span_several_threads():
    case = lc.stacked_positions()
    (rs, es), = lc.CASES["stacked_positions"][1]
    want = lc.expected("stacked_positions", rs, es)
    threads = {2048: 256, 4096: 512, 8192: 1024}[es]
    for g in (0, 1):
        pos = positions(case, 0, g)
        n_ev = len(pos)
        assert n_ev == want["need"][0, g, 0] <= es
        per = -(-n_ev // threads)
        _, counts = np.unique(pos, return_counts=True)
        assert per <= lc.KEYS_PER_THREAD < counts.max() == lc.STACK_N and counts.max() >= 3 * per        # one position lies over several [r0, r1)
    assert want["runs"][0][0] == want["runs"][0][2] and want["runs"][0][1] == want["runs"][0][3]       # the rectangle once; the widest one
    assert want["runs"][0][0] != want["runs"][0][1] and want["n_runs"][0, 0] == 41 and want["area"][0, 1] == 25 * 50


def digit_3_decides(case, n, g):
    """the second sort's keys are position << 1 | end, in the order (polygon, position) the first sort left: are there two events that
    a stable sort by the low three digits alone leaves in the wrong order?"""
    keys = np.concatenate([np.sort(e) for e in pr.row_events(case, n, g)]) << 1
    by_low = keys[np.argsort(keys & 0xffffff, kind="stable")]
    return bool((np.diff(by_low) < 0).any()) and len(set((keys >> 24).tolist())) > 1


def test_big_image_uses_the_top_digit_and_drops_h_w():
    case = lc.big_image()
    h, w = lc.BIG_HW
    assert pr.pixels(case["im_size"][0]) == 1 << 30 == h * w
    pos = positions(case, 0, 0)
    assert pos.max() >= 1 << 29 and pos.max() >> 24 and (pos.max() << 1) >> 24                      # digit 3 in both sorts
    assert digit_3_decides(case, 0, 0)
    dropped = []
    kept = pr.trace_positions(case["poly_xy"][0, :4], h, w, dropped=dropped)
    assert len(kept) == 155 and h * w in dropped and min(dropped) >= h * w                          # a candidate event on h w itself
    want = lc.expected("big_image", 512, 2048)
    spans = [s for e in pr.row_events(case, 0, 0) for s in pr.spans_of(e, h * w)]                   # the two polygons are disjoint
    assert want["area"][0, 0] == sum(b - a for a, b in spans) > 10000 and 2774 * h < want["runs"][0][0][0] < 2775 * h and max(want["runs"][0][0]) > 1 << 29
    assert sum(want["runs"][0][0]) == sum(want["runs"][0][1]) == h * w and want["runs"][0][1][0] == 0 and want["n_runs"][0, 1] > 2


def test_mid_image_uses_the_top_digit():
    case = lc.mid_image()
    assert pr.pixels(case["im_size"][0]) >= 1 << 23
    pos = positions(case, 0, 0)
    assert pos.max() >= 1 << 23 > pos.min() and len(pos) > 64 and digit_3_decides(case, 0, 0)


def test_far_vertices_cross_the_image_both_ways():
    case = lc.far_vertices()
    xy = case["poly_xy"][0, :4]
    X, Y = (5.0 * xy[:, 0] + 0.5).astype(np.int64), (5.0 * xy[:, 1] + 0.5).astype(np.int64)
    dx, dy = np.abs(np.roll(X, -1) - X), np.abs(np.roll(Y, -1) - Y)
    shallow, steep = dx >= dy, dx < dy
    assert (dx[shallow] > 1 << 22).any() and (dy[steep] > 1 << 22).any()
    h, w = lc.FAR_HW
    assert shallow[0] and dx[0] > 1 << 22 and steep[2] and dy[2] > 1 << 22
    for k, columns in ((0, w), (2, 10)):                          # the edge there and back: twice its events, one per pixel column it crosses
        assert len(pr.trace_positions(np.stack([xy[k], xy[(k + 1) % 4], xy[k]]), h, w)) == 2 * columns, k
    want = lc.expected("far_vertices", 1024, 2048)
    assert want["need"][0, 0, 0] == 319 and want["area"][0, 0] > 0
    assert (case["poly_xy"][0, 4:11] < 0).all() and want["runs"][0][1] == [h * w] and want["need"][0, 1].tolist() == [0, 1]


def test_im_size_rules():
    case = lc.im_sizes()
    assert [(pr.side(h), pr.side(w)) for h, w in case["im_size"]] == [(7, 5), (0, 9), (0, 9), (1, 1), (1 << 30, 1), (65536, 32768)]
    assert [pr.pixels(s) for s in case["im_size"]] == [35, 0, 0, 1, 1 << 30, 1 << 30] and np.isnan(case["im_size"][2, 0])
    want = lc.expected("im_sizes", 512, 2048)
    assert want["runs"][0][0] == [9, 3, 4, 3, 16]                # README_poly_rle.md's rectangle in a 7 x 5 image
    assert want["n_runs"][1:3, 0].tolist() == [0, 0] and not want["need"][1:3].any()
    assert want["runs"][3][0] == [0, 1] and want["runs"][4][0] == [2, 8, (1 << 30) - 10]
    dropped = []
    pr.trace_positions(case["poly_xy"][5, :4], 65536, 32768, dropped=dropped)
    assert dropped and want["need"][5, 0, 0] == 8 and sum(want["runs"][5][0]) == 1 << 30 and want["runs"][5][0][0] == 16380 * 65536 + 100


def test_max_shapes():
    case = lc.max_shapes()
    assert case["gt_poly_ptr"].shape == (4, 257) and case["poly_ptr"].shape == (4, 4097) and case["gt_counts"].tolist() == [256, 255, 300, -4]
    assert case["gt_poly_ptr"][0, 255:].tolist() == [4080, 4096]                          # the last polygon belongs to the last row
    want = lc.expected("max_shapes", 256, 2048)
    assert (want["n_runs"][0] > 1).all() and (want["n_runs"][1, :255] > 1).all() and want["n_runs"][1, 255] == 0
    assert (want["n_runs"][2] > 1).all() and not want["n_runs"][3].any() and not want["need"][3].any()
    assert len({tuple(want["runs"][2][g]) for g in (63, 64, 255)}) == 3 and want["runs"][1][:255] == want["runs"][2][:255]
