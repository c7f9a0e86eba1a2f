"""Polygons at image size to run lists on the GPU (include/detectorch_poly_hip.h, detectorch_amd/utils/segms.py) against the numpy
restatement (tests/poly_rle_ref.py; tests/README_poly_rle.md).  No tolerance anywhere: n_runs, runs[:n_runs], area and need are equal.
Outputs and workspace are pre-filled with 0xFF.
  * small and ragged shapes, invalid polygons, garbage and out-of-range offsets;
  * both branches of the trace, long and degenerate edges, vertices on the centre lines and outside the image;
  * more edges than threads, the capacities exactly met and exceeded by one, the three workgroup sizes of the sort;
  * the points are read as float64; two calls give the same bytes; the entry captured in a graph;
  * the consumers: hip_segm.segm_iou, segms.pack_gt_segms, evaluator.evaluate_masks; the training kernel's M x M masks."""
import numpy as np
import pytest
import torch

import mask_train_ref as mr
import poly_rle_ref as pr

pytestmark = pytest.mark.gpu

_REF = {}


def reference(key, make, runs_stride=2048, events_stride=2048):
    """the case and the restatement's answer at these capacities, each computed once"""
    if key not in _REF:
        _REF[key] = make()
    want_key = (key, runs_stride, events_stride)
    if want_key not in _REF:
        _REF[want_key] = pr.run(_REF[key], runs_stride, events_stride)
    return _REF[key], _REF[want_key]


def on_device(case):
    return {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in ("poly_xy", "poly_ptr", "gt_poly_ptr", "gt_counts", "im_size")}


def filled(out):
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    return out


def run_entry(case, runs_stride=2048, events_stride=2048, out=None, ws=None, dev=None):
    from detectorch_amd import hip, hip_poly
    d = on_device(case) if dev is None else dev
    N, G = case["gt_poly_ptr"].shape[0], case["gt_poly_ptr"].shape[1] - 1
    if out is None:
        out = filled(hip_poly.rle_outputs(N, G, runs_stride, d["im_size"].device))
    if ws is None:
        ws = hip.workspace(hip_poly.rle_workspace_bytes(N, G, case["poly_xy"].shape[1], case["poly_ptr"].shape[1] - 1, events_stride),
                           d["im_size"].device).fill_(0xFF)
    hip_poly.poly_rle(d["poly_xy"], d["poly_ptr"], d["gt_poly_ptr"], d["gt_counts"], d["im_size"], runs_stride, events_stride, out=out, ws=ws)
    return out


def check(out, want):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("n_runs", "area", "need"):
        assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())
    runs = got["runs"].view(np.uint32)
    for n, rows in enumerate(want["runs"]):
        for g, r in enumerate(rows):
            if r is not None:
                assert runs[n, g, :len(r)].tolist() == r, (n, g)
    return got


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)


def blob(rs, h, w, n=None, star=False):
    return mr.random_polygon(rs, rs.uniform(0, w), rs.uniform(0, h), rs.uniform(0.2, 0.7) * max(h, w) + 1, n or rs.randint(3, 12),
                             star=star).astype(np.float64)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def small_case():
    rs = np.random.RandomState(20261101)
    sizes = [(1, 1), (7, 5), (5, 7), (56, 56)]
    per = [[[rect(-1, -1, 3, 3)], [rect(0.2, 0.2, 0.4, 0.4)], [np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])]]]
    per.append([[rect(1, 2, 3, 5)], [blob(rs, 7, 5)], [blob(rs, 7, 5, star=True), rect(0, 0, 2, 2)]])
    per.append([[rect(2, 1, 5, 3)], [blob(rs, 5, 7)], [blob(rs, 5, 7), blob(rs, 5, 7)]])
    per.append([[blob(rs, 56, 56, 9)], [blob(rs, 56, 56, 11, star=True), blob(rs, 56, 56)], [rect(10.5, 10.5, 40.5, 30.5)]])
    return pr.make_case(per, sizes)


def ragged_case():
    rs = np.random.RandomState(20261102)
    nan_poly = rect(10, 10, 50, 60)
    nan_poly[2, 0] = np.nan
    far = rect(10, 10, 50, 60)
    far[1, 0] = 2.0 ** 26
    im0 = [[blob(rs, 97, 131, 8), blob(rs, 97, 131, 5, star=True), rect(20, 30, 25, 35)], [], [np.array([[5.0, 5.0], [60.0, 70.0]])], [nan_poly], [far]]
    im1 = [[blob(rs, 131, 97, 7)], [blob(rs, 131, 97, 10), rect(-5, -5, 30.2, 44.4)], [blob(rs, 131, 97)], [], []]
    im2 = [[blob(rs, 64, 64)], [rect(1, 1, 9, 9)], [], [], []]
    c = pr.make_case([im0, im1, im2], [(97, 131), (131, 97), (64, 64)], gt_counts=[5, 2, 0])
    return c


def garbage_past_counts_case():
    """the ragged case with the offsets past every count overwritten: huge, negative and backwards; the answer does not change"""
    c = {k: v.copy() for k, v in ragged_case().items()}
    c["gt_poly_ptr"][1, 3:] = [10 ** 9, -7, 3]                  # rows 2 .. 4 of image 1 lie past its count of 2 (row 2 ends at garbage)
    c["gt_poly_ptr"][2, 1:] = [-(10 ** 9), 2 ** 31 - 1, 0, 5, -1]
    used = int(c["gt_poly_ptr"][1, 2])
    c["poly_ptr"][1, used + 1:] = -12345
    c["poly_ptr"][2, :] = 2 ** 31 - 1
    return c


def bad_pointers_case():
    """offsets out of range INSIDE the counts: polygons that end past PTS, run backwards or start below 0 take part in nothing; a gt row
    whose polygon range is malformed takes part in nothing"""
    polys = [[rect(5, 5, 30, 40)], [rect(8, 8, 20, 20), rect(15, 15, 44, 50), rect(1, 1, 9, 9)], [rect(3, 3, 12, 12)], [rect(30, 30, 60, 60)],
             [rect(2, 2, 7, 7)]]
    c = pr.make_case([polys, polys], [(70, 64), (64, 70)])
    PTS = c["poly_xy"].shape[1]
    # image 0: polygon 1 ends past PTS (and so polygon 2 starts there), polygon 4 runs backwards, polygon 5 starts below 0
    c["poly_ptr"][0] = [0, 4, PTS + 9, 12, 16, 14, -4, 28][:c["poly_ptr"].shape[1]]
    # image 1: gt 1's range ends past NP, gt 3's runs backwards, gt 4's starts below 0
    c["gt_poly_ptr"][1] = [0, 1, 99, 5, 4, -2][:c["gt_poly_ptr"].shape[1]]
    return c


H_GEO, W_GEO = 200, 150


def geometry_case():
    """one polygon per row, each named for what its edges do"""
    h, w = H_GEO, W_GEO
    rows = [
        [np.array([[5.0, 20.0], [145.0, 60.0], [140.0, 90.0], [8.0, 45.0]])],                         # shallow, > 64 columns, both directions
        [np.array([[10.0, 5.0], [140.0, 190.0], [120.0, 195.0], [4.0, 30.0]])],                       # steep, dy > 64 px, > 64 columns: the bisection
        [np.array([[140.0, 190.0], [10.0, 5.0], [4.0, 30.0], [120.0, 195.0]])],                       # the same vertices another way round: self-intersecting
        [rect(20, 30, 90, 120)],                                                                       # horizontal and vertical edges
        [rect(20, 30, 90, 120)[::-1].copy()],                                                          # ... running right to left first
        [np.array([[12.0, 22.0], [12.0, 22.0], [60.0, 30.0], [60.0, 140.0], [60.0, 140.0], [30.0, 140.0], [12.0, 22.0]])],   # zero-length edges
        [np.array([[10.4, 10.4], [100.4, 12.4], [120.4, 150.4], [30.4, 99.4]])],                       # vertices on 5 i + 2
        [np.array([[0.4, 0.4], [149.4, 0.4], [149.4, 199.4], [0.4, 199.4]])],
        [np.array([[-20.3, -10.7], [w + 30.5, -3.2], [w + 10.1, h + 40.9], [-7.7, h + 12.3]])],        # around the image: j = h, the dropped h w
        [np.array([[-50.0, 100.0], [75.0, -80.0], [300.0, 100.0], [75.0, 400.0]])],
        [np.array([[w - 0.6, h - 3.0], [w + 5.0, h + 9.0], [w - 9.0, h + 2.0]])],                      # the last column's centre line, below the image
        [np.array([[w - 10.0, h - 0.2], [w - 0.6, h + 0.3], [w - 0.6, h - 8.0]])],
        [rect(-30, -30, -5, -5)],                                                                      # wholly outside
        [rect(-1000, -1000, 1000, 1000)],                                                              # covers it
    ]
    return pr.make_case([rows], [(h, w)])


def star_case():
    """300 vertices: more edges than threads in the tracing workgroup"""
    return pr.make_case([[[pr.star(60.3, 58.7, 30.0, 22.0, 300)], [rect(10, 10, 20, 20)], [pr.star(40.0, 70.0, 38.0, 22.0, 300), rect(2.5, 2.5, 117.5, 9.5)]]],
                        [(120, 120)])


def large_case():
    """480 x 640 with 8 instances: positions above 2^16, three digits of the position in the sort, thousands of events in a row"""
    rs = np.random.RandomState(20261103)
    rows = [[blob(rs, 480, 640, rs.randint(6, 16) if g % 3 == 2 else rs.randint(6, 40), star=(g % 3 == 2)) for _ in range(1 + g % 3)]
            for g in range(7)]
    rows.append([rect(3.5, 3.5, 636.5, 470.5), pr.star(320.0, 240.0, 230.0, 120.0, 64)])
    return pr.make_case([rows], [(480, 640)])


def capacity_case():
    return pr.make_case([[[rect(2, 2, 9, 9)], [pr.star(40.2, 33.1, 30.0, 11.0, 24), rect(50.5, 3.5, 75.5, 20.5)], [rect(60, 50, 70, 60)]]], [(70, 80)])


def double_polygon():
    """coordinates whose float32 round trip crosses a rounding boundary of trunc(5 x + 0.5)"""
    return np.array([[100.1, 37.3], [137.7, 21.9], [171.3, 48.1], [180.9, 90.7], [150.1, 130.3], [101.7, 141.9], [60.3, 120.1], [41.9, 77.7]])


# ---- the entry against the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make", [("small", small_case), ("ragged", ragged_case), ("bad_pointers", bad_pointers_case),
                                       ("geometry", geometry_case)])
def test_equals_the_restatement(name, make):
    case, want = reference(name, make)
    check(run_entry(case), want)
    assert (want["n_runs"] > 0).any()


def test_small_and_ragged_cases_hold_their_conditions():
    case, want = reference("small", small_case)
    assert want["runs"][0][0] == [0, 1] and want["runs"][0][1] == [1] and want["n_runs"][1:].min() >= 1
    case, want = reference("ragged", ragged_case)
    assert want["n_runs"][0].tolist()[1:4] == [0, 0, 0] and want["runs"][0][4] == [97 * 131] and want["need"][0, 4].tolist() == [0, 1]
    assert want["n_runs"][0, 0] > 3 and (want["n_runs"][1, :2] > 1).all() and not want["n_runs"][1, 2:].any() and not want["n_runs"][2].any()
    case, want = reference("bad_pointers", bad_pointers_case)
    assert want["n_runs"][0, 2:].tolist() == [0, 0, 0] and want["n_runs"][0, 0] > 1 and want["n_runs"][0, 1] > 1
    assert want["area"][0, 1] == pr.instance_bitmap([rect(1, 1, 9, 9).reshape(-1)], 70, 64).sum()               # gt 1 keeps one polygon of three
    assert want["n_runs"][1, 1:].tolist() == [0, 0, 0, 0] and want["n_runs"][1, 0] > 1
    case, want = reference("geometry", geometry_case)
    h, w = H_GEO, W_GEO
    assert want["runs"][0][12] == [h * w] and want["runs"][0][13] == [0, h * w] and want["runs"][0][3] == want["runs"][0][4]
    assert want["need"][0, 1, 0] > 128 and want["need"][0, 0, 0] > 128
    assert want["bitmaps"][0][8][h - 1].any() and want["bitmaps"][0][8][:, w - 1].any()


def test_garbage_offsets_past_the_counts():
    _, want = reference("ragged", ragged_case)
    case = garbage_past_counts_case()
    check(run_entry(case), want)


@pytest.mark.parametrize("events_stride", [2048, 4096, 8192])
def test_more_edges_than_threads(events_stride):
    """the three workgroup sizes of the sorting node on the same rows"""
    case, want = reference("star", star_case, events_stride=events_stride)
    check(run_entry(case, events_stride=events_stride), want)
    assert want["need"][0, 0, 0] > 256 and want["n_runs"][0, 0] > 100 and (want["n_runs"][0, 2] > 100) == (events_stride > 2048)


def test_capacities_exactly_met_and_exceeded_by_one():
    case, full = reference("capacity", capacity_case)
    E, R = (int(v) for v in full["need"][0, 1])
    assert E > 64 and R > 64 and (full["need"][0, [0, 2]] < [E, R]).all()
    for rs, es, fits in ((2048, E, True), (2048, E - 1, False), (R, 2048, True), (R - 1, 2048, False), (R, E, True)):
        _, want = reference("capacity", capacity_case, runs_stride=rs, events_stride=es)
        got = check(run_entry(case, runs_stride=rs, events_stride=es), want)
        assert (got["n_runs"][0, 1] > 0) == fits and got["n_runs"][0, 0] > 0 and got["n_runs"][0, 2] > 0      # the neighbours are intact
        if not fits:
            assert got["n_runs"][0, 1] == -1 and got["area"][0, 1] == 0 and got["need"][0, 1].tolist() == [E, -1 if es < E else R]


def test_large_image_several_sort_passes():
    case, want = reference("large", large_case, runs_stride=4096, events_stride=8192)
    got = check(run_entry(case, runs_stride=4096, events_stride=8192), want)
    assert got["need"][0, :, 0].max() > 2048 and got["area"][0].max() > 1 << 16 and (got["n_runs"][0] > 0).all()
    first_one = [r[0] for r in want["runs"][0]]
    assert max(first_one) > 1 << 16


def test_points_are_read_as_float64():
    poly = double_polygon()
    h, w = 160, 200
    case, want = reference("double", lambda: pr.make_case([[[poly]]], [(h, w)]))
    check(run_entry(case), want)
    rounded = pr.instance_bitmap([poly.astype(np.float32).astype(np.float64).reshape(-1)], h, w)
    assert not np.array_equal(rounded, want["bitmaps"][0][0])                      # the float32 round trip gives another mask


def test_two_calls_give_the_same_bytes():
    case, want = reference("large", large_case, runs_stride=4096, events_stride=8192)
    a = {k: v.cpu().numpy().tobytes() for k, v in run_entry(case, runs_stride=4096, events_stride=8192).items()}
    b = {k: v.cpu().numpy().tobytes() for k, v in run_entry(case, runs_stride=4096, events_stride=8192).items()}
    assert a == b


def stream_case(seed):
    rs = np.random.RandomState(20261110 + seed)
    sizes = [(60 + 7 * seed, 90 - 5 * seed), (80, 80)]
    per = [[[blob(rs, *sizes[i], rs.randint(3, 9)) for _ in range(rs.randint(1, 3))] for g in range(3)] for i in range(2)]
    return pr.make_case(per, sizes, gt_counts=[3, 2 + seed % 2], PTS=64, NP=8)


def test_captured_in_a_graph():
    """captured after one eager call, replayed on inputs rewritten in place"""
    from detectorch_amd import hip, hip_poly
    cases = [reference(("stream", s), lambda s=s: stream_case(s)) for s in (0, 1, 2)]
    dev = on_device(cases[0][0])
    out = filled(hip_poly.rle_outputs(2, 3, 2048, dev["im_size"].device))
    ws = hip.workspace(hip_poly.rle_workspace_bytes(2, 3, 64, 8, 2048), dev["im_size"].device)
    run_entry(cases[0][0], out=out, ws=ws, dev=dev)
    torch.cuda.synchronize()
    check(out, cases[0][1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_entry(cases[0][0], out=out, ws=ws, dev=dev)
    for case, want in cases[1:]:
        for k, v in on_device(case).items():
            dev[k].copy_(v)
        filled(out)
        graph.replay()
        torch.cuda.synchronize()
        check(out, want)


def test_wrong_dtypes_and_sizes_are_refused():
    """the binding's own checks, before the library is called"""
    from detectorch_amd import hip_poly
    case, _ = reference(("stream", 0), lambda: stream_case(0))
    d = on_device(case)
    call = lambda runs_stride=64, events_stride=64, out=None, **kw: hip_poly.poly_rle(*[kw.get(k, d[k]) for k in (
        "poly_xy", "poly_ptr", "gt_poly_ptr", "gt_counts", "im_size")], runs_stride, events_stride, out=out)
    with pytest.raises(TypeError, match="poly_xy"):
        call(poly_xy=d["poly_xy"].float())
    with pytest.raises(TypeError, match="poly_xy"):
        call(poly_xy=d["poly_xy"][:, ::2])
    with pytest.raises(TypeError, match="gt_counts"):
        call(gt_counts=d["gt_counts"].long())
    with pytest.raises(TypeError, match="im_size"):
        call(im_size=d["im_size"].double())
    with pytest.raises(ValueError, match="events stride"):
        call(events_stride=hip_poly.MAX_EVENTS + 1)
    with pytest.raises(ValueError, match="runs stride"):
        call(runs_stride=0)
    with pytest.raises(TypeError, match="runs"):
        call(out=hip_poly.rle_outputs(3, 3, 64, d["im_size"].device))
    with pytest.raises(ValueError, match="unsupported shape"):
        hip_poly.poly_rle(d["poly_xy"], d["poly_ptr"], torch.zeros((2, 258), dtype=torch.int32).cuda(), d["gt_counts"], d["im_size"], 64, 64)


# ---- the consumers -----------------------------------------------------------------------------------------------------------------------------
def test_run_lists_feed_segm_iou():
    """the entry's runs as gt_runs give the iou and gt_mask_area of the restatement's bitmaps packed by pack_gt_masks"""
    from detectorch_amd import hip_segm
    from detectorch_amd.utils.evaluator import pack_gt_masks
    case, want = reference("ragged", ragged_case)
    out = run_entry(case)
    N, G = want["n_runs"].shape
    sizes = [(97, 131), (131, 97), (64, 64)]
    packed = pack_gt_masks([[want["bitmaps"][n][g] for g in range(G)] for n in range(N)], sizes, "cuda", G, 2048)
    # the detections: the gt masks of image 0 shifted by one row, as uncompressed run lists
    dets, det_runs, det_n = np.zeros((N, 4, 6), np.float32), np.zeros((N, 4, 2048), np.uint32), np.zeros((N, 4), np.int32)
    for n in range(N):
        for d in range(4):
            m = want["bitmaps"][n][d % 2 if n else (0, 4, 0, 0)[d]]
            if m is None:
                continue
            r = pr.runs_of(np.roll(m, d, axis=0).T.reshape(-1))
            det_runs[n, d, :len(r)], det_n[n, d], dets[n, d, 4:] = r, len(r), (0.9 - 0.1 * d, 1)
    t = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    cls, crowd = t(np.ones((N, G), np.int32)), t(np.zeros((N, G), np.int32))
    args = (t(dets), t(np.full(N, 4, np.int32)), t(det_runs), t(det_n), t(case["im_size"]))
    a = hip_segm.segm_iou(*args, out["runs"], out["n_runs"], cls, crowd, t(case["gt_counts"]), 2)
    b = hip_segm.segm_iou(*args, packed["gt_runs"], packed["gt_n_runs"], cls, crowd, t(case["gt_counts"]), 2)
    for k in ("iou", "gt_mask_area", "det_area"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert (a["iou"] > 0).sum().item() >= 4 and np.array_equal(a["gt_mask_area"].cpu().numpy()[:2], want["area"][:2])


def wide_instance():
    """more than 2048 events and runs: pack_gt_segms's first guess is too small"""
    return [pr.star(600.0, 30.0, 590.0, 25.0, 8).reshape(-1).tolist(), [3.5, 3.5, 1196.5, 3.5, 1196.5, 60.5, 3.5, 60.5]]


def test_pack_gt_segms_mixes_every_form():
    from detectorch_amd.utils import result_utils as ru
    from detectorch_amd.utils import segms
    from detectorch_amd.utils.evaluator import pack_gt_masks
    rs = np.random.RandomState(20261104)
    crowd = np.zeros((64, 1200), bool)
    crowd[10:50, 100:900:2] = True
    tri = [[10.5, 5.5, 60.2, 9.9, 30.3, 50.1]]
    small = rs.rand(40, 30) < 0.5
    segm = [[wide_instance(), ru.rle_encode(crowd), None, tri, dict(size=[64, 1200], counts=ru.rle_counts(crowd))],
            [tri, small, [], tri + [[1.0, 1.0, 20.0, 1.0, 20.0, 30.0, 1.0, 30.0]]]]
    sizes = [(64, 1200), (40, 30)]
    out = segms.pack_gt_segms(segm, sizes, "cuda")
    bitmaps = [[pr.instance_bitmap(m, *sizes[i]) if segms.is_polygons(m) and len(m) else (None if segms.is_polygons(m) else m) for m in ms]
               for i, ms in enumerate(segm)]
    want = pack_gt_masks(bitmaps, sizes, "cuda")
    assert out["gt_runs"].shape == want["gt_runs"].shape and want["gt_n_runs"][0, 0].item() == out["gt_runs"].shape[2] > 2048   # sized from need, after the re-run
    assert torch.equal(out["gt_runs"], want["gt_runs"]) and torch.equal(out["gt_n_runs"], want["gt_n_runs"])
    areas = [[0 if b is None else int(np.asarray(b if not isinstance(b, dict) else crowd).sum()) for b in bs] for bs in bitmaps]
    assert out["area"].cpu().numpy()[0].tolist() == areas[0] and out["area"].cpu().numpy()[1, :4].tolist() == areas[1]
    with pytest.raises(ValueError, match="image 0 gt 0"):
        segms.pack_gt_segms([[wide_instance(), tri]], [(64, 1200)], "cuda", runs_stride=2000)
    one = segms.polys_to_rle(tri, 64, 70)
    assert one["size"] == [64, 70] and ru.rle_string_to_counts(one["counts"]) == pr.runs_of(pr.instance_bitmap(tri, 64, 70).T.reshape(-1))
    mask = segms.polys_to_mask(tri, 64, 70)
    assert mask.dtype == np.float32 and np.array_equal(mask, pr.instance_bitmap(tri, 64, 70).astype(np.float32))


def test_evaluate_masks_from_polygons():
    """gt given as polygons scores exactly as gt given as the restatement's bitmaps"""
    from detectorch_amd.utils import result_utils as ru
    from detectorch_amd.utils.evaluator import evaluate_masks
    rs = np.random.RandomState(20261105)
    h, w, N, K = 48, 64, 3, 3
    roidb, polys, all_boxes, all_segms = [], [], [[[] for _ in range(N)] for _ in range(K)], [[[] for _ in range(N)] for _ in range(K)]
    for n in range(N):
        ps = [[blob(rs, h, w, rs.randint(4, 9)).reshape(-1).tolist() for _ in range(rs.randint(1, 3))] for g in range(3)]
        cls = rs.randint(1, K, 3).astype(np.int32)
        roidb.append(dict(boxes=np.zeros((3, 4), np.float32), gt_classes=cls, is_crowd=np.array([0, 0, n == 1], np.int32),
                          seg_areas=np.full(3, 500.0, np.float32), height=h, width=w))
        polys.append(ps)
        for k in range(1, K):
            for g in range(3):                                  # detections: the gt masks moved a little, under both classes
                m = np.roll(pr.instance_bitmap(ps[g], h, w), rs.randint(-3, 4), axis=rs.randint(0, 2))
                all_segms[k][n].append(ru.rle_encode(m))
            all_boxes[k][n] = np.concatenate([np.zeros((3, 4), np.float32), rs.rand(3, 1).astype(np.float32)], 1)
    bitmaps = [[pr.instance_bitmap(p, h, w) for p in ps] for ps in polys]
    a = evaluate_masks(all_boxes, all_segms, roidb, polys, batch=2).accumulate()
    b = evaluate_masks(all_boxes, all_segms, roidb, bitmaps, batch=2).accumulate()
    for k in ("precision", "recall", "stats"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["stats"][0] > 0.05


def test_equals_the_training_kernel_on_an_m_by_m_image():
    """an M x M image and the identity normalisation: the decoded run list is the mask dtc_mask_targets writes for the same polygons"""
    from detectorch_amd import hip_mask
    M = 32                                                      # a power of two: (x * M) / M is x in float32
    polys = [p for p in mr.seeded_polygons(M, n=6)]
    for p in polys[:3], polys[3:]:
        img = mr.image([3], [0], [[0, 0, M, M]], [3], [list(p)], np.zeros((0, 4), np.float32))
        batch, _ = mr.stack([img], 4)
        t = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
        out = hip_mask.mask_targets(t["labels"], t["keep_inds"], t["n_rois"], t["gt_boxes"], t["gt_classes"], t["gt_is_crowd"], t["gt_counts"],
                                    t["proposals"], t["im_scale"], t["poly_xy"], t["poly_ptr"], t["gt_poly_ptr"], M=M, k_min=0, k_max=0, mask_rows=4)
        train = out["masks"][0, 0].cpu().numpy().reshape(M, M)
        case = pr.make_case([[[q.astype(np.float64) for q in p]]], [(M, M)])
        got = run_entry(case)
        n = int(got["n_runs"][0, 0])
        runs = got["runs"][0, 0, :n].cpu().numpy().view(np.uint32)
        flat = np.repeat(np.arange(n) % 2, runs).astype(np.int32)
        assert flat.size == M * M and np.array_equal(flat.reshape(M, M).T, train) and train.any()
