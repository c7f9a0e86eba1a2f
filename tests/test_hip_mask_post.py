"""libdetectorch_mpost_hip.so on the MI355X against the numpy restatement (tests/mask_post_ref.py, tests/README_mask_post.md): mask
boxes, mask overlaps, the mask NMS walk and mask voting on the cases of tests/mask_post_cases.py, with outputs and workspaces
pre-filled with 0xFF; crafted matrices at the thresholds; a 30000 x 30000 pair; filled rectangles against the box protocol and
utils.boxes.nms; the reference-shaped functions of utils/segms.py; hip.mask_paste -> hip.mask_rle -> overlaps -> NMS -> vote
captured in a graph and replayed on rewritten inputs.

REQUIRED AGREEMENT: every output equals the restatement exactly -- ovr bit for bit, integers and run lists equal.  No tolerance."""
import numpy as np
import pytest
import torch

import coco_eval_ref as cr
import mask_post_cases as mc
import mask_post_ref as mr
import segm_eval_ref as sr

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name):
    """a vote case, its overlaps and its AVG / UNION answers, computed once"""
    if name not in _REF:
        case = mc.VOTE_CASES[name]()
        ovr = mc.real_ovr(case)
        _REF[name] = (case, ovr, {m: mr.vote(case, ovr, m) for m in ("AVG", "UNION")})
    return _REF[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def cu(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def filled(out):
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    return out


def ws_ff(nbytes):
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device="cuda")


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_overlaps(a, b, im_size, crowd):
    """a, b: (runs, n_runs, count) as numpy"""
    from detectorch_amd import hip_mpost
    N, Ra, Sa = a[0].shape
    Rb, Sb = b[0].shape[1:]
    out = filled(hip_mpost.overlaps_outputs(N, Ra, Rb, "cuda"))
    hip_mpost.mask_overlaps(cu(a[0]), cu(a[1]), cu(a[2]), cu(b[0]), cu(b[1]), cu(b[2]), cu(im_size), crowd, out=out,
                            ws=ws_ff(hip_mpost.overlaps_workspace_bytes(N, Ra, Sa, Rb, Sb)))
    return host(out)


def check_overlaps(got, want):
    assert same_bits(got["ovr"], want["ovr"]), np.argwhere(got["ovr"] != want["ovr"])[:5]
    assert same_bits(got["a_area"], want["a_area"]) and same_bits(got["b_area"], want["b_area"])


def run_vote(case, ovr, method):
    from detectorch_amd import hip_mpost
    N, T = case["top_n_runs"].shape
    A, Sa = case["all_runs"].shape[1:]
    out = filled(hip_mpost.vote_outputs(N, T, case["out_stride"], "cuda"))
    hip_mpost.mask_vote(cu(case["top_runs"]), cu(case["top_n_runs"]), cu(case["top_count"]), cu(case["all_runs"]), cu(case["all_n_runs"]),
                        cu(case["all_dets"]), cu(case["all_count"]), cu(np.asarray(ovr, np.float64)), cu(case["im_size"]),
                        case["iou_thresh"], case["binarize_thresh"], method, out=out, ws=ws_ff(hip_mpost.vote_workspace_bytes(N, A, Sa)))
    return host(out)


def check_vote(got, want, case):
    """out_n_runs, need and the runs below out_n_runs; rows past top_count still hold the 0xFF they were filled with"""
    n, need, runs = got["out_n_runs"], got["need"], got["out_runs"].view(np.uint32)
    assert np.array_equal(n, want["out_n_runs"]), np.argwhere(n != want["out_n_runs"])[:5]       # (0xFFFFFFFF is the -1 of a row not written)
    assert np.array_equal(need, want["need"]), np.argwhere(need != want["need"])[:5]
    for i in range(n.shape[0]):
        nt = mr.clamp(case["top_count"][i], n.shape[1])
        assert (runs[i, nt:] == 0xFFFFFFFF).all()
        for t in range(nt):
            if n[i, t] >= 0:
                assert runs[i, t, :n[i, t]].tolist() == want["lists"][i][t], (i, t)


# ---- entries 2 and 4 on the shared cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.VOTE_CASES))
def test_overlaps_and_votes_equal_the_restatement(name):
    case, ovr, want = reference(name)
    tops = (case["top_runs"], case["top_n_runs"], case["top_count"])
    pool = (case["all_runs"], case["all_n_runs"], case["all_count"])
    got = run_overlaps(tops, pool, case["im_size"], False)
    assert same_bits(got["ovr"], ovr) and (got["ovr"] > 0).any()
    if name != "large":                                         # with crowd: the divisor is the first argument's area
        check_overlaps(run_overlaps(tops, pool, case["im_size"], True), mr.overlaps(*tops, *pool, case["im_size"], True))
    for method in ("AVG", "UNION"):
        check_vote(run_vote(case, got["ovr"], method), want[method], case)


@pytest.mark.parametrize("below", [False, True])
def test_votes_at_the_thresholds(below):
    """a crafted ovr one ulp below, at and above iou_thresh, NaN; pixels with num / den exactly binarize_thresh -- and one ulp above it
    when the threshold is the float64 below 0.5"""
    case, ovr = mc.threshold_vote()
    case = dict(case, binarize_thresh=np.nextafter(0.5, 0) if below else 0.5)
    want = mr.vote(case, ovr, "AVG")
    assert want["lists"][0][0] == ([2, 2, 1, 3, 8] if below else [3, 1, 1, 1, 10])
    check_vote(run_vote(case, ovr, "AVG"), want, case)
    check_vote(run_vote(case, ovr, "UNION"), mr.vote(case, ovr, "UNION"), case)


def test_vote_with_a_negative_threshold_turns_the_background_on():
    """binarize_thresh < 0: 0 / den passes, so the walk covers the whole image; NaN: nothing passes"""
    case, ovr, _ = reference("tiny")
    for bt in (-0.25, float("nan")):
        c = dict(case, binarize_thresh=bt)
        want = mr.vote(c, ovr, "AVG")
        check_vote(run_vote(c, ovr, "AVG"), want, c)
    assert [0, 35] in mr.vote(dict(case, binarize_thresh=-0.25), ovr, "AVG")["lists"][0]


# ---- entry 3 ---------------------------------------------------------------------------------------------------------------------------------------
def run_nms(dets, count, ovr, thresh, mode):
    from detectorch_amd import hip_mpost
    N, R = dets.shape[:2]
    out = filled(hip_mpost.nms_outputs(N, R, "cuda"))
    hip_mpost.mask_nms(cu(dets), cu(count), cu(np.asarray(ovr, np.float64)), thresh, mode, out=out)
    return host(out)


def test_nms_on_crafted_matrices():
    c = mc.threshold_nms()
    kept = {}
    for key, matrix, mode in (("walk", c["iou"], "IOU"), ("IOU", c["crowd"], "IOU"), ("IOMA", c["crowd"], "IOMA"),
                              ("CONTAINMENT", c["crowd"], "CONTAINMENT")):
        got, want = run_nms(c["dets"], c["count"], matrix, c["thresh"], mode), mr.nms(c["dets"], c["count"], matrix, c["thresh"], mode)
        assert same_bits(got["keep"], want["keep"]) and same_bits(got["keep_count"], want["keep_count"]), (key, got["keep"], want["keep"])
        kept[key] = frozenset(got["keep"][0, :got["keep_count"][0]].tolist())
    assert len({kept["walk"], kept["IOMA"], kept["CONTAINMENT"]}) == 3 and kept["IOU"] == kept["CONTAINMENT"]


@pytest.mark.parametrize("name", ["tiny", "chunks"])
def test_nms_on_real_overlaps(name):
    """the pool of a vote case against itself: overlaps with and without crowd, then the three modes; classes from the row index"""
    case, _, _ = reference(name)
    pool = (case["all_runs"], case["all_n_runs"], case["all_count"])
    N, A = case["all_n_runs"].shape
    dets = np.full((N, A, 6), np.nan, np.float32)
    dets[:, :, 4] = case["all_dets"][:, :, 4]
    dets[:, :, 5] = 1 + np.arange(A) % 2
    for mode, thresh in (("IOU", 0.3), ("IOMA", 0.6), ("CONTAINMENT", 0.6)):
        pairs = run_overlaps(pool, pool, case["im_size"], mode != "IOU")
        check_overlaps(pairs, mr.overlaps(*pool, *pool, case["im_size"], mode != "IOU"))
        got, want = run_nms(dets, case["all_count"], pairs["ovr"], thresh, mode), mr.nms(dets, case["all_count"], pairs["ovr"], thresh, mode)
        assert same_bits(got["keep"], want["keep"]) and same_bits(got["keep_count"], want["keep_count"]), mode
        assert (0 < want["keep_count"]).all() and (want["keep_count"] < case["all_count"]).all()


# ---- entry 1 ---------------------------------------------------------------------------------------------------------------------------------------
def run_boxes(runs, n_runs, counts, im_size):
    from detectorch_amd import hip_mpost
    N, R = n_runs.shape
    out = filled(hip_mpost.boxes_outputs(N, R, "cuda"))
    hip_mpost.mask_boxes(cu(runs), cu(n_runs), cu(im_size), None if counts is None else cu(counts), out=out)
    return host(out)


def test_boxes_equal_the_restatement():
    runs, n_runs, counts, im_size, _ = mc.boxes()
    got, want = run_boxes(runs, n_runs, counts, im_size), mr.masks_to_boxes(runs, n_runs, counts, im_size)
    assert all(same_bits(got[k], want[k]) for k in want), got                                    # rows past the counts: still 0xFF = -1
    for name in ("tiny", "chunks", "large"):
        case, _, _ = reference(name)
        got = run_boxes(case["all_runs"], case["all_n_runs"], case["all_count"], case["im_size"])
        want = mr.masks_to_boxes(case["all_runs"], case["all_n_runs"], case["all_count"], case["im_size"])
        assert all(same_bits(got[k], want[k]) for k in want), name
    got = run_boxes(runs[:, :14], n_runs[:, :14], None, im_size)                                 # counts NULL: all rows
    assert same_bits(got["boxes"], want_boxes(runs, n_runs, im_size)["boxes"][:, :14])


def want_boxes(runs, n_runs, im_size):
    return mr.masks_to_boxes(runs, n_runs, None, im_size)


def test_huge_image_in_integers():
    """30000 x 30000: areas and intersections near 9e8, positions near 2^30"""
    c = mc.huge()
    a, b = (c["a_runs"], c["a_n_runs"], c["a_count"]), (c["b_runs"], c["b_n_runs"], c["b_count"])
    for crowd in (False, True):
        check_overlaps(run_overlaps(a, b, c["im_size"], crowd), mr.overlaps(*a, *b, c["im_size"], crowd, counts=sr.interval_counts))
    got = run_boxes(c["b_runs"], c["b_n_runs"], c["b_count"], c["im_size"])
    for r in range(3):
        box, area = mr.interval_box(c["b_runs"][0, r], c["b_n_runs"][0, r], 30000, 30000)
        assert tuple(got["boxes"][0, r]) == box and got["area"][0, r] == area and got["nonempty"][0, r] == 1
    assert tuple(got["boxes"][0, 0]) == (29999, 29993, 29999, 29999) and tuple(got["boxes"][0, 2]) == (0, 0, 0, 29999)
    got = run_boxes(c["a_runs"], c["a_n_runs"], c["a_count"], c["im_size"])
    assert tuple(got["boxes"][0, 0]) == (0, 0, 29999, 29999) and got["area"][0, 0] == 30000 * 30000 - 1000


# ---- the bridge to what is already pinned --------------------------------------------------------------------------------------------------------
def test_filled_rectangles_equal_the_box_protocol():
    from detectorch_amd.utils import boxes as box_utils
    c = mc.rects()
    R = len(c["boxes"])
    got = run_boxes(c["runs"], c["n_runs"], c["count"], c["im_size"])
    assert np.array_equal(got["boxes"][0, :R], c["boxes"].astype(np.int32)) and (got["nonempty"][0, :R] == 1).all()
    side = (c["runs"], c["n_runs"], c["count"])
    for crowd in (False, True):
        ovr = run_overlaps(side, side, c["im_size"], crowd)["ovr"][0]
        want = np.array([[cr.bb_iou(cr.xywh(c["boxes"][i]), cr.xywh(c["boxes"][j]), crowd) for j in range(R)] for i in range(R)])
        assert same_bits(ovr[:R, :R], want) and (ovr[R:] == 0).all() and (ovr[:, R:] == 0).all()
    iou = run_overlaps(side, side, c["im_size"], False)["ovr"]
    dets = np.zeros((1, R + 2, 6), np.float32)
    dets[0, :R, :4], dets[0, :R, 4], dets[0, :, 5] = c["boxes"], c["scores"], 1
    got = run_nms(dets, c["count"], iou, c["thresh"], "IOU")
    kept = got["keep"][0, :got["keep_count"][0]]
    by_box = box_utils.nms(dets[0, :R, :5], np.float32(c["thresh"]))
    assert sorted(kept.tolist()) == sorted(np.asarray(by_box).tolist()) and len(kept) <= R - R // 3
    assert (np.diff(c["scores"][kept]) < 0).all()                # in the order kept: by descending score


# ---- the contract of the outputs -------------------------------------------------------------------------------------------------------------------
def test_second_call_rewrites_every_output():
    """the same buffers and workspace, first the chunks case's image, then other masks: nothing of the first call survives"""
    from detectorch_amd import hip_mpost
    case, ovr, want = reference("tiny")
    other = dict(case, top_runs=case["top_runs"][::-1].copy(), top_n_runs=case["top_n_runs"][::-1].copy(), all_runs=case["all_runs"][::-1].copy(),
                 all_n_runs=case["all_n_runs"][::-1].copy(), all_dets=case["all_dets"][::-1].copy(), im_size=case["im_size"][::-1].copy())
    N, T = case["top_n_runs"].shape
    A = case["all_n_runs"].shape[1]
    pairs, votes = filled(hip_mpost.overlaps_outputs(N, T, A, "cuda")), filled(hip_mpost.vote_outputs(N, T, case["out_stride"], "cuda"))
    ws = ws_ff(max(hip_mpost.overlaps_workspace_bytes(N, T, 36, A, 40), hip_mpost.vote_workspace_bytes(N, A, 40)))
    for c in (other, case):
        dev = {k: cu(c[k]) for k in ("top_runs", "top_n_runs", "top_count", "all_runs", "all_n_runs", "all_dets", "all_count", "im_size")}
        hip_mpost.mask_overlaps(dev["top_runs"], dev["top_n_runs"], dev["top_count"], dev["all_runs"], dev["all_n_runs"], dev["all_count"],
                                dev["im_size"], False, out=pairs, ws=ws)
        hip_mpost.mask_vote(dev["top_runs"], dev["top_n_runs"], dev["top_count"], dev["all_runs"], dev["all_n_runs"], dev["all_dets"],
                            dev["all_count"], pairs["ovr"], dev["im_size"], c["iou_thresh"], c["binarize_thresh"], "AVG", out=votes, ws=ws)
    assert same_bits(pairs["ovr"].cpu().numpy(), ovr)
    check_vote(host(votes), want["AVG"], case)


def test_wrong_dtypes_and_sizes_are_refused():
    from detectorch_amd import hip_mpost
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")
    f32, f64 = torch.float32, torch.float64
    with pytest.raises(TypeError):
        hip_mpost.mask_boxes(z(1, 2, 4, dt=torch.int64), z(1, 2), z(1, 2, dt=f32))
    with pytest.raises(TypeError):
        hip_mpost.mask_boxes(z(1, 2, 4), z(1, 3), z(1, 2, dt=f32))
    with pytest.raises(ValueError, match="unsupported shape"):
        hip_mpost.mask_boxes(z(1, 513, 4), z(1, 513), z(1, 2, dt=f32))
    with pytest.raises(TypeError):
        hip_mpost.mask_overlaps(z(1, 2, 4), z(1, 2), z(1), z(2, 2, 4), z(2, 2), z(2), z(1, 2, dt=f32))
    with pytest.raises(TypeError):
        hip_mpost.mask_nms(z(1, 2, 6, dt=f32), z(1), z(1, 2, 2, dt=f32), 0.5)
    with pytest.raises(NotImplementedError):
        hip_mpost.mask_nms(z(1, 2, 6, dt=f32), z(1), z(1, 2, 2, dt=f64), 0.5, "IOA")
    with pytest.raises(TypeError):
        hip_mpost.mask_vote(z(1, 2, 4), z(1, 2), z(1), z(1, 3, 4), z(1, 3), z(1, 3, 4, dt=f32), z(1), z(1, 2, 3, dt=f64), z(1, 2, dt=f32), 0.5, 0.5)
    with pytest.raises(ValueError, match="out_stride"):
        hip_mpost.mask_vote(z(1, 2, 4), z(1, 2), z(1), z(1, 3, 4), z(1, 3), z(1, 3, 5, dt=f32), z(1), z(1, 2, 3, dt=f64), z(1, 2, dt=f32), 0.5, 0.5,
                            out_stride=0)


# ---- the reference-shaped functions ----------------------------------------------------------------------------------------------------------------
def test_reference_shaped_functions():
    """utils.segms.rle_mask_nms / rle_mask_voting / rle_masks_to_boxes on RLE dicts (lists and compressed strings) of the chunks
    image: the restatement's answers; a copied row is the caller's own dict; a voted list longer than every input (the second call)"""
    from detectorch_amd.utils import segms
    from detectorch_amd.utils.result_utils import _rle_counts_to_string, rle_string_to_counts
    case, _, _ = reference("chunks")
    h, w = 32, 40
    lists = [case["all_runs"][0, k, :case["all_n_runs"][0, k]].astype(np.int64).tolist() for k in range(100, 180)]
    rle = lambda k, runs: dict(size=[h, w], counts=_rle_counts_to_string(runs) if k % 2 else runs)
    pool = [rle(k, runs) for k, runs in enumerate(lists)]
    tops = pool[25:50] + [dict(size=[h, w], counts=[h * w]), dict(size=[h, w], counts=[700, 3, h * w - 703])]   # ... an empty top, a lone one
    dets = case["all_dets"][0, 100:180]
    as_arrays = lambda ms: [(np.array(m["counts"] if isinstance(m["counts"], list) else rle_string_to_counts(m["counts"]), np.uint32),) * 2 for m in ms]
    arr = lambda ms: [(a, len(a)) for a, _ in as_arrays(ms)]
    # boxes
    boxes, keep = segms.rle_masks_to_boxes(tops)
    want = [mr.mask_box(mr.bitmap(a, k, h, w)) for a, k in arr(tops)]
    assert boxes.dtype == np.float64 and boxes.tolist() == [list(map(float, b)) for b, _ in want] and keep.tolist() == [i for i, (_, k) in enumerate(want) if k]
    assert len(keep) == len(tops) - 1
    # nms
    runs, n_runs = mc.pack_lists([[a for a, _ in arr(pool)]], len(pool), 280, 1)
    count, size = np.array([len(pool)], np.int32), np.array([[h, w]], np.float32)
    for mode, thresh in (("IOU", 0.3), ("IOMA", 0.7), ("CONTAINMENT", 0.7)):
        ovr = mr.overlaps(runs, n_runs, count, runs, n_runs, count, size, mode != "IOU")["ovr"][0]
        want = mr.nms_walk(dets[:, 4], np.ones(len(pool)), ovr, thresh, mode)
        assert segms.rle_mask_nms(pool, dets, thresh, mode) == want and 0 < len(want) < len(pool), mode
    # voting
    t_runs, t_n = mc.pack_lists([[a for a, _ in arr(tops)]], len(tops), 280, 2)
    ovr = mr.overlaps(t_runs, t_n, np.array([len(tops)], np.int32), runs, n_runs, count, size, False)["ovr"][0]
    for method in ("AVG", "UNION"):
        want = mr.vote_image(arr(tops), arr(pool), dets, ovr, h, w, 0.25, 0.4, method)
        got = segms.rle_mask_voting(tops, pool, dets, 0.25, 0.4, method)
        assert len(got) == len(tops) and got[-1] is tops[-1] and got[-2] is tops[-2]
        for j, (g, v) in enumerate(zip(got, want)):
            if v is None:
                assert g is tops[j], j
            else:
                assert g["size"] == [h, w] and isinstance(g["counts"], str) and rle_string_to_counts(g["counts"]) == v, (method, j)
        if method == "AVG":                                     # longer than the first out_stride: voted a second time
            assert max(len(v) for v in want if v is not None) > max(len(a) for a, _ in arr(tops) + arr(pool))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------
def _pasted_batch(seed):
    """hip.mask_paste -> hip.mask_rle on the 2-image synthetic batch of test_hip_segm.py -> (rle dict, dets, counts, im_size), on the
    device"""
    from detectorch_amd import hip, synth
    rs = synth.rng(11, seed)
    B, D, M, im = 2, 8, 14, [(61, 83), (70, 52)]
    counts = np.array([8, 6], np.int32)
    dets = np.zeros((B, D, 6), np.float32)
    for b, (h, w) in enumerate(im):
        dets[b, :, :4] = synth.make_rois(rs, D, im_h=h, im_w=w, min_side=6, max_side=60)
        dets[b, :, 4], dets[b, :, 5] = rs.rand(D), np.sort(rs.randint(1, 3, D))
    masks = synth.make_masks(rs, B * D, 4, M)
    im_size = cu(np.array(im, np.float32))
    paste = hip.mask_paste(cu(masks), cu(dets), cu(counts), im_size, M, 61 * 83 * D)
    return hip.mask_rle(paste, cu(counts), im_size, runs_stride=512, str_stride=1024), cu(dets), cu(counts), im_size


def _chain(state):
    """the detections and their flipped-back duplicates (scores scaled by 0.9) as one pool; mask NMS on the pool; the kept rows voted
    by the pool.  Every step on the device, nothing synced: this is what the graph captures."""
    from detectorch_amd import hip_flip
    from detectorch_amd.utils import segms
    rle, dets, counts, im_size = state["rle"], state["dets"], state["counts"], state["im_size"]
    B, D, S = rle["counts"].shape
    there = hip_flip.flip_rle(rle["counts"], rle["n_runs"], im_size, state["ones"], counts=counts, out=state["there"], ws=state["flip_ws"])
    back = hip_flip.flip_rle(there["out_runs"], there["out_n_runs"], im_size, state["ones"], counts=counts, out=state["back"], ws=state["flip_ws"])
    idx = torch.arange(2 * D, device="cuda")[None, :].expand(B, 2 * D)
    c = counts[:, None].to(torch.int64)
    src = torch.where(idx < c, idx, torch.clamp(idx - c + D, max=2 * D - 1))             # rows c .. 2c - 1 are the duplicates
    both_runs = torch.cat([rle["counts"], back["out_runs"]], 1)
    both_n = torch.cat([rle["n_runs"], back["out_n_runs"]], 1)
    both_dets = torch.cat([dets, dets * state["scale"]], 1)
    state["pool_runs"].copy_(torch.gather(both_runs, 1, src[:, :, None].expand(B, 2 * D, S)))
    state["pool_n"].copy_(torch.gather(both_n, 1, src))
    state["pool_dets"].copy_(torch.gather(both_dets, 1, src[:, :, None].expand(B, 2 * D, 6)))
    state["pool_count"].copy_(counts * 2)
    kept = segms.rle_mask_nms_batched(state["pool_runs"], state["pool_n"], state["pool_dets"], state["pool_count"], im_size, 0.5, 'IOU',
                                      out=state["nms"], ws=state["ws"])
    keep = torch.clamp(kept["keep"], min=0).to(torch.int64)
    state["top_runs"].copy_(torch.gather(state["pool_runs"], 1, keep[:, :, None].expand(B, 2 * D, S)))
    state["top_n"].copy_(torch.gather(state["pool_n"], 1, keep))
    return segms.rle_mask_voting_batched(state["top_runs"], state["top_n"], kept["keep_count"], state["pool_runs"], state["pool_n"],
                                         state["pool_dets"], state["pool_count"], im_size, 0.5, 0.5, 'AVG', out=state["vote"], ws=state["ws"])


def _check_chain(state):
    """the restatement on the pool read back"""
    pool_runs, pool_n = state["pool_runs"].cpu().numpy().view(np.uint32), state["pool_n"].cpu().numpy()
    pool_dets, pool_count, im_size = state["pool_dets"].cpu().numpy(), state["pool_count"].cpu().numpy(), state["im_size"].cpu().numpy()
    B, A = pool_n.shape
    iou = mr.overlaps(pool_runs, pool_n, pool_count, pool_runs, pool_n, pool_count, im_size, False)
    assert same_bits(state["nms"]["ovr"].cpu().numpy(), iou["ovr"]) and same_bits(state["nms"]["a_area"].cpu().numpy(), iou["a_area"])
    kept = mr.nms(pool_dets, pool_count, iou["ovr"], 0.5, 'IOU')
    assert same_bits(state["nms"]["keep"].cpu().numpy(), kept["keep"]) and same_bits(state["nms"]["keep_count"].cpu().numpy(), kept["keep_count"])
    keep = np.maximum(kept["keep"], 0)
    case = dict(top_runs=np.take_along_axis(pool_runs, keep[:, :, None], 1), top_n_runs=np.take_along_axis(pool_n, keep, 1),
                top_count=kept["keep_count"], all_runs=pool_runs, all_n_runs=pool_n, all_dets=pool_dets, all_count=pool_count, im_size=im_size,
                out_stride=state["vote"]["out_runs"].shape[2], iou_thresh=0.5, binarize_thresh=0.5)
    ovr = mr.overlaps(case["top_runs"], case["top_n_runs"], case["top_count"], pool_runs, pool_n, pool_count, im_size, False)["ovr"]
    assert same_bits(state["vote"]["ovr"].cpu().numpy(), ovr)
    want = mr.vote(case, ovr, 'AVG')
    got = {k: state["vote"][k].cpu().numpy() for k in ("out_runs", "out_n_runs", "need")}
    n = got["out_n_runs"]
    for b in range(B):
        for t in range(kept["keep_count"][b]):
            assert n[b, t] == want["out_n_runs"][b, t] >= 0 and got["need"][b, t] == want["need"][b, t]
            assert got["out_runs"].view(np.uint32)[b, t, :n[b, t]].tolist() == want["lists"][b][t], (b, t)
    # every duplicate is suppressed by its original (IoU 1), and every kept row has at least two voters: itself and its duplicate
    assert (kept["keep_count"] <= pool_count // 2).all() and (kept["keep_count"] >= 2).all() and not want["copied"][0, :kept["keep_count"][0]].any()
    return want


def test_end_to_end_in_a_graph():
    """hip.mask_paste -> hip.mask_rle; the detections and their flipped-back duplicates through overlaps -> nms -> vote in the batched
    forms, captured once in a graph and replayed twice on rewritten inputs; checked against the restatement on the runs read back"""
    from detectorch_amd import hip_flip, hip_mpost
    from detectorch_amd.utils import segms
    rle, dets, counts, im_size = _pasted_batch(2)
    B, D, S = rle["counts"].shape
    A = 2 * D
    e = lambda *shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device="cuda")
    state = dict(rle=dict(counts=rle["counts"], n_runs=rle["n_runs"]), dets=dets, counts=counts, im_size=im_size,
                 ones=torch.ones(B, dtype=torch.int32, device="cuda"), scale=torch.tensor([1, 1, 1, 1, 0.9, 1], dtype=torch.float32, device="cuda"),
                 there=hip_flip.rle_outputs(B, D, S, "cuda"), back=hip_flip.rle_outputs(B, D, S, "cuda"),
                 flip_ws=ws_ff(hip_flip.rle_workspace_bytes(B, D, S)),
                 pool_runs=e(B, A, S), pool_n=e(B, A), pool_dets=e(B, A, 6, dt=torch.float32), pool_count=e(B), top_runs=e(B, A, S), top_n=e(B, A),
                 nms=dict(hip_mpost.nms_outputs(B, A, "cuda"), **hip_mpost.overlaps_outputs(B, A, A, "cuda")),
                 vote=dict(filled(hip_mpost.vote_outputs(B, A, S, "cuda")), **hip_mpost.overlaps_outputs(B, A, A, "cuda")),
                 ws=ws_ff(segms.rle_mask_voting_workspace_bytes(B, A, S, A, S)))
    _chain(state)                                                # eager: loads the libraries, warms the allocator
    torch.cuda.synchronize()
    first = _check_chain(state)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _chain(state)
    answers = [first["lists"]]
    for seed in (3, 4):
        r2, d2, c2, s2 = _pasted_batch(seed)
        state["rle"]["counts"].copy_(r2["counts"]), state["rle"]["n_runs"].copy_(r2["n_runs"]), dets.copy_(d2), counts.copy_(c2), im_size.copy_(s2)
        graph.replay()
        torch.cuda.synchronize()
        answers.append(_check_chain(state)["lists"])
    assert answers[0] != answers[1] != answers[2]
