"""dtc_prepare_proposals on the MI355X: precomputed proposals -> RoIAlign-ready rois, against the reference's own preprocessing
(tests/golden/proposal_ingest.npz) and its numpy restatement (tests/proposal_prep_ref.py).  -m gpu."""
import numpy as np
import pytest
import torch

from conftest import golden
import proposal_prep_ref as pr

pytestmark = pytest.mark.gpu

CASES = sorted(pr.CASES)


def _batch(boxes_list, stride, garbage=None):
    B = len(boxes_list)
    x = np.full((B, stride, 4), np.nan if garbage is None else garbage, np.float32)
    if garbage is None:
        x[:, :, 1] = 1e30                                                  # NaN and out-of-domain values past the counts
    for b, bx in enumerate(boxes_list):
        x[b, :len(bx)] = bx
    counts = np.array([len(bx) for bx in boxes_list], np.int32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(counts).cuda()


def _check(out, b, want, k_min=2, k_max=5):
    m = len(want["rois"])
    assert int(out["n_out"][b]) == m
    r5 = out["rois5"][b, :m].cpu().numpy()
    assert np.array_equal(r5[:, 0], np.full(m, b, np.float32))
    assert np.array_equal(r5[:, 1:].view(np.uint32), want["rois"].view(np.uint32))              # bit for bit, -0. included
    lv = out["roi_levels"][b].cpu().numpy()
    assert np.array_equal(lv[:m], want["levels"]) and np.all(lv[m:] == -1)
    assert np.array_equal(out["level_counts"][b].cpu().numpy(), want["level_counts"][:k_max - k_min + 1])
    assert np.array_equal(out["rois_by_level"][b, :m].cpu().numpy(), want["rois_by_level"])
    assert np.array_equal(out["idx_restore"][b, :m].cpu().numpy(), want["idx_restore"])
    assert np.array_equal(out["src_index"][b, :m].cpu().numpy(), want["src_index"])
    T = out["roi_order"].shape[1]
    assert sorted(out["roi_order"][b].cpu().numpy().tolist()) == list(range(b * T, (b + 1) * T))


def test_prepare_proposals_equals_reference_fixture():
    from detectorch_amd import hip
    g = golden("proposal_ingest")
    boxes = [g[c + "_boxes"] for c in CASES]
    x, counts = _batch(boxes, 320)
    scales = [float(g[c + "_im_scale"]) for c in CASES]
    out = hip.prepare_proposals(x, counts, scales, max_out=384)
    torch.cuda.synchronize()
    for b, c in enumerate(CASES):
        want = pr.prepare(g[c + "_boxes"], scales[b])
        if len(g[c + "_boxes"]):
            assert np.array_equal(want["rois"], g[c + "_dedup"]) and np.array_equal(want["idx_restore"], g[c + "_rois_idx_restore_int32"])
            assert np.array_equal(want["rois_by_level"], np.concatenate([g["%s_rois_fpn%d" % (c, l)] for l in range(2, 6)], 0))
        _check(out, b, want)


def test_prepare_proposals_no_dedup_keeps_input_order_and_one_level():
    from detectorch_amd import hip
    g = golden("proposal_ingest")
    boxes = [g[c + "_boxes"] for c in CASES]
    x, counts = _batch(boxes, 300)
    scales = [float(g[c + "_im_scale"]) for c in CASES]
    out = hip.prepare_proposals(x, counts, scales, dedup_scale=0.0)
    c4 = hip.prepare_proposals(x, counts, scales, k_min=4, k_max=4)
    torch.cuda.synchronize()
    for b, c in enumerate(CASES):
        want = pr.prepare(g[c + "_boxes"], scales[b], dedup_scale=0)
        _check(out, b, want)
        assert np.array_equal(want["src_index"], np.arange(len(boxes[b])))
        if len(boxes[b]):
            assert np.array_equal(out["idx_restore"][b, :len(boxes[b])].cpu().numpy(), g[c + "_nodedup_restore"])
        _check(c4, b, pr.prepare(g[c + "_boxes"], scales[b], k_min=4, k_max=4), 4, 4)
        assert np.all(c4["roi_levels"][b, :int(c4["n_out"][b])].cpu().numpy() == 0)


def test_prepare_proposals_ignores_rows_past_counts_and_drops_non_finite_rows():
    from detectorch_amd import hip
    g = golden("proposal_ingest")
    a = g["a_boxes"]
    runs = []
    for garbage in (None, 0.0, 7.0, -1e9):
        x, counts = _batch([a, a[:17]], 512, garbage)
        runs.append(hip.prepare_proposals(x, counts, [1.5, 2.0]))
    torch.cuda.synchronize()
    for out in runs:
        _check(out, 0, pr.prepare(a, 1.5))
        _check(out, 1, pr.prepare(a[:17], 2.0))
    # rows whose scaled box is not finite are dropped (outside the reference's domain: it cannot pool them either)
    bad = a[:40].copy()
    bad[3, 1], bad[9, 2], bad[20, 0] = np.nan, np.inf, -np.inf
    x, counts = _batch([bad], 40)
    out = hip.prepare_proposals(x, counts, [1.25])
    keep = np.isfinite(bad).all(1)
    want = pr.prepare(bad[keep], 1.25)
    want["src_index"] = np.flatnonzero(keep)[want["src_index"]].astype(np.int32)
    torch.cuda.synchronize()
    _check(out, 0, want)


@pytest.mark.parametrize("n,B", [(1000, 8), (2048, 2), (64, 3)])
def test_prepare_proposals_random_batches(n, B):
    """random proposals on a coarse grid (many aliases) at the sizes of the sort's branches; the (2048, 2) case takes two keys per
    thread"""
    from detectorch_amd import hip
    rs = np.random.RandomState(n + B)
    boxes, scales = [], []
    for b in range(B):
        k = n - (37 if n > 100 else 7) * b
        xy = rs.randint(0, 600, (k // 2, 2)) * 1.5
        wh = rs.randint(1, 300, (k // 2, 2)) * 1.5
        base = np.hstack([xy, xy + wh])
        rows = base[rs.randint(0, len(base), k)] + rs.uniform(-0.5, 0.5, (k, 4))     # most rows alias another one
        boxes.append(np.maximum(rows, 0).astype(np.float32))
        scales.append(800.0 / rs.randint(400, 900))
    x, counts = _batch(boxes, n)
    out = hip.prepare_proposals(x, counts, scales)
    torch.cuda.synchronize()
    for b in range(B):
        want = pr.prepare(boxes[b], scales[b])
        assert len(want["rois"]) < len(boxes[b])
        _check(out, b, want)
    with pytest.raises(RuntimeError, match="DTC_EUNSUPPORTED"):
        hip.prepare_proposals(torch.zeros((1, 2049, 4), device="cuda"), torch.ones((1,), dtype=torch.int32, device="cuda"), [1.0])


def test_pooled_features_from_descriptors_equal_oracle_per_level(oracle):
    """the descriptors drive the existing RoIAlign launches unchanged: FPN (4 levels, 7x7, sr 2) and C4 (one level, 14x14, sr 0,
    the _ws entry) pooled features == oracle.roi_align_forward of each row on its own level, rows in output order"""
    from detectorch_amd import hip
    g = golden("proposal_ingest")
    rs = np.random.RandomState(3)
    boxes = [g["a_boxes"], g["b_boxes"]]
    scales = [float(g["a_im_scale"]), float(g["b_im_scale"])]
    x, counts = _batch(boxes, 300)
    H, W, C = 1344, 1344, 8
    scl = [0.25, 0.125, 0.0625, 0.03125]
    feats = [rs.standard_normal((2, C, H // int(1 / s), W // int(1 / s))).astype(np.float32) for s in scl]
    out = hip.prepare_proposals(x, counts, scales)
    T = out["rois5"].shape[1]
    dfeats = [torch.from_numpy(f).cuda() for f in feats]          # kept alive: the level table holds raw pointers
    lv, ch, dt = hip.make_levels(dfeats, scl)
    pooled = torch.zeros((2 * T, C, 7, 7), device="cuda")
    hip.check(hip.lib().dtc_roi_align_forward_packed(lv, 4, C, hip.DTC_F32, out["roi_desc"].data_ptr(), 2 * T, 7, 7, 2,
                                                     pooled.data_ptr(), hip.DTC_F32, hip.stream_ptr()), "packed")
    c4 = hip.prepare_proposals(x, counts, scales, k_min=4, k_max=4)
    f4 = rs.standard_normal((2, 16, H // 16, W // 16)).astype(np.float32)
    df4 = torch.from_numpy(f4).cuda()
    lv4, _, _ = hip.make_levels([df4], [0.0625])
    ws = hip.workspace(hip.lib().dtc_roi_align_workspace_bytes(2 * T), "cuda")
    p4 = torch.zeros((2 * T, 16, 14, 14), device="cuda")
    hip.check(hip.lib().dtc_roi_align_forward_packed_ws(lv4, 1, 16, hip.DTC_F32, c4["roi_desc"].data_ptr(), 2 * T, 14, 14, 0,
                                                        p4.data_ptr(), hip.DTC_F32, ws.data_ptr(), ws.numel(), hip.stream_ptr()), "ws")
    torch.cuda.synchronize()
    pooled, p4 = pooled.cpu().numpy().reshape(2, T, C, 7, 7), p4.cpu().numpy().reshape(2, T, 16, 14, 14)
    for b in range(2):
        want = pr.prepare(boxes[b], scales[b])
        m = len(want["rois"])
        rois5 = np.hstack([np.full((m, 1), b, np.float32), want["rois"]])
        assert len(set(want["levels"].tolist())) >= 3
        for l in range(4):
            sel = want["levels"] == l
            assert np.array_equal(pooled[b, :m][sel], oracle.roi_align_forward(feats[l], rois5[sel], 7, 7, scl[l], 2))
        assert np.array_equal(p4[b, :m], oracle.roi_align_forward(f4, rois5, 14, 14, 0.0625, 0))
        assert not np.any(pooled[b, m:]) and not np.any(p4[b, m:])          # padding rows zero-filled


def test_graph_replay_with_rewritten_proposals_matches_eager():
    from detectorch_amd import hip
    g = golden("proposal_ingest")
    rs = np.random.RandomState(11)
    x, counts = _batch([g["a_boxes"], g["b_boxes"]], 300)
    sc = torch.tensor([1.5, 2.5], device="cuda")
    out = hip.prepare_proposals(x, counts, sc)
    ws = hip.workspace(hip.lib().dtc_prepare_proposals_workspace_bytes(2, 300), "cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.prepare_proposals(x, counts, sc, out=out, ws=ws)
    torch.cuda.synchronize()
    for it in range(3):
        nb = [g["b_boxes"][rs.permutation(257)][:200 + 20 * it], g["a_boxes"][rs.permutation(300)][:250 - 30 * it]]
        x2, c2 = _batch(nb, 300)
        x.copy_(x2); counts.copy_(c2)
        sc.copy_(torch.tensor([1.0 + 0.3 * it, 800.0 / 427.0], device="cuda"))
        graph.replay()
        eager = hip.prepare_proposals(x2, c2, sc.clone())
        torch.cuda.synchronize()
        for k in eager:
            if k in ("rois5", "rois_by_level", "idx_restore", "src_index", "roi_order", "roi_desc"):
                for b in range(2):
                    m = int(eager["n_out"][b])
                    assert torch.equal(out[k][b, :m], eager[k][b, :m]), k
            else:
                assert torch.equal(out[k], eager[k]), k
        for b in range(2):
            _check(out, b, pr.prepare(nb[b], float(np.float32(sc[b].item()))))


def test_c4_region_path_graph_replay_with_bound_proposals():
    """C4RegionPath.bind_proposals: launch_proposals runs dtc_prepare_proposals (one level) in the captured graph; proposals, counts
    and scales copied into the bound tensors apply at the next replay"""
    from detectorch_amd.pipeline import C4RegionPath
    g = golden("proposal_ingest")
    B, C, T = 2, 16, 320
    path = C4RegionPath(B, "cuda", channels=C, post_nms_top_n=T, pooled=14, im_h=256, im_w=320)
    rs = np.random.RandomState(5)
    feat = torch.from_numpy(rs.standard_normal((B, C, 16, 20)).astype(np.float32)).cuda()
    x, counts = _batch([g["a_boxes"], g["b_boxes"]], 300)
    path.bind_proposals(x, counts, torch.tensor([0.25, 0.3], device="cuda"), feat)
    cls = torch.softmax(torch.from_numpy(rs.standard_normal((B, T, 81)).astype(np.float32) * 4).cuda(), 2).contiguous()
    bbox = torch.from_numpy(rs.standard_normal((B, T, 324)).astype(np.float32) * 0.1).cuda()
    path.bind_heads(cls, bbox, torch.tensor([0.25, 0.3], device="cuda"), torch.tensor([[427.0, 640.0], [1000.0, 750.0]], device="cuda"))
    for it, (nb, sc) in enumerate([([g["a_boxes"], g["b_boxes"]], [0.25, 0.3]), ([g["b_boxes"][:100], g["a_boxes"]], [0.3, 0.2])]):
        x2, c2 = _batch(nb, 300)
        path.prop_in.copy_(x2); path.prop_in_counts.copy_(c2); path.prop_im_scale.copy_(torch.tensor(sc, device="cuda"))
        path.step(use_graph=True)
        torch.cuda.synchronize()
        assert path.graph is not None
        for b in range(B):
            want = pr.prepare(nb[b], float(np.float32(sc[b])), k_min=4, k_max=4)
            n = len(want["rois"])
            assert int(path.n_rois[b]) == n
            assert np.array_equal(path.rois5[b, :n, 1:].cpu().numpy(), want["rois"])
            assert np.array_equal(path.prop_src[b, :n].cpu().numpy(), want["src_index"])
        assert int(path.det_count.min()) >= 0
