"""libdetectorch_aug_hip.so and the model-level entry on the MI355X against the numpy restatement (tests/tta_ref.py,
tests/README_tta.md), on the cases of tests/tta_cases.py, every output pre-filled with NaN (0xFF bytes for integers).

REQUIRED AGREEMENT: the merge, SOFT_AVG and SOFT_MAX equal the restatement bit for bit.  LOGIT_AVG is compared with the float64 form
of the rule within twice the largest distance of the float32 form Detectron runs (numpy's own float32 log and exp) from the float64
form on the same inputs -- the test computes that distance itself --, and must give exactly 1 where every view has 1 and the
correctly rounded chain's value where every view has 0."""
import numpy as np
import pytest
import torch

import det_options_ref as dr
import tta_cases as tc
import tta_ref as tr

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def aug():
    from detectorch_amd import hip_aug
    hip_aug.lib()
    return hip_aug


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def device_views(views):
    return [{k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in view.items()} for view in views]


def nan_filled(out):
    for v in out.values():
        v.fill_(float("nan")) if v.is_floating_point() else v.view(torch.uint8).fill_(0xFF)
    return out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_merge(aug, views, im, sh, ch, logits):
    B, R, C = views[0]["cls_score"].shape
    out = nan_filled(aug.merge_outputs(B, aug.merge_rows(len(views), R, sh), C, "cuda"))
    aug.merge_boxes(device_views(views), cu(im), sh, ch, logits, out=out)
    torch.cuda.synchronize()
    return host(out)


# ---- (a) the merge, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("T,heurs,counts", [(1, ("UNION", "UNION"), tc.UNION_COUNTS), (1, ("UNION", "UNION"), tc.UNION_COUNTS[::-1]),
                                            (8, ("UNION", "UNION"), tc.UNION_COUNTS), (3, ("AVG", "AVG"), tc.ALIGNED_COUNTS),
                                            (3, ("ID", "ID"), tc.ALIGNED_COUNTS), (3, ("AVG", "ID"), tc.ALIGNED_COUNTS),
                                            (3, ("ID", "AVG"), tc.ALIGNED_COUNTS)])
def test_merge_equals_the_restatement(aug, T, heurs, counts, logits):
    views, im = tc.merge_case(T, counts, logits)
    ref = tr.merge_boxes(views, im, heurs[0], heurs[1], logits)
    got = run_merge(aug, views, im, heurs[0], heurs[1], logits)
    for k in ("out_n", "out_src", "out_scores", "out_boxes"):                 # NaN pre-fill: rows past out_n must read zero, out_src -1
        assert same_bits(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:5])
    assert ref["out_n"].sum() > 0


# ---- (b) the merge of one unflipped view, through decoded_boxes, is the detection entry decoding the same rows itself ---------------
@pytest.mark.parametrize("method,vote", [("nms", None), ("linear", 0.8)])
def test_merged_single_view_through_decoded_boxes_is_the_detection_entry(aug, method, vote):
    from detectorch_amd import hip
    views, im = tc.merge_case(1, tc.ALIGNED_COUNTS, True, seed=3)
    v = device_views(views)[0]
    m = aug.merge_boxes([v], cu(im), scores_are_logits=True)
    kw = dr.kwargs_of(method, vote)
    a = hip.box_results_nms_limit(m["out_scores"], m["out_boxes"], m["out_n"], **kw)
    b = hip.postprocess_detections(v["rois5"], v["n_rois"], v["cls_score"], v["bbox_pred"], v["scale"], cu(im), scores_are_logits=True, **kw)
    torch.cuda.synchronize()
    assert int(b[3].sum()) > 10
    assert same_bits(a[0].cpu().numpy(), b[0].cpu().numpy()) and same_bits(a[1].cpu().numpy(), b[1].cpu().numpy())
    assert same_bits(a[2].cpu().numpy(), b[3].cpu().numpy())
    assert same_bits(m["out_n"].cpu().numpy(), views[0]["n_rois"])


# ---- (c) the combination -------------------------------------------------------------------------------------------------------------
def run_combine(aug, masks, flipped, cnt, mc, heur):
    out = torch.full(masks[0].shape, float("nan"), device="cuda")
    aug.combine_masks([cu(m) for m in masks], flipped, cu(cnt), None if mc is None else cu(mc), heur, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("with_class", [True, False])
@pytest.mark.parametrize("heur", ["SOFT_AVG", "SOFT_MAX"])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("M", [28, 7])
def test_soft_combinations_equal_the_restatement(aug, M, T, heur, with_class):
    masks, flipped, cnt, mc = tc.combine_case(M, T)
    mc = mc if with_class else None
    got = run_combine(aug, masks, flipped, cnt, mc, heur)
    assert same_bits(got, tr.combine_masks(masks, flipped, cnt, mc, heur))
    # the mirror: a flipped view of the mirrored tensor gives the unflipped answer exactly
    turned = [np.ascontiguousarray(m[..., ::-1]) if f else m for m, f in zip(masks, flipped)]
    assert same_bits(run_combine(aug, turned, [0] * T, cnt, mc, heur), got)
    turned = [m if f else np.ascontiguousarray(m[..., ::-1]) for m, f in zip(masks, flipped)]
    assert same_bits(run_combine(aug, turned, [1] * T, cnt, mc, heur), got)


@pytest.mark.parametrize("with_class", [True, False])
@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("M", [28, 7])
def test_logit_avg_within_the_restatements_own_error(aug, M, T, special, with_class):
    masks, flipped, cnt, mc = tc.combine_case(M, T, special=special)
    mc = mc if with_class else None
    ref64 = tr.combine_masks64(masks, flipped, cnt, mc)
    lit = tr.combine_masks(masks, flipped, cnt, mc, "LOGIT_AVG", exact=False)
    tol = 2 * np.abs(lit.astype(np.float64) - ref64).max()
    got = run_combine(aug, masks, flipped, cnt, mc, "LOGIT_AVG")
    dev = np.abs(got.astype(np.float64) - ref64).max()
    print("LOGIT_AVG M=%d T=%d special=%d class=%d: device %.3e, float32 form %.3e, tolerance %.3e" % (M, T, special, with_class, dev,
                                                                                                       tol / 2, tol))
    assert np.isfinite(got).all() and tol > 0 and dev <= tol
    assert same_bits(got == 0, ref64 == 0)                                   # the rows and channels that are not combined: +0.0
    assert not np.signbit(got).any()
    if special:                                                              # y = 1 in every view: exactly 1; y = 0 in every view: the chain's value
        live = ref64[..., 2] != 0
        assert live.any() and (got[..., 2][live] == 1.0).all()
        cr = tr.combine_masks(masks, flipped, cnt, mc, "LOGIT_AVG", exact=True)
        assert same_bits(got[..., 0], cr[..., 0]) and (got[..., 0][live] > 0).all() and (got[..., 0] < 2e-20).all()


# ---- (d) refusals write nothing ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(aug):
    import ctypes as C
    views, im = tc.merge_case(2, tc.UNION_COUNTS, False)
    dv, dim = device_views(views), cu(im)
    out = nan_filled(aug.merge_outputs(tc.B, 2 * tc.R, tc.N_CLS, "cuda"))
    before = {k: v.clone() for k, v in out.items()}
    arr = (aug.AugView * 9)(*[aug.AugView(v["rois5"].data_ptr(), v["n_rois"].data_ptr(), v["cls_score"].data_ptr(), v["bbox_pred"].data_ptr(),
                                          v["scale"].data_ptr(), 0, 0) for v in (dv * 5)[:9]])
    base = dict(views=arr, n_views=2, im_size=dim.data_ptr(), batch=tc.B, max_rois=tc.R, n_cls=tc.N_CLS, scores_are_logits=0, wx=10.0, wy=10.0,
                ww=5.0, wh=5.0, score_heur=0, coord_heur=0, **{k: v.data_ptr() for k, v in out.items()})
    order = [n for n, _ in aug.SIGNATURES["dtc_aug_merge_boxes"][1][:-1]]
    call = lambda **kw: aug.lib().dtc_aug_merge_boxes(*[dict(base, **kw)[n] for n in order], None)
    assert call(coord_heur=1) == -1 and call(score_heur=5, coord_heur=5) == -1 and call(n_cls=1) == -1 and call(im_size=None) == -1
    assert call(n_views=9) == -4 and call(max_rois=4097) == -4 and call(n_cls=258) == -4 and call(batch=65536) == -4
    torch.cuda.synchronize()
    for k in out:
        assert same_bits(out[k].cpu().numpy(), before[k].cpu().numpy()), k
    with pytest.raises(ValueError, match="both be UNION or neither"):
        aug.merge_boxes(dv, dim, "UNION", "AVG", out=out)
    masks, flipped, cnt, mc = tc.combine_case(28, 2)
    dm, o = [cu(m) for m in masks], torch.full(masks[0].shape, float("nan"), device="cuda")
    dcnt = cu(cnt)
    base = dict(masks=(C.c_void_p * 9)(*[dm[t % 2].data_ptr() for t in range(9)]), flipped=(C.c_int32 * 9)(), n_views=2,
                det_count=dcnt.data_ptr(), mask_class=None, batch=tc.MASK_B, max_out=tc.MAX_OUT, n_cls=tc.K, M=28, heur=0, out=o.data_ptr())
    order = [n for n, _ in aug.SIGNATURES["dtc_aug_combine_masks"][1][:-1]]
    call = lambda **kw: aug.lib().dtc_aug_combine_masks(*[dict(base, **kw)[n] for n in order], None)
    assert call(heur=3) == -1 and call(M=0) == -1 and call(det_count=None) == -1 and call(out=dm[1].data_ptr()) == -1
    assert call(n_views=9) == -4 and call(M=65) == -4 and call(n_cls=1025) == -4 and call(batch=1 << 19) == -4
    torch.cuda.synchronize()
    assert torch.isnan(o).all() and same_bits(dm[1].cpu().numpy(), masks[1])


# ---- (e) graph capture ---------------------------------------------------------------------------------------------------------------
def test_both_entries_replay_from_a_graph_on_rewritten_inputs(aug):
    views, im = tc.merge_case(3, tc.UNION_COUNTS, True, seed=1)
    views2, _ = tc.merge_case(3, tc.UNION_COUNTS[::-1], True, seed=2)
    masks, flipped, cnt, mc = tc.combine_case(28, 2, seed=1)
    masks2, _, _, mc2 = tc.combine_case(28, 2, special=True, seed=2)
    cnt2 = cnt[::-1].copy()
    dv, dim = device_views(views), cu(im)
    dm, dcnt, dmc = [cu(m) for m in masks], cu(cnt), cu(mc)
    out = nan_filled(aug.merge_outputs(tc.B, 3 * tc.R, tc.N_CLS, "cuda"))
    mo = torch.full(masks[0].shape, float("nan"), device="cuda")

    def launch():
        aug.merge_boxes(dv, dim, scores_are_logits=True, out=out)
        aug.combine_masks(dm, flipped, dcnt, dmc, "LOGIT_AVG", out=mo)
    launch()                                                                 # the eager call
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for v, v2 in zip(dv, views2):                                            # rewritten in place
        for k in ("rois5", "n_rois", "cls_score", "bbox_pred", "scale"):
            v[k].copy_(cu(v2[k]))
    for m, m2 in zip(dm, masks2):
        m.copy_(cu(m2))
    dcnt.copy_(cu(cnt2)), dmc.copy_(cu(mc2))
    nan_filled(out), mo.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    replayed, replayed_m = host(out), mo.cpu().numpy()
    nan_filled(out), mo.fill_(float("nan"))
    launch()
    torch.cuda.synchronize()
    eager = host(out)
    for k in eager:
        assert same_bits(replayed[k], eager[k]), k
    assert same_bits(replayed_m, mo.cpu().numpy())
    ref = tr.merge_boxes(views2, im, "UNION", "UNION", True)
    assert same_bits(eager["out_boxes"], ref["out_boxes"]) and same_bits(eager["out_scores"], ref["out_scores"])


# ---- (f) the model level ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_and_images():
    """the randomly initialised Mask R-CNN FPN model and the 320 x 448 blob of tests/test_hip_detector.py, B = 2 raw images of
    200 x 280 (scale 1.6); MIOpen's deterministic algorithms, so that two passes over one blob give the same bits"""
    from detectorch_amd.model.detector import detector
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(0)
    m = detector(arch="resnet50", conv_body_layers=['conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4'],
                 conv_head_layers='two_layer_mlp', fpn_layers=['layer1', 'layer2', 'layer3', 'layer4'], fpn_extra_lvl=True,
                 roi_height=7, roi_width=7, roi_spatial_scale=[0.25, 0.125, 0.0625, 0.03125], roi_sampling_ratio=2,
                 use_rpn_head=True, use_mask_head=True, mask_head_type='1up4convs').cuda()
    m.classif_head.weight.data *= 60.0               # random weights give ~uniform class scores: sharpen them so that detections exist
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    raw = [torch.randint(0, 256, (200, 280, 3), generator=g, device="cuda", dtype=torch.uint8) for _ in range(2)]
    yield m, raw
    torch.backends.cudnn.deterministic = old


def live_rows(path):
    cnt = path.det_count.cpu().numpy()
    return [min(int(c), path.max_out) for c in cnt]


def test_no_views_beyond_the_identity_is_forward_batched(model_and_images):
    from detectorch_amd.utils.blob import images_to_blob
    from detectorch_amd.utils.test_aug import AugOptions
    model, raw = model_and_images
    blob, scales = images_to_blob(raw, target_size=320, max_size=448, fpn_on=True)
    assert tuple(blob.shape) == (2, 3, 320, 448) and scales == pytest.approx([1.6, 1.6])
    sz = torch.tensor([[200.0, 280.0]] * 2, device="cuda")
    model.forward_batched(blob, scales, sz)                                # (warms MIOpen's algorithm choice up)
    pa = model.forward_batched_aug(raw, AugOptions(test_scale=320, test_max_size=448))
    torch.cuda.synchronize()
    got = [t.clone() for t in (pa.dets, pa.det_count, pa.rle_str, pa.rle_str_len, pa.det_roi, pa.det_src)]
    pb = model.forward_batched(blob, scales, sz)
    torch.cuda.synchronize()
    assert pb is not pa and torch.equal(got[1], pb.det_count) and min(live_rows(pb)) > 0
    for b, n in enumerate(live_rows(pb)):
        assert torch.equal(got[0][b, :n], pb.dets[b, :n]) and torch.equal(got[4][b, :n], pb.det_roi[b, :n])
        assert torch.equal(got[3][b, :n], pb.rle_str_len[b, :n]) and torch.equal(got[2][b, :n], pb.rle_str[b, :n])
        assert torch.equal(got[5][b, :n], pb.det_roi[b, :n]) and bool((got[5][b, n:] == -1).all())       # one view: det_src is the row


_AUG_RUNS = {}


def aug_run(model_and_images, heur, method="nms", vote=None):
    """one augmented call (T = 3: the mirrored view, one extra scale, the identity) and everything the checks read back"""
    key = (heur, method, vote)
    if key not in _AUG_RUNS:
        from detectorch_amd.utils.test_aug import AugOptions
        model, raw = model_and_images
        aug = AugOptions(h_flip=True, scales=(256,), max_size=448, test_scale=320, test_max_size=448, mask_heur=heur)
        p = model.forward_batched_aug(raw, aug, **dr.kwargs_of(method, vote))
        torch.cuda.synchronize()
        np_ = lambda t: t.cpu().numpy()
        views = [dict(rois5=np_(v.rois5), n_rois=np_(v.n_rois), cls_score=np_(v.cls_logits_out), bbox_pred=np_(v.bbox_pred_out),
                      scale=np_(v.sf), flipped=f) for v, (_, _, f) in zip(p.aug_views, aug.views())]
        _AUG_RUNS[key] = dict(views=views, flags=[f for _, _, f in aug.views()], dets=np_(p.dets), cnt=np_(p.det_count), roi=np_(p.det_roi),
                              src=np_(p.det_src), masks=np_(p.masks), probs=[np_(m) for m in p.aug_mask_probs], rle=np_(p.rle_str),
                              rle_len=np_(p.rle_str_len), im_size=np_(p.im_size), path=p)
    return _AUG_RUNS[key]


@pytest.mark.parametrize("method,vote", [("nms", None), ("linear", 0.8)])
def test_augmented_detections_are_the_restated_merge_through_the_detection_oracle(model_and_images, oracle, method, vote):
    r = aug_run(model_and_images, "SOFT_AVG", method, vote)
    assert [v["flipped"] for v in r["views"]] == [True, False, False] and r["views"][0]["cls_score"].shape == (2, 1000, 81)
    assert not np.array_equal(r["views"][1]["scale"], r["views"][2]["scale"])
    ref = tr.merge_boxes(r["views"], r["im_size"], logits=True)
    seen = set()
    for b in range(2):
        n = int(ref["out_n"][b])
        dets, roi = dr.compose(oracle, ref["out_scores"][b, :n], ref["out_boxes"][b, :n], method, vote)
        D = dets.shape[0]
        assert 0 < D <= 128 and int(r["cnt"][b]) == D
        assert same_bits(r["dets"][b, :D], dets) and np.array_equal(r["roi"][b, :D], roi)
        assert np.array_equal(r["src"][b, :D], ref["out_src"][b][roi]) and (r["src"][b, D:] == -1).all()
        seen |= set((r["src"][b, :D] // 1000).tolist())
    assert seen == {0, 1, 2}                                               # every view contributes a detection


@pytest.mark.parametrize("heur", ["SOFT_AVG", "SOFT_MAX"])
def test_augmented_masks_are_paste_and_rle_of_the_restated_combination(model_and_images, heur):
    from detectorch_amd import hip
    r = aug_run(model_and_images, heur)
    p = r["path"]
    mc = r["dets"][:, :, 5].astype(np.int32).reshape(-1)
    ref = tr.combine_masks(r["probs"], r["flags"], r["cnt"], mc, heur)
    assert same_bits(r["masks"], ref) and ref.any()
    paste = hip.mask_paste(cu(ref), cu(r["dets"]), cu(r["cnt"]), cu(r["im_size"]), 28, p.crop_capacity)
    rle = hip.mask_rle(paste, cu(r["cnt"]), cu(r["im_size"]), p.rle_runs_stride, p.rle_str_stride)
    torch.cuda.synchronize()
    strs, lens = rle["str"].cpu().numpy(), rle["str_len"].cpu().numpy()
    for b in range(2):
        n = min(int(r["cnt"][b]), 128)
        assert (lens[b, :n] > 0).all() and np.array_equal(lens[b, :n], r["rle_len"][b, :n])
        assert all(strs[b, k, :lens[b, k]].tobytes() == r["rle"][b, k, :lens[b, k]].tobytes() for k in range(n))


def test_augmented_logit_avg_masks_binarise_as_the_float64_rule(model_and_images):
    r = aug_run(model_and_images, "LOGIT_AVG")
    mc = r["dets"][:, :, 5].astype(np.int32).reshape(-1)
    ref64 = tr.combine_masks64(r["probs"], r["flags"], r["cnt"], mc)
    lit = tr.combine_masks(r["probs"], r["flags"], r["cnt"], mc, "LOGIT_AVG", exact=False)
    tol = 2 * np.abs(lit.astype(np.float64) - ref64).max()
    sel = np.zeros(ref64.shape[:2], bool)                                  # the combined (row, channel) pairs
    for b in range(2):
        n = min(int(r["cnt"][b]), 128)
        rows = np.arange(b * 128, b * 128 + n)
        sel[rows, mc[rows]] = True
    got, want = r["masks"][sel], ref64[sel]
    near = np.abs(want - 0.5) <= tol
    print("LOGIT_AVG at the model level: tolerance %.3e, %d of %d pixels within it of 0.5, largest deviation %.3e" % (
        tol, near.sum(), near.size, np.abs(got - want).max()))
    assert sel.any() and tol > 0 and near.mean() <= 1e-3
    assert np.array_equal((got > 0.5)[~near], (want > 0.5)[~near]) and np.abs(got - want).max() <= tol
    assert not r["masks"][~sel].any()


def test_avg_and_id_raise_at_the_model_level(model_and_images):
    from detectorch_amd.utils.test_aug import AugOptions
    model, raw = model_and_images
    for h in ("AVG", "ID"):
        with pytest.raises(NotImplementedError):
            model.forward_batched_aug(raw, AugOptions(score_heur=h, coord_heur=h))
    with pytest.raises(ValueError, match=r"5 views x 1000 rois = 5000"):
        model.forward_batched_aug(raw, AugOptions(h_flip=True, scales=(256, 288, 352), test_scale=320, test_max_size=448))
