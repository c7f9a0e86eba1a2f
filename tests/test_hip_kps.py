"""libdetectorch_kps_hip.so and the model-level keypoint branch on the MI355X against the numpy restatement (tests/kps_ref.py,
tests/README_keypoints.md), on the cases of tests/kps_cases.py, every output pre-filled with NaN (0xFF bytes for integers).

REQUIRED AGREEMENT: x, y, logit and kp_status equal the restatement bit for bit.  prob is within one float32 ulp: both sides add the
same float32 terms in double, any order of which is within (n - 1) 2^-53 <= 2^-29 relative of the exact sum for n <= 2^24, so the two
float32 roundings can differ only at a rounding boundary.  Every comparison prints how many prob values differ at all."""
import functools

import numpy as np
import pytest
import torch

import kps_cases as kc
import kps_ref as kr

pytestmark = pytest.mark.gpu
f32 = np.float32
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4


@pytest.fixture(scope="module")
def kps():
    from detectorch_amd import hip_kps
    hip_kps.lib()
    return hip_kps


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_filled(out):
    for v in out.values():
        v.fill_(float("nan")) if v.is_floating_point() else v.view(torch.uint8).fill_(0xFF)
    return out


def run(kps, heat, dets, cnt, person_class=-1, min_size=0):
    B, D = dets.shape[:2]
    out = nan_filled(kps.keypoint_outputs(B, D, heat.shape[1], "cuda"))
    kps.heatmaps_to_keypoints(cu(heat), cu(dets), cu(cnt), person_class, min_size, out=out)
    torch.cuda.synchronize()
    return out["keyps"].cpu().numpy(), out["kp_status"].cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(K, S, counts, person_class, min_size):
    """computed once per case and shared"""
    heat, dets, cnt = kc.case(K, S, counts)
    ref = kr.heatmaps_to_keypoints(heat, dets, cnt, person_class, min_size)
    for a in ref:
        a.setflags(write=False)
    return ref


def ulps_apart(a, b):
    """float32 arrays -> the distance of each pair in units in the last place (0 for two NaNs, a large number for a NaN and a number)"""
    a, b = np.ascontiguousarray(a, f32).reshape(-1), np.ascontiguousarray(b, f32).reshape(-1)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    d = np.abs(ia - ib)
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na | nb, np.where(na & nb, 0, 1 << 40), d)


def agree(got, ref, what):
    """the required agreement; prints the count of prob values that differ at all"""
    (gk, gs), (rk, rs) = got, ref
    assert gs.tobytes() == rs.tobytes(), (what, gs, rs)
    for c, name in enumerate(("x", "y", "logit")):
        assert gk[:, :, c].tobytes() == rk[:, :, c].tobytes(), (what, name, np.argwhere(gk[:, :, c] != rk[:, :, c])[:5])
    d = ulps_apart(gk[:, :, 3], rk[:, :, 3])
    n = int((rs == 1).sum()) * gk.shape[3]
    print("%s: %d of %d prob values differ from the restatement (largest distance %d ulp)" % (what, int((d != 0).sum()), n, int(d.max())))
    assert d.max() <= 1, (what, np.argwhere(d.reshape(gk[:, :, 3].shape) > 1)[:5])
    dead = rs != 1
    assert not gk[dead].view(np.uint32).any()                   # zeros, +0.0, in every row that is not computed


# ---- (a) the native entry against the restatement -----------------------------------------------------------------------------------
OPTIONS = [(-1, 0), (1, 20)]


@pytest.mark.parametrize("person_class,min_size", OPTIONS + [(1, 0), (-1, 20)])
@pytest.mark.parametrize("counts", kc.COUNTS)
def test_flagship_maps_equal_the_restatement(kps, counts, person_class, min_size):
    """K = 17, S = 56; (0, 5) holds 257 x 130 (five strips of 64 columns, five bands of 32 rows) and 4096 x 1 (the side limit)"""
    heat, dets, cnt = kc.case(17, 56, counts)
    agree(run(kps, heat, dets, cnt, person_class, min_size), reference(17, 56, counts, person_class, min_size),
          "K=17 S=56 counts=%s class=%d min_size=%d" % (counts, person_class, min_size))


@pytest.mark.parametrize("person_class,min_size", OPTIONS)
@pytest.mark.parametrize("counts", kc.COUNTS)
@pytest.mark.parametrize("K,S", kc.MAPS[1:])
def test_small_and_largest_maps_equal_the_restatement(kps, K, S, counts, person_class, min_size):
    heat, dets, cnt = kc.case(K, S, counts)
    agree(run(kps, heat, dets, cnt, person_class, min_size), reference(K, S, counts, person_class, min_size),
          "K=%d S=%d counts=%s class=%d min_size=%d" % (K, S, counts, person_class, min_size))


def test_tie_nan_and_zero_maps(kps):
    heat, dets, cnt = kc.special_case()
    got = run(kps, heat, dets, cnt)
    agree(got, kr.heatmaps_to_keypoints(heat, dets, cnt), "special maps")
    k = got[0][1]
    x1, y1 = dets[1, 0, 0], dets[1, 0, 1]
    assert (k[0, 0, 0], k[0, 1, 0], k[0, 2, 0]) == (x1 + f32(3.5), y1 + f32(2.5), f32(9.0))      # the first of two equal maxima, (2, 3)
    assert (k[0, 0, 1], k[0, 1, 1]) == (x1 + f32(0.5), y1 + f32(1.5)) and np.isnan(k[0, 2, 1]) and np.isnan(k[0, 3, 1])
    assert tuple(k[0, :, 2]) == (x1 + f32(0.5), y1 + f32(0.5), f32(0), f32(1.0 / 49))             # zeros: pos 0
    assert np.isnan(k[1, 2, 0]) and np.isnan(k[1, 3, 0]) and np.isfinite(k[1, :, 1:]).all()       # a NaN in a general upscale
    assert (k[2, 0, 0], k[2, 1, 0]) == (f32(4.5), f32(0.5)) and (k[2, 0, 1], k[2, 1, 1]) == (f32(0.5), f32(0.5)) and np.isnan(k[2, 2, 1])


@pytest.mark.parametrize("min_size", [0, 20])
def test_refused_rows_are_zeros_and_their_neighbours_stay_correct(kps, min_size):
    heat, dets, cnt, want = kc.refused_case()
    got = run(kps, heat, dets, cnt, -1, min_size)
    assert np.array_equal(got[1], want)
    agree(got, kr.heatmaps_to_keypoints(heat, dets, cnt, -1, min_size), "refused rows, min_size=%d" % min_size)
    assert (got[0][want == 1, 3] > 0).all()


def test_argument_refusals_write_nothing(kps):
    """every DTC_EINVAL / DTC_EUNSUPPORTED / DTC_EWORKSPACE arm with valid buffers, which stay NaN-filled"""
    import test_kps_host as th
    heat, dets, cnt = kc.case(3, 7, (6, 3))
    dh, dd, dc = cu(heat), cu(dets), cu(cnt)
    out = nan_filled(kps.keypoint_outputs(2, 6, 3, "cuda"))
    ws = kps.workspace(2, 6, 3, "cuda")
    ws.fill_(0xFF)
    order = [n for n, _ in kps.SIGNATURES["dtc_kps_heatmaps_to_keypoints"][1][:-1]]
    big = dict(heatmaps=dh.data_ptr(), dets=dd.data_ptr(), det_count=dc.data_ptr(), batch=2, max_out=6, K=3, S=7, person_class=-1, min_size=0,
               workspace=ws.data_ptr(), workspace_bytes=ws.numel(), keyps=out["keyps"].data_ptr(), kp_status=out["kp_status"].data_ptr())

    def call(**kw):
        a = dict(big)
        for k, v in kw.items():
            a[k] = (a[k] + (v - th.BOGUS) if isinstance(v, int) and v > th.BOGUS and k in ("keyps", "workspace") else v)
        with torch.cuda.device(0):
            return kps.lib().dtc_kps_heatmaps_to_keypoints(*[a[n] for n in order], torch.cuda.current_stream().cuda_stream)

    for kw in th.EINVAL_ARMS:
        assert call(**kw) == EINVAL, kw
    for kw in th.EUNSUPPORTED_ARMS:
        assert call(**kw) == EUNSUPPORTED, kw
    assert call(workspace_bytes=2 * 6 * 3 * 8 * 16 - 1) == EWORKSPACE
    assert call(batch=0, S=65) == EINVAL and call(S=65, keyps=None) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(out["keyps"]).all()) and bool((out["kp_status"] == -1).all()) and bool((ws == 0xFF).all())
    assert call() == 0                                           # and the same buffers, unrefused, are written completely
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out["keyps"]).any()) and bool((out["kp_status"] == 1).sum() == 9)


def test_graph_replay_picks_up_inputs_rewritten_in_place(kps):
    heat, dets, cnt = kc.case(3, 7, (6, 3))
    heat2, dets2, cnt2 = kc.case(3, 7, (0, 5), seed=5)
    dh, dd, dc = cu(heat), cu(dets), cu(cnt)
    out = nan_filled(kps.keypoint_outputs(2, 6, 3, "cuda"))
    ws = kps.workspace(2, 6, 3, "cuda")

    def launch():
        kps.heatmaps_to_keypoints(dh, dd, dc, 1, 20, out=out, ws=ws)
    launch()                                                     # the eager call
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    dh.copy_(cu(heat2)), dd.copy_(cu(dets2)), dc.copy_(cu(cnt2))                 # rewritten in place
    nan_filled(out), ws.fill_(0xFF)
    g.replay()
    torch.cuda.synchronize()
    replayed = out["keyps"].cpu().numpy(), out["kp_status"].cpu().numpy()
    nan_filled(out), ws.fill_(0xFF)
    launch()
    torch.cuda.synchronize()
    eager = out["keyps"].cpu().numpy(), out["kp_status"].cpu().numpy()
    assert replayed[0].tobytes() == eager[0].tobytes() and replayed[1].tobytes() == eager[1].tobytes()
    agree(replayed, kr.heatmaps_to_keypoints(heat2, dets2, cnt2, 1, 20), "graph replay")
    assert (replayed[1] == 1).sum() > 0


def test_detectron_shaped_entries(kps):
    from detectorch_amd.utils import keypoints as ku
    heat, dets, cnt = kc.case(3, 7, (6, 3))
    rows = [0, 1, 2, 5]
    ref = kr.heatmaps_to_keypoints(heat, dets, cnt)[0][0, rows]
    got = ku.heatmaps_to_keypoints(heat[rows], dets[0, rows, :4])
    assert got.shape == (4, 4, 3) and got[:, :3].tobytes() == ref[:, :3].tobytes() and ulps_apart(got[:, 3], ref[:, 3]).max() <= 1
    cls_boxes = [[], dets[0, rows, :5], []]
    cls_keyps = ku.keypoint_results(cls_boxes, cu(heat[rows]), dets[0, rows, :4], 3)
    assert len(cls_keyps[1]) == 4 and cls_keyps[1][2].tobytes() == got[2].tobytes() and cls_keyps[2] == []
    with pytest.raises(ValueError, match="rows \\[1\\]"):
        ku.heatmaps_to_keypoints(heat[:2], np.array([[0, 0, 5, 5], [0, 0, np.nan, 5]], f32))


# ---- (b) the model level ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deterministic_convs():
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def fpn_model(**kw):
    from detectorch_amd.model.detector import detector
    torch.manual_seed(0)
    return detector(arch='resnet50', conv_body_layers=['conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4'],
                    conv_head_layers='two_layer_mlp', fpn_layers=['layer1', 'layer2', 'layer3', 'layer4'], fpn_extra_lvl=True,
                    roi_height=7, roi_width=7, roi_spatial_scale=[0.25, 0.125, 0.0625, 0.03125], roi_sampling_ratio=2,
                    use_rpn_head=True, **kw).cuda()


def blob():
    g = torch.Generator(device="cuda")
    g.manual_seed(6)
    images = torch.randn(2, 3, 320, 448, generator=g, device="cuda")
    return images, torch.tensor([1.6, 1.6], device="cuda"), torch.tensor([[200.0, 280.0], [200.0, 280.0]], device="cuda")


def test_model_keypoints_equal_the_restatement_on_the_paths_own_heatmaps(deterministic_convs):
    from detectorch_amd.utils import result_utils as ru
    model = fpn_model(N_classes=2, use_keypoint_head=True)
    assert any(k.startswith("keypoint_head.kps_score_lowres") for k in model.state_dict())
    p = model.forward_batched(*blob())
    torch.cuda.synchronize()
    assert tuple(p.kp_heatmaps.shape) == (2 * p.max_out, 17, 56, 56) and tuple(p.keyps.shape) == (2, p.max_out, 4, 17)
    heat, dets, cnt = p.kp_heatmaps.cpu().numpy(), p.dets.cpu().numpy(), p.det_count.cpu().numpy()
    got = p.keyps.cpu().numpy(), p.kp_status.cpu().numpy()
    assert (got[1] == 1).sum(1).min() >= 1 and np.array_equal((got[1] == 1).sum(1), np.minimum(cnt, p.max_out))   # two classes: every row is a person
    # the restatement on a few rows of each image (all of them would take the host a minute): the first, the last, the largest
    keep = np.zeros(got[1].shape, bool)
    for b in range(2):
        n = int(min(cnt[b], p.max_out))
        area = (dets[b, :n, 2] - dets[b, :n, 0]) * (dets[b, :n, 3] - dets[b, :n, 1])
        keep[b, [0, n - 1, int(np.argmax(area)), int(np.argmin(area))]] = True
    sub_dets = dets.copy()
    sub_dets[~keep, 5] = 0                                        # person_class = 1 then skips the rows that are not compared
    ref = kr.heatmaps_to_keypoints(heat, sub_dets, cnt, person_class=1)
    sub = np.where(keep[:, :, None, None], got[0], 0).astype(f32), np.where(keep, got[1], 0).astype(np.int32)
    agree(sub, ref, "model level")
    boxes, _, keyps = ru.assemble_results(p.dets, p.det_count, num_classes=2, keyps=p.keyps, kp_status=p.kp_status)
    for b in range(2):
        assert len(keyps[1][b]) == int(cnt[b]) == boxes[1][b].shape[0] and keyps[1][b][0].tobytes() == got[0][b, 0].tobytes()
    res = ru.coco_keypoint_results(boxes[1], keyps[1], [7, 9], 1, 'prob')
    assert len(res) == int(cnt.sum()) and all(0 < r["score"] <= 1 and len(r["keypoints"]) == 51 for r in res)


def test_head_off_is_the_model_without_it(deterministic_convs):
    """a model with the keypoint head and one without, built from the same seed: same dets, counts and RLE strings, and the model
    without has no keypoint weights and leaves no keypoint result on its path"""
    sharpen = lambda m: (m.classif_head.weight.data.mul_(60.0), m)[1]
    off = sharpen(fpn_model(use_mask_head=True, mask_head_type='1up4convs'))
    on = sharpen(fpn_model(use_mask_head=True, mask_head_type='1up4convs', use_keypoint_head=True))
    assert not [k for k in off.state_dict() if "keypoint" in k] and not hasattr(off, "keypoint_head")
    assert [k for k in on.state_dict() if "keypoint" not in k] == list(off.state_dict())
    a, b = off.forward_batched(*blob()), on.forward_batched(*blob())
    torch.cuda.synchronize()
    assert not hasattr(a, "keyps") and min(a.det_count.tolist()) > 0
    for name in ("dets", "det_count", "rle_str", "rle_str_len"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    st = b.kp_status.cpu().numpy()
    cls = b.dets.cpu().numpy()[:, :, 5]
    live = np.arange(b.max_out)[None, :] < np.minimum(b.det_count.cpu().numpy(), b.max_out)[:, None]
    assert np.array_equal(st, (live & (cls == 1)).astype(np.int32))


def test_other_configurations_raise():
    from detectorch_amd.model.detector import detector
    torch.manual_seed(0)
    c4 = detector(arch='resnet50', use_rpn_head=True, use_keypoint_head=True).cuda()
    with pytest.raises(NotImplementedError, match="keypoint head covers the FPN models"):
        c4.forward_batched(torch.zeros(1, 3, 64, 64, device="cuda"), [1.0], [[64.0, 64.0]])
    m = fpn_model(N_classes=2, use_keypoint_head=True, head_dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="keypoint head covers the FPN models"):
        m.forward_batched(*blob())
