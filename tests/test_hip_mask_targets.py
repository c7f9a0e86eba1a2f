"""dtc_mask_targets on the GPU against the numpy restatement (tests/mask_train_ref.py): the integers and mask_rois bit for bit.  Every
output and the workspace start as 0xFF, every output is followed by guard words."""
import numpy as np
import pytest
import torch

import mask_train_ref as mr
from test_mask_train_host import all_cases

pytestmark = pytest.mark.gpu

OUTS = ("mask_rois", "masks", "mask_class", "mask_roi_levels", "roi_has_mask", "n_mask", "mask_gt")
GUARD = 16                                                                   # words behind every output
IN_DTYPES = dict(labels=torch.int32, keep_inds=torch.int32, n_rois=torch.int32, gt_boxes=torch.float32, gt_classes=torch.int32,
                 gt_is_crowd=torch.int32, gt_counts=torch.int32, proposals=torch.float32, im_scale=torch.float32,
                 poly_xy=torch.float32, poly_ptr=torch.int32, gt_poly_ptr=torch.int32)


@pytest.fixture(scope="module")
def cases():
    return all_cases()


def upload(batch):
    return {k: torch.from_numpy(np.ascontiguousarray(batch[k])).to(IN_DTYPES[k]).cuda().contiguous() for k in IN_DTYPES}


def fresh_outputs(B, R, Fm, M, null=()):
    """the output dict of hip_mask.mask_targets, every tensor a view of a 0xFF arena with GUARD words behind it"""
    from detectorch_amd import hip_mask
    shapes = dict(mask_rois=(B, Fm, 5), masks=(B, Fm, M * M), mask_class=(B, Fm), mask_roi_levels=(B, Fm), roi_has_mask=(B, R),
                  n_mask=(B,), mask_gt=(B, Fm))
    out, arenas = {}, {}
    for k, shape in shapes.items():
        n = int(np.prod(shape))
        arenas[k] = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
        view = arenas[k][:n].view(shape)
        out[k] = None if k in null else (view.view(torch.float32) if k == "mask_rois" else view)
    need = hip_mask.lib().dtc_mask_targets_workspace_bytes(B, Fm)
    out["workspace"] = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    return out, arenas


def stale(arenas, out):
    for a in arenas.values():
        a.fill_(-1)
    out["workspace"].fill_(0xFF)


def run(dev, M, k_min, k_max, Fm, null=(), out=None, arenas=None):
    from detectorch_amd import hip_mask
    B, R = dev["labels"].shape
    if out is None:
        out, arenas = fresh_outputs(B, R, Fm, M, null)
    hip_mask.mask_targets(dev["labels"], dev["keep_inds"], dev["n_rois"], dev["gt_boxes"], dev["gt_classes"], dev["gt_is_crowd"],
                          dev["gt_counts"], dev["proposals"], dev["im_scale"], dev["poly_xy"], dev["poly_ptr"], dev["gt_poly_ptr"], M=M,
                          k_min=k_min, k_max=k_max, out=out)
    torch.cuda.synchronize()
    return out, arenas


def snap(out, arenas):
    got = {k: (None if out[k] is None else out[k].cpu().numpy()) for k in OUTS}
    for k, a in arenas.items():
        assert bool((a[-GUARD:] == -1).all()), "guard words behind %s" % k
    return got


def check(got, padded, M, k_min, k_max, Fm, null=()):
    for b, img in enumerate(padded):
        want = mr.targets(img, M, k_min, k_max, Fm, b=b)
        for k in OUTS:
            if k in null:
                continue
            w, q = np.asarray(want[k]), got[k][b]
            assert w.dtype == q.dtype and w.shape == q.shape, k
            if k == "mask_rois" and np.isnan(w).any():                       # a NaN box: NaN where the restatement has NaN
                assert np.array_equal(np.isnan(w), np.isnan(q)) and np.array_equal(w[~np.isnan(w)], q[~np.isnan(w)]), (k, b)
            else:
                assert w.tobytes() == q.tobytes(), (k, b, np.argwhere(w != q)[:5].tolist())


@pytest.mark.parametrize("case", sorted(all_cases()))
def test_case_against_restatement(cases, case):
    img, M, k_min, k_max, Fm = cases[case]
    batch, padded = mr.stack([img], Fm)
    out, arenas = run(upload(batch), M, k_min, k_max, Fm)
    got = snap(out, arenas)
    check(got, padded, M, k_min, k_max, Fm)
    assert set(np.unique(got["masks"]).tolist()) <= {-1, 0, 1}


M14 = ("s14", "garbage", "two_points")


def test_batch_of_three_equals_three_calls(cases):
    """B = 3 (images of different shapes padded to common strides) equals three B = 1 calls on the same padded rows, and the
    restatement"""
    Fm = 8
    batch, padded = mr.stack([cases[n][0] for n in M14], Fm)
    out, arenas = run(upload(batch), 14, 2, 5, Fm)
    got = snap(out, arenas)
    check(got, padded, 14, 2, 5, Fm)
    for b in range(3):
        one = {k: v[b:b + 1] for k, v in batch.items()}
        o1, a1 = run(upload(one), 14, 2, 5, Fm)
        g1 = snap(o1, a1)
        for k in OUTS:
            w = got[k][b].copy()
            if k == "mask_rois":
                w[:, 0] = np.where(np.arange(Fm) < got["n_mask"][b], 0, w[:, 0])      # the batch index of a one-image call is 0
            assert np.array_equal(w, g1[k][0], equal_nan=True), (k, b)


def test_eager_calls_and_graph_replays_are_bit_identical(cases):
    Fm = 8
    batch, padded = mr.stack([cases[n][0] for n in M14], Fm)
    dev = upload(batch)
    out, arenas = fresh_outputs(3, batch["labels"].shape[1], Fm, 14)
    runs = []
    for _ in range(2):
        stale(arenas, out)
        run(dev, 14, 2, 5, Fm, out=out, arenas=arenas)
        runs.append(snap(out, arenas))
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run_args = dict(M=14, k_min=2, k_max=5, out=out)
            from detectorch_amd import hip_mask
            hip_mask.mask_targets(dev["labels"], dev["keep_inds"], dev["n_rois"], dev["gt_boxes"], dev["gt_classes"], dev["gt_is_crowd"],
                                  dev["gt_counts"], dev["proposals"], dev["im_scale"], dev["poly_xy"], dev["poly_ptr"],
                                  dev["gt_poly_ptr"], **run_args)
    for _ in range(2):
        stale(arenas, out)
        graph.replay()
        torch.cuda.synchronize()
        runs.append(snap(out, arenas))
    for other in runs[1:]:
        for k in OUTS:
            assert runs[0][k].tobytes() == other[k].tobytes(), k
    check(runs[0], padded, 14, 2, 5, Fm)
    # inputs rewritten in place: the images in another order, picked up by a replay
    order = [2, 0, 1]
    for k, t in dev.items():
        t.copy_(torch.from_numpy(np.ascontiguousarray(batch[k][order])).to(t.dtype))
    stale(arenas, out)
    graph.replay()
    torch.cuda.synchronize()
    check(snap(out, arenas), [padded[i] for i in order], 14, 2, 5, Fm)


def test_null_optional_outputs(cases):
    img, M, k_min, k_max, Fm = cases["s7"]
    batch, padded = mr.stack([img], Fm)
    null = ("roi_has_mask", "mask_gt")
    out, arenas = run(upload(batch), M, k_min, k_max, Fm, null=null)
    got = snap(out, arenas)
    check(got, padded, M, k_min, k_max, Fm, null=null)
    assert bool((arenas["roi_has_mask"] == -1).all()) and bool((arenas["mask_gt"] == -1).all())


def test_empty_inputs_may_be_null(cases):
    """G = 0 (every gt pointer and the polygon points NULL): rows are kept and match nothing"""
    from detectorch_amd import hip_mask
    i32, f32 = torch.int32, torch.float32
    t = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")
    labels, keep = t([[3, 0, 4]], i32), t([[1, 0, 0]], i32)
    out, arenas = fresh_outputs(1, 3, 2, 7)
    hip_mask.mask_targets(labels, keep, t([3], i32), torch.zeros((1, 0, 4), device="cuda"), torch.zeros((1, 0), dtype=i32, device="cuda"),
                          torch.zeros((1, 0), dtype=i32, device="cuda"), t([0], i32), t([[[1, 2, 30, 40], [5, 6, 70, 80]]], f32),
                          t([1.5], f32), torch.zeros((1, 0, 2), device="cuda"), t([[0]], i32), t([[0]], i32), M=7, k_min=0, k_max=0, out=out)
    torch.cuda.synchronize()
    got = snap(out, arenas)
    assert got["n_mask"].tolist() == [2] and got["mask_class"].tolist() == [[3, 4]] and np.all(got["masks"] == -1)
    assert got["mask_rois"][0].tolist() == [[0, 7.5, 9, 105, 120], [0, 1.5, 3, 45, 60]] and got["roi_has_mask"].tolist() == [[1, 0, 1]]
    assert got["mask_gt"].tolist() == [[-1, -1]]


@pytest.mark.parametrize("bad", [dict(M=57), dict(M=0), dict(k_min=3, k_max=2), dict(short_ws=True), dict(misaligned=True)])
def test_bad_arguments_write_nothing(cases, bad):
    from detectorch_amd import hip_mask
    img, M, k_min, k_max, Fm = cases["s7"]
    batch, _ = mr.stack([img], Fm)
    dev = upload(batch)
    out, arenas = fresh_outputs(1, batch["labels"].shape[1], Fm, M)
    if bad.pop("short_ws", False):
        out["workspace"] = out["workspace"][:-1]
    if bad.pop("misaligned", False):
        whole = torch.full((dev["gt_boxes"].numel() + 1,), 0.0, device="cuda")
        dev["gt_boxes"] = whole[1:].view(dev["gt_boxes"].shape)
    kw = dict(M=M, k_min=k_min, k_max=k_max)
    kw.update(bad)
    with pytest.raises(RuntimeError, match="DTC_E|failed"):
        hip_mask.mask_targets(dev["labels"], dev["keep_inds"], dev["n_rois"], dev["gt_boxes"], dev["gt_classes"], dev["gt_is_crowd"],
                              dev["gt_counts"], dev["proposals"], dev["im_scale"], dev["poly_xy"], dev["poly_ptr"], dev["gt_poly_ptr"],
                              out=out, **kw)
    torch.cuda.synchronize()
    for k, a in arenas.items():
        assert bool((a == -1).all()), k
    assert bool((out["workspace"] == 0xFF).all())


def test_mask_targets_batched_on_a_sampled_minibatch(cases):
    """through sample_rois_batched: mask_rois are the foreground rows of the minibatch's own rois, bit for bit; and the numpy entry"""
    from detectorch_amd.utils.fast_rcnn_sample_rois import sample_rois_batched
    from detectorch_amd.utils.mask_rcnn_targets import add_mask_rcnn_blobs, mask_targets_batched
    img = cases["s14"][0]
    batch, padded = mr.stack([img, cases["s28"][0]], 8)
    dev = upload(batch)
    counts = torch.tensor([10, 10], dtype=torch.int32, device="cuda")
    keys = torch.arange(2 * 14, dtype=torch.int32, device="cuda").reshape(2, 14)
    blobs = sample_rois_batched(dev["proposals"], counts, dev["gt_boxes"], dev["gt_classes"].clamp(min=1), dev["gt_is_crowd"],
                                dev["gt_counts"], dev["im_scale"], rand_keys=keys, rois_per_image=16, fg_thresh=0.3, bg_thresh_hi=0.3,
                                expanded=False)
    mb = mask_targets_batched(blobs, dev["proposals"], dev["gt_boxes"], dev["gt_classes"], dev["gt_is_crowd"], dev["gt_counts"],
                              dev["im_scale"], (dev["poly_xy"], dev["poly_ptr"], dev["gt_poly_ptr"]), M=14, mask_rows=8)
    torch.cuda.synchronize()
    rois, has, n = blobs["rois"].cpu().numpy(), mb["roi_has_mask_int32"].cpu().numpy(), mb["n_mask"].cpu().numpy()
    labels = blobs["labels_int32"].cpu().numpy()
    assert n.min() >= 2
    for b in range(2):
        rows = np.where(has[b] == 1)[0]
        assert len(rows) == n[b] and np.all(labels[b][rows] > 0)
        assert mb["mask_rois"][b, :n[b]].cpu().numpy().tobytes() == rois[b][rows].tobytes()
        assert mb["mask_class_labels"][b, :n[b]].cpu().numpy().tolist() == labels[b][rows].tolist()
        mini = dict(padded[b], labels=labels[b], keep_inds=blobs["keep_inds"][b].cpu().numpy(), n_rois=int(blobs["n_rois"][b]))
        want = mr.targets(mini, 14, 2, 5, 8, b=b)
        assert want["masks"].tobytes() == mb["masks_int32"][b].cpu().numpy().tobytes()
        assert want["mask_roi_levels"].tobytes() == mb["mask_roi_levels"][b].cpu().numpy().tobytes()
    # Detectron's signature for one roidb entry
    polys = [[p.reshape(-1).tolist() for p in (mr.valid_polys(img, q) or [])] for q in range(4)]
    roidb = dict(boxes=img["gt_boxes"], gt_classes=img["gt_classes"], is_crowd=img["gt_is_crowd"], segms=polys)
    one = add_mask_rcnn_blobs(dict(labels_int32=np.array([5, 0, 9], np.int32)), img["proposals"][:3], roidb, 1.5, 3, M=14)
    assert one["mask_rois"].shape == (2, 5) and one["mask_rois"][:, 0].tolist() == [3, 3] and one["roi_has_mask_int32"].tolist() == [1, 0, 1]
    assert one["masks_int32"].shape == (2, 196) and set(np.unique(one["masks_int32"]).tolist()) <= {0, 1}
