"""The flip augmentation on the MI355X (-m gpu; tests/README_flip.md): dtc_flip_prep_images, dtc_flip_boxes, dtc_flip_polygons and
dtc_flip_rle against the numpy restatements of tests/flip_ref.py, and one training step of each joint model on a device-flipped batch
against the same step on a host-flipped one.  Every comparison is bitwise."""
import contextlib

import numpy as np
import pytest
import torch

import flip_cases as fc
import flip_ref as fr
from detectorch_amd import synth

pytestmark = pytest.mark.gpu


def d(a, t=None):
    x = torch.as_tensor(np.ascontiguousarray(a))
    return x.to("cuda") if t is None else x.to("cuda", t)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the network input ------------------------------------------------------------------------------------------------------------------------
PREP_SIZES = ((1, 1), (5, 1), (1, 7), (5, 7), (13, 9))
PREP_TARGETS = ((24, 1000), (3, 1000), (20, 26))              # upscale; downscale; max_size caps the scale of every oblong image


def _images(rs, dtype):
    if dtype == np.uint8:
        return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in PREP_SIZES]
    return [rs.uniform(0, 255, (h, w, 3)).astype(np.float32) for h, w in PREP_SIZES]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_prep_single_images(oracle, dtype):
    from detectorch_amd import hip, hip_flip
    rs = synth.rng(91, 0)
    capped = 0
    for im in _images(rs, dtype):
        for target, mx in PREP_TARGETS:
            want, scales = oracle.prep_images([fr.flip_image(im)], target_size=target, max_size=mx, pad_stride=1)
            capped += scales[0] != target / min(im.shape[:2])
            t = d(im)
            got, got_scales, _ = hip_flip.prep_images([t], [1], target_size=target, max_size=mx, pad_stride=1)
            assert got_scales == scales and same(got.cpu().numpy(), want), (im.shape, target, mx)
            base, _, _ = hip.prep_images([torch.flip(t, [1])], target_size=target, max_size=mx, pad_stride=1)
            assert torch.equal(got, base)
    assert capped >= 2


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_prep_strided_view(oracle, dtype):
    """a 13 x 9 view with row_stride > 3 w: the columns 2 .. 10 of a 13 x 14 image"""
    from detectorch_amd import hip_flip
    rs = synth.rng(91, 1)
    wide = rs.randint(0, 256, (13, 14, 3)).astype(dtype)
    view = d(wide)[:, 2:11]
    assert view.stride(0) == 42 and not view.is_contiguous()
    for target, mx in PREP_TARGETS:
        want, _ = oracle.prep_images([fr.flip_image(wide[:, 2:11])], target_size=target, max_size=mx, pad_stride=1)
        got, _, _ = hip_flip.prep_images([view], [1], target_size=target, max_size=mx, pad_stride=1)
        assert same(got.cpu().numpy(), want), (target, mx)


def test_prep_batch_of_three_sizes(oracle):
    from detectorch_amd import hip
    from detectorch_amd.utils import blob as blob_utils
    rs = synth.rng(91, 2)
    ims = [rs.randint(0, 256, (13, 9, 3)).astype(np.uint8), rs.uniform(0, 255, (5, 7, 3)).astype(np.float32),
           rs.randint(0, 256, (9, 21, 3)).astype(np.uint8)]
    flags = (1, 0, 1)
    host = [fr.flip_image(im) if f else im for im, f in zip(ims, flags)]
    for target, mx in ((24, 50), (6, 50)):
        got, scales = blob_utils.images_to_blob(ims, target_size=target, max_size=mx, fpn_on=True, flipped=flags)
        want, want_scales = oracle.prep_images(host, target_size=target, max_size=mx, pad_stride=32)
        assert scales == want_scales and got.shape[2] % 32 == 0 and got.shape[3] % 32 == 0
        assert same(got.cpu().numpy(), want)
        ts = [d(im) for im in ims]
        base, _, sizes = hip.prep_images([torch.flip(t, [1]) if f else t for t, f in zip(ts, flags)], target_size=target, max_size=mx, pad_stride=32)
        assert torch.equal(got, base)
        for b, (oh, ow) in enumerate(sizes):                     # the padding is zero, and it is on the right and below
            assert float(got[b, :, oh:].abs().max()) == 0.0 and float(got[b, :, :, ow:].abs().max()) == 0.0
            assert float(got[b, :, :oh, :ow].abs().max()) > 0.0
        today, _, _ = hip.prep_images(ts, target_size=target, max_size=mx, pad_stride=32)
        assert torch.equal(got[1], today[1]) and not torch.equal(got[0], today[0])           # the unflipped image: today's output
        for none in (None, (0, 0, 0), [False] * 3):               # no flag set: hip.prep_images' blob
            assert torch.equal(blob_utils.images_to_blob(ims, target_size=target, max_size=mx, fpn_on=True, flipped=none)[0], today)
    from detectorch_amd import hip_flip
    assert torch.equal(hip_flip.prep_images(ts, [0, 0, 0], target_size=6, max_size=50)[0], today)      # the flip kernel itself, no flag set
    with pytest.raises(ValueError):
        blob_utils.images_to_blob(ims, flipped=(1, 0))


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [4, 8])
def test_flip_boxes(cols):
    from detectorch_amd import hip_flip
    from detectorch_amd.utils import boxes as box_utils
    boxes = fc.box_case(cols)
    widths = d(np.array(fc.BOX_WIDTHS, np.int32))
    for flags in fc.BOX_FLAGS:
        for counts in (None, fc.BOX_COUNTS, (fc.BOX_R, 0, 2)):
            want = fr.flip_boxes_batched(boxes, fc.BOX_WIDTHS, flags, counts)
            src = d(boxes)
            got = hip_flip.flip_boxes(src, widths, flags, counts=None if counts is None else d(np.array(counts, np.int32)))
            assert same(got.cpu().numpy(), want) and same(src.cpu().numpy(), boxes), (flags, counts)      # out of place: the input stays
            inplace = hip_flip.flip_boxes(src, widths, d(np.array(flags, np.int32)), counts=None if counts is None else d(np.array(counts, np.int32)),
                                          out=src)
            assert inplace is src and same(src.cpu().numpy(), want), (flags, counts)
            if counts is not None:                                # rows past the count and images that are not flipped: untouched
                for b in range(3):
                    n = counts[b] if flags[b] else 0
                    assert same(want[b, n:], boxes[b, n:])
    assert not same(fr.flip_boxes_batched(boxes, fc.BOX_WIDTHS, (1, 1, 1)), boxes)
    # the reference's signature, numpy in / numpy out
    for b, w in enumerate(fc.BOX_WIDTHS):
        assert same(box_utils.flip_boxes(boxes[b], w), fr.flip_boxes(boxes[b], w))
    assert box_utils.flip_boxes(np.zeros((0, cols), np.float32), 640).shape == (0, cols)


# ---- polygons ---------------------------------------------------------------------------------------------------------------------------------
def test_flip_polygons():
    from detectorch_amd import hip_flip
    from detectorch_amd.utils.mask_rcnn_targets import pack_polygons
    from detectorch_amd.utils.segms import pack_polygons64
    kw = dict(points=fc.POLY_PTS, polys=fc.POLY_NP)
    xy, ptr, gptr = pack_polygons64(fc.POLYS, fc.POLY_G, "cuda", **kw)
    widths = d(np.array(fc.POLY_WIDTHS, np.int32))
    assert xy[0, 0, 0].item() == 639.49 and xy[0, 1, 0].item() == 100.1 and int(ptr[0, -1]) < fc.POLY_PTS          # padding behind the points
    for flags in fc.POLY_FLAGS:
        host = fr.flip_polys_per_image(fc.POLYS, fc.POLY_WIDTHS, flags)
        want64 = pack_polygons64(host, fc.POLY_G, **kw)[0].numpy()
        want32 = pack_polygons(host, fc.POLY_G, **kw)[0].numpy()
        both = hip_flip.flip_polygons(xy, ptr, widths, flags)
        only64 = hip_flip.flip_polygons(xy, ptr, widths, flags, want32=False)
        only32 = hip_flip.flip_polygons(xy, ptr, widths, d(np.array(flags, np.int32)), want64=False)
        assert only64[1] is None and only32[0] is None
        for got64 in (both[0], only64[0]):
            assert same(got64.cpu().numpy(), want64), flags      # pack(host-flipped lists) == flip(pack(lists)), padding included
        for got32 in (both[1], only32[1]):
            assert same(got32.cpu().numpy(), want32), flags
        for b in range(3):                                        # padding points and images that are not flipped: copied
            n = int(ptr[b, -1]) if flags[b] else 0
            assert same(both[0][b, n:].cpu().numpy(), xy[b, n:].cpu().numpy())
            assert same(both[1][b, n:].cpu().numpy(), xy[b, n:].cpu().numpy().astype(np.float32))
        assert same(both[0][:, :, 1].cpu().numpy(), xy[:, :, 1].cpu().numpy())                  # y
    got32 = hip_flip.flip_polygons(xy, ptr, widths, (1, 1, 1), want64=False)[1]
    assert got32[0, 0, 0].item() == np.float32(-0.49) != np.float32(640) - np.float32(639.49) - np.float32(1)
    inplace = xy.clone()
    assert hip_flip.flip_polygons(inplace, ptr, widths, (1, 1, 1), want32=False, out64=inplace)[0] is inplace
    assert torch.equal(inplace, hip_flip.flip_polygons(xy, ptr, widths, (1, 1, 1), want32=False)[0])
    with pytest.raises(ValueError):
        hip_flip.flip_polygons(xy, ptr, widths, (1, 1, 1), want64=False, want32=False)


def test_mask_targets_on_device_flipped_polygons():
    """mask_targets_batched on the device-flipped f32 tensors equals the same call on pack_polygons(host-flipped lists)"""
    from detectorch_amd import hip_flip
    from detectorch_amd.utils.mask_rcnn_targets import mask_targets_batched, pack_polygons
    from detectorch_amd.utils.segms import pack_polygons64
    polys = [[[[20.3, 6, 48, 6.7, 60, 18, 60.49, 38, 48, 50, 20, 50, 8, 38.2, 8, 18]], [[40, 20, 90.1, 40, 40, 60], [60, 30, 85, 30, 85, 55.5, 60, 55]]]]
    W = 96
    boxes = np.array([[[8, 6, 60.49, 50], [40, 20, 90.1, 60]]], np.float32)
    flipped_boxes = d(fr.flip_boxes_batched(boxes, [W], [1]))
    i32 = torch.int32
    rois = torch.cat([flipped_boxes, flipped_boxes + d(np.array([2, -1, 3, 2], np.float32))], 1).contiguous()      # [1, 4, 4]: the gt and near copies
    mini = dict(labels_int32=d([[1, 3, 1, 3]], i32), keep_inds=d([[0, 1, 2, 3]], i32), n_rois=d([4], i32))
    args = (mini, rois, flipped_boxes, d([[1, 3]], i32), d([[0, 0]], i32), d([2], i32), d([1.0], torch.float32))
    xy, ptr, gptr = pack_polygons64(polys, 2, "cuda")
    dev32 = hip_flip.flip_polygons(xy, ptr, d(np.array([W], np.int32)), [1], want64=False)[1]
    host = pack_polygons(fr.flip_polys_per_image(polys, [W], [1]), 2, device="cuda")
    assert torch.equal(dev32, host[0])
    got = mask_targets_batched(*args, (dev32, ptr, gptr), M=14, k_min=0, k_max=0)
    want = mask_targets_batched(*args, host, M=14, k_min=0, k_max=0)
    for k in ("mask_rois", "masks_int32", "mask_class_labels", "roi_has_mask_int32", "n_mask"):
        assert torch.equal(got[k], want[k]), k
    assert int(got["n_mask"][0]) == 4 and int((got["masks_int32"] == 1).sum()) > 0


# ---- run lists --------------------------------------------------------------------------------------------------------------------------------
def _rle_check(res, lists, out_n, need, where=""):
    got_n, got_need = res["out_n_runs"].cpu().numpy(), res["need"].cpu().numpy()
    assert got_n.tolist() == out_n.tolist() and got_need.tolist() == need.tolist(), (where, got_n.tolist(), out_n.tolist(), got_need.tolist())
    runs = res["out_runs"].cpu().numpy().view(np.uint32)
    for n, per in enumerate(lists):
        for r, row in enumerate(per):
            if row is not None:
                assert runs[n, r, :len(row)].tolist() == row, (where, n, r)


def test_flip_rle_single_masks():
    """every mask of flip_cases.rle_rows(), one call per mask"""
    from detectorch_amd import hip_flip
    rows = fc.rle_rows()
    for name, h, w, row in rows:
        runs, n = fc.pack_runs([row], len(row) + 3)
        want = fr.flip_rle_batched(runs, n, [(h, w)], [1], 3 * len(row) + 1)
        res = hip_flip.flip_rle(d(runs), d(n), d(np.array([[h, w]], np.float32)), [1], out_stride=3 * len(row) + 1)
        _rle_check(res, *want, where=name)
        assert want[1][0, 0] == len(fr.flip_rle_runs(row, h, w)) >= 1
    # single row: the runs reverse; single column: the identity; the growth case
    by = {name: (h, w, row) for name, h, w, row in rows}
    assert fr.flip_rle_runs(by["3x4 growth"][2], 3, 4) == [3, 1, 4, 1, 3] and len(by["4x5 checkerboard"][2]) == 16
    assert len(by["5x4 checkerboard, h w + 1 runs"][2]) == len(by["4x5 stripes, h w + 1 runs"][2]) == 4 * 5 + 1       # every pixel a run, and the leading 0
    assert len(by["300 runs, more than one chunk"][2]) > 256


def test_flip_rle_rows_states_and_capacity():
    """one 5 x 7 image and one 3 x 4 image, mixed flags: rows with n_runs = -1, a wrong sum, no segmentation, rows past the count; an
    out_stride one short of what a row needs"""
    from detectorch_amd import hip_flip
    first = fr.encode(np.arange(35).reshape(7, 5).T % 3 == 0)
    a_rows = [first, [35], [0, 35], [4, 3, 0, 2, 26], [10, 5, 19], [0, 0, 4, 0, 0, 3, 0, 2, 6, 0, 20, 0], [35], [7, 28]]
    b_rows = [[5, 2, 5], [5, 2, 5], [12], [0, 12], [5, 2, 4], [], [1, 11], [12]]
    S = max(len(r) for r in a_rows + b_rows) + 2
    ra, na = fc.pack_runs(a_rows, S, {1: -1})
    rb, nb = fc.pack_runs(b_rows, S, {1: -7})
    runs, n = np.concatenate([ra, rb]), np.concatenate([na, nb])
    sizes = np.array([[5, 7], [3, 4]], np.float32)
    counts = np.array([7, 6], np.int32)
    for flags in ((1, 1), (1, 0), (0, 1), (0, 0)):
        for out_stride in (64, 4, 5):                            # 4: one short of the growth case's 5, and of `first`'s need
            for cnt in (None, counts):
                want = fr.flip_rle_batched(runs, n, sizes, flags, out_stride, cnt)
                poison = dict(out_runs=torch.full((2, 8, out_stride), -7, dtype=torch.int32, device="cuda"),
                              out_n_runs=torch.full((2, 8), -7, dtype=torch.int32, device="cuda"),
                              need=torch.full((2, 8), -7, dtype=torch.int32, device="cuda"))
                res = hip_flip.flip_rle(d(runs), d(n), d(sizes), flags, counts=None if cnt is None else d(cnt), out=poison)
                assert res is poison
                if cnt is not None:                               # rows past the count are not written, in any output
                    for b in range(2):
                        for k in res:
                            assert bool((res[k][b, cnt[b]:] == -7).all()), (k, flags, out_stride)
                        want[1][b, cnt[b]:] = -7
                        want[2][b, cnt[b]:] = -7
                _rle_check(res, *want, where=(flags, out_stride, cnt is not None))
    want = fr.flip_rle_batched(runs, n, sizes, (1, 1), 4)
    assert want[1][1].tolist() == [-1, -1, 1, 2, -1, 0, 4, 1] and want[2][1].tolist() == [5, 0, 1, 2, 0, 0, 4, 1]       # need exact where it did not fit
    # rows that do not fit leave their neighbours intact: checked above; the default out_stride is runs_stride
    assert hip_flip.flip_rle(d(runs), d(n), d(sizes), (1, 1))["out_runs"].shape == (2, 8, S)
    with pytest.raises(RuntimeError, match="DTC_EINVAL"):          # out_runs must not be runs
        t = d(runs)
        hip_flip.flip_rle(t, d(n), d(sizes), (1, 1), out=dict(out_runs=t, out_n_runs=d(n).clone(), need=d(n).clone()))


def test_flip_rle_large_mask_and_graph_replay():
    from detectorch_amd import hip_flip
    h, w = fc.BLOB_HW
    row = fc.blob_runs()
    want = fr.flip_rle_runs(row, h, w)
    assert 65 <= len(row) <= 4096 and 65 <= len(want) <= 4096
    S = 1024
    runs, n = fc.pack_runs([row, want, [h * w], row], S)
    sizes, flags = d(np.array([[h, w]], np.float32)), d(np.array([1], np.int32))
    t_runs, t_n = d(runs), d(n)
    res = hip_flip.flip_rle(t_runs, t_n, sizes, flags)
    lists = [[want, row, [h * w], want]]                          # flip(flip(x)) == x
    _rle_check(res, lists, np.array([[len(x) for x in lists[0]]]), np.array([[len(x) for x in lists[0]]]))
    back = hip_flip.flip_rle(res["out_runs"], res["out_n_runs"], sizes, flags)
    _rle_check(back, [[row, want, [h * w], row]], n, n)
    got = res["out_runs"][0, 0, :len(want)].cpu().numpy().view(np.uint32)
    assert int(got[1::2].sum()) == sum(row[1::2])                 # area preserved
    # capture and replay after the eager call: the same bits, and a replay picks up inputs rewritten in place
    out = hip_flip.rle_outputs(1, 4, S, "cuda")
    ws = torch.empty(hip_flip.rle_workspace_bytes(1, 4, S), dtype=torch.uint8, device="cuda")
    hip_flip.flip_rle(t_runs, t_n, sizes, flags, out=out, ws=ws)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip_flip.flip_rle(t_runs, t_n, sizes, flags, out=out, ws=ws)
    for k in out:
        out[k].fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    for k in ("out_n_runs", "need"):
        assert torch.equal(out[k], res[k]), k
    for r in range(4):
        m = int(res["out_n_runs"][0, r])
        assert torch.equal(out["out_runs"][0, r, :m], res["out_runs"][0, r, :m])
    flags.zero_()                                                 # not flipped: the replay copies the rows
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["out_n_runs"], t_n) and torch.equal(out["out_runs"][0, 0, :len(row)], t_runs[0, 0, :len(row)])


def test_flip_rle_more_than_65536_runs():
    """a 401 x 367 mask of random pixels: over 65536 runs in one row, hundreds of chunks with carried scan state in both passes; beside
    it a row of one run per column block (a background run over every column is three pieces, whatever the width)"""
    from detectorch_amd import hip_flip
    h, w = 401, 367
    m = np.random.RandomState(7).rand(h, w) < 0.5
    row = fr.encode(m)
    assert len(row) > 65536
    want = fr.flip_rle_runs(row, h, w)
    S = max(len(row), len(want)) + 1
    wide = [3 * h + 5, 2, h * w - 3 * h - 7]                       # two pixels deep inside: long runs over many columns
    runs, n = fc.pack_runs([row, wide, want], S)
    res = hip_flip.flip_rle(d(runs), d(n), d(np.array([[h, w]], np.float32)), [1])
    lists = [[want, fr.flip_rle_runs(wide, h, w), row]]
    counts = np.array([[len(x) for x in lists[0]]])
    _rle_check(res, lists, counts, counts)


def test_flip_segms_and_extend_with_flipped_entries():
    from detectorch_amd.utils import augment, result_utils as ru, segms
    m = fr.blob_mask(np.random.RandomState(5), 40, 60, blobs=3)
    poly = [[10.5, 5.0, 50.25, 5.0, 30.0, 35.5]]
    rles = [dict(size=[40, 60], counts=ru.rle_counts(m)), ru.rle_encode(m), dict(size=[40, 60], counts=ru.rle_encode(m)["counts"].encode())]
    got = segms.flip_segms([poly, rles[0], rles[1], [], rles[2]], 40, 60)
    want = ru.rle_encode(m[:, ::-1])
    assert got[0] == [fr.flip_poly(poly[0], 60)] and got[3] == [] and got[1] == got[2] == got[4] == want
    assert ru.rle_string_to_counts(got[1]["counts"]) == fr.flip_rle_runs(ru.rle_counts(m), 40, 60)
    grow = segms.flip_segms([dict(size=[3, 4], counts=[5, 2, 5])], 3, 4)[0]                     # longer than its input: the second call
    assert ru.rle_string_to_counts(grow["counts"]) == [3, 1, 4, 1, 3]
    with pytest.raises(ValueError):
        segms.flip_segms([dict(size=[3, 4], counts=[5, 2, 4])], 3, 4)
    boxes = np.array([[10.5, 5, 50.25, 35.5], [0, 0, 59, 39]], np.float32)
    roidb = [dict(boxes=boxes, segms=[poly, rles[0]], width=60, height=40, gt_classes=np.array([1, 2]), image="a.jpg"),
             dict(boxes=np.zeros((0, 4), np.float32), segms=[], width=7, height=5, gt_classes=np.zeros(0), image="b.jpg", flipped=False)]
    extra = augment.extend_with_flipped_entries(roidb)
    assert [e['flipped'] for e in roidb] == [False, False] and [e['flipped'] for e in extra] == [True, True] and len(extra) == 2
    assert same(extra[0]['boxes'], fr.flip_boxes(boxes, 60)) and same(roidb[0]['boxes'], boxes) and extra[1]['boxes'].shape == (0, 4)
    assert extra[0]['segms'] == [[fr.flip_poly(poly[0], 60)], want] and extra[0]['gt_classes'] is roidb[0]['gt_classes']
    assert extra[0]['image'] == "a.jpg" and extra[1]['segms'] == []
    with pytest.raises(AssertionError):                           # x2' >= x1', as the reference asserts
        augment.extend_with_flipped_entries([dict(boxes=np.array([[9, 0, 3, 5]], np.float32), segms=[[]], width=60, height=40)])


def test_flip_batch_runs_and_proposals():
    from detectorch_amd.utils import augment
    from detectorch_amd.utils.evaluator import pack_gt_masks
    m = fr.blob_mask(np.random.RandomState(6), 40, 60, blobs=3)
    gt = pack_gt_masks([[m, None, np.zeros((40, 60), bool)], [np.eye(5, 7, dtype=bool)]], [(40, 60), (5, 7)], "cuda")
    gt["gt_boxes"] = d(np.array([[[1, 2, 30.5, 20], [0, 0, 59, 39], [5, 5, 6, 6]], [[0, 1, 6, 4], [9, 9, 9, 9], [9, 9, 9, 9]]], np.float32))
    gt["gt_counts"] = d(np.array([3, 1], np.int32))
    gt["proposals"] = d(np.arange(2 * 5 * 4, dtype=np.float32).reshape(2, 5, 4) % 7)
    gt["proposal_counts"] = d(np.array([5, 2], np.int32))
    gt["gt_classes"] = d(np.array([[1, 2, 3], [1, 0, 0]], np.int32))
    flags, widths, heights = (1, 1), (60, 7), (40, 5)
    out = augment.flip_batch(gt, flags, widths, im_height=heights)
    assert out["gt_classes"] is gt["gt_classes"] and out["gt_counts"] is gt["gt_counts"] and out is not gt
    assert same(out["gt_boxes"].cpu().numpy(), fr.flip_boxes_batched(gt["gt_boxes"].cpu().numpy(), widths, flags, (3, 1)))
    assert same(out["proposals"].cpu().numpy(), fr.flip_boxes_batched(gt["proposals"].cpu().numpy(), widths, flags, (5, 2)))
    want = pack_gt_masks([[m[:, ::-1], None, np.zeros((40, 60), bool)], [np.eye(5, 7, dtype=bool)[:, ::-1]]], [(40, 60), (5, 7)], "cpu")
    n = want["gt_n_runs"].numpy()
    assert out["gt_n_runs"].cpu().numpy().tolist() == n.tolist()
    for b in range(2):
        for r in range(n.shape[1]):
            assert same(out["gt_runs"][b, r, :n[b, r]].cpu().numpy(), want["gt_runs"][b, r, :n[b, r]].numpy())
    fixed = augment.flip_batch(gt, d(np.array(flags, np.int32)), d(np.array(widths, np.int32)), im_height=heights, rle_out_stride=3)
    assert fixed["gt_runs"].shape[2] == 3 and fixed["gt_n_runs"].cpu().numpy().tolist() == np.where(n > 3, -1, n).tolist()
    with pytest.raises(ValueError):
        augment.flip_batch(gt, flags, widths)


# ---- end to end: one training step on a device-flipped batch == the step on a host-flipped batch ----------------------------------------------
@contextlib.contextmanager
def deterministic_framework():
    """The framework's convolutions are not run-to-run reproducible by default on this GPU: two steps on the SAME tensors differ in
    the last bits of the losses (measured: loss_rpn_cls 0x1.72309ap+0 / 0x1.72309cp+0).  Its deterministic mode makes them so, and a
    bitwise comparison of two steps means something; the settings are put back afterwards."""
    saved = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark, torch.are_deterministic_algorithms_enabled(),
             torch.is_deterministic_algorithms_warn_only_enabled())
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved[:2]
        torch.use_deterministic_algorithms(saved[2], warn_only=saved[3])


def _host_flipped(gt, polys, G, flags, widths):
    """the gt dict flipped on the host by flip_ref"""
    from detectorch_amd.utils.mask_rcnn_targets import pack_polygons
    out = dict(gt)
    out["gt_boxes"] = d(fr.flip_boxes_batched(gt["gt_boxes"].cpu().numpy(), widths, flags, gt["gt_counts"].cpu().numpy()))
    if polys is not None:
        out["poly_xy"], out["poly_ptr"], out["gt_poly_ptr"] = pack_polygons(fr.flip_polys_per_image(polys, widths, flags), G, device="cuda")
    return out


def _device_flipped(gt, polys, G, flags, widths):
    from detectorch_amd.utils import augment
    from detectorch_amd.utils.mask_rcnn_targets import pack_polygons
    from detectorch_amd.utils.segms import pack_polygons64
    src = dict(gt)
    if polys is not None:
        src["poly_xy"], src["poly_ptr"], src["gt_poly_ptr"] = pack_polygons(polys, G, device="cuda")
        src["poly_xy64"] = pack_polygons64(polys, G, device="cuda")[0]
    out = augment.flip_batch(src, flags, widths)
    out.pop("poly_xy64", None)
    return out


def test_mask_rcnn_train_step_on_a_flipped_batch():
    """the small C4 model and shapes of tests/test_hip_mask_train_step.py"""
    from detectorch_amd.model.detector import detector
    from detectorch_amd.optim import ClippedSGD
    from detectorch_amd.train import freeze_stem, mask_rcnn_train_step
    from detectorch_amd.utils import blob as blob_utils
    from test_hip_rpn_train_step import inputs
    rs, _, gt = inputs(3)
    gt["rand_keys"] = d(rs.randint(0, 2 ** 31 - 1, (1, 2 + 300)), torch.int32)
    polys = [[[[20.3, 6, 48, 6, 60, 18, 60, 38, 48, 50.7, 20, 50, 8, 38, 8, 18]], [[40, 20, 90.1, 40, 40, 60], [60, 30, 85, 30, 85, 55, 60, 55]]]]
    image = rs.randint(0, 256, (64, 96, 3)).astype(np.uint8)
    flags, widths = (1,), (96,)
    kw = dict(target_size=64, max_size=96)
    dev_blob, scales = blob_utils.images_to_blob([image], flipped=flags, **kw)
    host_blob, _ = blob_utils.images_to_blob([fr.flip_image(image)], **kw)
    assert scales == [1.0] and tuple(dev_blob.shape) == (1, 3, 64, 96) and torch.equal(dev_blob, host_blob)
    host_blob = d(np.ascontiguousarray(torch.flip(blob_utils.images_to_blob([image], **kw)[0], [3]).cpu().numpy()))      # scale 1: torch.flip of the blob
    assert torch.equal(dev_blob, host_blob)
    results = []
    for blob, batch in ((dev_blob, _device_flipped(gt, polys, 2, flags, widths)), (host_blob, _host_flipped(gt, polys, 2, flags, widths))):
        torch.manual_seed(9)
        model = detector(N_classes=5, use_rpn_head=True, use_mask_head=True).cuda()
        opt = ClippedSGD(freeze_stem(model), lr=0.01)
        torch.manual_seed(1234)                                   # the RPN minibatch draws its keys from the seeded generator
        with deterministic_framework():
            out = mask_rcnn_train_step(model, opt, blob, batch, it=0, rpn_knobs=dict(batch_size_per_im=16), post_nms_top_n=300, rois_per_image=16)
            torch.cuda.synchronize()
        results.append(torch.stack([v.detach().reshape(()) for v in out[:5]]).cpu().numpy())
    print("losses on the device-flipped batch %r, on the host-flipped batch %r" % (results[0].tolist(), results[1].tolist()))
    assert np.isfinite(results[0]).all() and results[0][4] > 0 and same(results[0], results[1])


def test_faster_rcnn_train_step_on_a_flipped_fpn_batch():
    """the FPN model and shapes of tests/test_hip_fpn_train_step.py: a 480 x 512 image at scale 1 and a 560 x 640 one that max_size
    caps at scale 0.8, flags (1, 1); the second image is mirrored about its own width 640"""
    from detectorch_amd.optim import ClippedSGD
    from detectorch_amd.train import faster_rcnn_train_step, freeze_stem
    from detectorch_amd.utils import blob as blob_utils
    from test_hip_fpn_train_step import STEP, fpn_detector, joint_inputs
    rs, _, gt = joint_inputs(4)
    images = [rs.randint(0, 256, (480, 512, 3)).astype(np.uint8), rs.randint(0, 256, (560, 640, 3)).astype(np.uint8)]
    flags, widths = (1, 1), (512, 640)
    kw = dict(target_size=480, max_size=512, fpn_on=True)
    dev_blob, scales = blob_utils.images_to_blob(images, flipped=flags, **kw)
    host_blob, _ = blob_utils.images_to_blob([fr.flip_image(im) for im in images], **kw)
    assert np.asarray(scales, np.float32).tolist() == gt["im_scale"].cpu().numpy().tolist() and tuple(dev_blob.shape) == (2, 3, 480, 512)
    assert torch.equal(dev_blob, host_blob)
    results = []
    for blob, batch in ((dev_blob, _device_flipped(gt, None, 4, flags, widths)), (host_blob, _host_flipped(gt, None, 4, flags, widths))):
        model = fpn_detector(13, use_rpn_head=True)
        opt = ClippedSGD(freeze_stem(model), lr=0.01)
        torch.manual_seed(1234)                                   # the RPN minibatch draws its keys from the seeded generator
        with deterministic_framework():
            out = faster_rcnn_train_step(model, opt, blob, batch, it=0, **STEP)
            torch.cuda.synchronize()
        results.append(torch.stack([v.detach().reshape(()) for v in out[:4]]).cpu().numpy())
    print("losses on the device-flipped batch %r, on the host-flipped batch %r" % (results[0].tolist(), results[1].tolist()))
    assert np.isfinite(results[0]).all() and same(results[0], results[1])
