"""The four flip entries on the MI355X past where tests/test_hip_flip.py stops (-m gpu; the "Limits" section of tests/README_flip.md):
the cases of tests/flip_limit_cases.py against the restatements of tests/flip_ref.py.  Every comparison is bitwise.  The outputs and
the workspace of dtc_flip_rle are pre-filled with 0xFF and the padding of its input rows is poisoned."""
import numpy as np
import pytest
import torch

import flip_limit_cases as lc
import flip_ref as fr
from test_hip_flip import same

pytestmark = pytest.mark.gpu

FF = -1                                                       # int32 of 0xFF bytes


def d(a):
    """a device copy of a (read-only) case array"""
    return torch.from_numpy(np.array(a)).cuda()


# ---- run lists --------------------------------------------------------------------------------------------------------------------------------
def launch_rle(name, out_stride):
    from detectorch_amd import hip_flip
    b = lc.rle_batches()[name][0]
    N, R, S = b["runs"].shape
    out = hip_flip.rle_outputs(N, R, out_stride, "cuda")
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    ws = torch.full((hip_flip.rle_workspace_bytes(N, R, S),), 0xFF, dtype=torch.uint8, device="cuda")
    res = hip_flip.flip_rle(d(b["runs"]), d(b["n_runs"]), d(b["im_size"]), b["flipped"], counts=None if b["counts"] is None else d(b["counts"]),
                            out=out, ws=ws)
    return b, {k: v.cpu().numpy() for k, v in res.items()}


def check_rle(name, out_stride):
    b, got = launch_rle(name, out_stride)
    lists, out_n, need = lc.rle_expected(name, out_stride)
    N, R = out_n.shape
    cnt = [R if b["counts"] is None else min(max(int(c), 0), R) for c in (b["counts"] if b["counts"] is not None else [0] * N)]
    runs = got["out_runs"].view(np.uint32)
    for n in range(N):
        assert np.array_equal(got["out_n_runs"][n, :cnt[n]], out_n[n, :cnt[n]]), (name, n, got["out_n_runs"][n].tolist(), out_n[n].tolist())
        assert np.array_equal(got["need"][n, :cnt[n]], need[n, :cnt[n]]), (name, n, got["need"][n].tolist(), need[n].tolist())
        for k in ("out_runs", "out_n_runs", "need"):              # rows past the clamped count keep their 0xFF
            assert (got[k][n, cnt[n]:] == FF).all(), (name, n, k)
        for r in range(cnt[n]):
            if lists[n][r] is not None:
                assert runs[n, r, :len(lists[n][r])].tolist() == lists[n][r], (name, n, r)
    return lists, out_n, need


RLE_CALLS = [(name, s) for name in ("tall_column", "zero_run_chunk", "growth", "chunk_edges", "pixels_2_30", "too_many_pixels", "im_sizes",
                                    "wrapped_sum", "counts") for s in lc.rle_batches()[name][1]]


@pytest.mark.parametrize("name,out_stride", RLE_CALLS, ids=["%s-%d" % c for c in RLE_CALLS])
def test_flip_rle_limit_case(name, out_stride):
    lists, out_n, need = check_rle(name, out_stride)
    if name == "pixels_2_30":                                     # the answers written out by hand
        assert lists[0] == [p[2] for p in lc.PIXELS_2_30]
    if name in ("tall_column", "zero_run_chunk", "chunk_edges", "pixels_2_30"):
        assert (out_n > 0).all()
    if name in ("too_many_pixels", "wrapped_sum"):
        assert (out_n[0] == -1)[:3].all() and not need[0, :3].any()


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(lc.BOX_CASES)), ids=["x".join(map(str, c[0])) for c in lc.BOX_CASES])
def test_flip_boxes_limit_case(k):
    from detectorch_amd import hip_flip
    shape, widths, calls = lc.BOX_CASES[k]
    boxes = lc.boxes(k)
    in_bits = boxes.view(np.uint32)
    t_widths = d(np.array(widths, np.int32))
    for flags, counts in calls:
        want = fr.flip_boxes_batched(boxes, widths, flags, counts)
        t_counts = None if counts is None else d(np.array(counts, np.int32))
        src = d(boxes)
        out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
        hip_flip.flip_boxes(src, t_widths, flags, counts=t_counts, out=out)
        assert same(src.cpu().numpy(), boxes)                    # out of place: the input stays
        hip_flip.flip_boxes(src, t_widths, d(np.array(flags, np.int32)), counts=t_counts, out=src)
        for got in (out.cpu().numpy(), src.cpu().numpy()):
            got_bits, want_bits = got.view(np.uint32), want.view(np.uint32)
            computed_nan = np.isnan(want) & (want_bits != in_bits)     # an x computed from a NaN: a NaN, its payload is not pinned
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert np.array_equal(np.where(computed_nan, 0, got_bits), np.where(computed_nan, 0, want_bits)), (flags, counts)
            assert np.array_equal(got_bits[:, :, 1::2], in_bits[:, :, 1::2])           # y: bit copies, NaN payloads included
            for b in range(shape[0]):                             # unflipped images, rows past the clamped count: bit copies
                n = (shape[1] if counts is None else min(max(counts[b], 0), shape[1])) if flags[b] else 0
                assert np.array_equal(got_bits[b, n:], in_bits[b, n:]), (flags, counts, b)


# ---- polygons ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", range(len(lc.POLY_CALLS)))
def test_flip_polygons_limit_case(call):
    from detectorch_amd import hip_flip
    last, flags = lc.POLY_CALLS[call]
    xy = lc.polygon_points()
    want64, want32 = lc.polygons_expected(xy, last, flags)
    t_xy, t_ptr, t_w = d(xy), d(lc.polygon_ptr(last)), d(np.array(lc.POLY_WIDTHS, np.int32))
    both = hip_flip.flip_polygons(t_xy, t_ptr, t_w, flags)
    only64 = hip_flip.flip_polygons(t_xy, t_ptr, t_w, flags, want32=False)
    only32 = hip_flip.flip_polygons(t_xy, t_ptr, t_w, d(np.array(flags, np.int32)), want64=False)
    assert only64[1] is None and only32[0] is None and same(t_xy.cpu().numpy(), xy)
    for got in (both[0], only64[0]):
        assert same(got.cpu().numpy().view(np.uint64), want64.view(np.uint64))
    for got in (both[1], only32[1]):
        assert same(got.cpu().numpy().view(np.uint32), want32.view(np.uint32))
    inplace = t_xy.clone()
    assert hip_flip.flip_polygons(inplace, t_ptr, t_w, flags, want32=False, out64=inplace)[0] is inplace
    assert same(inplace.cpu().numpy().view(np.uint64), want64.view(np.uint64))
    assert not same(want64, xy)


# ---- the network input ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target,max_size", lc.PREP_TARGETS)
def test_prep_wider_than_a_block(oracle, target, max_size):
    """the yardsticks of test_hip_flip.test_prep_single_images on 40 x 301 images: blobs of two and three blocks in x.  The downscaling
    target gives a blob 151 wide: it is here for its taps, not for its width"""
    from detectorch_amd import hip, hip_flip
    for im in lc.prep_images():
        want, scales = oracle.prep_images([fr.flip_image(im)], target_size=target, max_size=max_size, pad_stride=1)
        t = d(im)
        got, got_scales, _ = hip_flip.prep_images([t], [1], target_size=target, max_size=max_size, pad_stride=1)
        assert got_scales == scales == [target / 40.0] and same(got.cpu().numpy(), want)
        base, _, _ = hip.prep_images([torch.flip(t, [1])], target_size=target, max_size=max_size, pad_stride=1)
        assert torch.equal(got, base)
        assert (got.shape[3] > 256) == (target >= 40)
    # the batch of both, flags (1, 0), padded to a stride of 32: zeros on the right
    u8, f32 = lc.prep_images()
    ts = [d(u8), d(f32)]
    want, scales = oracle.prep_images([fr.flip_image(u8), f32], target_size=target, max_size=max_size, pad_stride=32)
    got, got_scales, sizes = hip_flip.prep_images(ts, [1, 0], target_size=target, max_size=max_size, pad_stride=32)
    assert got_scales == scales and same(got.cpu().numpy(), want)
    base, _, _ = hip.prep_images([torch.flip(ts[0], [1]), ts[1]], target_size=target, max_size=max_size, pad_stride=32)
    assert torch.equal(got, base) and not torch.equal(got[0], hip.prep_images(ts, target_size=target, max_size=max_size, pad_stride=32)[0][0])
    assert (got.shape[3] > 256) == (target >= 40) and got.shape[3] % 32 == 0
    for b, (oh, ow) in enumerate(sizes):
        assert ow < got.shape[3] and float(got[b, :, :, ow:].abs().max()) == 0.0 and float(got[b, :, :oh, :ow].abs().max()) > 0.0
