"""dtc_mask_paste / dtc_mask_rle away from the reference's default arguments and past their buffer limits.  -m gpu.

Everything is compared bit for bit with oracle.mask_resize_binarize(mask, ref_box, thresh) pasted into a numpy frame and
oracle.rle_encode(frame) (tests/output_args_cases.py: paste_ref / frame_of); tests/test_output_args_host.py pins, without a GPU, that
the inputs used here really hold the cases they are meant to (a multi-band detection, exact ties, more runs than the first guess).
Where a test checks bytes a kernel must NOT touch, it calls the C entry on tensors it allocated and filled with 0xAB itself.

  a  crop capacity overflow per image (helper and no-helper path), and what dtc_mask_rle makes of the skipped crops
  b  cls_specific_mask = 0 and an indirect, repeating mask_index
  c  thresh_binarize 0 ... 1 and exact ties at the threshold
  d  mask sides 1 ... 62 (and 63 rejected), geometry also against the reference's own expand_boxes
  e  a batch of different and fractional im_size rows
  f  RLE buffer limits: runs do not fit / runs fit and the string does not
  g  the re-run loop of result_utils.segm_results
  h  a crop overflow inside FpnRegionPath reaches the caller of assemble_results"""
import numpy as np
import pytest
import torch

import output_args_cases as oc
from conftest import golden
from detectorch_amd import synth

pytestmark = pytest.mark.gpu

FILL = 0xAB
FILL32 = 0xABABABAB
EINVAL = -1


@pytest.fixture(scope="module")
def hip():
    from detectorch_amd import hip as h
    h.lib()
    return h


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_dets(boxes, cls, max_out):
    """per-image box / class lists -> (dets [B, max_out, 6], det_count [B])"""
    B = len(boxes)
    dets = np.zeros((B, max_out, 6), np.float32)
    for b, rb in enumerate(boxes):
        dets[b, :len(rb), :4] = rb
        dets[b, :len(rb), 4] = 0.9
        dets[b, :len(rb), 5] = cls[b]
    return dets, np.array([len(rb) for rb in boxes], np.int32)


def raw_paste(hip, masks, mask_index, M, dets, counts, im_size, cap, tail, thresh=0.5, cls_specific=1):
    """dtc_mask_paste on buffers of this test: crops = ONE uint8 tensor of B * cap + tail bytes of 0xAB -> dict of device tensors"""
    B, D = dets.shape[0], dets.shape[1]
    t = dict(masks=cu(masks), dets=cu(dets), cnt=cu(counts), im=cu(np.asarray(im_size, np.float32)),
             crops=torch.full((B * cap + tail,), FILL, dtype=torch.uint8, device="cuda"),
             boxes=torch.full((B, D, 4), -77, dtype=torch.int32, device="cuda"),
             rects=torch.full((B, D, 4), -77, dtype=torch.int32, device="cuda"),
             offs=torch.full((B, D), -77, dtype=torch.int64, device="cuda"),
             bytes=torch.full((B,), -77, dtype=torch.int64, device="cuda"))
    idx = cu(mask_index) if mask_index is not None else None
    hip.check(hip.lib().dtc_mask_paste(t["masks"].data_ptr(), idx.data_ptr() if idx is not None else None, masks.shape[1], M,
                                       t["dets"].data_ptr(), t["cnt"].data_ptr(), t["im"].data_ptr(), B, D, float(thresh),
                                       cls_specific, t["crops"].data_ptr(), cap, t["boxes"].data_ptr(), t["rects"].data_ptr(),
                                       t["offs"].data_ptr(), t["bytes"].data_ptr(), hip.stream_ptr()), "mask_paste")
    torch.cuda.synchronize()
    return t


def raw_rle(hip, crops, cap, rects, offs, cnt, im, runs_stride, str_stride):
    """dtc_mask_rle on 0xAB-filled result buffers -> dict of numpy arrays"""
    B, D = rects.shape[0], rects.shape[1]
    counts = torch.full((B, D, runs_stride), FILL32 - (1 << 32), dtype=torch.int32, device="cuda")
    s = torch.full((B, D, str_stride), FILL, dtype=torch.uint8, device="cuda")
    n_runs = torch.full((B, D), -77, dtype=torch.int32, device="cuda")
    s_len = torch.full((B, D), -77, dtype=torch.int32, device="cuda")
    hip.check(hip.lib().dtc_mask_rle(crops.data_ptr(), cap, rects.data_ptr(), offs.data_ptr(), cnt.data_ptr(), im.data_ptr(), B, D,
                                     counts.data_ptr(), runs_stride, n_runs.data_ptr(), s.data_ptr(), str_stride, s_len.data_ptr(),
                                     hip.stream_ptr()), "mask_rle")
    torch.cuda.synchronize()
    return dict(counts=counts.cpu().numpy().view(np.uint32), n_runs=n_runs.cpu().numpy(), str=s.cpu().numpy(),
                str_len=s_len.cpu().numpy())


def check_tables(got, exp):
    """mask_bytes, and mask_boxes / mask_rects / mask_offsets of every row below the count, == the oracle geometry"""
    boxes, rects, offs, nbytes = [got[k].cpu().numpy() for k in ("boxes", "rects", "offs", "bytes")]
    for b, e in enumerate(exp):
        n = len(e["area"])
        assert nbytes[b] == e["bytes"], (b, nbytes[b], e["bytes"])
        assert np.array_equal(boxes[b, :n], e["box"]), b
        assert np.array_equal(rects[b, :n], e["rect"]), b
        assert np.array_equal(offs[b, :n], e["off"]), b


def expected_crops(exp, cap, tail):
    """the whole crops allocation: 0xAB except the crops of the detections with off + area <= cap -> (bytes, number of pasted
    (non-empty, fitting) crops per image)"""
    buf = np.full(len(exp) * cap + tail, FILL, np.uint8)
    n_fit = [0] * len(exp)
    for b, e in enumerate(exp):
        for d, c in enumerate(e["crop"]):
            if c.size and e["off"][d] + c.size <= cap:
                buf[b * cap + e["off"][d]:b * cap + e["off"][d] + c.size] = c.reshape(-1)
                n_fit[b] += 1
    return buf, n_fit


def check_rle(out, exp, im_sizes, oracle, cap=None):
    """per detection: fits (off + area <= cap) -> the oracle's runs and string of the pasted frame; else -1 / -1; d >= count: 0 / 0"""
    RS, SS = out["counts"].shape[2], out["str"].shape[2]
    for b, e in enumerate(exp):
        im_h, im_w = im_sizes[b]
        n = len(e["area"])
        for d in range(n):
            if cap is not None and e["off"][d] + e["area"][d] > cap:
                assert (out["n_runs"][b, d], out["str_len"][b, d]) == (-1, -1), (b, d)
                continue
            runs, s = oracle.rle_encode(oc.frame_of(e["crop"][d], e["rect"][d], im_h, im_w))
            assert len(runs) <= RS and len(s) <= SS
            assert out["n_runs"][b, d] == len(runs) and out["str_len"][b, d] == len(s), (b, d)
            assert np.array_equal(out["counts"][b, d, :len(runs)], runs), (b, d)
            assert out["str"][b, d, :len(s)].tobytes().decode("ascii") == s, (b, d)
        assert not out["n_runs"][b, n:].any() and not out["str_len"][b, n:].any()


# ---- a. capacity overflow -------------------------------------------------------------------------------------------------------
CAP_NAMES = ["all_fit", "image1_one_short", "multiband_one_short", "multiband_offset", "zero_area_offset", "zero"]


@pytest.mark.parametrize("max_out,case", [(16, c) for c in CAP_NAMES] + [(600, "multiband_one_short"), (600, "zero_area_offset")])
def test_crop_capacity_overflow_per_image(hip, oracle, max_out, case):
    """include/detectorch_hip.h, dtc_mask_paste: "a detection is pasted iff mask_offsets[b,d] + area <= per_image_capacity ... the
    others are skipped, their rows of mask_boxes / mask_rects / mask_offsets are still written"; dtc_mask_rle: "a detection with
    mask_offsets[b,d] + area > per_image_capacity gets -1 / -1".  So a zero-area rectangle behind the overflow point gets -1 / -1
    when its offset is above the capacity and a single run of im_h * im_w zeros when its offset EQUALS the capacity (0 bytes at the
    very end of the region fit) -- the `zero_area_offset` case, in which the multi-band detection in front of it fits to the byte.
    Three images of different sizes (9 / 7 / 0 detections): every byte of the allocation that no fitting crop owns, and a tail as
    large as the largest image's need behind the last region, must keep its 0xAB.  max_out 600: the no-helper path, whose offset
    is a running sum instead of the LDS prefix table."""
    M = 28
    boxes, cls, masks16 = oc.overflow_batch(M)
    exp = oc.paste_expectation(oracle, lambda b, d: masks16[b * 16 + d, cls[b][d]], boxes, oc.OVERFLOW_SIZES)
    cap = oc.overflow_capacities(exp)[CAP_NAMES.index(case)]
    tail = max(e["bytes"] for e in exp)
    B = len(boxes)
    masks = np.zeros((B * max_out, 3, M, M), np.float32)
    for b in range(B):
        masks[b * max_out:b * max_out + 16] = masks16[b * 16:(b + 1) * 16]
    dets, counts = make_dets(boxes, cls, max_out)
    got = raw_paste(hip, masks, None, M, dets, counts, oc.OVERFLOW_SIZES, cap, tail)
    check_tables(got, exp)
    want, n_fit = expected_crops(exp, cap, tail)
    crops = got["crops"].cpu().numpy()
    bad = np.flatnonzero(crops != want)
    assert bad.size == 0, (case, bad[:8], bad.size)
    k, z = oc.OVERFLOW_K, oc.OVERFLOW_Z
    e1 = exp[1]
    fits = lambda d: e1["off"][d] + e1["area"][d] <= cap
    assert n_fit[1] == {"all_fit": 6, "image1_one_short": 5, "multiband_one_short": 3, "multiband_offset": 3, "zero_area_offset": 4,
                        "zero": 0}[case] and n_fit[2] == 0
    assert n_fit[0] == 9 if case == "all_fit" else n_fit[0] < 9              # image 0 overflows by its own rule, not image 1's
    assert case != "image1_one_short" or 0 < n_fit[0]
    if case in ("multiband_one_short", "multiband_offset"):
        assert fits(k - 1) and not fits(k) and not fits(z) and e1["off"][z] > cap
    if case == "zero_area_offset":
        assert fits(k) and fits(z) and e1["off"][z] == cap and not fits(z + 1)
    out = raw_rle(hip, got["crops"], cap, got["rects"], got["offs"], got["cnt"], got["im"], 2048, 4096)
    check_rle(out, exp, oc.OVERFLOW_SIZES, oracle, cap=cap)
    if case == "zero_area_offset":                                           # the single run of zeros
        assert out["n_runs"][1, z] == 1 and out["counts"][1, z, 0] == 97 * 131
    if case in ("multiband_one_short", "multiband_offset"):
        assert (out["n_runs"][1, z], out["str_len"][1, z]) == (-1, -1)
    assert not out["n_runs"][2].any() and not out["str_len"][2].any()        # the image without detections: 0 / 0 everywhere


# ---- b. class-agnostic and indirect masks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cls,cls_specific,indexed", [(1, 0, False), (3, 0, False), (1, 0, True), (3, 0, True), (3, 1, True)])
def test_class_agnostic_and_indirect_masks(hip, oracle, n_cls, cls_specific, indexed):
    """cls_specific_mask = 0 (result_utils.py:192-195: `mask = padded_mask[0]`): channel 0 whatever dets[..., 5] says -- the other
    channels hold other random masks, and the class column holds 1 or 2 also when there is ONE channel (three spare mask rows
    behind the last one keep a kernel that wrongly follows the class inside the allocation).  mask_index: rows drawn with
    repetition from 9 masks for 2 x 12 detection slots, so detections share a mask row and n_masks < B * max_out."""
    M, max_out = 28, 12
    sizes = [(97, 131), (120, 160)]
    rs = synth.rng(46, 10 * n_cls + 2 * cls_specific + indexed)
    boxes = [synth.make_rois(rs, n, im_h=h, im_w=w, min_side=4, max_side=90) for n, (h, w) in zip((10, 6), sizes)]
    cls = [rs.randint(1, 3, len(rb)) for rb in boxes]
    n_masks = 9 if indexed else 2 * max_out
    masks = synth.make_masks(rs, n_masks + 3, n_cls, M)
    index = rs.randint(0, n_masks, (2, max_out)).astype(np.int32) if indexed else None
    if indexed:
        index[0, 3] = index[0, 1]                                            # two detections of one image on one mask row
        assert len(np.unique(index[0, :10])) < 10
    row = lambda b, d: int(index[b, d]) if indexed else b * max_out + d
    chan = lambda b, d: int(cls[b][d]) if cls_specific else 0
    exp = oc.paste_expectation(oracle, lambda b, d: masks[row(b, d), chan(b, d)], boxes, sizes)
    dets, counts = make_dets(boxes, cls, max_out)
    cap = max(e["bytes"] for e in exp)
    got = raw_paste(hip, masks, index, M, dets, counts, sizes, cap, 64, cls_specific=cls_specific)
    check_tables(got, exp)
    want, n_fit = expected_crops(exp, cap, 64)
    assert sum(n_fit) == 16 and np.array_equal(got["crops"].cpu().numpy(), want)
    if n_cls == 3:      # the test can tell the channels apart: channel 1 / 2 would give other crops
        other = oc.paste_expectation(oracle, lambda b, d: masks[row(b, d), int(cls[b][d]) if not cls_specific else 0], boxes, sizes)
        assert any(not np.array_equal(a, c) for e, o in zip(exp, other) for a, c in zip(e["crop"], o["crop"]))


# ---- c. threshold ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresh", [0.0, 0.3, 0.5, 0.7, 1.0])
def test_thresh_binarize_values(hip, oracle, thresh):
    """random sigmoid masks with a block of exact 1.0 and a block of exact 0.0: at 0.0 the zero border of the padded mask and the
    zero block are the only background, at 1.0 nothing but rounding above 1 could be foreground"""
    M, D, size = 28, 8, (120, 160)
    rs = synth.rng(47, 0)
    boxes = [synth.make_rois(rs, D, im_h=size[0], im_w=size[1], min_side=6, max_side=150)]
    boxes[0][0] = [-20, -10, 100, 90]
    cls = [rs.randint(1, 3, D)]
    masks = synth.make_masks(rs, D, 3, M)
    masks[:, :, 4:10, 4:10] = 1.0
    masks[:, :, 16:22, 14:24] = 0.0
    exp = oc.paste_expectation(oracle, lambda b, d: masks[d, cls[0][d]], boxes, [size], thresh)
    dets, counts = make_dets(boxes, cls, D)
    cap = exp[0]["bytes"]
    got = raw_paste(hip, masks, None, M, dets, counts, [size], cap, 64, thresh=thresh)
    check_tables(got, exp)
    want, _ = expected_crops(exp, cap, 64)
    crops = got["crops"].cpu().numpy()
    assert np.array_equal(crops, want)
    ones = int(want[:cap].sum())
    if thresh == 0.0:
        assert 0 < cap - ones < cap // 2                                     # mostly foreground, the zero block and border are not
    elif thresh == 1.0:
        assert ones < cap // 50
    else:
        assert cap // 20 < ones < cap - cap // 20


def test_exact_ties_at_the_threshold_are_background(hip, oracle):
    """result_utils.py:203 `mask > thresh_binarize`: strict.  Mask values on the 1/8 grid and an expanded box of exactly 60 x 60 pixels
    make every interpolation fraction 0.25 or 0.75, so every interpolated value is exact in float32 in any evaluation order, and
    26 of the 3600 pixels equal 0.5 exactly (located with the numpy restatement in output_args_cases.tie_case; the comparison
    itself is with the oracle)."""
    M, size = 28, (160, 160)
    mask, ref_box, val = oc.tie_case()
    masks = np.zeros((1, 2, M, M), np.float32)
    masks[0, 1] = mask
    masks[0, 0] = 1.0 - mask
    exp = oc.paste_expectation(oracle, lambda b, d: mask, [ref_box[None]], [size])
    assert exp[0]["rect"][0].tolist() == [98, 98, 158, 158]
    dets, counts = make_dets([ref_box[None]], [np.array([1])], 1)
    got = raw_paste(hip, masks, None, M, dets, counts, [size], 3600, 64)
    check_tables(got, exp)
    crop = got["crops"].cpu().numpy()[:3600].reshape(60, 60)
    ties = val == np.float32(0.5)
    assert int(ties.sum()) >= 20
    assert not crop[ties].any()
    assert np.array_equal(crop, exp[0]["crop"][0])
    # and at a threshold one ulp below the tie value the same pixels are foreground
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    got = raw_paste(hip, masks, None, M, dets, counts, [size], 3600, 64, thresh=below)
    crop = got["crops"].cpu().numpy()[:3600].reshape(60, 60)
    assert crop[ties].all() and np.array_equal(crop, oracle.mask_resize_binarize(mask, ref_box, below)[1])


# ---- d. mask side ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", oc.MASK_SIDES)
def test_mask_sides_vs_oracle_and_reference_geometry(hip, oracle, M):
    """M = 1 ... 62: the LDS layout ((M + 2)^2 mask behind the row table) and the ring of 16 source rows are sized from M; boxes that
    up-scale and boxes that down-scale on either axis (3 x 3 ... 300 x 5 pixels; at M = 56 / 62 one target row spans several source
    rows).  Crops == the oracle; the expanded integer boxes also == the reference's own expand_boxes
    (tests/golden/mask_geometry_sizes.npz)."""
    g = golden("mask_geometry_sizes")
    size = oc.SIZE_FRAME
    rb = oc.geometry_boxes()
    assert np.array_equal(rb, g["ref_boxes"])
    D = rb.shape[0]
    rs = synth.rng(48, M)
    cls = [rs.randint(0, 2, D)]
    masks = synth.make_masks(rs, D, 2, M)
    exp = oc.paste_expectation(oracle, lambda b, d: masks[d, cls[0][d]], [rb], [size])
    dets, counts = make_dets([rb], cls, D)
    cap = exp[0]["bytes"]
    got = raw_paste(hip, masks, None, M, dets, counts, [size], cap, 64)
    check_tables(got, exp)
    assert np.array_equal(got["boxes"][0].cpu().numpy(), g["exp_int_M%d" % M])
    want, n_fit = expected_crops(exp, cap, 64)
    assert n_fit == [D]
    crops = got["crops"].cpu().numpy()
    for d in range(D):                                                       # per detection first: a readable failure
        o, a = int(exp[0]["off"][d]), int(exp[0]["area"][d])
        assert np.array_equal(crops[o:o + a], want[o:o + a]), (M, d, rb[d].tolist())
    assert np.array_equal(crops, want)
    ones = int(want[:cap].sum())
    assert M < 7 or cap // 10 < ones < cap - cap // 10                       # (M = 1, 2: a handful of mask values)


def test_mask_side_63_is_rejected_without_a_launch(hip):
    M, D = 63, 2
    masks = torch.zeros((D, 1, M, M), device="cuda")
    dets = np.zeros((1, D, 6), np.float32)
    dets[0, :, :4] = [[10, 10, 40, 40], [5, 5, 9, 9]]
    t = dict(dets=cu(dets), cnt=cu(np.array([D], np.int32)), im=cu(np.array([[61, 83]], np.float32)),
             crops=torch.full((4096,), FILL, dtype=torch.uint8, device="cuda"),
             boxes=torch.full((1, D, 4), -77, dtype=torch.int32, device="cuda"),
             rects=torch.full((1, D, 4), -77, dtype=torch.int32, device="cuda"),
             offs=torch.full((1, D), -77, dtype=torch.int64, device="cuda"), bytes=torch.full((1,), -77, dtype=torch.int64, device="cuda"))
    call = lambda m: hip.lib().dtc_mask_paste(masks.data_ptr(), None, 1, m, t["dets"].data_ptr(), t["cnt"].data_ptr(), t["im"].data_ptr(), 1,
                                              D, 0.5, 1, t["crops"].data_ptr(), 2048, t["boxes"].data_ptr(), t["rects"].data_ptr(),
                                              t["offs"].data_ptr(), t["bytes"].data_ptr(), hip.stream_ptr())
    assert call(63) == EINVAL and call(0) == EINVAL
    torch.cuda.synchronize()
    assert int(t["bytes"][0]) == -77 and bool((t["crops"] == FILL).all()) and bool((t["offs"] == -77).all())


# ---- e. mixed and fractional image sizes ----------------------------------------------------------------------------------------
def test_mixed_and_fractional_im_sizes(hip, oracle):
    """im_size rows (61, 83), (83, 61) and (61.9, 83.9) in one batch, the same boxes in each image: the clipping differs per image,
    and a fractional size is truncated (`(int)im_size`: the frame of 61.9 x 83.9 is 61 x 83), by the paste and by the RLE."""
    M, D = 14, 7
    im = np.array([[61, 83], [83, 61], [61.9, 83.9]], np.float32)
    sizes = [(61, 83), (83, 61), (61, 83)]
    rs = synth.rng(49, 0)
    rb = np.array([[5, 5, 40, 30], [50, 40, 90, 90], [-5, -5, 70, 70], [58, 10, 64, 80], [10, 58, 80, 64], [70, 70, 100, 100],
                   [0, 0, 82, 60]], np.float32)
    boxes = [rb] * 3
    cls = [rs.randint(1, 3, D)] * 3
    masks = synth.make_masks(rs, 3 * D, 3, M)
    exp = oc.paste_expectation(oracle, lambda b, d: masks[b * D + d, cls[b][d]], boxes, sizes)
    assert exp[0]["rect"].tolist() != exp[1]["rect"].tolist() and exp[0]["bytes"] != exp[1]["bytes"]
    dets, counts = make_dets(boxes, cls, D)
    cap = max(e["bytes"] for e in exp)
    got = raw_paste(hip, masks, None, M, dets, counts, im, cap, 64)
    check_tables(got, exp)
    want, _ = expected_crops(exp, cap, 64)
    assert np.array_equal(got["crops"].cpu().numpy(), want)
    assert exp[2]["rect"].tolist() == exp[0]["rect"].tolist()
    out = raw_rle(hip, got["crops"], cap, got["rects"], got["offs"], got["cnt"], got["im"], 2048, 4096)
    check_rle(out, exp, sizes, oracle, cap=cap)


# ---- f. RLE buffer limits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fits_with_room", "runs_one_short", "fits_exactly", "string_one_short"])
def test_rle_buffer_limits(hip, oracle, case):
    """One 61 x 83 frame of noise with n runs and a string of s bytes (from the oracle), in row 0 of a two-row buffer whose row 1 lies
    past det_count.  runs_stride n - 1: n_runs == -n and str_len == -1 (the string is never formed: its length is not known);
    runs_stride n, str_stride s - 1: n_runs == n with valid run lengths and str_len == -s.  In every case row 1 of both buffers and
    whatever lies past a row's stride keeps its 0xAB."""
    fr = oc.noise_frame()
    im_h, im_w = fr.shape
    runs, s = oracle.rle_encode(fr)
    n, ln = len(runs), len(s)
    RS, SS = {"fits_with_room": (n, ln + 5), "runs_one_short": (n - 1, 7 * n), "fits_exactly": (n, ln), "string_one_short": (n, ln - 1)}[case]
    crops = cu(np.concatenate([fr.reshape(-1), np.full(64, FILL, np.uint8)]))
    rects = cu(np.array([[[0, 0, im_w, im_h], [0, 0, im_w, im_h]]], np.int32))
    offs = cu(np.zeros((1, 2), np.int64))
    out = raw_rle(hip, crops, fr.size, rects, offs, cu(np.array([1], np.int32)), cu(np.array([[im_h, im_w]], np.float32)), RS, SS)
    nr, sl = int(out["n_runs"][0, 0]), int(out["str_len"][0, 0])
    if case == "runs_one_short":
        assert (nr, sl) == (-n, -1)
    elif case == "string_one_short":
        assert (nr, sl) == (n, -ln)
        assert np.array_equal(out["counts"][0, 0, :n], runs)
    else:
        assert (nr, sl) == (n, ln)
        assert np.array_equal(out["counts"][0, 0, :n], runs)
        assert out["str"][0, 0, :ln].tobytes().decode("ascii") == s
    # row 1 begins right behind row 0's stride in both buffers: a write past runs_stride / str_stride of row 0 lands in it
    assert (out["n_runs"][0, 1], out["str_len"][0, 1]) == (0, 0)
    assert (out["str"][0, 1] == FILL).all() and (out["counts"][0, 1] == FILL32).all()


# ---- g. the re-run loop of segm_results --------------------------------------------------------------------------------------------
def test_segm_results_reruns_with_the_sizes_the_kernel_reports(hip, oracle):
    """A 28 x 28 checkerboard resized onto a 600 x 400 box of a 500 x 833 frame needs 16 821 runs and 18 030 bytes
    (tests/test_output_args_host.py), the first guess of result_utils.segm_results is 1 674 runs and 3 396 bytes: the loop must take the
    needed sizes from the negative results and encode again -- for the checkerboard and for the two ordinary detections next to it."""
    from detectorch_amd.utils import result_utils
    M = 28
    im_h, im_w = oc.CHECKER_FRAME
    rs = synth.rng(50, 0)
    rb = np.vstack([[30, 40, 200, 300], oc.CHECKER_BOX, [600, 300, 820, 480]]).astype(np.float32)
    cls = np.array([3, 3, 17])
    masks = synth.make_masks(rs, 3, 81, M)
    masks[1, 3] = oc.checker_mask(M)
    cls_boxes = [[] for _ in range(81)]
    for j in range(1, 81):
        cls_boxes[j] = np.hstack([rb[cls == j], np.ones((int((cls == j).sum()), 1), np.float32)])
    segms = result_utils.segm_results(cls_boxes, cu(masks), rb, im_h, im_w, M=M)
    got = [segms[3][0], segms[3][1], segms[17][0]]
    assert sum(len(x) for x in segms) == 3
    for d in range(3):
        _, rect, sub = oc.paste_ref(oracle, masks[d, cls[d]], rb[d], im_h, im_w)
        runs, s = oracle.rle_encode(oc.frame_of(sub, rect, im_h, im_w))
        assert got[d] == {"size": [im_h, im_w], "counts": s}, d
        if d == 1:
            assert len(runs) > oc.segm_first_guess(im_w)[0] and len(s) > oc.segm_first_guess(im_w)[1]


# ---- h. overflow reaches the caller ---------------------------------------------------------------------------------------------
def test_crop_overflow_in_the_region_path_reaches_assemble_results(hip):
    """FpnRegionPath with a crop_capacity that holds the smaller image's crops to the byte and not the larger image's: after a step
    mask_bytes[b] > crop_capacity for that image, assemble_results raises the "mask crop capacity exceeded" error naming it, and the
    other image's detections and segmentations equal those of the default-capacity run."""
    from detectorch_amd.pipeline import FpnRegionPath, synthetic_batch
    from detectorch_amd.utils import result_utils
    dev = torch.device("cuda", 0)
    B, C = 2, 8
    inputs = synthetic_batch(B, dev, seed=3200, channels=C)
    full = FpnRegionPath(B, dev, channels=C, with_rle=True)
    full.bind(*inputs)
    full.step(use_graph=False)
    torch.cuda.synchronize()
    need = full.mask_bytes.cpu().numpy()
    assert need.min() > 0 and need[0] != need[1] and need.max() <= full.crop_capacity
    big, small = int(np.argmax(need)), int(np.argmin(need))
    cap = int(need[small])
    ref_boxes, ref_segms = result_utils.assemble_results(full.dets, full.det_count, full.im_size, full.rle_str, full.rle_str_len)
    path = FpnRegionPath(B, dev, channels=C, with_rle=True, crop_capacity=cap)
    path.bind(*inputs)
    path.step(use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(path.mask_bytes, full.mask_bytes) and int(path.mask_bytes[big]) > cap >= int(path.mask_bytes[small])
    assert torch.equal(path.dets, full.dets) and torch.equal(path.det_count, full.det_count)
    assert torch.equal(path.mask_offsets, full.mask_offsets) and torch.equal(path.mask_rects, full.mask_rects)
    n_big = min(int(path.det_count[big]), path.max_out)
    fit = (path.mask_offsets[big, :n_big] + (path.mask_rects[big, :n_big, 2] - path.mask_rects[big, :n_big, 0]) *
           (path.mask_rects[big, :n_big, 3] - path.mask_rects[big, :n_big, 1]) <= cap).cpu().numpy()
    assert fit.any() and not fit.all()
    ln, ref_ln = path.rle_str_len[big, :n_big].cpu().numpy(), full.rle_str_len[big, :n_big].cpu().numpy()
    assert np.array_equal(ln[fit], ref_ln[fit]) and (ln[~fit] == -1).all()
    assert (path.rle_n_runs[big, :n_big].cpu().numpy()[~fit] == -1).all()
    with pytest.raises(RuntimeError, match=r"mask crop capacity exceeded\) for image %d detection %d$" % (big, int(np.flatnonzero(~fit)[0]))):
        result_utils.assemble_results(path.dets, path.det_count, path.im_size, path.rle_str, path.rle_str_len)
    s = slice(small, small + 1)
    boxes, segms = result_utils.assemble_results(path.dets[s], path.det_count[s], path.im_size[s], path.rle_str[s], path.rle_str_len[s])
    n_segm = 0
    for j in range(1, 81):
        assert np.array_equal(boxes[j][0], ref_boxes[j][small]) and segms[j][0] == ref_segms[j][small], j
        n_segm += len(segms[j][0])
    assert n_segm == min(int(path.det_count[small]), path.max_out) > 0
