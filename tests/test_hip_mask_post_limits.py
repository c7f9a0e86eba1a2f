"""libdetectorch_mpost_hip.so on the MI355X past where tests/test_hip_mask_post.py stops (-m gpu; the "Limits" section of
tests/README_mask_post.md): the cases of tests/mask_post_limit_cases.py against the restatement (tests/mask_post_ref.py: vote_sparse
on position windows for the votes, the interval forms for boxes and overlaps of the same lists, formulas for the 65535-image
batches).  Outputs and workspaces are pre-filled with 0xFF, the rows past the counts hold pack_lists' garbage.

REQUIRED AGREEMENT: every comparison is exact -- ovr bit for bit, integers and run lists equal.  No tolerance."""
import numpy as np
import pytest
import torch

import mask_post_limit_cases as lc
import mask_post_ref as mr
import segm_eval_ref as sr
from test_hip_mask_post import check_overlaps, check_vote, run_boxes, run_nms, run_overlaps, run_vote, same_bits

pytestmark = pytest.mark.gpu

GIB = 1 << 30


def thaw(case):
    """a writable copy of a read-only case (torch.from_numpy wants writable memory)"""
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in case.items()}


def pool_of(case):
    return np.array(case["all_runs"]), np.array(case["all_n_runs"]), np.array(case["all_count"])


# ---- the vote --------------------------------------------------------------------------------------------------------------------------------------
VOTES = [(name, method) for name in sorted(lc.VOTE_LIMIT_CASES) for method in ("AVG", "UNION")]


@pytest.mark.parametrize("name,method", VOTES, ids=["%s-%s" % v for v in VOTES])
def test_vote_limit_case(name, method):
    case, ovr = lc.VOTE_LIMIT_CASES[name]()
    want = lc.voted(name, method)
    check_vote(run_vote(thaw(case), np.array(ovr), method), want, case)
    assert (want["need"] > 0).any()


@pytest.mark.parametrize("binarize_thresh", [-0.25, -0.0, 0.0], ids=["-0.25", "-0.0", "0.0"])
def test_vote_walks_every_chunk_under_a_negative_threshold(binarize_thresh):
    """-0.25: the background is on in chunks no voter has a pixel in, a NaN score turns its support off, +inf too; -0.0 is not
    negative: the same lists as at 0.0"""
    case, ovr = lc.negative_threshold_chunks()
    c = dict(thaw(case), binarize_thresh=binarize_thresh)
    want = lc.voted("negative_threshold_chunks", "AVG", binarize_thresh)
    check_vote(run_vote(c, np.array(ovr), "AVG"), want, c)
    assert want["lists"] == lc.voted("negative_threshold_chunks", "AVG", 0.0 if binarize_thresh == 0 else binarize_thresh)["lists"]


# ---- boxes and overlaps of the same lists ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jumps", "im_size_rules"])
def test_boxes_and_overlaps_of_the_vote_lists_by_intervals(name):
    case, _ = lc.VOTE_LIMIT_CASES[name]()
    runs, n_runs, count = pool_of(case)
    im_size = np.array(case["im_size"])
    got, want = run_boxes(runs, n_runs, count, im_size), lc.interval_boxes(runs, n_runs, count, im_size)
    assert all(same_bits(got[k], want[k]) for k in want), got                                    # rows past the counts: still 0xFF = -1
    for crowd in (False, True):
        check_overlaps(run_overlaps((runs, n_runs, count), (runs, n_runs, count), im_size, crowd),
                       mr.overlaps(runs, n_runs, count, runs, n_runs, count, im_size, crowd, counts=sr.interval_counts))


def test_boxes_and_overlaps_at_the_largest_runs_stride():
    case, _ = lc.max_stride()
    runs, n_runs, count = pool_of(case)
    im_size = np.array(case["im_size"])
    got = run_boxes(runs, n_runs, count, im_size)
    for k, (box, area) in enumerate(lc.MAX_STRIDE_BOXES):
        assert tuple(got["boxes"][0, k]) == box and got["area"][0, k] == area and got["nonempty"][0, k] == 1, k
    for crowd in (False, True):
        check_overlaps(run_overlaps((runs, n_runs, count), (runs, n_runs, count), im_size, crowd), lc.max_stride_pairs(crowd))


# ---- the walk --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lc.nms_limits()))
def test_nms_limit_case(name):
    c = lc.nms_limits()[name]
    got = run_nms(np.array(c["dets"]), np.array(c["count"]), np.array(c["ovr"]), c["thresh"], c["mode"])
    want = mr.nms(c["dets"], c["count"], c["ovr"], c["thresh"], c["mode"])
    assert same_bits(got["keep"], want["keep"]) and same_bits(got["keep_count"], want["keep_count"]), (got["keep"], want["keep"])
    if name in lc.NMS_HAND:
        assert got["keep"][0, :got["keep_count"][0]].tolist() == lc.NMS_HAND[name]


def test_nms_on_65535_images():
    case, keep, keep_count = lc.nms_batch()
    got = run_nms(np.array(case["dets"]), np.array(case["count"]), np.array(case["ovr"]), case["thresh"], case["mode"])
    assert same_bits(got["keep"], keep) and same_bits(got["keep_count"], keep_count), np.argwhere(got["keep"] != keep)[:5]


# ---- the batch limit -------------------------------------------------------------------------------------------------------------------------------
def test_boxes_and_overlaps_on_65535_images():
    b = lc.batch_limit()
    a, bb, count, im_size = [np.array(x) for x in b["a"]], [np.array(x) for x in b["b"]], np.array(b["count"]), np.array(b["im_size"])
    got = run_boxes(a[0], a[1], count, im_size)
    assert same_bits(got["boxes"], b["boxes"]) and same_bits(got["area"], b["area"]) and (got["nonempty"] == 1).all()
    for crowd in (False, True):
        pairs = run_overlaps((a[0], a[1], count), (bb[0], bb[1], count), im_size, crowd)
        assert same_bits(pairs["ovr"], b["pairs"][crowd]), np.argwhere(pairs["ovr"] != b["pairs"][crowd])[:5]
        assert (pairs["a_area"] == 2).all() and (pairs["b_area"] == 2).all()


# ---- rows more than 4 GiB behind the base ----------------------------------------------------------------------------------------------------------
def need_memory(nbytes):
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes:
        pytest.skip("%.1f GiB of device memory free, the test takes %.1f" % (free / GIB, nbytes / GIB))


def test_boxes_of_rows_4_gib_behind_the_base():
    """N = 2049, R = 512, runs_stride = 1024: every count is 0 but the last two images', whose rows start 4 GiB (less one image)
    behind the base; the runs of the other images are never copied from the host and never read"""
    from detectorch_amd import hip_mpost
    need_memory(6 * GIB)
    N, R = lc.FAR_N, lc.FAR_R
    last_runs, last_n, last_size = lc.far_boxes()
    runs = torch.empty((N, R, 1024), dtype=torch.int32, device="cuda")
    assert runs.numel() * 4 > 4 * GIB
    runs.view(torch.uint8).fill_(0x7F)
    runs[-2:] = torch.from_numpy(np.array(last_runs).view(np.int32)).cuda()
    n_runs = torch.full((N, R), 1 << 30, dtype=torch.int32, device="cuda")
    n_runs[-2:] = torch.from_numpy(np.array(last_n)).cuda()
    counts = torch.zeros(N, dtype=torch.int32, device="cuda")
    counts[-2:] = R
    im_size = torch.full((N, 2), 25.0, device="cuda")
    im_size[-2:] = torch.from_numpy(np.array(last_size)).cuda()
    out = hip_mpost.boxes_outputs(N, R, "cuda")
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    hip_mpost.mask_boxes(runs, n_runs, im_size, counts, out=out)
    torch.cuda.synchronize()
    untouched = all(bool((v[:-2] == -1).all()) for v in out.values())
    got = {k: v[-2:].cpu().numpy() for k, v in out.items()}
    del runs, n_runs, out
    torch.cuda.empty_cache()
    want = mr.masks_to_boxes(last_runs, last_n, None, last_size)
    assert untouched and all(same_bits(got[k], want[k]) for k in want) and (want["area"] > 0).all()


def test_overlaps_of_rows_4_gib_behind_the_base():
    """N = 2049, Ra = Rb = 512, strides of 2: ovr [2049, 512, 512] float64 is just over 4 GiB; the counts are 0 but the last image's"""
    from detectorch_amd import hip_mpost
    need_memory(6 * GIB)
    N, R = lc.FAR_N, lc.FAR_R
    a_last, b_last, want = lc.far_overlaps()
    ws = torch.full((hip_mpost.overlaps_workspace_bytes(N, R, 2, R, 2),), 0xFF, dtype=torch.uint8, device="cuda")
    out = hip_mpost.overlaps_outputs(N, R, R, "cuda")
    assert out["ovr"].numel() * 8 > 4 * GIB
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    sides = []
    for last in (a_last, b_last):
        runs = torch.full((N, R, 2), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
        runs[-1:] = torch.from_numpy(np.array(last).view(np.int32)).cuda()
        n_runs = torch.full((N, R), 2, dtype=torch.int32, device="cuda")
        count = torch.zeros(N, dtype=torch.int32, device="cuda")
        count[-1] = R
        sides += [runs, n_runs, count]
    im_size = torch.full((N, 2), 10.0, device="cuda")
    for crowd in (False, True):
        hip_mpost.mask_overlaps(*sides, im_size, crowd, out=out, ws=ws)
        torch.cuda.synchronize()
        zero = int(torch.count_nonzero(out["ovr"][:-1].view(torch.int64))) + int(torch.count_nonzero(out["a_area"][:-1])) + \
            int(torch.count_nonzero(out["b_area"][:-1]))
        got = {k: v[-1:].cpu().numpy() for k, v in out.items()}
        assert zero == 0, crowd
        check_overlaps(got, want[crowd])
    del out, ws, sides
    torch.cuda.empty_cache()
