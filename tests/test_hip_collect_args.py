"""dtc_fpn_collect_distribute / dtc_fpn_collect_distribute_kept (csrc/fpn.hip) and the shared fpn_level / fpn_map_rows
(csrc/fpn_map.h) off their default point: tied scores, every input list count, both kernels and every branch of each, level ranges
other than (2, 5), NULL optional outputs.  -m gpu.

Every buffer is compared bit for bit with collect_args_cases.expected (oracle.collect + oracle.distribute): the tie order is the
canonical rule of csrc/block_sort.h (score descending, concatenation index ascending), the level mapping and distribution are the
reference's (tests/golden/collect_levels.npz pins the oracle, and the boundary rows here directly).  Inputs, the branch each case
is meant to reach and the conditions that keep the cases from passing emptily: tests/collect_args_cases.py,
tests/test_collect_args_host.py.  The outputs live in one arena pre-filled with -77, with guard words between them.

Run as a script with --knob-child the module runs the tie and list-count inputs once (the child process of
test_general_kernel_knob_in_child_process, started with DTC_FPN_NO_FAST=1)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden                     # first: puts the repository root on sys.path (this file also runs as a script)
import collect_args_cases as cc
from detectorch_amd import synth

pytestmark = pytest.mark.gpu

ORDER = ("rois5", "roi_scores", "roi_levels", "n_out", "rois_by_level", "level_counts", "idx_restore", "roi_order", "roi_desc")
FLOATS = ("rois5", "roi_scores", "rois_by_level", "roi_desc")
GAP = 64                                        # guard words between the output buffers
FILL = -77


@pytest.fixture(scope="module")
def hip():
    from detectorch_amd import hip as h
    h.lib()
    return h


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Outputs:
    """the nine output buffers as slices of one int32 arena, GAP guard words in front of, between and behind them; everything
    pre-filled with -77 (float buffers with -77.0)"""

    def __init__(self, B, T, nl):
        sizes = dict(rois5=B * T * 5, roi_scores=B * T, roi_levels=B * T, n_out=B, rois_by_level=B * T * 4, level_counts=B * nl,
                     idx_restore=B * T, roi_order=B * T, roi_desc=B * T * 8)
        shapes = dict(rois5=(B, T, 5), roi_scores=(B, T), roi_levels=(B, T), n_out=(B,), rois_by_level=(B, T, 4),
                      level_counts=(B, nl), idx_restore=(B, T), roi_order=(B, T), roi_desc=(B, T, 8))
        self.span, pos = {}, GAP
        for k in ORDER:
            self.span[k] = (pos, pos + sizes[k])
            pos = (pos + sizes[k] + GAP + 3) // 4 * 4                       # 16-byte aligned starts
        self.arena = torch.full((pos,), FILL, dtype=torch.int32, device="cuda")
        self.t = {}
        for k in ORDER:
            a, b = self.span[k]
            v = self.arena[a:b]
            if k in FLOATS:
                v = v.view(torch.float32)
                v.fill_(float(FILL))
            self.t[k] = v.view(shapes[k])
        self.guard = np.ones(pos, bool)
        for k in ORDER:
            a, b = self.span[k]
            self.guard[a:b] = False

    def ptr(self, k, null=()):
        return None if k in null else self.t[k].data_ptr()

    def check_untouched(self, null=()):
        arena = self.arena.cpu().numpy()
        assert (arena[self.guard] == FILL).all(), "a guard word between the output buffers was written"
        for k in null:
            got = self.t[k].cpu().numpy()
            assert (got == FILL).all(), "%s was passed as NULL and its allocation was written" % k


def call(hip, boxes, scores, counts, top_n, k_min=2, k_max=5, sorted_=True, null=()):
    B, L, P = boxes.shape[:3]
    tb, tc = cu(boxes), cu(counts.astype(np.int32))
    ts = None if scores is None else cu(scores)
    o = Outputs(B, top_n, k_max - k_min + 1)
    null = tuple(null) + (("roi_scores",) if scores is None else ())
    rc = hip.lib().dtc_fpn_collect_distribute(tb.data_ptr(), None if ts is None else ts.data_ptr(), tc.data_ptr(), B, L, P, top_n,
                                              k_min, k_max, *[o.ptr(k, null) for k in ORDER], 1 if sorted_ else 0, hip.stream_ptr())
    hip.check(rc, "dtc_fpn_collect_distribute")
    torch.cuda.synchronize()
    o.check_untouched(null)
    return o


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(o, exp, top_n, null=()):
    """every buffer of `o` against the expectation, image by image, bit for bit (float buffers as their bit patterns: -0.0 is not 0.0)"""
    res = {k: v.cpu().numpy() for k, v in o.t.items()}
    for b, e in enumerate(exp):
        n = e["n_out"]
        assert int(res["n_out"][b]) == n, (b, int(res["n_out"][b]), n)
        assert np.array_equal(bits(res["rois5"][b, :n, 1:]), bits(e["rois"])), (b, "rois5")
        assert np.all(res["rois5"][b, :n, 0] == b)
        if e["roi_scores"] is not None and "roi_scores" not in null:
            assert np.array_equal(bits(res["roi_scores"][b, :n]), bits(e["roi_scores"])), (b, "roi_scores")
        assert np.array_equal(res["roi_levels"][b], e["roi_levels"]), (b, "roi_levels")
        assert np.array_equal(res["idx_restore"][b, :n], e["idx_restore"]), (b, "idx_restore")
        assert np.array_equal(res["level_counts"][b], e["level_counts"]), (b, "level_counts")
        assert np.array_equal(bits(res["rois_by_level"][b, :n]), bits(e["rois_by_level"])), (b, "rois_by_level")
        if "roi_order" not in null:
            # the RoIAlign visiting order is a permutation of the image's rows and the packed descriptors repeat them
            order = res["roi_order"][b]
            assert np.array_equal(np.sort(order), np.arange(b * top_n, (b + 1) * top_n)), (b, "roi_order")
            if "roi_desc" not in null:
                rows, desc = order - b * top_n, res["roi_desc"][b]
                assert np.array_equal(bits(desc[:, :5]), bits(res["rois5"][b, rows])), (b, "roi_desc")
                assert np.array_equal(desc[:, 5], res["roi_levels"][b, rows]) and np.array_equal(desc[:, 6], order)
    return res


def run_case(hip, case, gen, seed, shuffle=False, k_min=2, k_max=5):
    L, P, top_n = case["L"], case["P"], case["top_n"]
    boxes, scores, counts = cc.make_inputs(seed, L, P, top_n, gen, shuffle=shuffle)
    exp = cc.expected(boxes, scores, counts, top_n, k_min, k_max)
    return check(call(hip, boxes, scores, counts, top_n, k_min, k_max, sorted_=not shuffle), exp, top_n)


# ---- ties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", cc.TIE_GENS)
def test_ties_fast_merge(hip, oracle, gen):
    """the fast kernel's pairwise merge-path tree, one and two output ranks per thread"""
    for case in cc.CASES["ties_fast_merge"]:
        run_case(hip, case, gen, 0)


@pytest.mark.parametrize("gen", cc.TIE_GENS)
def test_ties_general_sorted(hip, oracle, gen):
    """the general kernel's rank merge: `(q < l) ? v >= s : v > s`"""
    for case in cc.CASES["ties_general_sorted"]:
        run_case(hip, case, gen, 0)


@pytest.mark.parametrize("gen", ["quant16", "const", "cut"])
def test_ties_general_unsorted(hip, oracle, gen):
    """the general kernel's key sort, rows shuffled inside each list"""
    for case in cc.CASES["ties_general_unsorted"]:
        run_case(hip, case, gen, 0, shuffle=True)


# ---- list counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", ["free", "quant16"])
@pytest.mark.parametrize("L", cc.SWEEP_L)
def test_list_count_sweep(hip, oracle, L, gen):
    """the merge tree and its carries for every list count but 5 (L = 1 with sorted scores: no merge); (8, 1024, 1000) once"""
    for case in cc.CASES["list_count_sweep"]:
        if case["L"] == L and (case["P"] == 128 or gen == "quant16"):
            run_case(hip, case, gen, L)


# ---- the general kernel's sizes --------------------------------------------------------------------------------------------------------
def test_general_kernel_sizes(hip, oracle):
    """rank merge above the fast kernel's limits (top_n, in_stride, n_max, LDS), the general kernel without scores, the bitonic
    visiting order at top_n 2100 / 3000, and the key sort at every block_bitonic_sort width: 1 (network and merge sort), 2, 4, 8 and
    16 keys per thread, plus 0, 1 and 2 rows"""
    sizes = cc.CASES["general_kernel_sizes"]
    for case in sizes[:3]:
        run_case(hip, case, "quant16", 7)
    c = sizes[3]                                                              # no scores: the rows in the given order
    rs = synth.rng(67, 0)
    boxes = np.stack([synth.make_rois(rs, c["P"]) for _ in range(2)])[:, None]
    counts = np.array([[c["P"]], [1234]], np.int32)
    check(call(hip, boxes, None, counts, c["top_n"]), cc.expected(boxes, None, counts, c["top_n"], 2, 5), c["top_n"])
    c = sizes[4]                                                              # unsorted lists, 16384 padded keys and below
    rs = synth.rng(67, 1)
    totals = cc.UNSORTED_TOTALS
    for i in range(0, len(totals), 3):
        counts = np.stack([cc.split_total(rs, t, c["L"], c["P"]) for t in totals[i:i + 3]])
        boxes, scores, counts = cc.make_inputs(70 + i, c["L"], c["P"], c["top_n"], "quant16", counts=counts, shuffle=True)
        check(call(hip, boxes, scores, counts, c["top_n"], sorted_=False), cc.expected(boxes, scores, counts, c["top_n"], 2, 5), c["top_n"])


@pytest.mark.parametrize("T", [2049, 4096, 8192])
def test_visiting_order_above_2048(hip, oracle, T):
    """the block_bitonic_sort branch of the visiting order: roi_order is a permutation of the image's rows, roi_desc repeats
    rois5 / level / row (check), and RoIAlign driven by those descriptors equals RoIAlign in plain order"""
    B = 2
    rs = synth.rng(68, T)
    boxes = np.stack([synth.make_rois(rs, T) for _ in range(B)])[:, None]
    counts = np.array([[T], [T]], np.int32)
    o = call(hip, boxes, None, counts, T)
    check(o, cc.expected(boxes, None, counts, T, 2, 5), T)
    feats = [cu(synth.make_features(rs, (B, 8, h, w))) for (h, w) in synth.fpn_level_shapes()[:4]]
    ref = hip.roi_align_forward(feats, synth.FPN_ROI_SCALES, o.t["rois5"].reshape(-1, 5).contiguous(), 7, 7, 2,
                                roi_levels=o.t["roi_levels"].reshape(-1).contiguous())
    out = torch.full((B * T, 8, 7, 7), -1.0, device="cuda")
    lvs, ch, dt = hip.make_levels(feats, synth.FPN_ROI_SCALES)
    desc = o.t["roi_desc"].contiguous()
    assert hip.lib().dtc_roi_align_forward_packed(lvs, 4, ch, 0, desc.data_ptr(), B * T, 7, 7, 2, out.data_ptr(), 0, hip.stream_ptr()) == 0
    assert torch.equal(out, ref)


# ---- level ranges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_min,k_max", cc.K_RANGES[1:])
def test_level_ranges(hip, oracle, k_min, k_max):
    """boundary boxes + 300 boxes over every level, through the fast kernel, the general kernel and the no-scores form: every buffer
    equals the oracle; on the boundary rows roi_levels equals the reference's map_rois_to_fpn_levels, and on the boundary rows alone
    level_counts, idx_restore and rois_by_level equal the reference's distribute"""
    g = golden("collect_levels")
    tag = "%d_%d" % (k_min, k_max)
    rows, nb = cc.level_boxes()
    assert np.array_equal(bits(rows[:nb]), bits(g["boxes"]))
    fast, general, plain = cc.CASES["level_ranges"]
    for case in (fast, general):
        boxes, scores, counts, _ = cc.level_inputs(case["L"], case["P"], case["top_n"])
        res = check(call(hip, boxes, scores, counts, case["top_n"], k_min, k_max), cc.expected(boxes, scores, counts, case["top_n"], k_min, k_max),
                    case["top_n"])
        for b in range(boxes.shape[0]):
            n = int(res["n_out"][b])
            where = {bytes(r): i for i, r in enumerate(np.ascontiguousarray(res["rois5"][b, :n, 1:]))}
            at = np.array([where[bytes(r)] for r in rows[:nb]])
            assert np.array_equal(res["roi_levels"][b, at] + k_min, g["lvls_" + tag]), (case["branch"], b)
    P = plain["P"]
    boxes = np.zeros((2, 1, P, 4), np.float32)
    boxes[:, 0, :rows.shape[0]] = rows
    boxes[1, 0, :nb] = rows[:nb][::-1]
    counts = np.full((2, 1), rows.shape[0], np.int32)
    res = check(call(hip, boxes, None, counts, plain["top_n"], k_min, k_max), cc.expected(boxes, None, counts, plain["top_n"], k_min, k_max),
                plain["top_n"])
    assert np.array_equal(res["roi_levels"][0, :nb] + k_min, g["lvls_" + tag])
    assert np.array_equal(res["roi_levels"][1, :nb] + k_min, g["lvls_" + tag][::-1])
    # the boundary rows alone: the reference's distribute
    only = np.ascontiguousarray(rows[:nb])[None, None]
    res = call(hip, only, None, np.array([[nb]], np.int32), nb, k_min, k_max)
    res = {k: v.cpu().numpy() for k, v in res.t.items()}
    assert int(res["n_out"][0]) == nb
    assert np.array_equal(res["roi_levels"][0] + k_min, g["lvls_" + tag])
    assert np.array_equal(res["level_counts"][0], g["counts_" + tag])
    assert np.array_equal(res["idx_restore"][0], g["restore_" + tag])
    assert np.array_equal(bits(res["rois_by_level"][0]), bits(rows[:nb][g["order_" + tag]]))


@pytest.mark.parametrize("k_min,k_max", [(3, 5), (1, 8)])
def test_mask_branch_mapping_level_ranges(hip, oracle, k_min, k_max):
    """dtc_postprocess_detections_fpn with FpnMapOut(k_min, k_max) (fpn_map_rows): equals dtc_fpn_collect_distribute(in_scores = NULL)
    at the same range on the detection rows, buffer for buffer, and the oracle's levels; the detections carry the exact and the
    epsilon-band boundary boxes (tests/test_collect_args_host.py), whose levels are the reference's"""
    dev = torch.device("cuda", 0)
    rois5, cls, deltas, brows = cc.mask_branch_inputs()
    B, R, ncls, D, nl = 2, cc.MASK_R, cc.MASK_NCLS, cc.MASK_D, k_max - k_min + 1
    t_rois, t_cls, t_del, sf, im = cu(rois5), cu(cls), cu(deltas), cu(cc.MASK_SF), cu(cc.MASK_IM)
    n_rois = torch.tensor([R, R], dtype=torch.int32, device=dev)
    dets, det_roi, det_scaled, det_count = hip.postprocess_detections(t_rois, n_rois, t_cls, t_del, sf, im, nms_thresh=1.5, max_det=100,
                                                                       max_out=D)
    sep = hip.fpn_collect_distribute(det_scaled.view(B, 1, D, 4), None, det_count.view(B, 1), D, k_min, k_max)
    L = hip.lib()
    o = Outputs(B, D, nl)
    fm = hip.FpnMapOut(*[o.t[k].data_ptr() for k in ORDER if k != "roi_scores"], k_min, k_max)
    ws = hip.workspace(L.dtc_postprocess_detections_workspace_bytes(B, R, ncls), dev)
    d2, r2, s2, c2 = torch.zeros_like(dets), torch.zeros_like(det_roi), torch.zeros_like(det_scaled), torch.zeros_like(det_count)
    hip.check(L.dtc_postprocess_detections_fpn(t_rois.data_ptr(), n_rois.data_ptr(), t_cls.data_ptr(), 0, t_del.data_ptr(), sf.data_ptr(),
                                               im.data_ptr(), B, R, ncls, 10.0, 10.0, 5.0, 5.0, 0.05, 1.5, 100, ws.data_ptr(), ws.numel(),
                                               d2.data_ptr(), r2.data_ptr(), s2.data_ptr(), c2.data_ptr(), D, fm, hip.stream_ptr(dev)),
              "postprocess_detections_fpn")
    torch.cuda.synchronize()
    o.check_untouched(("roi_scores",))
    assert torch.equal(c2, det_count) and det_count.tolist() == [100, 100]
    g = golden("collect_levels")
    lv_of = {bytes(r): l for r, l in zip(g["boxes"], g["lvls_%d_%d" % (k_min, k_max)])}
    for b in range(B):
        assert torch.equal(s2[b, :100], det_scaled[b, :100])
        assert int(o.t["n_out"][b]) == int(sep["n_out"][b]) == 100
        for k in ("rois5", "roi_levels", "idx_restore", "roi_order", "roi_desc", "level_counts"):
            assert torch.equal(o.t[k][b], sep[k][b]), (k, b)
        assert torch.equal(o.t["rois_by_level"][b, :100], sep["rois_by_level"][b, :100])
        bx = np.ascontiguousarray(det_scaled[b, :100].cpu().numpy())
        lv = o.t["roi_levels"][b].cpu().numpy()
        assert np.array_equal(lv[:100] + k_min, oracle.map_rois_to_fpn_levels(bx, k_min, k_max)) and (lv[100:] == -1).all()
        hit = [(lv[i] + k_min, lv_of[bytes(r)]) for i, r in enumerate(bx) if bytes(r) in lv_of]
        assert len(hit) >= brows.shape[0] and all(a == r for a, r in hit)


# ---- the keep form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", ["free", "quant16"])
@pytest.mark.parametrize("L", [2, 3, 8])
def test_kept_form_list_counts_and_ties(hip, oracle, L, gen):
    """dtc_fpn_collect_distribute_kept against expected(...) on the gathered rows directly; garbage in `keep` past the counts"""
    top_n, ks, kst = 300, 128, cc.KEPT_K_STRIDE
    sb, ss, keep, counts, gb, gs = cc.make_kept_inputs(L, L, top_n, gen, ks, kst)
    B = counts.shape[0]
    t_b, t_s, t_k, t_c = cu(sb), cu(ss), cu(keep), cu(counts.reshape(-1))
    o = Outputs(B, top_n, 4)
    hip.check(hip.lib().dtc_fpn_collect_distribute_kept(t_b.data_ptr(), t_s.data_ptr(), kst, t_k.data_ptr(), t_c.data_ptr(), ks, B, L, top_n,
                                                        2, 5, *[o.ptr(k) for k in ORDER], hip.stream_ptr()), "dtc_fpn_collect_distribute_kept")
    torch.cuda.synchronize()
    o.check_untouched()
    check(o, cc.expected(gb, gs, counts, top_n, 2, 5), top_n)


# ---- optional outputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fast", "general"])
def test_optional_outputs_null(hip, oracle, which):
    """roi_scores NULL; roi_order and roi_desc NULL; roi_order given with roi_desc NULL: the other buffers are what the all-outputs
    call writes (and the oracle's), the allocations that were not passed and the guard words around every buffer stay as they were"""
    case = cc.CASES["optional_outputs_null"][0 if which == "fast" else 2]
    L, P, top_n = case["L"], case["P"], case["top_n"]
    boxes, scores, counts = cc.make_inputs(3, L, P, top_n, "quant16")
    exp = cc.expected(boxes, scores, counts, top_n, 2, 5)
    full = check(call(hip, boxes, scores, counts, top_n), exp, top_n)
    for null in (("roi_scores",), ("roi_order", "roi_desc"), ("roi_desc",)):
        got = check(call(hip, boxes, scores, counts, top_n, null=null), exp, top_n, null=null)
        for k in ORDER:
            if k in null:
                continue
            for b, e in enumerate(exp):
                rows = slice(None) if k in ("roi_levels", "roi_order", "roi_desc", "level_counts", "n_out") else slice(0, e["n_out"])
                assert np.array_equal(np.atleast_1d(got[k][b])[rows].view(np.uint32), np.atleast_1d(full[k][b])[rows].view(np.uint32)), (null, k, b)


# ---- the general kernel through the knob -----------------------------------------------------------------------------------------------
def knob_child(hip):
    """the inputs of test_ties_fast_merge and test_list_count_sweep; under DTC_FPN_NO_FAST=1 they take the general kernel"""
    for gen in cc.TIE_GENS:
        for case in cc.CASES["ties_fast_merge"]:
            run_case(hip, case, gen, 0)
    for gen in ("free", "quant16"):
        for case in cc.CASES["list_count_sweep"]:
            if case["P"] == 128 or gen == "quant16":
                run_case(hip, case, gen, case["L"])
    print("ok")


def test_general_kernel_knob_in_child_process(hip, oracle):
    """DTC_FPN_NO_FAST is resolved once per process, so the general kernel gets the fast kernel's inputs in a child process, which
    runs under its own time limit"""
    env = dict(os.environ, DTC_FPN_NO_FAST="1")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--knob-child"], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


if __name__ == "__main__" and "--knob-child" in sys.argv:
    assert os.environ.get("DTC_FPN_NO_FAST")
    from detectorch_amd import hip as _hip
    _hip.lib()
    knob_child(_hip)
