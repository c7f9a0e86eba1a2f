"""The conditions the collect / distribute argument tests on the GPU rely on (tests/test_hip_collect_args.py), pinned without a GPU:
  * oracle.map_rois_to_fpn_levels and oracle.distribute equal the reference's own functions at every level range
    (tests/golden/collect_levels.npz, made by tests/golden/make_collect_levels_golden.py), bit for bit;
  * the tie, level-range, list-count and mask-branch inputs are not empty of what they are about, on the oracle alone;
  * the restatement of fpn_collect_launch's kernel choice (collect_args_cases.plan) names the intended branch for every case, and
    no case needs more dynamic LDS than the kernels are raised to;
  * the host guard: shapes whose LDS need the general kernel cannot hold return DTC_EUNSUPPORTED, the largest that fit pass
    validation -- taken in a child process that sees no device, where a call that passes validation fails at its first HIP call
    (DTC_ELAUNCH) instead of running a kernel on a bogus pointer.
Run as a script with --codes the module prints the guard's return codes as JSON (the child process of the test)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden                     # first: puts the repository root on sys.path (this file also runs as a script)
import collect_args_cases as cc


# ---- the oracle against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_min,k_max", cc.K_RANGES)
def test_oracle_levels_and_distribute_equal_reference(oracle, k_min, k_max):
    g = golden("collect_levels")
    boxes, kind, j = cc.boundary_boxes()
    assert boxes.view(np.uint32).tolist() == g["boxes"].view(np.uint32).tolist() and np.array_equal(j, g["j"])
    tag = "%d_%d" % (k_min, k_max)
    lv = oracle.map_rois_to_fpn_levels(boxes, k_min, k_max)
    assert lv.dtype == np.int32 and np.array_equal(lv, g["lvls_" + tag])
    outs, restore, lv2 = oracle.distribute(boxes, k_min, k_max)
    assert np.array_equal(lv2, lv)
    assert np.array_equal(restore, g["restore_" + tag])
    assert np.array_equal([o.shape[0] for o in outs], g["counts_" + tag])
    assert np.concatenate(outs).view(np.uint32).tolist() == boxes[g["order_" + tag]].view(np.uint32).tolist()


def test_boundary_fixture_decides_something():
    """the epsilon band, the ulp neighbours and the clamps all show in the reference's levels"""
    g = golden("collect_levels")
    boxes, kind, j = cc.boundary_boxes()
    lv = g["lvls_0_7"]
    for jj in range(-3, 4):                                               # 4 + j inside [0, 7] with room below
        band = lv[(kind == "band") & (j == jj)]
        assert band.max() == 4 + jj and band.min() == 3 + jj, jj          # lifted by the epsilon / not lifted
        ulp = lv[(kind == "ulp") & (j == jj)]
        assert set(ulp.tolist()) <= {3 + jj, 4 + jj} and ulp.max() == 4 + jj
        assert lv[(kind == "exact") & (j == jj)].tolist() == [4 + jj]
    frac = np.tile(np.array(cc.BAND_FRACTIONS), len(cc.BOUNDARY_J))
    inside = (kind == "band")
    lifted = lv[inside] == 4 + j[inside]
    assert lifted[(frac <= 0.5) & (j[inside] >= -3) & (j[inside] <= 3)].all()     # well inside the band: always the upper level
    assert not lifted[(frac >= 3.0) & (j[inside] >= -3) & (j[inside] <= 3)].any()
    for k_min, k_max in cc.K_RANGES:
        l = g["lvls_%d_%d" % (k_min, k_max)]
        assert l.min() == k_min and l.max() == k_max
        assert np.array_equal(l, np.clip(g["lvls_0_7"] + (g["lvls_1_8"] == 8), k_min, k_max))      # the ranges differ by the clamp only
        assert l[-3:].tolist() == [k_min, k_min, k_max]                   # 1 x 1, zero area, overflowing area
    with np.errstate(over="ignore"):
        b = boxes[-1]
        assert np.isinf((b[2] - b[0] + np.float32(1)) * (b[3] - b[1] + np.float32(1)))
    b = boxes[-2]
    assert (b[2] - b[0] + np.float32(1)) * (b[3] - b[1] + np.float32(1)) == 0 and b[2] - b[0] + 1 >= 0


# ---- non-emptiness of the inputs, on the oracle alone --------------------------------------------------------------------------------
def _tie_shapes():
    return ([(c, False) for c in cc.CASES["ties_fast_merge"] + cc.CASES["ties_general_sorted"]] +
            [(c, True) for c in cc.CASES["ties_general_unsorted"]])


@pytest.mark.parametrize("gen", cc.TIE_GENS)
def test_tie_cases_tie_where_it_matters(oracle, gen):
    for case, shuffle in _tie_shapes():
        if shuffle and gen == "zeros":
            continue
        L, P, top_n = case["L"], case["P"], case["top_n"]
        boxes, scores, counts = cc.make_inputs(0, L, P, top_n, gen, shuffle=shuffle)
        exp = cc.expected(boxes, scores, counts, top_n, 2, 5)
        assert counts[0, L - 1] == P and (counts == 0).any() and (counts == 1).any() and counts[2].sum() < top_n
        e, (rc, sc) = exp[0], cc.concat(boxes[0], scores[0], counts[0])
        pairs, inside, outside = cc.tie_stats(e, sc, counts[0], top_n)
        assert pairs >= 20, (gen, L, P, top_n, pairs)
        # tied rows are distinguishable: no two rows of an image share a box
        assert len(set(map(bytes, rc))) == rc.shape[0]
        if gen == "const":
            assert np.array_equal(e["src"], np.arange(e["n_out"])) and np.array_equal(e["rois"], rc[:e["n_out"]])
        if gen == "cut":
            run = sc == np.float32(0.5)
            assert int(run.sum()) >= 40 and len(set(cc.list_of(np.flatnonzero(run), counts[0]).tolist())) >= 3
            if L * P > top_n + 40:                                         # the image is longer than top_n: the cut is inside the run
                assert e["roi_scores"][-1] == np.float32(0.5) and inside and outside and len(inside | outside) >= 3, (L, P, top_n)
            else:
                assert e["n_out"] == rc.shape[0] < top_n
        if gen == "zeros":
            z = sc == 0
            assert int(z.sum()) >= 40 and int(np.signbit(sc[z]).sum()) >= 3 and int((~np.signbit(sc[z])).sum()) >= 3
            assert int((e["roi_scores"] == 0).sum()) >= 20                 # zeros inside the result ...
            if L * P > top_n + 40:
                assert e["n_out"] == top_n and len(outside) >= 1           # ... and cut off behind it


@pytest.mark.parametrize("k_min,k_max", cc.K_RANGES)
def test_level_cases_populate_every_level(oracle, k_min, k_max):
    rows, nb = cc.level_boxes()
    g = golden("collect_levels")
    assert nb == g["boxes"].shape[0] == 156 and rows.shape[0] == nb + 300
    for case in cc.CASES["level_ranges"]:
        L, P, top_n = case["L"], case["P"], case["top_n"]
        if case["scores"]:
            boxes, scores, counts, nb2 = cc.level_inputs(L, P, top_n)
        else:
            boxes, scores, counts = rows[None, None].repeat(2, 0), None, np.full((2, 1), rows.shape[0], np.int32)
            boxes = np.concatenate([boxes, np.zeros((2, 1, P - rows.shape[0], 4), np.float32)], 2)
        for b, e in enumerate(cc.expected(boxes, scores, counts, top_n, k_min, k_max)):
            assert (e["level_counts"] >= 1).all(), (case, b, e["level_counts"])
            assert e["n_out"] == min(rows.shape[0], top_n)
            if case["scores"]:
                # every boundary row is collected, and its level is the reference's
                rc, _ = cc.concat(boxes[b], scores[b], counts[b])
                where = {bytes(r): i for i, r in enumerate(e["rois"])}
                at = np.array([where[bytes(r)] for r in rows[:nb]])
                assert np.array_equal(e["roi_levels"][at] + k_min, g["lvls_%d_%d" % (k_min, k_max)])


@pytest.mark.parametrize("gen", ["free", "quant16"])
def test_list_count_sweep_uses_every_list(oracle, gen):
    for case in cc.CASES["list_count_sweep"]:
        L, P, top_n = case["L"], case["P"], case["top_n"]
        boxes, scores, counts = cc.make_inputs(L, L, P, top_n, gen)
        e = cc.expected(boxes, scores, counts, top_n, 2, 5)[0]
        used = set(cc.list_of(e["src"], counts[0]).tolist())
        assert used == set(range(L)), (L, P, used)                         # every list contributes to the result
        short = [l for l in range(L) if counts[0, l] < P]
        assert L == 1 or short                                            # a list with rows past its count ...
        assert all((scores[0, l, counts[0, l]:] == cc.GARBAGE_SCORE).all() for l in range(L))
        assert e["roi_scores"].max() < cc.GARBAGE_SCORE                   # ... that would outrank everything, and none is in the result
    for L in (2, 3, 8):
        sb, ss, keep, counts, gb, gs = cc.make_kept_inputs(L, L, 300, gen)
        assert (np.diff(ss, axis=1) <= 0).all() and (keep.min() < 0 or keep.max() >= cc.KEPT_K_STRIDE)      # garbage past the counts
        e = cc.expected(gb, gs, counts, 300, 2, 5)[0]
        assert set(cc.list_of(e["src"], counts[0]).tolist()) == set(range(L))


def test_unsorted_totals_reach_every_sort_width():
    rs = np.random.RandomState(0)
    widths = set()
    for t in cc.UNSORTED_TOTALS:
        c = cc.split_total(rs, t, 8, 2048)
        assert c.sum() == t and c.max() <= 2048
        widths.add(cc.sort_keys_per_thread(t))
    assert widths == {1, 2, 4, 8, 16}
    assert {cc.next_pow2(t) for t in cc.UNSORTED_TOTALS} >= {2, 512, 1024, 2048, 4096, 8192, 16384}     # 512 / 1024: the merge sort


def test_mask_branch_inputs_carry_the_band_rows(oracle):
    rois5, cls, deltas, rows = cc.mask_branch_inputs()
    g = golden("collect_levels")
    lv_of = {bytes(b): i for i, b in enumerate(g["boxes"])}
    for b in range(2):
        dets, roi = oracle.postprocess_detections(rois5[b, :, 1:], cc.MASK_SF[b], cc.MASK_IM[b], cls[b], deltas[b], nms_thresh=1.5,
                                                  max_det=100)
        assert dets.shape[0] == 100
        got = {bytes(np.ascontiguousarray(d[:4])) for d in dets}
        assert all(bytes(r) in got for r in rows)                          # decoding returned every boundary box bit for bit
        for k_min, k_max in ((3, 5), (1, 8)):
            lv = oracle.map_rois_to_fpn_levels(np.ascontiguousarray(dets[:, :4]), k_min, k_max)
            ref = g["lvls_%d_%d" % (k_min, k_max)]
            hit = [(lv[i], ref[lv_of[bytes(np.ascontiguousarray(d[:4]))]]) for i, d in enumerate(dets)
                   if bytes(np.ascontiguousarray(d[:4])) in lv_of]
            assert len(hit) == rows.shape[0] and all(a == r for a, r in hit)
            assert len(set(lv.tolist())) >= min(3, k_max - k_min + 1)


# ---- the branch restatement ------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_its_branch():
    seen = set()
    for test, cases in cc.CASES.items():
        for c in cases:
            p = cc.plan(c["L"], c["P"], c["top_n"], c["scores"], c["sorted_"], c["keep"], c["roi_order"], c["no_fast"])
            assert p["branch"] == c["branch"], (test, c, p)
            # inside what the launcher raises the kernels to (fpn.hip: 152 KB for the fast kernels, whose budget is 150 KB of
            # dynamic LDS; 144 KB less the static arrays for the general kernel, every case of which needs at most 131 088 bytes)
            assert p["lds"] <= (cc.FAST_LDS_BUDGET if p["kernel"] != "general" else 131088), (test, c, p)
            seen.add(p["branch"])
    assert seen >= {"fast1:merge:bucket", "fast2:merge:bucket", "fast1:plain:bucket", "fast1:merge:none", "general:rank_merge:count",
                    "general:rank_merge:bitonic", "general:rank_merge:none", "general:key_sort:count", "general:no_scores:bitonic"}
    # the thresholds between the kernels, each from its own side
    assert cc.plan(5, 200, 2048)["kernel"] == "fast2" and cc.plan(5, 200, 2049)["kernel"] == "general"
    assert cc.plan(3, 1024, 1000)["kernel"] == "fast1" and cc.plan(3, 1025, 1000)["kernel"] == "general"
    assert cc.plan(8, 1024, 1000)["kernel"] == "fast1" and cc.plan(8, 1025, 2000)["kernel"] == "general"
    assert cc.plan(8, 1024, 2048)["kernel"] == "general" and cc.plan(5, 1000, 2000)["kernel"] == "fast2"
    assert cc.plan(5, 200, 300, sorted_=False)["kernel"] == "general" and cc.plan(5, 200, 300, no_fast=True)["kernel"] == "general"
    assert cc.plan(5, 200, 300, keep=True, no_fast=True)["kernel"] == "fast1"


# ---- the host guard ------------------------------------------------------------------------------------------------------------------------
BOGUS = 256                                                                  # a bogus, non-NULL, 16-byte aligned device pointer
ELAUNCH = -2


def _guard_call(hip, L, P, top_n, scores=True, sorted_=True, keep=False, roi_order=True):
    v = lambda on=True: C.c_void_p(BOGUS) if on else None
    outs = [v(), v(scores), v(), v(), v(), v(), v(), v(roi_order), v(roi_order)]
    lib = hip.lib()
    if keep:
        return lib.dtc_fpn_collect_distribute_kept(v(), v(), 2000, v(), v(), P, 2, L, top_n, 2, 5, *outs, None)
    return lib.dtc_fpn_collect_distribute(v(), v(scores), v(), 2, L, P, top_n, 2, 5, *outs, 1 if sorted_ else 0, None)


def test_guard_table_agrees_with_the_restatement():
    for name, (kw, passes) in cc.GUARD_CASES.items():
        p = cc.plan(kw["L"], kw["P"], kw["top_n"], kw.get("scores", True), kw.get("sorted_", True), kw.get("keep", False),
                    kw.get("roi_order", True))
        assert (p["kernel"] is not None) == passes, (name, p)
        if passes and p["kernel"] == "general":
            assert p["lds"] + cc.GENERAL_STATIC_LDS <= cc.GENERAL_LDS_LIMIT
    fits = [cc.plan(k["L"], k["P"], k["top_n"], k.get("scores", True), k.get("sorted_", True), False, k.get("roi_order", True))["lds"]
            for k, ok in cc.GUARD_CASES.values() if ok and not k.get("keep")]
    assert max(fits) == cc.GENERAL_LDS_LIMIT - cc.GENERAL_STATIC_LDS       # the largest shape that fits, to the byte


def test_lds_guard_return_codes_without_a_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--codes"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = json.loads(out.stdout.decode())
    assert got == {k: (ELAUNCH if ok else cc.EUNSUPPORTED) for k, (kw, ok) in cc.GUARD_CASES.items()}


if __name__ == "__main__" and "--codes" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from detectorch_amd import hip as _hip
    print(json.dumps({k: _guard_call(_hip, **kw) for k, (kw, _) in cc.GUARD_CASES.items()}))
