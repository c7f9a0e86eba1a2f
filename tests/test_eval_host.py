"""The evaluation without a GPU:
  * the numpy restatement of COCOeval (tests/coco_eval_ref.py) against cases whose answers are known without it;
  * every condition the cases of tests/README_eval.md name actually occurs in them;
  * the greedy rounds of dtc_eval_proposal_recall's header, restated in numpy on the pinned bbox_overlaps, against the reference's own
    evaluate_box_proposals (tests/golden/eval.npz, made by tests/golden/make_eval_golden.py);
  * libdetectorch_eval_hip.so exports exactly what include/detectorch_eval_hip.h declares and hip_eval.SIGNATURES binds it, parameter
    names in order; the header compiles as pedantic C99 and C++11; the other libraries export nothing of it;
  * CPU tensors, wrong dtypes and over-limit sizes are refused; the return codes of the three entries on bad arguments (validation
    precedes every HIP call, so nothing is launched); the constants of the binding are those of the source text."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden
import coco_eval_ref as cr
import eval_cases as ec

sys.path.insert(0, GOLDEN)


# ---- the restatement against known answers -----------------------------------------------------------------------------------------------
SIZES = (20, 60, 150)                                          # small, medium, large


def grid_case(n_images=6, jitter=0, seed=0, drop=0.0, extra=0):
    """image i holds one gt per class 1..3 on a wide grid, class c of size SIZES[(i + c) % 3]; the detections are the gt boxes (moved by
    up to `jitter`), with unique scores; `extra`: far-away false positives per image"""
    rs = np.random.RandomState(seed)
    scores = iter(rs.permutation(n_images * (3 + extra) * 2) / 1000.0 + 0.001)
    images = []
    for i in range(n_images):
        g, d = [], []
        for c in (1, 2, 3):
            s, x = SIZES[(i + c) % 3], 400.0 * c
            g.append((x, 50, x + s - 1, 50 + s - 1, c, 0, None))
            if rs.rand() >= drop:
                j = rs.randint(-jitter, jitter + 1, 4) if jitter else np.zeros(4)
                d.append((x + j[0], 50 + j[1], x + s - 1 + j[2], 50 + s - 1 + j[3], next(scores), c))
        for e in range(extra):
            d.append((3000 + 300 * e, 900, 3000 + 300 * e + rs.randint(10, 200), 1000, next(scores), int(rs.randint(1, 4))))
        images.append((d, g, None))
    return ec.build(images)


def test_detections_equal_to_the_gt_score_one():
    out = cr.run(grid_case())
    assert out["stats"].tolist() == [1.0] * 12
    assert np.all(out["precision"] == 1.0) and np.all(out["recall"] == 1.0) and np.all(out["counts"][:, 0] == 6)


def test_false_positive_above_the_true_positive():
    c = ec.build([([(500, 500, 520, 520, 0.9, 1), (0, 0, 49, 49, 0.8, 1)], [(0, 0, 49, 49, 1, 0, None)], None)], num_classes=2)
    out = cr.run(c)
    assert abs(out["stats"][0] - 0.5) <= 1e-12 and out["stats"][8] == 1.0
    assert out["stats"][6] == 0.0                              # AR at one detection per image: the false positive


def test_no_detections():
    c = ec.build([([], [(0, 0, 49, 49, 1, 0, None)], None), ([], [(0, 0, 9, 9, 1, 0, None)], None)], num_classes=2)
    out = cr.run(c)
    assert out["stats"][0] == 0.0 and out["stats"][8] == 0.0 and np.all(out["precision"][:, :, 0, 0, :] == 0) and np.all(out["dt_rank"] == -1)


def test_class_with_only_crowd_gt():
    c = ec.build([([(0, 0, 49, 49, 0.9, 1), (0, 0, 49, 49, 0.8, 2)], [(0, 0, 49, 49, 1, 1, None), (0, 0, 49, 49, 2, 0, None)], None)],
                 num_classes=3)
    out = cr.run(c)
    assert np.all(out["precision"][:, :, 0] == -1) and np.all(out["recall"][:, 0] == -1) and np.all(out["counts"][0] == 0)
    assert out["stats"][0] == 1.0 / (1.0 + np.spacing(1))      # class 2 alone: one true positive
    assert out["dt_ignore"][0, 0] == np.uint64((1 << 40) - 1) and out["dt_match"][0, 0] == np.uint64((1 << 40) - 1)


def test_consistent_permutations_leave_the_stats():
    c = grid_case(jitter=6, seed=3, drop=0.2, extra=2)
    want = cr.run(c)["stats"]
    assert 0.05 < want[0] < 0.95
    p = dict(c)
    relabel = np.array([0, 3, 1, 2])
    p["dets"] = c["dets"].copy()
    p["dets"][:, :, 5] = relabel[np.nan_to_num(c["dets"][:, :, 5]).astype(int)]
    p["gt_classes"] = relabel[c["gt_classes"]].astype(np.int32)
    order = np.array([4, 0, 5, 2, 1, 3])
    q = {k: (v[order] if isinstance(v, np.ndarray) and v.shape[:1] == (6,) and k not in ("iou_thrs", "rec_thrs", "area_rngs") else v)
         for k, v in c.items()}
    # the same entries enter every mean, in another order: a few roundings of a float64 sum of at most 10 x 101 x 3 terms <= 1
    for other in (p, q):
        assert np.allclose(cr.run(other)["stats"], want, rtol=0, atol=1e-12)


def test_a_duplicate_at_a_lower_score_never_raises_ap():
    """the gt of one class are far apart, so a duplicate can only meet the gt its original met"""
    c = grid_case(jitter=6, seed=4, drop=0.1, extra=1)
    base = cr.run(c)["stats"]
    rs = np.random.RandomState(0)
    for trial in range(6):
        d = dict(c, dets=c["dets"].copy(), det_count=c["det_count"].copy())
        for n in range(6):
            nd = int(d["det_count"][n])
            if nd == 0 or nd >= 16:
                continue
            src = rs.randint(nd)
            d["dets"][n, nd] = d["dets"][n, src]
            d["dets"][n, nd, 4] = d["dets"][n, src, 4] * np.float32(rs.uniform(0.1, 0.9))
            d["det_count"][n] = nd + 1
        got = cr.run(d)["stats"]
        assert np.all(got[:6] <= base[:6] + 1e-12), trial


# ---- every condition the cases name occurs -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ran():
    out = {}
    for name in ("exact_iou", "basic", "overflow", "random", "many_gt", "many_dets", "nondefault"):
        tally = dict.fromkeys(("stop_at_ignored", "equal_iou_later_gt", "iou_equals_threshold", "crowd_rematched", "matched_to_ignored",
                               "unmatched_out_of_range"), 0)
        case = ec.MATCH_CASES[name]()
        out[name] = (case, cr.run(case, tally), tally)
    return out


def bit(word, a, t, T=10):
    return (int(word) >> (a * T + t)) & 1


def test_exact_iou_case(ran):
    case, o, tally = ran["exact_iou"]
    # image 0 / 1 / 2: IoU 1/2, 3/4, 19/20 = thresholds 0, 5, 9; class 1 exact (row 0), class 2 one ulp below (row 1), class 3 above
    assert case["iou_thrs"][0] == 0.5 and case["iou_thrs"][9] == 0.95 and abs(case["iou_thrs"][5] - 0.75) < 1e-15
    for n, t in enumerate((0, 5, 9)):
        frac = (0.5, 0.75, 0.95)[n]
        exact = frac >= case["iou_thrs"][t]                    # linspace's 0.75 may sit an ulp off: the restatement decides as COCO does
        assert bit(o["dt_match"][n, 0], 0, t) == int(exact) and bit(o["dt_match"][n, 1], 0, t) == 0 and bit(o["dt_match"][n, 2], 0, t) == 1
        if t + 1 < 10:
            assert [bit(o["dt_match"][n, r], 0, t + 1) for r in range(3)] == [0, 0, 0]
        if t > 0:
            assert [bit(o["dt_match"][n, r], 0, t - 1) for r in range(3)] == [1, 1, 1]
    assert tally["iou_equals_threshold"] >= 2 * 4
    d = case["dets"]
    assert d[0, 1, 3] < d[0, 0, 3] < d[0, 2, 3] and np.float32(d[0, 0, 3]) == 4.0


def test_engineered_conditions_occur(ran):
    case, o, tally = ran["basic"]
    T = 10
    assert tally["equal_iou_later_gt"] >= T and o["gt_match"][0, 1, 0].tolist() == [0] * T and o["gt_match"][0, 0, 0].tolist() == [-1] * T
    assert tally["crowd_rematched"] >= 2 * T and [int(o["dt_match"][0, r]) & 1 for r in (1, 2, 3)] == [1, 1, 1]
    assert [int(o["dt_ignore"][0, r]) & 1 for r in (1, 2, 3)] == [1, 1, 1] and o["gt_match"][0, 2, 0, 0] == 3
    assert tally["stop_at_ignored"] >= 1 and o["gt_match"][1, 0, 0, 0] == 0 and o["gt_match"][1, 1, 0, 0] == -1
    assert bit(o["dt_match"][1, 0], 0, 1) == 1 and bit(o["dt_ignore"][1, 0], 0, 1) == 0     # t = .55: the plain gt
    assert bit(o["dt_match"][1, 0], 0, 3) == 1 and bit(o["dt_ignore"][1, 0], 0, 3) == 1     # t = .65: only the crowd gt is left
    # matched to a gt out of the area range: ignored, not a false positive (medium, large); an unmatched detection out of range
    assert bit(o["dt_match"][0, 4], 2, 0) == 1 and bit(o["dt_ignore"][0, 4], 2, 0) == 1 and bit(o["dt_ignore"][0, 4], 1, 0) == 0
    assert o["dt_match"][0, 5] == 0 and bit(o["dt_ignore"][0, 5], 2, 0) == 1 and bit(o["dt_ignore"][0, 5], 1, 0) == 0
    assert tally["matched_to_ignored"] > 0 and tally["unmatched_out_of_range"] > 0
    # gt_area against the box area, across 32^2 and 96^2
    assert o["gt_ignore"][1, 2] == 0b1100 and o["gt_ignore"][1, 3] == 0b0110 and 40 * 40 > 32 ** 2 > 900 and 90 * 90 < 96 ** 2 < 10000
    # equal scores within an image and across images; a class with detections and no gt, and the reverse; empty images
    s = case["dets"][:, :, 4]
    assert s[0, 2] == s[0, 3] and s[0, 5] == s[0, 6] and s[0, 0] == s[1, 0] == s[3, 0] == s[3, 1]
    assert o["dt_rank"][0, 2] == 1 and o["dt_rank"][0, 3] == 2 and o["dt_rank"][3, :2].tolist() == [0, 1]
    assert o["npig"][1, 2, 0] == 0 and o["dt_rank"][1, 3] == 0 and o["npig"][2, 0, 0] == 1 and case["det_count"][2] == 0
    assert case["gt_counts"][3] == 0 and case["det_count"][3] == 3 and np.all(o["npig"][3] == 0)
    # rows past the counts: NaN boxes and a class that would count
    assert np.isnan(case["dets"][2, 0, 0]) and case["dets"][2, 0, 5] == 1 and np.isnan(case["gt_boxes"][3, 0, 0]) and case["gt_classes"][3, 0] == 1
    assert np.all(o["sort_key"][2] == cr.PAD_KEY) and np.all(o["dt_rank"][2] == -1)


def test_size_conditions_occur(ran):
    case, o, _ = ran["overflow"]
    assert case["det_count"][0] == 21 > case["dets"].shape[1] == 16 and np.all(o["dt_rank"][0] >= 0)
    case, o, _ = ran["many_gt"]
    cls, n = case["gt_classes"][0], int(case["gt_counts"][0])
    assert (cls[:n] == 1).sum() == 33 and (cls[:n] == 2).sum() == 65
    assert o["gt_match"][0, 32, 0, 0] >= 0 and o["gt_match"][0, 97, 0, 0] >= 0      # the 33rd of class 1, the 65th of class 2: matched
    case, o, _ = ran["many_dets"]
    assert case["dets"].shape[1] == 160 and (case["dets"][0, :150, 5] == 1).sum() == 130
    r = o["dt_rank"][0, :130]
    assert (r == -1).sum() == 30 and sorted(r[r >= 0]) == list(range(100)) and np.all(o["sort_key"][0, :130][r == -1] == cr.PAD_KEY)
    case, o, _ = ran["nondefault"]
    assert o["precision"].shape == (3, 11, 3, 2, 2) and np.all(o["stats"] == -1) and (o["precision"] > 0).any()
    long = ec.long_segment()
    from detectorch_amd import hip_eval
    assert int(long["det_count"].sum()) == 3000 > 4 * hip_eval.ACC_TILE and np.all(long["dets"][:, :, 5] == 1)


def test_sort_keys_at_the_class_limit():
    """num_classes = 1024: (k + 2) << 53 of the last class is 2^63, beyond the padding key; its segment must end at the padding rows"""
    from detectorch_amd import hip_eval
    case = ec.max_classes()
    assert case["num_classes"] == hip_eval.MAX_CLASSES == 1024
    o = cr.run(case)
    keys, rank = o["sort_key"].reshape(-1), o["dt_rank"].reshape(-1)
    cls = np.nan_to_num(case["dets"][:, :, 5]).reshape(-1).astype(int)
    assert (keys == cr.PAD_KEY).sum() == (rank < 0).sum() > 0 and np.all((keys == cr.PAD_KEY) == (rank < 0))
    assert ((cls == 1023) & (rank < 0) & (np.arange(len(cls)) < 16)).sum() == 2                 # image 0: two rows cut by max_det = 5
    worst = (1023 << 53) | (cr.score_key(-np.finfo(np.float32).max) << 21) | ((1 << 21) - 1)    # the largest key of a finite score
    assert keys[rank >= 0].max() < worst < int(cr.PAD_KEY) < (1024 << 53) == 1 << 63
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    for k in (0, 511, 1021, 1022):
        lo, hi = cr.class_segment(skeys, k)
        rows = order[lo:hi]
        assert np.all(rank[rows] >= 0) and np.all(cls[rows] == k + 1) and hi - lo == ((cls == k + 1) & (rank >= 0)).sum() > 0
    assert cr.class_segment(skeys, 1022)[1] == (rank >= 0).sum() < len(keys) and len(set(cr.class_segment(skeys, 5))) == 1
    assert o["counts"][1022].tolist() == [6, 6] and (o["precision"][:, :, 1022] > 0).any() and (o["precision"][:, :, 1022] < 1).any()


# ---- the proposal rounds against the reference ---------------------------------------------------------------------------------------------
def greedy_rounds(props, gt_boxes):
    """the header's rounds on mask_train_ref.bbox_overlaps (pinned to the Cython build): largest remaining overlap, ties to the smallest
    gt and then the smallest proposal"""
    import mask_train_ref as mr
    out = np.zeros(len(gt_boxes))
    if len(props) == 0 or len(gt_boxes) == 0:
        return out
    ov = mr.bbox_overlaps(np.ascontiguousarray(props, np.float32), np.ascontiguousarray(gt_boxes, np.float32)).astype(np.float64)
    for j in range(min(ov.shape)):
        best = ov.max()
        g = int(np.flatnonzero(ov.max(axis=0) == best)[0])
        p = int(np.flatnonzero(ov[:, g] == best)[0])
        out[j] = best
        ov[p, :] = -1
        ov[:, g] = -1
    return out


def split_entry(e, area, limit):
    """-> (proposals, the gt boxes taking part) of a roidb entry, as the reference selects them"""
    lo, hi = ec_area(area)
    g = np.flatnonzero((e['gt_classes'] > 0) & (e['is_crowd'] == 0))
    g = g[(e['seg_areas'][g] >= lo) & (e['seg_areas'][g] <= hi)]
    p = e['boxes'][np.flatnonzero(e['gt_classes'] == 0)]
    return (p if limit is None else p[:limit]), e['boxes'][g], len(p)


def ec_area(area):
    from detectorch_amd.utils.evaluator import PROPOSAL_AREAS
    return PROPOSAL_AREAS[area]


@pytest.mark.parametrize("case", sorted(ec.proposal_cases()))
def test_greedy_rounds_equal_the_reference(case):
    g = golden("eval")
    roidb, limit = ec.proposal_cases()[case]
    rounds, meta, at = g[case + "_rounds"], g[case + "_meta"], 0
    for a, area in enumerate(ec.AREAS):
        for i, e in enumerate(roidb):
            props, gts, n_all = split_entry(e, area, limit)
            n, n_pos = meta[a, i]
            assert n_pos == len(gts) and n == (len(gts) if n_all else 0)          # the image is left out before the limit is applied
            assert np.array_equal(greedy_rounds(props, gts)[:n], rounds[at:at + n])
            at += n
    assert at == len(rounds)


def test_proposal_conditions_occur():
    g, cases = golden("eval"), ec.proposal_cases()
    m = {k: g[k + "_meta"] for k in cases}
    n_props = lambda name, i: int((cases[name][0][i]['gt_classes'] == 0).sum())
    assert n_props("fewer_proposals", 0) < m["fewer_proposals"][0, 0, 1] and n_props("more_proposals", 0) > m["more_proposals"][0, 0, 1] > 0
    assert n_props("no_proposals", 0) == 0 and m["no_proposals"][0, 0].tolist() == [0, 7] and m["no_gt"][0, 0].tolist() == [0, 0]
    r = g["duplicates_rounds"][:7]
    assert r[0] == r[1] == 1.0 and len(set(r.tolist())) < 7                       # the duplicated gt and its two exact proposals
    z = g["zero_overlap_late_rounds"][:4]
    assert z[3] == 0.0 and z[2] > 0.0 and n_props("zero_overlap_late", 0) > 4      # a zero overlap chosen in the last round
    assert cases["limit_below"][1] == 4 < n_props("limit_below", 0) < cases["limit_above"][1] and (g["limit_below_rounds"][4:7] == 0).all()
    e = cases["crowd_and_class0"][0][0]
    assert e['is_crowd'][:6].sum() == 2 and e['gt_classes'][1] == 0 and m["crowd_and_class0"][0, 0, 1] == 3
    assert n_props("p600_g40", 0) == 600 > 2 * 256 and m["p600_g40"][0, 0, 1] == 40
    lz = g["limit_zero_meta"]
    assert cases["limit_zero"][1] == 0 and lz[0, 0].tolist() == [7, 7] and lz[0, 1].tolist() == [0, 4] and not g["limit_zero_rounds"].any()
    for name in cases:                                                             # each of the eight area ranges selects some gt somewhere
        assert m[name].shape[0] == 8
    assert all(any(m[name][a, :, 1].sum() > 0 for name in cases) for a in range(8))
    assert any(0 < m[name][a, :, 1].sum() < m[name][0, :, 1].sum() for name in cases for a in range(1, 8))


# ---- the library: exports, binding, header, constants -----------------------------------------------------------------------------------
NAMES = ["dtc_eval_accumulate", "dtc_eval_match", "dtc_eval_proposal_recall", "dtc_eval_target_arch"]


def test_header_symbols_are_exported_and_bound():
    from make_native_host_codes import exports
    from test_binding_signatures_host import prototypes
    from detectorch_amd import hip_eval
    L = hip_eval.lib()
    protos = prototypes("detectorch_eval_hip.h")
    assert sorted(protos) == NAMES and exports(hip_eval.LIB_PATH) == NAMES and sorted(hip_eval.SIGNATURES) == NAMES
    for entry, (ret, params) in protos.items():
        row = hip_eval.SIGNATURES[entry]
        assert row[0] == ret and [n for n, _ in row[1]] == [n for n, _ in params], entry
        assert [k for _, k in row[1]] == [k for _, k in params], entry
    assert L.dtc_eval_target_arch() == b"gfx950"


def test_the_other_libraries_export_nothing_of_the_evaluation():
    from make_native_host_codes import exports
    from detectorch_amd import build, hip, hip_grad, hip_loss, hip_mask, hip_optim, hip_rpn, hip_train
    build.build()
    for mod in (hip, hip_train, hip_loss, hip_grad, hip_optim, hip_rpn, hip_mask):
        if mod is not hip:
            mod.lib()
        assert not [n for n in exports(mod.LIB_PATH) if n.startswith("dtc_eval")], mod.__name__


@pytest.mark.parametrize("compiler,flags", [("gcc", ["-std=c99"]), ("g++", ["-std=c++11"])])
def test_header_compiles_as_pedantic_c99_and_cxx11(tmp_path, compiler, flags):
    cc = shutil.which(compiler) or shutil.which({"gcc": "cc", "g++": "c++"}[compiler])
    assert cc, compiler + " not found"
    src = tmp_path / ("use_header" + {"gcc": ".c", "g++": ".cpp"}[compiler])
    src.write_text('#include "detectorch_eval_hip.h"\nint use(void) { return DTC_EVAL_MAX_GT + DTC_EVAL_MAX_IMAGES; }\n')
    subprocess.check_call([cc] + flags + ["-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                                          str(tmp_path / "use_header.o")])


def test_constants_are_those_of_the_source():
    from detectorch_amd import hip_eval
    src = lambda name: open(os.path.join(ROOT, "detectorch_amd", "csrc", "eval", name)).read()
    const = lambda name, s: int(re.search(r"constexpr int %s = (\d+);" % name, s).group(1))
    assert const("kAccTile", src("eval_accumulate.hip")) == hip_eval.ACC_TILE
    assert const("kPropThreads", src("proposal_recall.hip")) == hip_eval.PROP_BLOCK
    header = open(os.path.join(ROOT, "include", "detectorch_eval_hip.h")).read()
    define = lambda name: eval(re.search(r"#define DTC_EVAL_MAX_%s (\(?[\d <]+\)?)" % name, header).group(1))
    for name, want in (("GT", hip_eval.MAX_GT), ("OUT", hip_eval.MAX_OUT), ("PAIRS", hip_eval.MAX_PAIRS), ("AREAS", hip_eval.MAX_AREAS),
                       ("CLASSES", hip_eval.MAX_CLASSES), ("BATCH", hip_eval.MAX_BATCH), ("IMAGES", hip_eval.MAX_IMAGES),
                       ("ROWS", hip_eval.MAX_ROWS), ("REC_THRS", hip_eval.MAX_REC_THRS), ("MAX_DETS", hip_eval.MAX_MAX_DETS),
                       ("PROPOSALS", hip_eval.MAX_PROPOSALS)):
        assert define(name) == want, name


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_wrappers_raise_on_cpu_tensors():
    import torch
    from detectorch_amd import hip_eval
    from detectorch_amd.utils import evaluator
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
    i32, f64 = torch.int32, torch.float64
    gt = dict(gt_boxes=z(1, 2, 4), gt_classes=z(1, 2, dt=i32), gt_is_crowd=z(1, 2, dt=i32), gt_counts=z(1, dt=i32))
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_eval.eval_match(z(1, 4, 6), z(1, dt=i32), gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"], None, 3,
                            z(10, dt=f64), z(4, 2, dt=f64), 100)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_eval.eval_accumulate(z(4, dt=i32), z(4, dt=torch.int64), z(4, dt=torch.int64), z(4, dt=torch.int64), z(1, 2, 4, dt=i32), 3, 10,
                                 4, z(101, dt=f64), z(3, dt=i32))
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_eval.proposal_recall(z(1, 5, 4), z(1, dt=i32), gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"], None,
                                 z(2, dt=f64))
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluator.evaluate_box_proposals_batched(z(1, 5, 4), z(1, dt=i32), gt)
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluator.BoxEvaluator(device="cpu")
    with pytest.raises(ValueError):
        evaluator.BoxEvaluator(on_overflow="ignore")
    with pytest.raises(ValueError, match="area must be one of"):
        evaluator.evaluate_box_proposals_batched(z(1, 5, 4), z(1, dt=i32), gt, area="huge")
    with pytest.raises(ValueError, match="limit must be"):
        evaluator.evaluate_box_proposals_batched(z(1, 5, 4), z(1, dt=i32), gt, limit=-1)
    with pytest.raises(ValueError, match="max_dets must be non-decreasing"):
        evaluator.BoxEvaluator(max_dets=(10, 1, 100))


BOGUS = 256                                                                  # a bogus, non-NULL, 16-byte aligned device pointer
EINVAL, EUNSUPPORTED = -1, -4
M_PTRS = ("dets", "det_count", "gt_boxes", "gt_classes", "gt_is_crowd", "gt_counts", "gt_area", "iou_thrs", "area_rngs", "dt_rank",
          "dt_match", "dt_ignore", "gt_ignore", "gt_match", "npig", "sort_key")
M_INTS = dict(batch=3, max_out=16, G=12, num_classes=4, T=10, A=4, max_det=100, image_base=0)
A_PTRS = ("dt_rank", "dt_match", "dt_ignore", "sort_key", "order", "npig", "rec_thrs", "max_dets", "precision", "recall", "counts")
A_INTS = dict(rows=48, images=3, num_classes=4, T=10, A=4, R=101, M=3)
P_PTRS = ("proposals", "prop_counts", "gt_boxes", "gt_classes", "gt_is_crowd", "gt_counts", "gt_area", "area_rng", "gt_overlaps", "n_pos",
          "n_overlaps")
P_INTS = dict(batch=2, P=600, G=40, limit=0)

M_CODES = {
    "batch 0": (dict(batch=0), EINVAL), "max_out 0": (dict(max_out=0), EINVAL), "G -1": (dict(G=-1), EINVAL),
    "one class": (dict(num_classes=1), EINVAL), "T 0": (dict(T=0), EINVAL), "A 0": (dict(A=0), EINVAL), "max_det 0": (dict(max_det=0), EINVAL),
    "image_base -1": (dict(image_base=-1), EINVAL), "max_out 513 + T 0": (dict(max_out=513, T=0), EINVAL),
    "max_out 513": (dict(max_out=513), EUNSUPPORTED), "G 257": (dict(G=257), EUNSUPPORTED), "T x A 65": (dict(T=13, A=5), EUNSUPPORTED),
    "A 17": (dict(T=1, A=17), EUNSUPPORTED), "1025 classes": (dict(num_classes=1025), EUNSUPPORTED),
    "batch 65536": (dict(batch=65536), EUNSUPPORTED), "image_base 2^21 - 2": (dict(image_base=(1 << 21) - 2), EUNSUPPORTED),
    "G 257 + dets NULL": (dict(G=257, dets=None), EUNSUPPORTED),
    **{k + " NULL": ({k: None}, EINVAL) for k in M_PTRS if k != "gt_area"},
    "gt_boxes misaligned": (dict(gt_boxes=BOGUS + 4), EINVAL),
}
A_CODES = {
    "rows 0": (dict(rows=0), EINVAL), "images 0": (dict(images=0), EINVAL), "one class": (dict(num_classes=1), EINVAL),
    "R 0": (dict(R=0), EINVAL), "M 0": (dict(M=0), EINVAL), "R 1025 + M 0": (dict(R=1025, M=0), EINVAL),
    "rows 2^30 + 1": (dict(rows=(1 << 30) + 1), EUNSUPPORTED), "R 1025": (dict(R=1025), EUNSUPPORTED), "M 17": (dict(M=17), EUNSUPPORTED),
    "T x A 65": (dict(T=13, A=5), EUNSUPPORTED), "M 17 + order NULL": (dict(M=17, order=None), EUNSUPPORTED),
    **{k + " NULL": ({k: None}, EINVAL) for k in A_PTRS},
}
P_CODES = {
    "batch 0": (dict(batch=0), EINVAL), "P 0": (dict(P=0), EINVAL), "G -1": (dict(G=-1), EINVAL), "limit -1": (dict(limit=-1), EINVAL),
    "P 65537 + batch 0": (dict(P=65537, batch=0), EINVAL),
    "P 65537": (dict(P=65537), EUNSUPPORTED), "G 257": (dict(G=257), EUNSUPPORTED), "batch 65536": (dict(batch=65536), EUNSUPPORTED),
    "G 257 + n_pos NULL": (dict(G=257, n_pos=None), EUNSUPPORTED),
    **{k + " NULL": ({k: None}, EINVAL) for k in P_PTRS if k != "gt_area"},
    "proposals misaligned": (dict(proposals=BOGUS + 8), EINVAL), "gt_boxes misaligned": (dict(gt_boxes=BOGUS + 4), EINVAL),
}


def _call(L, entry, ptrs, ints, names, kw):
    kw = dict(kw)
    n = dict(ints, **{k: kw.pop(k) for k in list(kw) if k in ints})
    ptr = {k: kw.pop(k, BOGUS) for k in ptrs}
    assert not kw
    args = [(None if ptr[k] is None else C.c_void_p(ptr[k])) if k in ptr else n[k] for k in names]
    return getattr(L, entry)(*args, None)


def test_return_codes_on_bad_arguments():
    """every row returns before the first launch: nothing is enqueued, the bogus pointers are never used"""
    from detectorch_amd import hip_eval
    L = hip_eval.lib()
    m_order = ("dets", "det_count", "gt_boxes", "gt_classes", "gt_is_crowd", "gt_counts", "gt_area", "batch", "max_out", "G", "num_classes",
               "iou_thrs", "T", "area_rngs", "A", "max_det", "image_base", "dt_rank", "dt_match", "dt_ignore", "gt_ignore", "gt_match", "npig",
               "sort_key")
    a_order = ("dt_rank", "dt_match", "dt_ignore", "sort_key", "order", "rows", "npig", "images", "num_classes", "T", "A", "rec_thrs", "R",
               "max_dets", "M", "precision", "recall", "counts")
    p_order = ("proposals", "prop_counts", "gt_boxes", "gt_classes", "gt_is_crowd", "gt_counts", "gt_area", "batch", "P", "G", "area_rng",
               "limit", "gt_overlaps", "n_pos", "n_overlaps")
    for entry, ptrs, ints, order, codes in (("dtc_eval_match", M_PTRS, M_INTS, m_order, M_CODES),
                                            ("dtc_eval_accumulate", A_PTRS, A_INTS, a_order, A_CODES),
                                            ("dtc_eval_proposal_recall", P_PTRS, P_INTS, p_order, P_CODES)):
        got = {k: _call(L, entry, ptrs, ints, order, kw) for k, (kw, _) in codes.items()}
        assert got == {k: v[1] for k, v in codes.items()}, entry
    assert len(M_CODES) >= 30 and len(A_CODES) >= 20 and len(P_CODES) >= 18
