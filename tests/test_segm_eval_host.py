"""The mask evaluation without a GPU (tests/README_segm_eval.md):
  * the numpy restatement (tests/segm_eval_ref.py) against answers known without it, and -- the bridge -- against the box protocol's
    restatement (tests/coco_eval_ref.py) on filled integer rectangles, bit for bit;
  * the interval form of the counts (for the image too large to decode) against the bitmaps on every other case;
  * every condition the cases of tests/segm_eval_cases.py are named for occurs in them;
  * libdetectorch_segm_hip.so exports exactly what include/detectorch_segm_hip.h declares and hip_segm.SIGNATURES binds it, parameter
    names and kinds in order; the header compiles as pedantic C99 and C++11; the other libraries export nothing of it;
  * CPU tensors are refused; the return codes of the entries on bad arguments, in the documented order (validation precedes every
    HIP call, so nothing is launched); the constants of the binding are those of the source text;
  * result_utils.rle_string_to_counts inverts _rle_counts_to_string; pack_gt_masks takes bitmaps, uncompressed and compressed RLEs.
The first three pin the yardstick and pass whatever the library does; the others need the feature."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import coco_eval_ref as cr
import segm_eval_cases as sc
import segm_eval_ref as sr

sys.path.insert(0, GOLDEN)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the restatement against known answers ---------------------------------------------------------------------------------------------------
def iou_of(d, g, hw, crowd=False):
    return sr.mask_iou(sr.decode(np.asarray(d[0], np.uint32), d[1], hw), sr.decode(np.asarray(g[0], np.uint32), g[1], hw), crowd)


def L(runs, n=None):
    return (runs, len(runs) if n is None else n)


def test_known_answers():
    hw = 35
    blob = L([9, 20, 6])
    assert iou_of(blob, blob, hw) == (1.0, 20, 20, 20)                                        # a mask against itself
    assert iou_of(L([0, 10, 25]), L([10, 25]), hw) == (0.0, 0, 10, 25)                        # disjoint
    assert iou_of(L([12, 5, 18]), L([9, 20, 6]), hw, crowd=True) == (1.0, 5, 5, 20)           # inside a crowd gt: exactly 1
    assert iou_of(L([12, 5, 18]), L([9, 20, 6]), hw)[0] == np.float64(5) / np.float64(20)
    for empty in (L([]), L([hw]), L([0, hw], 0), L([0, hw], -3)):
        iou, i, da, ga = iou_of(empty, L([hw]), hw)
        assert iou == 0.0 and not np.isnan(iou) and (i, da, ga) == (0, 0, 0)                  # both empty: 0, not NaN
        assert iou_of(empty, empty, hw, crowd=True)[0] == 0.0
    assert sr.decode(np.array([0, 3, 32], np.uint32), 3, hw).nonzero()[0].tolist() == [0, 1, 2]            # a zero-length first run
    assert sr.decode(np.array([3, 4, 0, 2, 5, 0, 0, 6, 1], np.uint32), 9, hw).nonzero()[0].tolist() == [3, 4, 5, 6, 7, 8] + list(range(14, 20))
    assert sr.decode(np.array([2, 5, 3, 4], np.uint32), 4, hw).sum() == 9                                  # short of h * w: zeros behind
    assert sr.decode(np.array([29, 4, 1, 100, 7, 9], np.uint32), 6, hw).nonzero()[0].tolist() == [29, 30, 31, 32, 34]   # past h * w: cut
    assert sr.decode(np.array([10, 0xffffffff, 0xffffffff, 5], np.uint32), 4, hw).sum() == 25              # no wrap at 2^32
    assert sr.decode(np.array([0, 35, 7, 7], np.uint32), 9, hw).all()                                      # the count clamped to the list
    # column-major: position x * h + y
    m = np.zeros((7, 5), bool)
    m[2:5, 1:3] = True
    assert np.array_equal(sr.decode(np.asarray(sc.runs_of(m), np.uint32), len(sc.runs_of(m)), hw).reshape(5, 7).T, m)
    assert sc.rect_runs(7, 1, 2, 2, 4) == sc.runs_of(m)[:-1] and sc.rect_runs(7, 1, 0, 2, 6) == [7, 7, 0, 7]
    assert sr.pixels((7.9, 5.2)) == 35 and sr.pixels((np.nan, 5)) == 0 and sr.pixels((0.5, 5)) == 0 and sr.pixels((1e6, 1e6)) == 1 << 30


# ---- the bridge to the box protocol -----------------------------------------------------------------------------------------------------------
_BRIDGE = {}


def bridge(name, with_gt_area):
    """(box case, segm case, the box restatement's answer, the segm restatement's), computed once"""
    key = (name, with_gt_area)
    if key not in _BRIDGE:
        b, s = sc.from_boxes(sc.BOX_CASES[name](), with_gt_area=with_gt_area)
        _BRIDGE[key] = (b, s, cr.run(b), sr.run(s))
    return _BRIDGE[key]


RECORDS = ("dt_rank", "dt_match", "dt_ignore", "gt_ignore", "gt_match", "npig", "sort_key")


@pytest.mark.parametrize("with_gt_area", [True, False])
@pytest.mark.parametrize("name", sorted(sc.BOX_CASES))
def test_filled_rectangles_equal_the_box_protocol(name, with_gt_area):
    """pixel counts of integer rectangles are the box protocol's (x2 - x1 + 1)(y2 - y1 + 1), intersections likewise, all exact in
    float64: the records, precision, recall and stats are the same bits"""
    b, s, want, got = bridge(name, with_gt_area)
    N, max_out = b["dets"].shape[:2]
    for n in range(N):
        for d in range(min(int(b["det_count"][n]), max_out)):
            x, y, w, h = cr.xywh(b["dets"][n, d, :4])
            assert got["det_area"][n, d] == w * h
            for g in range(int(b["gt_counts"][n])):
                if b["gt_classes"][n, g] == b["dets"][n, d, 5]:
                    box = cr.bb_iou((x, y, w, h), cr.xywh(b["gt_boxes"][n, g]), bool(b["gt_is_crowd"][n, g]))
                    assert same_bits(np.float64(got["iou"][n, d, g]), np.float64(box))
    for k in RECORDS:
        assert same_bits(got[k], want[k]), k
    assert np.array_equal(got["counts"], want["counts"])
    for k in ("precision", "recall", "stats"):
        assert same_bits(got[k], want[k]), k
    assert (want["dt_match"] != 0).any()


def test_bridge_conditions_occur():
    b, s, want, _ = bridge("exact_rects", True)
    bit = lambda word, a, t: (int(word) >> (a * 10 + t)) & 1
    for n, t in enumerate((0, 5, 9)):                          # IoU 1/2, 3/4, 19/20 exactly (class 1), a row below (2) and above (3)
        exact = (0.5, 0.75, 0.95)[n] >= b["iou_thrs"][t]
        assert [bit(want["dt_match"][n, r], 0, t) for r in range(3)] == [int(exact), 0, 1]
    tally = dict.fromkeys(("stop_at_ignored", "equal_iou_later_gt", "iou_equals_threshold", "crowd_rematched", "matched_to_ignored",
                           "unmatched_out_of_range"), 0)
    sr.run(sc.from_boxes(sc.BOX_CASES["basic"]())[1], tally)
    assert all(v > 0 for k, v in tally.items() if k != "iou_equals_threshold"), tally      # crowd, ties, out-of-range areas, the stop
    sr.run(s, tally)
    assert tally["iou_equals_threshold"] >= 2
    b, s, want, _ = bridge("many_dets", True)
    assert (want["dt_rank"][0, :130] == -1).sum() == 30           # the max_det cut
    b, s, _, _ = bridge("overflow", True)
    assert b["det_count"][0] > b["dets"].shape[1] and s["det_count"][0] == b["det_count"][0]
    b, s, want, _ = bridge("nondefault", True)
    assert want["precision"].shape == (3, 11, 3, 2, 2)
    # a column-high rectangle has zero-length runs of zeros inside
    assert 0 in sc.rect_runs(10, 2, 0, 4, 9)[1:]


# ---- the interval form, and the conditions of the IoU cases -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ran():
    return {name: (lambda c: (c, sr.run(c)))(make()) for name, make in sc.IOU_CASES.items()}


def test_interval_counts_equal_the_bitmaps(ran):
    for name, (case, want) in ran.items():
        got = sr.iou_matrix(case, sr.interval_counts)
        for k in ("iou", "det_area", "gt_mask_area", "n_bad"):
            assert same_bits(got[k], want[k]), (name, k)


def one_runs(runs, n, hw):
    e = sr.run_ends(runs, n, hw)
    return sum(1 for j in range(1, len(e), 2) if e[j] > e[j - 1])


def test_iou_cases_hold_their_conditions(ran):
    case, o = ran["tiny"]
    assert case["im_size"].tolist() == [[7, 5], [5, 7]] and case["det_runs"].shape[2] == 36 != case["gt_runs"].shape[2]
    n_runs = case["det_n_runs"][0, :14]
    assert 36 in n_runs and 35 in n_runs and 0 in n_runs and (n_runs < 0).sum() == 1             # n_runs == stride, == h * w, empty, bad
    areas = sorted(o["det_area"][0, :14].tolist())
    assert areas[:4] == [0, 0, 0, 0] and 35 in areas and areas.count(1) == 2 and areas.count(17) == 2
    assert o["n_bad"].tolist() == [1, 1]
    iou = o["iou"][0, :14, :14]
    assert (iou == 1.0).sum() >= 10 and (iou == 0.0).sum() >= 40 and len(np.unique(iou)) > 12
    assert np.all(o["iou"][:, 16:18] == 0) and np.all(o["iou"][:, :, 16:18] == 0)                  # classes 7 and 0, 3 and 0: no pair
    assert o["det_area"][0, 16] == 0 and o["det_area"][0, 17] == 0 and o["gt_mask_area"][0, 17] == 0 and o["gt_mask_area"][0, 16] == 35
    assert case["det_n_runs"][0, 18] != 0 and case["dets"][0, 18, 5] == 1                          # garbage past the count
    assert (o["iou"][0, 14, 14], o["iou"][0, 15, 14]) == (10.0 / 20.0, 17.0 / 35.0)                 # a crowd gt: i / da

    case, o = ran["random_masks"]
    hw = 37 * 53
    ones = [one_runs(case["det_runs"][0, d], case["det_n_runs"][0, d], hw) for d in range(6)]
    assert max(ones) > 3 * 64 and min(ones) > 64                                                 # several strides of the lane loop
    assert case["gt_n_runs"][0, :4].max() > 900 and case["gt_n_runs"][0, :4].min() > 256           # binary searches deeper than 8
    assert case["det_runs"].shape[2] == 1200 != case["gt_runs"].shape[2] == 1100
    pairs = o["iou"][o["iou"] > 0]
    assert len(pairs) >= 20 and pairs.min() < 0.1 and pairs.max() > 0.7 and case["gt_is_crowd"][:, 3].all()

    case, o = ran["large"]
    assert o["det_area"][0, 0] > 1 << 16 and o["gt_mask_area"][0, 0] > 1 << 16 and case["det_n_runs"][0, 0] > 1000
    assert 0 < o["iou"][0, 0, 0] < 1 and int(case["det_runs"][0, 0, 0]) > 1 << 16

    case, o = ran["counts"]
    assert o["n_bad"].tolist() == [2, 0, 0, 0, 0] and case["det_count"].tolist() == [5, 2, 0, 9, -5]
    assert case["gt_counts"].tolist() == [3, 0, 2, 2, 1] and not o["iou"][1].any() and not o["iou"][2].any() and not o["iou"][4].any()
    assert o["det_area"][0].tolist() == [54, 0, 27, 0, 1, 0] and o["iou"][0, 0].tolist() == [0.5, 0.0, 1.0 / 54.0]
    assert o["det_area"][3].tolist() == [27] * 6 and o["det_area"][4].tolist() == [0] * 6 and o["gt_mask_area"][2].tolist() == [27, 54, 0]
    assert o["gt_ignore"][0, 2] == 0b1100 and o["gt_ignore"][0, 0] == 0b1010 and case["gt_area"][0, 0] == 2000      # gt_area, not the 27 pixels


def test_huge_case_by_intervals():
    case = sc.huge()
    o = sr.iou_matrix(case, sr.interval_counts)
    hw = 900000000
    assert sr.pixels(case["im_size"][0]) == hw
    i, u = hw - 12345, hw - 1000
    assert i > 8.9e8 and int(np.float32(i)) != i                                                     # a float32 sum would lose it
    assert o["iou"][0, 0].tolist() == [np.float64(i) / np.float64(u), 7.0 / u, 0.0] and o["det_area"][0, 0] == u


def test_crafted_matrices_hold_their_conditions():
    for params in (None, sc.NONDEFAULT_PARAMS):
        for with_gt_area in (False, True):
            case, iou, det_area, gt_mask_area = sc.crafted(params, with_gt_area)
            tally = dict.fromkeys(("stop_at_ignored", "equal_iou_later_gt", "iou_equals_threshold", "crowd_rematched",
                                   "matched_to_ignored", "unmatched_out_of_range"), 0)
            rec, _ = sr.match_records(case, iou, det_area, gt_mask_area, tally)
            assert all(v > 0 for v in tally.values()), tally
            T = len(case["iou_thrs"])
            t = min(1, T - 1)
            bit = lambda word, a, tt: (int(word) >> (a * T + tt)) & 1
            assert [bit(rec["dt_match"][0, r], 0, t) for r in range(3)] == [0, 1, 1]               # an ulp below, at, an ulp above
            assert [bit(rec["dt_match"][0, r], 0, t - 1) for r in range(3)] == [1, 1, 1]
            assert rec["gt_match"][0, 4, 0, 0] == 3 and rec["gt_match"][0, 3, 0, 0] == 4            # equal IoU: the later gt
            assert rec["gt_match"][0, 5, 0, 0] == 5 and rec["gt_match"][0, 6, 0, 0] == 6            # stopped at the crowd gt; met again
            assert rec["gt_ignore"][0].tolist() != rec["gt_ignore"][1].tolist()
    ig = [sr.match_records(*sc.crafted(None, with_gt_area))[0]["gt_ignore"] for with_gt_area in (False, True)]
    assert not np.array_equal(*ig)                                                               # gt_area, where given, sets the ranges


# ---- the library: exports, binding, header, constants -----------------------------------------------------------------------------------
NAMES = ["dtc_segm_iou", "dtc_segm_iou_workspace_bytes", "dtc_segm_match", "dtc_segm_target_arch"]


def test_header_symbols_are_exported_and_bound():
    from make_native_host_codes import exports
    from test_binding_signatures_host import prototypes
    from detectorch_amd import hip_segm
    lib = hip_segm.lib()
    protos = prototypes("detectorch_segm_hip.h")
    assert sorted(protos) == NAMES and exports(hip_segm.LIB_PATH) == NAMES and sorted(hip_segm.SIGNATURES) == NAMES
    for entry, (ret, params) in protos.items():
        row = hip_segm.SIGNATURES[entry]
        assert row[0] == ret and [n for n, _ in row[1]] == [n for n, _ in params], entry
        assert [k for _, k in row[1]] == [k for _, k in params], entry
    assert lib.dtc_segm_target_arch() == b"gfx950"


def test_the_other_libraries_export_nothing_of_the_mask_evaluation():
    from make_native_host_codes import exports
    from detectorch_amd import build, hip, hip_eval, hip_grad, hip_loss, hip_mask, hip_optim, hip_rpn, hip_train
    build.build()
    for mod in (hip, hip_train, hip_loss, hip_grad, hip_optim, hip_rpn, hip_mask, hip_eval):
        if mod is not hip:
            mod.lib()
        assert not [n for n in exports(mod.LIB_PATH) if n.startswith("dtc_segm_")], mod.__name__      # (dtc_segment_sort_desc is hip's)


@pytest.mark.parametrize("compiler,flags", [("gcc", ["-std=c99"]), ("g++", ["-std=c++11"])])
def test_header_compiles_as_pedantic_c99_and_cxx11(tmp_path, compiler, flags):
    cc = shutil.which(compiler) or shutil.which({"gcc": "cc", "g++": "c++"}[compiler])
    assert cc, compiler + " not found"
    src = tmp_path / ("use_header" + {"gcc": ".c", "g++": ".cpp"}[compiler])
    src.write_text('#include "detectorch_segm_hip.h"\nint use(void) { return DTC_SEGM_MAX_RUNS + DTC_SEGM_MAX_PIXELS / DTC_EVAL_MAX_GT; }\n')
    subprocess.check_call([cc] + flags + ["-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                                          str(tmp_path / "use_header.o")])


def test_constants_are_those_of_the_source():
    from detectorch_amd import hip_eval, hip_segm
    src = open(os.path.join(ROOT, "detectorch_amd", "csrc", "segm_eval", "segm_iou.hip")).read()
    assert int(re.search(r"constexpr int kSegmPairWaves = (\d+);", src).group(1)) == hip_segm.PAIR_WAVES
    assert hip_segm.PAIR_WAVES * 64 >= hip_eval.MAX_GT                                              # one thread per gt row
    header = open(os.path.join(ROOT, "include", "detectorch_segm_hip.h")).read()
    define = lambda name: eval(re.search(r"#define DTC_SEGM_MAX_%s (\(?[\d <]+\)?)" % name, header).group(1))
    assert define("RUNS") == hip_segm.MAX_RUNS == 1 << 20 and define("PIXELS") == hip_segm.MAX_PIXELS == sr.MAX_PIXELS == 1 << 30
    assert (hip_segm.MAX_GT, hip_segm.MAX_OUT, hip_segm.MAX_BATCH) == (hip_eval.MAX_GT, hip_eval.MAX_OUT, hip_eval.MAX_BATCH)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_wrappers_raise_on_cpu_tensors():
    import torch
    from detectorch_amd import hip_segm
    from detectorch_amd.utils import evaluator
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
    i32, f64 = torch.int32, torch.float64
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_segm.segm_iou(z(1, 4, 6), z(1, dt=i32), z(1, 4, 8, dt=i32), z(1, 4, dt=i32), z(1, 2), z(1, 2, 8, dt=i32), z(1, 2, dt=i32),
                          z(1, 2, dt=i32), z(1, 2, dt=i32), z(1, dt=i32), 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_segm.segm_match(z(1, 4, 6), z(1, dt=i32), z(1, 4, 2, dt=f64), z(1, 4, dt=i32), z(1, 2, dt=i32), z(1, 2, dt=i32), z(1, dt=i32),
                            None, z(1, 2, dt=i32), 3, z(10, dt=f64), z(4, 2, dt=f64), 100)
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluator.MaskEvaluator(device="cpu")
    with pytest.raises(ValueError):
        evaluator.MaskEvaluator(on_overflow="ignore")


BOGUS = 256                                                                  # a bogus, non-NULL, 16-byte aligned device pointer
EINVAL, EUNSUPPORTED = -1, -4
I_ORDER = ("dets", "det_count", "det_runs", "det_n_runs", "im_size", "gt_runs", "gt_n_runs", "gt_classes", "gt_is_crowd", "gt_counts", "batch",
           "max_out", "det_stride", "G", "gt_stride", "num_classes", "workspace", "workspace_bytes", "iou", "det_area", "gt_mask_area", "n_bad")
I_INTS = dict(batch=3, max_out=16, det_stride=64, G=12, gt_stride=48, num_classes=4, workspace_bytes=1 << 20)
M_ORDER = ("dets", "det_count", "iou", "det_area", "gt_classes", "gt_is_crowd", "gt_counts", "gt_area", "gt_mask_area", "batch", "max_out", "G",
           "num_classes", "iou_thrs", "T", "area_rngs", "A", "max_det", "image_base", "dt_rank", "dt_match", "dt_ignore", "gt_ignore", "gt_match",
           "npig", "sort_key")
M_INTS = dict(batch=3, max_out=16, G=12, num_classes=4, T=10, A=4, max_det=100, image_base=0)
I_PTRS = tuple(k for k in I_ORDER if k not in I_INTS)
M_PTRS = tuple(k for k in M_ORDER if k not in M_INTS)

I_CODES = {
    "batch 0": (dict(batch=0), EINVAL), "max_out 0": (dict(max_out=0), EINVAL), "det_stride 0": (dict(det_stride=0), EINVAL),
    "gt_stride 0": (dict(gt_stride=0), EINVAL), "G -1": (dict(G=-1), EINVAL), "one class": (dict(num_classes=1), EINVAL),
    "max_out 513 + one class": (dict(max_out=513, num_classes=1), EINVAL), "G 257 + batch 0": (dict(G=257, batch=0), EINVAL),
    "max_out 513": (dict(max_out=513), EUNSUPPORTED), "G 257": (dict(G=257), EUNSUPPORTED), "batch 65536": (dict(batch=65536), EUNSUPPORTED),
    "det_stride 2^20 + 1": (dict(det_stride=(1 << 20) + 1), EUNSUPPORTED), "gt_stride 2^20 + 1": (dict(gt_stride=(1 << 20) + 1), EUNSUPPORTED),
    "1025 classes": (dict(num_classes=1025), EUNSUPPORTED), "G 257 + dets NULL": (dict(G=257, dets=None), EUNSUPPORTED),
    "1025 classes + workspace 0": (dict(num_classes=1025, workspace_bytes=0), EUNSUPPORTED),
    **{k + " NULL": ({k: None}, EINVAL) for k in I_PTRS},
    "workspace misaligned": (dict(workspace=BOGUS + 8), EINVAL), "workspace one byte short": (dict(workspace_bytes=-1), EINVAL),
}
M_CODES = {
    "batch 0": (dict(batch=0), EINVAL), "max_out 0": (dict(max_out=0), EINVAL), "G -1": (dict(G=-1), EINVAL),
    "one class": (dict(num_classes=1), EINVAL), "T 0": (dict(T=0), EINVAL), "A 0": (dict(A=0), EINVAL), "max_det 0": (dict(max_det=0), EINVAL),
    "image_base -1": (dict(image_base=-1), EINVAL), "max_out 513 + T 0": (dict(max_out=513, T=0), EINVAL),
    "max_out 513": (dict(max_out=513), EUNSUPPORTED), "G 257": (dict(G=257), EUNSUPPORTED), "T x A 65": (dict(T=13, A=5), EUNSUPPORTED),
    "A 17": (dict(T=1, A=17), EUNSUPPORTED), "1025 classes": (dict(num_classes=1025), EUNSUPPORTED),
    "batch 65536": (dict(batch=65536), EUNSUPPORTED), "image_base 2^21 - 2": (dict(image_base=(1 << 21) - 2), EUNSUPPORTED),
    "G 257 + dets NULL": (dict(G=257, dets=None), EUNSUPPORTED),
    **{k + " NULL": ({k: None}, EINVAL) for k in M_PTRS if k not in ("gt_area", "gt_mask_area")},
    "gt_area and gt_mask_area NULL": (dict(gt_area=None, gt_mask_area=None), EINVAL),
}
M_OK_NULLS = ({"gt_area": None}, {"gt_mask_area": None})                       # either alone may be NULL: checked on the GPU


def _call(lib, entry, order, ints, kw):
    kw = dict(kw)
    n = dict(ints, **{k: kw.pop(k) for k in list(kw) if k in ints})
    ptr = {k: kw.pop(k, BOGUS) for k in order if k not in ints}
    assert not kw
    return getattr(lib, entry)(*[(None if ptr[k] is None else C.c_void_p(ptr[k])) if k in ptr else n[k] for k in order], None)


def test_return_codes_on_bad_arguments():
    """every row returns before the first launch: nothing is enqueued, the bogus pointers are never used"""
    from detectorch_amd import hip_segm
    lib = hip_segm.lib()
    need = lib.dtc_segm_iou_workspace_bytes(*[I_INTS[k] for k in ("batch", "max_out", "det_stride", "G", "gt_stride")])
    assert 0 < need <= I_INTS["workspace_bytes"] and need % 16 == 0
    I_CODES["workspace one byte short"] = (dict(workspace_bytes=need - 1), EINVAL)
    for entry, order, ints, codes in (("dtc_segm_iou", I_ORDER, I_INTS, I_CODES), ("dtc_segm_match", M_ORDER, M_INTS, M_CODES)):
        got = {k: _call(lib, entry, order, ints, kw) for k, (kw, _) in codes.items()}
        assert got == {k: v[1] for k, v in codes.items()}, entry
    assert len(I_CODES) >= 30 and len(M_CODES) >= 30


def test_workspace_bytes():
    from detectorch_amd import hip_segm
    f = hip_segm.lib().dtc_segm_iou_workspace_bytes
    assert f(0, 16, 64, 12, 48) == 0 and f(3, 513, 64, 12, 48) == 0 and f(3, 16, 64, 257, 48) == 0 and f(3, 16, (1 << 20) + 1, 12, 48) == 0
    a, b, c = f(3, 16, 64, 12, 48), f(3, 16, 64, 0, 48), f(4, 16, 128, 12, 48)
    assert 0 < b < a < c and a >= 3 * (16 * 64 * 4 + 12 * 48 * 8 + 16 * 4 + 12 * 4)
    assert f(65535, 512, 1 << 20, 256, 1 << 20) > 1 << 45                                          # no 32-bit overflow


# ---- the host helpers ----------------------------------------------------------------------------------------------------------------------
def test_rle_string_round_trip():
    from detectorch_amd.utils import result_utils as ru
    rs = np.random.RandomState(0)
    lists = [[], [0], [35], [0, 35], [1] * 35, [0, 1, 0, 1, 33], [900000000 - 7, 7], [5, 1 << 31, 3, 0, 0, 9, 1, 2]]
    lists += [rs.randint(0, 1 << rs.randint(1, 31), rs.randint(1, 200)).tolist() for _ in range(50)]
    for cnts in lists:
        s = ru._rle_counts_to_string(cnts)
        assert ru.rle_string_to_counts(s) == cnts and ru.rle_string_to_counts(s.encode("ascii")) == cnts
    m = rs.rand(37, 53) < 0.5
    assert ru.rle_string_to_counts(ru.rle_encode(m)["counts"]) == sc.runs_of(m)


def test_pack_gt_masks_takes_every_form():
    from detectorch_amd.utils import evaluator as E
    from detectorch_amd.utils import result_utils as ru
    rs = np.random.RandomState(1)
    a, b = rs.rand(7, 5) < 0.5, rs.rand(5, 7) < 0.5
    a[0, 0], b[0, 0] = True, False
    forms = lambda m: [m, m.astype(np.uint8), dict(size=list(m.shape), counts=sc.runs_of(m)), ru.rle_encode(m),
                       dict(size=list(m.shape), counts=ru.rle_encode(m)["counts"].encode("ascii")), None]
    out = E.pack_gt_masks([forms(a), forms(b)[:3]], [(7, 5), (5, 7)], "cpu")
    runs, n = out["gt_runs"].numpy().view(np.uint32), out["gt_n_runs"].numpy()
    assert runs.shape[:2] == (2, 6) and out["gt_runs"].dtype.is_signed and n[0, 5] == 0 and n[1, 3:].tolist() == [0, 0, 0]
    for i, m in enumerate((a, b)):
        want = sc.runs_of(m)
        for j in range(5 if i == 0 else 3):
            assert n[i, j] == len(want) and runs[i, j, :len(want)].tolist() == want
            assert np.array_equal(sr.decode(runs[i, j], n[i, j], 35).reshape(m.shape[::-1]).T, m)
    assert ru.rle_counts(a) == sc.runs_of(a) and ru.rle_counts(a)[0] == 0
    out = E.pack_gt_masks([[a]], [(7, 5)], "cpu", G=4, runs_stride=50)
    assert tuple(out["gt_runs"].shape) == (1, 4, 50)
    with pytest.raises(ValueError, match="do not fit"):
        E.pack_gt_masks([[a, a]], [(7, 5)], "cpu", G=1)
    with pytest.raises(ValueError, match="bitmap of shape"):
        E.pack_gt_masks([[b]], [(7, 5)], "cpu")
    with pytest.raises(ValueError, match="RLE of size"):
        E.pack_gt_masks([[ru.rle_encode(b)]], [(7, 5)], "cpu")
    with pytest.raises(ValueError, match="run lengths"):
        E.pack_gt_masks([[dict(size=[7, 5], counts=[3, -1])]], [(7, 5)], "cpu")
