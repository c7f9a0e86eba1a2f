"""Mask post-processing without a GPU (tests/README_mask_post.md):
  * libdetectorch_mpost_hip.so exports exactly what include/detectorch_mpost_hip.h declares and hip_mpost.SIGNATURES binds it,
    parameter names and kinds in order; the eleven other libraries export no dtc_mpost_ name and what they did; the header compiles
    as pedantic C99 and C++11; the constants of header and binding agree; the workspace sizes; the return codes on bad arguments
    (validation precedes every HIP call, so nothing is launched and the bogus pointers are never used);
  * the numpy restatement (tests/mask_post_ref.py) against answers derived by hand, its AVG loop against np.average on every case,
    its bitmap-free forms against its bitmaps, and on filled rectangles against coco_eval_ref's box IoU;
  * every case (tests/mask_post_cases.py) holds the condition it was built for, and tells every mutant of the README's table from
    the contract;
  * the Python layer: CPU tensors are refused, the trivial answers need no GPU."""
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
import mask_post_cases as mc
import mask_post_ref as mr
import segm_eval_ref as sr

sys.path.insert(0, GOLDEN)                                    # make_native_host_codes.exports

NAMES = ["dtc_mpost_boxes", "dtc_mpost_nms", "dtc_mpost_overlaps", "dtc_mpost_overlaps_workspace_bytes", "dtc_mpost_target_arch",
         "dtc_mpost_vote", "dtc_mpost_vote_workspace_bytes"]
_REF = {}


def reference(name):
    """a vote case, its overlaps and its AVG / UNION answers, computed once"""
    if name not in _REF:
        case = mc.VOTE_CASES[name]()
        ovr = mc.real_ovr(case)
        _REF[name] = (case, ovr, {m: mr.vote(case, ovr, m) for m in ("AVG", "UNION")})
    return _REF[name]


# ---- the library: exports, binding, header, constants -----------------------------------------------------------------------------------
def prototypes(header):
    """test_binding_signatures_host.prototypes with the double kind this header adds"""
    import test_binding_signatures_host as tb
    scalars = dict(tb.SCALARS, double="d")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    out = {}
    for ret, entry, params in re.findall(r"^([\w \*]+?)\b(dtc_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        kinds = []
        for p in [q.strip() for q in params.split(",") if q.strip() != "void"]:
            ctype, name = re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()
            ctype = ctype.strip()
            kinds.append((name, "p" if ctype.endswith("*") or ctype == "dtc_stream_t" else scalars[ctype.replace("const", "").strip()]))
        out[entry] = (tb.RETURNS.get(ret.strip()) or "status", kinds)
    return out


def test_header_symbols_are_exported_and_bound():
    from make_native_host_codes import exports
    from detectorch_amd import hip, hip_mpost
    lib = hip_mpost.lib()
    protos = prototypes("detectorch_mpost_hip.h")
    assert sorted(protos) == NAMES and exports(hip_mpost.LIB_PATH) == NAMES and sorted(hip_mpost.SIGNATURES) == NAMES
    assert list(protos) == list(hip_mpost.SIGNATURES)                                            # the header's order
    for entry, (ret, params) in protos.items():
        row = hip_mpost.SIGNATURES[entry]
        assert row[0] == ret and [n for n, _ in row[1]] == [n for n, _ in params], entry
        assert [k for _, k in row[1]] == [k for _, k in params], entry
        fn = getattr(lib, entry)
        assert list(fn.argtypes) == [hip._KINDS[k] for _, k in row[1]] and fn.restype == hip._RETURNS[row[0]], entry
    assert hip._KINDS["d"] is C.c_double
    assert lib.dtc_mpost_target_arch() == b"gfx950"
    assert [k for n, k in hip_mpost.SIGNATURES["dtc_mpost_nms"][1] if n == "thresh"] == ["d"]
    assert [k for n, k in hip_mpost.SIGNATURES["dtc_mpost_vote"][1] if n.endswith("_thresh")] == ["d", "d"]


def test_the_other_libraries_export_what_they_did():
    """the first library's 42 exports are the recorded ones; every other side library exports what its own binding table names, and
    none of the eleven a dtc_mpost_ name"""
    import json
    from make_native_host_codes import exports
    from detectorch_amd import (build, hip, hip_eval, hip_flip, hip_grad, hip_loss, hip_mask, hip_optim, hip_poly, hip_rpn, hip_segm,
                                hip_train)
    build.build()
    recorded = json.load(open(os.path.join(GOLDEN, "native_host_codes.json")))["exports"]
    assert exports(hip.LIB_PATH) == recorded and len(recorded) == 42
    sides = (hip_train, hip_loss, hip_grad, hip_optim, hip_rpn, hip_mask, hip_eval, hip_segm, hip_poly, hip_flip)
    for mod in sides:
        mod.lib()
        assert exports(mod.LIB_PATH) == sorted(mod.SIGNATURES), mod.__name__
    assert len(sides) + 1 == 11
    for mod in (hip,) + sides:
        assert not [n for n in exports(mod.LIB_PATH) if n.startswith("dtc_mpost_")], mod.__name__


@pytest.mark.parametrize("compiler,flags", [("gcc", ["-std=c99"]), ("g++", ["-std=c++11"])])
def test_header_compiles_as_pedantic_c99_and_cxx11(tmp_path, compiler, flags):
    cc = shutil.which(compiler) or shutil.which({"gcc": "cc", "g++": "c++"}[compiler])
    assert cc, compiler + " not found"
    src = tmp_path / ("use_header" + {"gcc": ".c", "g++": ".cpp"}[compiler])
    src.write_text('#include "detectorch_mpost_hip.h"\nint use(void) { return DTC_MPOST_MAX_RUNS / DTC_MPOST_MAX_ROWS + DTC_MPOST_NMS_IOMA; }\n')
    subprocess.check_call([cc] + flags + ["-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                                          str(tmp_path / "use_header.o")])


def test_constants_are_those_of_the_header():
    from detectorch_amd import hip_mpost, hip_segm
    header = open(os.path.join(ROOT, "include", "detectorch_mpost_hip.h")).read()
    define = lambda name: eval(re.search(r"#define DTC_MPOST_%s (\(?[\d <]+\)?)" % name, header).group(1))
    assert (define("MAX_BATCH"), define("MAX_ROWS"), define("MAX_RUNS"), define("MAX_PIXELS")) == (
        hip_mpost.MAX_BATCH, hip_mpost.MAX_ROWS, hip_mpost.MAX_RUNS, hip_mpost.MAX_PIXELS) == (65535, 512, 1 << 20, 1 << 30)
    assert (hip_mpost.MAX_RUNS, hip_mpost.MAX_PIXELS) == (hip_segm.MAX_RUNS, hip_segm.MAX_PIXELS)
    assert {k: define("NMS_" + k) for k in hip_mpost.NMS_MODES} == hip_mpost.NMS_MODES == dict(IOU=0, IOMA=1, CONTAINMENT=2)
    assert {k: define("VOTE_" + k) for k in hip_mpost.VOTE_METHODS} == hip_mpost.VOTE_METHODS == dict(AVG=0, UNION=1)
    assert "wrong about their own" in header and "one deliberate choice" in header      # the two statements the header owes


def test_workspace_bytes():
    from detectorch_amd import hip_mpost
    f, g = hip_mpost.lib().dtc_mpost_overlaps_workspace_bytes, hip_mpost.lib().dtc_mpost_vote_workspace_bytes
    ok = (3, 12, 500, 7, 300)
    for at, bad in ((0, 0), (0, 65536), (1, 0), (1, 513), (2, 0), (2, (1 << 20) + 1), (3, 0), (3, 513), (4, 0), (4, (1 << 20) + 1)):
        assert f(*[bad if i == at else v for i, v in enumerate(ok)]) == 0, (at, bad)
    base = f(*ok)
    assert base >= 3 * (12 * 500 * 4 + 7 * 300 * 8) and base % 16 == 0
    for at in range(5):                                         # monotone in every argument
        assert f(*[v + 1 if i == at else v for i, v in enumerate(ok)]) > base, at
    assert f(65535, 512, 1 << 20, 512, 1 << 20) >= 65535 * 512 * (1 << 20) * 12     # no 32-bit overflow
    okv = (3, 12, 500)
    for at, bad in ((0, 0), (0, 65536), (1, 0), (1, 513), (2, 0), (2, (1 << 20) + 1)):
        assert g(*[bad if i == at else v for i, v in enumerate(okv)]) == 0, (at, bad)
    assert g(*okv) >= 3 * 12 * 500 * 4 and g(*okv) % 16 == 0 and g(*okv) < 3 * 12 * 500 * 4 + 3 * 12 * 16 + 64      # runs, not pixels
    for at in range(3):
        assert g(*[v + 1 if i == at else v for i, v in enumerate(okv)]) > g(*okv), at
    assert g(65535, 512, 1 << 20) >= 65535 * 512 * (1 << 20) * 4


BOGUS = 256                                                    # a bogus, non-NULL, 16-byte aligned device pointer
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -3, -4


def _caller(entry, apart=()):
    """-> call(**overrides) by the binding's table: every pointer bogus but non-NULL unless overridden (None: NULL) -- those of
    `apart` 256 MiB from each other --, the scalars from the overrides over DEFAULTS"""
    def call(**kw):
        from detectorch_amd import hip_mpost
        args = []
        for name, kind in hip_mpost.SIGNATURES[entry][1][:-1]:
            if kind == "p":
                v = kw.pop(name, (apart.index(name) + 1) << 28 if name in apart else BOGUS)
                args.append(None if v is None else C.c_void_p(v))
            else:
                args.append(kw.pop(name, DEFAULTS[name]))
        assert not kw, kw
        return getattr(hip_mpost.lib(), entry)(*args, None)
    return call


DEFAULTS = dict(batch=3, rows_stride=12, runs_stride=500, a_rows=12, a_runs_stride=500, b_rows=7, b_runs_stride=300, crowd=0,
                workspace_bytes=1 << 30, thresh=0.5, mode=0, top_rows=12, top_runs_stride=500, all_rows=7, all_runs_stride=300,
                dets_stride=6, iou_thresh=0.5, binarize_thresh=0.5, method=0, out_stride=700)


def _check(call, codes):
    assert {k: call(**kw) for k, (kw, _) in codes.items()} == {k: v[1] for k, v in codes.items()}


def test_return_codes_of_boxes():
    _check(_caller("dtc_mpost_boxes"), {
        "batch 0": (dict(batch=0), EINVAL), "R 0": (dict(rows_stride=0), EINVAL), "stride 0": (dict(runs_stride=0), EINVAL),
        "R 0 + batch 65536": (dict(rows_stride=0, batch=65536), EINVAL),
        "batch 65536": (dict(batch=65536), EUNSUPPORTED), "R 513": (dict(rows_stride=513), EUNSUPPORTED),
        "stride 2^20 + 1": (dict(runs_stride=(1 << 20) + 1), EUNSUPPORTED), "R 513 + runs NULL": (dict(rows_stride=513, runs=None), EUNSUPPORTED),
        **{k + " NULL": ({k: None}, EINVAL) for k in ("runs", "n_runs", "im_size", "boxes", "area", "nonempty")},
        "boxes misaligned": (dict(boxes=BOGUS + 4), EINVAL),
    })


def test_return_codes_of_overlaps():
    from detectorch_amd import hip_mpost
    need = hip_mpost.lib().dtc_mpost_overlaps_workspace_bytes(3, 12, 500, 7, 300)
    _check(_caller("dtc_mpost_overlaps"), {
        "batch 0": (dict(batch=0), EINVAL), "Ra 0": (dict(a_rows=0), EINVAL), "Rb 0": (dict(b_rows=0), EINVAL),
        "a stride 0": (dict(a_runs_stride=0), EINVAL), "b stride -1": (dict(b_runs_stride=-1), EINVAL),
        "Ra 513 + Rb 0": (dict(a_rows=513, b_rows=0), EINVAL),
        "batch 65536": (dict(batch=65536), EUNSUPPORTED), "Ra 513": (dict(a_rows=513), EUNSUPPORTED), "Rb 513": (dict(b_rows=513), EUNSUPPORTED),
        "a stride 2^20 + 1": (dict(a_runs_stride=(1 << 20) + 1), EUNSUPPORTED), "b stride 2^20 + 1": (dict(b_runs_stride=(1 << 20) + 1), EUNSUPPORTED),
        "Rb 513 + ovr NULL": (dict(b_rows=513, ovr=None), EUNSUPPORTED),
        **{k + " NULL": ({k: None}, EINVAL) for k in ("a_runs", "a_n_runs", "a_count", "b_runs", "b_n_runs", "b_count", "im_size", "ovr",
                                                     "a_area", "b_area")},
        "workspace misaligned": (dict(workspace=BOGUS + 8), EINVAL),
        "workspace NULL": (dict(workspace=None), EWORKSPACE), "workspace 0 bytes": (dict(workspace_bytes=0), EWORKSPACE),
        "workspace one byte short": (dict(workspace_bytes=need - 1), EWORKSPACE), "ovr NULL + workspace short": (dict(ovr=None, workspace_bytes=0), EINVAL),
    })


def test_return_codes_of_nms():
    _check(_caller("dtc_mpost_nms"), {
        "batch 0": (dict(batch=0), EINVAL), "R 0": (dict(rows_stride=0), EINVAL), "mode -1": (dict(mode=-1), EINVAL), "mode 3": (dict(mode=3), EINVAL),
        "mode 3 + R 513": (dict(mode=3, rows_stride=513), EINVAL),
        "batch 65536": (dict(batch=65536), EUNSUPPORTED), "R 513": (dict(rows_stride=513), EUNSUPPORTED),
        "R 513 + dets NULL": (dict(rows_stride=513, dets=None), EUNSUPPORTED),
        **{k + " NULL": ({k: None}, EINVAL) for k in ("dets", "count", "ovr", "keep", "keep_count")},
    })


def test_return_codes_of_vote():
    from detectorch_amd import hip_mpost
    need = hip_mpost.lib().dtc_mpost_vote_workspace_bytes(3, 7, 300)
    pointers = [n for n, k in hip_mpost.SIGNATURES["dtc_mpost_vote"][1][:-1] if k == "p" and n != "workspace"]
    assert len(pointers) == 12
    codes = {
        "batch 0": (dict(batch=0), EINVAL), "T 0": (dict(top_rows=0), EINVAL), "A 0": (dict(all_rows=0), EINVAL),
        "top stride 0": (dict(top_runs_stride=0), EINVAL), "all stride 0": (dict(all_runs_stride=0), EINVAL), "out_stride 0": (dict(out_stride=0), EINVAL),
        "dets_stride 4": (dict(dets_stride=4), EINVAL), "method 2": (dict(method=2), EINVAL), "method -1": (dict(method=-1), EINVAL),
        "method 2 + T 513": (dict(method=2, top_rows=513), EINVAL), "out_stride 0 + A 513": (dict(out_stride=0, all_rows=513), EINVAL),
        "batch 65536": (dict(batch=65536), EUNSUPPORTED), "T 513": (dict(top_rows=513), EUNSUPPORTED), "A 513": (dict(all_rows=513), EUNSUPPORTED),
        "top stride 2^20 + 1": (dict(top_runs_stride=(1 << 20) + 1), EUNSUPPORTED), "all stride 2^20 + 1": (dict(all_runs_stride=(1 << 20) + 1), EUNSUPPORTED),
        "out_stride 2^20 + 1": (dict(out_stride=(1 << 20) + 1), EUNSUPPORTED), "T 513 + need NULL": (dict(top_rows=513, need=None), EUNSUPPORTED),
        **{k + " NULL": ({k: None}, EINVAL) for k in pointers},
        "workspace misaligned": (dict(workspace=BOGUS + 8), EINVAL),
        "out_runs is top_runs": (dict(out_runs=1 << 28), EINVAL), "out_runs is all_runs": (dict(out_runs=2 << 28), EINVAL),
        "out_runs inside top_runs": (dict(out_runs=(1 << 28) + 3 * 12 * 500 * 4 - 4), EINVAL),
        "all_runs inside out_runs": (dict(all_runs=(3 << 28) + 3 * 12 * 700 * 4 - 4), EINVAL),
        "out_runs right behind top_runs": (dict(out_runs=(1 << 28) + 3 * 12 * 500 * 4, workspace_bytes=0), EWORKSPACE),
        "workspace NULL": (dict(workspace=None), EWORKSPACE), "workspace 0 bytes": (dict(workspace_bytes=0), EWORKSPACE),
        "workspace one byte short": (dict(workspace_bytes=need - 1), EWORKSPACE),
    }
    _check(_caller("dtc_mpost_vote", apart=("top_runs", "all_runs", "out_runs")), codes)
    assert len(codes) >= 38


def test_refusals_write_nothing():
    """a refused call has written nothing: every refusal returns from the host body in front of the first launch, so outputs that
    are host memory filled with 0xFF -- which a kernel could not even reach -- stay 0xFF"""
    from detectorch_amd import hip_mpost
    bufs = {k: np.full(64, 0xFF, np.uint8) for k in ("boxes", "area", "nonempty", "ovr", "a_area", "b_area", "keep", "keep_count", "out_runs",
                                                     "out_n_runs", "need")}
    ptr = {k: v.ctypes.data for k, v in bufs.items()}
    calls = [("dtc_mpost_boxes", ("boxes", "area", "nonempty"), dict(rows_stride=513), EUNSUPPORTED),
             ("dtc_mpost_boxes", ("boxes", "area", "nonempty"), dict(runs=None), EINVAL),
             ("dtc_mpost_overlaps", ("ovr", "a_area", "b_area"), dict(workspace_bytes=8), EWORKSPACE),
             ("dtc_mpost_overlaps", ("ovr", "a_area", "b_area"), dict(b_rows=513), EUNSUPPORTED),
             ("dtc_mpost_nms", ("keep", "keep_count"), dict(mode=7), EINVAL),
             ("dtc_mpost_vote", ("out_runs", "out_n_runs", "need"), dict(workspace_bytes=8), EWORKSPACE),
             ("dtc_mpost_vote", ("out_runs", "out_n_runs", "need"), dict(method=5), EINVAL)]
    for entry, outs, kw, code in calls:
        assert _caller(entry)(**dict({k: ptr[k] for k in outs}, **kw)) == code, (entry, kw)
    assert all((v == 0xFF).all() for v in bufs.values())


# ---- the restatement against answers derived by hand --------------------------------------------------------------------------------------
def test_ref_known_answers():
    # encode / bitmap: the 3 x 4 mask with pixels (2, 1) and (0, 2): positions 5 and 6
    m = mr.bitmap(np.array([5, 2, 5], np.uint32), 3, 3, 4)
    assert m.nonzero()[0].tolist() == [0, 2] and m.nonzero()[1].tolist() == [2, 1] and mr.encode(m) == [5, 2, 5]
    assert mr.encode(np.ones((2, 3), bool)) == [0, 6] and mr.encode(np.zeros((2, 3), bool)) == [6]
    assert mr.encode(np.array([[1, 0], [0, 1]], bool)) == [0, 1, 2, 1]
    # boxes
    runs, n_runs, counts, im_size, names = mc.boxes()
    got = mr.masks_to_boxes(runs, n_runs, counts, im_size)
    at = names.index
    for n, (h, w) in enumerate(((5, 4), (3, 6))):
        want = {"corner_00": (0, 0, 0, 0, 1), "corner_h0": (0, h - 1, 0, h - 1, 1), "corner_0w": (w - 1, 0, w - 1, 0, 1),
                "corner_hw": (w - 1, h - 1, w - 1, h - 1, 1), "full_column": (1, 0, 1, h - 1, h), "wraps": (1, 0, 2, h - 1, 2),
                "full": (0, 0, w - 1, h - 1, h * w), "empty": (0, 0, 0, 0, 0), "no_runs": (0, 0, 0, 0, 0), "count_negative": (0, 0, 0, 0, 0),
                "zero_runs_in_front": (1, 1, 1, 1, 1), "two_columns_inside": (1, 1, 2, 2, 2), "short": (0, 1, 0, 2, 2),
                "past": ((h * w - 2) // h, (h * w - 2) % h, w - 1, h - 1, 2)}
        for k, v in want.items():
            assert tuple(got["boxes"][n, at(k)]) == v[:4] and got["area"][n, at(k)] == v[4] and got["nonempty"][n, at(k)] == int(v[4] > 0), (n, k)
            assert mr.interval_box(runs[n, at(k)], n_runs[n, at(k)], h, w) == (v[:4], v[4]), (n, k)
        assert (got["boxes"][n, 14:] == -1).all() and (got["area"][n, 14:] == -1).all()
    assert tuple(got["boxes"][0, at("corner_00")]) == tuple(got["boxes"][0, at("empty")]) and got["nonempty"][0, at("corner_00")] == 1
    # overlaps: with crowd the divisor is the area of the FIRST argument's mask
    a, b = (np.array([[[0, 4, 8]]], np.uint32), np.array([[3]], np.int32)), (np.array([[[2, 6, 4]]], np.uint32), np.array([[3]], np.int32))
    one, size = np.array([1], np.int32), np.array([[3, 4]], np.float32)
    assert mr.overlaps(*a, one, *b, one, size, False)["ovr"][0, 0, 0] == 2 / 8 and mr.overlaps(*a, one, *b, one, size, True)["ovr"][0, 0, 0] == 2 / 4
    assert mr.overlaps(*b, one, *a, one, size, True)["ovr"][0, 0, 0] == 2 / 6
    # the walk: three rows, thresh 0.5
    iou = np.array([[1, .6, .5], [.6, 1, .2], [.5, .2, 1]])
    assert mr.nms_walk([.9, .8, .7], [1, 1, 1], iou, 0.5, 'IOU') == [0, 2] and mr.nms_walk([.9, .8, .7], [1, 2, 1], iou, 0.5, 'IOU') == [0, 1, 2]
    assert mr.nms_walk([.7, .8, .9], [1, 1, 1], iou, 0.5, 'IOU') == [2, 1] and mr.nms_walk([.9, .8, .7], [1, 1, 1], iou, 0.5, 'IOU', 'lt') == [0]
    assert mr.nms_walk([.5, np.nan, .5, .9], [1] * 4, np.zeros((4, 4)), 0.5, 'IOU') == [3, 0, 2, 1]       # ties by row, NaN last
    assert mr.nms_walk([.5, np.nan, .5, .9], [1] * 4, np.zeros((4, 4)), 0.5, 'IOU', 'reverse_ties') == [3, 2, 0, 1]
    assert mr.nms_walk([.9, .8], [1, 1], [[1, np.nan], [0, 1]], 0.5, 'IOU') == [0]                        # a NaN value suppresses
    asym = np.array([[1, .2], [.8, 1]])
    assert mr.nms_walk([.9, .8], [1, 1], asym, 0.5, 'CONTAINMENT') == [0, 1] and mr.nms_walk([.9, .8], [1, 1], asym, 0.5, 'IOMA') == [0]
    with pytest.raises(NotImplementedError):
        mr.nms_walk([.9], [1], [[1]], 0.5, 'IOA')
    # the support: on an 8-wide image the x-range 2 .. -5 gives columns 2 and 3; truncation, not floor
    wp = mr.weight_planes(np.array([[2, 0, -5, 0, 0.5], [-0.5, -0.9, 2.7, 0.9, 0.25], [0, 0, -0.5, -0.3, 0.75], [3, 0, 1, 0, 0.5],
                                    [0, 0, 7, 0, -1.0]], np.float32), 1, 8)
    assert wp[0, 0].tolist() == [1e-5, 1e-5, .5, .5, 1e-5, 1e-5, 1e-5, 1e-5] and wp[1, 0].tolist() == [.25] * 3 + [1e-5] * 5
    assert wp[2, 0].tolist() == [.75] + [1e-5] * 7 and (wp[3] == 1e-5).all() and (wp[4] == 1e-5).all()
    # a vote by hand: two voters of weight 0.5 and 0.25 everywhere: a pixel only the first has is 2/3 > 0.5, only the second 1/3
    lists = [(np.array([0, 2, 2], np.uint32), 3), (np.array([1, 2, 1], np.uint32), 3)]
    dets = np.array([[0, 0, 3, 0, 0.5], [0, 0, 3, 0, 0.25]], np.float32)
    assert mr.vote_image(lists[:1], lists, dets, [[1.0, 1 / 3]], 1, 4, 0.3, 0.5, 'AVG') == [[0, 2, 2]]
    assert mr.vote_image(lists[:1], lists, dets, [[1.0, 1 / 3]], 1, 4, 0.3, 0.3, 'AVG') == [[0, 3, 1]]
    assert mr.vote_image(lists[:1], lists, dets, [[1.0, 1 / 3]], 1, 4, 0.3, 0.5, 'UNION') == [[0, 3, 1]]
    assert mr.vote_image(lists[:1], lists, dets, [[1.0, 1 / 3]], 1, 4, 0.5, 0.5, 'AVG') == [None]       # one voter: copied
    with pytest.raises(NotImplementedError):
        mr.vote_image(lists[:1], lists, dets, [[1.0, 1.0]], 1, 4, 0.5, 0.5, 'MAX')


@pytest.mark.parametrize("name", ["tiny", "order", "chunks"])
def test_the_avg_loop_is_np_average(name):
    case, ovr, want = reference(name)
    got = mr.vote(case, ovr, 'AVG', average=lambda masks, ws, order=None: mr.avg_numpy(masks, ws))
    assert got["lists"] == want["AVG"]["lists"] and np.array_equal(got["need"], want["AVG"]["need"])


def test_the_avg_loop_is_np_average_on_the_threshold_case():
    case, ovr = mc.threshold_vote()
    for bt in (0.5, np.nextafter(0.5, 0)):
        c = dict(case, binarize_thresh=bt)
        assert mr.vote(c, ovr, 'AVG')["lists"] == mr.vote(c, ovr, 'AVG', average=lambda m, ws, order=None: mr.avg_numpy(m, ws))["lists"]


# ---- every case holds its condition ------------------------------------------------------------------------------------------------------------
def voters(case, ovr, n, t):
    na = mr.clamp(case["all_count"][n], case["all_n_runs"].shape[1])
    with np.errstate(invalid='ignore'):
        return np.flatnonzero(ovr[n, t, :na] >= case["iou_thresh"])


def differs(a, b):
    return a["lists"] != b["lists"] or not np.array_equal(a["need"], b["need"])


def test_tiny_holds_its_conditions():
    case, ovr, want = reference("tiny")
    assert case["top_count"].tolist() == [15, 15] and case["all_count"].tolist() == [18, 18] and case["top_runs"].shape[1:] == (16, 36)
    for n in range(2):
        nv = [len(voters(case, ovr, n, t)) for t in range(15)]
        assert sum(v >= 2 for v in nv) >= 6 and 1 in nv and nv[14] == 0, nv
        avg, uni = want["AVG"], want["UNION"]
        assert avg["copied"][n, :15].sum() >= 3 and (avg["out_n_runs"][n, :15] == -1).sum() == 1            # count_negative
        assert (avg["need"][n, 15] == -1) and avg["lists"][n] != uni["lists"][n]
        assert sum(1 for t in range(15) if not avg["copied"][n, t] and avg["out_n_runs"][n, t] >= 0) >= 6
    for variant in ("reverse", "gt", "floor", "clamp_neg", "no_floor"):
        if variant not in ("reverse", "gt"):                    # the supports and the floor decide pixels here
            assert differs(mr.vote(case, ovr, 'AVG', variant), want["AVG"]), variant


def test_threshold_vote_holds_its_conditions():
    case, ovr = mc.threshold_vote()
    at = mr.vote(case, ovr, 'AVG')
    assert [len(voters(case, ovr, 0, t)) for t in range(4)] == [3, 2, 1, 0] and at["copied"][0].tolist() == [False, False, True, True, False]
    # voters 0, 1, 2: pixel 3 has all (1.0), 5 two (0.75); 2, 6, 7 sit at exactly 0.5: off
    assert at["lists"][0][0] == [3, 1, 1, 1, 10]
    below = mr.vote(dict(case, binarize_thresh=np.nextafter(0.5, 0)), ovr, 'AVG')
    assert below["lists"][0][0] == [2, 2, 1, 3, 8]              # ... and on when the threshold is one ulp lower: 3 pixels at equality
    assert at["lists"][0][1] == [8, 4, 4]                       # voters 0 (0.25) and 3 (1.0): 0.2 and 0.8: only voter 3's pixels pass
    assert differs(mr.vote(case, ovr, 'AVG', 'gt'), at)         # at iou_thresh: a voter


def test_threshold_nms_holds_its_conditions():
    c = mc.threshold_nms()
    t, crowd, iou = c["thresh"], c["crowd"], c["iou"]
    live = crowd[0, :10, :10]
    for v in (np.nextafter(t, 0), t, np.nextafter(t, 1)):
        assert (live == v).any()
    assert np.isnan(live).any() and not np.array_equal(live, live.T)
    keep = {m: mr.nms(c["dets"], c["count"], crowd, t, m)["keep"][0].tolist() for m in ("IOU", "IOMA", "CONTAINMENT")}
    assert keep["IOU"] == keep["CONTAINMENT"]                   # the same walk on the same matrix: the modes differ in how it is made
    walk_iou = mr.nms(c["dets"], c["count"], iou, t, "IOU")["keep"][0].tolist()
    sets = [frozenset(k) for k in (walk_iou, keep["IOMA"], keep["CONTAINMENT"])]
    assert len(set(sets)) == 3, (walk_iou, keep)                # the IoU walk, IOMA and CONTAINMENT keep three different sets
    for variant, mode in (("lt", "IOU"), ("lt", "IOMA"), ("swap", "CONTAINMENT"), ("reverse_ties", "IOU")):
        assert mr.nms(c["dets"], c["count"], crowd, t, mode, variant)["keep"][0].tolist() != keep[mode], variant
    k = keep["CONTAINMENT"]
    assert k[-1] == -1 and 4 not in k[:2] and set(k) - {-1} <= set(range(10))       # rows past the count are never kept


def test_order_holds_its_conditions():
    on, bt = mc.order_search()
    case, ovr, want = reference("order")
    assert case["binarize_thresh"] == bt and len(voters(case, ovr, 0, 0)) == 5 and mc.order_weights()[0] == 1e-5
    rev = mr.vote(case, ovr, 'AVG', 'reverse')
    p = sum(1 << k for k in on)                                  # the pixel that has exactly the voters of `on`
    h, w = 4, 8
    a = mr.bitmap(np.array(want["AVG"]["lists"][0][0], np.uint32), 99, h, w).reshape(-1, order='F')
    b = mr.bitmap(np.array(rev["lists"][0][0], np.uint32), 99, h, w).reshape(-1, order='F')
    assert a[p] != b[p] and differs(rev, want["AVG"])            # summing in the other order flips it


def test_chunks_holds_its_conditions():
    case, ovr, want = reference("chunks")
    avg = want["AVG"]
    n_in = case["all_n_runs"][0, :180]
    assert {64, 65, 128, 129} <= set(n_in.tolist()) and case["top_count"][0] == 180 and case["top_runs"].shape[1] == 200
    assert len(voters(case, ovr, 0, 0)) >= 130
    need, out_n = avg["need"][0, :180], avg["out_n_runs"][0, :180]
    assert need.max() > case["out_stride"] and (out_n[need > case["out_stride"]] == -1).all() and (need == case["out_stride"]).any()
    assert (out_n[need == case["out_stride"]] == case["out_stride"]).all()
    longer = [t for t in range(180) if not avg["copied"][0, t] and need[t] > max(n_in[voters(case, ovr, 0, t)].max(), case["top_n_runs"][0, t])]
    assert longer, "no voted list is longer than every list that went into it"
    ends = [set(np.cumsum(case["all_runs"][0, k, :n_in[k]].astype(np.int64)).tolist()) for k in range(130, 150)]
    assert all({256, 512} <= e for e in ends)                    # run ends on the chunk borders
    assert (~avg["copied"][0, :180]).sum() >= 150 and differs(want["UNION"], avg)


def test_large_holds_its_conditions():
    case, ovr, want = reference("large")
    assert sum(len(voters(case, ovr, 0, t)) >= 2 for t in range(6)) >= 4
    ends = np.cumsum(case["top_runs"][0, 0, :case["top_n_runs"][0, 0]].astype(np.int64))
    assert ends[0] > 1 << 16 and (~want["AVG"]["copied"][0, :6]).sum() >= 4 and differs(want["AVG"], want["UNION"])


def test_huge_answers_come_from_intervals():
    c = mc.huge()
    got = mr.overlaps(c["a_runs"], c["a_n_runs"], c["a_count"], c["b_runs"], c["b_n_runs"], c["b_count"], c["im_size"], False,
                      counts=sr.interval_counts)
    hw = 30000 * 30000
    assert got["a_area"][0].tolist() == [hw - 1000, hw - 12345, 0] and got["b_area"][0].tolist() == [7, 3, 30000, 0]
    assert got["ovr"][0, 0, 0] == 7 / (hw - 1000) and got["ovr"][0, 1, 2] == (30000 - 12345) / (hw - 12345 + 12345)
    assert mr.interval_box(c["a_runs"][0, 0], 2, 30000, 30000) == ((0, 0, 29999, 29999), hw - 1000)
    assert mr.interval_box(c["b_runs"][0, 0], 2, 30000, 30000) == ((29999, 29993, 29999, 29999), 7)
    assert mr.interval_box(c["b_runs"][0, 1], 3, 30000, 30000) == ((29999, 5, 29999, 7), 3)


def test_interval_forms_equal_the_bitmaps():
    for name in ("tiny", "order"):
        case, ovr, _ = reference(name)
        args = (case["top_runs"], case["top_n_runs"], case["top_count"], case["all_runs"], case["all_n_runs"], case["all_count"], case["im_size"])
        for crowd in (False, True):
            a, b = mr.overlaps(*args, crowd), mr.overlaps(*args, crowd, counts=sr.interval_counts)
            assert all(np.array_equal(a[k], b[k]) for k in a)
        boxes = mr.masks_to_boxes(case["all_runs"], case["all_n_runs"], case["all_count"], case["im_size"])
        for n in range(len(case["im_size"])):
            h, w = mr.sides(case["im_size"][n])
            for k in range(case["all_count"][n]):
                assert mr.interval_box(case["all_runs"][n, k], case["all_n_runs"][n, k], h, w) == (tuple(boxes["boxes"][n, k]), boxes["area"][n, k])


def test_rects_bridge_to_the_box_protocol():
    """filled integer rectangles: the mask box is the rectangle, the mask overlap the +1 box IoU bit for bit; no IoU within 1e-6 of the NMS
    threshold (the box NMS compares in float32), and the walk suppresses at least a third"""
    c = mc.rects()
    R = len(c["boxes"])
    got = mr.masks_to_boxes(c["runs"], c["n_runs"], c["count"], c["im_size"])
    assert np.array_equal(got["boxes"][0, :R], c["boxes"].astype(np.int32)) and got["nonempty"][0, :R].all()
    for crowd in (False, True):
        ovr = mr.overlaps(c["runs"], c["n_runs"], c["count"], c["runs"], c["n_runs"], c["count"], c["im_size"], crowd)["ovr"][0]
        want = np.array([[cr.bb_iou(cr.xywh(c["boxes"][i]), cr.xywh(c["boxes"][j]), crowd) for j in range(R)] for i in range(R)])
        assert ovr[:R, :R].tobytes() == want.tobytes() and (ovr[R:] == 0).all() and (ovr[:, R:] == 0).all()
    iou = mr.overlaps(c["runs"], c["n_runs"], c["count"], c["runs"], c["n_runs"], c["count"], c["im_size"], False)["ovr"]
    assert np.abs(iou[0] - c["thresh"]).min() > 1e-6 and len(set(c["scores"].tolist())) == R
    dets = np.zeros((1, R + 2, 6), np.float32)
    dets[0, :R, 4], dets[0, :, 5] = c["scores"], 1
    kept = mr.nms(dets, c["count"], iou, c["thresh"], "IOU")["keep_count"][0]
    assert kept <= R - R // 3 and kept >= 3


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_the_cpu_and_answer_the_trivial():
    import torch
    from detectorch_amd import hip_mpost
    from detectorch_amd.utils import segms
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    f32, f64 = torch.float32, torch.float64
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_mpost.mask_boxes(z(1, 2, 4), z(1, 2), z(1, 2, dt=f32))
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_mpost.mask_overlaps(z(1, 2, 4), z(1, 2), z(1), z(1, 2, 4), z(1, 2), z(1), z(1, 2, dt=f32))
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_mpost.mask_nms(z(1, 2, 6, dt=f32), z(1), z(1, 2, 2, dt=f64), 0.5)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_mpost.mask_vote(z(1, 2, 4), z(1, 2), z(1), z(1, 3, 4), z(1, 3), z(1, 3, 5, dt=f32), z(1), z(1, 2, 3, dt=f64), z(1, 2, dt=f32), 0.5, 0.5)
    rle = dict(size=[3, 4], counts=[5, 2, 5])
    dets = np.array([[0, 0, 3, 2, 0.9]] * 2, np.float32)
    with pytest.raises(RuntimeError, match="GPU only"):
        segms.rle_mask_nms([rle, rle], dets, 0.5, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        segms.rle_mask_voting([rle], [rle, rle], dets, 0.5, 0.5, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        segms.rle_masks_to_boxes([rle], device="cpu")
    # what the reference answers without looking at a mask
    assert segms.rle_mask_nms([], dets[:0], 0.5) == [] and segms.rle_mask_nms([rle], dets[:1], 0.5) == [0]
    assert segms.rle_masks_to_boxes([]) == [] and segms.rle_mask_voting([], [rle], dets[:1], 0.5, 0.5) is None
    with pytest.raises(NotImplementedError, match="Mode IOA is unknown"):
        segms.rle_mask_nms([rle, rle], dets, 0.5, mode='IOA')
    with pytest.raises(NotImplementedError, match="Method MAX is unknown"):
        segms.rle_mask_voting([rle], [rle, rle], dets, 0.5, 0.5, method='MAX')
