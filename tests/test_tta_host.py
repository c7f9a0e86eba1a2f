"""Test-time augmentation without a GPU (tests/README_tta.md):
  * libdetectorch_aug_hip.so exports exactly what include/detectorch_aug_hip.h declares and hip_aug.SIGNATURES binds it, names and
    kinds in order; the twelve other libraries export no dtc_aug_ name; the header compiles as pedantic C99 and C++11; the constants
    of header and binding agree; the limit arithmetic and the return codes on bad arguments (validation precedes every HIP call,
    so nothing is launched and the bogus pointers are never used);
  * the numpy restatement (tests/tta_ref.py) against itself: one unflipped view under UNION, AVG or ID is the per-view decode, which
    is oracle/'s decode on the same rows; flipping twice is the identity on integer-valued boxes; the masks' rules on small hand
    cases; the LOGIT_AVG forms at y = 0 and y = 1;
  * every case (tests/tta_cases.py) holds the condition it was built for;
  * the Python layer: CPU tensors are refused; AugOptions validates, the view order is Detectron's, T * top_n above 4096 raises."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import det_options_ref as dr
import tta_cases as tc
import tta_ref as tr

sys.path.insert(0, GOLDEN)                                    # make_native_host_codes.exports

NAMES = ["dtc_aug_combine_masks", "dtc_aug_merge_boxes", "dtc_aug_target_arch"]
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
f32 = np.float32


# ---- the library: exports, binding, header, constants ------------------------------------------------------------------------------
def test_header_symbols_are_exported_and_bound():
    import test_binding_signatures_host as tb
    from make_native_host_codes import exports
    from detectorch_amd import hip, hip_aug
    lib = hip_aug.lib()
    protos = tb.prototypes("detectorch_aug_hip.h")
    assert sorted(protos) == NAMES and exports(hip_aug.LIB_PATH) == NAMES and sorted(hip_aug.SIGNATURES) == NAMES
    assert list(protos) == list(hip_aug.SIGNATURES)                                              # the header's order
    for entry, (ret, params) in protos.items():
        row = hip_aug.SIGNATURES[entry]
        assert row[0] == ret and [n for n, _ in row[1]] == [n for n, _ in params], entry
        assert [k if isinstance(k, str) else tb._struct_of(k) for _, k in row[1]] == [k for _, k in params], entry
        fn = getattr(lib, entry)
        want = [hip._KINDS[k] if isinstance(k, str) else C.POINTER(k) for _, k in row[1]]
        assert list(fn.argtypes) == want and fn.restype == hip._RETURNS[row[0]], entry
    assert lib.dtc_aug_target_arch() == b"gfx950"
    # struct dtc_aug_view: five pointers, the flag, padding to 48 bytes
    assert C.sizeof(hip_aug.AugView) == 48 and [n for n, _ in hip_aug.AugView._fields_] == re.findall(
        r"(\w+);", re.search(r"typedef struct dtc_aug_view \{(.*?)\}", open(os.path.join(ROOT, "include", "detectorch_aug_hip.h")).read(),
                             flags=re.S).group(1))


def test_the_other_libraries_export_no_aug_name():
    from make_native_host_codes import exports
    from detectorch_amd import (build, hip, hip_eval, hip_flip, hip_grad, hip_loss, hip_mask, hip_mpost, hip_optim, hip_poly, hip_rpn,
                                hip_segm, hip_train)
    build.build()
    sides = (hip_train, hip_loss, hip_grad, hip_optim, hip_rpn, hip_mask, hip_eval, hip_segm, hip_poly, hip_flip, hip_mpost)
    for mod in sides:
        mod.lib()
        assert exports(mod.LIB_PATH) == sorted(mod.SIGNATURES), mod.__name__
    assert len(sides) + 1 == 12
    for mod in (hip,) + sides:
        assert not [n for n in exports(mod.LIB_PATH) if n.startswith("dtc_aug_")], mod.__name__


@pytest.mark.parametrize("compiler,flags", [("gcc", ["-std=c99"]), ("g++", ["-std=c++11"])])
def test_header_compiles_as_pedantic_c99_and_cxx11(tmp_path, compiler, flags):
    cc = shutil.which(compiler) or shutil.which({"gcc": "cc", "g++": "c++"}[compiler])
    assert cc, compiler + " not found"
    src = tmp_path / ("use_header" + {"gcc": ".c", "g++": ".cpp"}[compiler])
    src.write_text('#include "detectorch_aug_hip.h"\nint use(void) { dtc_aug_view v; v.flipped = DTC_AUG_ID; '
                   'return DTC_AUG_MAX_ROWS / DTC_AUG_MAX_VIEWS + DTC_AUG_LOGIT_AVG + v.flipped; }\n')
    subprocess.check_call([cc] + flags + ["-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                                          str(tmp_path / "use_header.o")])


def test_constants_are_those_of_the_header():
    from detectorch_amd import hip_aug
    header = open(os.path.join(ROOT, "include", "detectorch_aug_hip.h")).read()
    define = lambda name: eval(re.search(r"#define DTC_AUG_%s (\(?[\d <]+\)?)" % name, header).group(1))
    assert (define("MAX_VIEWS"), define("MAX_ROIS"), define("MAX_ROWS"), define("MAX_CLASSES"), define("MAX_BATCH")) == (
        hip_aug.MAX_VIEWS, hip_aug.MAX_ROIS, hip_aug.MAX_ROWS, hip_aug.MAX_CLASSES, hip_aug.MAX_BATCH) == (8, 4096, 32768, 256, 65535)
    assert (define("MAX_MASK"), define("MAX_CHANNELS"), define("MAX_MASK_ROWS")) == (
        hip_aug.MAX_MASK, hip_aug.MAX_CHANNELS, hip_aug.MAX_MASK_ROWS) == (64, 1024, 1 << 20)
    assert {k: define(k) for k in hip_aug.BOX_HEURS} == hip_aug.BOX_HEURS == dict(UNION=0, AVG=1, ID=2)
    assert {k: define(k) for k in hip_aug.MASK_HEURS} == hip_aug.MASK_HEURS == dict(SOFT_AVG=0, SOFT_MAX=1, LOGIT_AVG=2)
    assert tuple(hip_aug.BOX_HEURS) == tr.BOX_HEURS and tuple(hip_aug.MASK_HEURS) == tr.MASK_HEURS
    assert "parity with Detectron itself is unpinned" in header


# ---- return codes: every refusal comes before the first HIP call, so bogus pointers are never touched -------------------------------
BOGUS = 256                                                    # a bogus, non-NULL, 16-byte aligned device pointer


def _merge(T=2, views="ok", **kw):
    from detectorch_amd import hip_aug
    arr = (hip_aug.AugView * max(T, 1))()
    for t in range(max(T, 1)):
        arr[t] = hip_aug.AugView(BOGUS, None, BOGUS, BOGUS, BOGUS, t % 2, 0)
    if callable(views):
        views(arr)
    a = dict(views=None if views is None else arr, n_views=T, im_size=BOGUS, batch=2, max_rois=67, n_cls=5, scores_are_logits=0, wx=10.0,
             wy=10.0, ww=5.0, wh=5.0, score_heur=0, coord_heur=0, out_scores=BOGUS, out_boxes=BOGUS, out_n=BOGUS, out_src=BOGUS)
    a.update(kw)
    order = [n for n, _ in hip_aug.SIGNATURES["dtc_aug_merge_boxes"][1][:-1]]
    return hip_aug.lib().dtc_aug_merge_boxes(*[a[n] for n in order], None)


def _combine(T=2, ptrs=None, flags=None, **kw):
    from detectorch_amd import hip_aug
    a = dict(masks=(C.c_void_p * max(T, 1))(*(ptrs or [(t + 1) << 28 for t in range(max(T, 1))])),
             flipped=(C.c_int32 * max(T, 1))(*(flags or [t % 2 for t in range(max(T, 1))])), n_views=T, det_count=BOGUS, mask_class=BOGUS,
             batch=3, max_out=4, n_cls=3, M=28, heur=0, out=15 << 28)
    a.update(kw)
    order = [n for n, _ in hip_aug.SIGNATURES["dtc_aug_combine_masks"][1][:-1]]
    return hip_aug.lib().dtc_aug_combine_masks(*[a[n] for n in order], None)


def test_return_codes_of_merge_boxes():
    for kw in (dict(T=0), dict(batch=0), dict(max_rois=0), dict(n_cls=1), dict(score_heur=3), dict(coord_heur=-1),
               dict(score_heur=0, coord_heur=1), dict(score_heur=2, coord_heur=0),              # Detectron: UNION for both or neither
               dict(views=None), dict(im_size=None), dict(out_scores=None), dict(out_boxes=None), dict(out_n=None), dict(out_src=None),
               dict(out_boxes=BOGUS + 4),
               dict(views=lambda a: setattr(a[1], "rois5", None)), dict(views=lambda a: setattr(a[1], "cls_score", None)),
               dict(views=lambda a: setattr(a[0], "bbox_pred", None)), dict(views=lambda a: setattr(a[1], "scale", None)),
               dict(views=lambda a: setattr(a[1], "bbox_pred", BOGUS + 8)), dict(views=lambda a: setattr(a[0], "flipped", 2))):
        assert _merge(**kw) == EINVAL, kw
    # limits: T <= 8, R <= 4096 (so T R <= 32768 holds by itself), n_cls - 1 <= 256, B <= 65535 -- and the last value inside each (a NULL keeps it from launching)
    for kw in (dict(T=9), dict(max_rois=4097), dict(T=5, max_rois=6554), dict(n_cls=258), dict(batch=65536)):
        assert _merge(**kw) == EUNSUPPORTED, kw
    for kw in (dict(T=8, max_rois=4096, score_heur=1, coord_heur=1), dict(T=8, max_rois=4096), dict(n_cls=257), dict(batch=65535),
               dict(T=1, max_rois=4096)):
        assert _merge(out_n=None, **kw) == EINVAL, kw
    assert _merge(T=0, max_rois=4097) == EINVAL                 # shapes and parameters in front of limits
    assert _merge(T=9, out_n=None) == EUNSUPPORTED              # limits in front of pointers


def test_return_codes_of_combine_masks():
    for kw in (dict(T=0), dict(batch=0), dict(max_out=0), dict(n_cls=0), dict(M=0), dict(heur=3), dict(heur=-1), dict(masks=None),
               dict(flipped=None), dict(det_count=None), dict(out=None), dict(out=(15 << 28) + 4), dict(ptrs=[1 << 28, 0]),
               dict(ptrs=[1 << 28, (2 << 28) + 8]), dict(flags=[0, 2]),
               dict(ptrs=[1 << 28, (15 << 28) + 16]), dict(ptrs=[(15 << 28) - 16, 2 << 28])):      # an input that overlaps out
        assert _combine(**kw) == EINVAL, kw
    for kw in (dict(T=9), dict(M=65), dict(n_cls=1025), dict(batch=65536), dict(batch=1024, max_out=1025), dict(batch=65535, max_out=17)):
        assert _combine(**kw) == EUNSUPPORTED, kw
    for kw in (dict(T=8), dict(M=64), dict(n_cls=1024), dict(batch=1024, max_out=1024, n_cls=1, M=1)):
        assert _combine(out=None, **kw) == EINVAL, kw
    assert _combine(mask_class=None, det_count=None) == EINVAL  # (mask_class may be NULL; det_count may not)
    assert _combine(T=0, M=65) == EINVAL and _combine(T=9, out=None) == EUNSUPPORTED


def test_wrapper_limit_arithmetic_and_heuristics():
    from detectorch_amd import hip_aug
    assert hip_aug.merge_rows(3, 1000) == 3000 and hip_aug.merge_rows(3, 1000, "AVG") == 1000 and hip_aug.merge_rows(8, 4096) == 32768
    for T, Rr in ((0, 10), (9, 10), (1, 4097), (1, 0)):
        with pytest.raises(ValueError):
            hip_aug.merge_rows(T, Rr)
    assert hip_aug.box_heurs("UNION", "UNION") == (0, 0) and hip_aug.box_heurs("AVG", "ID") == (1, 2)
    for pair in (("UNION", "AVG"), ("ID", "UNION")):
        with pytest.raises(ValueError, match="both be UNION or neither"):
            hip_aug.box_heurs(*pair)
    with pytest.raises(NotImplementedError):
        hip_aug.box_heurs("MAX", "MAX")


def test_wrappers_refuse_cpu_tensors():
    import torch
    from detectorch_amd import hip_aug
    views, im = tc.merge_case(1, tc.UNION_COUNTS, False)
    v = {k: (torch.from_numpy(x) if isinstance(x, np.ndarray) else x) for k, x in views[0].items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_aug.merge_boxes([v], torch.from_numpy(im))
    masks, flipped, cnt, mc = tc.combine_case(7, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_aug.combine_masks([torch.from_numpy(m) for m in masks], flipped, torch.from_numpy(cnt), torch.from_numpy(mc))
    with pytest.raises(NotImplementedError):
        hip_aug.combine_masks([torch.from_numpy(m) for m in masks], flipped, torch.from_numpy(cnt), heur="HARD")


# ---- the restatement against itself and against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("heur", tr.BOX_HEURS)
@pytest.mark.parametrize("logits", [False, True])
def test_single_unflipped_view_is_the_per_view_decode_is_the_oracles(oracle, heur, logits):
    views, im = tc.merge_case(1, tc.ALIGNED_COUNTS, logits)
    assert not views[0]["flipped"]
    out = tr.merge_boxes(views, im, heur, heur, logits)
    v = views[0]
    for b in range(tc.B):
        n = int(v["n_rois"][b])
        assert out["out_n"][b] == n
        per_view = tr.view_boxes(v["rois5"][b, :n, 1:], v["scale"][b], im[b], v["bbox_pred"][b, :n], False)
        orc = dr.decode(oracle, v["rois5"][b, :n, 1:], v["scale"][b], im[b], v["bbox_pred"][b, :n])
        assert out["out_boxes"][b, :n].tobytes() == per_view.tobytes() == orc.tobytes()
        sc = oracle.softmax_rows(v["cls_score"][b, :n]) if logits else v["cls_score"][b, :n]
        assert out["out_scores"][b, :n].tobytes() == sc.tobytes()
        assert not out["out_boxes"][b, n:].any() and not out["out_scores"][b, n:].any() and (out["out_src"][b, n:] == -1).all()
        assert (out["out_src"][b, :n] == np.arange(n)).all()


def test_flipping_twice_is_the_identity_on_integer_boxes():
    rs = np.random.RandomState(5)
    for w in (1, 2, 833, 4097):
        x = np.sort(rs.randint(0, w, (50, 2, 3)), axis=1).astype(f32)
        y = rs.randint(0, 600, (50, 2, 3)).astype(f32)
        boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=2).reshape(50, 12)
        once = tr.flip_boxes(boxes, w)
        assert np.array_equal(tr.flip_boxes(once, w), boxes)
        assert (once[:, 0::4] <= once[:, 2::4]).all() and np.array_equal(once[:, 1::4], boxes[:, 1::4])
        assert np.array_equal(once[:, 0::4], w - 1 - boxes[:, 2::4])


def test_merge_rules_on_the_cases():
    """UNION stacks the views' live rows in view order; AVG is the float32 sum in view order over T; ID the last view; a flipped view is
    clipped BEFORE it is mirrored (the cases hold boxes the clip moves)"""
    views, im = tc.merge_case(8, tc.UNION_COUNTS, False)
    assert [v["flipped"] for v in views] == [bool(f) for f in tc.FLIPS] and {tuple(v["n_rois"]) for v in views} == {(0, 67), (67, 1)}
    out = tr.merge_boxes(views, im)
    assert out["out_n"].tolist() == [4 * 67, 4 * 67 + 4] and out["out_boxes"].shape == (2, 8 * 67, 20)
    at = 0
    for t, v in enumerate(views):
        n = int(v["n_rois"][1])
        assert (out["out_src"][1, at:at + n] == t * tc.R + np.arange(n)).all()
        one = tr.view_boxes(v["rois5"][1, :n, 1:], v["scale"][1], im[1], v["bbox_pred"][1, :n], v["flipped"])
        assert np.array_equal(out["out_boxes"][1, at:at + n], one)
        if v["flipped"] and n > 1:
            raw = tr.bbox_transform(v["rois5"][1, :n, 1:] / v["scale"][1], v["bbox_pred"][1, :n])
            moved = (raw[:, 0::4] < 0) | (raw[:, 2::4] > im[1, 1] - 1)
            assert moved.any() and not np.array_equal(tr.flip_boxes(raw, im[1, 1])[moved.repeat(4, 1)], one[moved.repeat(4, 1)])
        at += n
    assert np.isfinite(out["out_boxes"]).all() and np.isfinite(out["out_scores"]).all()          # the NaN rows past the counts stay out
    assert (out["out_boxes"][0, :, 0::2] == 0).all()                                               # width 1: every x is 0
    views, im = tc.merge_case(3, tc.ALIGNED_COUNTS, False)
    avg, last = tr.merge_boxes(views, im, "AVG", "AVG"), tr.merge_boxes(views, im, "ID", "ID")
    per = [tr.merge_boxes([v], im, "ID", "ID") for v in views]
    want = ((per[0]["out_boxes"] + per[1]["out_boxes"]) + per[2]["out_boxes"]) / f32(3)
    assert avg["out_boxes"].tobytes() == want.astype(f32).tobytes() and last["out_boxes"].tobytes() == per[2]["out_boxes"].tobytes()
    assert avg["out_n"].tolist() == [61, 67] and (last["out_src"][1] == 2 * tc.R + np.arange(67)).all()
    mixed = tr.merge_boxes(views, im, "AVG", "ID")
    assert mixed["out_scores"].tobytes() == avg["out_scores"].tobytes() and mixed["out_boxes"].tobytes() == last["out_boxes"].tobytes()
    with pytest.raises(AssertionError):
        tr.merge_boxes(views, im, "UNION", "AVG")


def test_saturated_deltas_reach_the_clips():
    views, im = tc.merge_case(3, tc.ALIGNED_COUNTS, False)
    v = views[1]
    d = v["bbox_pred"][1, :67]
    assert (d[:, 2::4] / 5 > tr.BBOX_XFORM_CLIP).any() and (np.abs(d[:, 0::4]) == 1e4).any()


def test_mask_rules_by_hand():
    a = np.array([0.25, 0.5, 0.75, 1.0], f32).reshape(1, 1, 1, 4).repeat(2, 2)[:, :, :2]      # [1,1,2,4]
    b = np.array([0.5, 0.5, 0.25, 0.0], f32).reshape(1, 1, 1, 4).repeat(2, 2)[:, :, :2]
    cnt = np.array([1], np.int32)
    pad = lambda m: np.pad(m, ((0, 0), (0, 0), (0, 2), (0, 0)))                                # square maps: [1,1,4,4]
    a, b = pad(a), pad(b)
    avg = tr.combine_masks([a, b], (0, 1), cnt, None, "SOFT_AVG")
    assert avg[0, 0, 0].tolist() == [0.125, 0.375, 0.625, 0.75]                                # b mirrored: 0, .25, .5, .5
    assert tr.combine_masks([a, b], (0, 1), cnt, None, "SOFT_MAX")[0, 0, 0].tolist() == [0.25, 0.5, 0.75, 1.0]
    assert tr.combine_masks([a, b], (1, 0), cnt, None, "SOFT_MAX")[0, 0, 0].tolist() == [1.0, 0.75, 0.5, 0.25]
    # the mirror: a flipped view of the mirrored tensor is the unflipped view
    for heur in tr.MASK_HEURS:
        assert np.array_equal(tr.combine_masks([a, b[..., ::-1]], (0, 1), cnt, None, heur), tr.combine_masks([a, b], (0, 0), cnt, None, heur))
    # LOGIT_AVG: the mean of logits of p and 1 - p is 0 -> 0.5; y = 1 in any view -> exactly 1; y = 0 in every view -> 1e-20's sigmoid
    p = np.full((1, 1, 4, 4), 0.25, f32)
    for exact in (True, False):
        assert np.allclose(tr.combine_masks([p, 1 - p], (0, 0), cnt, None, "LOGIT_AVG", exact), 0.5, atol=1e-7)
        one = tr.combine_masks([np.ones_like(p), p * 0], (0, 0), cnt, None, "LOGIT_AVG", exact)
        assert (one == 1.0).all()
        zero = tr.combine_masks([p * 0, p * 0], (0, 0), cnt, None, "LOGIT_AVG", exact)
        assert np.isfinite(zero).all() and (zero > 0).all() and (zero < 2e-20).all()
    assert (tr.combine_masks64([np.ones_like(p), p * 0], (0, 0), cnt) == 1.0).all()
    # rows past det_count and the channels that are not the row's class are zeros
    masks, flipped, cnt, mc = tc.combine_case(7, 2)
    out = tr.combine_masks(masks, flipped, cnt, mc, "SOFT_MAX")
    D = tc.MAX_OUT
    assert not out[:D].any() and not out[D + 3:2 * D].any() and out[D:D + 3].any() and out[2 * D:].any()
    assert not out[D + 1].any() and not out[2 * D + 2].any()                                    # classes -1 and K select nothing
    for r in (D, 2 * D + 3):
        for k in range(tc.K):
            assert out[r, k].any() == (k == mc[r])
    assert np.array_equal(tr.combine_masks(masks, flipped, cnt, None, "SOFT_MAX")[D], np.maximum(masks[0][D], masks[1][D][..., ::-1]))


@pytest.mark.parametrize("M", [28, 7])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_logit_avg_forms_stay_close_and_special_values_meet(M, T):
    """the tolerance the GPU test derives exists and is small: the float32 form Detectron runs stays within 1e-5 of the float64 form on
    the special-value case; zeros meet zeros and ones meet ones in every view"""
    masks, flipped, cnt, mc = tc.combine_case(M, T, special=True)
    seen = [m[..., ::-1] if f else m for m, f in zip(masks, flipped)]
    assert all((s[..., 0] == 0).all() and (s[..., 2] == 1).all() for s in seen)
    assert all(np.isin(tc.SPECIAL, m).all() for m in masks)
    lit = tr.combine_masks(masks, flipped, cnt, None, "LOGIT_AVG", exact=False)
    ref = tr.combine_masks64(masks, flipped, cnt)
    dev = np.abs(lit.astype(np.float64) - ref).max()
    assert 0 < dev < 1e-5
    assert np.isfinite(lit).all() and (lit[2 * tc.MAX_OUT:, :, :, 2] == 1).all() and (ref[2 * tc.MAX_OUT:, :, :, 2] == 1).all()
    cr_ = tr.combine_masks(masks, flipped, cnt, None, "LOGIT_AVG", exact=True)
    assert np.abs(cr_.astype(np.float64) - ref).max() <= 2 * dev


# ---- the model-level options ----------------------------------------------------------------------------------------------------------
def test_aug_options_defaults_validation_and_view_order():
    from detectorch_amd.utils.test_aug import AugOptions
    a = AugOptions()
    assert (a.h_flip, a.scales, a.max_size, a.scale_h_flip, a.score_heur, a.coord_heur, a.mask_heur, a.test_scale, a.test_max_size) == (
        False, (), 4000, False, 'UNION', 'UNION', 'SOFT_AVG', 800, 1333)
    assert a.views() == [(800, 1333, False)]                                                    # the identity view alone
    # Detectron's order: the flip of the base scale, each extra scale (followed by its flip with scale_h_flip), the identity last
    assert AugOptions(h_flip=True, scales=(400, 1200)).views() == [(800, 1333, True), (400, 4000, False), (1200, 4000, False), (800, 1333, False)]
    assert AugOptions(h_flip=True, scales=(400,), scale_h_flip=True, max_size=2000, test_scale=600, test_max_size=1000).views() == [
        (600, 1000, True), (400, 2000, False), (400, 2000, True), (600, 1000, False)]
    assert AugOptions(scales=(400,), scale_h_flip=True).views() == [(400, 4000, False), (400, 4000, True), (800, 1333, False)]
    for pair in (("UNION", "AVG"), ("ID", "UNION"), ("AVG", "UNION")):
        with pytest.raises(ValueError, match="both be UNION or neither"):
            AugOptions(score_heur=pair[0], coord_heur=pair[1])
    assert AugOptions(score_heur="AVG", coord_heur="ID").score_heur == "AVG"
    with pytest.raises(NotImplementedError):
        AugOptions(score_heur="MAX", coord_heur="MAX")
    with pytest.raises(NotImplementedError):
        AugOptions(mask_heur="HARD")
    with pytest.raises(ValueError):
        AugOptions(scales=(0,))
    with pytest.raises(ValueError, match="at most 8"):
        AugOptions(h_flip=True, scales=(1, 2, 3, 4), scale_h_flip=True)                          # 1 + 8 + 1 views
    assert len(AugOptions(h_flip=True, scales=(1, 2, 3), scale_h_flip=True).views()) == 8


def test_rows_past_the_detection_entry_raise_naming_both_numbers():
    from detectorch_amd.utils.test_aug import AugOptions
    assert AugOptions(h_flip=True, scales=(400, 1200)).check_rows(1000) == 4 and AugOptions().check_rows(4096) == 1
    with pytest.raises(ValueError, match=r"5 views x 1000 rois = 5000 .* takes 4096"):
        AugOptions(h_flip=True, scales=(400, 1200, 1600)).check_rows(1000)
    with pytest.raises(ValueError, match=r"2 views x 2049 rois"):
        AugOptions(h_flip=True).check_rows(2049)


def test_logit_avg_binarisation_cap_holds_for_the_restatement_alone():
    """the model-level LOGIT_AVG check compares binarised pixels away from the threshold: on the seeded case the band of the
    tolerance around 0.5 holds far fewer than 0.1 % of the pixels, and outside it the float32 form binarises as the float64 form"""
    masks, flipped, cnt, mc = tc.combine_case(28, 2)
    ref = tr.combine_masks64(masks, flipped, cnt, mc)
    lit = tr.combine_masks(masks, flipped, cnt, mc, "LOGIT_AVG", exact=False)
    tol = 2 * np.abs(lit.astype(np.float64) - ref).max()
    near = np.abs(ref - 0.5) <= tol
    assert near.mean() <= 1e-3 and np.array_equal((lit > 0.5)[~near], (ref > 0.5)[~near])
