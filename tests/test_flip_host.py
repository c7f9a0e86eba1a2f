"""The flip augmentation without a GPU (tests/README_flip.md):
  * libdetectorch_flip_hip.so exports exactly what include/detectorch_flip_hip.h declares and hip_flip.SIGNATURES binds it, parameter
    names and kinds in order; the exports of the ten other libraries are unchanged; the header compiles as pedantic C99 and C++11;
    the constants of header and binding agree; the workspace size; the return codes on bad arguments (validation precedes every HIP
    call, so nothing is launched and the bogus pointers are never used);
  * the numpy restatements (tests/flip_ref.py) against answers derived by hand and against the recorded outputs of the reference's
    own flip_boxes (tests/golden/flip_boxes_reference.npz);
  * the Python layer: CPU tensors are refused, flip_segms on polygon-only input."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden
import flip_cases as fc
import flip_ref as fr

sys.path.insert(0, GOLDEN)                                    # make_native_host_codes.exports

NAMES = ["dtc_flip_boxes", "dtc_flip_polygons", "dtc_flip_prep_images", "dtc_flip_rle", "dtc_flip_rle_workspace_bytes",
         "dtc_flip_target_arch"]


# ---- the library: exports, binding, header, constants -----------------------------------------------------------------------------------
def test_header_symbols_are_exported_and_bound():
    from make_native_host_codes import exports
    from test_binding_signatures_host import _struct_of, prototypes
    from detectorch_amd import hip_flip
    lib = hip_flip.lib()
    protos = prototypes("detectorch_flip_hip.h")
    assert sorted(protos) == NAMES and exports(hip_flip.LIB_PATH) == NAMES and sorted(hip_flip.SIGNATURES) == NAMES
    assert list(protos) == list(hip_flip.SIGNATURES)                                             # the header's order
    for entry, (ret, params) in protos.items():
        row = hip_flip.SIGNATURES[entry]
        assert row[0] == ret and [n for n, _ in row[1]] == [n for n, _ in params], entry
        assert [k if isinstance(k, str) else _struct_of(k) for _, k in row[1]] == [k for _, k in params], entry
    assert lib.dtc_flip_target_arch() == b"gfx950"


def test_the_other_libraries_export_what_they_did():
    """the first library's 42 exports are the recorded ones; every other side library exports what its own binding table names, and
    none of them a dtc_flip_ name"""
    import json
    from make_native_host_codes import exports
    from detectorch_amd import build, hip, hip_eval, hip_grad, hip_loss, hip_mask, hip_optim, hip_poly, hip_rpn, hip_segm, hip_train
    build.build()
    recorded = json.load(open(os.path.join(GOLDEN, "native_host_codes.json")))["exports"]
    assert exports(hip.LIB_PATH) == recorded and len(recorded) == 42
    for mod in (hip_train, hip_loss, hip_grad, hip_optim, hip_rpn, hip_mask, hip_eval, hip_segm, hip_poly):
        mod.lib()
        assert exports(mod.LIB_PATH) == sorted(mod.SIGNATURES), mod.__name__
    for mod in (hip, hip_train, hip_loss, hip_grad, hip_optim, hip_rpn, hip_mask, hip_eval, hip_segm, hip_poly):
        assert not [n for n in exports(mod.LIB_PATH) if n.startswith("dtc_flip_")], mod.__name__


@pytest.mark.parametrize("compiler,flags", [("gcc", ["-std=c99"]), ("g++", ["-std=c++11"])])
def test_header_compiles_as_pedantic_c99_and_cxx11(tmp_path, compiler, flags):
    cc = shutil.which(compiler) or shutil.which({"gcc": "cc", "g++": "c++"}[compiler])
    assert cc, compiler + " not found"
    src = tmp_path / ("use_header" + {"gcc": ".c", "g++": ".cpp"}[compiler])
    src.write_text('#include "detectorch_flip_hip.h"\nint use(void) { return DTC_FLIP_MAX_RUNS / DTC_FLIP_MAX_ROWS + DTC_FLIP_MAX_BOX_COLS; }\n')
    subprocess.check_call([cc] + flags + ["-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                                          str(tmp_path / "use_header.o")])


def test_constants_are_those_of_the_header():
    from detectorch_amd import hip_flip, hip_poly, hip_segm
    header = open(os.path.join(ROOT, "include", "detectorch_flip_hip.h")).read()
    define = lambda name: eval(re.search(r"#define DTC_FLIP_MAX_%s (\(?[\d <]+\)?)" % name, header).group(1))
    assert (define("BATCH"), define("BOX_ROWS"), define("BOX_COLS")) == (hip_flip.MAX_BATCH, hip_flip.MAX_BOX_ROWS, hip_flip.MAX_BOX_COLS)
    assert (define("POINTS"), define("POLYS")) == (hip_flip.MAX_POINTS, hip_flip.MAX_POLYS) == (hip_poly.MAX_POINTS, hip_poly.MAX_POLYS)
    assert (define("RUNS"), define("PIXELS")) == (hip_flip.MAX_RUNS, hip_flip.MAX_PIXELS) == (hip_segm.MAX_RUNS, hip_segm.MAX_PIXELS)
    assert define("ROWS") == hip_flip.MAX_ROWS == 65535 and define("RUNS") >= 65536 and define("PIXELS") == 1 << 30
    src = open(os.path.join(ROOT, "detectorch_amd", "csrc", "prep_pixel.h")).read()
    assert int(re.search(r"constexpr int kPrepMaxBatch = (\d+);", src).group(1)) == hip_flip.MAX_PREP_BATCH


def test_workspace_bytes():
    from detectorch_amd import hip_flip
    f = hip_flip.lib().dtc_flip_rle_workspace_bytes
    ok = (3, 12, 500)
    for at, bad in ((0, 0), (0, 65536), (1, -1), (1, 65536), (2, 0), (2, (1 << 20) + 1)):
        assert f(*[bad if i == at else v for i, v in enumerate(ok)]) == 0, (at, bad)
    base = f(*ok)
    assert base >= 3 * 12 * 500 * 3 * 8 and base % 16 == 0 and f(3, 0, 1) > 0
    for at in range(3):                                         # monotone in every argument
        assert f(*[v + 1 if i == at else v for i, v in enumerate(ok)]) > base, at
    assert f(65535, 65535, 1 << 20) > 1 << 50                     # no 32-bit overflow


BOGUS = 256                                                    # a bogus, non-NULL, 16-byte aligned device pointer
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -3, -4


def _caller(entry, order, ints, apart=()):
    """-> call(**overrides): every pointer of `order` bogus but non-NULL unless overridden (None: NULL) -- those of `apart` 16 MiB from
    each other, the others all the same --, the ints from `ints`"""
    def call(**kw):
        from detectorch_amd import hip_flip
        vals = dict(ints, **{k: kw.pop(k) for k in list(kw) if k in ints})
        ptrs = {k: kw.pop(k, (apart.index(k) + 1) << 24 if k in apart else BOGUS) for k in order if k not in ints}
        assert not kw, kw
        args = [vals[k] if k in vals else (None if ptrs[k] is None else C.c_void_p(ptrs[k])) for k in order]
        return getattr(hip_flip.lib(), entry)(*args, None)
    return call


def test_return_codes_of_flip_boxes():
    call = _caller("dtc_flip_boxes", ("boxes", "counts", "im_width", "flipped", "batch", "R", "cols", "out"), dict(batch=3, R=6, cols=4))
    codes = {
        "batch 0": (dict(batch=0), EINVAL), "R -1": (dict(R=-1), EINVAL), "cols 0": (dict(cols=0), EINVAL), "cols 6": (dict(cols=6), EINVAL),
        "cols -4": (dict(cols=-4), EINVAL), "cols 5 + batch 65536": (dict(cols=5, batch=65536), EINVAL),
        "batch 65536": (dict(batch=65536), EUNSUPPORTED), "R 2^20 + 1": (dict(R=(1 << 20) + 1), EUNSUPPORTED),
        "cols 4100": (dict(cols=4100), EUNSUPPORTED), "batch 65536 + boxes NULL": (dict(batch=65536, boxes=None), EUNSUPPORTED),
        "boxes NULL": (dict(boxes=None), EINVAL), "im_width NULL": (dict(im_width=None), EINVAL), "flipped NULL": (dict(flipped=None), EINVAL),
        "out NULL": (dict(out=None), EINVAL),
        "partial overlap": (dict(boxes=4096, out=4096 + 16), EINVAL), "overlap from below": (dict(boxes=4096 + 3 * 6 * 16 - 4, out=4096), EINVAL),
        "R 0": (dict(R=0), OK), "R 0, NULL boxes": (dict(R=0, boxes=None, out=None, counts=None), OK), "R 0 + flipped NULL": (dict(R=0, flipped=None), EINVAL),
    }
    assert {k: call(**kw) for k, (kw, _) in codes.items()} == {k: v[1] for k, v in codes.items()}


def test_return_codes_of_flip_polygons():
    call = _caller("dtc_flip_polygons", ("poly_xy", "poly_ptr", "im_width", "flipped", "batch", "PTS", "NP", "out64", "out32"),
                   dict(batch=3, PTS=16, NP=5))
    codes = {
        "batch 0": (dict(batch=0), EINVAL), "PTS -1": (dict(PTS=-1), EINVAL), "NP -1": (dict(NP=-1), EINVAL),
        "batch 65536": (dict(batch=65536), EUNSUPPORTED), "PTS 65537": (dict(PTS=65537), EUNSUPPORTED), "NP 4097": (dict(NP=4097), EUNSUPPORTED),
        "NP 4097 + both outputs NULL": (dict(NP=4097, out64=None, out32=None), EUNSUPPORTED),
        "both outputs NULL": (dict(out64=None, out32=None), EINVAL), "poly_xy NULL": (dict(poly_xy=None), EINVAL),
        "poly_ptr NULL": (dict(poly_ptr=None), EINVAL), "im_width NULL": (dict(im_width=None), EINVAL), "flipped NULL": (dict(flipped=None), EINVAL),
        "poly_xy misaligned": (dict(poly_xy=BOGUS + 4), EINVAL), "out64 misaligned": (dict(out64=8192 + 4), EINVAL),
        "out64 overlaps": (dict(poly_xy=4096, out64=4096 + 16, out32=1 << 20), EINVAL), "out32 overlaps": (dict(poly_xy=4096, out64=1 << 20, out32=4096 + 8), EINVAL),
        "outputs overlap": (dict(poly_xy=4096, out64=1 << 20, out32=(1 << 20) + 64), EINVAL),
        "PTS 0": (dict(PTS=0, poly_xy=None), OK), "PTS 0 + both outputs NULL": (dict(PTS=0, out64=None, out32=None), EINVAL),
    }
    assert {k: call(**kw) for k, (kw, _) in codes.items()} == {k: v[1] for k, v in codes.items()}


def test_return_codes_of_flip_rle():
    from detectorch_amd import hip_flip
    order = ("runs", "n_runs", "counts", "im_size", "flipped", "batch", "R", "runs_stride", "workspace", "workspace_bytes", "out_runs",
             "out_stride", "out_n_runs", "need")
    ints = dict(batch=3, R=12, runs_stride=500, workspace_bytes=1 << 30, out_stride=700)
    call = _caller("dtc_flip_rle", order, ints, apart=("runs", "out_runs"))
    need = hip_flip.lib().dtc_flip_rle_workspace_bytes(3, 12, 500)
    assert 0 < need <= ints["workspace_bytes"]
    codes = {
        "batch 0": (dict(batch=0), EINVAL), "R -1": (dict(R=-1), EINVAL), "runs_stride 0": (dict(runs_stride=0), EINVAL),
        "out_stride 0": (dict(out_stride=0), EINVAL), "R 65536 + out_stride 0": (dict(R=65536, out_stride=0), EINVAL),
        "batch 65536": (dict(batch=65536), EUNSUPPORTED), "R 65536": (dict(R=65536), EUNSUPPORTED),
        "runs_stride 2^20 + 1": (dict(runs_stride=(1 << 20) + 1), EUNSUPPORTED), "out_stride 2^20 + 1": (dict(out_stride=(1 << 20) + 1), EUNSUPPORTED),
        "R 65536 + im_size NULL": (dict(R=65536, im_size=None), EUNSUPPORTED),
        **{k + " NULL": ({k: None}, EINVAL) for k in ("runs", "n_runs", "im_size", "flipped", "out_runs", "out_n_runs", "need")},
        "counts NULL is no error": (dict(counts=None, workspace_bytes=0), EWORKSPACE),
        "workspace misaligned": (dict(workspace=BOGUS + 8), EINVAL),
        "out_runs is runs": (dict(runs=1 << 20, out_runs=1 << 20), EINVAL),
        "out_runs inside runs": (dict(runs=1 << 20, out_runs=(1 << 20) + 3 * 12 * 500 * 4 - 4), EINVAL),
        "runs inside out_runs": (dict(out_runs=1 << 20, runs=(1 << 20) + 3 * 12 * 700 * 4 - 4), EINVAL),
        "out_runs right behind runs": (dict(runs=1 << 20, out_runs=(1 << 20) + 3 * 12 * 500 * 4, workspace_bytes=0), EWORKSPACE),
        "workspace NULL": (dict(workspace=None), EWORKSPACE), "workspace 0 bytes": (dict(workspace_bytes=0), EWORKSPACE),
        "workspace one byte short": (dict(workspace_bytes=need - 1), EWORKSPACE),
        "R 0": (dict(R=0), OK), "R 0, NULL pointers": (dict(R=0, runs=None, n_runs=None, counts=None, out_runs=None, out_n_runs=None, need=None), OK),
        "R 0 + flipped NULL": (dict(R=0, flipped=None), EINVAL), "R 0 + workspace NULL": (dict(R=0, workspace=None), EWORKSPACE),
    }
    assert {k: call(**kw) for k, (kw, _) in codes.items()} == {k: v[1] for k, v in codes.items()}
    assert len(codes) >= 28


def test_return_codes_of_flip_prep_images():
    """dtc_prep_images' checks, plus the flags"""
    from detectorch_amd import hip, hip_flip
    lib = hip_flip.lib()
    B = 2
    good = lambda: (hip.Image * B)(hip.Image(BOGUS, 5, 7, 2, 21), hip.Image(BOGUS, 13, 9, 0, 40))
    flags, means, scales = (C.c_int32 * B)(1, 0), (C.c_double * 3)(1, 2, 3), (C.c_double * B)(1.0, 1.0)
    out_hw = (C.c_int32 * (2 * B))(5, 7, 13, 9)
    blob = C.c_void_p(BOGUS)

    def call(images=None, batch=B, flipped=flags, pixel_means=means, im_scales=scales, hw=out_hw, blob=blob, bh=13, bw=9):
        return lib.dtc_flip_prep_images(good() if images is None else images, batch, flipped, pixel_means, im_scales, hw, blob, bh, bw, None)
    assert call(flipped=None) == EINVAL and call(batch=0) == EINVAL and call(pixel_means=None) == EINVAL and call(im_scales=None) == EINVAL
    assert call(hw=None) == EINVAL and call(blob=None) == EINVAL and call(bh=0) == EINVAL and call(bw=0) == EINVAL
    assert call(bh=12) == EINVAL and call(bw=8) == EINVAL                                       # a resized image larger than the blob
    big = (hip.Image * 33)(*[hip.Image(BOGUS, 5, 7, 2, 21)] * 33)
    assert lib.dtc_flip_prep_images(big, 33, (C.c_int32 * 33)(), means, (C.c_double * 33)(), (C.c_int32 * 66)(), blob, 13, 9, None) == EUNSUPPORTED
    for bad in (hip.Image(0, 5, 7, 2, 21), hip.Image(BOGUS, 0, 7, 2, 21), hip.Image(BOGUS, 5, 0, 2, 21), hip.Image(BOGUS, 5, 7, 1, 21),
                hip.Image(BOGUS, 5, 7, 2, 20)):
        ims = good()
        ims[0] = bad
        assert call(images=ims) == EINVAL


# ---- the restatements against answers derived by hand ----------------------------------------------------------------------------------------
def test_flip_ref_known_answers():
    # boxes: float32, (w - x2) - 1 and (w - x1) - 1; y untouched; a box touching both borders maps onto itself
    assert fr.flip_boxes(np.array([[0, 3, 639, 7], [10.5, 1, 20.25, 2]], np.float32), 640).tolist() == [[0, 3, 639, 7], [618.75, 1, 628.5, 2]]
    assert fr.flip_boxes(np.array([[0, 0, 0, 0]], np.float32), 1).tolist() == [[0, 0, 0, 0]]
    b8 = fr.flip_boxes(np.array([[1, 2, 3, 4, 5, 6, 8, 9]], np.float32), 10)
    assert b8.dtype == np.float32 and b8.tolist() == [[6, 2, 8, 4, 1, 6, 4, 9]]
    # polygons: double; at w = 640, x = 639.49 the float32 rounding of the double flip is not the float32 flip of the float32 point
    x = fr.flip_poly([639.49, 5.0, 100.1, 6.0], 640)
    assert x == [640 - 639.49 - 1, 5.0, 640 - 100.1 - 1, 6.0]
    f32_of_double, f32_flip = np.float32(x[0]), np.float32(640) - np.float32(639.49) - np.float32(1)
    assert f32_of_double == np.float32(-0.49) and f32_flip == np.float32(-0.48999023) and f32_of_double != f32_flip
    for v in (100.1, 0.3, 333.33, 12.7, 17.05):                 # and here the two agree
        assert np.float32(fr.flip_poly([v, 0.0], 640)[0]) == np.float32(640) - np.float32(v) - np.float32(1), v
    # run lists: the 3 x 4 mask with pixels (2, 1) and (0, 2) -- positions 5 and 6 -- goes to (2, 2) and (0, 1): positions 3 and 8
    assert fr.decode([5, 2, 5], 3, 4).nonzero()[0].tolist() == [0, 2] and fr.decode([5, 2, 5], 3, 4).nonzero()[1].tolist() == [2, 1]
    assert fr.flip_rle_runs([5, 2, 5], 3, 4) == [3, 1, 4, 1, 3]
    assert fr.flip_rle_runs([1], 1, 1) == [1] and fr.flip_rle_runs([0, 1], 1, 1) == [0, 1]
    assert fr.flip_rle_runs([0, 1, 2, 2, 1], 1, 6) == [1, 2, 2, 1]                               # a single row reverses the runs
    assert fr.flip_rle_runs([1, 2, 2, 1], 6, 1) == [1, 2, 2, 1]                                 # a single column is the identity
    assert fr.flip_rle_runs([0, 35], 5, 7) == [0, 35] and fr.flip_rle_runs([35], 5, 7) == [35]
    assert fr.flip_rle_runs([0, 0, 4, 0, 0, 3, 0, 2, 6, 0, 20, 0], 5, 7) == fr.flip_rle_runs([4, 3, 0, 2, 26], 5, 7)      # zero-length runs
    assert fr.flip_rle_runs([0, 0, 0, 12], 3, 4) == [0, 12]
    # 7 x 1333, pixels (3, 2) and (6, 1200): positions 17 and 8406 -> columns 1330 and 132: positions 9313 and 930
    assert fr.flip_rle_runs([17, 1, 8388, 1, 924], 7, 1333) == [930, 1, 8382, 1, 17]
    runs = fc.blob_runs()
    assert 65 <= len(runs) <= 4096 and len(runs) == 889
    twice = fr.flip_rle_runs(fr.flip_rle_runs(runs, *fc.BLOB_HW), *fc.BLOB_HW)
    assert twice == runs and sum(fr.flip_rle_runs(runs, *fc.BLOB_HW)[1::2]) == sum(runs[1::2])
    for name, h, w, row in fc.rle_rows():                         # every shared case is well-formed, and its answer canonical
        got = fr.flip_rle_runs(row, h, w)
        assert sum(got) == h * w and all(v > 0 for v in got[1:]), name
        assert np.array_equal(fr.decode(got, h, w), fr.decode(row, h, w)[:, ::-1]), name
    # the batched form: the states of a row
    runs, n = fc.pack_runs([[5, 2, 5], [5, 2, 5], [5, 2, 4], [12], []], 4, {1: -1})
    lists, out_n, need = fr.flip_rle_batched(runs, n, [(3, 4)], [1], 5)
    assert out_n.tolist() == [[5, -1, -1, 1, 0]] and need.tolist() == [[5, 0, 0, 1, 0]] and lists[0][0] == [3, 1, 4, 1, 3]
    assert fr.flip_rle_batched(runs, n, [(3, 4)], [1], 4)[1].tolist() == [[-1, -1, -1, 1, 0]]
    assert fr.flip_rle_batched(runs, n, [(3, 4)], [0], 3, counts=[3])[1].tolist() == [[3, -1, 3, 0, 0]]


def test_flip_boxes_restatement_is_the_reference():
    """tests/golden/flip_boxes_reference.npz: the outputs of the reference's own lib/utils/boxes.py:flip_boxes on the box cases"""
    ref = golden("flip_boxes_reference")
    for cols in (4, 8):
        boxes = fc.box_case(cols)
        for b, w in enumerate(fc.BOX_WIDTHS):
            want = ref["cols%d_image%d" % (cols, b)]
            got = fr.flip_boxes(boxes[b], w)
            assert want.dtype == np.float32 and got.tobytes() == want.tobytes(), (cols, b)
    assert np.array_equal(ref["widths"], fc.BOX_WIDTHS)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_the_cpu():
    import torch
    from detectorch_amd import hip_flip
    from detectorch_amd.utils import augment, segms
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_flip.flip_boxes(z(1, 2, 4, dt=torch.float32), z(1), z(1))
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_flip.flip_polygons(z(1, 4, 2, dt=torch.float64), z(1, 2), z(1), z(1))
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_flip.flip_rle(z(1, 2, 4), z(1, 2), z(1, 2, dt=torch.float32), z(1))
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_flip.prep_images([torch.zeros(5, 7, 3, dtype=torch.uint8)], [1])
    with pytest.raises(RuntimeError, match="GPU only"):
        segms.flip_segms([dict(size=[3, 4], counts=[5, 2, 5])], 3, 4, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        augment.flip_batch(dict(gt_boxes=z(1, 2, 4, dt=torch.float32)), z(1), z(1))


def test_flip_segms_on_polygons_needs_no_gpu():
    from detectorch_amd.utils import segms
    src = [[[639.49, 10.0, 100.1, 20.5, 0.3, 333.33]], [[12.7, 1.0, 17.05, 2.0, 333.33, 3.0], [0.0, 0.0, 639.0, 0.0, 320.5, 479.0]], []]
    keep = [[list(p) for p in s] for s in src]
    got = segms.flip_segms(src, 480, 640)
    assert got == [[fr.flip_poly(p, 640) for p in s] for s in src] and src == keep              # equal as doubles; the input is untouched
    assert got[0][0][0] == 640 - 639.49 - 1 and got[0][0][1] == 10.0 and isinstance(got[0][0][0], float)
    assert segms.flip_segms(got, 480, 640)[2] == [] and segms.flip_segms([], 480, 640) == []
