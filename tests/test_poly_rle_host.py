"""The polygon conversion without a GPU (tests/README_poly_rle.md):
  * the numpy restatement (tests/poly_rle_ref.py) against two yardsticks written apart from it -- tests/mask_train_ref.raster (the
    point-by-point trace for h = w = M) and the even-odd rule at pixel centres on polygons where the two must agree exactly -- and
    against run lists derived by hand;
  * libdetectorch_poly_hip.so exports exactly what include/detectorch_poly_hip.h declares and hip_poly.SIGNATURES binds it, parameter
    names and kinds in order; the header compiles as pedantic C99 and C++11; no other library exports a dtc_poly_ name; the constants
    of header, binding and source agree; the workspace size; the return codes on bad arguments, in the documented order (validation
    precedes every HIP call, so nothing is launched);
  * the Python layer: CPU tensors and polygons on a CPU device are refused, pack_polygons64 keeps doubles, pack_gt_segms with only
    host forms is pack_gt_masks, polys_to_boxes.
The first group pins the yardstick and passes whatever the library does; the others need the feature."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import mask_train_ref as mr
import poly_rle_ref as pr

sys.path.insert(0, GOLDEN)                                    # make_native_host_codes.exports


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)


# ---- the restatement against two independent yardsticks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [7, 14, 28, 56])
def test_square_images_equal_the_training_restatement(M):
    """h = w = M: the bitmap of every seeded polygon, and the OR over groups of three, is mask_train_ref.raster's"""
    polys = [p.astype(np.float64) for p in mr.seeded_polygons(M)]
    singles = [mr.raster(p, M) for p in polys]
    for p, want in zip(polys, singles):
        flat, events = pr.poly_bitmap(p, M, M)
        assert np.array_equal(flat.reshape(M, M).T, want.astype(bool)) and events == len(mr.trace_events(p, M))
    case = pr.make_case([[polys[k:k + 3] for k in range(0, 39, 3)]], [(M, M)])
    out = pr.run(case, 1 << 20, 1 << 20)
    for g in range(13):
        want = singles[3 * g] | singles[3 * g + 1] | singles[3 * g + 2]
        assert np.array_equal(out["bitmaps"][0][g], want.astype(bool)) and out["area"][0, g] == want.sum()
    assert sum(s.any() for s in singles) > 30


OFFSETS = ((0, 1), (0, 4), (1, 0), (4, 0))                    # sub-pixel offsets (of 5) of a polygon's lattice: see octilinear()


def octilinear(rs, h, w):
    """A closed polygon whose vertices lie on the 1/5 grid, none nearer than 0.3 to a pixel-centre line, and whose edges are
    horizontal, vertical or diagonal.  Every vertex is (a + ox / 5, b + oy / 5) with integers a, b >= 0 and one offset pair per polygon.
    On such edges the 5x trace is exact: a horizontal or vertical edge lies on a grid line, and on a diagonal the trace points are the
    edge's own grid points; the rule and the even-odd rule at pixel centres then differ only where an edge passes exactly through
    a pixel centre (touches_a_centre finds those)."""
    ox, oy = OFFSETS[rs.randint(len(OFFSETS))]
    x, y = rs.randint(-2, w + 2), rs.randint(-2, h + 2)
    pts = [(x, y)]
    for _ in range(rs.randint(2, 7)):
        dx, dy = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)][rs.randint(8)]
        n = rs.randint(1, max(h, w))
        x, y = x + n * dx, y + n * dy
        pts.append((x, y))
    ex, ey = pts[0][0] - x, pts[0][1] - y                       # close it: a diagonal, then an axis-parallel edge
    d = min(abs(ex), abs(ey))
    if d and max(abs(ex), abs(ey)) > d:
        pts.append((x + d * np.sign(ex), y + d * np.sign(ey)))
    ax, ay = min(0, min(a for a, _ in pts)), min(0, min(b for _, b in pts))      # no negative coordinate: trunc(5 x + 0.5) rounds those up
    return np.array([((5 * (a - ax) + ox) / 5.0, (5 * (b - ay) + oy) / 5.0) for a, b in pts], np.float64)


def touches_a_centre(p, h, w):
    """an edge of p passes exactly through a pixel centre of the h x w image: exact, in tenths of a pixel"""
    q = [(Fraction(round(x * 5), 5), Fraction(round(y * 5), 5)) for x, y in p]
    for (x0, y0), (x1, y1) in zip(q, q[1:] + q[:1]):
        for i in range(w):
            cx = Fraction(2 * i + 1, 2)
            if min(x0, x1) <= cx <= max(x0, x1) and x0 != x1:
                cy = y0 + (cx - x0) * (y1 - y0) / (x1 - x0)
                if (cy - Fraction(1, 2)).denominator == 1 and 0 <= cy <= h:
                    return True
    return False


def test_even_odd_rule_on_octilinear_polygons():
    """where the trace is exact the restatement is the even-odd rule at pixel centres, on h x w images of both orientations; at most
    5 % of the seeded polygons may be skipped as ambiguous (an edge through a pixel centre)"""
    rs = np.random.RandomState(20261106)
    skipped = compared = filled = 0
    for k in range(200):
        h, w = [(7, 5), (5, 7), (23, 31), (40, 17)][k % 4]
        p = octilinear(rs, h, w)
        assert np.array_equal(np.round(p * 5) / 5, p) and not np.isin(np.round(p * 5).astype(int) % 5, (2, 3)).any()
        if touches_a_centre(p, h, w):
            skipped += 1
            continue
        got = pr.poly_bitmap(p, h, w)[0].reshape(w, h).T
        assert np.array_equal(got, pr.even_odd_hw(p, h, w).astype(bool)), (k, p.tolist())
        compared += 1
        filled += bool(got.any())
    assert skipped <= 0.05 * 200 and compared + skipped == 200 and filled > 100


def test_even_odd_generalisation_is_the_training_checker_on_squares():
    for M in (7, 28):
        for p in mr.seeded_polygons(M)[:10]:
            assert np.array_equal(pr.even_odd_hw(p, M, M), mr.even_odd(p, M))


# ---- known answers, derived by hand -------------------------------------------------------------------------------------------------------------
def answer(polys, h, w):
    out = pr.run(pr.make_case([[polys]], [(h, w)]), 1 << 20, 1 << 20)
    return out["runs"][0][0], int(out["area"][0, 0]), out["need"][0, 0].tolist()


def test_known_answers():
    # 7 x 5 (h x w), the rectangle x 1 .. 3, y 2 .. 5: the pixels whose centres lie inside are columns 1, 2 and rows 2, 3, 4; column-major
    # position x * 7 + y: 9, 10, 11 and 16, 17, 18.  Four events (two column centre lines, top and bottom edge each), five runs.
    assert answer([rect(1, 2, 3, 5)], 7, 5) == ([9, 3, 4, 3, 16], 6, [4, 5])
    # 5 x 7, the rectangle x 2 .. 5, y 1 .. 3: columns 2, 3, 4 and rows 1, 2: positions 11, 12, 16, 17, 21, 22
    assert answer([rect(2, 1, 5, 3)], 5, 7) == ([11, 2, 3, 2, 3, 2, 12], 6, [6, 7])
    assert answer([rect(-9, -9, -2, -3)], 7, 5) == ([35], 0, [0, 1])                                 # wholly outside
    assert answer([rect(20, 2, 30, 4)], 7, 5) == ([35], 0, [0, 1])
    # covering the image and beyond: the top edge toggles the head of every column (5 events); the bottom edge's events fall on j = h,
    # the head of the next column, where they cancel the top edge's -- the last one is position h w and dropped
    assert answer([rect(-3, -3, 9, 9)], 7, 5) == ([0, 35], 35, [9, 2])
    # nested: the union has no hole (XOR would cut one)
    outer, inner = rect(1, 1, 6, 6), rect(2, 2, 5, 5)
    assert answer([outer, inner], 8, 8)[:2] == answer([outer], 8, 8)[:2] and answer([outer, inner], 8, 8)[2] == [16, 11]
    assert answer([outer], 8, 8)[0] == [9, 5, 3, 5, 3, 5, 3, 5, 3, 5, 18]
    # disjoint: pixel (0, 0), and columns 3, 4 x rows 5, 6 (positions 26, 27, 33, 34): the first run is 0, nothing behind the last one-run
    assert answer([rect(0, 0, 1, 1), rect(3, 5, 5, 7)], 7, 5) == ([0, 1, 25, 2, 5, 2], 5, [5, 6])
    # entered twice: the same mask as once, twice the events
    once, twice = answer([rect(1, 2, 3, 5)], 7, 5), answer([rect(1, 2, 3, 5), rect(1, 2, 3, 5)], 7, 5)
    assert twice[:2] == once[:2] and twice[2] == [8, 5]
    # the states of a row: past the count, no polygon, an invalid polygon only, a coordinate of 2^26, an image without pixels
    nan = rect(1, 2, 3, 5)
    nan[0, 0] = np.nan
    far = rect(1, 2, 3, 5)
    far[1, 0] = 2.0 ** 26
    case = pr.make_case([[[rect(1, 2, 3, 5)], [], [nan], [far], [rect(1, 2, 3, 5)[:2]], [rect(1, 2, 3, 5)]]] * 2, [(7, 5), (0.5, 5)], gt_counts=[5, 6])
    out = pr.run(case, 4, 3)
    assert out["n_runs"].tolist() == [[-1, 0, 0, 1, 0, 0], [0] * 6] and out["need"][0].tolist() == [[4, -1], [0, 0], [0, 0], [0, 1], [0, 0], [0, 0]]
    assert pr.run(case, 4, 4)["n_runs"][0, 0] == -1 and pr.run(case, 5, 4)["n_runs"][0, 0] == 5 and pr.run(case, 4, 4)["need"][0, 0].tolist() == [4, 5]
    assert pr.side(7.9) == 7 and pr.side(np.nan) == 0 and pr.side(0.99) == 0 and pr.side(1e12) == 1 << 30 and pr.pixels((1e6, 1e6)) == 1 << 30


def test_run_length_coding_is_result_utils():
    from detectorch_amd.utils import result_utils as ru
    rs = np.random.RandomState(2)
    for h, w in ((1, 1), (7, 5), (13, 9)):
        for m in (rs.rand(h, w) < 0.5, np.zeros((h, w), bool), np.ones((h, w), bool)):
            assert pr.runs_of(m.T.reshape(-1)) == ru.rle_counts(m)


# ---- the library: exports, binding, header, constants -----------------------------------------------------------------------------------
NAMES = ["dtc_poly_rle", "dtc_poly_rle_workspace_bytes", "dtc_poly_target_arch"]


def test_header_symbols_are_exported_and_bound():
    from make_native_host_codes import exports
    from test_binding_signatures_host import prototypes
    from detectorch_amd import hip_poly
    lib = hip_poly.lib()
    protos = prototypes("detectorch_poly_hip.h")
    assert sorted(protos) == NAMES and exports(hip_poly.LIB_PATH) == NAMES and sorted(hip_poly.SIGNATURES) == NAMES
    for entry, (ret, params) in protos.items():
        row = hip_poly.SIGNATURES[entry]
        assert row[0] == ret and [n for n, _ in row[1]] == [n for n, _ in params], entry
        assert [k for _, k in row[1]] == [k for _, k in params], entry
    assert lib.dtc_poly_target_arch() == b"gfx950"


def test_the_other_libraries_export_nothing_of_the_polygon_conversion():
    from make_native_host_codes import exports
    from detectorch_amd import build, hip, hip_eval, hip_grad, hip_loss, hip_mask, hip_optim, hip_rpn, hip_segm, hip_train
    build.build()
    for mod in (hip, hip_train, hip_loss, hip_grad, hip_optim, hip_rpn, hip_mask, hip_eval, hip_segm):
        if mod is not hip:
            mod.lib()
        assert not [n for n in exports(mod.LIB_PATH) if n.startswith("dtc_poly_")], mod.__name__


@pytest.mark.parametrize("compiler,flags", [("gcc", ["-std=c99"]), ("g++", ["-std=c++11"])])
def test_header_compiles_as_pedantic_c99_and_cxx11(tmp_path, compiler, flags):
    cc = shutil.which(compiler) or shutil.which({"gcc": "cc", "g++": "c++"}[compiler])
    assert cc, compiler + " not found"
    src = tmp_path / ("use_header" + {"gcc": ".c", "g++": ".cpp"}[compiler])
    src.write_text('#include "detectorch_poly_hip.h"\nint use(void) { return DTC_POLY_MAX_EVENTS + DTC_POLY_MAX_RUNS / DTC_POLY_MAX_GT; }\n')
    subprocess.check_call([cc] + flags + ["-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                                          str(tmp_path / "use_header.o")])


def test_constants_are_those_of_the_header_and_the_source():
    from detectorch_amd import hip_mask, hip_poly, hip_segm
    src = open(os.path.join(ROOT, "detectorch_amd", "csrc", "poly_rle", "poly_rle.hip")).read()
    header = open(os.path.join(ROOT, "include", "detectorch_poly_hip.h")).read()
    define = lambda name: eval(re.search(r"#define DTC_POLY_MAX_%s (\(?[\d <]+\)?)" % name, header).group(1))
    k = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert define("EVENTS") == hip_poly.MAX_EVENTS == k("kPolyMaxEvents") == pr.MAX_EVENTS >= 8192
    assert hip_poly.SORT_CAPACITIES == tuple(t * k("kPolyKeysPerThread") for t in (256, 512, 1024)) and hip_poly.SORT_CAPACITIES[-1] == hip_poly.MAX_EVENTS
    # two key buffers, the digit counters of every wavefront, the digit bases and 20 words of scratch fit what the entry asks of a CU's LDS
    assert 2 * 8 * hip_poly.MAX_EVENTS + (1024 // 64) * 256 * 4 + 256 * 4 + 20 * 4 <= 152 * 1024 < 160 * 1024
    assert (define("GT"), define("POLYS"), define("POINTS")) == (hip_poly.MAX_GT, hip_poly.MAX_POLYS, hip_poly.MAX_POINTS) == \
        (hip_mask.MAX_GT, hip_mask.MAX_POLYS, hip_mask.MAX_POINTS)
    assert (define("RUNS"), define("PIXELS")) == (hip_poly.MAX_RUNS, hip_poly.MAX_PIXELS) == (hip_segm.MAX_RUNS, hip_segm.MAX_PIXELS)
    assert define("BATCH") == hip_poly.MAX_BATCH == 65535 and pr.MAX_PIXELS == hip_poly.MAX_PIXELS


def test_workspace_bytes():
    from detectorch_amd import hip_poly
    f = hip_poly.lib().dtc_poly_rle_workspace_bytes
    ok = (3, 12, 500, 40, 2048)
    for at, bad in ((0, 0), (0, 65536), (1, -1), (1, 257), (2, -1), (2, 65537), (3, -1), (3, 4097), (4, 0), (4, 8193)):
        assert f(*[bad if i == at else v for i, v in enumerate(ok)]) == 0, (at, bad)
    base = f(*ok)
    assert base >= 3 * 12 * (2048 * 8 + 4) and base % 16 == 0 and f(3, 0, 0, 0, 1) > 0
    for at in range(5):                                         # monotone in every argument
        more = f(*[v + 1 if i == at else v for i, v in enumerate(ok)])
        assert more >= base and (more > base or at in (2, 3)), at
    assert f(65535, 256, 65536, 4096, 8192) > 1 << 39             # no 32-bit overflow


BOGUS = 256                                                                  # a bogus, non-NULL, 16-byte aligned device pointer
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -3, -4
ORDER = ("poly_xy", "poly_ptr", "gt_poly_ptr", "gt_counts", "im_size", "batch", "G", "PTS", "NP", "events_stride", "workspace",
         "workspace_bytes", "runs", "runs_stride", "n_runs", "area", "need")
INTS = dict(batch=3, G=12, PTS=500, NP=40, events_stride=2048, workspace_bytes=1 << 30, runs_stride=1024)
PTRS = tuple(k for k in ORDER if k not in INTS)
CODES = {
    "batch 0": (dict(batch=0), EINVAL), "G -1": (dict(G=-1), EINVAL), "PTS -1": (dict(PTS=-1), EINVAL), "NP -1": (dict(NP=-1), EINVAL),
    "events_stride 0": (dict(events_stride=0), EINVAL), "runs_stride 0": (dict(runs_stride=0), EINVAL),
    "G 257 + batch 0": (dict(G=257, batch=0), EINVAL), "events 8193 + runs_stride 0": (dict(events_stride=8193, runs_stride=0), EINVAL),
    "G 257": (dict(G=257), EUNSUPPORTED), "NP 4097": (dict(NP=4097), EUNSUPPORTED), "PTS 65537": (dict(PTS=65537), EUNSUPPORTED),
    "batch 65536": (dict(batch=65536), EUNSUPPORTED), "events_stride 8193": (dict(events_stride=8193), EUNSUPPORTED),
    "runs_stride 2^20 + 1": (dict(runs_stride=(1 << 20) + 1), EUNSUPPORTED), "G 257 + im_size NULL": (dict(G=257, im_size=None), EUNSUPPORTED),
    "NP 4097 + workspace 0": (dict(NP=4097, workspace_bytes=0), EUNSUPPORTED),
    **{k + " NULL": ({k: None}, EINVAL) for k in PTRS if k != "workspace"},
    "poly_xy misaligned": (dict(poly_xy=BOGUS + 4), EINVAL), "workspace misaligned": (dict(workspace=BOGUS + 8), EINVAL),
    "runs NULL + workspace 0": (dict(runs=None, workspace_bytes=0), EINVAL),
    "workspace NULL": (dict(workspace=None), EWORKSPACE), "workspace 0 bytes": (dict(workspace_bytes=0), EWORKSPACE),
    "workspace one byte short": (dict(workspace_bytes=-1), EWORKSPACE),
    # without gt rows there is nothing to write and nothing to launch: every pointer but im_size may be NULL
    "G 0": (dict(G=0), OK), "G 0, NULL pointers": (dict(G=0, poly_xy=None, poly_ptr=None, gt_poly_ptr=None, gt_counts=None, runs=None, n_runs=None,
                                                        area=None, need=None), OK),
    "G 0 + im_size NULL": (dict(G=0, im_size=None), EINVAL), "G 0 + workspace NULL": (dict(G=0, workspace=None), EWORKSPACE),
}


def _call(lib, kw):
    kw = dict(kw)
    n = dict(INTS, **{k: kw.pop(k) for k in list(kw) if k in INTS})
    ptr = {k: kw.pop(k, BOGUS) for k in PTRS}
    assert not kw
    return lib.dtc_poly_rle(*[(None if ptr[k] is None else C.c_void_p(ptr[k])) if k in ptr else n[k] for k in ORDER], None)


def test_return_codes_on_bad_arguments():
    """every row returns before the first launch: nothing is enqueued, the bogus pointers are never used"""
    from detectorch_amd import hip_poly
    lib = hip_poly.lib()
    need = lib.dtc_poly_rle_workspace_bytes(*[INTS[k] for k in ("batch", "G", "PTS", "NP", "events_stride")])
    assert 0 < need <= INTS["workspace_bytes"]
    CODES["workspace one byte short"] = (dict(workspace_bytes=need - 1), EWORKSPACE)
    got = {k: _call(lib, kw) for k, (kw, _) in CODES.items()}
    assert got == {k: v[1] for k, v in CODES.items()}
    assert len(CODES) >= 30


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_the_cpu_and_bad_arguments():
    import torch
    from detectorch_amd import hip_poly
    from detectorch_amd.utils import evaluator, segms
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    args = (z(1, 8, 2, dt=torch.float64), z(1, 3), z(1, 2), z(1), z(1, 2, dt=torch.float32))
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_poly.poly_rle(*args, 64, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        segms.polys_to_rle_batched(*args, 64, 64)
    tri = [[1.0, 1.0, 5.0, 1.0, 3.0, 6.0]]
    with pytest.raises(RuntimeError, match="GPU only"):
        segms.pack_gt_segms([[tri]], [(7, 5)], "cpu")
    with pytest.raises(ValueError, match="more than G"):
        segms.pack_polygons64([[tri, tri]], 1)
    with pytest.raises(ValueError, match="more than PTS"):
        segms.pack_polygons64([[tri]], 1, points=2)
    with pytest.raises(ValueError, match="nothing tells its size"):
        evaluator.evaluate_masks([[[]], [np.zeros((0, 5), np.float32)]], [[[]], [[]]], [dict(boxes=np.zeros((1, 4)), gt_classes=np.array([1]),
                                 is_crowd=np.array([0]), seg_areas=np.array([9.0]))], [[tri]])


def test_pack_polygons64_keeps_doubles():
    from detectorch_amd.utils import mask_rcnn_targets, segms
    polys = [[[[100.1, 37.3, 150.7, 40.9, 120.3, 90.1]], None, [[1.0, 2.0, 3.0, 4.0, 5.0, 7.0], [0.1, 0.2, 0.3, 0.4, 0.5, 0.7]]], [[]]]
    xy, ptr, gptr = segms.pack_polygons64(polys, 4)
    xy32, ptr32, gptr32 = mask_rcnn_targets.pack_polygons(polys, 4)
    assert xy.dtype.is_floating_point and xy.element_size() == 8 and xy[0, 0, 0].item() == 100.1 and xy[0, 0, 1].item() == 37.3
    assert xy32[0, 0, 0].item() != 100.1 and np.array_equal(xy.numpy().astype(np.float32), xy32.numpy())
    assert np.array_equal(ptr.numpy(), ptr32.numpy()) and np.array_equal(gptr.numpy(), gptr32.numpy())          # the layout is pack_polygons'
    assert ptr[0].tolist() == [0, 3, 6, 9] and gptr[0].tolist() == [0, 1, 1, 3, 3] and gptr[1].tolist() == [0, 0, 0, 0, 0]
    assert tuple(segms.pack_polygons64(polys, 4, points=20, polys=5)[0].shape) == (2, 20, 2)


def test_pack_gt_segms_of_host_forms_is_pack_gt_masks():
    from detectorch_amd.utils import result_utils as ru
    from detectorch_amd.utils import segms
    from detectorch_amd.utils.evaluator import pack_gt_masks
    rs = np.random.RandomState(3)
    a, b = rs.rand(7, 5) < 0.5, rs.rand(5, 7) < 0.5
    forms = lambda m: [m, m.astype(np.uint8), dict(size=list(m.shape), counts=ru.rle_counts(m)), ru.rle_encode(m), None]
    masks, sizes = [forms(a), forms(b)[:3]], [(7, 5), (5, 7)]
    for kw in ({}, dict(G=6, runs_stride=50)):
        got, want = segms.pack_gt_segms(masks, sizes, "cpu", **kw), pack_gt_masks(masks, sizes, "cpu", **kw)
        for k in ("gt_runs", "gt_n_runs"):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].numpy().tobytes() == want[k].numpy().tobytes()
        assert got["area"].numpy()[0, :5].tolist() == [a.sum()] * 4 + [0] and got["area"].numpy()[1, :3].tolist() == [b.sum()] * 3
        assert sorted(got) == ["area", "gt_n_runs", "gt_runs"] and not got["area"].numpy()[1, 3:].any()


def test_polys_to_boxes():
    from detectorch_amd.utils import segms
    polys = [[[10.5, 20.25, 30.0, 5.0, 12.0, 40.0]], [[1.0, 2.0, 3.0, 4.0, 5.0, 0.5], [9.0, -1.0, 2.0, 8.0, 4.0, 4.0]]]
    boxes = segms.polys_to_boxes(polys)
    assert boxes.dtype == np.float32 and boxes.tolist() == [[10.5, 5.0, 30.0, 40.0], [1.0, -1.0, 9.0, 8.0]]
    got = mr.poly_boxes([[np.asarray(p, np.float32).reshape(-1, 2) for p in ps] for ps in polys])
    assert np.array_equal(boxes, got)
