"""RoIAlign backward without a GPU:
  * the numpy restatement (tests/roi_align_backward_ref.py) against the reference's own output on every recorded case, BIT FOR BIT
    (tests/golden/roi_align_backward.npz, made by tests/golden/make_roi_align_backward_golden.py from the reference's unmodified
    roi_align_backward_cpu.cpp), the inputs checked by digest;
  * what keeps the GPU tests from passing emptily, asserted on the cases themselves;
  * libdetectorch_grad_hip.so exports exactly what include/detectorch_grad_hip.h declares, hip_grad binds all of it under the
    header's parameter names in the header's order, and the other three libraries' export lists are the pinned ones;
  * the return codes on bad arguments (validation precedes every HIP call, so these need no device: they are taken in a child
    process that sees none) and the workspace size, monotone in its arguments;
  * the model wrappers raise on CPU tensors;
  * the tile / channel-block arithmetic restated in the cases module, tied to the source text.
Run as a script with --codes the module prints the return-code table as JSON (the child process of the test)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden
import roi_align_backward_ref as rb

sys.path.insert(0, GOLDEN)

HEADER = os.path.join(ROOT, "include", "detectorch_grad_hip.h")
SOURCE = os.path.join(ROOT, "detectorch_amd", "csrc", "grad", "roi_align_backward.hip")


@pytest.fixture(scope="module")
def g():
    return golden("roi_align_backward")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", rb.GOLDEN_CASES)
def test_restatement_equals_reference(g, case):
    c = rb.make_case(case)
    assert np.array_equal(rb.digest(c), g[case + "_digest"])
    ch = rb.sample_channels(case, c["top"].shape[1])
    assert (len(ch) == rb.SAMPLED_CHANNELS) == (case in rb.SAMPLED_CASES)
    for l, (r32, y64, mag) in enumerate(rb.reference(c, ch)):
        want = g["%s_L%d" % (case, l)]
        assert want.shape == r32.shape and np.array_equal(bits(r32), bits(want)), (case, l)
        # the float32 reference lies within its recorded e_ref of the float64 yardstick, a few roundings per term
        assert np.all(np.abs(r32.astype(np.float64) - y64) <= float(g[case + "_e_ref"]) * rb.EPS * mag * (1 + 1e-9))
    assert case == "fsmall" or float(g[case + "_e_ref"]) <= float(g["e_ref"]) < 4.0


def test_cases_are_the_engineered_ones():
    a = rb.make_case("a")
    assert a["top"].shape == (1, 1, 2, 2) and a["shapes"] == [(5, 7)] and a["ratio"] == 2
    assert rb.CHANNEL_WIDTHS == (1, 3, 64, 65, 256, 257) and rb.CH_BLOCK + 1 in rb.CHANNEL_WIDTHS
    b = rb.make_case("b65")
    assert b["top"].shape == (40, 65, 7, 7) and b["batch"] == 2 and b["shapes"] == [(13, 17)]
    assert rb.n_tiles(b["shapes"], 2) == 2 * 4 * 2                              # more than one tile in both directions
    c = rb.make_case("c")
    assert c["ratio"] == 0 and c["top"].shape[2:] == (14, 14)
    assert [rb.roi_geometry(r[1:], c["scales"][0], 14, 14, 0)[4:6] for r in c["rois"]] == c["grids"]
    assert {(1, 1), (5, 3)} <= set(c["grids"])
    # (d): samples in [-1, 0], collapsed taps on the last row and column, empty samples, forced 1 x 1 boxes
    d = rb.make_case("d")
    seen = set()
    for r in d["rois"]:
        sw, sh, bin_w, bin_h, gh, gw, _ = rb.roi_geometry(r[1:], 1.0, 7, 7, 2)
        seen |= {"forced"} if (r[3] <= r[1] or r[4] <= r[2]) and (bin_w == np.float32(1) / np.float32(7) or bin_h == np.float32(1) / np.float32(7)) else set()
        for p in range(7):
            for i in range(2):
                for start, binsz, extent in ((sh, bin_h, 13), (sw, bin_w, 17)):
                    v = np.float32(np.float32(start + np.float32(p) * binsz) + np.float32(np.float32(i + .5) * binsz) / np.float32(2))
                    ok, lo, hi, l, h = rb.axis(start, binsz, p, i, 2, extent)
                    seen |= {"empty"} if not ok else set()
                    seen |= {"clamped to 0"} if ok and -1 <= v <= 0 else set()
                    seen |= {"collapsed"} if ok and lo == hi == extent - 1 else set()
    assert seen == {"forced", "empty", "clamped to 0", "collapsed"}
    assert rb.TILE_EXTENTS_H == (1, 3, 4, 5, 9) and rb.TILE_EXTENTS_W == (1, 15, 16, 17, 33) and len(rb.TILE_CASES) == 25
    f = rb.make_case("fsmall")
    assert len(f["rois"]) == 300 and 0 < np.abs(f["top"]).max() < np.finfo(np.float32).tiny
    assert np.abs(rb.make_case("fbig")["top"]).max() > 1e30
    piled = rb.reference(rb.make_case("f"))[0][0]
    assert np.count_nonzero(piled) <= 2 * 36                                     # 300 RoIs on one neighbourhood of 9 x 9
    gc = rb.make_case("g")
    assert len(gc["shapes"]) == 4 and 2 not in gc["levels"] and not np.any((gc["levels"] == 3) & (gc["rois"][:, 0] == 1))
    assert {0, 1, 3} == set(gc["levels"].tolist()) and rb.make_case("g4")["rois"].shape[1] == 4
    h = rb.make_case("h")
    assert all(rb.is_bad(h["rois"][r], h["levels"][r], 2, 2) for r in h["bad_rows"]) and len(h["bad_rows"]) == 11
    kinds = h["rois"][h["bad_rows"]]
    assert np.isnan(kinds).any() and np.isinf(kinds).any() and (kinds[:, 0] == -1).any() and (kinds[:, 0] == 2).any()
    assert -1 in h["levels"] and 2 in h["levels"]
    i = rb.make_case("i")
    assert i["top"].shape == (512, 256, 7, 7) and i["shapes"] == [(50, 84)] and i["batch"] == 2


def test_bad_rois_rule():
    ok = [0, 1.0, 2.0, 30.0, 40.0]
    assert not rb.is_bad(ok, 0, 2, 1) and not rb.is_bad([-0.5] + ok[1:], 0, 2, 1) and not rb.is_bad([1.9] + ok[1:], 0, 2, 1)
    assert rb.is_bad([-1.0] + ok[1:], 0, 2, 1) and rb.is_bad([2.0] + ok[1:], 0, 2, 1) and rb.is_bad([np.nan] + ok[1:], 0, 2, 1)
    assert rb.is_bad(ok, -1, 2, 1) and rb.is_bad(ok, 1, 2, 1)
    for k in range(1, 5):
        for v in (np.nan, np.inf, -np.inf, 3e38, 2.0 ** 29):
            r = list(ok)
            r[k] = v
            assert rb.is_bad(r, 0, 2, 1, scale=1.0), (k, v)
    assert not rb.is_bad([0, 0, 0, 1e6, 1e6], 0, 2, 1, 1.0, (7, 7), 2) and not rb.is_bad([0, 0, 0, 2e5, 2e5], 0, 2, 1, 1.0, (7, 7), 0)
    assert rb.is_bad([0, 0, 0, 3e5, 10], 0, 2, 1, 1.0, (7, 7), 0)               # an adaptive grid above 32768


# ---- the library: exports, binding, return codes ---------------------------------------------------------------------------------
def _declared():
    """[(entry, [parameter names])] of include/detectorch_grad_hip.h, in its order"""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = []
    for name, params in re.findall(r"\b(dtc_\w+)\s*\(([^)]*)\)\s*;", text):
        names = [] if params.strip() == "void" else [re.findall(r"\w+", p)[-1] for p in params.split(",")]
        out.append((name, names))
    return out


def test_header_symbols_are_exported_and_bound():
    from make_native_host_codes import exports
    from detectorch_amd import hip_grad
    L = hip_grad.lib()
    decl = _declared()
    names = sorted(n for n, _ in decl)
    assert names == ["dtc_grad_target_arch", "dtc_roi_align_backward", "dtc_roi_align_backward_workspace_bytes"]
    assert exports(hip_grad.LIB_PATH) == names
    assert sorted(hip_grad.SIGNATURES) == names
    for n, params in decl:
        assert [p for p, _ in hip_grad.SIGNATURES[n][1]] == params, n          # the header's names in the header's order
        assert len(getattr(L, n).argtypes) == len(params)
    assert L.dtc_grad_target_arch() == b"gfx950"
    with open(HEADER) as f:
        text = f.read()
    macro = lambda m: int(re.search(r"#define %s (\d+)" % m, text).group(1))
    assert (macro("DTC_GRAD_MAX_POOLED"), macro("DTC_GRAD_MAX_SAMPLING"), macro("DTC_GRAD_MAX_ROIS"), macro("DTC_GRAD_MAX_BATCH"),
            macro("DTC_GRAD_MAX_EXTENT"), macro("DTC_GRAD_MAX_GRID")) == \
        (hip_grad.MAX_POOLED, hip_grad.MAX_SAMPLING, hip_grad.MAX_ROIS, hip_grad.MAX_BATCH, hip_grad.MAX_EXTENT, hip_grad.MAX_GRID) == \
        (1024, 1024, 1 << 24, 65536, 1 << 20, 32768)
    fields = re.search(r"typedef struct dtc_grad_level \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [n for n, _ in hip_grad.GradLevel._fields_]
    assert C.sizeof(hip_grad.GradLevel) == 24


def test_other_libraries_exports_unchanged():
    from make_native_host_codes import exports
    from detectorch_amd import hip, hip_loss, hip_train
    with open(os.path.join(GOLDEN, "native_host_codes.json")) as f:
        want = json.load(f)["exports"]
    got = exports(hip.LIB_PATH)
    assert got == want and len(got) == 42 and not [n for n in got if "backward" in n or "grad" in n]
    hip_train.lib()
    assert exports(hip_train.LIB_PATH) == ["dtc_fast_rcnn_targets", "dtc_train_target_arch"]
    hip_loss.lib()
    assert exports(hip_loss.LIB_PATH) == sorted(hip_loss.SIGNATURES) and len(hip_loss.SIGNATURES) == 5


def test_workspace_size_is_monotone_and_restated():
    from detectorch_amd import hip_grad
    ws = hip_grad.lib().dtc_roi_align_backward_workspace_bytes
    for levels in (1, 2, 4, 8):
        for batch in (1, 2, 3, 8, 65536):
            for rois in (0, 1, 2, 40, 512, 4096, 1 << 24):
                n = ws(levels, batch, rois)
                assert n == rb.workspace_bytes(levels, batch, rois) and n % 16 == 0 and n > 0
                assert ws(min(levels + 1, 8), batch, rois) >= n and ws(levels, min(batch + 1, 65536), rois) >= n
                assert ws(levels, batch, min(rois + 1, 1 << 24)) >= n
    assert ws(4, 8, 4096) == 4 * 8 * 8 + 4096 * 48                                 # bounded by R records, not R per tile
    for bad in ((0, 1, 1), (9, 1, 1), (1, 0, 1), (1, 65537, 1), (1, 1, -1), (1, 1, (1 << 24) + 1)):
        assert ws(*bad) == 0, bad


def test_tile_arithmetic_is_tied_to_the_source():
    with open(SOURCE) as f:
        text = f.read()
    const = lambda n: int(re.search(r"constexpr int %s = (\d+)" % n, text).group(1))
    th, tw = (int(v) for v in re.search(r"constexpr int kTileH = (\d+), kTileW = (\d+);", text).groups())
    assert (th, tw, const("kBwdThreads")) == (rb.TILE_H, rb.TILE_W, rb.CH_BLOCK) == (4, 16, 256)
    assert "kTilePitch = kBwdThreads + 1" in text and "sizeof(BwdRec) == %d" % rb.REC_BYTES in text
    assert rb.LDS_BYTES == 65792 and 2 * rb.LDS_BYTES <= 160 * 1024 < 3 * rb.LDS_BYTES   # two workgroups per CU
    assert "-ffp-contract=off" in open(os.path.join(ROOT, "detectorch_amd", "build.py")).read()
    assert "atomic" not in re.sub(r"//.*", "", text).lower() and "hipMemset" not in text
    # the flagship training shape: four levels of an 800 x 1333 batch of 8
    assert rb.n_tiles([(200, 336), (100, 168), (50, 84), (25, 42)], 8) == 8 * (50 * 21 + 25 * 11 + 13 * 6 + 7 * 3)
    assert rb.n_tiles([(1, 1)], 1) == 1 and rb.n_tiles([(4, 16)], 3) == 3 and rb.n_tiles([(5, 17)], 1) == 4


BOGUS = 256                                                                  # a bogus, non-NULL, 16-byte aligned device pointer

# label -> (keyword overrides of _call, expected code).  -1 DTC_EINVAL, -3 DTC_EWORKSPACE, -4 DTC_EUNSUPPORTED
CODES = {
    "levels NULL": (dict(levels=None), -1), "n_levels 0": (dict(n_levels=0), -1), "batch 0": (dict(batch=0), -1),
    "channels 0": (dict(channels=0), -1), "roi_cols 3": (dict(roi_cols=3), -1), "roi_cols 6": (dict(roi_cols=6), -1),
    "n_rois -1": (dict(n_rois=-1), -1), "pooled_h 0": (dict(pooled_h=0), -1), "pooled_w -2": (dict(pooled_w=-2), -1),
    "height 0": (dict(height=0), -1), "width -1": (dict(width=-1), -1), "scale nan": (dict(scale=float("nan")), -1),
    "scale inf": (dict(scale=float("inf")), -1),
    # shapes before limits, limits before pointers, pointers before the workspace
    "n_levels 9": (dict(n_levels=9), -4), "batch 65537": (dict(batch=65537), -4), "n_rois 2^24 + 1": (dict(n_rois=(1 << 24) + 1), -4),
    "pooled_h 1025": (dict(pooled_h=1025), -4), "pooled_w 1025": (dict(pooled_w=1025), -4), "ratio 1025": (dict(sampling_ratio=1025), -4),
    "channels 2^23 + 1": (dict(channels=(1 << 23) + 1), -4), "height 2^20 + 1": (dict(height=(1 << 20) + 1), -4),
    "too many tiles": (dict(height=1 << 20, width=1 << 20), -4),
    "n_levels 9 + pooled_h 0": (dict(n_levels=9, pooled_h=0), -1), "n_levels 9 + rois NULL": (dict(n_levels=9, rois=None), -4),
    "pooled_h 1025 + workspace NULL": (dict(pooled_h=1025, workspace=None), -4),
    "grad NULL": (dict(grad=None), -1), "grad misaligned": (dict(grad=BOGUS + 4), -1), "rois NULL": (dict(rois=None), -1),
    "grad_output NULL": (dict(grad_output=None), -1), "rois misaligned": (dict(rois=BOGUS + 2), -1),
    "roi_levels misaligned": (dict(roi_levels=BOGUS + 1), -1), "grad_output misaligned": (dict(grad_output=BOGUS + 2), -1),
    "workspace misaligned": (dict(workspace=BOGUS + 8), -1), "rois NULL + workspace NULL": (dict(rois=None, workspace=None), -1),
    "workspace NULL": (dict(workspace=None), -3), "workspace short": (dict(workspace_bytes=32 + 40 * 48 - 1), -3),
}


def _call(hg, n_levels=2, batch=2, channels=8, roi_cols=5, n_rois=40, pooled_h=7, pooled_w=7, sampling_ratio=2, height=13, width=17,
          scale=0.25, workspace_bytes=1 << 20, **kw):
    v = lambda k: None if kw.get(k, BOGUS) is None else C.c_void_p(kw.get(k, BOGUS))
    lv = (hg.GradLevel * 9)()
    for k in range(9):
        lv[k] = hg.GradLevel(kw.get("grad", BOGUS), height, width, scale, 0)
    return hg.lib().dtc_roi_align_backward(None if "levels" in kw else lv, n_levels, batch, channels, v("rois"), roi_cols, v("roi_levels"),
                                           n_rois, pooled_h, pooled_w, sampling_ratio, v("grad_output"), v("workspace"), workspace_bytes,
                                           None)


def test_return_codes_on_bad_arguments():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--codes"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert json.loads(out.stdout.decode()) == {k: v[1] for k, v in CODES.items()}


def test_model_wrappers_raise_on_cpu_tensors():
    from detectorch_amd import hip_grad
    from detectorch_amd.model.roi_align import RoIAlign, roi_align_fpn
    feats = torch.zeros(1, 4, 8, 8, requires_grad=True)
    rois = torch.zeros(2, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RoIAlign(7, 7, 0.25, 2)(feats, rois)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        roi_align_fpn([feats, torch.zeros(1, 4, 4, 4)], [0.25, 0.125], rois, torch.zeros(2, dtype=torch.int32), 7, 7, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_grad.roi_align_backward(torch.zeros(2, 4, 7, 7), rois, (1, 4, 8, 8), 0.25, 7, 7, 2)


if __name__ == "__main__" and "--codes" in sys.argv:
    from detectorch_amd import hip_grad as hg
    print(json.dumps({k: _call(hg, **kw) for k, (kw, _) in CODES.items()}))
