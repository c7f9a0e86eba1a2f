"""The training-minibatch side without a GPU:
  * the numpy restatement (tests/train_targets_ref.py) against the reference's own chain (tests/golden/train_targets.npz, made by
    tests/golden/make_train_targets_golden.py): integers, rois, classes, dx and dy bit for bit, dw and dh within e_ref + 2 float32
    ulps of w * log(float64(ratio)) -- np.log is a float32 implementation of its own, so another numpy build may differ from the
    golden by as much as the reference differs from the yardstick;
  * libdetectorch_train_hip.so exports exactly what include/detectorch_train_hip.h declares, and hip_train binds all of it;
  * the return codes of dtc_fast_rcnn_targets on bad arguments, in the order shapes, batch 0, limits, pointers (validation precedes
    every HIP call, so these need no device: they are taken in a child process that sees none);
  * the inference library's export list is still the pinned one.
Run as a script with --codes the module prints the return-code table as JSON (the child process of the test)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden
import train_targets_ref as tr

sys.path.insert(0, GOLDEN)


@pytest.fixture(scope="module")
def g():
    return golden("train_targets")


def test_cases_are_the_engineered_ones(g):
    assert set(tr.GOLDEN_CASES) == set("abcdefgi") and float(g["e_ref"]) > 0
    a, pa = tr.make_case("a"), tr.params_of("a")
    assert len(a["gt_boxes"]) == 5 and int(a["is_crowd"].sum()) == 1 and len(a["proposals"]) == 300 and pa["rois_per_image"] == 64
    mo = g["a_max_overlaps"]
    assert np.sum(mo >= 0.5) > 16 and np.sum((mo < 0.5) & (mo >= 0)) > 48 and np.sum(mo[5:] == -1) > 0
    b = g["b_keep_inds"]
    assert int(g["b_n_fg"]) < 16 and len(b) - int(g["b_n_fg"]) < 48 and len(b) < 64            # short on both sides
    assert len(g["c_gt_boxes"]) == 0 and int(g["c_n_fg"]) == 0 and np.all(g["c_max_overlaps"] == 0)
    # d: only a crowd gt; proposal 0 (candidate 1) has IoU = IoA = 0.6: an fg label of the crowd's class, zero targets
    assert np.all(g["d_is_crowd"] == 1) and abs(float(g["d_max_overlaps"][1]) - 0.6) < 1e-2 and int(g["d_max_classes"][1]) == 17
    assert list(g["d_keep_inds"][:1]) == [1] and list(g["d_labels"][:1]) == [17] and not g["d_targets5"].any()
    assert np.sum(g["d_max_overlaps"][1:] == -1) >= 2
    # e: identical gt of classes 3 and 7 -> the first; IoU exactly 0.5 is fg and not bg; equal keys -> index order
    mo, mc = g["e_max_overlaps"], g["e_max_classes"]
    assert mo[3] == 1.0 and mc[3] == 3 and mo[4] == 0.5 and mo[5] == 0.5 and mc[4] == 3
    assert list(g["e_keep_inds"][:2]) == [0, 1] and list(g["e_labels"][:2]) == [3, 7]
    assert len(set(g["e_rand_keys"].tolist())) == 2
    # f: rows that are neither fg nor bg, and bg-labelled rows that carry targets
    mo = g["f_max_overlaps"]
    assert np.sum((mo >= 0.4) & (mo < 0.6)) > 0 and np.sum((mo >= 0) & (mo < 0.1)) > 0
    nf = int(g["f_n_fg"])
    assert np.any(g["f_bbox_inside_weights"][nf:] > 0) and np.all(g["f_labels"][nf:] == 0)
    assert len(g["g_keep_inds"]) == 512 and int(g["g_n_fg"]) == 128 and len(g["g_proposals"]) == 2000
    # i: class-agnostic targets: class 1, two regression classes
    assert g["i_bbox_targets"].shape[1] == 8 and set(np.unique(g["i_targets5"][:, 0])) == {0.0, 1.0}


@pytest.mark.parametrize("case", tr.GOLDEN_CASES)
def test_restatement_equals_reference(g, case):
    c = tr.make_case(case)
    for k in ("gt_boxes", "gt_classes", "is_crowd", "proposals", "rand_keys"):
        assert tr.same_bits(c[k], g[case + "_" + k]), k                       # the seeded inputs are reproducible
    assert c["im_scale"] == float(g[case + "_im_scale"])
    m = tr.minibatch(c, tr.params_of(case))
    assert tr.same_bits(m["max_overlaps"], g[case + "_max_overlaps"])
    assert tr.same_bits(m["max_classes"], g[case + "_max_classes"])
    assert tr.same_bits(m["keep_inds"], g[case + "_keep_inds"]) and m["n_fg"] == int(g[case + "_n_fg"])
    assert tr.same_bits(m["labels"], g[case + "_labels"])
    assert tr.same_bits(m["rois"], g[case + "_rois"])
    want5 = g[case + "_targets5"]
    assert tr.same_bits(m["targets5"][:, :3], want5[:, :3])                  # class, dx, dy
    bound = float(g["e_ref"]) + 2.0
    assert tr.ulps_from(m["targets5"][:, 3:], m["want64"]).max(initial=0.0) <= bound
    assert tr.ulps_from(want5[:, 3:], m["want64"]).max(initial=0.0) <= float(g["e_ref"])
    if case in tr.EXPANDED_CASES:
        bt, want = m["bbox_targets"], g[case + "_bbox_targets"]
        assert bt.shape == want.shape
        dwdh = np.zeros(bt.shape, bool)
        dwdh[:, 2::4] = dwdh[:, 3::4] = True
        assert tr.same_bits(np.where(dwdh, 0, bt), np.where(dwdh, 0, want))
        assert np.array_equal(bt != 0, want != 0)
        assert tr.same_bits(m["bbox_inside_weights"], g[case + "_bbox_inside_weights"])
        assert tr.same_bits(m["bbox_outside_weights"], g[case + "_bbox_outside_weights"])


def test_restatement_at_the_limits():
    c, p = tr.make_case("h"), tr.params_of("h")
    assert len(c["gt_boxes"]) == 256 and len(c["proposals"]) == 2048
    m = tr.minibatch(c, p)
    assert m["n_rois"] == 512 and m["n_fg"] == 128 and np.sum(m["max_overlaps"] == -1) > 4


# ---- the library: exports, binding, return codes ---------------------------------------------------------------------------------
def _declared():
    with open(os.path.join(ROOT, "include", "detectorch_train_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dtc_\w+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    from make_native_host_codes import exports
    from detectorch_amd import hip_train
    L = hip_train.lib()
    names = _declared()
    assert names == ["dtc_fast_rcnn_targets", "dtc_train_target_arch"]
    assert exports(hip_train.LIB_PATH) == names
    for n in names:
        f = getattr(L, n)
        assert f.argtypes is not None or f.restype is not C.c_int, n          # hip_train.lib() declared it
    assert L.dtc_train_target_arch() == b"gfx950"
    assert C.sizeof(hip_train.TrainParams) == 64


def test_inference_library_exports_unchanged():
    from make_native_host_codes import exports
    from detectorch_amd import hip
    with open(os.path.join(GOLDEN, "native_host_codes.json")) as f:
        want = json.load(f)["exports"]
    got = exports(hip.LIB_PATH)
    assert got == want and len(got) == 42 and not [n for n in got if "train" in n or "fast_rcnn" in n]


BOGUS = 256                                                                  # a bogus, non-NULL, 16-byte aligned device pointer
ARGS = ("gt_boxes", "gt_classes", "gt_is_crowd", "gt_counts", "proposals", "proposal_counts", "im_scale", "rand_keys")
OUTS = ("rois5", "labels", "bbox_targets5", "bbox_targets", "bbox_inside_weights", "bbox_outside_weights", "keep_inds", "n_fg",
        "n_rois", "max_overlaps", "max_classes")

# label -> (keyword overrides of _call, expected code).  -1 DTC_EINVAL, -4 DTC_EUNSUPPORTED, 0 DTC_OK
CODES = {
    "batch -1": (dict(batch=-1), -1), "G -1": (dict(G=-1), -1), "P -1": (dict(P=-1), -1), "G 0 and P 0": (dict(G=0, P=0), -1),
    "params NULL": (dict(params=None), -1), "R 0": (dict(rois_per_image=0), -1), "num_classes 1": (dict(num_classes=1), -1),
    "fg_thresh nan": (dict(fg_thresh=float("nan")), -1), "bg_hi above fg_thresh": (dict(bg_thresh_hi=0.6), -1),
    "fg_fraction 1.5": (dict(fg_fraction=1.5), -1), "reg weight inf": (dict(reg_weights=(10, 10, float("inf"), 5)), -1),
    # shapes before batch 0, batch 0 before limits and pointers
    "batch 0 + R 0": (dict(batch=0, rois_per_image=0), -1), "batch 0 + G 257": (dict(batch=0, G=257), 0),
    "batch 0 + every pointer NULL": (dict(batch=0, **{k: None for k in ARGS + OUTS}), 0),
    # limits before pointers
    "G 257": (dict(G=257), -4), "P 2049": (dict(P=2049), -4), "R 4097": (dict(rois_per_image=4097), -4),
    "G 257 + R 0": (dict(G=257, rois_per_image=0), -1), "P 2049 + rois5 NULL": (dict(P=2049, rois5=None), -4),
    # pointers
    **{k + " NULL": ({k: None}, -1) for k in ARGS + ("rois5", "labels", "bbox_targets5", "keep_inds", "n_fg", "n_rois")},
    "bbox_targets alone NULL": (dict(bbox_targets=None), -1), "outside weights alone NULL": (dict(bbox_outside_weights=None), -1),
    "max_overlaps without max_classes": (dict(max_classes=None), -1), "proposals misaligned": (dict(proposals=BOGUS + 4), -1),
    "bbox_targets misaligned": (dict(bbox_targets=BOGUS + 8), -1),
}


def _call(hip_train, batch=2, G=16, P=2000, params=True, **kw):
    ptr = {k: kw.pop(k, BOGUS) for k in ARGS + OUTS}
    prm = hip_train.train_params(**kw) if params else None
    v = lambda k: None if ptr[k] is None else C.c_void_p(ptr[k])
    return hip_train.lib().dtc_fast_rcnn_targets(*[v(k) for k in ARGS], batch, G, P, C.byref(prm) if prm is not None else None,
                                                 *[v(k) for k in OUTS], None)


def test_return_codes_on_bad_arguments():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--codes"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = json.loads(out.stdout.decode())
    assert got == {k: v[1] for k, v in CODES.items()}


if __name__ == "__main__" and "--codes" in sys.argv:
    from detectorch_amd import hip_train as ht
    print(json.dumps({k: _call(ht, **kw) for k, (kw, _) in CODES.items()}))
