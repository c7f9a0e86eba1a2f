"""The head losses without a GPU:
  * the float64 restatement (tests/loss_ref.py) against the reference's own smooth_L1 / accuracy and torch's float64 cross_entropy
    with autograd gradients (tests/golden/loss.npz, made by tests/golden/make_loss_golden.py): to a few float64 roundings, far
    below e_ref, the float32 reference's own distance from those values, which the fixture stores per case;
  * the argmax over the logits (what the entry computes) against the argmax over the float32 softmax (loss.py:24): equal wherever
    the two largest logits of a row differ by at least 2^-10, on 100 000 rows;
  * libdetectorch_loss_hip.so exports exactly what include/detectorch_loss_hip.h declares, hip_loss binds all of it under the
    header's parameter names in the header's order, and the other two libraries' export lists are the pinned ones;
  * the return codes of both entries on bad arguments (validation precedes every HIP call, so these need no device: they are taken
    in a child process that sees none);
  * detectorch_amd.model.loss raises on CPU tensors.
Run as a script with --codes the module prints the return-code table as JSON (the child process of the test)."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden
import loss_ref as lr

sys.path.insert(0, GOLDEN)


@pytest.fixture(scope="module")
def g():
    return golden("loss")


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def test_cases_are_the_engineered_ones():
    shape = lambda n: lr.make_case(n)["cls_score"].shape
    assert shape("a") == (1, 81) and shape("b") == (65, 81) and shape("i4097") == (4097, 81) and shape("i65536") == (65536, 81)
    assert [lr.CASES[n][2] for n in ("c2", "c3", "c64", "c65", "c129", "c1024")] == [2, 3, 64, 65, 129, 1024]
    assert lr.make_case("c2")["bbox_pred"].shape == (33, 8)                                   # class-agnostic
    d = lr.make_case("d1e4")
    rows = np.arange(65)
    assert np.abs(d["cls_score"]).max() > 2e4 and np.all(d["cls_score"].max(axis=1) - d["cls_score"][rows, d["labels"]] > 1e4)
    for n, beta in (("e1", 1.0), ("e05", 0.5), ("e19", 1.0 / 9.0)):                         # x on, and on either side of, +-beta
        c = lr.make_case(n)
        k = c["targets5"][:, 0].astype(int)
        x = np.concatenate([c["bbox_pred"][r, 4 * k[r]:4 * k[r] + 4] - c["targets5"][r, 1:] for r in np.where(k > 0)[0]])
        b = np.float32(beta)
        assert c["beta"] == float(b)
        for v in (b, -b, 0.0, np.nextafter(b, np.float32(2)), np.nextafter(b, np.float32(0)), -np.nextafter(b, np.float32(2))):
            assert np.any(x == np.float32(v)), (n, v)
    b = lr.make_case("b")                                                    # a background row that carries targets
    assert np.any((b["labels"] == 0) & (b["targets5"][:, 0] > 0))
    i = lr.make_case("i4097")
    assert 0.2 < np.mean(i["labels"] < 0) < 0.3 and not i["targets5"][i["labels"] < 0].any()
    s = lr.make_smooth_case("s7")
    assert s["pred"].size % 4 == 3 and set(np.unique(s["alpha_out"])) == {0.0, 0.25, 2.0} and np.all(s["alpha_in"] != 1.0)


@pytest.mark.parametrize("case", lr.GOLDEN_CASES)
def test_restatement_equals_reference(g, case):
    c = lr.make_case(case)
    assert np.array_equal(_digest(c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"]), g[case + "_digest"])
    y = lr.head(c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"], c["beta"])
    nv = int(g[case + "_n_valid"])
    assert y["n_valid"] == nv and round(float(y["accuracy"]) * nv) == round(float(g[case + "_accuracy"]) * nv)     # the same hits
    top = float(np.abs(c["cls_score"]).max())
    # float64 against float64: sums of <= 65536 * 1024 terms in another order
    assert abs(float(y["loss_cls"]) - float(g[case + "_loss_cls"])) <= 1e-12 * max(top, float(g[case + "_loss_cls"]))
    assert abs(float(y["loss_bbox"]) - float(g[case + "_loss_bbox"])) <= 1e-12 * float(g[case + "_loss_bbox"])
    if case not in ("a",):                                                   # (one row: a sum of one term)
        assert float(g[case + "_e_ref_cls"]) > 1e-12 * max(top, float(g[case + "_loss_cls"]))   # e_ref is far above that
    rows = lr.sample_rows(case, len(c["labels"])) if case in lr.SAMPLED_CASES else np.arange(len(c["labels"]))
    assert np.abs(y["grad_cls"][rows] - g[case + "_grad_cls"]).max() <= 1e-13 / nv
    k = c["targets5"][:, 0].astype(int)
    k = np.where(k > 0, 1 if c["bbox_pred"].shape[1] == 8 else k, 0)
    sel = np.take_along_axis(y["grad_box"], 4 * k[:, None] + np.arange(4)[None, :], 1) * (k[:, None] > 0)
    want = g[case + "_grad_box4"]
    assert np.abs(sel[rows] - want).max() <= 1e-13 * np.abs(want).max()
    assert np.count_nonzero(y["grad_box"]) == np.count_nonzero(sel)          # nothing outside the selected columns
    assert not y["grad_cls"][c["labels"] < 0].any() and not y["grad_box"][c["labels"] < 0].any()


@pytest.mark.parametrize("case", sorted(lr.SMOOTH_CASES))
def test_smooth_l1_restatement_equals_reference(g, case):
    c = lr.make_smooth_case(case)
    assert np.array_equal(_digest(c["pred"], c["targets"], c["alpha_in"], c["alpha_out"]), g[case + "_digest"])
    loss, grad = lr.smooth_l1(c["pred"], c["targets"], c["alpha_in"], c["alpha_out"], c["beta"])
    assert abs(float(loss) - float(g[case + "_loss"])) <= 1e-12 * float(g[case + "_loss"]) < float(g[case + "_e_ref"])
    assert np.abs(grad - g[case + "_grad"]).max() <= 1e-13 * np.abs(grad).max()
    x = (c["pred"].astype(np.float64) - c["targets"]) * c["alpha_in"]
    assert np.sum(np.abs(x) == c["beta"]) >= 2 and np.sum(x == 0) >= 1       # the edges are in


def test_exact_ties_take_the_lowest_index():
    x = np.zeros((4, 7), np.float32)
    x[1, [2, 5]] = 3.0
    x[2, 6] = 1.0
    x[3] = -2.5
    assert list(lr.argmax_logits(x)) == [0, 2, 6, 0]
    y = lr.head(x, np.array([0, 5, 6, 1], np.int32))
    assert float(y["accuracy"]) == 0.5


def test_argmax_over_logits_is_the_reference_argmax_where_the_gap_is_wide():
    """loss.py:24 takes the argmax over softmax(cls_score) in float32; the entry takes it over the logits.  Wherever the two largest
    logits differ by >= 2^-10 the two agree: 100 000 rows, logit scales 1 .. 1e4, the reference's torch expression on the CPU."""
    rs = np.random.RandomState(5)
    x = (rs.standard_normal((100000, 81)) * rs.choice([1.0, 10.0, 100.0, 1e4], (100000, 1))).astype(np.float32)
    x[::7, 3] = x[::7].max(axis=1) + np.float32(2.0 ** -10)                  # rows whose gap is the narrowest admitted
    top2 = np.sort(x, axis=1)[:, -2:]
    wide = (top2[:, 1] - top2[:, 0]) >= 2.0 ** -10
    assert wide.sum() > 90000
    t = torch.from_numpy(x)
    ref = torch.max(torch.nn.functional.softmax(t, dim=1), 1)[1].numpy()
    assert np.array_equal(ref[wide], lr.argmax_logits(x)[wide])
    assert np.array_equal(lr.argmax_softmax(x)[wide], ref[wide])


# ---- the library: exports, binding, return codes ---------------------------------------------------------------------------------
def _declared():
    """[(entry, [parameter names])] of include/detectorch_loss_hip.h, in its order"""
    with open(os.path.join(ROOT, "include", "detectorch_loss_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = []
    for name, params in re.findall(r"\b(dtc_\w+)\s*\(([^)]*)\)\s*;", text):
        names = [] if params.strip() == "void" else [re.findall(r"\w+", p)[-1] for p in params.split(",")]
        out.append((name, names))
    return out


def test_header_symbols_are_exported_and_bound():
    from make_native_host_codes import exports
    from detectorch_amd import hip_loss
    L = hip_loss.lib()
    decl = _declared()
    names = sorted(n for n, _ in decl)
    assert names == ["dtc_fast_rcnn_loss", "dtc_fast_rcnn_loss_workspace_bytes", "dtc_loss_target_arch", "dtc_smooth_l1",
                     "dtc_smooth_l1_workspace_bytes"]
    assert exports(hip_loss.LIB_PATH) == names
    assert sorted(hip_loss.SIGNATURES) == names
    for n, params in decl:
        assert [p for p, _ in hip_loss.SIGNATURES[n][1]] == params, n        # the header's names in the header's order
        f = getattr(L, n)
        assert len(f.argtypes) == len(params)
    assert L.dtc_loss_target_arch() == b"gfx950"
    with open(os.path.join(ROOT, "include", "detectorch_loss_hip.h")) as f:
        text = f.read()
    macro = lambda m: int(re.search(r"#define %s (\d+)" % m, text).group(1))
    assert (macro("DTC_LOSS_MAX_CLASSES"), macro("DTC_LOSS_MAX_ROWS"), macro("DTC_LOSS_MAX_ELEMS")) == \
        (hip_loss.MAX_CLASSES, hip_loss.MAX_ROWS, hip_loss.MAX_ELEMS) == (1024, 65536, 1 << 30)
    assert L.dtc_fast_rcnn_loss_workspace_bytes(65536, 1024) == L.dtc_fast_rcnn_loss_workspace_bytes(1, 2) > 0
    assert L.dtc_fast_rcnn_loss_workspace_bytes(65537, 81) == 0 and L.dtc_fast_rcnn_loss_workspace_bytes(8, 1025) == 0
    assert L.dtc_smooth_l1_workspace_bytes(33, 7) > 0 and L.dtc_smooth_l1_workspace_bytes(1 << 20, 1025) == 0


def test_other_libraries_exports_unchanged():
    from make_native_host_codes import exports
    from detectorch_amd import hip, hip_train
    with open(os.path.join(GOLDEN, "native_host_codes.json")) as f:
        want = json.load(f)["exports"]
    got = exports(hip.LIB_PATH)
    assert got == want and len(got) == 42 and not [n for n in got if "loss" in n or "smooth" in n]
    hip_train.lib()
    assert exports(hip_train.LIB_PATH) == ["dtc_fast_rcnn_targets", "dtc_train_target_arch"]


BOGUS = 256                                                                  # a bogus, non-NULL, 16-byte aligned device pointer
HEAD_PTRS = ("cls_score", "labels", "bbox_pred", "bbox_targets5", "upstream", "workspace", "losses", "grad_cls_score", "grad_bbox_pred")
SL1_PTRS = ("pred", "targets", "alpha_in", "alpha_out", "upstream", "workspace", "loss", "grad_pred")

# label -> (keyword overrides of _head / _sl1, expected code).  -1 DTC_EINVAL, -3 DTC_EWORKSPACE, -4 DTC_EUNSUPPORTED
HEAD_CODES = {
    "n 0": (dict(n=0), -1), "c 1": (dict(c=1), -1), "beta 0": (dict(beta=0.0), -1), "beta -1": (dict(beta=-1.0), -1),
    "beta nan": (dict(beta=float("nan")), -1), "beta inf": (dict(beta=float("inf")), -1),
    "width neither 4c nor 8": (dict(bbox_width=320), -1),
    # shapes before limits, limits before pointers
    "c 1025": (dict(c=1025, bbox_width=4100), -4), "n 65537": (dict(n=65537), -4), "c 1025 + beta 0": (dict(c=1025, beta=0.0), -1),
    "n 65537 + cls_score NULL": (dict(n=65537, cls_score=None), -4),
    "cls_score NULL": (dict(cls_score=None), -1), "labels NULL": (dict(labels=None), -1),
    "bbox_pred without targets": (dict(bbox_targets5=None), -1), "targets without bbox_pred": (dict(bbox_pred=None), -1),
    "both output groups NULL": (dict(losses=None, grad_cls_score=None, grad_bbox_pred=None), -1),
    "grad_cls_score alone": (dict(grad_bbox_pred=None), -1), "grad_bbox_pred alone": (dict(grad_cls_score=None), -1),
    "grad_bbox_pred without box inputs": (dict(bbox_pred=None, bbox_targets5=None), -1),
    "bbox_pred misaligned": (dict(bbox_pred=BOGUS + 4), -1), "grad_bbox_pred misaligned": (dict(grad_bbox_pred=BOGUS + 8), -1),
    "workspace misaligned": (dict(workspace=BOGUS + 8), -1),
    "workspace NULL": (dict(workspace=None), -3), "workspace short": (dict(workspace_bytes=1024), -3),
}
SL1_CODES = {
    "n 0": (dict(n=0), -1), "w 0": (dict(w=0), -1), "beta 0": (dict(beta=0.0), -1), "beta nan": (dict(beta=float("nan")), -1),
    "beta -inf": (dict(beta=float("-inf")), -1),
    "n * w past the limit": (dict(n=1 << 20, w=1025), -4), "past the limit + pred NULL": (dict(n=1 << 20, w=1025, pred=None), -4),
    "past the limit + beta 0": (dict(n=1 << 20, w=1025, beta=0.0), -1),
    **{k + " NULL": ({k: None}, -1) for k in ("pred", "targets", "alpha_in", "alpha_out")},
    "loss and grad_pred NULL": (dict(loss=None, grad_pred=None), -1),
    "pred misaligned": (dict(pred=BOGUS + 4), -1), "alpha_out misaligned": (dict(alpha_out=BOGUS + 8), -1),
    "grad_pred misaligned": (dict(grad_pred=BOGUS + 4), -1), "workspace misaligned": (dict(workspace=BOGUS + 4), -1),
    "loss without workspace": (dict(workspace=None), -3), "workspace short": (dict(workspace_bytes=64), -3),
}


def _head(hl, n=64, c=81, bbox_width=324, beta=1.0, workspace_bytes=1 << 20, **kw):
    v = lambda k: None if kw.get(k, BOGUS) is None else C.c_void_p(kw.get(k, BOGUS))
    return hl.lib().dtc_fast_rcnn_loss(v("cls_score"), v("labels"), v("bbox_pred"), v("bbox_targets5"), n, c, bbox_width, beta,
                                       v("upstream"), v("workspace"), workspace_bytes, v("losses"), v("grad_cls_score"),
                                       v("grad_bbox_pred"), None)


def _sl1(hl, n=64, w=324, beta=1.0, workspace_bytes=1 << 20, **kw):
    v = lambda k: None if kw.get(k, BOGUS) is None else C.c_void_p(kw.get(k, BOGUS))
    return hl.lib().dtc_smooth_l1(v("pred"), v("targets"), v("alpha_in"), v("alpha_out"), n, w, beta, v("upstream"), v("workspace"),
                                  workspace_bytes, v("loss"), v("grad_pred"), None)


def test_return_codes_on_bad_arguments():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--codes"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = json.loads(out.stdout.decode())
    assert got == {"head": {k: v[1] for k, v in HEAD_CODES.items()}, "smooth_l1": {k: v[1] for k, v in SL1_CODES.items()}}


def test_model_loss_raises_on_cpu_tensors():
    from detectorch_amd.model import loss
    x, labels = torch.zeros(4, 81), torch.zeros(4, dtype=torch.int64)
    p = torch.zeros(4, 324)
    blobs = dict(labels_int32=torch.zeros(1, 4, dtype=torch.int32), bbox_targets5=torch.zeros(1, 4, 5))
    for call in (lambda: loss.smooth_L1(p, p, p, p), lambda: loss.accuracy(x, labels), lambda: loss.cross_entropy(x, labels),
                 lambda: loss.fast_rcnn_losses(x, p, blobs), lambda: loss.fast_rcnn_losses_fused(x, p, blobs)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


if __name__ == "__main__" and "--codes" in sys.argv:
    from detectorch_amd import hip_loss as hl
    print(json.dumps({"head": {k: _head(hl, **kw) for k, (kw, _) in HEAD_CODES.items()},
                      "smooth_l1": {k: _sl1(hl, **kw) for k, (kw, _) in SL1_CODES.items()}}))
