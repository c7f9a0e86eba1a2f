"""Host side of detections.hip, nms.hip, fpn.hip and bbox_ops.hip, without a GPU: the return code of every call of the table in
tests/golden/make_native_host_codes.py (calls that stop in argument validation -- each wrapper's own precondition, every
dtc_det_options / dtc_vote_scoring rejection, the shape limits, batch 0, a workspace one byte short, and pairs of simultaneous
faults that pin the ORDER of the checks), the exact value of the seven workspace-size functions over a grid of shapes and option
sets, and the set of exported dtc_* / launch_* symbols must equal tests/golden/native_host_codes.json, which was generated from the
library before the host bodies of these files were rebuilt on shared plan structs and helpers."""
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "native_host_codes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    """the record of the library in place, taken by the generator in a CHILD process that sees no device (the generator hides them
    before it loads the library): a call that slipped past validation comes back as a launch failure, which the generator refuses,
    instead of running a kernel on a bogus pointer where there is a GPU"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_native_host_codes.py"), "--stdout"], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return json.loads(out.stdout.decode())


def _table(rows):
    return {(r[0], r[1]): r[2] for r in rows}


def test_the_table_covers_what_it_should(want):
    codes, sizes = _table(want["codes"]), _table(want["sizes"])
    assert len(codes) == len(want["codes"]) > 600 and len(sizes) == len(want["sizes"]) > 1300
    assert {e for e, _ in codes} == {
        "dtc_postprocess_detections", "dtc_postprocess_detections_logits", "dtc_postprocess_detections_fpn",
        "dtc_box_results_nms_limit", "dtc_postprocess_detections_ex", "dtc_postprocess_detections_ex2", "dtc_nms", "dtc_nms_sorted",
        "dtc_segment_sort_desc", "dtc_soft_nms", "dtc_fpn_collect_distribute", "dtc_fpn_collect_distribute_kept", "dtc_bbox_overlaps",
        "dtc_box_voting", "dtc_box_voting_scored", "dtc_bbox_transform"}
    assert {f for f, _ in sizes} == {
        "dtc_postprocess_detections_workspace_bytes", "dtc_postprocess_detections_ex_workspace_bytes",
        "dtc_postprocess_detections_ex2_workspace_bytes", "dtc_nms_sorted_workspace_bytes", "dtc_nms_workspace_bytes",
        "dtc_prepare_proposals_workspace_bytes", "dtc_rpn_topk_decode_workspace_bytes"}
    assert -2 not in codes.values()                                  # DTC_ELAUNCH: a call that reached HIP has no place here
    # the order of the checks, on the parent: options before shapes, shapes before the fused mapping's row limit, that before
    # batch 0, batch 0 before the R limit, the R limit before the pointers, the pointers before the workspace
    ex = "dtc_postprocess_detections_ex"
    assert codes[ex, "opt nms_method 4 + R 4097"] == -1 and codes[ex, "opt nms_method 4 + batch 0"] == -1
    assert codes[ex, "fpn, max_out 513 + n_cls 258"] == -1 and codes[ex, "fpn, max_out 513 + batch 0"] == -4
    assert codes[ex, "batch 0 + R 4097"] == 0 and codes[ex, "batch 0 + every pointer NULL"] == 0
    assert codes[ex, "R 4097 + cls NULL"] == -4 and codes[ex, "dets NULL + workspace 0 bytes"] == -1
    assert codes[ex, "decoded + fpn + batch 0"] == -1 and codes["dtc_postprocess_detections_fpn", "fpn NULL + batch 0"] == -1
    assert codes["dtc_box_results_nms_limit", "boxes NULL + batch 0"] == -1
    assert codes["dtc_nms_sorted", "n_stride 16385, workspace 0 bytes"] == -3
    assert codes["dtc_nms_sorted", "n_stride 16385, workspace large"] == -4


def test_return_codes_equal_fixture(got, want):
    g, w = _table(got["codes"]), _table(want["codes"])
    assert sorted(g) == sorted(w)
    assert {k: (g[k], w[k]) for k in w if g[k] != w[k]} == {}


def test_workspace_sizes_equal_fixture(got, want):
    g, w = _table(got["sizes"]), _table(want["sizes"])
    assert sorted(g) == sorted(w)
    assert {k: (g[k], w[k]) for k in w if g[k] != w[k]} == {}


def test_exported_symbols_equal_fixture(got, want):
    """a stale or partial library (an entry lost, a helper leaked) shows up here"""
    assert got["exports"] == want["exports"] and len(want["exports"]) == 42
