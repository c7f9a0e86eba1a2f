"""The native calls of the hip.py / hip_train.py wrappers, without a GPU: every wrapper runs on CPU tensors against a recording
stand-in for the native libraries (tests/golden/make_hip_wrapper_calls.py), once per branch that changes the call, and every dtc_*
call -- entry point, order, each argument with pointers named by the wrapper argument or the buffer they belong to -- must equal
tests/golden/hip_wrapper_calls.json, which was generated before the wrappers were moved onto the by-name call helper."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN

WRAPPERS = ("bias_act", "roi_align", "roi_align_set_exact", "nms", "nms_sorted", "soft_nms", "generate_proposals",
            "fpn_collect_distribute", "prepare_proposals", "det_workspace_bytes", "postprocess_detections", "box_results_nms_limit",
            "mask_paste", "mask_rle", "bbox_overlaps", "box_voting", "bbox_transform", "prep_images", "fast_rcnn_targets")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_hip_wrapper_calls", os.path.join(GOLDEN, "make_hip_wrapper_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "hip_wrapper_calls.json")) as f:
        return json.load(f)


@pytest.fixture()
def got(monkeypatch):
    rec = _recorder()
    return json.loads(rec.dumps(rec.record(monkeypatch.setattr)))          # through JSON: tuples -> lists, as in the fixture


def test_same_cases_and_every_wrapper_covered(got, want):
    assert sorted(got) == sorted(want) and len(want) == 49
    assert sorted({case.split("/")[0] for case in want}) == sorted(WRAPPERS)


def test_calls_equal_fixture(got, want):
    for case in want:
        assert [c[0] for c in got[case]] == [c[0] for c in want[case]], case
        for cg, cw in zip(got[case], want[case]):
            assert cg == cw, (case, cw[0])


def test_stand_ins_are_restored():
    from detectorch_amd import hip, hip_train
    assert not type(hip._lib).__name__ == "WrapperLib" and not type(hip_train._lib).__name__ == "WrapperLib"
    assert hip.stream_ptr.__name__ == "stream_ptr" and hip._require_cuda.__name__ == "_require_cuda"
    assert isinstance(torch.cuda.device, type)
