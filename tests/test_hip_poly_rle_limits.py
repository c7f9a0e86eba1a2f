"""dtc_poly_rle on the MI355X past where tests/test_hip_poly_rle.py stops (-m gpu; the "Limits" section of tests/README_poly_rle.md):
the cases of tests/poly_rle_limit_cases.py against poly_rle_ref.run_sparse, which tests/test_poly_rle_limits_host.py holds to the
bitmap restatement.  No tolerance: n_runs, runs[:n_runs], area and need are equal.  Every output and the workspace are pre-filled
with 0xFF, and so are the points behind every image's own."""
import numpy as np
import pytest
import torch

import poly_rle_limit_cases as lc
from test_hip_poly_rle import check, filled

pytestmark = pytest.mark.gpu

_DEV = {}


def on_device(name):
    """the case's tensors, uploaded once; the padding of poly_xy is 0xFF bytes (a NaN no polygon owns)"""
    if name not in _DEV:
        case = lc.CASES[name][0]()
        xy = case["poly_xy"].copy()
        for n in range(len(xy)):
            xy[n, int(case["poly_ptr"][n].max()):].view(np.uint8)[...] = 0xFF
        arrays = dict(case, poly_xy=xy)
        _DEV[name] = {k: torch.from_numpy(np.array(arrays[k])).cuda() for k in ("poly_xy", "poly_ptr", "gt_poly_ptr", "gt_counts", "im_size")}
    return _DEV[name]


def launch(name, runs_stride, events_stride):
    from detectorch_amd import hip, hip_poly
    d = on_device(name)
    N, G = d["gt_poly_ptr"].shape[0], d["gt_poly_ptr"].shape[1] - 1
    out = filled(hip_poly.rle_outputs(N, G, runs_stride, "cuda"))
    ws = hip.workspace(hip_poly.rle_workspace_bytes(N, G, d["poly_xy"].shape[1], d["poly_ptr"].shape[1] - 1, events_stride), "cuda").fill_(0xFF)
    hip_poly.poly_rle(d["poly_xy"], d["poly_ptr"], d["gt_poly_ptr"], d["gt_counts"], d["im_size"], runs_stride, events_stride, out=out, ws=ws)
    return check(out, lc.expected(name, runs_stride, events_stride))


@pytest.mark.parametrize("name", [n for n in lc.CASES if n != "full_strides"])
def test_limit_case_equals_the_restatement(name):
    for runs_stride, events_stride in lc.CASES[name][1]:
        got = launch(name, runs_stride, events_stride)
        assert (got["n_runs"] > 0).any()


@pytest.mark.parametrize("runs_stride,events_stride", lc.CASES["full_strides"][1])
def test_full_strides(runs_stride, events_stride):
    """each capacity of the sorting node exactly met (the row is valid) and missed by one (-1, area 0, need = (events, -1))"""
    got = launch("full_strides", runs_stride, events_stride)
    for k, cap in enumerate(lc.SORT_CAPACITIES):
        fits = cap <= events_stride and cap + 1 <= runs_stride
        assert got["n_runs"][k, 1] == (cap + 1 if fits else -1) and got["need"][k, 1, 0] == cap and (got["n_runs"][k, [0, 2]] > 1).all()


def test_rows_past_the_clamped_counts_take_part_in_nothing():
    got = launch("max_shapes", 256, 2048)
    assert got["n_runs"][1, 255] == 0 and not got["n_runs"][3].any() and (got["n_runs"][2] > 1).all() and (got["n_runs"][0] > 1).all()
