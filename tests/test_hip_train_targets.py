"""dtc_fast_rcnn_targets on the MI355X: the Fast R-CNN training minibatch (assignment, crowd filter, sampling, labels, box targets,
expansion) against the reference's own chain (tests/golden/train_targets.npz) and its numpy restatement
(tests/train_targets_ref.py).  -m gpu.

Everything integer, max_overlaps, the rois, the weights, the target classes, dx and dy are compared bit for bit.  dw and dh: the
device may be at most e_ref + 2 float32 ulps from w * log(float64(ratio)) (e_ref: the reference's own largest distance from that
value, measured by the golden generator and stored in the fixture; + 1 ulp for the device logarithm, + 0.5 for the multiply, + 0.5
margin), and an exact 0 must be an exact 0.  The measured distance is printed before it is asserted."""
import numpy as np
import pytest
import torch

from conftest import golden
import train_limit_cases as tl
import train_targets_ref as tr

pytestmark = pytest.mark.gpu

EXPANDED = tl.EXPANDED


@pytest.fixture(scope="module")
def g():
    return golden("train_targets")


_want = {}


def want_of(case, params=None):
    """the restatement's result, computed once per (case, parameter set)"""
    p = tr.params_of(case) if params is None else params
    key = (case, tuple(sorted((k, str(v)) for k, v in p.items())))
    if key not in _want:
        _want[key] = tr.minibatch(tr.make_case(case), p)
    return _want[key]


def _batch(cases, G=None, P=None):
    """device inputs of a batch of cases, NaN / garbage past every count"""
    return tl.batch([tr.make_case(c) for c in cases], G, P)


_run, _host, _check = tl.run, tl.host, tl.check                              # shared with tests/test_hip_train_limits.py


@pytest.mark.parametrize("case", sorted(tr.CASES))
def test_case_equals_reference_and_restatement(g, case):
    params = tr.params_of(case)
    bound = float(g["e_ref"]) + 2.0
    o = _host(_run(_batch([case]), params))
    want = want_of(case)
    _check(o, 0, want, params, bound, case)
    if case not in tr.GOLDEN_CASES:
        return
    n = len(g[case + "_keep_inds"])                                          # ... and the reference's own arrays
    assert int(o["n_rois"][0]) == n and int(o["n_fg"][0]) == int(g[case + "_n_fg"])
    assert tr.same_bits(o["max_overlaps"][0], g[case + "_max_overlaps"]) and tr.same_bits(o["max_classes"][0], g[case + "_max_classes"])
    assert tr.same_bits(o["keep_inds"][0, :n], g[case + "_keep_inds"]) and tr.same_bits(o["labels"][0, :n], g[case + "_labels"])
    assert tr.same_bits(o["rois5"][0, :n], g[case + "_rois"])
    ref5 = g[case + "_targets5"][g[case + "_keep_inds"]]
    assert tr.same_bits(o["bbox_targets5"][0, :n, :3], ref5[:, :3])
    if case in tr.EXPANDED_CASES:
        for k in ("bbox_inside_weights", "bbox_outside_weights"):
            assert tr.same_bits(o[k][0, :n], g[case + "_" + k])
        assert np.array_equal(o["bbox_targets"][0, :n] != 0, g[case + "_bbox_targets"] != 0)


def test_batch_of_three_with_garbage_past_counts_and_stale_outputs(g):
    from detectorch_amd import hip_train
    params = tr.params_of("a")
    x = _batch(["a", "b", "c"], G=8, P=320)
    out = hip_train.targets_outputs(3, 328, hip_train.train_params(**params), "cuda", expanded=True, assignment=True)
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    o = _host(_run(x, params, out=out))
    for b, c in enumerate("abc"):
        _check(o, b, want_of(c, params), params, float(g["e_ref"]) + 2.0, "batch")
    assert int(o["n_rois"][1]) < 64 and int(o["n_rois"][0]) == 64            # padding rows present and checked above


def test_null_expanded_pointers_leave_compact_outputs_identical():
    params = tr.params_of("f")
    x = _batch(["f", "a"])
    full, lean = _host(_run(x, params)), _host(_run(x, params, expanded=False, assignment=False))
    assert all(lean[k] is None for k in EXPANDED + ("max_overlaps", "max_classes"))
    for k in ("rois5", "labels", "bbox_targets5", "keep_inds", "n_fg", "n_rois"):
        assert tr.same_bits(full[k], lean[k]), k


def test_graph_replay_follows_rewritten_inputs(g):
    params = tr.params_of("a")
    x = _batch(["a", "f"], G=8, P=320)
    out = _run(x, params)                                                    # one eager call, then the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run(x, params, out=out)
    torch.cuda.synchronize()
    y = _batch(["i", "b"], G=8, P=320)
    y["rand_keys"] = y["rand_keys"].flip(1).contiguous()                     # ... and another sampling order
    for k in x:
        x[k].copy_(y[k])
    graph.replay()
    o = _host(out)
    eager = _host(_run(y, params))
    for k in o:
        assert tr.same_bits(o[k], eager[k]), k
    for b, c in enumerate("ib"):                                             # the restatement on the rewritten inputs
        case = tr.make_case(c)
        nc = len(case["rand_keys"])
        case["rand_keys"] = y["rand_keys"][b, :nc].cpu().numpy().view(np.uint32)
        _check(o, b, tr.minibatch(case, params), params, float(g["e_ref"]) + 2.0, "replay")


def test_reference_shaped_call_equals_batched(g):
    from detectorch_amd.utils import fast_rcnn_sample_rois as fs
    case, params = tr.make_case("a"), tr.params_of("a")
    entry = dict(boxes=np.vstack([case["gt_boxes"], case["proposals"]]),
                 gt_classes=np.r_[case["gt_classes"], np.zeros(len(case["proposals"]), np.int32)],
                 is_crowd=np.r_[case["is_crowd"], np.zeros(len(case["proposals"]), np.int32)].astype(bool))
    blobs = fs.fast_rcnn_sample_rois(entry, case["im_scale"], 3, train_batch_size_per_image=64, rand_keys=case["rand_keys"])
    o = _host(_run(_batch(["a"]), params))
    n = int(o["n_rois"][0])
    assert sorted(blobs) == sorted(fs.BLOB_NAMES) and np.all(blobs["rois"][:, 0] == 3)
    assert tr.same_bits(blobs["rois"][:, 1:], o["rois5"][0, :n, 1:]) and tr.same_bits(blobs["labels_int32"], o["labels"][0, :n])
    for k in EXPANDED:
        assert tr.same_bits(blobs[k], o[k][0, :n]), k
    assert tr.same_bits(blobs["labels_int32"], g["a_labels"]) and tr.same_bits(blobs["rois"][:, 1:], g["a_rois"][:, 1:])
    # without keys the order is drawn on the device: a valid sample of the same sizes, the same for the same generator state
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    r1 = fs.fast_rcnn_sample_rois(entry, case["im_scale"], 0, train_batch_size_per_image=64, generator=gen)
    gen.manual_seed(5)
    r2 = fs.fast_rcnn_sample_rois(entry, case["im_scale"], 0, train_batch_size_per_image=64, generator=gen)
    assert all(tr.same_bits(r1[k], r2[k]) for k in r1) and r1["rois"].shape == (64, 5)
    assert int(np.sum(r1["labels_int32"] > 0)) == 16 and not tr.same_bits(r1["rois"], blobs["rois"])


def test_compact_equals_the_reference_concatenation(g):
    from detectorch_amd.utils import fast_rcnn_sample_rois as fs
    params = tr.params_of("a")
    x = _batch(["a", "b"])
    blobs = fs.sample_rois_batched(x["proposals"], x["proposal_counts"], x["gt_boxes"], x["gt_classes"], x["gt_is_crowd"],
                                   x["gt_counts"], x["im_scale"], rand_keys=x["rand_keys"], rois_per_image=64)
    assert sorted(blobs) == sorted(fs.BLOB_NAMES + ("bbox_targets5", "keep_inds", "n_fg", "n_rois"))
    assert blobs["rois"].shape == (2, 64, 5) and blobs["bbox_targets"].shape == (2, 64, 324)
    c = {k: v.cpu().numpy() for k, v in fs.compact(blobs).items()}
    rois_b = g["b_rois"].copy()
    rois_b[:, 0] = 1                                                         # the second image of the batch
    assert tr.same_bits(c["rois"], np.vstack([g["a_rois"], rois_b]))
    assert tr.same_bits(c["labels_int32"], np.r_[g["a_labels"], g["b_labels"]])
    for k in ("bbox_inside_weights", "bbox_outside_weights"):
        assert tr.same_bits(c[k], np.vstack([g["a_" + k], g["b_" + k]]))
    want = np.vstack([g["a_bbox_targets"], g["b_bbox_targets"]])
    assert c["bbox_targets"].shape == want.shape and np.array_equal(c["bbox_targets"] != 0, want != 0)
    wa, wb = want_of("a"), want_of("b", params)
    dxdy = np.zeros(want.shape, bool)
    dxdy[:, 0::4] = dxdy[:, 1::4] = True
    assert tr.same_bits(np.where(dxdy, c["bbox_targets"], 0), np.where(dxdy, want, 0))
    assert len(c["rois"]) == wa["n_rois"] + wb["n_rois"]
