"""dtc_roi_align_backward on the GPU, off its default point: the cases of tests/roi_align_backward_limit_cases.py, launched the way
tests/test_hip_roi_align_backward.py launches its own (maps pre-filled with 0xFF bytes, 64 guard words behind each, a workspace of
0xFF bytes).  Every comparison is BITWISE: against the reference's own output where tests/golden/roi_align_backward_limits.npz
records it, and always against the numpy restatement that tests/test_roi_align_backward_limits_host.py holds to that fixture; a
case with bad rows also against the call without them.  Only `nonfinite_top` lets a NaN equal a NaN of another payload (the rule
and reason of tests/README_optim.md); the SET of NaN elements must be equal.  tests/README_roi_align_backward.md says what each
group is there for."""
import numpy as np
import pytest
import torch

from conftest import golden
import roi_align_backward_limit_cases as lc
import roi_align_backward_ref as rb
from test_hip_roi_align_backward import bits, check_restatement, dev, launch, outputs, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return golden("roi_align_backward_limits")


def same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", lc.CASES)
def test_limit_case(g, name):
    c = lc.case(name)
    got = run(c)
    want = lc.restatement(name)
    if name == "nonfinite_top":
        assert name not in lc.GOLDEN_CASES and np.isnan(want[0][0]).sum() == 10
        assert all(lc.same_bits_or_nan(got[l], want[l][0]) for l in range(len(c["shapes"])))
        return
    assert np.array_equal(rb.digest(c), g[name + "_digest"])
    ch = lc.sample_channels(name, c["top"].shape[1])
    for l in range(len(c["shapes"])):
        assert np.array_equal(bits(got[l][:, ch]), bits(g["%s_L%d" % (name, l)])), (name, l)       # the reference's own bits
    check_restatement(c, got, want)
    if c["bad_rows"]:                                # the bits of the call without those rows
        clean = run(lc.without_bad_rows(c))
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, clean))


def group_counts(c):
    bad = set(lc.bad_rows_by_rule(c))
    counts = np.zeros((len(c["shapes"]), c["batch"]), np.int64)
    for r in range(len(c["rois"])):
        if r not in bad:
            counts[c["levels"][r], int(c["rois"][r, 0])] += 1
    return counts


def rewritten_513():
    """groups_513 with rois and roi_levels changed so that EVERY group's count changes: a third of the rows moved one level up, 40 rows
    made bad, the group (level 2, image 1) emptied"""
    c = lc.case("groups_513")
    rois, levels = c["rois"].copy(), c["levels"].copy()
    rs = rb._rs(12, 20)
    moved = rs.choice(513, 171, replace=False)
    levels[moved] = (levels[moved] + 1) % 3
    for k, r in enumerate(rs.choice(513, 40, replace=False)):
        if k % 2:
            levels[r] = 3 + k
        else:
            rois[r, 1 + k % 4] = (np.nan, np.inf)[k // 2 % 2]
    empty = (levels == 2) & (rois[:, 0] == 1)
    levels[empty] = 0
    c2 = dict(c, rois=rois, levels=levels, top=np.ascontiguousarray(c["top"][::-1] * np.float32(0.5)))
    c2["bad_rows"] = lc.bad_rows_by_rule(c2)
    return c2


def test_replay_after_every_group_count_changed():
    c, c2 = lc.case("groups_513"), rewritten_513()
    before, after = group_counts(c), group_counts(c2)
    assert np.all(before != after) and after[2, 1] == 0 and before.min() > 0 and len(c2["bad_rows"]) >= 40
    top, rois, levels = dev(c["top"]), dev(c["rois"]), dev(c["levels"])
    eager, replayed = outputs(c), outputs(c)
    first = [r.clone() for r in launch(c, eager, top, rois, levels)]            # one eager call, then the capture
    torch.cuda.synchronize()
    check_restatement(c, [r.cpu().numpy() for r in first], lc.restatement("groups_513"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(c, replayed, top, rois, levels)
    graph.replay()
    torch.cuda.synchronize()
    assert same(first, replayed["grads"])
    top.copy_(dev(c2["top"])); rois.copy_(dev(c2["rois"])); levels.copy_(dev(c2["levels"]))
    for buf in replayed["raw"] + eager["raw"]:
        buf.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    second = launch(c2, eager, top, rois, levels)
    torch.cuda.synchronize()
    assert same(second, replayed["grads"]) and not same(first, second)
    for buf in replayed["raw"] + eager["raw"]:
        assert bool((buf[-64:] == -1).all())
    got = [r.cpu().numpy() for r in replayed["grads"]]
    check_restatement(c2, got)
    assert not got[2][1].any() and got[2][0].any()                              # the emptied group: +0.0 over the 0xFF


def test_workspace_left_by_a_larger_call():
    big, small = lc.case("groups_513"), lc.case("groups_257")
    out_big = outputs(big)
    launch(big, out_big)
    torch.cuda.synchronize()
    assert not bool((out_big["workspace"] == 0xFF).all())                       # the larger call left its lists there
    out = outputs(small)
    assert out["workspace"].numel() < out_big["workspace"].numel()
    used = dict(out, workspace=out_big["workspace"])                            # not refilled
    got = [r.cpu().numpy() for r in launch(small, used)]
    torch.cuda.synchronize()
    assert all(bool((buf[-64:] == -1).all()) for buf in out["raw"])
    fresh = run(small)                                                          # on a workspace of 0xFF bytes
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, fresh))
    check_restatement(small, got, lc.restatement("groups_257"))
