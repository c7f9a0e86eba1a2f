"""dtc_mask_targets and dtc_mask_loss on the GPU past the sizes of their first tests (cases: tests/mask_train_limit_cases.py; what
each one reaches is asserted on the CPU by tests/test_mask_train_limits_host.py and listed in tests/README_mask_train.md).  Targets:
every integer and mask_rois bit for bit against the numpy restatement, computed once per case.  Loss: the float64 yardstick
mask_train_ref.loss64 with the bounds of tests/README_loss.md -- loss max(4 e_ref, 32 eps max(|y|, max |x|)), gradient 16 eps
|upstream| / n_valid absolute, n_valid and every promised +0.0 exact --, every distance printed in units of its bound.  The helpers
are those of tests/test_hip_mask_targets.py and tests/test_hip_mask_loss.py: every output and the workspace start as 0xFF, guard
words sit behind every output."""
import numpy as np
import pytest

from conftest import golden
import mask_train_limit_cases as lc
import mask_train_ref as mr
from test_hip_mask_loss import call, compare
from test_hip_mask_targets import OUTS, check, run, snap, upload

pytestmark = pytest.mark.gpu

SINGLE = sorted(n for n in lc.TARGETS if not n.startswith("all_m"))


@pytest.fixture(scope="module")
def g():
    return golden("mask_train_limits")


def loss_inputs(case, extremes=False):
    """the shared, read-only arrays of a loss case as writable copies for the upload"""
    return {k: v.copy() for k, v in lc.loss_case(case, extremes).items()}


def same_as_restatement(got, b, want, batch_index=None):
    """image b of a call's outputs against the restatement of that image alone (its own R rows; batch index 0)"""
    n, R = int(want["n_mask"]), len(want["roi_has_mask"])
    for k in OUTS:
        w, q = np.asarray(want[k]), got[k][b]
        if k == "roi_has_mask":                                                  # rows past the image's own are padding: 0
            assert not q[R:].any()
            q = q[:R]
        if k == "mask_rois" and batch_index:
            w = w.copy()
            w[:n, 0] = batch_index
        assert w.dtype == q.dtype and w.shape == q.shape, k
        assert w.tobytes() == q.tobytes(), (k, b, np.argwhere(w != q)[:5].tolist())


# ---- targets ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SINGLE)
def test_targets_case_against_restatement(case):
    img, M, k_min, k_max, Fm = lc.case(case)
    batch, _ = mr.stack([img], Fm)
    out, arenas = run(upload(batch), M, k_min, k_max, Fm)
    got = snap(out, arenas)
    same_as_restatement(got, 0, lc.want(case))
    assert set(np.unique(got["masks"]).tolist()) <= {-1, 0, 1}


def test_targets_at_every_m():
    """M = 1 .. 56 on one image, one call per M: every chunk size of the parity scan from 1 to 13, M * M = 256 exactly, idle tail
    threads, short last chunks"""
    batch, _ = mr.stack([lc.all_m()], 4)
    dev = upload(batch)
    for M in lc.ALL_M:
        _, _, k_min, k_max, Fm = lc.case("all_m%d" % M)
        out, arenas = run(dev, M, k_min, k_max, Fm)
        same_as_restatement(snap(out, arenas), 0, lc.want("all_m%d" % M))


def test_targets_batch_of_two_large_images():
    """rows700_fm512 and rows4096 stacked, Fm = 512: blockIdx.y together with 512 raster workgroups per image; each image equals its
    restatement and its own B = 1 call on the same padded rows, apart from the batch index column"""
    (a, M, k_min, k_max, Fm), (b, _, _, _, _) = (lc.case(n) for n in lc.BATCH2)
    batch, padded = mr.stack([a, b], Fm)
    out, arenas = run(upload(batch), M, k_min, k_max, Fm)
    got = snap(out, arenas)
    check(got, padded, M, k_min, k_max, Fm)                                      # the restatement of the padded images
    for i, name in enumerate(lc.BATCH2):
        same_as_restatement(got, i, lc.want(name), batch_index=i)
        o1, a1 = run(upload({k: v[i:i + 1] for k, v in batch.items()}), M, k_min, k_max, Fm)
        g1 = snap(o1, a1)
        for k in OUTS:
            w = got[k][i].copy()
            if k == "mask_rois":
                w[:int(got["n_mask"][i]), 0] = 0                                 # the batch index of a one-image call is 0
            assert w.tobytes() == g1[k][0].tobytes(), (k, i)


# ---- loss -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(lc.LOSS))
def test_loss_case_against_yardstick(g, case):
    c, y = loss_inputs(case), lc.loss_want(case)
    e_ref = float(g["loss_" + case + "_e_ref"])
    got = call(c)
    compare(case, got, y, e_ref=e_ref)
    compare(case + " (ref)", dict(got, grad=None), y, e_ref=e_ref, want_loss=float(g["loss_" + case]))
    keep = lc.grad_sample(case)                                                  # the reference's own float64 gradient, sampled
    assert np.max(np.abs(got["grad"].ravel()[keep].astype(np.float64) - g["loss_" + case + "_grad"])) <= mr.loss_bounds(y)["grad"]
    assert call(c, grad=False)["loss"].tobytes() == got["loss"].tobytes()        # loss-only: the fused call's bits


@pytest.mark.parametrize("case", lc.MULTI_ROW)
def test_loss_extreme_rows_that_share_a_workgroup(g, case):
    """the EXTREMES logits on rows that share a workgroup with class -1, class K and all-padding rows, in both orders"""
    c, y = loss_inputs(case, True), lc.loss_want(case, True)
    got = call(c)
    assert np.isfinite(got["loss"]) and np.isfinite(got["grad"]).all()
    compare(case + "_x", got, y, e_ref=float(g["loss_" + case + "_x_e_ref"]))
    compare(case + "_x (ref)", dict(got, grad=None), y, want_loss=float(g["loss_" + case + "_x"]))
    assert call(c, grad=False)["loss"].tobytes() == got["loss"].tobytes()


@pytest.mark.parametrize("case", ("r3077m7k3", "r1025m7k2"))
def test_loss_gradient_off_a_16_byte_boundary_on_the_stride_path(case):
    """the gradient 1, 2 and 3 words past a 16-byte boundary, where a workgroup's second and later rows have their own heads and
    tails: the bits of the aligned call, guard words untouched (`call` checks them)"""
    c = loss_inputs(case, True)
    want = call(c)
    compare(case + " aligned", want, lc.loss_want(case, True))
    for offset in (1, 2, 3):
        got = call(c, offset=offset)
        assert got["loss"].tobytes() == want["loss"].tobytes() and got["n_valid"] == want["n_valid"], offset
        assert got["grad"].tobytes() == want["grad"].tobytes(), offset


def test_loss_upstream_on_the_stride_path():
    c = loss_inputs("r2048")
    got = call(c, upstream=-2.0)
    compare("r2048 upstream -2", got, lc.loss_want("r2048", False, -2.0), upstream=-2.0)
    assert got["loss"].tobytes() == call(c)["loss"].tobytes()                    # scales the gradient only


def test_loss_ignored_elements_do_not_leak_on_the_stride_path():
    """r2049 with NaN logits under every ignored target, in every channel but the row's own and in the rows with a class outside
    [0, K): the bits of the clean call"""
    c = loss_inputs("r2049", True)
    want = call(c)
    Rm, K, M, _ = c["logits"].shape
    x = c["logits"].copy().reshape(Rm, K, M * M)
    keep = np.zeros((Rm, K, M * M), bool)
    on = np.flatnonzero((c["cls"] >= 0) & (c["cls"] < K))
    keep[on, c["cls"][on]] = (c["masks"][on] == 0) | (c["masks"][on] == 1)
    x[~keep] = np.nan
    assert np.isnan(x).sum() > x.size // 2
    got = call(dict(c, logits=x.reshape(c["logits"].shape)))
    assert got["n_valid"] == want["n_valid"] == lc.loss_want("r2049", True)["n_valid"]
    assert got["loss"].tobytes() == want["loss"].tobytes() and got["grad"].tobytes() == want["grad"].tobytes()
