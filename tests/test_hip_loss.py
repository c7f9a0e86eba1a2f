"""dtc_fast_rcnn_loss and dtc_smooth_l1 on the MI355X: the Fast R-CNN head losses, the accuracy and both gradients against the
float64 yardstick -- the reference's own functions with autograd (tests/golden/loss.npz) and their restatement
(tests/loss_ref.py).  -m gpu.

Bounds against the yardstick y, eps = 2^-24 (they are the issue's; e_ref is the float32 CPU reference's own distance from y, stored
per case by the golden generator):
    loss_cls        max(4 e_ref, 32 eps max(|y|, max|cls_score|))        loss_bbox        max(4 e_ref, 32 eps |y|)
    grad_cls_score  absolute 16 eps / n_valid                            grad_bbox_pred   relative 8 eps
    accuracy, n_valid, and every zero the contract promises: exact
Every measured distance is printed, in units of its bound, before it is asserted (tests/README_loss.md records them)."""
import numpy as np
import pytest
import torch

from conftest import golden
import loss_ref as lr
import train_targets_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return golden("loss")


_yard = {}


def yard(case):
    """the float64 restatement of a seeded case, computed once"""
    if case not in _yard:
        c = lr.make_case(case)
        _yard[case] = (c, lr.head(c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"], c["beta"]))
    return _yard[case]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(x, labels, pred=None, t5=None, beta=1.0, upstream=None, losses=True, grads=True, stale=True):
    """dtc_fast_rcnn_loss on host arrays over outputs pre-filled with 0xFF -> dict of host arrays (None for a group not asked for)"""
    from detectorch_amd import hip_loss
    N, C = x.shape
    out = hip_loss.loss_outputs(N, C, 0 if pred is None else pred.shape[1], "cuda", losses, grads)
    if stale:
        for v in out.values():
            if v is not None:
                v.view(torch.uint8).fill_(0xFF)
    hip_loss.fast_rcnn_loss(dev(x), dev(labels), None if pred is None else dev(pred), None if t5 is None else dev(t5), beta=beta,
                            upstream=None if upstream is None else dev(np.asarray(upstream, np.float32)), out=out)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items() if k != "workspace"}


def check(label, got, y, x, e_ref=(0.0, 0.0), rows=None, box4=None):
    """the device's `got` against a yardstick dict y (lr.head's keys).  rows: y's gradient arrays hold these rows only; box4: y's
    grad_box holds the four selected columns, whose first column index per row is box4."""
    b = lr.bounds(y, x, *e_ref)
    nv = int(y["n_valid"])
    L = got["losses"]
    if L is not None:
        d_cls, d_box = abs(float(L[0]) - float(y["loss_cls"])), abs(float(L[1]) - float(y["loss_bbox"]))
        print("%s: loss_cls %.9g off by %.3g = %.3f of its bound, loss_bbox %.9g off by %.3g = %.3f of its bound" % (
            label, L[0], d_cls, d_cls / b["loss_cls"] if b["loss_cls"] else 0.0, L[1], d_box, d_box / b["loss_bbox"] if b["loss_bbox"] else 0.0))
        assert d_cls <= b["loss_cls"] and d_box <= b["loss_bbox"]
        assert L[2] == np.float32(float(y["accuracy"])) and L[3] == np.float32(nv)
    gc, gb = got["grad_cls_score"], got["grad_bbox_pred"]
    if gc is not None:
        sel = slice(None) if rows is None else rows
        d = float(np.abs(gc[sel].astype(np.float64) - y["grad_cls"]).max())
        print("%s: grad_cls_score off by at most %.3g = %.3f of 16 eps / n_valid" % (label, d, d / b["grad_cls"]))
        assert d <= b["grad_cls"]
    if gb is not None and y["grad_box"] is not None:
        mine = gb[slice(None) if rows is None else rows].astype(np.float64)
        want = y["grad_box"]
        if box4 is not None:
            cols = box4[:, None] + np.arange(4)[None, :]
            rest = mine.copy()
            np.put_along_axis(rest, cols, 0.0, 1)
            assert not rest.any()                                            # exact zeros outside the selected columns
            mine = np.take_along_axis(mine, cols, 1)
        nz = want != 0
        assert not mine[~nz].any()                                           # ... and wherever the yardstick is an exact zero
        rel = float((np.abs(mine[nz] - want[nz]) / np.abs(want[nz])).max()) if nz.any() else 0.0
        print("%s: grad_bbox_pred off by at most %.3g relative = %.3f of 8 eps" % (label, rel, rel / b["grad_box"]))
        assert rel <= b["grad_box"]


# ---- (a) .. (e), (i): the seeded cases against the restatement and the reference's own values ----------------------------------
@pytest.mark.parametrize("case", lr.GOLDEN_CASES)
def test_case_against_reference_and_restatement(g, case):
    c, y = yard(case)
    got = run(c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"], c["beta"])
    e = (float(g[case + "_e_ref_cls"]), float(g[case + "_e_ref_box"]))
    valid = c["labels"] >= 0
    check(case + " / restatement", got, y, c["cls_score"][valid], e)
    assert not got["grad_cls_score"][~valid].any() and not got["grad_bbox_pred"][~valid].any()
    N = len(c["labels"])
    rows = lr.sample_rows(case, N) if case in lr.SAMPLED_CASES else np.arange(N)
    k = c["targets5"][:, 0].astype(np.int64)
    k = np.where(k > 0, 1 if c["bbox_pred"].shape[1] == 8 else k, 0)
    ref = dict(loss_cls=g[case + "_loss_cls"], loss_bbox=g[case + "_loss_bbox"], n_valid=int(g[case + "_n_valid"]),
               accuracy=y["accuracy"], grad_cls=g[case + "_grad_cls"], grad_box=g[case + "_grad_box4"])
    assert round(float(g[case + "_accuracy"]) * ref["n_valid"]) == round(float(got["losses"][2]) * ref["n_valid"])
    check(case + " / reference", got, ref, c["cls_score"][valid], e, rows=rows, box4=4 * k[rows])


@pytest.mark.parametrize("case", ("e1", "e05", "e19"))
def test_edge_values_through_smooth_l1(case):
    """(e) on the other entry: the case's expanded targets and unit weights through dtc_smooth_l1"""
    from detectorch_amd import hip_loss
    c, y = yard(case)
    bt, bi, bo = lr.expand(c["targets5"], c["bbox_pred"].shape[1])
    loss, grad = hip_loss.smooth_l1(dev(c["bbox_pred"]), dev(bt), dev(bi), dev(bo), beta=c["beta"])
    torch.cuda.synchronize()
    want = dict(loss_cls=0.0, loss_bbox=y["loss_bbox"], accuracy=0.0, n_valid=y["n_valid"], grad_cls=None, grad_box=y["grad_box"])
    got = dict(losses=np.array([0.0, float(loss.cpu()[0]), 0.0, y["n_valid"]], np.float32), grad_cls_score=None,
               grad_bbox_pred=grad.cpu().numpy())
    check(case + " / dtc_smooth_l1", got, want, np.zeros((1, 1), np.float32))


# ---- (e): general weights on dtc_smooth_l1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(lr.SMOOTH_CASES))
def test_smooth_l1_general_weights(g, case):
    from detectorch_amd import hip_loss
    c = lr.make_smooth_case(case)
    args = [dev(c[k]) for k in ("pred", "targets", "alpha_in", "alpha_out")]
    loss, grad = hip_loss.smooth_l1(*args, beta=c["beta"])
    up = torch.tensor([3.0], device="cuda")
    loss_only, none = hip_loss.smooth_l1(*args, beta=c["beta"], grad=False)
    none2, grad_up = hip_loss.smooth_l1(*args, beta=c["beta"], upstream=up, loss=False)
    torch.cuda.synchronize()
    assert none is None and none2 is None and lr.same_bits(loss.cpu().numpy(), loss_only.cpu().numpy())
    y_loss, y_grad = lr.smooth_l1(c["pred"], c["targets"], c["alpha_in"], c["alpha_out"], c["beta"])
    for label, yl, yg in (("restatement", float(y_loss), y_grad), ("reference", float(g[case + "_loss"]), g[case + "_grad"])):
        bound = max(4 * float(g[case + "_e_ref"]), 32 * lr.EPS * abs(yl))
        d = abs(float(loss.cpu()[0]) - yl)
        nz = yg != 0
        mine = grad.cpu().numpy().astype(np.float64)
        rel = float((np.abs(mine[nz] - yg[nz]) / np.abs(yg[nz])).max())
        rel3 = float((np.abs(grad_up.cpu().numpy().astype(np.float64)[nz] - 3.0 * yg[nz]) / np.abs(3.0 * yg[nz])).max())
        print("%s / %s: loss off by %.3g = %.3f of its bound; grad_pred off by %.3g relative = %.3f of 8 eps (upstream 3: %.3f)" % (
            case, label, d, d / bound, rel, rel / (8 * lr.EPS), rel3 / (8 * lr.EPS)))
        assert d <= bound and rel <= 8 * lr.EPS and rel3 <= 8 * lr.EPS
        assert not mine[~nz].any()                                           # alpha_out 0 (and x = 0): exact zeros


def test_smooth_l1_autograd():
    from detectorch_amd.model import loss as ml
    c = lr.make_smooth_case("s20")
    pred = dev(c["pred"]).requires_grad_()
    out = ml.smooth_L1(pred, dev(c["targets"]), dev(c["alpha_in"]), dev(c["alpha_out"]), c["beta"])
    assert out.dim() == 0 and out.is_cuda
    (out * 3.0).backward()
    torch.cuda.synchronize()
    y_loss, y_grad = lr.smooth_l1(c["pred"], c["targets"], c["alpha_in"], c["alpha_out"], c["beta"], upstream=3.0)
    nz = y_grad != 0
    mine = pred.grad.cpu().numpy().astype(np.float64)
    assert abs(float(out) - float(y_loss)) <= 32 * lr.EPS * float(y_loss)
    assert float((np.abs(mine[nz] - y_grad[nz]) / np.abs(y_grad[nz])).max()) <= 8 * lr.EPS and not mine[~nz].any()


# ---- (f) the padded batch ---------------------------------------------------------------------------------------------------------
def _padded_batch(cases, params, seed, expanded=False):
    """the targets of a batch of train_targets_ref cases through sample_rois_batched, and head outputs for them: NaN past n_rois"""
    from test_hip_train_targets import _batch
    from detectorch_amd.utils import fast_rcnn_sample_rois as fs
    x = _batch(cases)
    knobs = {k: params[k] for k in ("rois_per_image", "fg_fraction", "fg_thresh", "bg_thresh_hi", "bg_thresh_lo", "bbox_thresh",
                                    "crowd_thresh", "reg_weights", "num_classes", "cls_agnostic_bbox_reg")}
    blobs = fs.sample_rois_batched(x["proposals"], x["proposal_counts"], x["gt_boxes"], x["gt_classes"], x["gt_is_crowd"],
                                   x["gt_counts"], x["im_scale"], rand_keys=x["rand_keys"], expanded=expanded, **knobs)
    torch.cuda.synchronize()
    B, R = blobs["labels_int32"].shape
    C = params["num_classes"]
    rs = np.random.RandomState(seed)
    cls_score = (rs.standard_normal((B * R, C)) * 3.0).astype(np.float32)
    bbox_pred = (rs.standard_normal((B * R, 4 * C)) * 0.7).astype(np.float32)
    n = blobs["n_rois"].cpu().numpy()
    valid = (np.arange(R)[None, :] < n[:, None]).reshape(-1)
    cls_score[~valid] = np.nan
    bbox_pred[~valid] = np.nan
    return x, blobs, cls_score, bbox_pred, valid


def test_padded_batch_with_nan_past_n_rois_and_stale_outputs():
    from detectorch_amd import hip_loss
    from detectorch_amd.model import loss as ml
    from detectorch_amd.utils import fast_rcnn_sample_rois as fs
    params = tr.params_of("a")
    x, blobs, cls_score, bbox_pred, valid = _padded_batch(["a", "b", "c"], params, 31)
    assert blobs["bbox_targets"] is None and 0 < valid.sum() < len(valid)     # expanded=False; padding rows present
    labels = blobs["labels_int32"].cpu().numpy().reshape(-1)
    t5 = blobs["bbox_targets5"].cpu().numpy().reshape(-1, 5)
    assert np.array_equal(labels >= 0, valid)
    assert np.array_equal(fs.compact(blobs)["labels_int32"].cpu().numpy(), labels[valid])
    out = hip_loss.loss_outputs(len(labels), 81, 324, "cuda")
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    res = ml.fast_rcnn_losses_fused(dev(cls_score).view(3, -1, 81), dev(bbox_pred).view(3, -1, 324), blobs, out=out)
    torch.cuda.synchronize()
    assert res is out
    got = {k: v.cpu().numpy() for k, v in out.items() if k != "workspace"}
    # the yardstick on the compacted rows, as the reference would see them
    y = lr.head(cls_score[valid], labels[valid], bbox_pred[valid], t5[valid])
    compacted = dict(losses=got["losses"], grad_cls_score=got["grad_cls_score"][valid], grad_bbox_pred=got["grad_bbox_pred"][valid])
    check("padded batch a + b + c", compacted, y, cls_score[valid])
    assert lr.same_bits(got["grad_cls_score"][~valid], np.zeros((int((~valid).sum()), 81), np.float32))
    assert lr.same_bits(got["grad_bbox_pred"][~valid], np.zeros((int((~valid).sum()), 324), np.float32))


def test_compact_targets_against_expanded_through_smooth_l1():
    """the non-default-threshold case of the targets suite: background rows carry targets, so the target class != the label"""
    from detectorch_amd import hip_loss
    from detectorch_amd.utils import fast_rcnn_sample_rois as fs
    params = tr.params_of("f")
    x, blobs, cls_score, bbox_pred, valid = _padded_batch(["f", "a"], params, 32, expanded=True)
    labels = blobs["labels_int32"].cpu().numpy().reshape(-1)
    t5 = blobs["bbox_targets5"].cpu().numpy().reshape(-1, 5)
    assert np.any((t5[:, 0] > 0) & (t5[:, 0] != labels) & valid)
    got = run(cls_score, labels, bbox_pred, t5)
    c = fs.compact(blobs)
    loss, grad = hip_loss.smooth_l1(dev(bbox_pred[valid]), c["bbox_targets"], c["bbox_inside_weights"], c["bbox_outside_weights"])
    torch.cuda.synchronize()
    y = lr.head(cls_score[valid], labels[valid], bbox_pred[valid], t5[valid])
    y_loss, y_grad = lr.smooth_l1(bbox_pred[valid], *[c[k].cpu().numpy() for k in ("bbox_targets", "bbox_inside_weights",
                                                                                  "bbox_outside_weights")], 1.0)
    assert abs(float(y_loss) - float(y["loss_bbox"])) <= 1e-12 * float(y_loss) and np.abs(y_grad - y["grad_box"]).max() <= 1e-15
    check("compact", dict(losses=got["losses"], grad_cls_score=got["grad_cls_score"][valid], grad_bbox_pred=got["grad_bbox_pred"][valid]),
          y, cls_score[valid])
    want = dict(y, loss_cls=0.0, accuracy=0.0)
    check("expanded", dict(losses=np.array([0.0, float(loss.cpu()[0]), 0.0, y["n_valid"]], np.float32), grad_cls_score=None,
                           grad_bbox_pred=grad.cpu().numpy()), want, np.zeros((1, 1), np.float32))


# ---- (g) every row ignored --------------------------------------------------------------------------------------------------------
def test_every_row_ignored_gives_zeros():
    N, C = 70, 81
    got = run(np.full((N, C), np.nan, np.float32), np.full(N, -1, np.int32), np.full((N, 4 * C), np.nan, np.float32),
              np.full((N, 5), np.nan, np.float32))
    assert lr.same_bits(got["losses"], np.zeros(4, np.float32))
    assert lr.same_bits(got["grad_cls_score"], np.zeros((N, C), np.float32))
    assert lr.same_bits(got["grad_bbox_pred"], np.zeros((N, 4 * C), np.float32))


# ---- (h) exact logit ties ----------------------------------------------------------------------------------------------------------
def test_exact_ties_take_the_lowest_index():
    rs = np.random.RandomState(9)
    x = rs.randint(-2, 3, (200, 81)).astype(np.float32)                      # few distinct values: ties everywhere
    x[0] = 0.0
    x[1, [40, 70]] = 5.0                                                     # a tie across the two halves of a row's lanes
    x[2, [31, 32]] = 5.0
    labels = lr.argmax_logits(x).astype(np.int32)
    labels[120:] = rs.randint(0, 81, 80)
    top = x.max(axis=1)
    labels[3] = int(np.where(x[3] == top[3])[0][-1]) if np.sum(x[3] == top[3]) > 1 else labels[3]
    y = lr.head(x, labels)
    got = run(x, labels)
    assert np.sum((x == top[:, None]).sum(axis=1) > 1) > 100
    assert got["losses"][2] == np.float32(float(y["accuracy"])) and 0.5 < got["losses"][2] < 1.0
    check("ties", got, y, x)


# ---- (i) many workgroups: the same bits eagerly and under graph replay --------------------------------------------------------------
@pytest.mark.parametrize("case", ("i4097", "i65536"))
def test_eager_calls_and_graph_replay_are_bit_identical(case):
    from detectorch_amd import hip_loss
    c, _ = yard(case)
    x, labels, pred, t5 = dev(c["cls_score"]), dev(c["labels"]), dev(c["bbox_pred"]), dev(c["targets5"])
    N, C = c["cls_score"].shape
    outs = [hip_loss.loss_outputs(N, C, 4 * C, "cuda") for _ in range(3)]
    for fill, out in zip((0xFF, 0x00, 0x7F), outs):
        for v in out.values():
            v.view(torch.uint8).fill_(fill)
    hip_loss.fast_rcnn_loss(x, labels, pred, t5, out=outs[0])
    hip_loss.fast_rcnn_loss(x, labels, pred, t5, out=outs[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip_loss.fast_rcnn_loss(x, labels, pred, t5, out=outs[2])
    torch.cuda.synchronize()
    for v in outs[2].values():
        v.view(torch.uint8).fill_(0x7F)
    graph.replay()
    graph.replay()                                                           # the arrival counter is readied by the call itself
    torch.cuda.synchronize()
    for k in ("losses", "grad_cls_score", "grad_bbox_pred"):
        a = outs[0][k].cpu().numpy()
        assert lr.same_bits(a, outs[1][k].cpu().numpy()) and lr.same_bits(a, outs[2][k].cpu().numpy()), k


# ---- (j) a label or a target class that is no index ---------------------------------------------------------------------------------
def test_label_and_target_class_out_of_range_are_never_an_index():
    c = lr.make_case("b")
    x, labels, pred, t5 = c["cls_score"].copy(), c["labels"].copy(), c["bbox_pred"].copy(), c["targets5"].copy()
    N, C = x.shape
    labels[3] = C                                                            # a naive index lands in row 4 of cls_score
    labels[10] = C + 5
    t5[5, 0] = C                                                             # ... in row 6 of bbox_pred
    t5[7, 0] = 1.5
    t5[9, 0] = np.nan
    t5[11, 0] = -3.0
    t5[5, 1:] = t5[7, 1:] = t5[9, 1:] = t5[11, 1:] = 0.25
    y = lr.head(x, labels, pred, t5)
    got = run(x, labels, pred, t5)
    check("out of range", got, y, x)
    assert y["n_valid"] == N and got["losses"][3] == N
    assert not got["grad_cls_score"][[3, 10]].any() and not got["grad_bbox_pred"][[5, 7, 9, 11]].any()
    # the contract: such a row is ignored for the term it would have indexed -- the same bits as with the row's term switched off
    labels2, t52 = labels.copy(), t5.copy()
    t52[[5, 7, 9, 11]] = 0.0
    ref = run(x, labels2, pred, t52)
    assert lr.same_bits(got["losses"], ref["losses"]) and lr.same_bits(got["grad_bbox_pred"], ref["grad_bbox_pred"])
    x2 = x.copy()
    x2[4] += 1.0                                                             # the row a naive index would have read
    x2[[3, 10]] = np.nan                                                     # and the rows themselves are not read
    other = run(x2, labels, pred, t5)
    keep = np.ones(N, bool)
    keep[4] = False
    assert lr.same_bits(other["grad_cls_score"][keep], got["grad_cls_score"][keep])


# ---- (k) upstream factors and the nullable groups ----------------------------------------------------------------------------------
def test_upstream_and_nullable_groups():
    c, _ = yard("b")
    x, labels, pred, t5 = c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"]
    up = (0.5, 3.0)
    y = lr.head(x, labels, pred, t5, upstream=up)
    fused = run(x, labels, pred, t5, upstream=up)
    check("upstream (0.5, 3)", fused, y, x)
    loss_only = run(x, labels, pred, t5, upstream=up, grads=False)
    grad_only = run(x, labels, pred, t5, upstream=up, losses=False)
    assert loss_only["grad_cls_score"] is None and loss_only["grad_bbox_pred"] is None and grad_only["losses"] is None
    assert lr.same_bits(loss_only["losses"], fused["losses"])
    assert lr.same_bits(grad_only["grad_cls_score"], fused["grad_cls_score"])
    assert lr.same_bits(grad_only["grad_bbox_pred"], fused["grad_bbox_pred"])
    plain = run(x, labels, pred, t5)                                         # the losses do not carry the factors
    assert lr.same_bits(plain["losses"], fused["losses"])
    # cross-entropy and accuracy only: the box arguments NULL
    for kw in (dict(), dict(grads=False), dict(losses=False)):
        ce = run(x, labels, upstream=up, **kw)
        assert ce["grad_bbox_pred"] is None
        if ce["losses"] is not None:
            assert ce["losses"][1] == 0 and lr.same_bits(ce["losses"][[0, 2, 3]], fused["losses"][[0, 2, 3]])
        if ce["grad_cls_score"] is not None:
            assert lr.same_bits(ce["grad_cls_score"], fused["grad_cls_score"])


# ---- (l) autograd --------------------------------------------------------------------------------------------------------------------
def _torch_restatement(cls_score, bbox_pred, labels, t5, beta=1.0):
    """train_fast.py:141-154 in torch ops on device tensors, float64: compact the valid rows, expand the targets, the formulas of
    loss.py:13-20 and cross_entropy -> (loss_cls, loss_bbox)"""
    keep = labels >= 0
    x, p, l, t = cls_score[keep].double(), bbox_pred[keep].double(), labels[keep].long(), t5[keep].double()
    W = p.shape[1]
    k = t[:, 0].long()
    cols = 4 * k[:, None] + torch.arange(4, device=p.device)[None, :]
    bt = torch.zeros_like(p).scatter_(1, cols, t[:, 1:]) * (k[:, None] > 0)
    bw = torch.zeros_like(p).scatter_(1, cols, 1.0) * (k[:, None] > 0)
    d = (p - bt) * bw
    a = d.abs()
    case1 = (a <= beta).double()
    loss_bbox = torch.sum((0.5 * d ** 2 / beta * case1 + (a - 0.5 * beta) * (1 - case1)) * (bw > 0).double()) / p.shape[0]
    return torch.nn.functional.cross_entropy(x, l), loss_bbox


def test_autograd_of_fast_rcnn_losses():
    from detectorch_amd.model import loss as ml
    params = tr.params_of("a")
    _, blobs, cls_score, bbox_pred, valid = _padded_batch(["a", "b"], params, 33)
    cls_score[~valid] = 0.0                                                  # (finite everywhere: the torch side multiplies by masks)
    bbox_pred[~valid] = 0.0
    xs, ps = dev(cls_score).requires_grad_(), dev(bbox_pred).requires_grad_()
    loss_cls, loss_bbox, acc = ml.fast_rcnn_losses(xs.view(2, -1, 81), ps.view(2, -1, 324), blobs)
    assert loss_cls.dim() == 0 and loss_bbox.dim() == 0 and acc.dim() == 0 and not acc.requires_grad
    (loss_cls + loss_bbox).backward()
    xt, pt = dev(cls_score).requires_grad_(), dev(bbox_pred).requires_grad_()
    labels, t5 = blobs["labels_int32"].reshape(-1), blobs["bbox_targets5"].reshape(-1, 5)
    want_cls, want_bbox = _torch_restatement(xt, pt, labels, t5)
    (want_cls + want_bbox).backward()
    torch.cuda.synchronize()
    nv = int(valid.sum())
    y = dict(loss_cls=float(want_cls), loss_bbox=float(want_bbox), n_valid=nv, grad_cls=xt.grad.double().cpu().numpy(),
             grad_box=pt.grad.double().cpu().numpy(), accuracy=float(acc))
    got = dict(losses=np.array([float(loss_cls), float(loss_bbox), float(acc), nv], np.float32),
               grad_cls_score=xs.grad.cpu().numpy(), grad_bbox_pred=ps.grad.cpu().numpy())
    check("autograd", got, y, cls_score[valid])
    assert not got["grad_cls_score"][~valid].any() and not got["grad_bbox_pred"][~valid].any()
    # the reference-shaped entries on the compacted rows
    lab = labels.cpu().numpy()
    ce = ml.cross_entropy(dev(cls_score[valid]), dev(lab[valid]).long())
    ac = ml.accuracy(dev(cls_score[valid]), dev(lab[valid]).long())
    assert ce.dim() == 0 and abs(float(ce) - float(loss_cls)) <= 2 * lr.EPS * float(loss_cls) and float(ac) == float(acc)


# ---- (m) targets -> losses -> gradients in one graph ------------------------------------------------------------------------------
def test_one_graph_from_proposals_to_gradients():
    from test_hip_train_targets import _batch
    from detectorch_amd import hip_loss
    from detectorch_amd.model import loss as ml
    from detectorch_amd.utils import fast_rcnn_sample_rois as fs
    params = tr.params_of("a")
    knobs = dict(rois_per_image=params["rois_per_image"], expanded=False)
    x = _batch(["a", "f"], G=8, P=320)
    B, R, C = 2, params["rois_per_image"], 81
    rs = np.random.RandomState(34)
    cls_score = dev((rs.standard_normal((B, R, C)) * 3.0).astype(np.float32))
    bbox_pred = dev((rs.standard_normal((B, R, 4 * C)) * 0.7).astype(np.float32))
    args = lambda v: (v["proposals"], v["proposal_counts"], v["gt_boxes"], v["gt_classes"], v["gt_is_crowd"], v["gt_counts"], v["im_scale"])
    blobs = fs.sample_rois_batched(*args(x), rand_keys=x["rand_keys"], **knobs)          # one eager pass, then the capture
    out = ml.fast_rcnn_losses_fused(cls_score, bbox_pred, blobs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fs.sample_rois_batched(*args(x), rand_keys=x["rand_keys"], out=blobs, **knobs)
        ml.fast_rcnn_losses_fused(cls_score, bbox_pred, blobs, out=out)
    torch.cuda.synchronize()
    y = _batch(["i", "b"], G=8, P=320)                                       # rewritten in place: proposals, gt, keys, logits
    y["rand_keys"] = y["rand_keys"].flip(1).contiguous()
    for k in x:
        x[k].copy_(y[k])
    cls2 = dev((rs.standard_normal((B, R, C)) * 3.0).astype(np.float32))
    box2 = dev((rs.standard_normal((B, R, 4 * C)) * 0.7).astype(np.float32))
    cls_score.copy_(cls2)
    bbox_pred.copy_(box2)
    graph.replay()
    torch.cuda.synchronize()
    eager_blobs = fs.sample_rois_batched(*args(y), rand_keys=y["rand_keys"], **knobs)
    eager = ml.fast_rcnn_losses_fused(cls2, box2, eager_blobs)
    torch.cuda.synchronize()
    assert lr.same_bits(blobs["labels_int32"].cpu().numpy(), eager_blobs["labels_int32"].cpu().numpy())
    assert lr.same_bits(blobs["bbox_targets5"].cpu().numpy(), eager_blobs["bbox_targets5"].cpu().numpy())
    for k in ("losses", "grad_cls_score", "grad_bbox_pred"):
        assert lr.same_bits(out[k].cpu().numpy(), eager[k].cpu().numpy()), k
    assert float(out["losses"][3]) == float(eager_blobs["n_rois"].sum()) and float(out["losses"][0]) > 0
