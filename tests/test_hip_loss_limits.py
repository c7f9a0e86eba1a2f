"""dtc_fast_rcnn_loss and dtc_smooth_l1 on the MI355X off their default points: the cases of tests/loss_limit_cases.py (the table
is in tests/README_loss.md) against the float64 restatement (tests/loss_ref.py) first, then against what the reference's own
functions gave in float64 (tests/golden/loss_limits.npz) wherever the reference can compute the case.  -m gpu.

Bounds against a yardstick y, eps = 2^-24 (loss_ref.bounds; e_ref is the float32 CPU reference's own distance from y, stored per case
by the fixture's generator, 0 for a case the reference cannot compute):
    loss_cls        max(4 e_ref, 32 eps max(|y|, max|cls_score|))        loss_bbox        max(4 e_ref, 32 eps |y|)
    grad_cls_score  absolute 16 eps |upstream[0]| / n_valid              grad_bbox_pred   relative 8 eps
    accuracy, n_valid and every promised zero: exact; gradient rows of ignored rows and unselected columns: the bits of +0.0
Every measured distance is printed, in units of its bound, before it is asserted, and the largest per quantity at the end of the
module (tests/README_loss.md records them).  Every output is pre-filled with 0xFF, and tests/test_loss_limits_host.py holds what
keeps a case from passing emptily."""
import numpy as np
import pytest
import torch

from conftest import golden
import loss_limit_cases as ll
import loss_ref as lr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    yield dict(golden("loss_limits"))
    for q, (u, label) in sorted(ll.WORST.items()):
        print("largest %s: %.3f of its bound (%s)" % (q, u, label))


def _valid_x(c):
    labels = c["labels"]
    return c["cls_score"][(labels >= 0) & (labels < c["cls_score"].shape[1])]


def _zero_bits(c, got):
    """gradient rows of ignored rows (and of rows whose label is no index), and every unselected column: the bits of +0.0"""
    labels = c["labels"]
    C = c["cls_score"].shape[1]
    dead = (labels < 0) | (labels >= C)
    gc = got["grad_cls_score"]
    assert lr.same_bits(gc[dead], np.zeros_like(gc[dead]))
    gb = got["grad_bbox_pred"]
    if gb is not None:
        keep = np.zeros(gb.shape, bool)
        with np.errstate(invalid="ignore"):
            k = c["targets5"][:, 0]
            has = (labels >= 0) & (k > 0) & (k < C) & (k == np.floor(k))
        first = 4 * np.where(has, 1 if gb.shape[1] == 8 else np.nan_to_num(k, nan=0.0, posinf=0.0).astype(np.int64), 0)
        np.put_along_axis(keep, first[:, None] + np.arange(4)[None, :], True, 1)
        keep[~has] = False
        assert lr.same_bits(gb[~keep], np.zeros(int((~keep).sum()), np.float32))


def _against_both(g, name, got):
    """a head case against the restatement and, where the fixture has it, the reference's values"""
    c, y = ll.case(name), ll.want(name)
    e = tuple(g[name + "_scalars"][4:6]) if name in ll.RECORDED else (0.0, 0.0)
    ll.measure(name + " / restatement", got, y, _valid_x(c), e)
    if got["grad_cls_score"] is not None:
        _zero_bits(c, got)
    if name not in ll.RECORDED:
        return
    loss_cls, loss_bbox, acc, nv = g[name + "_scalars"][:4]
    assert round(acc * nv) == round(float(y["accuracy"]) * nv)
    rows = ll.sample_rows(name)
    rows = np.arange(len(c["labels"])) if rows is None else rows
    ref = dict(loss_cls=loss_cls, loss_bbox=loss_bbox, accuracy=y["accuracy"], n_valid=int(nv), grad_cls=g[name + "_grad_cls"],
               grad_box=g.get(name + "_grad_box4"))
    ll.measure(name + " / reference", got, ref, _valid_x(c), e, rows=rows, box4=None if c["bbox_pred"] is None else ll.selected(c)[rows])


# ---- 1, 2: lane widths, register depths, the class-agnostic form ----------------------------------------------------------------------
@pytest.mark.parametrize("C", ll.SWEEP_C)
def test_lane_width_sweep(g, C):
    name = "s%d" % C
    got = ll.head_call(ll.case(name))
    _against_both(g, name, got)
    assert 0 < got["losses"][2] < 1 and got["losses"][3] == 54


@pytest.mark.parametrize("C", ll.AGNOSTIC_C)
def test_class_agnostic_width_8(g, C):
    name = "w%d" % C
    got = ll.head_call(ll.case(name))
    _against_both(g, name, got)
    gb = got["grad_bbox_pred"]
    assert gb.shape == (67, 8) and lr.same_bits(gb[:, :4], np.zeros((67, 4), np.float32))
    k = ll.case(name)["targets5"][:, 0]
    assert gb[k == 1, 4:].all() and gb[k == C - 1, 4:].all() and not gb[k == 0].any()


# ---- 3: the row loop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ll.WRAPS))
def test_row_loop_trips(g, name):
    c = ll.case(name)
    on_device = {k: (ll.dev(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    first, second = ll.head_call(on_device), ll.head_call(on_device)
    for k in first:
        assert (first[k] is None and second[k] is None) or lr.same_bits(first[k], second[k]), k
    assert (first["grad_bbox_pred"] is None) == (not ll.WRAPS[name][2])
    _against_both(g, name, first)


def test_one_valid_row_on_the_second_trip(g):
    c = ll.case(ll.ONE_VALID)
    got = ll.head_call(c)
    _against_both(g, ll.ONE_VALID, got)
    alone = ll.head_call({k: (v[4098:] if isinstance(v, np.ndarray) else v) for k, v in c.items()})
    assert got["losses"][3] == 1 and lr.same_bits(got["losses"], alone["losses"])      # that row's own losses, the divisor 1
    for k in ("grad_cls_score", "grad_bbox_pred"):
        assert lr.same_bits(got[k][4098:], alone[k]) and lr.same_bits(got[k][:4098], np.zeros_like(got[k][:4098])), k


# ---- 4: target-class values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agnostic", (False, True))
def test_target_class_values_are_never_an_index(agnostic):
    c, off = ll.make_target_classes(agnostic)
    label = "target classes W = %d" % c["bbox_pred"].shape[1]
    got, plain = ll.head_call(c), ll.head_call(off)
    y = lr.head(c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"])
    ll.measure(label, got, y, c["cls_score"])
    _zero_bits(c, got)
    assert not got["grad_bbox_pred"][:6].any() and got["grad_bbox_pred"][6].any()
    for k in got:                                                            # the same bits as with those rows' terms switched off
        assert lr.same_bits(got[k], plain[k]), k


# ---- 5: magnitudes ----------------------------------------------------------------------------------------------------------------------------
def test_extreme_finite_logits(g):
    c = ll.case("mlogits")
    got = ll.head_call(c)
    _against_both(g, "mlogits", got)
    gc, labels = got["grad_cls_score"], c["labels"]
    assert np.all(np.isfinite(got["losses"])) and got["losses"][0] > 5e37
    # a one-hot softmax: the label column's gradient is an exact zero on the hit and exactly -1 / n_valid on the miss
    assert gc[4, labels[4]] == 0 and not gc[4].any()
    assert gc[5, labels[5]] == np.float32(-0.125) and gc[5, 45] == np.float32(0.125) and np.count_nonzero(gc[5]) == 2
    others = np.delete(gc[2], labels[2])                                     # the all-equal row: one value off the label column
    assert np.all(others == others[0]) and others[0] > 0
    up = ll.head_call(c, upstream=(-2.0, 0.25))
    assert up["grad_cls_score"][5, labels[5]] == np.float32(0.25) and up["grad_cls_score"][4, labels[4]] == 0


def _flat_call(c, upstream=None, loss=True, grad=True):
    from detectorch_amd import hip_loss
    args = [ll.dev(c[k]) for k in ("pred", "targets", "alpha_in", "alpha_out")]
    out = hip_loss.smooth_l1(*args, beta=c["beta"], upstream=upstream, loss=loss, grad=grad)
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in out)


def _measure_flat(label, loss, grad, y_loss, y_grad, e_ref=0.0):
    """dtc_smooth_l1's outputs against (y_loss, y_grad): through measure(), as the box term of a head call of as many rows"""
    want = dict(loss_cls=0.0, loss_bbox=y_loss, accuracy=0.0, n_valid=0, grad_cls=None, grad_box=y_grad)
    got = dict(losses=None if loss is None else np.array([0.0, float(loss[0]), 0.0, 0.0], np.float32), grad_cls_score=None,
               grad_bbox_pred=grad)
    ll.measure(label, got, want, np.zeros((1, 1), np.float32), (0.0, e_ref))


@pytest.mark.parametrize("name", sorted(ll.MAG_BETAS))
def test_extreme_box_terms_through_both_entries(g, name):
    c = ll.case(name)
    got = ll.head_call(c)
    _against_both(g, name, got)
    assert np.all(np.isfinite(got["losses"])) and np.all(np.isfinite(got["grad_bbox_pred"]))
    bt, bi, bo = lr.expand(c["targets5"], 20)
    flat = dict(pred=c["bbox_pred"], targets=bt, alpha_in=bi, alpha_out=bo, beta=c["beta"])
    loss, grad = _flat_call(flat)
    y = ll.want(name)
    _measure_flat(name + " / dtc_smooth_l1", loss, grad, y["loss_bbox"], y["grad_box"])
    # one formula behind both entries (loss_common.h), one divisor: every gradient element the same value
    assert np.array_equal(grad, got["grad_bbox_pred"])


def test_extreme_weights_through_smooth_l1():
    c = ll.make_magnitude_alpha()
    loss, grad = _flat_call(c)
    y_loss, y_grad = lr.smooth_l1(c["pred"], c["targets"], c["alpha_in"], c["alpha_out"], c["beta"])
    _measure_flat("alpha_in {0, -1.5, 1e10} x alpha_out {0, -1, 2^-20}", loss, grad, y_loss, y_grad)
    assert not grad[(c["alpha_in"] == 0) | (c["alpha_out"] == 0)].any() and np.isfinite(loss[0])


# ---- 6: upstream ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", ll.UPSTREAMS)
def test_upstream_factors(up):
    c = lr.make_case("b")
    y = lr.head(c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"], upstream=up)
    got, plain = ll.head_call(c, upstream=up), ll.head_call(c)
    ll.measure("upstream %s" % (up,), got, y, c["cls_score"], upstream=up)
    assert lr.same_bits(got["losses"], plain["losses"])                      # the losses do not carry the factors
    if up[0] == 0:
        assert not got["grad_cls_score"].any()                               # compares equal to zero; the sign bit is not pinned
    else:
        assert got["grad_cls_score"].any()
    assert got["grad_bbox_pred"].any() == (up[1] != 0)


def test_graph_replay_reads_rewritten_upstream():
    from detectorch_amd import hip_loss
    c = lr.make_case("b")
    x, labels, pred, t5 = (ll.dev(c[k]) for k in ("cls_score", "labels", "bbox_pred", "targets5"))
    up = ll.dev(np.array([0.5, 3.0], np.float32))
    out = hip_loss.loss_outputs(65, 81, 324, "cuda")
    hip_loss.fast_rcnn_loss(x, labels, pred, t5, upstream=up, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip_loss.fast_rcnn_loss(x, labels, pred, t5, upstream=up, out=out)
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in out.items()}
    up.copy_(ll.dev(np.array([-2.0, 0.25], np.float32)))                     # the two floats rewritten in place
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    eager = ll.head_call(c, upstream=(-2.0, 0.25))
    for k in ("losses", "grad_cls_score", "grad_bbox_pred"):
        assert lr.same_bits(out[k].cpu().numpy(), eager[k]), k
    assert not torch.equal(first["grad_cls_score"], out["grad_cls_score"])


# ---- 7: pointer offsets ------------------------------------------------------------------------------------------------------------------------
HEAD_OUT = ("losses", "grad_cls_score", "grad_bbox_pred")


def _carve_head(c, skew):
    """every buffer of a dtc_fast_rcnn_loss call from one arena; skew: buffer name -> words past a 16-byte boundary"""
    from detectorch_amd import hip, hip_loss
    N, C = c["cls_score"].shape
    W = c["bbox_pred"].shape[1]
    need = hip.invoke(hip_loss.lib(), hip_loss.SIGNATURES, "dtc_fast_rcnn_loss_workspace_bytes", dict(n=N, c=C))
    assert need % 4 == 0
    a = ll.Arena(2 * N * (C + W) + N * 6 + need // 4 + 12 * (ll.GUARD + 8))
    s = lambda k: skew.get(k, 0)
    b = dict(cls_score=a.take(N * C, s("cls_score"), host=c["cls_score"]), labels=a.take(N, s("labels"), host=c["labels"]),
             bbox_pred=a.take(N * W, s("bbox_pred"), host=c["bbox_pred"]),
             bbox_targets5=a.take(N * 5, s("bbox_targets5"), host=c["targets5"]),
             upstream=a.take(2, s("upstream"), host=np.array([0.5, 3.0], np.float32)),
             workspace=a.take(need // 4, s("workspace")), losses=a.take(4, s("losses"), dtype=torch.float32),
             grad_cls_score=a.take(N * C, s("grad_cls_score"), dtype=torch.float32),
             grad_bbox_pred=a.take(N * W, s("grad_bbox_pred"), dtype=torch.float32))
    args = dict(b, n=N, c=C, bbox_width=W, beta=c["beta"], workspace_bytes=need)
    return a, b, args


def _invoke_head(args):
    from detectorch_amd import hip, hip_loss
    hip.invoke(hip_loss.lib(), hip_loss.SIGNATURES, "dtc_fast_rcnn_loss", dict(args))
    torch.cuda.synchronize()


def test_four_byte_aligned_pointers():
    c = ll.make_sweep(81)
    assert c["cls_score"].shape == (67, 81)
    a0, b0, args0 = _carve_head(c, {})
    _invoke_head(args0)
    odd = dict(cls_score=1, labels=3, bbox_targets5=1, upstream=3, losses=1, grad_cls_score=3)
    a1, b1, args1 = _carve_head(c, odd)
    for k, v in b1.items():
        assert v.data_ptr() % 16 == (4 * odd[k] if k in odd else 0), k
    _invoke_head(args1)
    y = lr.head(c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"], upstream=(0.5, 3.0))
    host = lambda b: {k: b[k].cpu().numpy().reshape(67, -1) if k != "losses" else b[k].cpu().numpy() for k in HEAD_OUT}
    ll.measure("4-byte aligned pointers", host(b1), y, _valid_x(c), upstream=(0.5, 3.0))
    for k in HEAD_OUT:
        assert lr.same_bits(b0[k].cpu().numpy(), b1[k].cpu().numpy()), k
    assert a0.outside_is_untouched() and a1.outside_is_untouched()          # the guard words behind every buffer


@pytest.mark.parametrize("which", ("bbox_pred", "grad_bbox_pred", "workspace"))
def test_sixteen_byte_requirement_is_checked_before_anything_is_written(which):
    c = ll.make_sweep(81)
    a, b, args = _carve_head(c, {which: 1})
    assert b[which].data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="DTC_EINVAL"):
        _invoke_head(args)
    torch.cuda.synchronize()
    for k in HEAD_OUT + ("workspace",):
        assert bool((b[k].view(torch.int32) == -1).all()), k                 # every output byte still 0xFF
    assert a.outside_is_untouched()


# ---- 8: the flat pass of dtc_smooth_l1 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(ll.FLAT), ids=ll.flat_name)
def test_flat_pass_left_overs_and_wraps(g, shape):
    from detectorch_amd import hip, hip_loss
    N, W = shape
    total = N * W
    c, name = ll.make_flat(shape), ll.flat_name(shape)
    L, S = hip_loss.lib(), hip_loss.SIGNATURES
    need = hip.invoke(L, S, "dtc_smooth_l1_workspace_bytes", dict(n=N, w=W))
    a = ll.Arena(6 * (total + 4) + 2 * need // 4 + 16 + 12 * (ll.GUARD + 8))
    ins = {k: a.take(total, host=c[k]) for k in ("pred", "targets", "alpha_in", "alpha_out")}
    f32 = torch.float32
    forms = {"both": (a.take(1, dtype=f32), a.take(total, dtype=f32), a.take(need // 4)),
             "loss": (a.take(1, dtype=f32), None, a.take(need // 4)), "grad": (None, a.take(total, dtype=f32), None)}
    for loss, grad, ws in forms.values():
        assert all(v is None or v.data_ptr() % 16 == 0 for v in (loss, grad, ws))
        hip.invoke(L, S, "dtc_smooth_l1", dict(ins, n=N, w=W, beta=c["beta"], upstream=None, workspace=ws,
                                               workspace_bytes=need if ws is not None else 0, loss=loss, grad_pred=grad))
    torch.cuda.synchronize()
    loss, grad = forms["both"][0].cpu().numpy(), forms["both"][1].cpu().numpy()
    assert lr.same_bits(loss, forms["loss"][0].cpu().numpy()) and lr.same_bits(grad, forms["grad"][1].cpu().numpy())
    assert a.outside_is_untouched()                                          # the guard words behind grad_pred among them
    y_loss, y_grad = lr.smooth_l1(c["pred"], c["targets"], c["alpha_in"], c["alpha_out"], c["beta"])
    e_ref = float(g[name + "_scalars"][1])
    _measure_flat(name + " / restatement", loss, grad.reshape(N, W), y_loss, y_grad, e_ref)
    sample = ll.flat_sample(shape)
    _measure_flat(name + " / reference", loss, grad[sample][None], float(g[name + "_scalars"][0]), g[name + "_grad"][None], e_ref)
