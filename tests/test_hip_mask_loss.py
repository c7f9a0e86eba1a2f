"""dtc_mask_loss on the GPU against the float64 yardstick of tests/mask_train_ref.py (and the reference's own float64 values where
tests/golden/mask_train.npz has the case), with the bound rules of tests/README_loss.md: loss max(4 e_ref, 32 eps max(|y|, max |x|)),
gradient absolute 16 eps |upstream| / n_valid, n_valid and every promised zero exact (+0.0: the sign bit is checked).  Every distance
is printed in units of its bound.  Outputs are pre-filled with 0xFF and followed by guard words."""
import numpy as np
import pytest
import torch

from conftest import golden
import mask_train_ref as mr

pytestmark = pytest.mark.gpu

GUARD = 16


@pytest.fixture(scope="module")
def g():
    return golden("mask_train")


def fresh(Rm, K, M, grad=True, offset=0):
    """loss / n_valid / grad as views of 0xFF arenas with GUARD words behind them; `offset`: words the gradient starts past a 16-byte
    boundary"""
    from detectorch_amd import hip_mask
    n = Rm * K * M * M
    arenas = dict(loss=torch.full((1 + GUARD,), -1, dtype=torch.int32, device="cuda"),
                  n_valid=torch.full((1 + GUARD,), -1, dtype=torch.int32, device="cuda"),
                  grad=torch.full((offset + n + GUARD,), -1, dtype=torch.int32, device="cuda"))
    need = hip_mask.lib().dtc_mask_loss_workspace_bytes(Rm, K, M)
    out = dict(loss=arenas["loss"][:1].view(torch.float32), n_valid=arenas["n_valid"][:1],
               grad_mask_logits=arenas["grad"][offset:offset + n].view(torch.float32).view(Rm, K, M, M) if grad else None,
               workspace=torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda"))
    return out, arenas


def stale(out, arenas):
    for a in arenas.values():
        a.fill_(-1)
    out["workspace"].fill_(0xFF)


def call(c, upstream=None, grad=True, offset=0, out=None, arenas=None):
    from detectorch_amd import hip_mask
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    Rm, K, M, _ = c["logits"].shape
    if out is None:
        out, arenas = fresh(Rm, K, M, grad, offset)
    up = None if upstream is None else dev(np.asarray([upstream], np.float32), torch.float32)
    hip_mask.mask_loss(dev(c["logits"], torch.float32), dev(c["masks"], torch.int32), dev(c["cls"], torch.int32), upstream=up, out=out)
    torch.cuda.synchronize()
    for k, a in arenas.items():
        assert bool((a[-GUARD:] == -1).all()), "guard words behind %s" % k
    if not grad:
        assert bool((arenas["grad"] == -1).all())
    return dict(loss=out["loss"].cpu().numpy()[0], n_valid=int(out["n_valid"].cpu()[0]),
                grad=None if out["grad_mask_logits"] is None else out["grad_mask_logits"].cpu().numpy())


def compare(tag, got, y, upstream=1.0, e_ref=0.0, want_loss=None):
    b = mr.loss_bounds(y, e_ref=e_ref, upstream=upstream)
    assert got["n_valid"] == y["n_valid"]
    d_loss = abs(float(got["loss"]) - (y["loss"] if want_loss is None else want_loss))
    line = "%-14s loss %.6g: %.3f of its bound" % (tag, float(got["loss"]), d_loss / b["loss"] if b["loss"] else 0.0)
    if got["grad"] is not None:
        zero = ~y["valid"]                                                   # the promised zeros: +0.0, sign bit clear
        assert np.array_equal(got["grad"].view(np.uint32)[zero], np.zeros(int(zero.sum()), np.uint32))
        d_grad = float(np.max(np.abs(got["grad"].astype(np.float64) - y["grad"]))) if got["grad"].size else 0.0
        line += "; gradient %.3f of its bound" % (d_grad / b["grad"] if b["grad"] else 0.0)
        print(line)
        assert d_grad <= b["grad"]
    else:
        print(line)
    assert d_loss <= b["loss"]
    if y["n_valid"] == 0:
        assert got["loss"].tobytes() == np.float32(0).tobytes()


@pytest.mark.parametrize("case", sorted(mr.LOSS_CASES))
def test_case_against_yardstick(g, case):
    c = mr.make_loss_case(case)
    y = mr.loss64(c["logits"], c["masks"], c["cls"])
    e_ref = float(g["loss_" + case + "_e_ref"]) if "loss_" + case in g.files else 0.0
    got = call(c)
    compare(case, got, y, e_ref=e_ref)
    if "loss_" + case in g.files:
        compare(case + " (ref)", dict(got, grad=None), y, e_ref=e_ref, want_loss=float(g["loss_" + case]))
    assert call(c, grad=False)["loss"].tobytes() == got["loss"].tobytes()      # loss-only: the fused call's bits


@pytest.mark.parametrize("case", ("r1m1", "r3m14", "r65m7", "r64m28", "r257m14", "m3k81", "m28k81", "m5k2"))
def test_extreme_logits(g, case):
    """0, +-1e-40, +-16.7, +-88, +-104, +-1e4, +-3e38 on the first elements of every valid row's class channel, each against both
    targets over the rows"""
    c = mr.make_loss_case(case, extremes=True)
    y = mr.loss64(c["logits"], c["masks"], c["cls"])
    got = call(c)
    assert np.isfinite(got["loss"]) and np.isfinite(got["grad"]).all()
    compare(case + "_x", got, y, e_ref=float(g["loss_" + case + "_x_e_ref"]))
    compare(case + "_x (ref)", dict(got, grad=None), y, want_loss=float(g["loss_" + case + "_x"]))


@pytest.mark.parametrize("upstream", (None, 0.0, -2.0))
def test_upstream(upstream):
    c = mr.make_loss_case("r65m7")
    up = 1.0 if upstream is None else upstream
    y = mr.loss64(c["logits"], c["masks"], c["cls"], upstream=up)
    got = call(c, upstream=upstream)
    compare("upstream %s" % upstream, got, y, upstream=up)
    assert got["loss"].tobytes() == call(c)["loss"].tobytes()                   # scales the gradient only
    if upstream == 0.0:
        assert not got["grad"].any()                    # (sigmoid(x) - t) * 0 on the valid elements: zero of either sign, as IEEE has it


def test_all_ignored():
    c = mr.make_loss_case("r65m7")
    for what in ("targets", "classes"):
        d = dict(c, masks=c["masks"].copy(), cls=c["cls"].copy())
        if what == "targets":
            d["masks"][:] = np.array([-1, 2, np.iinfo(np.int32).min, 7], np.int32)[np.arange(d["masks"].size).reshape(d["masks"].shape) % 4]
        else:
            d["cls"][:] = np.where(np.arange(len(d["cls"])) % 2, -1, 81)
        d["logits"] = d["logits"].copy()
        d["logits"][::2] = np.nan                                             # an ignored logit is not read
        got = call(d)
        assert got["n_valid"] == 0 and got["loss"].tobytes() == np.float32(0).tobytes() and not got["grad"].view(np.uint32).any()


def test_ignored_elements_do_not_leak():
    """NaN logits under every ignored target, in every channel but the row's own and in the rows with a class outside [0, K): the bits
    of the clean call"""
    c = mr.make_loss_case("r65m7")
    want = call(c)
    Rm, K, M, _ = c["logits"].shape
    x = c["logits"].copy().reshape(Rm, K, M * M)
    for r in range(Rm):
        k = c["cls"][r]
        keep = np.zeros((K, M * M), bool)
        if 0 <= k < K:
            keep[k] = (c["masks"][r] == 0) | (c["masks"][r] == 1)
        x[r][~keep] = np.nan
    got = call(dict(c, logits=x.reshape(c["logits"].shape)))
    assert got["loss"].tobytes() == want["loss"].tobytes() and got["grad"].tobytes() == want["grad"].tobytes()


@pytest.mark.parametrize("offset", (1, 2, 3))
@pytest.mark.parametrize("case", ("m3k81", "m5k2", "r3m14"))
def test_gradient_off_a_16_byte_boundary(case, offset):
    """the single words at the two ends of every row's flat range: the bits of the aligned call, guard words untouched"""
    c = mr.make_loss_case(case)
    want = call(c)
    got = call(c, offset=offset)
    assert got["loss"].tobytes() == want["loss"].tobytes() and got["grad"].tobytes() == want["grad"].tobytes()


def test_repeat_and_capture_at_the_flagship_size():
    """Rm = 1024 (B = 8, 128 fg rows), M = 28, K = 81: two eager calls and two graph replays over refilled buffers, the same bits"""
    from detectorch_amd import hip_mask
    Rm, K, M = 1024, 81, 28
    gen = torch.Generator(device="cuda").manual_seed(7)
    logits = torch.randn((Rm, K, M, M), device="cuda", generator=gen) * 3
    masks = torch.randint(-1, 2, (Rm, M * M), device="cuda", generator=gen, dtype=torch.int32)
    cls = torch.randint(0, K, (Rm,), device="cuda", generator=gen, dtype=torch.int32)
    out, arenas = fresh(Rm, K, M)
    snap = lambda: (out["loss"].cpu().numpy().tobytes(), int(out["n_valid"].cpu()[0]), out["grad_mask_logits"].clone())
    runs = []
    for _ in range(2):
        stale(out, arenas)
        hip_mask.mask_loss(logits, masks, cls, out=out)
        torch.cuda.synchronize()
        runs.append(snap())
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            hip_mask.mask_loss(logits, masks, cls, out=out)
    for _ in range(2):
        stale(out, arenas)
        graph.replay()
        torch.cuda.synchronize()
        runs.append(snap())
    for other in runs[1:]:
        assert other[0] == runs[0][0] and other[1] == runs[0][1] and torch.equal(other[2].view(torch.int32), runs[0][2].view(torch.int32))
    assert bool((arenas["grad"][-GUARD:] == -1).all())
    # against torch on the same device, in float64
    rows = torch.arange(Rm, device="cuda")
    x = logits.reshape(Rm, K, M * M)[rows, cls.long()].double()
    valid = masks >= 0
    want = torch.nn.functional.binary_cross_entropy_with_logits(x[valid], masks[valid].double(), reduction="sum") / valid.sum()
    assert runs[0][1] == int(valid.sum()) and abs(float(out["loss"][0]) - float(want)) <= 32 * mr.EPS * max(float(want), float(x[valid].abs().max()))


def test_autograd_against_torch_autograd_of_the_restatement():
    from detectorch_amd.model.loss import mask_rcnn_loss
    c = mr.make_loss_case("r65m7")
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    Rm, K, M, _ = c["logits"].shape
    x = dev(c["logits"], torch.float32).requires_grad_()
    blobs = dict(masks_int32=dev(c["masks"], torch.int32).reshape(5, 13, M * M), mask_class_labels=dev(c["cls"], torch.int32).reshape(5, 13))
    loss = mask_rcnn_loss(x, blobs)
    (loss * 3.0).backward()
    x64 = dev(c["logits"], torch.float64).requires_grad_()
    cls, masks = dev(c["cls"], torch.int64), dev(c["masks"], torch.int64)
    ok = (cls >= 0) & (cls < K)
    sel = x64.reshape(Rm, K, M * M)[torch.arange(Rm, device="cuda")[ok], cls[ok]]
    t = masks[ok]
    valid = (t == 0) | (t == 1)
    xv, tv = sel[valid], t[valid].double()
    want = (xv.clamp(min=0) - xv * tv + torch.log1p(torch.exp(-xv.abs()))).sum() / valid.sum()         # the restatement's formula
    (want * 3.0).backward()
    n = int(valid.sum())
    assert abs(float(loss) - float(want)) <= 32 * mr.EPS * max(float(want), float(xv.abs().max()))
    d = float((x.grad.double() - x64.grad).abs().max())
    print("autograd: gradient %.3f of its bound" % (d / (16 * mr.EPS * 3.0 / n)))
    assert d <= 16 * mr.EPS * 3.0 / n and torch.equal(x.grad == 0, x64.grad == 0)
