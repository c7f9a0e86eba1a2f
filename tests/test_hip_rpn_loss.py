"""dtc_rpn_loss and model.loss.rpn_losses on the MI355X (-m gpu) against the float64 yardstick of tests/rpn_train_ref.py (pinned to
torch's and the reference's own float64 chain by tests/test_rpn_train_host.py).  The bounds are those of tests/README_loss.md:
loss max(4 e_ref, 32 eps scale), grad_cls_logits absolute 16 eps |upstream| / n_valid, grad_bbox_pred relative 8 eps, every promised
zero exact.  Every distance is printed in units of its bound.  Outputs are pre-filled with 0xFF and followed by guard words."""
import numpy as np
import pytest
import torch

from conftest import golden
import rpn_train_ref as rr
from test_hip_rpn_targets import GUARD, ff

pytestmark = pytest.mark.gpu
BETA = float(np.float32(1.0 / 9.0))
WORST = {}


@pytest.fixture(scope="module")
def g():
    return golden("rpn_train")


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dt).contiguous()


def run_loss(c, beta=BETA, upstream=None, g_cls=True, g_box=True, out=None):
    """-> dict(losses [2], n_valid, grad_cls / grad_box: lists of arrays or None) from one dtc_rpn_loss call on case c"""
    from detectorch_amd import hip_rpn
    f32, i32 = torch.float32, torch.int32
    cls, box = [dev(x, f32) for x in c["cls"]], [dev(x, f32) for x in c["box"]]
    gc = [ff(x.shape, f32) for x in cls] if g_cls else None
    gb = [ff(x.shape, f32) for x in box] if g_box else None
    levels, B, N = hip_rpn.map_levels(cls, box, [t for t, _ in gc] if gc else None, [t for t, _ in gb] if gb else None)
    if out is None:
        out = hip_rpn.loss_outputs(levels, B, "cuda")
        out["workspace"].fill_(0xFF)
        out["losses"].view(i32).fill_(-1)
        out["n_valid"].fill_(-1)
    up = None if upstream is None else dev(np.asarray(upstream, np.float32), f32)
    hip_rpn.rpn_loss(levels, dev(c["labels"], i32), dev(c["fg_index"], i32), dev(c["fg_targets"], f32), dev(c["n_fg"], i32),
                     dev(c["n_bg"], i32), beta=beta, upstream=up, out=out)
    torch.cuda.synchronize()
    for lst in (gc, gb):
        for _, full in lst or ():
            assert bool((full[-GUARD:] == -1).all())
    return dict(losses=out["losses"].cpu().numpy(), n_valid=int(out["n_valid"][0]),
                grad_cls=[t.cpu().numpy() for t, _ in gc] if gc else None, grad_box=[t.cpu().numpy() for t, _ in gb] if gb else None)


def compare(got, c, beta=BETA, upstream=None, e_ref=(0.0, 0.0), what=""):
    up = (1.0, 1.0) if upstream is None else tuple(float(np.float32(u)) for u in upstream)
    y = rr.y_of(c, beta, up)
    b = rr.loss_bounds(y, *e_ref)
    assert got["n_valid"] == y["n_valid"]
    d = {"loss_cls": abs(float(got["losses"][0]) - y["loss_cls"]) / b["loss_cls"] if b["loss_cls"] else 2.0 * float(got["losses"][0] != 0),
         "loss_bbox": abs(float(got["losses"][1]) - y["loss_bbox"]) / b["loss_bbox"] if b["loss_bbox"] else 2.0 * float(got["losses"][1] != 0),
         "grad_cls": 0.0, "grad_box": 0.0}
    for l in range(len(c["spec"])):
        if got["grad_cls"] is not None:
            mine, want = got["grad_cls"][l].astype(np.float64), y["grad_cls"][l]
            if up[0] != 0:
                d["grad_cls"] = max(d["grad_cls"], float(np.abs(mine - want).max(initial=0.0)) / (b["grad_cls"] * abs(up[0])))
            else:
                assert not mine.any()
            lab = c["labels"][:, rr.offsets(c["spec"])[l]:rr.offsets(c["spec"])[l + 1]].reshape(mine.shape)
            ignored = (lab != 0) & (lab != 1)
            assert not got["grad_cls"][l][ignored].any() and not np.signbit(got["grad_cls"][l][ignored]).any()   # +0.0
        if got["grad_box"] is not None:
            mine, want = got["grad_box"][l].astype(np.float64), y["grad_box"][l]
            z = want == 0
            if up[1] != 0:
                assert not got["grad_box"][l][z].any() and not np.signbit(got["grad_box"][l][z]).any()
                if (~z).any():
                    d["grad_box"] = max(d["grad_box"], float((np.abs(mine - want)[~z] / np.abs(want[~z])).max()) / b["grad_box"])
            else:
                assert not mine.any()
    print("%-28s loss_cls %.3f loss_bbox %.3f grad_cls_logits %.3f grad_bbox_pred %.3f of their bounds" % (
        what, d["loss_cls"], d["loss_bbox"], d["grad_cls"], d["grad_box"]))
    for k, v in d.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= 1.0, (what, k, v)
    return y


@pytest.mark.parametrize("name", [n for n in rr.LOSS_CASES if n != "fpn"])
def test_sizes_and_the_five_level_layout(g, name):
    c = rr.make_loss_case(name)
    e_ref = (float(g["loss_%s_e_ref_cls" % name]), float(g["loss_%s_e_ref_box" % name]))
    y = compare(run_loss(c), c, e_ref=e_ref, what=name)
    assert abs(y["loss_cls"] - float(g["loss_%s_cls" % name])) <= 1e-12 * max(1.0, y["loss_cls"])     # the recorded yardstick


def small(labels, logits=None, n_bg=None, F=4):
    """one level of 1 x 4 x 8 = 32 anchors, B = 1, with the given labels; fg rows: the anchors labelled 1, at most F"""
    spec = rr.single(1, 4, 8)
    rs = np.random.RandomState(11)
    labels = np.asarray(labels, np.int64).astype(np.int32).reshape(1, 32)
    fg = np.where(labels[0] == 1)[0][:F]
    fg_index = np.full((1, F), -1, np.int32)
    fg_index[0, :len(fg)] = fg
    cls = rs.standard_normal((1, 1, 4, 8)).astype(np.float32) if logits is None else np.asarray(logits, np.float32).reshape(1, 1, 4, 8)
    n_valid = int(np.sum((labels == 0) | (labels == 1)))
    return dict(spec=spec, cls=[cls], box=[(rs.standard_normal((1, 4, 4, 8)) * 0.3).astype(np.float32)], labels=labels,
                fg_index=fg_index, fg_targets=(rs.standard_normal((1, F, 4)) * 0.3).astype(np.float32),
                n_fg=np.array([len(fg)], np.int32), n_bg=np.array([n_valid - len(fg) if n_bg is None else n_bg], np.int32))


def test_extreme_logits():
    vals = [0.0] + [s * v for v in (1e-40, 16.7, 88.0, 104.0, 1e4, 3e38) for s in (1, -1)]
    x = np.zeros(32, np.float32)
    x[:26] = np.repeat(np.asarray(vals, np.float32), 2)
    labels = np.full(32, -1)
    labels[:26] = [0, 1] * 13
    c = small(labels, x, F=16)
    c["fg_index"][:], c["n_fg"][:], c["n_bg"][:] = -1, 0, 26                    # the classification term alone
    for up in (None, (-2.0, 0.25)):
        got = run_loss(c, upstream=up)
        compare(got, c, upstream=up, what="extreme logits, upstream %s" % (up,))
        assert np.isfinite(got["losses"]).all() and got["n_valid"] == 26
        gc, u = got["grad_cls"][0].ravel(), 1.0 if up is None else up[0]
        unit = np.float32(u / 26.0)
        for i in range(26):
            if abs(x[i]) >= 1e4:                                                # saturated: exactly 0 or -+ upstream / n_valid
                assert gc[i] == (np.float32(0) if (x[i] > 0) == (labels[i] == 1) else (unit if x[i] > 0 else -unit)), (x[i], labels[i])


def test_ignored_labels():
    c = small(np.full(32, -1))
    got = run_loss(c)
    compare(got, c, what="all labels ignored")
    assert not got["losses"].any() and got["n_valid"] == 0 and not got["grad_cls"][0].any() and not got["grad_box"][0].any()
    labels = np.array([1, 0, 2, -7, -2 ** 31, 0, 1, 3] * 4)
    c = small(labels, n_bg=8)
    c["cls"][0].ravel()[[2, 3, 4, 7]] = [50.0, -50.0, 30.0, 1e30]               # what a mask `label >= 0` would have counted
    got = run_loss(c)
    y = compare(got, c, what="labels 2, -7, INT_MIN")
    assert got["n_valid"] == 12 and y["loss_cls"] < 5.0
    bad = ~np.isin(labels, (0, 1)).reshape(1, 1, 4, 8)
    assert not got["grad_cls"][0][bad].any()


def test_smooth_l1_boundary():
    b32 = np.float32(1.0 / 9.0)
    ds = [b32, -b32, np.nextafter(b32, np.float32(1)), np.nextafter(b32, np.float32(0)), -np.nextafter(b32, np.float32(1)),
          -np.nextafter(b32, np.float32(0)), np.float32(0), np.float32(1e-30)]
    labels = np.full(32, -1)
    labels[:2], labels[2:6] = 1, 0
    c = small(labels, F=2)
    c["fg_targets"][:] = 0
    for j, i in enumerate(c["fg_index"][0]):
        c["box"][0][0, :, i // 8, i % 8] = ds[4 * j:4 * j + 4]
    got = run_loss(c, beta=float(b32), upstream=(1.0, 1.0))
    y = compare(got, c, beta=float(b32), upstream=(1.0, 1.0), what="residuals at +-beta and their neighbours")
    gb = got["grad_box"][0]
    unit = 1.0 / 6.0                                                            # 1 / (n_fg + n_bg) / B
    i0 = c["fg_index"][0, 0]
    assert gb[0, 0, i0 // 8, i0 % 8] == np.float32(unit) and gb[0, 1, i0 // 8, i0 % 8] == np.float32(-unit)     # x / beta = +-1 at the boundary
    assert gb[0, 2, i0 // 8, i0 % 8] == np.float32(unit)                        # above beta: the linear arm, sign(x)


def test_fg_rows_counts_and_indices():
    labels = np.full(32, 0)
    labels[[3, 9, 17, 30]] = 1
    c = small(labels)
    compare(run_loss(c), c, what="n_fg = F")
    none = dict(c, n_fg=np.array([0], np.int32))
    got = run_loss(none)
    compare(got, none, what="n_fg = 0")
    assert got["losses"][1] == 0 and not got["grad_box"][0].any()
    for bad in (-1, 32, 2 ** 30):
        skip = dict(c, fg_index=c["fg_index"].copy())
        skip["fg_index"][0, 1] = bad
        got = run_loss(skip)
        compare(got, skip, what="fg_index %d" % bad)
        assert not got["grad_box"][0][0, :, 9 // 8, 9 % 8].any()                # the row that was replaced has no gradient
    over = dict(c, n_fg=np.array([7], np.int32))                                # clamped to F
    compare(run_loss(over), over, what="n_fg above F")


def test_upstream_and_loss_only():
    c = rr.make_loss_case("n257")
    base = run_loss(c)
    for up in ((0.0, 0.0), (-2.0, 0.25), None):
        got = run_loss(c, upstream=up)
        compare(got, c, upstream=up, what="upstream %s" % (up,))
        assert rr.same_bits(got["losses"], base["losses"])                      # upstream scales the gradients only
    for g_cls, g_box in ((False, False), (True, False), (False, True)):
        got = run_loss(c, g_cls=g_cls, g_box=g_box)
        assert rr.same_bits(got["losses"], base["losses"]) and got["n_valid"] == base["n_valid"]
        for k, on in (("grad_cls", g_cls), ("grad_box", g_box)):
            assert (got[k] is None) if not on else all(rr.same_bits(a, b) for a, b in zip(got[k], base[k]))


def repeat_and_capture(c):
    """two eager calls and two graph replays over outputs and workspace refilled with 0xFF, bit-identical -> (the first, B, N)"""
    from detectorch_amd import hip_rpn
    f32, i32 = torch.float32, torch.int32
    cls, box = [dev(x, f32) for x in c["cls"]], [dev(x, f32) for x in c["box"]]
    gc, gb = [torch.empty_like(x) for x in cls], [torch.empty_like(x) for x in box]
    levels, B, N = hip_rpn.map_levels(cls, box, gc, gb)
    args = [dev(c["labels"], i32), dev(c["fg_index"], i32), dev(c["fg_targets"], f32), dev(c["n_fg"], i32), dev(c["n_bg"], i32)]
    out = hip_rpn.loss_outputs(levels, B, "cuda")
    snap = lambda: [out["losses"].cpu().numpy().copy(), out["n_valid"].cpu().numpy().copy()] + [t.cpu().numpy().copy() for t in gc + gb]

    def stale():
        for t in gc + gb + [out["losses"]]:
            t.view(i32).fill_(-1)
        out["workspace"].fill_(0xFF)
    runs = []
    for _ in range(2):
        stale()
        hip_rpn.rpn_loss(levels, *args, beta=BETA, out=out)
        torch.cuda.synchronize()
        runs.append(snap())
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            hip_rpn.rpn_loss(levels, *args, beta=BETA, out=out)
    for _ in range(2):
        stale()
        graph.replay()
        torch.cuda.synchronize()
        runs.append(snap())
    for other in runs[1:]:
        assert all(rr.same_bits(a, b) for a, b in zip(runs[0], other))
    return dict(losses=runs[0][0], n_valid=int(runs[0][1][0]), grad_cls=runs[0][2:2 + len(gc)], grad_box=runs[0][2 + len(gc):]), B, N


def test_repeat_and_capture_at_full_size(g):
    c = rr.make_loss_case("fpn")
    got, B, N = repeat_and_capture(c)
    assert (B, N) == (2, 121515)
    e_ref = (float(g["loss_fpn_e_ref_cls"]), float(g["loss_fpn_e_ref_box"]))
    compare(got, c, e_ref=e_ref, what="fpn, B = 2")


# ---- past one round of each stride loop (rr.LOSS_BIG_CASES): against the float64 yardstick alone, e_ref = (0, 0) ----------------------
@pytest.mark.parametrize("name", sorted(rr.LOSS_BIG_SHAPES))
def test_dense_pass_past_one_round(name):
    c = rr.big_loss_case(name)
    compare(run_loss(c), c, what=name)


@pytest.mark.parametrize("name", ["rows_4096", "rows_300"])
def test_fg_rows_past_one_round(name):
    c = rr.big_loss_case(name)
    got = run_loss(c)
    compare(got, c, what=name)
    if name == "rows_4096":                                                     # the anchors named past n_fg have no gradient
        past = c["fg_index"][1, 2500:-3]
        assert not got["grad_box"][0][1].reshape(3, 4, 32 * 48)[past // (32 * 48), :, past % (32 * 48)].any()
        assert got["n_valid"] == 4096 + 2500 + int(c["n_bg"].sum())


@pytest.mark.parametrize("name", ["batch_257", "batch_600"])
def test_large_batches_and_clamped_counts(name):
    c = rr.big_loss_case(name)
    got = run_loss(c)
    compare(got, c, what=name)
    F = c["fg_index"].shape[1]
    assert got["n_valid"] == int((np.clip(c["n_fg"].astype(np.int64), 0, F) + np.maximum(c["n_bg"].astype(np.int64), 0)).sum())


def test_repeat_capture_and_loss_only_past_one_round():
    c = rr.big_loss_case("two_level")
    got, B, N = repeat_and_capture(c)
    assert B == 2 and N > rr.LOSS_DENSE_ROUND
    compare(got, c, what="two_level, repeated and replayed")
    only = run_loss(c, g_cls=False, g_box=False)
    assert rr.same_bits(only["losses"], got["losses"]) and only["n_valid"] == got["n_valid"]


def test_rpn_losses_autograd():
    from detectorch_amd.model.loss import rpn_losses
    c = rr.make_loss_case("fpn5")
    spec, B = c["spec"], 2
    f32, i32 = torch.float32, torch.int32
    cls = [dev(x, f32).requires_grad_() for x in c["cls"]]
    box = [dev(x, f32).requires_grad_() for x in c["box"]]
    blobs = dict(labels=dev(c["labels"], i32), fg_index=dev(c["fg_index"], i32), fg_targets=dev(c["fg_targets"], f32),
                 n_fg=dev(c["n_fg"], i32), n_bg=dev(c["n_bg"], i32))
    loss_cls, loss_bbox = rpn_losses(cls, box, blobs)
    (1.5 * loss_cls - 0.5 * loss_bbox).backward()
    # torch autograd of the float64 restatement on the same device tensors
    c64, b64 = [x.detach().double().requires_grad_() for x in cls], [x.detach().double().requires_grad_() for x in box]
    lab = blobs["labels"]
    flat = torch.cat([x.reshape(B, -1) for x in c64], 1)
    valid = (lab == 0) | (lab == 1)
    nv = (blobs["n_fg"] + blobs["n_bg"]).double()
    want_cls = torch.nn.functional.binary_cross_entropy_with_logits(flat[valid], (lab[valid] == 1).double(), reduction="sum") / nv.sum().clamp(min=1)
    off = rr.offsets(spec)
    want_box = 0.0
    for b in range(B):
        for j in range(int(c["n_fg"][b])):
            i = int(c["fg_index"][b, j])
            l = int(np.searchsorted(off, i, side="right") - 1)
            A, H, W = spec[l][:3]
            a, h, w = np.unravel_index(i - off[l], (A, H, W))
            d = b64[l][b, 4 * a:4 * a + 4, h, w] - blobs["fg_targets"][b, j].double()
            t = torch.where(d.abs() <= BETA, 0.5 * d * d / BETA, d.abs() - 0.5 * BETA)
            want_box = want_box + t.sum() / nv[b].clamp(min=1) / B
    (1.5 * want_cls - 0.5 * want_box).backward()
    torch.cuda.synchronize()
    y = rr.y_of(c)
    bnd = rr.loss_bounds(y)
    assert abs(float(loss_cls.detach()) - float(want_cls.detach())) <= bnd["loss_cls"]
    assert abs(float(loss_bbox.detach()) - float(want_box.detach())) <= bnd["loss_bbox"]
    for x, x64 in zip(cls, c64):
        d = float((x.grad.double() - x64.grad).abs().max()) / (bnd["grad_cls"] * 1.5)
        print("rpn_losses autograd: grad_cls_logits %.3f of its bound" % d)
        assert d <= 1.0 and x.grad.shape == x.shape
    for x, x64 in zip(box, b64):
        if x64.grad is None:                                                    # a level without a sampled foreground anchor
            assert not x.grad.any()
            continue
        nz = x64.grad != 0
        assert not x.grad[~nz].any()
        if nz.any():
            d = float(((x.grad.double() - x64.grad)[nz] / x64.grad[nz]).abs().max()) / bnd["grad_box"]
            print("rpn_losses autograd: grad_bbox_pred %.3f of its bound" % d)
            assert d <= 1.0


def test_print_the_largest_distances():
    print("largest distance per quantity over this module, in units of its bound: %s" % {k: round(v, 3) for k, v in WORST.items()})
