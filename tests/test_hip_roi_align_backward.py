"""dtc_roi_align_backward on the GPU (include/detectorch_grad_hip.h), through detectorch_amd.hip_grad and the autograd wrappers of
detectorch_amd.model.roi_align.  Every comparison of the native result is BITWISE: against the reference's own output where
tests/golden/roi_align_backward.npz records it, otherwise against the numpy restatement that tests/test_roi_align_backward_host.py
holds to that fixture (tests/roi_align_backward_ref.py).  Every output map is pre-filled with 0xFF bytes and followed by guard
words, the workspace is pre-filled too: an element the call does not write, or a word it writes past a map, shows.
tests/README_roi_align_backward.md says what each case is there for."""
import numpy as np
import pytest
import torch

from conftest import golden
import roi_align_backward_ref as rb

pytestmark = pytest.mark.gpu

GUARD = 64                                           # float32 words behind every map


@pytest.fixture(scope="module")
def g():
    return golden("roi_align_backward")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def outputs(c, channels=None):
    """dict(grads, workspace, raw): maps of 0xFF bytes with GUARD words behind each, a workspace of 0xFF bytes"""
    from detectorch_amd import hip, hip_grad
    ch = c["top"].shape[1] if channels is None else channels
    raw, grads = [], []
    for h, w in c["shapes"]:
        n = c["batch"] * ch * h * w
        buf = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
        raw.append(buf)
        grads.append(buf[:n].view(torch.float32).view(c["batch"], ch, h, w))
    need = hip.invoke(hip_grad.lib(), hip_grad.SIGNATURES, "dtc_roi_align_backward_workspace_bytes",
                      dict(n_levels=len(c["shapes"]), batch=c["batch"], n_rois=len(c["rois"])))
    assert need == rb.workspace_bytes(len(c["shapes"]), c["batch"], len(c["rois"]))
    return dict(grads=grads, workspace=torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda"), raw=raw)


def launch(c, out, top=None, rois=None, levels=None):
    from detectorch_amd import hip_grad
    top = dev(c["top"]) if top is None else top
    rois = dev(c["rois"]) if rois is None else rois
    levels = dev(c["levels"]) if levels is None else levels
    shapes = [(c["batch"], top.shape[1], h, w) for h, w in c["shapes"]]
    return hip_grad.roi_align_backward(top, rois, shapes, c["scales"], top.shape[2], top.shape[3], c["ratio"], roi_levels=levels,
                                       out=out)


def run(c):
    """-> the per-level results as numpy arrays; the guard words are checked"""
    out = outputs(c)
    res = launch(c, out)
    torch.cuda.synchronize()
    for buf in out["raw"]:
        assert bool((buf[-GUARD:] == -1).all()), "a word behind a map was written"
    return [r.cpu().numpy() for r in res]


def check_golden(g, name, got):
    c = rb.make_case(name)
    assert np.array_equal(rb.digest(c), g[name + "_digest"])
    ch = rb.sample_channels(name, c["top"].shape[1])
    for l in range(len(c["shapes"])):
        assert np.array_equal(bits(got[l][:, ch]), bits(g["%s_L%d" % (name, l)])), (name, l)


def check_restatement(c, got, want=None):
    want = rb.reference(c) if want is None else want
    for l in range(len(c["shapes"])):
        assert np.array_equal(bits(got[l]), bits(want[l][0])), l
    return want


def test_a_one_roi(g):
    c = rb.make_case("a")
    got = run(c)
    check_golden(g, "a", got)
    assert np.count_nonzero(got[0]) > 0 and np.count_nonzero(got[0] == 0) > 0


@pytest.mark.parametrize("channels", rb.CHANNEL_WIDTHS)
def test_b_channel_widths(g, channels):
    name = "b%d" % channels
    got = run(rb.make_case(name))
    check_golden(g, name, got)
    if channels > 65:                                # the fixture samples the wide cases: every channel against the restatement
        check_restatement(rb.make_case(name), got)


def test_c_adaptive_sampling(g):
    c = rb.make_case("c")
    grids = [rb.roi_geometry(r[1:], c["scales"][0], 14, 14, 0)[4:6] for r in c["rois"]]
    assert grids == c["grids"] and (1, 1) in grids and (5, 3) in grids
    check_golden(g, "c", run(c))


def test_d_map_edges_and_degenerate_boxes(g):
    check_golden(g, "d", run(rb.make_case("d")))


@pytest.mark.parametrize("name", rb.TILE_CASES)
def test_e_tile_boundaries(g, name):
    c = rb.make_case(name)
    got = run(c)
    if name in rb.GOLDEN_CASES:
        check_golden(g, name, got)
    check_restatement(c, got)


@pytest.mark.parametrize("name", ["f", "fsmall", "fbig"])
def test_f_pile_up_and_denormals(g, name):
    got = run(rb.make_case(name))
    check_golden(g, name, got)
    top = np.abs(got[0]).max()
    if name == "fsmall":
        assert 0 < top < np.finfo(np.float32).tiny   # denormal sums: kept, not flushed
        assert np.count_nonzero(got[0]) > 20
    if name == "fbig":
        assert 1e29 < top < np.inf


def test_g_multi_level_and_empty_groups(g):
    c = rb.make_case("g")
    got = run(c)
    check_golden(g, "g", got)
    assert not got[2].any() and not got[3][1].any() and got[3][0].any()      # zeros over the 0xFF where no RoI is
    assert np.array_equal(bits(got[2]), np.zeros_like(bits(got[2])))          # +0.0
    c4 = rb.make_case("g4")
    got4 = run(c4)
    check_golden(g, "g4", got4)
    assert got4[0][0].any() and not got4[0][1].any()


def test_h_bad_rois_contribute_nothing():
    c = rb.make_case("h")
    got = run(c)
    good = [r for r in range(len(c["rois"])) if r not in c["bad_rows"]]
    clean = dict(c, top=c["top"][good], rois=c["rois"][good], levels=c["levels"][good])
    assert not [r for r in good if rb.is_bad(c["rois"][r], c["levels"][r], 2, 2)] and len(good) == 13
    check_restatement(clean, got)                    # the bits of the call without them ...
    check_restatement(clean, run(clean))             # ... computed either way
    check_restatement(c, got)                        # (and the restatement's own rule for bad rows says the same)


def test_i_middle_sized(g):
    check_golden(g, "i", run(rb.make_case("i")))


def test_j_determinism_and_capture():
    c = rb.make_case("g")
    top, rois, levels = dev(c["top"]), dev(c["rois"]), dev(c["levels"])
    outs = [outputs(c) for _ in range(3)]
    first = [r.clone() for r in launch(c, outs[0], top, rois, levels)]
    second = launch(c, outs[1], top, rois, levels)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, second))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(c, outs[2], top, rois, levels)
    replays = []
    for _ in range(2):
        for buf in outs[2]["raw"]:
            buf.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        replays.append([r.clone() for r in outs[2]["grads"]])
    for rep in replays:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, rep))
    # other values in the same buffers: the replay reads them when it runs
    order = np.arange(len(c["rois"]))[::-1].copy()
    c2 = dict(c, top=np.ascontiguousarray(c["top"][order] * np.float32(0.5) + np.float32(0.25)), rois=c["rois"][order].copy(),
              levels=((c["levels"][order] + 1) % 4).astype(np.int32))
    c2["rois"][:, 1:] *= np.float32(0.5)
    top.copy_(dev(c2["top"])); rois.copy_(dev(c2["rois"])); levels.copy_(dev(c2["levels"]))
    for buf in outs[2]["raw"]:
        buf.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    eager = launch(c2, outs[0], top, rois, levels)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(eager, outs[2]["grads"]))
    check_restatement(c2, [r.cpu().numpy() for r in eager])
    assert any(not torch.equal(a, b) for a, b in zip(first, eager))


def forward64(features, tables, n_rois, pooled_h, pooled_w):
    """The forward pass in float64 torch ops on the taps of rb.forward_tables (the reference's float32 sample geometry; products
    and sums in float64) -> [R, C, PH, PW], differentiable with respect to features [B, C, H, W] float64."""
    t = torch.from_numpy(tables).to(features.device)
    n, ph, pw, b, y, x = (t[:, k].long() for k in range(6))
    vals = features[b, :, y, x] * (t[:, 6] * t[:, 7])[:, None]
    out = torch.zeros((n_rois * pooled_h * pooled_w, features.shape[1]), dtype=torch.float64, device=features.device)
    out = out.index_add(0, (n * pooled_h + ph) * pooled_w + pw, vals)
    return out.view(n_rois, pooled_h, pooled_w, -1).permute(0, 3, 1, 2)


def check_against_float64(g, name, native, feats64_grads, mags):
    """|native - float64 autograd| <= 4 e_ref eps sum|terms| on every element; prints the distance in those units"""
    e_ref = float(g["e_ref"])
    worst = 0.0
    for got, want, mag in zip(native, feats64_grads, mags):
        d = np.abs(got.astype(np.float64) - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(mag > 0, d / (rb.EPS * mag), 0.0))))
        assert np.all(d <= 4 * e_ref * rb.EPS * mag), name
    print("%s: native gradient lies %.3f eps*sum|terms| from float64 autograd (e_ref %.3f, bound %.3f)"
          % (name, worst, e_ref, 4 * e_ref))


def test_k_autograd_module_single_level(g):
    from detectorch_amd.model.roi_align import RoIAlign
    c = rb.make_case("b3")
    (h, w), scale = c["shapes"][0], c["scales"][0]
    feats = torch.randn(2, 3, h, w, device="cuda", requires_grad=True)
    rois = dev(c["rois"]).requires_grad_(True)
    out = RoIAlign(7, 7, scale, 2)(feats, rois)
    assert out.requires_grad and tuple(out.shape) == c["top"].shape
    out.backward(dev(c["top"]))
    assert rois.grad is None                                                       # rois gets no gradient
    assert feats.grad.dtype == torch.float32 and feats.grad.is_contiguous()
    native = feats.grad.cpu().numpy()
    assert np.array_equal(bits(native), bits(g["b3_L0"]))                           # the reference's own bits
    tables = rb.forward_tables(c["rois"], 2, h, w, scale, 7, 7, 2)
    f64 = feats.detach().double().requires_grad_(True)
    out64 = forward64(f64, tables, len(c["rois"]), 7, 7)
    assert float((out64.detach() - out.detach().double()).abs().max()) <= 1e-5      # the same forward
    out64.backward(dev(c["top"]).double())
    check_against_float64(g, "RoIAlign module (b3)", [native], [f64.grad.cpu().numpy()], [rb.reference(c)[0][2]])
    # nothing requires grad: nothing changes, backward is never reached
    plain = RoIAlign(7, 7, scale, 2)(feats.detach(), dev(c["rois"]))
    assert not plain.requires_grad and torch.equal(plain, out.detach())


def test_k_autograd_fpn_and_16_bit_channels_last(g):
    from detectorch_amd.model.roi_align import roi_align_fpn
    c = rb.make_case("k")
    feats = [torch.randn(2, 8, h, w, device="cuda", requires_grad=True) for h, w in c["shapes"]]
    rois, levels, top = dev(c["rois"]).requires_grad_(True), dev(c["levels"]), dev(c["top"])
    out = roi_align_fpn(feats, c["scales"], rois, levels, 7, 7, 2)
    out.backward(top)
    assert rois.grad is None
    native = [f.grad.cpu().numpy() for f in feats]
    want = check_restatement(c, native)
    f64 = [f.detach().double().requires_grad_(True) for f in feats]
    total = 0
    for l, ((h, w), s) in enumerate(zip(c["shapes"], c["scales"])):
        rows = np.where(c["levels"] == l)[0]
        o = forward64(f64[l], rb.forward_tables(c["rois"][rows], 2, h, w, s, 7, 7, 2), len(rows), 7, 7)
        assert float((o.detach() - out.detach()[torch.from_numpy(rows).cuda()].double()).abs().max()) <= 1e-5
        total = total + (o * top[torch.from_numpy(rows).cuda()].double()).sum()
    total.backward()
    check_against_float64(g, "roi_align_fpn (k)", native, [f.grad.cpu().numpy() for f in f64], [w[2] for w in want])
    # fp16 channels_last features: a gradient of their dtype and layout, the float32 result rounded once; only the maps that ask
    half = [f.detach().half().contiguous(memory_format=torch.channels_last) for f in feats]
    half[0].requires_grad_(True)
    out16 = roi_align_fpn(half, c["scales"], dev(c["rois"]), levels, 7, 7, 2)
    out16.backward(top)
    assert half[1].grad is None and half[0].grad.dtype == torch.float16
    assert half[0].grad.is_contiguous(memory_format=torch.channels_last) and not half[0].grad.is_contiguous()
    assert torch.equal(half[0].grad, torch.from_numpy(want[0][0]).cuda().half())


def test_l_bad_arguments_write_nothing():
    from detectorch_amd import hip, hip_grad
    c = rb.make_case("g")
    out = outputs(c)
    top, rois, levels = dev(c["top"]), dev(c["rois"]), dev(c["levels"])
    lv = (hip_grad.GradLevel * 9)()
    for k in range(9):
        t = out["grads"][min(k, 3)]
        lv[k] = hip_grad.GradLevel(t.data_ptr(), t.shape[2], t.shape[3], c["scales"][min(k, 3)], 0)
    base = dict(levels=lv, n_levels=4, batch=2, channels=3, rois=rois, roi_cols=5, roi_levels=levels, n_rois=30, pooled_h=7, pooled_w=7,
                sampling_ratio=2, grad_output=top, workspace=out["workspace"], workspace_bytes=out["workspace"].numel())
    off = (hip_grad.GradLevel * 4)(*[lv[k] for k in range(4)])
    off[1].grad += 4
    bad = [(dict(pooled_h=0), "DTC_EINVAL"), (dict(roi_cols=3), "DTC_EINVAL"), (dict(channels=0), "DTC_EINVAL"),
           (dict(n_levels=9), "DTC_EUNSUPPORTED"), (dict(sampling_ratio=1025), "DTC_EUNSUPPORTED"),
           (dict(pooled_w=1025), "DTC_EUNSUPPORTED"), (dict(n_levels=9, rois=None), "DTC_EUNSUPPORTED"),
           (dict(rois=None), "DTC_EINVAL"), (dict(grad_output=None), "DTC_EINVAL"), (dict(levels=off), "DTC_EINVAL"),
           (dict(workspace=out["workspace"][8:], workspace_bytes=out["workspace"].numel() - 8), "DTC_EINVAL"),
           (dict(workspace=None), "DTC_EWORKSPACE"), (dict(workspace_bytes=out["workspace"].numel() - 1), "DTC_EWORKSPACE")]
    for change, code in bad:
        with pytest.raises(RuntimeError, match=code):
            hip.invoke(hip_grad.lib(), hip_grad.SIGNATURES, "dtc_roi_align_backward", dict(base, **change))
    torch.cuda.synchronize()
    assert all(bool((buf == -1).all()) for buf in out["raw"]) and bool((out["workspace"] == 0xFF).all())
    hip.invoke(hip_grad.lib(), hip_grad.SIGNATURES, "dtc_roi_align_backward", dict(base))      # the same arguments, unchanged: fine
    torch.cuda.synchronize()
    check_restatement(c, [r.cpu().numpy() for r in out["grads"]])
    # n_rois == 0: all zeros
    empty = dict(c, top=c["top"][:0], rois=c["rois"][:0], levels=c["levels"][:0])
    assert all(np.array_equal(bits(r), np.zeros_like(bits(r))) for r in run(empty))
