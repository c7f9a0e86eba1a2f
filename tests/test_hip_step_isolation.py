"""Serving-loop isolation of the batched hot path: FpnRegionPath, C4RegionPath, OverlappedRegionPath and StepPipeline allocate their
buffers once (torch.empty, uint8 workspaces), bake the pointers into a hipGraph and get new data COPIED into the bound tensors
between steps.  Every stage writes fixed-stride rows plus a device-side count (pre_counts, keep_cnt, n_rois, det_count, m_n,
mask_bytes) and the next stage reads up to that count.  Pinned here:

  1. replays over CHANGING input sets (dense -> sparse -> crowded -> sparse' -> dense): after every step, what the header defines
     (contract_view) is bit-equal to a fresh path whose every internal buffer was zero-filled first -- stale rows of another input
     set, in outputs and workspaces, never leak into a step, and every padding row the header promises is rewritten;
  2. caller rows past the counts (cls_score / bbox_pred rows >= n_rois, masks rows >= det_count, RPN cells outside an image's
     extent) filled with values that WOULD change the result are ignored;
  3. each C entry point on its own, dense call then sparse call on the same workspace and outputs == a call on zero-filled ones;
  4. the resident decode of dtc_rpn_topk_decode_sized == its ticket decode (DTC_RPN_DECODE_TICKETS=1) on the same inputs.

Poison rule: nothing a kernel turns into an address, a count, a loop bound or a box coordinate is ever filled with arbitrary bits.
Stale state is what a valid step over ANOTHER input set left behind (in range by construction).  Value-only sentinels go into:
  box_feats / mask_feats: NaN          -- written by the RoIAlign kernels, read by no kernel of the path;
  crops / rle_str bytes: 0xAB          -- crops: read by dtc_mask_rle only inside each pasted rect; rle_str: read by no kernel;
  roi_scores / prop_scores: NaN        -- written by collect / gather_kept, read by no later kernel of the path.
Caller inputs are poisoned with finite values, NaN only in score arrays (cls_score rows past n_rois: read by det_candidates /
det_softmax_stats, masked by the count).  -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from detectorch_amd import synth

pytestmark = pytest.mark.gpu

B, C, C4_C = 4, 8, 16
SOFT_VOTE = dict(do_soft_nms=True, soft_nms_method="linear", do_bbox_vote=True, bbox_vote_thresh=0.8)
FULL = (synth.FPN_PAD_H, synth.FPN_PAD_W)
C4_FULL = (synth.IM_H, synth.IM_W)
# the tensors a caller binds (copied into between steps); everything else a path holds is its own output / workspace
BOUND = {"rpn_cls", "rpn_bbox", "feats", "feat", "cls_score", "bbox_pred", "masks", "sf", "im_size", "rpn_im_hw"}


def dev():
    return torch.device("cuda", 0)


# ---- input sets ---------------------------------------------------------------------------------------------------------------
def _to_logits(p):
    return torch.log(torch.clamp(p, min=1e-30))


def fpn_set(kind, seed, logits=False, perm=(0, 1, 2, 3)):
    """kind: 'dense' (synthetic_batch), 'sparse' (image roles: small extent, all background, normal, empty extent -- then permuted by
    perm: image perm[k] takes role k), 'crowded' (image 2: 10 classes tied at 0.1 on every roi -> det_count > max_out)."""
    from detectorch_amd.pipeline import synthetic_batch
    rpn_cls, rpn_bbox, feats, cls, bbox, masks, sf, im_size = synthetic_batch(B, dev(), seed=seed, channels=C)
    hw = [FULL] * B
    if kind == "sparse":
        small, bg, _, empty = perm
        hw[small], hw[empty] = (96, 160), (0, 0)
        im_size[small] = torch.tensor([96 / 1.6, 160 / 1.6])
        cls[bg].zero_()
        cls[bg, :, 0] = 1.0
    elif kind == "crowded":
        cls[2].zero_()
        cls[2, :, 1:11] = 0.1
    if logits:
        cls = _to_logits(cls)
    return dict(rpn_cls=rpn_cls, rpn_bbox=rpn_bbox, feats=feats, cls=cls.contiguous(), bbox=bbox, masks=masks, sf=sf,
                im_size=im_size, hw=torch.tensor(hw, dtype=torch.float32, device=dev()), hw_list=hw)


def c4_set(kind, seed):
    from detectorch_amd.pipeline import synthetic_c4_batch
    rpn_cls, rpn_bbox, feat, cls, bbox, sf, im_size = synthetic_c4_batch(B, dev(), seed=seed, channels=C4_C)
    hw = [C4_FULL] * B
    if kind == "sparse":
        hw[0], hw[3] = (96, 160), (160, 240)
        im_size[0] = torch.tensor([96 / 1.6, 160 / 1.6])
        im_size[3] = torch.tensor([160 / 1.6, 240 / 1.6])
        cls[1].zero_()
        cls[1, :, 0] = 1.0
    return dict(rpn_cls=[rpn_cls], rpn_bbox=[rpn_bbox], feats=[feat], cls=cls, bbox=bbox, masks=None, sf=sf, im_size=im_size,
                hw=torch.tensor(hw, dtype=torch.float32, device=dev()), hw_list=hw)


def make_fpn(mode, batch=B, **kw):
    from detectorch_amd.pipeline import FpnRegionPath
    rle = kw.pop("rle", False) or mode == "soft_vote_rle"
    return FpnRegionPath(batch, dev(), channels=C, cls_logits=mode == "logits", with_rle=rle,
                         det_options=SOFT_VOTE if mode.startswith("soft_vote") else None, **kw)


def make_c4(mode):
    from detectorch_amd.pipeline import C4RegionPath
    return C4RegionPath(B, dev(), channels=C4_C, det_options=SOFT_VOTE if mode.startswith("soft_vote") else None)


def bind(path, s):
    """bind CLONES of set s (the set's own tensors stay the source of later copies)"""
    cl = lambda x: [t.clone() for t in x] if isinstance(x, list) else x.clone()
    if hasattr(path, "bind_rpn"):
        path.bind_rpn(cl(s["rpn_cls"]), cl(s["rpn_bbox"]), cl(s["feats"]), im_hw=s["hw_list"])
        path.bind_heads(cl(s["cls"]), cl(s["bbox"]), cl(s["sf"]), cl(s["im_size"]))
        path.bind_masks(cl(s["masks"]))
    else:
        path.bind(cl(s["rpn_cls"][0]), cl(s["rpn_bbox"][0]), cl(s["feats"][0]), cl(s["cls"]), cl(s["bbox"]), cl(s["sf"]),
                  cl(s["im_size"]), im_hw=s["hw_list"])


def load(path, s):
    """copy set s into the tensors the path (and its captured graph) reads, on the current stream"""
    fpn = hasattr(path, "bind_rpn")
    dst = ([path.rpn_cls, path.rpn_bbox, path.feats] if fpn else [[path.rpn_cls], [path.rpn_bbox], [path.feat]])
    for d, k in zip(dst, ("rpn_cls", "rpn_bbox", "feats")):
        for a, b in zip(d, s[k]):
            a.copy_(b)
    path.cls_score.copy_(s["cls"]); path.bbox_pred.copy_(s["bbox"]); path.sf.copy_(s["sf"]); path.im_size.copy_(s["im_size"])
    if fpn:
        path.masks.copy_(s["masks"])
    path.rpn_im_hw.copy_(s["hw"])


def zero_internal(path):
    for k, v in vars(path).items():
        if isinstance(v, torch.Tensor) and k not in BOUND:
            v.zero_()


# ---- what the header defines after a step ------------------------------------------------------------------------------------
def contract_view(path, b):
    """image b's rows that include/detectorch_hip.h defines after a step, as host arrays keyed 'stage/buffer' (stage order =
    launch order, so the first mismatching key names the first stage that went wrong).  Padding rows the header promises are
    included (roi_levels / m_levels == -1, zero box / mask features, RLE 0 / 0); rows it leaves unspecified are not."""
    torch.cuda.synchronize()
    h = lambda t: t.detach().cpu().numpy()
    v = {}
    L = path.pre_counts.shape[0] // path.B
    for l in range(L):
        s = b * L + l
        pc = int(path.pre_counts[s])
        v["rpn/pre_counts%d" % l] = np.array(pc)
        v["rpn/pre_boxes%d" % l], v["rpn/pre_scores%d" % l] = h(path.pre_boxes[s, :pc]), h(path.pre_scores[s, :pc])
        kc = int(path.keep_cnt[s])
        v["nms/keep_cnt%d" % l], v["nms/keep%d" % l] = np.array(kc), h(path.keep[s, :kc])
    pb, ps = path.prop_boxes, path.prop_scores          # (FpnRegionPath: gathered on demand from the NMS output)
    torch.cuda.synchronize()
    for l in range(L):
        s, kc = b * L + l, int(path.keep_cnt[b * L + l])
        v["nms/prop_boxes%d" % l], v["nms/prop_scores%d" % l] = h(pb[s, :kc]), h(ps[s, :kc])
    n, T = int(path.n_rois[b]), path.top_n
    v["collect/n_rois"] = np.array(n)
    for k in ("rois5", "idx_restore", "rois_by_level"):
        v["collect/" + k] = h(getattr(path, k)[b, :n])
    v["collect/roi_levels"] = h(path.roi_levels[b])                 # rows >= n_rois: -1
    v["collect/level_counts"] = h(path.level_counts[b])
    v["box/box_feats"] = h(path.box_feats[b * T:(b + 1) * T])       # rows >= n_rois: zeros
    dc, Do = int(path.det_count[b]), path.max_out
    D = min(dc, Do)
    v["det/det_count"] = np.array(dc)
    for k in ("dets", "det_roi", "det_scaled"):
        v["det/" + k] = h(getattr(path, k)[b, :D])
    if not hasattr(path, "m_levels"):
        return v
    v["maskmap/m_n"] = np.array(int(path.m_n[b]))
    v["maskmap/m_levels"] = h(path.m_levels[b])                     # rows >= D: -1
    v["maskmap/m_rois5"] = h(path.m_rois5[b, :D])
    v["maskfeat/mask_feats"] = h(path.mask_feats[b * Do:(b + 1) * Do])   # rows >= D: zeros
    nbytes = int(path.mask_bytes[b])
    v["paste/mask_bytes"] = np.array(nbytes)
    for k in ("mask_boxes", "mask_rects", "mask_offsets"):
        v["paste/" + k] = h(getattr(path, k)[b, :D])
    crops, rects, offs = h(path.crops[b]), v["paste/mask_rects"], v["paste/mask_offsets"]
    pieces = []
    for d in range(D):
        x0, y0, x1, y1 = (int(c) for c in rects[d])
        a = max(x1 - x0, 0) * max(y1 - y0, 0)
        if offs[d] >= 0 and offs[d] + a <= path.crop_capacity:
            pieces.append(crops[offs[d]:offs[d] + a])
    v["paste/crops"] = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    if path.with_rle:
        v["rle/n_runs"], v["rle/str_len"] = h(path.rle_n_runs[b]), h(path.rle_str_len[b])   # d >= det_count: 0 / 0
        lens = v["rle/str_len"]
        v["rle/str"] = np.concatenate([h(path.rle_str[b, d, :max(int(lens[d]), 0)]) for d in range(D)] + [np.zeros(0, np.uint8)])
    return v


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_views_equal(got, want, tag, stage=None):
    assert got.keys() == want.keys(), tag
    for k in want:
        if stage is not None and k.split("/")[0] not in stage:
            continue
        g, w = _bits(got[k]), _bits(want[k])
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differs (shape %s vs %s)" % (tag, k, g.shape, w.shape)


def check_padding(view, T, Do):
    """the padding promises on their own (a failure here names the broken promise, not only 'differs from fresh')"""
    n, D = int(view["collect/n_rois"]), min(int(view["det/det_count"]), Do)
    assert (view["collect/roi_levels"][n:] == -1).all()
    assert not _bits(view["box/box_feats"][n:]).any()
    if "maskmap/m_levels" in view:
        assert (view["maskmap/m_levels"][D:] == -1).all()
        assert not _bits(view["maskfeat/mask_feats"][D:]).any()
    if "rle/n_runs" in view:
        assert not view["rle/n_runs"][D:].any() and not view["rle/str_len"][D:].any()


def fresh_views(make, s):
    """a NEW path, every internal buffer zero-filled, one eager step on set s"""
    p = make()
    bind(p, s)
    zero_internal(p)
    p.step(use_graph=False)
    torch.cuda.synchronize()
    return [contract_view(p, b) for b in range(p.B)]


def _host(s, b, key):
    x = s[key]
    return [t[b].cpu().numpy() for t in x] if isinstance(x, list) else x[b].cpu().numpy()


def oracle_anchor(path, s, b):
    """image b of the path == the oracle chain on set s (prop_hw = the image's own extent)"""
    import chain
    D = path.max_out
    ref = chain.fpn_hot_path(_host(s, b, "rpn_cls"), _host(s, b, "rpn_bbox"), [f[b:b + 1].cpu().numpy() for f in s["feats"]],
                             _host(s, b, "cls"), _host(s, b, "bbox"), s["masks"][b * D:(b + 1) * D].cpu().numpy(),
                             float(s["sf"][b]), _host(s, b, "im_size"), path.pad_h, path.pad_w, prop_hw=s["hw_list"][b])
    im = s["im_size"][b]
    assert chain.compare_with_gpu(path, b, ref, int(im[0]), int(im[1]))
    return ref


# ---- 1. replays over changing input sets ----------------------------------------------------------------------------------
def fpn_sequence(logits):
    return [("dense", fpn_set("dense", 3000, logits)), ("sparse", fpn_set("sparse", 3500, logits)),
            ("crowded", fpn_set("crowded", 3600, logits)), ("sparse'", fpn_set("sparse", 3700, logits, perm=(2, 3, 0, 1))),
            ("dense", fpn_set("dense", 3000, logits))]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("mode", ["hard", "logits", "soft_vote_rle"])
def test_fpn_replay_sequence(oracle, mode, use_graph):
    seq = fpn_sequence(mode == "logits")
    path = make_fpn(mode)
    bind(path, seq[0][1])
    for i, (name, s) in enumerate(seq):
        if i:
            load(path, s)
        path.step(use_graph=use_graph)
        torch.cuda.synchronize()
        want = fresh_views(lambda: make_fpn(mode), s)
        for b in range(B):
            got = contract_view(path, b)
            assert_views_equal(got, want[b], "step %d (%s) image %d" % (i, name, b))
            check_padding(got, path.top_n, path.max_out)
        counts = [int(path.det_count[b]) for b in range(B)]
        if name == "dense":
            assert min(counts) >= 100 and int(path.n_rois.min()) == path.top_n
        elif name.startswith("sparse"):
            small, bg, _, empty = (0, 1, 2, 3) if name == "sparse" else (2, 3, 0, 1)
            assert counts[bg] == 0 and int(path.n_rois[empty]) == 0 and 0 < int(path.n_rois[small]) < path.top_n
            assert min(int(path.level_counts[small].min()), 2) <= 1            # some level list of the small image: 0 or 1 rois
        elif mode != "soft_vote_rle":
            assert counts[2] > path.max_out
        if mode == "hard" and name == "sparse":
            oracle_anchor(path, s, 0)
        if mode == "hard" and i == len(seq) - 1:
            oracle_anchor(path, s, 1)


@pytest.mark.parametrize("use_graph", [True], ids=["graph"])
def test_c4_replay_sequence(oracle, use_graph):
    seq = [("dense", c4_set("dense", 2000)), ("sparse", c4_set("sparse", 2200)), ("dense", c4_set("dense", 2300))]
    path = make_c4("hard")
    bind(path, seq[0][1])
    for i, (name, s) in enumerate(seq):
        if i:
            load(path, s)
        path.step(use_graph=use_graph)
        torch.cuda.synchronize()
        want = fresh_views(lambda: make_c4("hard"), s)
        for b in range(B):
            got = contract_view(path, b)
            assert_views_equal(got, want[b], "step %d (%s) image %d" % (i, name, b))
            check_padding(got, path.top_n, path.max_out)
        if name == "sparse":
            assert int(path.det_count[1]) == 0 and 0 < int(path.n_rois[0]) < path.top_n


def test_overlapped_replay_sequence():
    from detectorch_amd.pipeline import OverlappedRegionPath
    dense, sparse = fpn_set("dense", 3000), fpn_set("sparse", 3500)
    ov = OverlappedRegionPath(B, dev(), n_split=2, channels=C)
    k = B // 2
    ov.bind(*[[t.clone() for t in dense[x]] for x in ("rpn_cls", "rpn_bbox", "feats")],
            *[dense[x].clone() for x in ("cls", "bbox", "masks", "sf", "im_size")])
    for i, p in enumerate(ov.sub):        # per-image sizes in a device tensor the graph reads (the sub-paths' own API)
        p.bind_rpn(p.rpn_cls, p.rpn_bbox, p.feats, im_hw=dense["hw_list"][i * k:(i + 1) * k])
    for step, s in enumerate((dense, sparse)):
        if step:
            for i, p in enumerate(ov.sub):
                load(p, half(s, i, k, p.max_out))
        ov.step(use_graph=True)
        torch.cuda.synchronize()
        for i, p in enumerate(ov.sub):
            want = fresh_views(lambda: make_fpn("hard", batch=k), half(s, i, k, p.max_out))
            for b in range(k):
                assert_views_equal(contract_view(p, b), want[b], "step %d sub %d image %d" % (step, i, b))


def half(s, i, k, max_out):
    sl = slice(i * k, (i + 1) * k)
    h = {x: [t[sl] for t in s[x]] for x in ("rpn_cls", "rpn_bbox", "feats")}
    h.update({x: s[x][sl] for x in ("cls", "bbox", "sf", "im_size", "hw")})
    h["masks"] = s["masks"][i * k * max_out:(i + 1) * k * max_out]
    h["hw_list"] = s["hw_list"][sl]
    return h


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_step_pipeline_alternating_sets(use_graph):
    """two paths, 6 steps in flight; path j's bound inputs alternate between sets[j][0] and sets[j][1], refilled on the path's own
    stream behind its previous step (StepPipeline.step's contract)"""
    from detectorch_amd.pipeline import StepPipeline
    sets = [(fpn_set("dense", 3300), fpn_set("sparse", 3310)), (fpn_set("sparse", 3320, perm=(3, 2, 1, 0)), fpn_set("crowded", 3330))]
    paths = []
    for j in range(2):
        p = make_fpn("hard")
        bind(p, sets[j][0])
        paths.append(p)
    torch.cuda.synchronize()
    pipe = StepPipeline(paths, dev(), n_inflight=2)
    last = [None, None]
    for i in range(6):
        j, k = i % 2, i // 2
        if k:
            with torch.cuda.stream(last[j]):
                load(paths[j], sets[j][k % 2])
        _, st = pipe.step(use_graph=use_graph)
        last[j] = st
    pipe.synchronize()
    torch.cuda.synchronize()
    for j in range(2):
        want = fresh_views(lambda: make_fpn("hard"), sets[j][0])          # 3 steps per path: set 0, set 1, set 0
        for b in range(B):
            assert_views_equal(contract_view(paths[j], b), want[b], "path %d image %d" % (j, b))


def fill_sentinels(path):
    path.box_feats.fill_(float("nan"))
    path.mask_feats.fill_(float("nan"))
    path.crops.fill_(0xAB)
    path.rle_str.fill_(0xAB)
    path.roi_scores.fill_(float("nan"))
    path._prop_scores.fill_(float("nan"))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_value_sentinels_in_outputs(use_graph):
    s = fpn_set("sparse", 3800)
    want = fresh_views(lambda: make_fpn("hard", rle=True), s)
    path = make_fpn("hard", rle=True)
    bind(path, s)
    if use_graph:
        path.step(use_graph=True)             # warm-up + capture (+ one replay)
        torch.cuda.synchronize()
    fill_sentinels(path)                      # between capture and replay
    path.step(use_graph=use_graph)
    for b in range(B):
        got = contract_view(path, b)
        assert_views_equal(got, want[b], "image %d" % b)
        check_padding(got, path.top_n, path.max_out)


# ---- 2. caller rows past the counts ----------------------------------------------------------------------------------------
def poison_caller_rows(s, view, fill, strides, logits=False):
    """a copy of set s whose rows past the counts (taken from the clean run's view) hold values that would change the result"""
    p = {k: ([t.clone() for t in v] if k in ("rpn_cls", "rpn_bbox", "feats") else v.clone() if isinstance(v, torch.Tensor) else v)
         for k, v in s.items()}
    for b in range(B):
        n = int(view[b]["collect/n_rois"])
        if fill == "nan":
            p["cls"][b, n:] = float("nan")
        elif logits:
            p["cls"][b, n:] = 0.0
            p["cls"][b, n:, 7] = 30.0
        else:
            p["cls"][b, n:, 1:] = 1.0
        p["bbox"][b, n:] = 3.0
        p["bbox"][b, n:, 1::2] = -3.0
        if p["masks"] is not None:
            Do = p["masks"].shape[0] // B
            d = min(int(view[b]["det/det_count"]), Do)
            p["masks"][b * Do + d:(b + 1) * Do] = 1.0
        h, w = s["hw_list"][b]
        for m, dl, st in zip(p["rpn_cls"], p["rpn_bbox"], strides):
            out = torch.ones(m.shape[2:], dtype=torch.bool, device=m.device)
            out[:-(-int(h) // st), :-(-int(w) // st)] = False
            m[b][:, out] = 0.99
            sign = torch.ones(dl.shape[1], device=dl.device)
            sign[1::2] = -1.0
            dl[b][:, out] = 3.0 * sign[:, None]
    return p


@pytest.mark.parametrize("flavour,mode,fill", [("fpn", "hard", "ones"), ("fpn", "logits", "ones"), ("fpn", "hard", "nan"),
                                               ("fpn", "soft_vote_rle", "ones"), ("c4", "hard", "ones"), ("c4", "hard", "nan"),
                                               ("c4", "soft_vote", "ones")])
def test_caller_rows_past_counts_ignored(oracle, flavour, mode, fill):
    fpn = flavour == "fpn"
    make = (lambda: make_fpn(mode)) if fpn else (lambda: make_c4(mode))
    strides = synth.FPN_STRIDES if fpn else [16]
    for s in ((fpn_set("sparse", 3900, mode == "logits"), fpn_set("crowded", 3910, mode == "logits")) if fpn else
              (c4_set("sparse", 2400),)):
        clean = fresh_views(make, s)
        bad = poison_caller_rows(s, clean, fill, strides, logits=mode == "logits")
        if s["hw_list"] != [s["hw_list"][0]] * B:     # a set with small extents: rows past n_rois exist
            assert any(int(clean[b]["collect/n_rois"]) < clean[b]["box/box_feats"].shape[0] for b in range(B))
        got = fresh_views(make, bad)
        for b in range(B):
            assert_views_equal(got[b], clean[b], "%s image %d" % (flavour, b))
    if fpn and mode == "hard" and fill == "ones":        # the sparse set's small image: the clean rows == the oracle chain
        s = fpn_set("sparse", 3900)
        path = make()
        bind(path, poison_caller_rows(s, fresh_views(make, s), fill, strides))
        path.step(use_graph=True)
        torch.cuda.synchronize()
        oracle_anchor(path, s, 0)


# ---- 3. each entry point on its own: dense call, then sparse call on the same workspace / outputs == zero-filled call -------------
def fpn_stages(p, st):
    return [
        ("rpn", lambda: p._rpn_topk_decode(st)),
        ("nms", lambda: p._nms_sorted(st)),
        ("collect", lambda: p._collect_kept(st)),            # dtc_fpn_collect_distribute_kept
        ("box", lambda: p._roi_align_box(st)),
        (("det", "maskmap", "maskfeat"), lambda: p.launch_detections(st)),   # + the mask-branch mapping (fused or separate), mask RoIAlign
        ("paste", lambda: p._mask_paste(st)),
        ("rle", lambda: p._mask_rle(st)),
    ]


def c4_stages(p, st):
    from detectorch_amd import hip
    L, ck, Bp, T = hip.lib(), hip.check, p.B, p.top_n
    return [
        ("rpn", lambda: p._rpn_topk_decode(st)),
        ("nms_sorted", lambda: p._nms_sorted(st)),
        ("nms", lambda: p._gather_kept(st)),
        ("collect", lambda: p._collect(st)),               # dtc_fpn_collect_distribute, inputs_sorted = 1
        ("box", lambda: p._roi_align_box(st)),             # dtc_roi_align_forward_packed_ws: the map kernel's preparation workspace
        ("det", lambda: ck(L.dtc_postprocess_detections_ex(
            p.rois5.data_ptr(), p.n_rois.data_ptr(), p.cls_score.data_ptr(), 0, p.bbox_pred.data_ptr(), None, p.sf.data_ptr(),
            p.im_size.data_ptr(), Bp, T, p.n_cls, 10.0, 10.0, 5.0, 5.0, 0.05, 0.5, p.max_det, p.det_opt, p.det_ws.data_ptr(),
            p.det_ws.numel(), p.dets.data_ptr(), p.det_roi.data_ptr(), p.det_scaled.data_ptr(), p.det_count.data_ptr(), p.max_out,
            None, st), "det_ex")),
    ]


def _stagewise(make, stages, dense, sparse):
    from detectorch_amd import hip
    want = fresh_views(make, sparse)
    p = make()
    bind(p, dense)
    p.step(use_graph=False)                  # every output and workspace now holds the dense set's state
    load(p, sparse)
    st = hip.stream_ptr(dev())
    for name, run in stages(p, st):
        run()
        for b in range(B):
            assert_views_equal(contract_view(p, b), want[b], "entry %s image %d" % (name, b),
                               stage=name if isinstance(name, tuple) else (name,))
    # collect: roi_order is still a permutation of the rows, roi_desc rows past n_rois are padding (level -1)
    T = p.top_n
    for b in range(B):
        n = int(p.n_rois[b])
        assert np.array_equal(np.sort(p.roi_order[b].cpu().numpy()), b * T + np.arange(T))
        assert (p.roi_desc[b, :, 5] < 0).sum().item() == T - n


@pytest.mark.parametrize("fused_map", [True, False])
@pytest.mark.parametrize("mode", ["hard", "logits", "soft_vote_rle"])
def test_fpn_entry_points_dense_then_sparse(mode, fused_map):
    lg = mode == "logits"

    def make():
        p = make_fpn(mode, rle=True)
        p.fused_mask_map = fused_map          # False: dtc_postprocess_detections_ex without fpn + dtc_fpn_collect_distribute
        return p
    _stagewise(make, fpn_stages, fpn_set("dense", 4000, lg), fpn_set("sparse", 4100, lg, perm=(1, 0, 3, 2)))


@pytest.mark.parametrize("mode", ["hard", "soft_vote"])
def test_c4_entry_points_dense_then_sparse(mode):
    _stagewise(lambda: make_c4(mode), c4_stages, c4_set("dense", 2500), c4_set("sparse", 2600))


# ---- 4. resident vs ticket decode on the same inputs (DTC_RPN_DECODE_TICKETS=1, resolved once per process) -------------------
_TICKET_CHILD = r"""
import hashlib, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
import test_hip_step_isolation as T
from detectorch_amd.pipeline import FpnRegionPath
out = []
for batch, ch, seeds in ((4, 8, (3000, 3500)), (8, 256, (3000, 3600))):
    T.B, T.C = batch, ch
    sets = [T.fpn_set("dense", seeds[0])]
    s2 = T.fpn_set("dense", seeds[1])
    s2["hw_list"] = [(96, 160), (0, 0), (512, 1344), (800, 576)] * (batch // 4)
    s2["hw"] = torch.tensor(s2["hw_list"], dtype=torch.float32, device="cuda")
    sets.append(s2)
    p = FpnRegionPath(batch, torch.device("cuda", 0), channels=ch)
    T.bind(p, sets[0])
    for i, s in enumerate(sets):          # the second set runs on the workspace the first one left (tickets, histograms)
        if i:
            T.load(p, s)
        p.step(use_graph=True)
        p.step(use_graph=True)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for b in range(batch):
            v = T.contract_view(p, b)
            for k in sorted(v):
                h.update(k.encode()); h.update(np.ascontiguousarray(v[k]).tobytes())
        out.append("%%d/%%d %%s" %% (batch, i, h.hexdigest()))
print("\n".join(out))
print("ok")
"""


def test_resident_decode_equals_ticket_decode_in_child_process():
    """B = 4 at pre 1000 and the bench shape (B = 8, 5 levels, C = 256) take the resident decode by default; the same graph steps with
    DTC_RPN_DECODE_TICKETS=1 give the same pre-NMS boxes, scores and counts and the same whole step, bit for bit -- also on a second
    input set of other sizes replayed over the first one's workspace."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = _TICKET_CHILD % (os.path.dirname(here), here)
    res = []
    for knob in (None, "1"):
        e = dict(os.environ)
        e.pop("DTC_RPN_DECODE_TICKETS", None)
        if knob:
            e["DTC_RPN_DECODE_TICKETS"] = knob
        r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), str(knob) + "\n" + r.stdout[-1500:] + r.stderr[-3000:]
        res.append([l for l in r.stdout.splitlines() if "/" in l])
    assert len(res[0]) == 4 and res[0] == res[1], res
