"""dtc_fast_rcnn_targets off its default point (test support, not a test module): the (image, parameter set) table that
tests/golden/make_train_limits_golden.py runs through the reference's own chain (tests/golden/train_targets_limits.npz), that
tests/test_train_limits_host.py pins on the CPU and that tests/test_hip_train_limits.py launches; the device-side helpers both GPU
modules share (batch, run, host, check, check_fixture).

An IMAGE is a dict like train_targets_ref.make_case's (gt_boxes, gt_classes, is_crowd, proposals, im_scale, rand_keys), made by
image(name) and never modified; a CASE id names one image with one parameter set.  Every input stays inside the contract of
include/detectorch_train_hip.h: finite boxes with x2 >= x1, gt classes in (0, num_classes).
"""
import functools
import hashlib

import numpy as np

import train_targets_ref as tr

BASE_SEED = 20261019
EXPANDED = ("bbox_targets", "bbox_inside_weights", "bbox_outside_weights")
THREADS = 1024                                                               # kTgtThreads of fast_rcnn_targets.hip


def P(**kw):
    return dict(tr.DEFAULTS, **kw)


# ---- images ----------------------------------------------------------------------------------------------------------------------
def _keys(rs, n):
    return rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def synth(seed, G, n_crowd, n_prop, im_scale=1.6, num_classes=81):
    """the recipe of train_targets_ref.make_case's seeded cases: random gt, half of the proposals jittered copies of gt (two exact
    copies among them), four small boxes inside every crowd region, the rest random; the last gt carries class num_classes - 1"""
    rs = np.random.RandomState(BASE_SEED + seed)
    keys = _keys(rs, G + n_prop)
    gt = tr._boxes(rs, G, 30, tr.IM_W / 2.0, tr.IM_H / 2.0)
    cls = rs.randint(1, num_classes, G).astype(np.int32)
    if G:
        cls[G - 1] = num_classes - 1
    crowd = np.zeros(G, np.int32)
    if n_crowd:
        crowd[rs.choice(G, n_crowd, replace=False)] = 1
    prop = tr._boxes(rs, n_prop, 4, tr.IM_W / 2.0, tr.IM_H / 2.0)
    if G and n_prop:
        k = (n_prop + 1) // 2
        src = rs.randint(0, G, k)
        size = np.tile(gt[src, 2:] - gt[src, :2], 2)
        prop[:k] = gt[src] + (rs.uniform(-0.22, 0.22, (k, 4)) * size).astype(np.float32)
        prop[:k, 2:] = np.maximum(prop[:k, 2:], prop[:k, :2])
        if k > 8:
            prop[3] = gt[src[3]]
            prop[4] = gt[src[3]]
        if n_prop - k >= 4 * n_crowd:
            for j, ci in enumerate(np.where(crowd == 1)[0]):
                cb = gt[ci]
                for t in range(4):
                    fx, fy = rs.uniform(0.05, 0.5, 2)
                    w, h = (cb[2] - cb[0]) * 0.4, (cb[3] - cb[1]) * 0.4
                    x, y = cb[0] + fx * (cb[2] - cb[0]), cb[1] + fy * (cb[3] - cb[1])
                    prop[n_prop - 1 - 4 * j - t] = [x, y, x + w, y + h]
    return dict(gt_boxes=np.ascontiguousarray(gt, np.float32), gt_classes=cls, is_crowd=crowd,
                proposals=np.ascontiguousarray(prop, np.float32), im_scale=float(im_scale), rand_keys=keys)


def hand(seed, gt, cls, crowd, prop, im_scale=1.25):
    gt = np.asarray(gt, np.float32).reshape(-1, 4)
    prop = np.asarray(prop, np.float32).reshape(-1, 4)
    rs = np.random.RandomState(BASE_SEED + seed)
    return dict(gt_boxes=np.ascontiguousarray(gt), gt_classes=np.asarray(cls, np.int32).reshape(-1),
                is_crowd=np.asarray(crowd, np.int32).reshape(-1), proposals=np.ascontiguousarray(prop), im_scale=float(im_scale),
                rand_keys=_keys(rs, len(gt) + len(prop)))


GT4 = np.array([[10, 10, 59, 69], [100, 20, 179, 99], [200, 200, 299, 259], [400, 300, 479, 419]], np.float32)


def far(n, row=0):
    """n boxes of 10 x 20 that overlap neither each other nor anything inside the 640 x 480 image"""
    i = np.arange(n, dtype=np.float32)
    y = np.float32(1000 + 40 * row)
    return np.stack([1000 + 20 * i, y + 0 * i, 1009 + 20 * i, y + 19 + 0 * i], 1).astype(np.float32)


# name -> (G, P) of the sort sweep, and the branch of block_bitonic_sort its key count takes (csrc/block_sort.h:170-179)
SWEEP = {"n1_gt": (1, 0), "n1_prop": (0, 1), "n2": (1, 1), "n3": (1, 2), "n4": (2, 2), "n64": (4, 60), "n65": (4, 61),
         "n128": (4, 124), "n129": (4, 125), "n255": (5, 250), "n256": (6, 250), "n257": (6, 251), "n512": (12, 500),
         "n513": (13, 500), "n1024": (24, 1000), "n1025": (25, 1000), "n2048": (48, 2000), "n2049": (49, 2000),
         "n2304": (256, 2048)}
SWEEP_REACHES = {"n1_gt": (2, "regs1"), "n1_prop": (2, "regs1"), "n2": (2, "regs1"), "n3": (4, "regs1"), "n4": (4, "regs1"),
                 "n64": (64, "regs1"), "n65": (128, "regs1"), "n128": (128, "regs1"), "n129": (256, "merge"),
                 "n255": (256, "merge"), "n256": (256, "merge"), "n257": (512, "merge"), "n512": (512, "merge"),
                 "n513": (1024, "merge"), "n1024": (1024, "merge"), "n1025": (2048, "regs2"), "n2048": (2048, "regs2"),
                 "n2049": (4096, "regs4"), "n2304": (4096, "regs4")}
SWEEP_FULL = ("n2", "n4", "n64", "n128", "n256", "n512", "n1024", "n2048")   # every key a candidate's: no pad key

# name -> (fg keys, bg keys, pad keys present) after the sort
GROUPS = {"only_fg_pads": (True, False, True), "only_fg_full": (True, False, False), "only_bg_full": (False, True, False),
          "fg_bg_full": (True, True, False), "neither": (False, False, True), "one_each": (True, True, False)}

DUP_SAME_LANE = ((3, 67), (20, 148), (10, 138))                              # gt pairs (j, j + 64 k): one lane of the argmax visits both
DUP_OTHER_LANE = ((5, 90), (40, 150))
MANY_CROWD = (7, 100)


def next_pow2(n):
    """csrc/block_sort.h:262"""
    p = 2
    while p < n:
        p <<= 1
    return p


def sort_branch(n_pow2):
    """block_bitonic_sort<1024> (csrc/block_sort.h:170-179)"""
    per = (n_pow2 + THREADS - 1) // THREADS
    if per <= 1:
        return "merge" if n_pow2 >= 256 else "regs1"
    return "regs%d" % per


def _thresholds_image():
    im = synth(20, 6, 1, 300)
    im["proposals"][150:270] = np.vstack([far(40, r) for r in range(3)])     # no overlap with any gt: overlap 0, class 0
    c = int(np.where(im["is_crowd"] == 1)[0][0])
    im["rand_keys"][c] = 0                                                   # the crowd gt row and the boxes inside the crowd
    im["rand_keys"][6 + 296:6 + 300] = 1                                     # region come first wherever they are candidates
    return im


def _ties_image():
    im = tr.make_case("e")
    rs = np.random.RandomState(BASE_SEED + 21)
    extra = np.array([[0, 0, 9, 79],       # contains gt 0: IoU 100 / 800 = 0.125 = bg_thresh_lo
                      [0, 0, 9, 39],       # 100 / 400 = 0.25 = bg_thresh_hi
                      [4, 0, 15, 9],       # 60 / 160 = 0.375 = bbox_thresh
                      [0, 0, 9, 59],       # 1 / 6: background
                      [0, 0, 9, 99],       # 0.1: below bg_thresh_lo
                      [0, 0, 9, 19],       # 0.5 = fg_thresh
                      [0, 0, 9, 24]],      # 0.4: neither, carries targets
                     np.float32)
    return dict(im, proposals=np.vstack([im["proposals"], extra]), rand_keys=np.r_[im["rand_keys"], _keys(rs, len(extra))])


def _crowd_image():
    rs = np.random.RandomState(BASE_SEED + 22)
    gt = [[100, 100, 299, 299], [400, 50, 499, 249], [50, 320, 249, 459]]
    prop = [[120, 120, 200, 180], [150, 200, 298, 299], [100, 100, 299, 299],       # wholly inside crowd 0: IoA exactly 1.0
            [410, 60, 450, 100],                                                    # wholly inside crowd 1
            [290, 120, 309, 139], [480, 240, 519, 259],                             # exactly half (0) / a quarter (1) inside
            [299, 150, 318, 169],                                                   # touches crowd 0 by one pixel column: 0.05
            [50, 320, 249, 459], [60, 330, 240, 450], [40, 300, 260, 470]]          # on the non-crowd gt
    prop = np.vstack([np.array(prop, np.float32), tr._boxes(rs, 30, 8, 200, 200), far(8)])
    return hand(22, gt, [5, 9, 3], [1, 1, 0], prop)


def _many_gt_image():
    im = synth(23, 200, 0, 1500, im_scale=1.5)
    gt, prop, keys = im["gt_boxes"], im["proposals"], im["rand_keys"]
    for a, b in DUP_SAME_LANE + DUP_OTHER_LANE:
        gt[b] = gt[a]
    row = 760                                                                # past the jittered half
    for a, b in DUP_SAME_LANE + DUP_OTHER_LANE:                              # copies and near copies of every duplicated gt
        w, h = gt[a, 2] - gt[a, 0], gt[a, 3] - gt[a, 1]
        for dx in (0.0, 0.05, -0.04):
            prop[row] = gt[a] + np.float32(dx) * np.array([w, h, w, h], np.float32)
            keys[200 + row] = row - 760                                      # ... drawn first
            row += 1
    for c in MANY_CROWD:                                                     # the crowd box grown by half: IoU = IoA = 2 / 3, not filtered
        im["is_crowd"][c] = 1
        w = gt[c, 2] - gt[c, 0] + 1
        for f in (0.5, 0.48, 0.46):
            prop[row] = [gt[c, 0], gt[c, 1], gt[c, 2] + np.float32(f) * w, gt[c, 3]]
            keys[200 + row] = row - 760
            row += 1
    return im


def _keys_image(pattern):
    im = synth(30, 5, 1, 300)
    i = np.arange(305, dtype=np.uint64)
    rs = np.random.RandomState(BASE_SEED + 31)
    keys = {"zeros": 0 * i, "ones": 0 * i + 0xFFFFFFFF, "top_bits": (i % 7) << 29, "low_bits": i % 5,
            "negative_int32": _keys(rs, 305).astype(np.uint64) | ((i % 2) << 31)}[pattern]
    return dict(im, rand_keys=keys.astype(np.uint32))


@functools.lru_cache(maxsize=None)
def image(name):
    if name in SWEEP:
        G, n_prop = SWEEP[name]
        return synth(100 + sorted(SWEEP).index(name), G, 0, n_prop)
    if name == "only_fg_pads":
        return hand(1, GT4[:3], [3, 7, 2], [0, 0, 0], GT4[:3])
    if name == "only_fg_full":
        return hand(2, GT4, [3, 7, 2, 80], [0, 0, 0, 0], GT4)
    if name == "only_bg_full":
        return hand(3, np.zeros((0, 4)), [], [], far(8))
    if name == "fg_bg_full":
        return hand(4, GT4[:2], [3, 7], [0, 0], np.vstack([GT4[:2], far(4)]))
    if name == "neither":
        return hand(5, GT4[:1], [17], [1], far(6))
    if name == "one_each":
        return hand(6, GT4[:1], [17], [0], far(1))
    if name == "small":
        return synth(10, 5, 1, 300)
    if name == "large":
        return synth(11, 256, 4, 2048, im_scale=1.5)
    if name == "large3":
        return synth(12, 256, 4, 2048, im_scale=1.5, num_classes=3)
    if name == "thresholds":
        return _thresholds_image()
    if name == "ties":
        return _ties_image()
    if name == "crowd":
        return _crowd_image()
    if name == "many_gt":
        return _many_gt_image()
    if name == "h":
        return tr.make_case("h")
    if name.startswith("keys_"):
        return _keys_image(name[5:])
    if name.startswith("classes_"):
        im = synth(40, 6, 1, 200, num_classes=int(name[8:]))
        top = int(np.where(im["is_crowd"] == 0)[0][-1])                      # a gt row of the last class, drawn first
        im["gt_classes"][top], im["rand_keys"][top] = int(name[8:]) - 1, 0
        return im
    raise KeyError(name)


# ---- the table: case id -> (image, parameters) -------------------------------------------------------------------------------------
CASES = {}
for _n in SWEEP:
    CASES["sweep_" + _n] = (_n, P(rois_per_image=64))
GROUP_PARAMS = {"only_fg_pads": P(rois_per_image=16, fg_fraction=1.0), "only_fg_full": P(rois_per_image=16, fg_fraction=1.0),
                "only_bg_full": P(rois_per_image=16), "fg_bg_full": P(rois_per_image=16),
                "neither": P(rois_per_image=16, bg_thresh_lo=0.05), "one_each": P(rois_per_image=16)}
for _n in GROUPS:
    CASES["group_" + _n] = (_n, GROUP_PARAMS[_n])
# (R, fg_fraction): QUOTA_HALVES are the ones whose quota lands on a half
QUOTA = ((1, 0.5), (1, 1.0), (2, 0.25), (2, 0.0), (6, 0.25), (6, 0.5), (10, 0.25), (10, 1.0), (17, 0.5), (17, 0.25))
QUOTA_HALVES = ((1, 0.5), (2, 0.25), (6, 0.25), (10, 0.25), (17, 0.5))
for _R, _f in QUOTA:
    CASES["quota_R%d_f%s" % (_R, _f)] = ("small", P(rois_per_image=_R, fg_fraction=_f))
CASES["quota_R4095_f0.5"] = ("large", P(rois_per_image=4095, fg_fraction=0.5))
CASES["quota_R4096_f0.25_nc3"] = ("large3", P(rois_per_image=4096, num_classes=3))
QUOTA_IDS = tuple(c for c in CASES if c.startswith("quota_"))
THRESHOLDS = {
    "bbox0": P(rois_per_image=64, bbox_thresh=0.0),
    "bbox_m1": P(rois_per_image=64, bbox_thresh=-1.0, bg_thresh_lo=-1.0),    # (crowd rows are sampled only as background)
    "bbox0_agnostic": P(rois_per_image=64, bbox_thresh=0.0, cls_agnostic_bbox_reg=True),
    "bg_lo_m1": P(rois_per_image=64, bg_thresh_lo=-1.0),
    "fg_bg_0": P(rois_per_image=64, fg_thresh=0.0, bg_thresh_hi=0.0),
    "fg_bg_1": P(rois_per_image=64, fg_thresh=1.0, bg_thresh_hi=1.0),
    "not_float32": P(rois_per_image=64, fg_thresh=0.7, bg_thresh_hi=0.3, bg_thresh_lo=0.1, bbox_thresh=0.45),
}
for _n, _p in THRESHOLDS.items():
    CASES["thresh_" + _n] = ("thresholds", _p)
CASES["thresh_ties"] = ("ties", P(rois_per_image=16, fg_fraction=0.5, fg_thresh=0.5, bg_thresh_hi=0.25, bg_thresh_lo=0.125,
                                  bbox_thresh=0.375))
THRESH_IDS = tuple(c for c in CASES if c.startswith("thresh_"))
CROWD_THRESH = (0.0, 1e-9, 0.5, 1.0)
for _t in CROWD_THRESH:
    CASES["crowd_%s" % _t] = ("crowd", P(rois_per_image=32, crowd_thresh=_t))
CASES["many_gt"] = ("many_gt", P())
CASES["many_gt_h"] = ("h", P())
KEY_PATTERNS = ("zeros", "ones", "top_bits", "low_bits", "negative_int32")
for _n in KEY_PATTERNS:
    CASES["keys_" + _n] = ("keys_" + _n, P(rois_per_image=64))
CASES["weights_odd"] = ("small", P(rois_per_image=32, reg_weights=(10.1, 9.9, 5.3, 4.7)))
CASES["weights_mixed"] = ("small", P(rois_per_image=32, reg_weights=(1.0, 2.0, 3.0, 0.5)))
for _c in (2, 3, 64, 65, 1204):
    CASES["classes_%d" % _c] = ("classes_%d" % _c, P(rois_per_image=8 if _c == 1204 else 32, num_classes=_c))
REG_IDS = ("weights_odd", "weights_mixed") + tuple("classes_%d" % c for c in (2, 3, 64, 65, 1204))
# the cases whose expanded blobs the fixture holds: few classes, or class-agnostic
EXPANDED_IDS = ("thresh_bbox0_agnostic", "classes_2", "classes_3")
# fast_rcnn_sample_rois.py:103 expands with the default 81 classes whatever the roidb was built with, and raises on a target class
# above 80 (:161): that case is pinned against the restatement only
REFERENCE_RAISES = ("classes_1204",)
RECORDED = tuple(c for c in CASES if c not in REFERENCE_RAISES)
# the small images the 300-image batch cycles through (G <= 8, P <= 320)
SMALL_IMAGES = ("small", "only_fg_pads", "n1_prop", "only_bg_full", "neither", "n65", "one_each", "n3", "fg_bg_full", "n128", "n1_gt")


def case(cid):
    name, params = CASES[cid]
    return image(name), params


@functools.lru_cache(maxsize=None)
def want(cid):
    """the restatement's result of a case, computed once and left unchanged"""
    return tr.minibatch(*case(cid))


_by_image = {}


def want_of(name, params):
    """... of any (image, parameter set)"""
    key = (name, tuple(sorted((k, str(v)) for k, v in params.items())))
    if key not in _by_image:
        _by_image[key] = tr.minibatch(image(name), params)
    return _by_image[key]


SHA_ROWS = ("inputs", "assign", "overlap", "kept")                           # the rows of the fixture's <case>_sha


def fixture_sha(g, cid, row):
    return g[cid + "_sha"][SHA_ROWS.index(row)]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def input_digest(cid):
    im, params = case(cid)
    text = repr(sorted((k, tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in params.items())).encode()
    return sha(im["gt_boxes"], im["gt_classes"], im["is_crowd"], im["proposals"], im["rand_keys"], np.float64(im["im_scale"]),
               np.frombuffer(text, np.uint8))


def assign_digest(max_overlaps, max_classes, targets5):
    """of the per-candidate arrays that are compared bit for bit (dw and dh are not)"""
    return sha(np.asarray(max_overlaps, np.float32), np.asarray(max_classes, np.int32), np.asarray(targets5, np.float32)[:, :3])


def kept_digest(rois, kept_targets5):
    return sha(np.asarray(rois, np.float32), np.asarray(kept_targets5, np.float32)[:, :3])


def truncated_shift_order(inds, keys):
    """the sampling order of a kernel that shifts the key by 12 inside 32 bits: ascending ((key << 12) mod 2^32, index)"""
    k32 = (keys[inds].astype(np.uint64) << np.uint64(12)) & np.uint64(0xFFFFFFFF)
    return inds[np.lexsort((inds, k32))]


# ---- the device side -----------------------------------------------------------------------------------------------------------
def batch(images, G=None, n_prop=None, gt_counts=None, proposal_counts=None):
    """device inputs of a batch of images at strides G / n_prop, NaN / 1e30 / 0xDEADBEEF / crowd = 1 garbage past every image's own
    rows; the counts are the images' own unless given"""
    import torch
    B = len(images)
    G = max(len(c["gt_boxes"]) for c in images) if G is None else G
    n_prop = max(len(c["proposals"]) for c in images) if n_prop is None else n_prop
    gt = np.full((B, G, 4), np.nan, np.float32)
    cls = np.full((B, G), -12345, np.int32)
    crowd = np.full((B, G), 1, np.int32)
    prop = np.full((B, n_prop, 4), np.nan, np.float32)
    prop[:, :, 1] = 1e30
    keys = np.full((B, G + n_prop), 0xDEADBEEF, np.uint32)
    for b, c in enumerate(images):
        ng, npr = len(c["gt_boxes"]), len(c["proposals"])
        gt[b, :ng], cls[b, :ng], crowd[b, :ng], prop[b, :npr] = c["gt_boxes"], c["gt_classes"], c["is_crowd"], c["proposals"]
        keys[b, :ng + npr] = c["rand_keys"]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gc = [len(c["gt_boxes"]) for c in images] if gt_counts is None else gt_counts
    pc = [len(c["proposals"]) for c in images] if proposal_counts is None else proposal_counts
    return dict(gt_boxes=d(gt), gt_classes=d(cls), gt_is_crowd=d(crowd), gt_counts=d(np.array(gc, np.int32)), proposals=d(prop),
                proposal_counts=d(np.array(pc, np.int32)), im_scale=d(np.array([c["im_scale"] for c in images], np.float32)),
                rand_keys=d(keys.view(np.int32)))


def outputs_ff(B, n_cand, params, expanded=True, assignment=True):
    """the output set, every byte 0xFF"""
    import torch
    from detectorch_amd import hip_train
    out = hip_train.targets_outputs(B, n_cand, hip_train.train_params(**params), "cuda", expanded=expanded, assignment=assignment)
    for v in out.values():
        if v is not None:
            v.view(torch.uint8).fill_(0xFF)
    return out


def run(x, params, out=None, expanded=True, assignment=True):
    from detectorch_amd import hip_train
    return hip_train.fast_rcnn_targets(x["gt_boxes"], x["gt_classes"], x["gt_is_crowd"], x["gt_counts"], x["proposals"],
                                       x["proposal_counts"], x["im_scale"], x["rand_keys"], hip_train.train_params(**params),
                                       out=out, expanded=expanded, assignment=assignment)


def run_ff(x, params, expanded=True, assignment=True):
    """run() into outputs pre-filled with 0xFF"""
    B, n_cand = x["rand_keys"].shape
    return run(x, params, outputs_ff(B, n_cand, params, expanded, assignment), expanded, assignment)


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def check(o, b, want, params, bound, label):
    """image b of the host copy `o` of the outputs against a restatement result: all integers, max_overlaps, rois, weights, target
    classes, dx, dy, every padding row and every expanded blob bit for bit; dw / dh within `bound` float32 ulps of
    w * log(float64(ratio)), an exact 0 an exact 0.  -> the largest distance"""
    R, n, nf = params["rois_per_image"], want["n_rois"], want["n_fg"]
    assert int(o["n_rois"][b]) == n and int(o["n_fg"][b]) == nf
    nc = len(want["max_overlaps"])
    if o["max_overlaps"] is not None:
        assert tr.same_bits(o["max_overlaps"][b, :nc], want["max_overlaps"])
        assert tr.same_bits(o["max_classes"][b, :nc], want["max_classes"])
        assert not o["max_overlaps"][b, nc:].any() and not o["max_classes"][b, nc:].any()
    assert tr.same_bits(o["keep_inds"][b, :n], want["keep_inds"]) and np.all(o["keep_inds"][b, n:] == -1)
    assert tr.same_bits(o["labels"][b, :n], want["labels"]) and np.all(o["labels"][b, n:] == -1)
    rois = want["rois"].copy()
    rois[:, 0] = b
    assert tr.same_bits(o["rois5"][b, :n], rois)
    pad = np.zeros((R - n, 5), np.float32)
    pad[:, 0] = b
    assert tr.same_bits(o["rois5"][b, n:], pad)
    t5 = o["bbox_targets5"][b]
    assert tr.same_bits(t5[:n, :3], want["bbox_targets5"][:, :3]) and tr.same_bits(t5[n:], np.zeros((R - n, 5), np.float32))
    u = tr.ulps_from(t5[:n, 3:], want["want64"][want["keep_inds"]])
    worst = float(u.max(initial=0.0))
    print("%s image %d: dw / dh at most %.3f ulp from w * log(float64(ratio)) (bound %.3f)" % (label, b, worst, bound))
    assert worst <= bound
    if o["bbox_targets"] is not None:
        W = want["bbox_targets"].shape[1]
        bt = o["bbox_targets"][b]
        assert bt.shape == (R, W) and not bt[n:].any()
        slot = np.zeros((n, W), bool)                                        # the expanded targets are the compact ones, in their slot
        for r in np.where(want["bbox_targets5"][:, 0] > 0)[0]:
            c = int(want["bbox_targets5"][r, 0])
            slot[r, 4 * c:4 * c + 4] = True
            assert tr.same_bits(bt[r, 4 * c:4 * c + 4], t5[r, 1:])
        assert not bt[:n][~slot].any()
        for k in ("bbox_inside_weights", "bbox_outside_weights"):
            assert tr.same_bits(o[k][b, :n], want[k]) and not o[k][b, n:].any()
    return worst


def check_fixture(o, b, g, cid, n_cand):
    """image b of the host copy `o` against what the reference's own chain gave for case `cid` (tests/golden/
    train_targets_limits.npz): digests of the exact arrays always, the arrays themselves where the fixture holds them"""
    keep, labels = g[cid + "_kept"]
    n = len(keep)
    assert int(o["n_rois"][b]) == n and int(o["n_fg"][b]) == int(g[cid + "_n_fg"])
    assert tr.same_bits(o["keep_inds"][b, :n], keep) and tr.same_bits(o["labels"][b, :n], labels)
    rois = o["rois5"][b, :n].copy()
    rois[:, 0] = 0                                                           # the reference ran every image as batch index 0
    assert tr.same_bits(kept_digest(rois, o["bbox_targets5"][b, :n]), fixture_sha(g, cid, "kept"))
    # the device's targets of the candidates it did not keep are not output: the kept rows' stand in the digest above, and the
    # per-candidate overlaps and classes in this one
    assert tr.same_bits(sha(o["max_overlaps"][b, :n_cand], o["max_classes"][b, :n_cand]), fixture_sha(g, cid, "overlap"))
    if cid + "_rois" in g:
        assert tr.same_bits(rois, g[cid + "_rois"])
        assert tr.same_bits(o["bbox_targets5"][b, :n, :3], g[cid + "_targets5"][keep][:, :3])
        assert tr.same_bits(o["max_overlaps"][b, :n_cand], g[cid + "_max_overlaps"])
        assert tr.same_bits(o["max_classes"][b, :n_cand], g[cid + "_max_classes"])
    if cid + "_bbox_inside_weights" in g and o["bbox_targets"] is not None:
        for k in ("bbox_inside_weights", "bbox_outside_weights"):
            assert tr.same_bits(o[k][b, :n], g[cid + "_" + k])
        assert np.array_equal(o["bbox_targets"][b, :n] != 0, g[cid + "_bbox_targets"] != 0)
