"""The checker of RPN training (test support, not a test module): the contract of include/detectorch_rpn_hip.h restated in numpy
float32, one image at a time, with the seeded and hand-made CASES the golden generator and the tests use, and the float64
yardsticks of both losses and their gradients.

The reference has no text for the anchor assignment; its building blocks are pinned to it through tests/golden/rpn_train.npz (made by
tests/golden/make_rpn_train_golden.py): cython_bbox.bbox_overlaps (restated in train_targets_ref.bbox_overlaps), bbox_transform_inv
(lib/utils/boxes.py:211-242), generate_anchors and the shifted-anchor enumeration of lib/model/generate_proposals.py:124-149.
A level is (A, H, W, feat_stride, base anchors [A,4]); a spec is a list of levels.
"""
import math

import numpy as np

from train_targets_ref import bbox_overlaps, choose, same_bits, ulps_from  # noqa: F401

EPS = 2.0 ** -24
BLOCK, SELECT_BLOCK = 256, 1024                # csrc/rpn_train/rpn_train_common.h: kRpnThreads, kRpnSelThreads
DEFAULTS = dict(batch_size_per_im=256, fg_fraction=0.5, positive_overlap=0.7, negative_overlap=0.3, straddle_thresh=0.0)
_SETS = {1: ((32,), (1,)), 3: ((32,), (0.5, 1, 2)), 5: ((32, 64, 128, 256, 512), (1,)), 15: ((32, 64, 128, 256, 512), (0.5, 1, 2))}


def base_anchors(A, stride, size=None):
    from detectorch_amd.utils.generate_anchors import generate_anchors
    sizes, ratios = _SETS[A]
    if size is not None:
        sizes = (size,)
    return generate_anchors(stride=stride, sizes=sizes, aspect_ratios=ratios).astype(np.float32)


def single(A, H, W, stride=16):
    return [(A, H, W, float(stride), base_anchors(A, stride))]


def fpn(h0, w0, n=5):
    """n levels of 3 anchors (size 32 * 2^l, ratios 0.5, 1, 2) on maps h0 x w0, ceil(/2), ... at strides 4, 8, ..."""
    spec, h, w = [], h0, w0
    for l in range(n):
        spec.append((3, h, w, 4.0 * 2 ** l, base_anchors(3, 4 * 2 ** l, 32 * 2 ** l)))
        h, w = (h + 1) // 2, (w + 1) // 2
    return spec


def count_anchors(spec):
    return sum(A * H * W for A, H, W, _, _ in spec)


def anchors_of(spec):
    """every anchor of the spec in image-wide index order i = off_l + (a H + h) W + w, float32 [N,4] (generate_proposals.py:130-148)"""
    out = []
    for A, H, W, stride, base in spec:
        base = np.asarray(base, np.float32).reshape(A, 4)
        sx = np.arange(W, dtype=np.float32) * np.float32(stride)
        sy = np.arange(H, dtype=np.float32) * np.float32(stride)
        box = np.empty((A, H, W, 4), np.float32)
        box[..., 0] = base[:, None, None, 0] + sx[None, None, :]
        box[..., 1] = base[:, None, None, 1] + sy[None, :, None]
        box[..., 2] = base[:, None, None, 2] + sx[None, None, :]
        box[..., 3] = base[:, None, None, 3] + sy[None, :, None]
        out.append(box.reshape(-1, 4))
    return np.concatenate(out)


# name -> (spec, G, crowd rows among them, image (h, w), im_scale, parameter overrides, seed)
SIZE_SHAPES = {63: (3, 3, 7), 64: (1, 8, 8), 65: (5, 1, 13), 255: (3, 5, 17), 256: (1, 16, 16), 257: (1, 1, 257),
               1023: (3, 11, 31), 1024: (1, 32, 32), 1025: (5, 5, 41)}
CASES = {"n%d" % n: (single(*s), 3, 0, (s[1] * 16, s[2] * 16), 1.0,
                     dict(batch_size_per_im=8, straddle_thresh=-1.0 if n in (65, 257, 1025) else 0.0), n) for n, s in SIZE_SHAPES.items()}
CASES["fpn5"] = (fpn(48, 64), 6, 0, (192, 256), 1.6, dict(batch_size_per_im=32), 1)
CASES["c4"] = (single(15, 38, 50), 20, 2, (600, 797), 800.0 / 600.0, dict(), 2)
CASES["fpn"] = (fpn(152, 200), 30, 2, (608, 800), 1.25, dict(), 3)
JITTER = {"fpn": 0.02}                         # tighter copies: more anchors above positive_overlap than the quota of 128
SIZE_CASES = tuple("n%d" % n for n in SIZE_SHAPES)
GOLDEN_CASES = SIZE_CASES + ("fpn5", "c4", "fpn", "hand")
SAMPLED_CASES = ("c4", "fpn")                  # the golden keeps sampled rows of these


def params_of(name):
    return dict(DEFAULTS, **(HAND_PARAMS if name == "hand" else CASES[name][5]))


def make_case(name):
    """Seeded inputs of case `name`: dict(spec, gt_boxes f32 [G,4] (original image coordinates), is_crowd i32 [G], count, im_scale,
    im_hw (h, w), rand_keys u32 [N])."""
    if name == "hand":
        return hand_case()
    spec, G, n_crowd, (im_h, im_w), im_scale, _, seed = CASES[name]
    rs = np.random.RandomState(20261019 + seed)
    anchors = anchors_of(spec)
    N = len(anchors)
    keys = rs.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    ok = np.where((anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] < im_w) & (anchors[:, 3] < im_h))[0]
    pick = rs.choice(ok if len(ok) >= G else np.arange(N), G, replace=len(ok) < G)
    src = anchors[pick].astype(np.float64)
    size = np.tile(src[:, 2:] - src[:, :2] + 1.0, 2)
    jit = JITTER.get(name, 0.12)
    gt = src + rs.uniform(-jit, jit, (G, 4)) * size                          # jittered anchors: fg and near-fg around each
    gt[:, 2:] = np.maximum(gt[:, 2:], gt[:, :2] + 1.0)
    if G > 2:
        gt[G - 1] = [im_w * 0.25, im_h * 0.25, im_w * 0.75, im_h * 0.75]    # one large box: a low-quality best anchor
    crowd = np.zeros(G, np.int32)
    crowd[:n_crowd] = 1
    return dict(spec=spec, gt_boxes=np.ascontiguousarray(gt / im_scale, np.float32), is_crowd=crowd, count=G, im_scale=float(im_scale),
                im_hw=(float(im_h), float(im_w)), rand_keys=keys)


# ---- (c): hand-made anchors on a 1 x 1 map, integer gt, thresholds 0.5 / 0.25 -----------------------------------------------------
HAND_PARAMS = dict(batch_size_per_im=8, positive_overlap=0.5, negative_overlap=0.25)
E10 = 2.0 ** -10
HAND_ANCHORS = np.array([
    [0, 0, 9, 9],                  # 0: IoU exactly 1/2 with gt 0: fg by the threshold
    [0, 0, 9, 9 - E10],            # 1: the float32 neighbourhood below 1/2: ignored
    [0, 0, 9, 9 + E10],            # 2: above 1/2: fg
    [100, 100, 109, 109],          # 3: IoU exactly 1/4 with gt 1: not bg (ignored)
    [100, 100, 119, 119],          # 4: gt 1 itself
    [100, 100, 109, 109 - E10],    # 5: below 1/4: bg
    [100, 100, 109, 109 + E10],    # 6: above 1/4: ignored
    [200, 200, 209, 209],          # 7, 8: both tie gt 2's best overlap (1/3 < 1/2): both fg
    [220, 200, 229, 209],
    [300, 300, 319, 319],          # 9: equals gt 3 and gt 4: matched to the first
    [400, 400, 419, 419],          # 10: gt 5's best, IoU 0.04 < negative_overlap: fg, not bg
    [600, 600, 609, 609], [620, 600, 629, 609], [640, 600, 649, 609], [660, 600, 669, 609], [680, 600, 689, 609],   # 11-15: bg
], np.float32)
HAND_GT = np.array([[0, 0, 9, 19], [100, 100, 119, 119], [200, 200, 229, 209], [300, 300, 319, 319], [300, 300, 319, 319],
                    [400, 400, 499, 499], [1000, 1000, 1010, 1010]], np.float32)   # 6: best overlap 0: marks nothing
HAND_KEYS = {"random": None, "equal": np.full(16, 7, np.uint32),
             "extremes": np.array([0, 2 ** 32 - 1] * 8, np.uint32)}


def hand_case(keys="random"):
    rs = np.random.RandomState(20261019 + 77)
    k = HAND_KEYS[keys]
    if k is None:
        k = rs.randint(0, 2 ** 32, 16, dtype=np.uint64).astype(np.uint32)
    return dict(spec=[(16, 1, 1, 16.0, HAND_ANCHORS)], gt_boxes=HAND_GT.copy(), is_crowd=np.zeros(7, np.int32), count=7, im_scale=1.0,
                im_hw=(2000.0, 2000.0), rand_keys=k)


# ---- (d): straddle ---------------------------------------------------------------------------------------------------------------
BELOW0 = np.nextafter(np.float32(0), np.float32(-1))
STRADDLE_ANCHORS = np.array([[0, 0, 49, 49], [-0.0, 0, 49, 49], [BELOW0, 0, 49, 49], [100, 10, 199, 60], [100, 10, 200, 60],
                             [10, 50, 60, 99], [10, 50, 60, 100], [0, BELOW0, 49, 49]], np.float32)
STRADDLE_INSIDE = {0.0: [1, 1, 0, 1, 0, 1, 0, 0], 2.5: [1] * 8, -1.0: [1] * 8}


def straddle_case(st):
    rs = np.random.RandomState(20261019 + 78)
    gt = np.array([[100, 10, 199, 60], [0, 0, 49, 49], [10, 50, 60, 100]], np.float32)
    return dict(spec=[(8, 1, 1, 16.0, STRADDLE_ANCHORS)], gt_boxes=gt, is_crowd=np.zeros(3, np.int32), count=3, im_scale=1.0,
                im_hw=(100.0, 200.0), rand_keys=rs.randint(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)), \
        dict(DEFAULTS, batch_size_per_im=8, straddle_thresh=st)


def transform_inv(ex, g):
    """bbox_transform_inv (boxes.py:224-238), weights (1, 1, 1, 1), float32 -> (targets f32 [n,4], want64 [n,2]: log(float64(ratio)))"""
    ex, g = np.asarray(ex, np.float32), np.asarray(g, np.float32)
    ex_w, ex_h = ex[:, 2] - ex[:, 0] + np.float32(1), ex[:, 3] - ex[:, 1] + np.float32(1)
    ex_cx, ex_cy = ex[:, 0] + np.float32(0.5) * ex_w, ex[:, 1] + np.float32(0.5) * ex_h
    g_w, g_h = g[:, 2] - g[:, 0] + np.float32(1), g[:, 3] - g[:, 1] + np.float32(1)
    g_cx, g_cy = g[:, 0] + np.float32(0.5) * g_w, g[:, 1] + np.float32(0.5) * g_h
    t = np.stack([(g_cx - ex_cx) / ex_w, (g_cy - ex_cy) / ex_h, np.log(g_w / ex_w), np.log(g_h / ex_h)], 1).astype(np.float32)
    want = np.stack([np.log((g_w / ex_w).astype(np.float64)), np.log((g_h / ex_h).astype(np.float64))], 1)
    return t, want


def minibatch(case, params):
    """The contract for one image -> dict(inside bool [N], max_overlaps f32 [N], arg i32 [N], gt_max f32 [G], fg / bg bool [N] (the
    groups before sampling), labels i32 [N], fg_index i32 [F], fg_targets f32 [F,4], want64 f64 [F,2], fg_gt i32 [F], n_fg, n_bg)"""
    spec, keys = case["spec"], np.asarray(case["rand_keys"], np.uint32)
    anchors = anchors_of(spec)
    N, G = len(anchors), len(case["gt_boxes"])
    n_g = min(max(int(case["count"]), 0), G)
    gt = (np.asarray(case["gt_boxes"], np.float32)[:n_g] * np.float32(case["im_scale"])).astype(np.float32)
    ok = np.asarray(case["is_crowd"])[:n_g] == 0
    h, w = np.float32(case["im_hw"][0]), np.float32(case["im_hw"][1])
    st = np.float32(params["straddle_thresh"])
    if st < 0:
        inside = np.ones(N, bool)
    else:
        inside = (anchors[:, 0] >= -st) & (anchors[:, 1] >= -st) & (anchors[:, 2] < w + st) & (anchors[:, 3] < h + st)
    ov = np.zeros((N, n_g), np.float32)
    if ok.any() and inside.any():
        ov[np.ix_(inside, ok)] = bbox_overlaps(anchors[inside], gt[ok])
    max_ov, arg = np.zeros(N, np.float32), np.full(N, -1, np.int32)
    if ok.any():
        sub = ov[:, ok]
        max_ov, arg = sub.max(axis=1), np.where(ok)[0][sub.argmax(axis=1)].astype(np.int32)
    max_ov, arg = np.where(inside, max_ov, np.float32(0)).astype(np.float32), np.where(inside, arg, -2).astype(np.int32)
    gt_max = np.zeros(G, np.float32)
    if inside.any():
        gt_max[:n_g] = np.where(ok, ov[inside].max(axis=0), 0)
    ties = ((ov == gt_max[None, :n_g]) & (gt_max[None, :n_g] > 0) & ok[None, :]).any(axis=1)
    fg = inside & ((max_ov >= np.float32(params["positive_overlap"])) | ties)
    bg = inside & ~fg & (max_ov < np.float32(params["negative_overlap"]))
    R = int(params["batch_size_per_im"])
    F = int(params["fg_fraction"] * R)
    fg_inds = choose(np.where(fg)[0], min(F, int(fg.sum())), keys)
    bg_inds = choose(np.where(bg)[0], min(R - len(fg_inds), int(bg.sum())), keys)
    labels = np.full(N, -1, np.int32)
    labels[fg_inds], labels[bg_inds] = 1, 0
    fg_index, fg_gt = np.full(F, -1, np.int32), np.full(F, -1, np.int32)
    fg_targets, want64 = np.zeros((F, 4), np.float32), np.zeros((F, 2), np.float64)
    n = len(fg_inds)
    fg_index[:n], fg_gt[:n] = fg_inds, arg[fg_inds]
    has = fg_gt[:n] >= 0
    if has.any():
        t, want = transform_inv(anchors[fg_inds[has]], gt[fg_gt[:n][has]])
        fg_targets[:n][has], want64[:n][has] = t, want
    return dict(inside=inside, max_overlaps=max_ov, arg=arg, gt_max=gt_max, fg=fg, bg=bg, labels=labels, fg_index=fg_index,
                fg_targets=fg_targets, want64=want64, fg_gt=fg_gt, n_fg=n, n_bg=len(bg_inds), anchors=anchors)


def offsets(spec):
    return np.cumsum([0] + [A * H * W for A, H, W, _, _ in spec])


def expanded(spec, labels, fg_index, fg_targets, n_fg, n_bg):
    """bbox_targets / inside / outside weights f32 [4N] of one image from the compact outputs: per level [4A, H, W], channel 4a + k"""
    N, off = count_anchors(spec), offsets(spec)
    bt, bi, bo = (np.zeros(4 * N, np.float32) for _ in range(3))
    w_out = np.float32(1) / np.float32(n_fg + n_bg) if n_fg + n_bg else np.float32(0)
    for l, (A, H, W, _, _) in enumerate(spec):
        lab = labels[off[l]:off[l + 1]].reshape(A, H, W)
        view = lambda a: a[4 * off[l]:4 * off[l + 1]].reshape(A, 4, H, W)
        view(bo)[:] = np.where(lab >= 0, w_out, np.float32(0))[:, None]
        for j in range(n_fg):
            i = fg_index[j] - off[l]
            if 0 <= i < A * H * W:
                a, h, w = np.unravel_index(i, (A, H, W))
                view(bt)[a, :, h, w], view(bi)[a, :, h, w] = fg_targets[j], 1.0
    return bt, bi, bo


# ---- the losses: float64 yardsticks ------------------------------------------------------------------------------------------------
def losses64(spec, cls, box, labels, fg_index, fg_targets, n_fg, n_bg, beta, upstream=(1.0, 1.0)):
    """cls / box: per level float32 [B,A,H,W] / [B,4A,H,W]; labels i32 [B,N]; fg_index [B,F]; fg_targets f32 [B,F,4]; n_fg, n_bg [B].
    -> dict(loss_cls, loss_bbox, n_valid, grad_cls, grad_box (lists of float64 arrays), scale_cls: max |logit| over the valid elements)"""
    B, F = fg_index.shape
    N, off = count_anchors(spec), offsets(spec)
    nf = np.clip(np.asarray(n_fg, np.int64), 0, F)
    nv = nf + np.maximum(np.asarray(n_bg, np.int64), 0)
    n_valid = int(nv.sum())
    beta = float(np.float32(beta))
    terms, grad_cls, grad_box, scale = [], [], [], 0.0
    for l, (A, H, W, _, _) in enumerate(spec):
        lab = labels[:, off[l]:off[l + 1]].reshape(B, A, H, W)
        x = cls[l].astype(np.float64)
        valid, y = (lab == 0) | (lab == 1), (lab == 1).astype(np.float64)
        with np.errstate(over="ignore"):
            e = np.exp(-np.abs(x))
            t = np.maximum(x, 0) - x * y + np.log1p(e)
            sig = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        terms += t[valid].tolist()
        scale = max(scale, float(np.abs(x[valid]).max(initial=0.0)))
        grad_cls.append(np.where(valid, float(upstream[0]) * (sig - y) / max(n_valid, 1), 0.0))
        grad_box.append(np.zeros(box[l].shape, np.float64))
    per_image = []
    for b in range(B):
        rows = []
        for j in range(int(nf[b])):
            i = int(fg_index[b, j])
            if i < 0 or i >= N:
                continue
            l = int(np.searchsorted(off, i, side="right") - 1)
            A, H, W = spec[l][:3]
            a, h, w = np.unravel_index(i - off[l], (A, H, W))
            for k in range(4):
                d = float(box[l][b, 4 * a + k, h, w]) - float(fg_targets[b, j, k])
                quad = abs(d) <= beta
                rows.append(0.5 * d * d / beta if quad else abs(d) - 0.5 * beta)
                slope = d / beta if quad else math.copysign(1.0, d)
                grad_box[l][b, 4 * a + k, h, w] = float(upstream[1]) * slope / (max(int(nv[b]), 1) * B)
        per_image.append(math.fsum(rows) / max(int(nv[b]), 1))
    return dict(loss_cls=math.fsum(terms) / max(n_valid, 1), loss_bbox=math.fsum(per_image) / B, n_valid=n_valid, grad_cls=grad_cls,
                grad_box=grad_box, scale_cls=scale)


def loss_bounds(y, e_ref_cls=0.0, e_ref_box=0.0):
    """tests/README_loss.md's rule: loss max(4 e_ref, 32 eps scale); grad_cls absolute 16 eps |upstream| / n_valid (the caller
    multiplies by |upstream|); grad_box relative 8 eps"""
    return dict(loss_cls=max(4 * e_ref_cls, 32 * EPS * max(abs(y["loss_cls"]), y["scale_cls"])),
                loss_bbox=max(4 * e_ref_box, 32 * EPS * abs(y["loss_bbox"])), grad_cls=16 * EPS / max(y["n_valid"], 1), grad_box=8 * EPS)


LOSS_SHAPES = {1: (1, 1, 1), 3: (3, 1, 1), 4: (1, 2, 2), 5: (5, 1, 1)}
LOSS_SHAPES.update(SIZE_SHAPES)
LOSS_CASES = tuple("n%d" % n for n in LOSS_SHAPES) + ("fpn5", "fpn")
LOSS_F = {"fpn": 128}


def loss_spec(name):
    return CASES[name][0] if name in ("fpn5", "fpn") else single(*LOSS_SHAPES[int(name[1:])])


def make_loss_case(name, B=2, seed=0, logit_scale=3.0):
    """Seeded loss inputs on the maps of case `name` (the losses do not depend on how the labels came about): dict(spec, cls, box
    (lists of float32 arrays), labels [B,N] in {1, 0, -1}, fg_index [B,F] = the anchors labelled 1 in a random order, -1 behind,
    fg_targets [B,F,4], n_fg, n_bg [B])"""
    spec = loss_spec(name)
    N = count_anchors(spec)
    F = LOSS_F.get(name, 16)
    rs = np.random.RandomState(20261019 + 1000 + seed + 7 * sorted(LOSS_CASES).index(name))
    labels, fg_index = np.full((B, N), -1, np.int32), np.full((B, F), -1, np.int32)
    fg_targets, n_fg, n_bg = np.zeros((B, F, 4), np.float32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        perm = rs.permutation(N)
        n_fg[b] = rs.randint(1 if b == 0 else 0, min(F, N) + 1)
        n_bg[b] = rs.randint(0, min(N - n_fg[b], 3 * F) + 1)
        labels[b, perm[:n_fg[b]]], labels[b, perm[n_fg[b]:n_fg[b] + n_bg[b]]] = 1, 0
        fg_index[b, :n_fg[b]] = perm[:n_fg[b]]
        fg_targets[b, :n_fg[b]] = (rs.standard_normal((n_fg[b], 4)) * 0.4).astype(np.float32)
    cls = [(rs.standard_normal((B, A, H, W)) * logit_scale).astype(np.float32) for A, H, W, _, _ in spec]
    box = [(rs.standard_normal((B, 4 * A, H, W)) * 0.3).astype(np.float32) for A, H, W, _, _ in spec]
    return dict(spec=spec, cls=cls, box=box, labels=labels, fg_index=fg_index, fg_targets=fg_targets, n_fg=n_fg, n_bg=n_bg)


def y_of(c, beta=1.0 / 9.0, upstream=(1.0, 1.0)):
    return losses64(c["spec"], c["cls"], c["box"], c["labels"], c["fg_index"], c["fg_targets"], c["n_fg"], c["n_bg"], beta, upstream)


def sample_rows(name, n, k=2000):
    """the rows of a large case that the golden keeps"""
    return np.sort(np.random.RandomState(20261019 + 500 + len(name)).choice(n, min(k, n), replace=False))
