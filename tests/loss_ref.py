"""The checker of the Fast R-CNN head losses (test support, not a test module): the reference's formulas restated in numpy at a
chosen precision, the contract of dtc_fast_rcnn_loss (include/detectorch_loss_hip.h) built from them, and the seeded CASES that
the golden generator and the tests share.

    smooth_l1       lib/model/loss.py:13-20   smooth_L1(pred, targets, alpha_in, alpha_out, beta), and what autograd gives for pred
    cross_entropy   lib/model/loss.py:11      torch.nn.functional.cross_entropy (train_fast.py:147): mean of logsumexp - row[label]
    accuracy        lib/model/loss.py:22-26   argmax over softmax == label, mean
    expand          lib/utils/fast_rcnn_sample_rois.py:139-163   _expand_bbox_targets, keyed by the TARGET class

tests/test_loss_host.py pins the float64 restatement against the reference's own functions and torch's float64 cross_entropy
(tests/golden/loss.npz, made by tests/golden/make_loss_golden.py); the GPU tests measure the kernels against both.
"""
import numpy as np

EPS = 2.0 ** -24


def f32(beta):
    """beta as the entry receives it: a C float"""
    return float(np.float32(beta))


# ---- the formulas -----------------------------------------------------------------------------------------------------------------
def smooth_l1(pred, targets, alpha_in, alpha_out, beta, dtype=np.float64, upstream=1.0):
    """loss.py:13-20 -> (loss, d loss / d pred * upstream) in `dtype`"""
    pred, targets, alpha_in, alpha_out = (np.asarray(a, dtype) for a in (pred, targets, alpha_in, alpha_out))
    beta = dtype(beta)
    x = (pred - targets) * alpha_in                                          # :14
    xabs = np.abs(x)                                                         # :15
    y1 = dtype(0.5) * x ** 2 / beta                                          # :16
    y2 = xabs - dtype(0.5) * beta                                            # :17
    case1 = (xabs <= beta).astype(dtype)                                     # :18
    case2 = 1 - case1                                                        # :19
    n = dtype(pred.shape[0])
    loss = np.sum((y1 * case1 + y2 * case2) * alpha_out) / n                 # :20
    grad = (case1 * x / beta + case2 * np.sign(x)) * alpha_in * alpha_out * dtype(upstream) / n
    return dtype(loss), grad.astype(dtype)


def cross_entropy(cls_score, labels, dtype=np.float64, upstream=1.0):
    """mean over the rows of logsumexp(row) - row[label], the row maximum subtracted -> (loss, d loss / d cls_score * upstream)"""
    x = np.asarray(cls_score, dtype)
    n = x.shape[0]
    z = x - x.max(axis=1, keepdims=True)
    e = np.exp(z)
    s = e.sum(axis=1, keepdims=True)
    rows = np.arange(n)
    loss = np.sum(np.log(s[:, 0]) - z[rows, labels]) / dtype(n)
    grad = e / s
    grad[rows, labels] -= 1
    return dtype(loss), (grad * dtype(upstream) / dtype(n)).astype(dtype)


def argmax_logits(cls_score):
    """the entry's argmax: over the logits, lowest index among equal ones"""
    return np.argmax(np.asarray(cls_score), axis=1)


def argmax_softmax(cls_score):
    """loss.py:24: the reference's argmax, over the float32 softmax"""
    x = np.asarray(cls_score, np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return np.argmax(e / e.sum(axis=1, keepdims=True), axis=1)


def expand(targets5, width):
    """fast_rcnn_sample_rois.py:139-163 (and :107) on rows of (class, dx, dy, dw, dh): -> bbox_targets, inside, outside [N, width];
    width 8 is the class-agnostic form (any class > 0 -> 1)"""
    t5 = np.asarray(targets5, np.float32)
    bt = np.zeros((len(t5), width), np.float32)
    bw = np.zeros_like(bt)
    for ind in np.where(t5[:, 0] > 0)[0]:
        c = 1 if width == 8 else int(t5[ind, 0])
        bt[ind, 4 * c:4 * c + 4] = t5[ind, 1:]
        bw[ind, 4 * c:4 * c + 4] = 1.0
    return bt, bw, (bw > 0).astype(np.float32)


# ---- the contract of dtc_fast_rcnn_loss -------------------------------------------------------------------------------------------
def head(cls_score, labels, bbox_pred=None, targets5=None, beta=1.0, upstream=(1.0, 1.0), dtype=np.float64):
    """What include/detectorch_loss_hip.h specifies, from the formulas above applied to the rows the reference would see:
    rows with label < 0 are dropped; a label >= C takes the row out of the cross-entropy, the accuracy hits and the gradient
    (it stays in the divisor); a target class that is no integer in [0, C) takes it out of the box term.
    -> dict(loss_cls, loss_bbox, accuracy, n_valid, grad_cls [N, C], grad_box [N, W] or None)"""
    x = np.asarray(cls_score)
    labels = np.asarray(labels)
    N, C = x.shape
    valid = labels >= 0
    nv = int(valid.sum())
    out = dict(loss_cls=dtype(0), loss_bbox=dtype(0), accuracy=dtype(0), n_valid=nv, grad_cls=np.zeros((N, C), dtype), grad_box=None)
    if bbox_pred is not None:
        out["grad_box"] = np.zeros(np.asarray(bbox_pred).shape, dtype)
    if nv == 0:
        return out
    ok = valid & (labels < C)
    if ok.any():
        idx = np.where(ok)[0]
        l, g = cross_entropy(x[idx], labels[idx], dtype)
        out["loss_cls"] = dtype(l * dtype(len(idx)) / dtype(nv))
        out["grad_cls"][idx] = g * dtype(len(idx)) / dtype(nv) * dtype(upstream[0])
        out["accuracy"] = dtype(np.sum(argmax_logits(x[idx]) == labels[idx])) / dtype(nv)
    if bbox_pred is not None:
        W = np.asarray(bbox_pred).shape[1]
        t5 = np.array(targets5, np.float32)
        with np.errstate(invalid="ignore"):
            k = t5[:, 0]
            usable = valid & (k >= 0) & (k < C) & (k == np.floor(k))
        idx = np.where(usable)[0]
        if len(idx):
            bt, bi, bo = expand(t5[idx], W)
            l, g = smooth_l1(np.asarray(bbox_pred)[idx], bt, bi, bo, beta, dtype)
            out["loss_bbox"] = dtype(l * dtype(len(idx)) / dtype(nv))
            out["grad_box"][idx] = g * dtype(len(idx)) / dtype(nv) * dtype(upstream[1])
    return out


# ---- the seeded cases -------------------------------------------------------------------------------------------------------------
# name -> (seed, N, C, class-agnostic, logit scale, beta, fraction of ignored rows)
CASES = {
    "a": (0, 1, 81, False, 3.0, 1.0, 0.0),
    "b": (1, 65, 81, False, 3.0, 1.0, 0.0),                 # rows off 16-byte alignment, one row past a wave's worth
    "c2": (2, 33, 2, True, 3.0, 1.0, 0.0),                  # the lane boundaries of the row reduction, and the limit
    "c3": (3, 33, 3, False, 3.0, 1.0, 0.0),
    "c64": (4, 33, 64, False, 3.0, 1.0, 0.0),
    "c65": (5, 33, 65, False, 3.0, 1.0, 0.0),
    "c129": (6, 33, 129, False, 3.0, 1.0, 0.0),
    "c1024": (7, 33, 1024, False, 3.0, 1.0, 0.0),
    "d80": (8, 65, 81, False, 80.0, 1.0, 0.0),              # the label's logit far below the row maximum
    "d1e4": (9, 65, 81, False, 1e4, 1.0, 0.0),
    "e1": (10, 33, 5, False, 3.0, 1.0, 0.0),                # smooth-L1 edge values
    "e05": (11, 33, 5, False, 3.0, 0.5, 0.0),
    "e19": (12, 33, 5, False, 3.0, 1.0 / 9.0, 0.0),
    "i4097": (13, 4097, 81, False, 3.0, 1.0, 0.25),         # many workgroups; a quarter of the rows ignored
    "i65536": (14, 65536, 81, False, 3.0, 1.0, 0.25),
}
GOLDEN_CASES = tuple(CASES)
SAMPLED_CASES = {"c1024": 8, "i4097": 64, "i65536": 64}                    # the golden keeps scalars and a sample of gradient rows


def edge_values(beta):
    """x exactly +-beta, 0, and the float32 neighbours of +-beta on either side"""
    b = np.float32(beta)
    up, dn = np.nextafter(b, np.float32(np.inf)), np.nextafter(b, np.float32(0))
    return np.array([b, -b, 0.0, up, dn, -up, -dn, 0.5 * b, -2.0 * b], np.float32)


def make_case(name):
    """Seeded inputs of case `name`: dict(cls_score f32 [N,C], labels i32 [N], bbox_pred f32 [N,W], targets5 f32 [N,5], beta)."""
    seed, N, C, agnostic, scale, beta, ignored = CASES[name]
    rs = np.random.RandomState(20261019 + seed)
    W = 8 if agnostic else 4 * C
    x = (rs.standard_normal((N, C)) * scale).astype(np.float32)
    labels = rs.randint(0, C, N).astype(np.int32)
    labels[rs.uniform(size=N) < 0.5] = 0                                     # half the rows background
    if N == 1:
        labels[:] = 17                                                       # the one row is foreground: a box term
    if name.startswith("d"):                                                 # the label's logit far below the maximum
        rows = np.arange(N)
        x[rows, labels] = x.min(axis=1) - np.float32(0.5 * scale)
        x[rows, (labels + 1) % C] = x.max(axis=1) + np.float32(0.25 * scale)
    pred = (rs.standard_normal((N, W)) * 0.7).astype(np.float32)
    t5 = np.zeros((N, 5), np.float32)
    fg = labels > 0
    t5[fg, 0] = 1.0 if agnostic else labels[fg]
    t5[:, 1:] = (rs.standard_normal((N, 4)) * 0.7).astype(np.float32) * (t5[:, :1] > 0)
    if N >= 8:                                                               # a background row that carries targets of another class
        r = int(np.where(~fg)[0][0]) if (~fg).any() else 0
        t5[r] = [1.0 if agnostic else float(C - 1), 0.3, -0.2, 1.7, -2.5]
    if name.startswith("e"):                                                 # edge values: target 0, so x = pred exactly
        ev = edge_values(beta)
        for i, r in enumerate(np.where(t5[:, 0] > 0)[0]):
            k = int(t5[r, 0])
            t5[r, 1:] = 0.0
            pred[r, 4 * k:4 * k + 4] = ev[(4 * i + np.arange(4)) % len(ev)]
    if ignored > 0:
        drop = rs.uniform(size=N) < ignored
        labels[drop] = -1
        t5[drop] = 0.0
    return dict(cls_score=x, labels=labels, bbox_pred=pred, targets5=t5, beta=f32(beta))


# general smooth_L1: name -> (seed, N, W, beta); alpha_in != 1, alpha_out in {0, 0.25, 2}, edge values through alpha_in = 0.5
SMOOTH_CASES = {"s7": (20, 33, 7, 1.0), "s324": (21, 65, 324, 0.5), "s20": (22, 33, 20, 1.0 / 9.0)}


def make_smooth_case(name):
    """dict(pred, targets, alpha_in, alpha_out f32 [N,W], beta): the first elements sit on the edges (x = pred * 0.5 exactly)"""
    seed, N, W, beta = SMOOTH_CASES[name]
    rs = np.random.RandomState(20261019 + seed)
    pred = rs.standard_normal((N, W)).astype(np.float32)
    targets = rs.standard_normal((N, W)).astype(np.float32)
    alpha_in = rs.uniform(0.5, 3.0, (N, W)).astype(np.float32)
    alpha_out = rs.choice(np.array([0.0, 0.25, 2.0], np.float32), (N, W)).astype(np.float32)
    ev = edge_values(beta)
    flat = lambda a: a.reshape(-1)
    n = len(ev)
    flat(pred)[:n] = ev * np.float32(2.0)
    flat(targets)[:n] = 0.0
    flat(alpha_in)[:n] = 0.5
    flat(alpha_out)[:n] = 2.0
    return dict(pred=pred, targets=targets, alpha_in=alpha_in, alpha_out=alpha_out, beta=f32(beta))


def sample_rows(name, n):
    """the gradient rows the golden keeps for a sampled case"""
    return np.sort(np.random.RandomState(77 + CASES[name][0]).choice(n, SAMPLED_CASES[name], replace=False))


# ---- the tolerances of the issue, against a float64 yardstick y -------------------------------------------------------------------
def bounds(y, cls_score, e_ref_cls=0.0, e_ref_box=0.0):
    """-> dict(loss_cls, loss_bbox: absolute; grad_cls: absolute; grad_box: relative)"""
    x = np.asarray(cls_score)
    top = float(np.max(np.abs(x))) if x.size else 0.0
    return dict(loss_cls=max(4 * e_ref_cls, 32 * EPS * max(abs(float(y["loss_cls"])), top)),
                loss_bbox=max(4 * e_ref_box, 32 * EPS * abs(float(y["loss_bbox"]))),
                grad_cls=16 * EPS / max(int(y["n_valid"]), 1), grad_box=8 * EPS)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
