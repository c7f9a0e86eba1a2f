"""dtc_fast_rcnn_loss and dtc_smooth_l1 off their default points (test support, not a test module): the seeded inputs, the parameter
sets and the branch table that tests/golden/make_loss_limits_golden.py runs through the reference's own functions
(tests/golden/loss_limits.npz), that tests/test_loss_limits_host.py pins on the CPU and that tests/test_hip_loss_limits.py
launches; the launch arithmetic of detectorch_amd/csrc/loss/*.hip restated (lanes_per_row .. flat_wraps); the device-side helpers
of the GPU module (Arena, head_call, measure).

A HEAD case is a dict like loss_ref.make_case's (cls_score, labels, bbox_pred, targets5, beta; the box arrays None in a
cross-entropy-only case), a FLAT case a dict like loss_ref.make_smooth_case's.  Valid rows hold finite values only, as
include/detectorch_loss_hip.h requires; ignored rows hold NaN.
"""
import functools
import hashlib

import numpy as np

import loss_ref as lr

BASE_SEED = 20261019 + 1000
N_SWEEP = 67

# ---- the launch arithmetic, restated ------------------------------------------------------------------------------------------------
THREADS, WAVES, MAX_BLOCKS = 256, 4, 1024                                    # kLossThreads, kLossWaves, kLossMaxBlocks


def lanes_per_row(c):
    """fast_rcnn_loss.hip lanes_per_row: the least power of two with 4 L >= C, 64 at the most"""
    L = 1
    while L < 64 and 4 * L < c:
        L <<= 1
    return L


def regs(c):
    """the E of the body dtc_fast_rcnn_loss launches"""
    return 4 if c <= 256 else 16


def rows_per_block(c):
    return 64 // lanes_per_row(c) * WAVES


def grid(n, c):
    return min(-(-n // rows_per_block(c)), MAX_BLOCKS)


def trips(n, c):
    """trips of the row loop of workgroup 0 (the most of any workgroup)"""
    return -(-n // (grid(n, c) * rows_per_block(c)))


def slots(c):
    """the register slots of a lane that hold a column < C in lane 0"""
    return -(-c // lanes_per_row(c))


def flat_blocks(total):
    return min(max((total // 4 + THREADS - 1) // THREADS, 1), MAX_BLOCKS)


def flat_wraps(total):
    """the 16-byte loop of smooth_l1_kernel runs a second trip in some thread"""
    return total // 4 > flat_blocks(total) * THREADS


# ---- 1, 2: the lane-width sweep and the class-agnostic form ----------------------------------------------------------------------
SWEEP_C = (4, 5, 8, 9, 16, 17, 32, 33, 128, 256, 257, 1023, 1024)
# C -> (L, E): what lanes_per_row and the c <= 256 choice must give; both sides of 4/5, 8/9, 16/17, 32/33, 128/129(130), 256/257
SWEEP_REACHES = {4: (1, 4), 5: (2, 4), 8: (2, 4), 9: (4, 4), 16: (4, 4), 17: (8, 4), 32: (8, 4), 33: (16, 4), 128: (32, 4),
                 256: (64, 4), 257: (64, 16), 1023: (64, 16), 1024: (64, 16)}
AGNOSTIC_C = (3, 81, 257)
ROW_LABEL_C, ROW_LABEL_C7, ROW_LAST_CLASS, ROW_TIE = 3, 8, 6, 11           # rows of the sweep with a fixed role (none is i % 5 == 4)


def walk(c):
    """the label columns the valid rows of a sweep case walk: lane 0 and lane L - 1 of every register slot first (the last slot:
    its last column), then a stride coprime to C"""
    L = lanes_per_row(c)
    cols = []
    for e in range(slots(c)):
        cols += [e * L, min(e * L + L - 1, c - 1)]
    stride = next(s for s in range(max(c // 3, 2), 2 * c + 7) if np.gcd(s, c) == 1)
    return cols + [(7 + i * stride) % c for i in range(N_SWEEP)]


def make_sweep(c, agnostic=False):
    """N = 67 rows of C classes.  Valid row number r (in row order) has label walk(C)[r]; its argmax is its label when r is even
    and the label of the row that mirrors it (walk(C)[n - 1 - r]) otherwise, the winning logit 4 above the row's largest.  Every
    fifth row is ignored and NaN; one row has label C and one C + 7; row ROW_TIE has two equal winners, columns 1 and max(L, 2),
    and label 1; ROW_LAST_CLASS carries target class C - 1; the first background row carries targets of class min(2, C - 1)."""
    rs = np.random.RandomState(BASE_SEED + c + (5000 if agnostic else 0))
    N, W = N_SWEEP, 8 if agnostic else 4 * c
    x = (rs.standard_normal((N, c)) * 3.0).astype(np.float32)
    pred = (rs.standard_normal((N, W)) * 0.7).astype(np.float32)
    labels = np.zeros(N, np.int32)
    valid = np.arange(N) % 5 != 4
    plain = valid.copy()
    plain[[ROW_LABEL_C, ROW_LABEL_C7, ROW_TIE]] = False
    rows = np.where(plain)[0]
    cols = walk(c)[:len(rows)]
    labels[rows] = cols
    for r, i in enumerate(rows):
        x[i, cols[r] if r % 2 == 0 else cols[len(rows) - 1 - r]] = x[i].max() + np.float32(4.0)
    labels[ROW_LABEL_C], labels[ROW_LABEL_C7], labels[ROW_TIE] = c, c + 7, 1
    x[ROW_TIE, [1, max(lanes_per_row(c), 2)]] = x[ROW_TIE].max() + np.float32(4.0)
    t5 = np.zeros((N, 5), np.float32)
    fg = valid & (labels > 0) & (labels < c)
    t5[fg, 0] = labels[fg]
    t5[ROW_LAST_CLASS, 0] = c - 1
    bg = int(np.where(valid & (labels == 0))[0][0])
    t5[bg, 0] = min(2, c - 1)
    t5[:, 1:] = (rs.standard_normal((N, 4)) * 0.7).astype(np.float32) * (t5[:, :1] > 0)
    labels[~valid] = -1
    x[~valid], pred[~valid], t5[~valid] = np.nan, np.nan, np.nan
    return dict(cls_score=x, labels=labels, bbox_pred=pred, targets5=t5, beta=1.0)


# ---- 3: the row loop ---------------------------------------------------------------------------------------------------------------
# name -> (C, N, box arguments, trips of the row loop)
WRAPS = {"r130": (130, 4099, True, 2), "r257": (257, 4101, True, 2), "r33": (33, 16387, True, 2), "r17": (17, 32771, True, 2),
         "ce257": (257, 65536, False, 16), "ce2": (2, 65536, False, 1)}
ONE_VALID = "one130"                                                         # (130, 4099): row 4098 alone is valid


def make_wrap(name):
    c, N, box, _ = WRAPS[name]
    rs = np.random.RandomState(BASE_SEED + 100 + sorted(WRAPS).index(name))
    x = rs.standard_normal((N, c)).astype(np.float32) * np.float32(3.0)
    labels = rs.randint(0, c, N).astype(np.int32)
    labels[rs.uniform(size=N) < 0.5] = 0
    drop = rs.uniform(size=N) < 0.25
    pred = t5 = None
    if box:
        pred = rs.standard_normal((N, 4 * c)).astype(np.float32) * np.float32(0.7)
        t5 = np.zeros((N, 5), np.float32)
        t5[:, 0] = labels
        t5[:, 1:] = (rs.standard_normal((N, 4)) * 0.7).astype(np.float32) * (t5[:, :1] > 0)
        pred[drop], t5[drop] = np.nan, np.nan
    labels[drop] = -1
    x[drop] = np.nan
    return dict(cls_score=x, labels=labels, bbox_pred=pred, targets5=t5, beta=1.0)


def make_one_valid():
    c = dict(make_wrap("r130"))
    x, labels, pred, t5 = (c[k].copy() for k in ("cls_score", "labels", "bbox_pred", "targets5"))
    rs = np.random.RandomState(BASE_SEED + 190)
    last = len(labels) - 1
    labels[:] = -1
    x[:], pred[:], t5[:] = np.nan, np.nan, np.nan
    labels[last] = 77
    x[last] = (rs.standard_normal(x.shape[1]) * 3.0).astype(np.float32)
    pred[last] = (rs.standard_normal(pred.shape[1]) * 0.7).astype(np.float32)
    t5[last] = [77.0, 0.3, -0.2, 1.7, -2.5]
    return dict(cls_score=x, labels=labels, bbox_pred=pred, targets5=t5, beta=1.0)


# ---- 4: target-class values ---------------------------------------------------------------------------------------------------------
TC_C = 81
TC_VALUES = (-0.0, 1e-40, 0.999, TC_C - 0.5, np.inf, 2.0 ** 24, TC_C - 1.0)  # rows 0 .. 6 of the case; the last alone has a box term


def make_target_classes(agnostic):
    """loss_ref's case (b) with the target classes of TC_VALUES on its first rows -> (the case, the same with the terms of the rows
    that must have none switched off)"""
    c = lr.make_case("b")
    pred = np.ascontiguousarray(c["bbox_pred"][:, :8]) if agnostic else c["bbox_pred"]
    t5 = c["targets5"].copy()
    n = len(TC_VALUES)
    t5[:n, 0] = np.array(TC_VALUES, np.float32)
    t5[:n, 1:] = 0.25
    off = t5.copy()
    off[:n - 1] = 0.0
    return dict(c, bbox_pred=pred, targets5=t5), dict(c, bbox_pred=pred, targets5=off)


# ---- 5: magnitudes -------------------------------------------------------------------------------------------------------------------
BIG = np.float32(1e38)
MAG_ROWS = ("low_label", "low_label2", "equal", "denormal", "onehot_hit", "onehot_miss", "plain", "plain2")


def make_magnitude_logits():
    """8 rows of 81 logits, all valid: +-1e38 with the label's logit among the lowest (the difference 2e38 is a float32); an
    all-equal row; a row of float32 denormals; one column at +1e38 over -1e38 with the label on it, and off it; two plain rows"""
    rs = np.random.RandomState(BASE_SEED + 200)
    N, C = len(MAG_ROWS), 81
    x = (rs.standard_normal((N, C)) * 3.0).astype(np.float32)
    labels = rs.randint(0, C, N).astype(np.int32)
    for r in (0, 1):
        x[r] = np.where(rs.uniform(size=C) < 0.5, BIG, -BIG)
        x[r, labels[r]] = -BIG
        x[r, (labels[r] + 3 + r) % C] = BIG
    x[2] = 3.5
    x[3] = (rs.randint(1, 2 ** 22, C).astype(np.uint32)).view(np.float32)   # k * 2^-149
    for r, hit in ((4, True), (5, False)):
        x[r] = -BIG
        x[r, 40 + r] = BIG
        labels[r] = 40 + r if hit else 17
    return dict(cls_score=x, labels=labels, bbox_pred=None, targets5=None, beta=1.0)


B149, B126, B100 = 2.0 ** -149, 2.0 ** -126, 2.0 ** 100
# beta -> the residuals |pred - target| of the case (each in both signs, and an exact 0): from the smallest whose gradient x / beta / 8
# is still >= 2^-100 up to 1e38, with |x| == beta and its float32 neighbours where they exist
MAG_BETAS = {
    "b149": (B149, [B149, 2 * B149, 1e-40, 1e-30, 1.0, 1e30, 1e38]),
    "b126": (B126, [B126, B126 / 2, float(np.nextafter(np.float32(B126), np.float32(1))), 1e-40, 1e-30, 1.0, 1e30, 1e38]),
    "b100": (B100, [B100, float(np.nextafter(np.float32(B100), np.float32(0))), 1e3, 1e10, 1e30, 1e31, 1e38]),
    "b3e38": (3e38, [float(np.float32(3e38)), 1e10, 1e20, 1e30, 1e38, 2e38]),
}


def make_magnitude_box(name):
    """8 rows of C = 5, every row foreground, the case's residuals through the selected columns: pred = +-r against target 0, and
    +-r/2 against -+r/2 for the even ones (|x| up to 6e38 for beta 3e38: the float32 difference would overflow, the double does
    not).  loss_ref.head's arguments."""
    beta, res = MAG_BETAS[name]
    rs = np.random.RandomState(BASE_SEED + 210 + sorted(MAG_BETAS).index(name))
    N, C = 8, 5
    v = np.array([0.0] + [s * r for r in res for s in (1.0, -1.0)], np.float32)
    p = np.resize(v, 4 * N).astype(np.float32)
    t = np.zeros(4 * N, np.float32)
    split = np.arange(4 * N) % 3 == 2                                        # a third of them as pred = x / 2, target = -x / 2
    t[split] = -p[split] / np.float32(2)
    p[split] = p[split] / np.float32(2)
    if name == "b3e38":                                                      # |x| = 6e38 > beta: the only linear elements of this beta
        p[[5, 6]], t[[5, 6]] = np.float32([3e38, -3e38]), np.float32([-3e38, 3e38])
    x = (rs.standard_normal((N, C)) * 3.0).astype(np.float32)
    labels = (np.arange(N) % (C - 1) + 1).astype(np.int32)
    pred = (rs.standard_normal((N, 4 * C)) * 0.7).astype(np.float32)
    t5 = np.zeros((N, 5), np.float32)
    t5[:, 0] = labels
    t5[:, 1:] = t.reshape(N, 4)
    for i in range(N):
        pred[i, 4 * labels[i]:4 * labels[i] + 4] = p[4 * i:4 * i + 4]
    return dict(cls_score=x, labels=labels, bbox_pred=pred, targets5=t5, beta=lr.f32(beta))


ALPHA_IN, ALPHA_OUT = (0.0, -1.5, 1e10), (0.0, -1.0, 2.0 ** -20)


def make_magnitude_alpha():
    """dtc_smooth_l1 with alpha_in in {0, -1.5, 1e10} x alpha_out in {0, -1, 2^-20} over residuals 2^-20 .. 1e20 in both signs,
    beta 1: [9, 12]"""
    r = np.array([s * m for m in (2.0 ** -20, 1e-10, 0.5, 1.0, 3.0, 1e20) for s in (1.0, -1.0)], np.float32)
    pred = np.tile(r + np.float32(0.25), (9, 1)).astype(np.float32)
    targets = np.full_like(pred, 0.25)
    ai = np.repeat(np.array(ALPHA_IN, np.float32), 3)[:, None] * np.ones_like(pred)
    ao = np.tile(np.array(ALPHA_OUT, np.float32), 3)[:, None] * np.ones_like(pred)
    return dict(pred=pred, targets=targets, alpha_in=ai.astype(np.float32), alpha_out=ao.astype(np.float32), beta=1.0)


# ---- 6: upstream ---------------------------------------------------------------------------------------------------------------------
UPSTREAMS = ((0.0, 0.0), (-2.0, 0.25), (0.0, 3.0), (1.0, 0.0))

# ---- 8: the flat pass of dtc_smooth_l1 ------------------------------------------------------------------------------------------------
# (N, W) -> (total % 4, the 16-byte loop wraps).  (1, 1048579) has total / 4 = 1024 * 256 + 3 / 4: exactly one 16-byte piece for every
# thread of the full grid and no second trip -- the last size before the wrap; (1, 1048583) is the wrap with a left-over of 3.
FLAT = {(1, 1): (1, False), (1, 2): (2, False), (1, 3): (3, False), (7, 1): (3, False), (5, 1): (1, False), (2, 3): (2, False),
        (3, 2): (2, False), (1025, 1024): (0, True), (3, 349527): (1, True), (1, 1048579): (3, False), (1, 1048583): (3, True)}
FLAT_SAMPLE = 64


def flat_name(shape):
    return "f%dx%d" % shape


def make_flat(shape):
    N, W = shape
    rs = np.random.RandomState(BASE_SEED + 300 + sorted(FLAT).index(shape))
    f = lambda a: a.astype(np.float32)
    return dict(pred=f(rs.standard_normal((N, W))), targets=f(rs.standard_normal((N, W))), alpha_in=f(rs.uniform(0.5, 3.0, (N, W))),
                alpha_out=rs.choice(np.array([0.25, 2.0, -1.0], np.float32), (N, W)).astype(np.float32), beta=1.0)


def flat_sample(shape):
    """the flat gradient elements the fixture keeps: the last 8 (the left-over elements among them) and a seeded sample"""
    total = shape[0] * shape[1]
    if total <= FLAT_SAMPLE:
        return np.arange(total)
    rs = np.random.RandomState(BASE_SEED + 400 + sorted(FLAT).index(shape))
    return np.unique(np.concatenate([rs.choice(total - 8, FLAT_SAMPLE - 8, replace=False), np.arange(total - 8, total)]))


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _head_cases():
    t = {}
    for c in SWEEP_C:
        t["s%d" % c] = functools.partial(make_sweep, c)
    for c in AGNOSTIC_C:
        t["w%d" % c] = functools.partial(make_sweep, c, True)
    for n in WRAPS:
        t[n] = functools.partial(make_wrap, n)
    t[ONE_VALID] = make_one_valid
    t["tc324"] = lambda: make_target_classes(False)[0]
    t["tc8"] = lambda: make_target_classes(True)[0]
    t["mlogits"] = make_magnitude_logits
    for n in MAG_BETAS:
        t[n] = functools.partial(make_magnitude_box, n)
    return t


HEAD = _head_cases()
# the cases the reference can compute: every label an index, every target class an integer, float32 formulas without inf * 0.
# A sweep case is recorded on its rows with label < C (the reference's cross_entropy indexes with the label); see the generator.
RECORDED = tuple(n for n in HEAD if n[0] in "swrco")
UNRECORDED = tuple(n for n in HEAD if n not in RECORDED)                    # tc324, tc8, mlogits, b149, b126, b100, b3e38
FULL_MAX_ROWS, FULL_MAX_C, SAMPLE_ROWS, SAMPLE_ROWS_WIDE = 70, 17, 8, 3


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of a head case, made once and never modified"""
    c = HEAD[name]()
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def want(name):
    """the float64 restatement of a head case, computed once and shared"""
    c = case(name)
    return lr.head(c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"], c["beta"])


def sample_rows(name):
    """the gradient rows the fixture keeps: all of a case of at most 70 rows and 17 classes; else a seeded sample of valid rows (8, 3
    above 256 classes) -- None for all"""
    c = case(name)
    N, C = c["cls_score"].shape
    if N <= FULL_MAX_ROWS and C <= FULL_MAX_C:
        return None
    rs = np.random.RandomState(BASE_SEED + 500 + sorted(HEAD).index(name))
    valid = np.where(c["labels"] >= 0)[0]
    k = min(SAMPLE_ROWS_WIDE if C > 256 else SAMPLE_ROWS, len(valid))
    return np.sort(rs.choice(valid, k, replace=False))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            a = np.ascontiguousarray(a)
            h.update(str((a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def head_digest(name):
    c = case(name)
    return sha(c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"], np.float32(c["beta"]))


def flat_digest(c):
    return sha(c["pred"], c["targets"], c["alpha_in"], c["alpha_out"], np.float32(c["beta"]))


def selected(c):
    """first selected column of bbox_pred per row (0 where the row has no box term), for rows whose target class is an integer"""
    k = np.nan_to_num(c["targets5"][:, 0], nan=0.0).astype(np.int64)
    return 4 * np.where(k > 0, 1 if c["bbox_pred"].shape[1] == 8 else k, 0)


# ---- device-side helpers of tests/test_hip_loss_limits.py ----------------------------------------------------------------------------
GUARD = 64
DEVICE = "cuda"


class Arena:
    """one device allocation pre-filled with 0xFF from which every buffer of a call is carved: take(n, skew) gives n 4-byte words
    that start `skew` words past a 16-byte boundary, with GUARD untouched words behind them"""

    def __init__(self, words):
        import torch
        self.buf = torch.empty(words + 8, dtype=torch.int32, device=DEVICE)
        self.buf.fill_(-1)
        self.pos = (-(self.buf.data_ptr() // 4)) % 4                         # a 16-byte boundary
        self.taken = []

    def take(self, n, skew=0, dtype=None, host=None):
        import torch
        start = self.pos + skew
        self.pos = -(-(start + n + GUARD) // 4) * 4
        assert self.pos <= self.buf.numel()
        v = self.buf[start:start + n]
        self.taken.append((start, n))
        if host is not None:
            host = np.array(host, copy=True)
            dtype = torch.int32 if host.dtype == np.int32 else torch.float32
            v.view(dtype).copy_(torch.from_numpy(host.reshape(-1)))
        assert (v.data_ptr() % 16) == 4 * (skew % 4)
        return v if dtype in (None, torch.int32) else v.view(dtype)

    def outside_is_untouched(self):
        """every word that was never handed out still holds 0xFF"""
        import torch
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEVICE)
        for start, n in self.taken:
            mask[start:start + n] = False
        return bool((self.buf[mask] == -1).all())


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEVICE)


def head_call(c, upstream=None, losses=True, grads=True, out=None):
    """dtc_fast_rcnn_loss on a head case (host arrays or device tensors) over outputs pre-filled with 0xFF -> the outputs as host
    arrays, None for a group not asked for"""
    import torch
    from detectorch_amd import hip_loss
    t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else dev(a))
    x, pred = t(c["cls_score"]), t(c["bbox_pred"])
    if out is None:
        out = hip_loss.loss_outputs(x.shape[0], x.shape[1], 0 if pred is None else pred.shape[1], "cuda", losses, grads)
    for v in out.values():
        if v is not None:
            v.view(torch.uint8).fill_(0xFF)
    hip_loss.fast_rcnn_loss(x, t(c["labels"]), pred, t(c["targets5"]), beta=c["beta"],
                            upstream=None if upstream is None else t(np.asarray(upstream, np.float32)), out=out)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items() if k != "workspace"}


WORST = {}                                                                   # quantity -> (distance in units of its bound, label)


def _note(quantity, units, label):
    if units > WORST.get(quantity, (-1.0, ""))[0]:
        WORST[quantity] = (units, label)


def measure(label, got, y, cls_score, e_ref=(0.0, 0.0), upstream=(1.0, 1.0), rows=None, box4=None):
    """The device's outputs against a yardstick dict y (loss_ref.head's keys; its gradients already carry `upstream`), every
    distance printed in units of its bound before it is asserted.  The bounds are loss_ref.bounds, the one on grad_cls_score times
    |upstream[0]|.  rows: y's gradient arrays hold these rows only; box4: y's grad_box holds the four selected columns, which start
    at column box4 of each row.  A promised zero is compared as a value here; the callers compare the bit patterns."""
    valid_x = np.asarray(cls_score)
    b = lr.bounds(y, valid_x, *e_ref)
    b["grad_cls"] *= abs(float(upstream[0]))
    unit = lambda d, bound: (0.0 if d == 0 else np.inf) if bound == 0 else d / bound
    nv = int(y["n_valid"])
    L = got["losses"]
    if L is not None:
        d_cls, d_box = abs(float(L[0]) - float(y["loss_cls"])), abs(float(L[1]) - float(y["loss_bbox"]))
        u_cls, u_box = unit(d_cls, b["loss_cls"]), unit(d_box, b["loss_bbox"])
        print("%s: loss_cls %.9g off by %.3g = %.3f of its bound, loss_bbox %.9g off by %.3g = %.3f of its bound" % (
            label, L[0], d_cls, u_cls, L[1], d_box, u_box))
        _note("loss_cls", u_cls, label)
        _note("loss_bbox", u_box, label)
        assert u_cls <= 1.0 and u_box <= 1.0
        assert L[2] == np.float32(float(y["accuracy"])) and L[3] == np.float32(nv)
    sel = slice(None) if rows is None else rows
    gc, gb = got["grad_cls_score"], got["grad_bbox_pred"]
    if gc is not None and y["grad_cls"] is not None:
        d = float(np.abs(gc[sel].astype(np.float64) - y["grad_cls"]).max())
        u = unit(d, b["grad_cls"])
        print("%s: grad_cls_score off by at most %.3g = %.3f of 16 eps |upstream[0]| / n_valid" % (label, d, u))
        _note("grad_cls_score", u, label)
        assert u <= 1.0
    if gb is not None and y["grad_box"] is not None:
        mine, wanted = gb[sel].astype(np.float64), y["grad_box"]
        if box4 is not None:
            cols = box4[:, None] + np.arange(4)[None, :]
            rest = mine.copy()
            np.put_along_axis(rest, cols, 0.0, 1)
            assert not rest.any()
            mine = np.take_along_axis(mine, cols, 1)
        nz = wanted != 0
        assert not mine[~nz].any()
        rel = float((np.abs(mine[nz] - wanted[nz]) / np.abs(wanted[nz])).max()) if nz.any() else 0.0
        print("%s: grad_bbox_pred off by at most %.3g relative = %.3f of 8 eps" % (label, rel, rel / b["grad_box"]))
        _note("grad_bbox_pred", rel / b["grad_box"], label)
        assert rel <= b["grad_box"]
