"""The cases of the test-time-augmentation tests (test support, not a test module; tests/README_tta.md).  Seeded numpy only, so the
host tests (tests/test_tta_host.py) check on the CPU that every case holds the condition it was built for, and the GPU tests
(tests/test_hip_tta.py) send the same arrays to the device."""
import numpy as np

f32 = np.float32
B, R, N_CLS = 2, 67, 5                       # R = 67: the last wave of a workgroup's four rows is partial, 67 rows are no multiple of 4
IM_SIZE = np.array([[37.0, 1.0], [600.0, 4097.0]], f32)      # widths 1 and 4097: w - 1 = 0 clips everything, 4097 = 2^12 + 1
FLIPS = (0, 1, 1, 0, 1, 0, 0, 1)             # mixed flags, by view
SCALES = (1.0, 1.6, 0.5, 2.0, 1.25, 0.75, 1.0, 3.0)
UNION_COUNTS = ((0, 67), (67, 1))            # n_rois of the two images, alternating over the views
ALIGNED_COUNTS = ((61, 67),)                 # AVG / ID: the same counts in every view


def merge_case(T, counts, logits, seed=0):
    """-> (views, im_size): T views of B x R rows.  Rois touch and cross the image border on every side (so the clip acts before the
    flip), one in eight deltas is saturated (the exp clip at log(1000 / 16), centres thrown far outside), rows past n_rois hold NaN
    deltas and scores (they must never reach an output)."""
    rs = np.random.RandomState(1000 + 17 * seed + T)
    views = []
    for t in range(T):
        n_rois = np.array(counts[t % len(counts)], np.int32)
        scale = (f32(SCALES[t]) * np.array([1.0, 1.03125], f32)).astype(f32)
        rois5 = np.zeros((B, R, 5), f32)
        for b in range(B):
            h, w = IM_SIZE[b] * scale[b]
            x = np.sort(rs.uniform(-20, w + 20, (R, 2)), axis=1)
            y = np.sort(rs.uniform(-20, h + 20, (R, 2)), axis=1)
            rois5[b] = np.stack([np.full(R, b), x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1)
            rois5[b, 0, 1:] = [0, 0, w - 1, h - 1]                   # the whole view
            rois5[b, 1, 1:] = [w - 1, h - 1, w - 1, h - 1]           # one pixel in the far corner
        deltas = (rs.randn(B, R, 4 * N_CLS) * 0.5).astype(f32)
        sat = rs.rand(B, R, N_CLS) < 0.125
        big = np.stack([rs.choice([-1e4, 1e4], sat.shape), rs.choice([-1e4, 1e4], sat.shape), rs.choice([50.0, -50.0], sat.shape),
                        rs.choice([50.0, -50.0], sat.shape)], axis=-1).astype(f32)
        deltas = np.where(np.repeat(sat, 4, axis=2), big.reshape(B, R, 4 * N_CLS), deltas)
        lg = (rs.randn(B, R, N_CLS) * 3.0).astype(f32)
        if logits:
            cls = lg
        else:
            e = np.exp(lg - lg.max(axis=2, keepdims=True))
            cls = (e / e.sum(axis=2, keepdims=True)).astype(f32)
        for b in range(B):                                          # what lies past the counts must not matter
            deltas[b, n_rois[b]:] = np.nan
            cls[b, n_rois[b]:] = np.nan
            rois5[b, n_rois[b]:, 1:] = np.nan
        views.append(dict(rois5=rois5, n_rois=n_rois, cls_score=cls, bbox_pred=deltas, scale=scale, flipped=bool(FLIPS[t])))
    return views, IM_SIZE.copy()


MASK_B, MAX_OUT, K = 3, 4, 3
DET_COUNT = np.array([0, 3, MAX_OUT], np.int32)
MASK_FLIPS = {1: (0,), 2: (0, 1), 5: (1, 0, 1, 1, 0)}
SPECIAL = np.array([0.0, 1.0, 1e-30, 2.0 ** -24, 1.0 - 2.0 ** -24], f32)


def combine_case(M, T, special=False, seed=0):
    """-> (masks, flipped, det_count, mask_class): T asymmetric maps float32 [B*max_out, K, M, M] in [0, 1).  mask_class holds one -1 and
    one K among the live rows (a class outside [0, K) selects nothing).  special: the values of SPECIAL scattered over every view,
    plus -- in every view at once, at mirrored places, so that they meet -- a column of zeros and a column of ones."""
    rs = np.random.RandomState(2000 + 31 * seed + 7 * M + T)
    N = MASK_B * MAX_OUT
    flipped = MASK_FLIPS[T]
    masks = []
    for t in range(T):
        m = rs.uniform(0, 1, (N, K, M, M)).astype(f32)
        m = np.minimum(m, np.nextafter(f32(1), f32(0)))
        if special:
            at = rs.randint(0, m.size, 4000)
            m.reshape(-1)[at] = SPECIAL[rs.randint(0, len(SPECIAL), len(at))]
            zero_col, one_col = (0, 2) if not flipped[t] else (M - 1, M - 3)
            m[:, :, :, zero_col] = 0.0
            m[:, :, :, one_col] = 1.0
        masks.append(m)
    mask_class = rs.randint(0, K, N).astype(np.int32)
    mask_class[MAX_OUT + 1], mask_class[2 * MAX_OUT + 2] = -1, K
    return masks, flipped, DET_COUNT.copy(), mask_class
