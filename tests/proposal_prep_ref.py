"""The checker of the precomputed-proposal preprocessing (test support, not a test module): the Fast R-CNN test-time steps of
lib/utils/preprocess_sample.py:35-45 restated in numpy -- scale by im_scale (:36), remove_dup_prop (:63-70), and the level
distribution of add_multilevel_rois_for_test (lib/utils/multilevel_rois.py:19-83).  tests/test_proposal_prep_host.py pins it
against the reference's own outputs (tests/golden/proposal_ingest.npz); the GPU tests compare dtc_prepare_proposals with it."""
import numpy as np

# the cases of make_proposal_ingest_golden.py: name -> (image height, width, im_scale, number of proposals)
CASES = {
    "a": (427, 640, 800.0 / 427.0, 300),
    "b": (1000, 750, 1333.0 / 1000.0, 257),
    "c": (480, 640, 800.0 / 480.0, 1),
    "d": (600, 800, 1333.0 / 800.0, 0),
}


def _tie(s, m0):
    """a float32 coordinate v >= 16 (m0 + 0.5) / s whose float32 product with s lies exactly on a .5 of the 1/16 grid"""
    s32 = np.float32(s)
    for m in range(m0, m0 + 64):
        v = np.float32((m + 0.5) * 16.0 / s)
        if np.float32(v * s32) * np.float32(0.0625) == np.float32(m + 0.5):
            return v
    raise ValueError("no tie near %d" % m0)


def make_proposals(name):
    """Seeded proposals of case `name` (float32 [n, 4], original-image coordinates), with engineered aliases: rows that differ by
    less than one 1/16 grid cell after scaling, exact duplicates, coordinates that land on a .5 tie of the grid after the float32
    scaling, zero-width / zero-height boxes and -0.0."""
    h, w, s, n = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)) + 20261016)
    if n == 0:
        return np.zeros((0, 4), np.float32)
    x1 = rs.uniform(0, w - 20, n)
    y1 = rs.uniform(0, h - 20, n)
    bw = rs.uniform(1, w / 2.0, n)
    bh = rs.uniform(1, h / 2.0, n)
    b = np.stack([x1, y1, np.minimum(x1 + bw, w - 1), np.minimum(y1 + bh, h - 1)], 1).astype(np.float32)
    if n >= 40:
        k = n // 8
        src = rs.randint(0, n, k)
        b[-k:] = b[src] + rs.uniform(-0.2, 0.2, (k, 4)).astype(np.float32) / np.float32(s)     # sub-cell jitter: aliases
        b[-k - 5:-k] = b[src[:5]]                                                               # exact duplicates
        for t in range(6):                                                                       # .5 ties on the 1/16 grid
            b[t] = [_tie(s, 2 + 3 * t), _tie(s, 1 + 2 * t), _tie(s, 20 + 3 * t), _tie(s, 16 + 2 * t)]
        b[6, 2] = b[6, 0]                                                                         # zero width
        b[7, 3] = b[7, 1]                                                                         # zero height
        b[8] = b[9]                                                                              # adjacent duplicate
        b[10, 0] = np.float32(-0.0)
        b[11, 0] = np.float32(0.0)
        b[11, 1:] = b[10, 1:]                                                                    # -0. and 0. alias
    return np.ascontiguousarray(b, np.float32)


def scale(boxes, im_scale):
    """preprocess_sample.py:36: a float32 array times a Python float (numpy 2: the scale is rounded to float32 first)"""
    return np.asarray(boxes, np.float32) * float(im_scale)


def remove_dup(p, spatial_scale=0.0625):
    """remove_dup_prop (:63-70) -> (unique rows in ascending hash order, index of each = its first occurrence)"""
    v = np.array([1e3, 1e6, 1e9, 1e12])
    hashes = np.round(p * spatial_scale).dot(v)
    _, index = np.unique(hashes, return_index=True)
    return p[index, :], index


def fpn_levels(rois, k_min=2, k_max=5):
    """map_rois_to_fpn_levels (multilevel_rois.py:41-53) in numpy's float32 arithmetic (boxes_area: lib/utils/boxes.py:77-79)"""
    w = rois[:, 2] - rois[:, 0] + 1
    h = rois[:, 3] - rois[:, 1] + 1
    s = np.sqrt(w * h)
    t = np.floor(4 + np.log2(s / 224 + 1e-6))
    return np.clip(t, k_min, k_max)


def distribute(rois, k_min=2, k_max=5):
    """add_multilevel_roi_blobs (:56-83) -> (per-level lists, rois_idx_restore int32, level of each row)"""
    lv = fpn_levels(rois, k_min, k_max)
    per, order = [], np.empty((0,))
    for l in range(k_min, k_max + 1):
        idx = np.where(lv == l)[0]
        per.append(rois[idx, :])
        order = np.concatenate((order, idx))
    return per, np.argsort(order).astype(np.int32, copy=False), lv


def prepare(boxes, im_scale, dedup_scale=0.0625, k_min=2, k_max=5):
    """The device entry's outputs for one image: dict(rois [m,4], src_index [m], levels [m] (level - k_min), rois_by_level [m,4],
    level_counts [nl], idx_restore [m])."""
    p = scale(boxes, im_scale)
    if dedup_scale:
        rois, index = remove_dup(p, dedup_scale)
    else:
        rois, index = p, np.arange(p.shape[0])
    per, restore, lv = distribute(rois, k_min, k_max)
    by_level = np.concatenate(per, 0) if len(rois) else np.zeros((0, 4), np.float32)
    return dict(rois=rois, src_index=index.astype(np.int32), levels=(lv - k_min).astype(np.int32), rois_by_level=by_level,
                level_counts=np.array([len(q) for q in per], np.int32), idx_restore=restore)
