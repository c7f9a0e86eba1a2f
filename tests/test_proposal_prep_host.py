"""CPU pinning of the precomputed-proposal checker (tests/proposal_prep_ref.py) against the reference's own preprocessing
(tests/golden/proposal_ingest.npz, made by tests/golden/make_proposal_ingest_golden.py from lib/utils/preprocess_sample.py and
lib/utils/multilevel_rois.py), plus the properties the device entry relies on: the hash is exact in int64 as the key the
kernel sorts, and the fixture exercises every engineered case."""
import numpy as np
import pytest

from conftest import golden
import proposal_prep_ref as pr


@pytest.fixture(scope="module")
def g():
    return golden("proposal_ingest")


@pytest.mark.parametrize("case", sorted(pr.CASES))
def test_restatement_equals_reference(g, case):
    boxes = g[case + "_boxes"]
    assert np.array_equal(boxes, pr.make_proposals(case))                    # the seeded inputs are reproducible
    im_scale = float(g[case + "_im_scale"])
    scaled = pr.scale(boxes, im_scale)
    assert scaled.dtype == np.float32 and np.array_equal(scaled.view(np.uint32), g[case + "_scaled"].view(np.uint32))
    # numpy multiplies by the scale rounded to float32 (not in float64 and rounded after)
    assert np.array_equal(scaled, boxes * np.float32(im_scale))
    if len(boxes) == 0:
        return
    out = pr.prepare(boxes, im_scale)
    assert np.array_equal(out["rois"].view(np.uint32), g[case + "_dedup"].view(np.uint32))     # -0. included
    assert np.array_equal(out["src_index"], g[case + "_dedup_index"])
    by_level = np.concatenate([g["%s_rois_fpn%d" % (case, l)] for l in range(2, 6)], 0)
    assert np.array_equal(out["rois_by_level"], by_level)
    assert np.array_equal(out["level_counts"], [len(g["%s_rois_fpn%d" % (case, l)]) for l in range(2, 6)])
    assert np.array_equal(out["idx_restore"], g[case + "_rois_idx_restore_int32"])
    assert np.array_equal(pr.prepare(boxes, im_scale, dedup_scale=0)["idx_restore"], g[case + "_nodedup_restore"])


def _int_hash(p, ds=0.0625):
    """the kernel's key: r1 + 1e3 r2 + 1e6 r3 + 1e9 r4 in int64 (the reference's hash / 1000)"""
    r = np.round(p * ds).astype(np.int64)
    return r[:, 0] + 1000 * r[:, 1] + 1000000 * r[:, 2] + 1000000000 * r[:, 3]


def test_int64_hash_orders_like_the_float64_dot_product(g):
    for case in pr.CASES:
        p = g[case + "_scaled"]
        if len(p) == 0:
            continue
        h64 = np.round(p * 0.0625).dot(np.array([1e3, 1e6, 1e9, 1e12]))
        hi = _int_hash(p)
        assert np.array_equal(h64, hi.astype(np.float64) * 1000.0)
        # np.unique's order and first occurrences == a sort of (hash, row) keys, taking the first row of every run
        key = np.lexsort((np.arange(len(hi)), hi))
        first = key[np.r_[True, hi[key][1:] != hi[key][:-1]]]
        assert np.array_equal(first, g[case + "_dedup_index"])
    # the edge of the exact domain: |r| = 8192 in every coordinate stays exact (< 2^53) and inside the kernel's 44-bit key
    edge = np.array([[131071.0, -131071.0, 131071.0, 131071.0]], np.float32)
    assert abs(int(_int_hash(edge)[0])) < 2 ** 43
    assert float(np.round(edge * 0.0625).dot(np.array([1e3, 1e6, 1e9, 1e12]))[0]) == float(_int_hash(edge)[0]) * 1000.0


def test_fixture_covers_the_engineered_cases(g):
    p = g["a_scaled"]
    q = p * np.float32(0.0625)
    assert int(np.sum(q == np.floor(q) + 0.5)) >= 12                         # exact .5 ties after scaling
    assert len(g["a_dedup"]) < len(p) and len(g["b_dedup"]) < len(g["b_scaled"])   # aliases removed
    assert not np.array_equal(g["a_dedup_index"], np.sort(g["a_dedup_index"]))        # ... and the rows reordered
    assert np.any(g["a_boxes"][:, 2] == g["a_boxes"][:, 0])                   # zero width
    assert np.any(np.signbit(g["a_dedup"][:, 0]) & (g["a_dedup"][:, 0] == 0))  # -0. kept as the first occurrence
    assert all(len(g["a_rois_fpn%d" % l]) > 0 for l in (2, 3, 4))             # several levels populated
    assert len(g["c_boxes"]) == 1 and len(g["d_boxes"]) == 0
    assert np.float32(g["a_im_scale"]) != g["a_im_scale"] and np.float32(g["b_im_scale"]) != g["b_im_scale"]
