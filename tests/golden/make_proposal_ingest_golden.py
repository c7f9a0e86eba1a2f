"""Generate tests/golden/proposal_ingest.npz from the REFERENCE ITSELF (build container only; needs /root/reference +
`make -C oracle ref`), in the style of make_golden.py, which it leaves alone.

    python tests/golden/make_proposal_ingest_golden.py

The reference's Fast R-CNN test-time preprocessing of precomputed proposals (lib/utils/preprocess_sample.py:35-45, imported in
place): `sample['dbentry']['boxes'] * im_scales[0]` with the Python-float scale of prep_im_for_blob (blob.py:74-77), then its
own remove_dup_prop (:63-70) and add_multilevel_rois_for_test (lib/utils/multilevel_rois.py:19-39), on the seeded cases of
tests/proposal_prep_ref.py (images of different sizes, scales 800/427 and 1333/1000 that are not exact in float32, engineered
1/16-grid aliases, .5 ties, zero-width boxes, counts 0, 1 and full).  Stored per case <c>: boxes, im_scale (float64), scaled,
dedup, dedup_index, dedup_inv, the FPN blobs rois_fpn2..5 and rois_idx_restore_int32, and nodedup_restore (the blobs of the
scaled rows without deduplication: remove_dup_proposals=False).
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import proposal_prep_ref as pr  # noqa: E402
import ref_harness as rh  # noqa: E402


def main():
    ns = rh.load_reference()
    ps = importlib.import_module("utils.preprocess_sample").preprocess_sample(remove_dup_proposals=True, fpn_on=True)
    arrs = {}
    for c, (h, w, s, n) in pr.CASES.items():
        boxes = pr.make_proposals(c)
        assert boxes.shape == (n, 4) and (n == 0 or bool(np.all(boxes[:, 2:] >= boxes[:, :2])))
        im_scale = float(s)                                          # a Python float, as blob.py:77 returns it
        scaled = boxes * im_scale                                    # preprocess_sample.py:36
        arrs[c + "_boxes"], arrs[c + "_im_scale"], arrs[c + "_scaled"] = boxes, np.float64(im_scale), scaled
        if n == 0:                                                   # :35 skips the proposal branch for an empty roidb entry
            arrs[c + "_dedup"], arrs[c + "_dedup_index"] = np.zeros((0, 4), np.float32), np.zeros((0,), np.int64)
            arrs[c + "_dedup_inv"] = np.zeros((0,), np.int64)
            continue
        v = np.array([1e3, 1e6, 1e9, 1e12])
        _, index, inv = np.unique(np.round(scaled * ps.spatial_scale).dot(v), return_index=True, return_inverse=True)
        dedup, inv2 = ps.remove_dup_prop(scaled)                    # the reference's own call (:38)
        assert np.array_equal(dedup, scaled[index]) and np.array_equal(inv2, inv)
        arrs[c + "_dedup"], arrs[c + "_dedup_index"], arrs[c + "_dedup_inv"] = dedup, index, inv
        blobs = ns.multilevel_rois.add_multilevel_rois_for_test({'rois': dedup}, 'rois')   # :43
        for l in range(2, 6):
            arrs["%s_rois_fpn%d" % (c, l)] = np.asarray(blobs['rois_fpn%d' % l], np.float32)
        arrs[c + "_rois_idx_restore_int32"] = np.asarray(blobs['rois_idx_restore_int32'], np.int32)
        nb = ns.multilevel_rois.add_multilevel_rois_for_test({'rois': scaled}, 'rois')
        arrs[c + "_nodedup_restore"] = np.asarray(nb['rois_idx_restore_int32'], np.int32)
    path = os.path.join(HERE, "proposal_ingest.npz")
    np.savez_compressed(path, **arrs)
    print("%-28s %7.1f KB  %d arrays" % ("proposal_ingest", os.path.getsize(path) / 1024.0, len(arrs)))
    for c in pr.CASES:
        print(c, len(arrs[c + "_boxes"]), "->", len(arrs[c + "_dedup"]))


if __name__ == "__main__":
    main()
