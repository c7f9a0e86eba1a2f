"""The mask restatement (tests/segm_eval_ref.py) against pycocotools' own maskUtils.iou / area and COCOeval 'segm', from
tests/golden/segm_eval_pycocotools.npz -- a file made by tests/golden/make_segm_eval_golden.py where pycocotools exists.  That script
has not been run: the file is absent, this test is skipped, and parity with pycocotools itself is unpinned until it is committed
(tests/README_segm_eval.md)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
import segm_eval_ref as sr

sys.path.insert(0, GOLDEN)
PATH = os.path.join(GOLDEN, "segm_eval_pycocotools.npz")


@pytest.mark.skipif(not os.path.exists(PATH), reason="tests/golden/segm_eval_pycocotools.npz has not been made (needs pycocotools)")
def test_restatement_equals_pycocotools():
    import make_segm_eval_golden as mk
    g = np.load(PATH)
    for name, case in mk.cases().items():
        want = sr.run(case)
        assert np.array_equal(want["det_area"], g[name + "_det_area"]) and np.array_equal(want["gt_mask_area"], g[name + "_gt_mask_area"])
        for n in range(len(case["dets"])):
            dr, gr = mk.rows(case, n)
            for d in dr:
                for j in gr:
                    if case["dets"][n, d, 5] == case["gt_classes"][n, j]:
                        assert want["iou"][n, d, j].tobytes() == g[name + "_iou"][n, d, j].tobytes(), (name, n, d, j)
        for k in ("precision", "recall", "stats"):
            assert want[k].tobytes() == np.ascontiguousarray(g[name + "_" + k], np.float64).tobytes(), (name, k)
