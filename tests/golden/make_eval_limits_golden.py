"""Generates tests/golden/eval_limits.npz: the reference's own evaluate_box_proposals (lib/utils/json_dataset_evaluator.py:238-319) on
the proposal cases of tests/eval_limit_cases.py, under 'all' and 'medium'.

Run in the build container, where the reference tree is mounted, after `make -C oracle ref`:

    python tests/golden/make_eval_limits_golden.py

The function is imported in place through oracle/ref_harness.py exactly as tests/golden/make_eval_golden.py does (its Cython
bbox_overlaps, a stand-in pycocotools).  Only outputs are stored -- per case and area range the overlaps by round of every image,
(entries, num_pos) per image, and the ten recalls, ar and num_pos of the whole roidb; the inputs are regenerated from their seeds.
np.savez_compressed writes no time stamp: a second run gives the same bytes.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import eval_limit_cases as lc  # noqa: E402
from make_eval_golden import load, per_round  # noqa: E402


def main():
    ev = load()
    arrs = {}
    for name, case in lc.proposal_cases().items():
        roidb, limit = [dict(e) for e in case["roidb"]], case["limit"]
        rounds, meta, summary = [], [], []
        for area in lc.PROPOSAL_AREAS:
            r = ev.evaluate_box_proposals(None, roidb, area=area, limit=limit)
            summary.append(np.concatenate([np.asarray(r['recalls'], np.float64), [r['ar'], r['num_pos']]]))
            for entry in roidb:
                ov, n_pos = per_round(ev, entry, area, limit)
                rounds.append(ov)
                meta.append((len(ov), n_pos))
        arrs[name + "_rounds"] = np.concatenate(rounds).astype(np.float64)
        arrs[name + "_meta"] = np.asarray(meta, np.int64).reshape(len(lc.PROPOSAL_AREAS), len(roidb), 2)
        arrs[name + "_summary"] = np.asarray(summary, np.float64)            # [areas, 12]: ten recalls, ar, num_pos
    out = os.path.join(ROOT, "tests", "golden", "eval_limits.npz")
    np.savez_compressed(out, **arrs)
    print("wrote %s: %d arrays, %d bytes" % (out, len(arrs), os.path.getsize(out)))


if __name__ == "__main__":
    main()
