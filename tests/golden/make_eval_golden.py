"""Generates tests/golden/eval.npz: the reference's own evaluate_box_proposals (lib/utils/json_dataset_evaluator.py:238-319) on the
proposal cases of tests/eval_cases.py, for each of the eight named area ranges.

Run in the build container, where the reference tree is mounted, after `make -C oracle ref`:

    python tests/golden/make_eval_golden.py

The function is imported in place through oracle/ref_harness.py with the reference's Cython bbox_overlaps; pycocotools, which the
module imports for COCOeval and which is not installed, is a stand-in module in sys.modules (evaluate_box_proposals never touches
it).  Per case and area range the fixture records, per image, the overlaps by round (the function is run on each image on its own: its
per-image values are what the kernel writes) and, for the whole roidb, num_pos, recalls, ar and the sorted gt_overlaps.
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402
import eval_cases as ec  # noqa: E402


def load():
    rh.load_reference()
    coco = sys.modules["pycocotools"]
    stand_in = types.ModuleType("pycocotools.cocoeval")
    stand_in.COCOeval = object
    sys.modules.setdefault("pycocotools.cocoeval", stand_in)
    coco.cocoeval = sys.modules["pycocotools.cocoeval"]
    return importlib.import_module("utils.json_dataset_evaluator")


def per_round(ev, entry, area, limit):
    """the reference's per-image values by round: np.sort of the result is a permutation, so the rounds are recovered by running the
    image alone with its sort undone -- the rounds are non-increasing, so descending order is the round order"""
    r = ev.evaluate_box_proposals(None, [entry], area=area, limit=limit)
    return r['gt_overlaps'][::-1].copy(), r['num_pos']


def main():
    ev = load()
    arrs = {}
    for name, (roidb, limit) in ec.proposal_cases().items():
        rounds, meta, summary, whole = [], [], [], []
        for area in ec.AREAS:
            r = ev.evaluate_box_proposals(None, roidb, area=area, limit=limit)
            assert np.array_equal(r['thresholds'], np.arange(0.5, 0.95 + 1e-5, 0.05))
            whole.append(np.asarray(r['gt_overlaps'], np.float64))
            summary.append(np.concatenate([np.asarray(r['recalls'], np.float64), [r['ar'], r['num_pos']]]))
            for entry in roidb:
                ov, n_pos = per_round(ev, entry, area, limit)
                rounds.append(ov)
                meta.append((len(ov), n_pos))
        # [areas x images] in that order: the per-image values by round, concatenated; (entries, num_pos) per image
        arrs[name + "_rounds"] = np.concatenate(rounds)
        arrs[name + "_meta"] = np.asarray(meta, np.int64).reshape(len(ec.AREAS), len(roidb), 2)
        arrs[name + "_summary"] = np.asarray(summary, np.float64)            # [areas, 12]: ten recalls, ar, num_pos
        arrs[name + "_gt_overlaps"] = np.concatenate(whole)                  # the sorted overlaps of the roidb, area after area
    out = os.path.join(ROOT, "tests", "golden", "eval.npz")
    np.savez_compressed(out, **arrs)
    print("wrote %s: %d arrays, %d bytes" % (out, len(arrs), os.path.getsize(out)))


if __name__ == "__main__":
    main()
