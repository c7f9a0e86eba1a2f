"""Generate tests/golden/collect_levels.npz from the REFERENCE ITSELF (build container only; needs the reference tree +
`make -C oracle ref`), in the style of make_golden.py, which it leaves alone (collect_distribute.npz keeps lvl_boxes at (2, 5)).

    python tests/golden/make_collect_levels_golden.py

On the boundary boxes of tests/collect_args_cases.py (sqrt(area) / 224 exactly 2^j for j = -4 ... 4, a few float32 ulps either side,
inside and just outside the 1e-6 band below 2^j, a 1 x 1 box, a zero-area box, a box whose float32 area overflows) and for every
level range of collect_args_cases.K_RANGES:
  * lvls_<kmin>_<kmax>     the reference's map_rois_to_fpn_levels (lib/utils/multilevel_rois.py:41-53, imported in place), int32;
  * order_/counts_/restore_<kmin>_<kmax>   the numpy half of the reference's distribute
    (lib/model/collect_and_distribute_fpn_rpn_proposals.py:108-128, called in place on a CPU tensor of the boxes): the per-level index
    lists concatenated, their lengths, and rois_idx_restore.
No scores are involved, so nothing here depends on a tie order.  The archive is written with fixed member timestamps, so that
running the generator again gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import collect_args_cases as cc  # noqa: E402


def save_deterministic(path, arrs):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrs[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ns = rh.load_reference()
    boxes, kind, j = cc.boundary_boxes()
    arrs = {"boxes": boxes, "j": j, "kind_code": np.array([("exact", "ulp", "band", "edge").index(k) for k in kind], np.int8)}
    with np.errstate(over="ignore", divide="ignore"):
        for k_min, k_max in cc.K_RANGES:
            tag = "%d_%d" % (k_min, k_max)
            lv = ns.multilevel_rois.map_rois_to_fpn_levels(boxes, k_min, k_max)
            assert np.all(lv == np.floor(lv)) and lv.min() >= k_min and lv.max() <= k_max
            arrs["lvls_" + tag] = lv.astype(np.int32)
            distr, restore = ns.collect.distribute(torch.from_numpy(boxes.copy()), k_min, k_max)
            assert len(distr) == k_max - k_min + 1
            arrs["counts_" + tag] = np.array([int(d.shape[0]) for d in distr], np.int32)
            arrs["restore_" + tag] = np.asarray(restore, np.int64)
            # the per-level lists themselves, as indices: the rows of distr, level by level, are boxes[order]
            order = np.argsort(np.asarray(restore), kind="stable").astype(np.int64)
            got = np.concatenate([np.asarray(d).reshape(-1, 4) for d in distr])
            assert got.view(np.uint32).tolist() == boxes[order].view(np.uint32).tolist()
            arrs["order_" + tag] = order
    path = os.path.join(HERE, "collect_levels.npz")
    save_deterministic(path, arrs)
    print("%-28s %7.1f KB  %s" % ("collect_levels", os.path.getsize(path) / 1024.0, sorted(arrs)))


if __name__ == "__main__":
    main()
