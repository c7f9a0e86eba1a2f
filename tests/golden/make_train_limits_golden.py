"""Generate tests/golden/train_targets_limits.npz from the REFERENCE ITSELF (needs the reference tree and
`make -C oracle ref`): the reference's training-minibatch chain, imported in place through make_train_targets_golden.load() /
run_chain() (the stand-ins are described there), on every (image, parameter set) of tests/train_limit_cases.CASES for which the
reference is defined (train_limit_cases.RECORDED).

    python tests/golden/make_train_limits_golden.py

Outputs only.  Per case <c>:
    <c>_kept          int32 [2, n_rois]: keep_inds, labels;    <c>_n_fg
    <c>_sha           uint8 [4, 32], four SHA-256 (train_limit_cases.SHA_ROWS):
        inputs        of the seeded inputs and the parameter set (train_limit_cases.input_digest), in place of the inputs
        assign        of max_overlaps, max_classes and the (class, dx, dy) columns of the entry's bbox_targets, every candidate
        overlap       of max_overlaps and max_classes
        kept          of rois and of the (class, dx, dy) columns of bbox_targets[keep_inds]
    <c>_max_overlaps, <c>_max_classes, <c>_targets5, <c>_rois    the arrays themselves, for the images of at most FULL_MAX candidates
    <c>_bbox_targets, <c>_bbox_inside_weights, <c>_bbox_outside_weights    for train_limit_cases.EXPANDED_IDS
e_ref: the largest distance of the reference's own dw / dh from w * log(float64(ratio)), in float32 ulps of that value, over these
cases, measured as make_train_targets_golden.py measures it.  The file is byte-reproducible (fixed member order and dates).
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_train_targets_golden as mt  # noqa: E402
import train_limit_cases as tl  # noqa: E402
import train_targets_ref as tr  # noqa: E402

FULL_MAX = 130


def save_deterministic(path, arrs):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrs):
            buf = io.BytesIO()
            a = np.asarray(arrs[name])
            np.lib.format.write_array(buf, np.ascontiguousarray(a) if a.ndim else a, allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ns = mt.load()
    arrs, e_ref = {}, 0.0
    for c in tl.RECORDED:
        case, params = tl.case(c)
        entry, blobs, keep = mt.run_chain(ns, case, params)
        mo = np.asarray(entry["max_overlaps"])
        t5 = entry["bbox_targets"]
        assert mo.dtype == np.float32 and t5.dtype == np.float32
        n_fg = min(int(np.round(params["fg_fraction"] * params["rois_per_image"])), int(np.sum(mo >= params["fg_thresh"])))
        mc = np.asarray(entry["max_classes"], np.int32)
        rois = np.asarray(blobs["rois"], np.float32)
        assert blobs["rois"].dtype == np.float32 and len(rois) == len(keep)
        assert blobs["labels_int32"].dtype == np.int32 and keep.dtype == np.int32
        arrs[c + "_kept"], arrs[c + "_n_fg"] = np.stack([keep, blobs["labels_int32"]]), np.int32(n_fg)
        arrs[c + "_sha"] = np.stack([tl.input_digest(c), tl.assign_digest(mo, mc, t5), tl.sha(mo, mc), tl.kept_digest(rois, t5[keep])])
        if len(mo) <= FULL_MAX:
            arrs[c + "_max_overlaps"], arrs[c + "_max_classes"], arrs[c + "_targets5"], arrs[c + "_rois"] = mo, mc, t5, rois
        if c in tl.EXPANDED_IDS:
            if not params["cls_agnostic_bbox_reg"]:                          # fast_rcnn_sample_rois expands with the default 81 classes
                bt, bw = ns.sample._expand_bbox_targets(t5[keep, :], params["num_classes"], False)
                blobs.update(bbox_targets=bt, bbox_inside_weights=bw, bbox_outside_weights=np.array(bw > 0, dtype=bw.dtype))
            for k in tl.EXPANDED:
                assert blobs[k].dtype == np.float32
                arrs[c + "_" + k] = blobs[k]
        # the reference's own distance from the float64 yardstick (the ratios are the restatement's, whose dx / dy and target
        # classes are bit-equal to the reference's: the same gt was assigned)
        mine = tl.want(c)
        assert tr.same_bits(mine["targets5"][:, :3], t5[:, :3]), c
        u = tr.ulps_from(t5[:, 3:], mine["want64"])
        worst = float(u.max()) if u.size else 0.0
        e_ref = max(e_ref, worst)
        print("%-24s candidates %4d  fg %4d  bg %4d  filtered %3d  kept %4d (fg %4d)  max ulps of dw/dh %.2f" % (
            c, len(mo), int(np.sum(mo >= params["fg_thresh"])),
            int(np.sum((mo < params["bg_thresh_hi"]) & (mo >= params["bg_thresh_lo"]))),
            int(np.sum(mo[len(case["gt_boxes"]):] == -1)), len(keep), n_fg, worst))
    assert np.isfinite(e_ref)
    arrs["e_ref"] = np.float64(e_ref)
    path = os.path.join(HERE, "train_targets_limits.npz")
    save_deterministic(path, arrs)
    print("%-28s %7.1f KB  %d arrays  e_ref %.3f ulp" % ("train_targets_limits", os.path.getsize(path) / 1024.0, len(arrs), e_ref))


if __name__ == "__main__":
    main()
