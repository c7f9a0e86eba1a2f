"""Generate tests/golden/rpn_train.npz from the REFERENCE ITSELF (build container only; needs the reference tree and
`make -C oracle ref`), in the style of make_train_targets_golden.py.

    python tests/golden/make_rpn_train_golden.py

The reference has no RPN training; what the contract of include/detectorch_rpn_hip.h is built from is the reference's own and is run
here, imported in place, on the cases of tests/rpn_train_ref.py:
  * utils.generate_anchors.generate_anchors and model.generate_proposals.GenerateProposals.get_all_anchors (:124-149): the shifted
    anchors of every level, reordered from its (h, w, a) rows to the contract's (a, h, w) index;
  * cython_bbox.bbox_overlaps of those anchors (the inside ones) against the scaled non-crowd gt;
  * utils.boxes.bbox_transform_inv (:211-242) of the restatement's sampled foreground anchors against their gt;
  * model.loss.smooth_L1 (:13-20) on the expanded blobs and torch.nn.functional.binary_cross_entropy_with_logits over the sampled
    anchors, in float64 (the yardstick `y`) and in float32 (e_ref: the float32 CPU reference's own distance from y).

Stored per targets case <c>: <c>_anchors [N,4] and <c>_overlaps [N,G'] (rows outside the image zero; G': the non-crowd gt) -- for the
cases of rpn_train_ref.SAMPLED_CASES only the rows rpn_train_ref.sample_rows names -- <c>_fg_targets [F,4] (the reference's deltas of
the restatement's fg rows) and the restatement's integers (<c>_labels as int8, <c>_fg_index, <c>_fg_gt, <c>_n).
e_ref: the largest distance of the reference's dw / dh from log(float64(ratio)), in float32 ulps, over all cases.
Per loss case <c>: loss_<c>_cls, loss_<c>_bbox (float64), loss_<c>_e_ref_cls, loss_<c>_e_ref_box, loss_<c>_grad_cls and
loss_<c>_grad_box (float64 autograd gradients of level 0, at most 2000 sampled elements), loss_<c>_e_grad (the float32 reference's
gradient distances in units of the two gradient bounds).
The archive is written with fixed zip timestamps: the same inputs give the same bytes.
"""
import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402
import rpn_train_ref as rr  # noqa: E402


def load():
    ns = rh.load_reference()
    for name in ("torchvision", "torchvision.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    stand_in = types.ModuleType("model.roi_align")
    stand_in.RoIAlign = object
    sys.modules.setdefault("model.roi_align", stand_in)
    utils = importlib.import_module("utils.utils")
    for name in ("isnan", "infbreak", "printmax"):
        if not hasattr(utils, name):
            setattr(utils, name, None)
    ns.loss = importlib.import_module("model.loss")
    return ns


def reference_anchors(ns, spec):
    """get_all_anchors per level, (h, w, a) rows -> (a, h, w)"""
    out = []
    for A, H, W, stride, base in spec:
        gen = ns.generate_proposals.GenerateProposals.__new__(ns.generate_proposals.GenerateProposals)
        gen._anchors, gen._num_anchors = np.asarray(base, np.float64), A
        all_anchors = gen.get_all_anchors(1, H, W, 1.0 / stride)
        out.append(all_anchors.reshape(H, W, A, 4).transpose(2, 0, 1, 3).reshape(-1, 4))
    return np.concatenate(out)


def write_npz(path, arrs):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def loss_chain(ns, c, dtype):
    """-> (loss_cls, loss_bbox, grad of level 0's logits, grad of level 0's deltas) as float64"""
    spec, B = c["spec"], c["labels"].shape[0]
    off = rr.offsets(spec)
    nv = np.clip(c["n_fg"], 0, None).astype(np.int64) + np.clip(c["n_bg"], 0, None)
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    cls = [t(x).requires_grad_() for x in c["cls"]]
    box = [t(x).requires_grad_() for x in c["box"]]
    flat_cls = torch.cat([x.reshape(B, -1) for x in cls], 1)
    labels = torch.from_numpy(c["labels"])
    valid = (labels == 0) | (labels == 1)
    loss_cls = torch.nn.functional.binary_cross_entropy_with_logits(flat_cls[valid], (labels[valid] == 1).to(dtype), reduction="sum") \
        / max(int(nv.sum()), 1)
    ex = [rr.expanded(spec, c["labels"][b], c["fg_index"][b], c["fg_targets"][b], int(c["n_fg"][b]), int(c["n_bg"][b])) for b in range(B)]
    bt, bi = (np.stack([e[k] for e in ex]) for k in (0, 1))
    bo = np.stack([(ex[b][2] > 0) / np.float64(max(nv[b], 1)) for b in range(B)])      # float64 weights for the yardstick
    if dtype == torch.float32:
        bo = np.stack([e[2] for e in ex])
    flat_box = torch.cat([x.reshape(B, -1) for x in box], 1)
    loss_bbox = ns.loss.smooth_L1(flat_box, t(bt), t(bi), t(bo), float(np.float32(1.0 / 9.0)))
    (loss_cls + loss_bbox).backward()
    return float(loss_cls.detach()), float(loss_bbox.detach()), cls[0].grad.double().numpy(), box[0].grad.double().numpy()


def main():
    ns = load()
    arrs, e_ref = {}, 0.0
    for name in rr.GOLDEN_CASES:
        case, params = rr.make_case(name), rr.params_of(name)
        spec = case["spec"]
        m = rr.minibatch(case, params)
        for l, (A, H, W, stride, base) in enumerate(spec):
            if name not in ("hand",):                                        # the models' anchors are generate_anchors' own
                sizes, ratios = rr._SETS[A]
                sizes = (32 * 2 ** l,) if name in ("fpn5", "fpn") else sizes
                want = ns.generate_anchors.generate_anchors(stride=stride, sizes=sizes, aspect_ratios=ratios)
                assert np.array_equal(np.asarray(base, np.float64), want), (name, l)
        anchors = reference_anchors(ns, spec)
        assert np.array_equal(anchors, anchors.astype(np.float32)) and rr.same_bits(anchors.astype(np.float32), m["anchors"]), name
        anchors = anchors.astype(np.float32)
        n_g = case["count"]
        gt = (case["gt_boxes"][:n_g] * np.float32(case["im_scale"])).astype(np.float32)
        ok = case["is_crowd"][:n_g] == 0
        ov = np.zeros((len(anchors), int(ok.sum())), np.float32)
        inside = m["inside"]
        ov[inside] = ns.cython_bbox.bbox_overlaps(anchors[inside].astype(np.float32), gt[ok].astype(np.float32))
        n = m["n_fg"]
        ft = np.zeros((len(m["fg_index"]), 4), np.float32)
        if n:
            ft[:n] = ns.boxes.bbox_transform_inv(anchors[m["fg_index"][:n]], gt[m["fg_gt"][:n]], (1.0, 1.0, 1.0, 1.0))
            u = rr.ulps_from(ft[:n, 2:], m["want64"][:n])
            e_ref = max(e_ref, float(u.max()))
        rows = rr.sample_rows(name, len(anchors)) if name in rr.SAMPLED_CASES else np.arange(len(anchors))
        arrs.update({name + "_anchors": anchors[rows], name + "_overlaps": ov[rows], name + "_fg_targets": ft,
                     name + "_labels": m["labels"].astype(np.int8), name + "_fg_index": m["fg_index"], name + "_fg_gt": m["fg_gt"],
                     name + "_n": np.array([m["n_fg"], m["n_bg"], int(m["fg"].sum()), int(m["bg"].sum())], np.int32)})
        print("%-6s N %6d  inside %6d  fg %4d  bg %6d  taken %3d + %3d" % (name, len(anchors), int(inside.sum()), int(m["fg"].sum()),
                                                                          int(m["bg"].sum()), m["n_fg"], m["n_bg"]))
    arrs["e_ref"] = np.float64(e_ref)
    for name in rr.LOSS_CASES:
        c = rr.make_loss_case(name)
        y, r = loss_chain(ns, c, torch.float64), loss_chain(ns, c, torch.float32)
        mine = rr.y_of(c)
        b = rr.loss_bounds(mine)
        keep = lambda a: a.ravel()[rr.sample_rows(name, a.size)]
        nz = y[3] != 0
        e_gc = float(np.max(np.abs(r[2] - y[2]))) / b["grad_cls"]
        e_gb = float(np.max(np.abs(r[3][nz] - y[3][nz]) / np.abs(y[3][nz]))) / b["grad_box"] if nz.any() else 0.0
        arrs.update({"loss_" + name + "_cls": np.float64(y[0]), "loss_" + name + "_bbox": np.float64(y[1]),
                     "loss_" + name + "_e_ref_cls": np.float64(abs(r[0] - y[0])), "loss_" + name + "_e_ref_box": np.float64(abs(r[1] - y[1])),
                     "loss_" + name + "_grad_cls": keep(y[2]), "loss_" + name + "_grad_box": keep(y[3]),
                     "loss_" + name + "_e_grad": np.array([e_gc, e_gb])})
        print("%-6s loss_cls %.6f loss_bbox %.6f | float32 reference: loss_cls %.2f loss_bbox %.2f of their bounds (4 e_ref arm "
              "excluded), grad_cls %.2f grad_box %.2f of theirs" % (
                  name, y[0], y[1], abs(r[0] - y[0]) / (32 * rr.EPS * max(abs(mine["loss_cls"]), mine["scale_cls"])),
                  abs(r[1] - y[1]) / (32 * rr.EPS * abs(mine["loss_bbox"])) if mine["loss_bbox"] else 0.0, e_gc, e_gb))
    path = os.path.join(HERE, "rpn_train.npz")
    write_npz(path, arrs)
    print("%-28s %7.1f KB  %d arrays  e_ref %.3f ulp" % ("rpn_train", os.path.getsize(path) / 1024.0, len(arrs), e_ref))


if __name__ == "__main__":
    main()
