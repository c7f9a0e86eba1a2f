"""dtc_fast_rcnn_targets on the MI355X off its default point: the cases of tests/train_limit_cases.py (the table is in
tests/README.md) against the numpy restatement (tests/train_targets_ref.py) first -- all integers, max_overlaps, rois, weights,
target classes, dx, dy, every padding row and every expanded blob bit for bit -- then against what the reference's own chain gave
(tests/golden/train_targets_limits.npz) wherever the reference is defined.  -m gpu.

dw and dh: at most e_ref + 2 float32 ulps from w * log(float64(ratio)) (e_ref: the reference's own largest distance from that value
over these cases, measured by the fixture's generator; + 1 ulp for the device logarithm, + 0.5 for the multiply, + 0.5 margin), an
exact 0 an exact 0; the measured distance is printed before it is asserted.  Every output buffer is pre-filled with 0xFF, and
tests/test_train_limits_host.py holds what keeps a case from passing emptily."""
import numpy as np
import pytest
import torch

from conftest import golden
import train_limit_cases as tl
import train_targets_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return dict(golden("train_targets_limits"))


def _one(g, cid):
    """a case on its own (B = 1, strides = its sizes): the restatement, then the fixture"""
    im, params = tl.case(cid)
    o = tl.host(tl.run_ff(tl.batch([im]), params))
    tl.check(o, 0, tl.want(cid), params, float(g["e_ref"]) + 2.0, cid)
    if cid in tl.RECORDED:
        tl.check_fixture(o, 0, g, cid, len(im["rand_keys"]))
    return o


def test_sort_size_sweep(g):
    names = list(tl.SWEEP)
    params = tl.CASES["sweep_n2304"][1]
    o = tl.host(tl.run_ff(tl.batch([tl.image(n) for n in names], G=256, n_prop=2048), params))
    for b, n in enumerate(names):
        assert tl.CASES["sweep_" + n][1] == params
        tl.check(o, b, tl.want("sweep_" + n), params, float(g["e_ref"]) + 2.0, "sweep " + n)
        tl.check_fixture(o, b, g, "sweep_" + n, sum(tl.SWEEP[n]))


@pytest.mark.parametrize("name", sorted(tl.GROUPS))
def test_group_boundaries(g, name):
    o = _one(g, "group_" + name)
    if name == "neither":
        assert int(o["n_rois"][0]) == 0 and np.all(o["keep_inds"] == -1) and not o["bbox_targets"].any()


@pytest.mark.parametrize("cid", tl.QUOTA_IDS)
def test_quota_rounding_and_R(g, cid):
    _one(g, cid)


@pytest.mark.parametrize("cid", tl.THRESH_IDS)
def test_thresholds(g, cid):
    _one(g, cid)


@pytest.mark.parametrize("thresh", tl.CROWD_THRESH)
def test_crowd_threshold(g, thresh):
    _one(g, "crowd_%s" % thresh)


def test_many_gt_argmax(g):
    _one(g, "many_gt")
    _one(g, "many_gt_h")


@pytest.mark.parametrize("pattern", tl.KEY_PATTERNS)
def test_key_patterns(g, pattern):
    from detectorch_amd.utils import fast_rcnn_sample_rois as fs
    cid = "keys_" + pattern
    o = _one(g, cid)
    if pattern != "negative_int32":
        return
    im, params = tl.case(cid)                                                # ... and as int32 tensors through the Python entry
    x = tl.batch([im])
    assert x["rand_keys"].dtype == torch.int32 and int((x["rand_keys"] < 0).sum()) > 100
    blobs = fs.sample_rois_batched(x["proposals"], x["proposal_counts"], x["gt_boxes"], x["gt_classes"], x["gt_is_crowd"],
                                   x["gt_counts"], x["im_scale"], rand_keys=x["rand_keys"], rois_per_image=64)
    for mine, theirs in (("rois5", "rois"), ("labels", "labels_int32"), ("keep_inds", "keep_inds"), ("bbox_targets5", "bbox_targets5"),
                         ("bbox_targets", "bbox_targets"), ("n_fg", "n_fg"), ("n_rois", "n_rois")):
        assert tr.same_bits(o[mine], blobs[theirs].cpu().numpy()), mine


@pytest.mark.parametrize("cid", tl.REG_IDS)
def test_reg_weights_and_classes(g, cid):
    o = _one(g, cid)
    assert o["bbox_targets"].shape[2] == 4 * tl.CASES[cid][1]["num_classes"]


def _trimmed(im, n_gt, n_prop):
    """the image the kernel sees at these counts: candidate c reads rand_keys[c]"""
    return dict(im, gt_boxes=im["gt_boxes"][:n_gt], gt_classes=im["gt_classes"][:n_gt], is_crowd=im["is_crowd"][:n_gt],
                proposals=im["proposals"][:n_prop], rand_keys=im["rand_keys"][:n_gt + n_prop])


def test_counts_outside_the_stride(g):
    G, n_prop, params = 8, 320, tl.P(rois_per_image=64)
    ims = [tl.synth(50 + i, G, 1, n_prop) for i in range(4)]
    # 140 more images behind the four that are launched: stride + 1000 rows of gt, proposals and keys all lie inside the allocation
    guard = tl.batch([ims[i % 4] for i in range(144)], G=G, n_prop=n_prop)
    x = {k: v[:4] for k, v in guard.items()}
    assert all(v.is_contiguous() for v in x.values()) and guard["gt_boxes"].shape[0] * G >= 4 * G + 1000
    dev = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")
    wild = dict(x, gt_counts=dev([-5, 0, G, G + 1000]), proposal_counts=dev([n_prop + 1000, n_prop, 0, -5]))
    clamped = dict(x, gt_counts=dev([0, 0, G, G]), proposal_counts=dev([n_prop, n_prop, 0, 0]))
    a, b = tl.host(tl.run_ff(wild, params)), tl.host(tl.run_ff(clamped, params))
    for k in a:
        assert tr.same_bits(a[k], b[k]), k
    for i, (ng, npr) in enumerate([(0, n_prop), (0, n_prop), (G, 0), (G, 0)]):
        tl.check(a, i, tr.minibatch(_trimmed(ims[i], ng, npr), params), params, float(g["e_ref"]) + 2.0, "counts")


def _invoke(x, params, B, G, n_prop):
    """dtc_fast_rcnn_targets through hip.invoke, NULL for every input that is None"""
    from detectorch_amd import hip, hip_train
    out = tl.outputs_ff(B, G + n_prop, params)
    hip.invoke(hip_train.lib(), hip_train.SIGNATURES, "dtc_fast_rcnn_targets", dict(
        batch=B, gt_stride=G, proposal_stride=n_prop, params=hip_train.train_params(**params), **x, **out))
    return tl.host(out)


def test_zero_strides_with_null_pointers(g):
    params = tl.P(rois_per_image=16)
    gt_names = ("gt_boxes", "gt_classes", "gt_is_crowd", "gt_counts")
    # G stride 0, the gt pointers NULL
    ims = [tl.image("only_bg_full"), tl.image("n1_prop"), tl.synth(60, 0, 0, 100)]
    x0 = tl.batch(ims, G=0, n_prop=100)
    o0 = _invoke(dict(x0, **{k: None for k in gt_names}), params, 3, 0, 100)
    o4 = tl.host(tl.run_ff(tl.batch(ims, G=4, n_prop=100), params))
    for k in o0:
        if k in ("max_overlaps", "max_classes"):
            assert tr.same_bits(o0[k], o4[k][:, :100]) and not o4[k][:, 100:].any()
        else:
            assert tr.same_bits(o0[k], o4[k]), k
    for b, im in enumerate(ims):
        tl.check(o0, b, tr.minibatch(im, params), params, float(g["e_ref"]) + 2.0, "G = 0")
    # P stride 0, the proposal pointers NULL
    ims = [tl.image("n1_gt"), tl.hand(61, tl.GT4, [3, 7, 2, 80], [0, 1, 0, 0], np.zeros((0, 4))), _trimmed(tl.image("small"), 5, 0)]
    x0 = tl.batch(ims, G=5, n_prop=0)
    o0 = _invoke(dict(x0, proposals=None, proposal_counts=None), params, 3, 5, 0)
    o8 = tl.host(tl.run_ff(tl.batch(ims, G=5, n_prop=8), params))
    for k in o0:
        if k in ("max_overlaps", "max_classes"):
            assert tr.same_bits(o0[k], o8[k][:, :5]) and not o8[k][:, 5:].any()
        else:
            assert tr.same_bits(o0[k], o8[k]), k
    for b, im in enumerate(ims):
        tl.check(o0, b, tr.minibatch(im, params), params, float(g["e_ref"]) + 2.0, "P = 0")


def test_batch_of_300_images(g):
    G, n_prop, params = 8, 320, tl.P(rois_per_image=64)
    names = [tl.SMALL_IMAGES[i % len(tl.SMALL_IMAGES)] for i in range(300)]
    o = tl.host(tl.run_ff(tl.batch([tl.image(n) for n in names], G=G, n_prop=n_prop), params))
    alone = {}
    for n in tl.SMALL_IMAGES:
        alone[n] = tl.host(tl.run_ff(tl.batch([tl.image(n)], G=G, n_prop=n_prop), params))
        tl.check(alone[n], 0, tl.want_of(n, params), params, float(g["e_ref"]) + 2.0, "alone " + n)
    for b, n in enumerate(names):
        for k, v in o.items():
            one = alone[n][k][0]
            if k == "rois5":
                one = one.copy()
                one[:, 0] = b
            assert tr.same_bits(v[b], one), (b, n, k)


def test_device_drawn_keys_give_a_valid_sample(g):
    from detectorch_amd.utils import fast_rcnn_sample_rois as fs
    names, R = ("small", "n257", "crowd"), 64
    params = tl.P(rois_per_image=R)
    ims = [tl.image(n) for n in names]
    x = tl.batch(ims)
    gen = torch.Generator(device="cuda")

    def draw(seed):
        gen.manual_seed(seed)
        blobs = fs.sample_rois_batched(x["proposals"], x["proposal_counts"], x["gt_boxes"], x["gt_classes"], x["gt_is_crowd"],
                                       x["gt_counts"], x["im_scale"], generator=gen, rois_per_image=R)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in blobs.items()}

    first, again, other = draw(5), draw(5), draw(6)
    assert all(tr.same_bits(first[k], again[k]) for k in first)
    quota = int(np.round(params["fg_fraction"] * R))
    for b, (n, im) in enumerate(zip(names, ims)):
        w = tl.want_of(n, params)                                            # per-candidate values only: the order is the device's
        mo = w["max_overlaps"]
        fg = np.where(mo >= np.float32(params["fg_thresh"]))[0]
        bg = np.where((mo < np.float32(params["bg_thresh_hi"])) & (mo >= np.float32(params["bg_thresh_lo"])))[0]
        nf, nr = int(first["n_fg"][b]), int(first["n_rois"][b])
        keep = first["keep_inds"][b, :nr]
        assert nf == min(quota, len(fg)) and nr - nf == min(R - nf, len(bg)) and len(set(keep.tolist())) == nr
        assert np.all(np.isin(keep[:nf], fg)) and np.all(np.isin(keep[nf:], bg)) and np.all(first["keep_inds"][b, nr:] == -1)
        assert tr.same_bits(first["labels_int32"][b, :nr], np.r_[w["max_classes"][keep[:nf]], np.zeros(nr - nf, np.int32)])
        boxes = np.vstack([im["gt_boxes"], im["proposals"]])
        rois = np.hstack((np.full((nr, 1), b, np.float32), boxes[keep] * im["im_scale"]))
        assert tr.same_bits(first["rois"][b, :nr], rois)
        t5 = first["bbox_targets5"][b, :nr]
        assert tr.same_bits(t5[:, :3], w["targets5"][keep][:, :3])
        u = float(tr.ulps_from(t5[:, 3:], w["want64"][keep]).max(initial=0.0))
        print("device keys, image %s: dw / dh at most %.3f ulp (bound %.3f)" % (n, u, float(g["e_ref"]) + 2.0))
        assert u <= float(g["e_ref"]) + 2.0
        assert not tr.same_bits(first["keep_inds"][b], other["keep_inds"][b])     # another seed, another sample
