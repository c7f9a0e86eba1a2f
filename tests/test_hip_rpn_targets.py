"""dtc_rpn_targets on the MI355X (-m gpu) against the numpy restatement of its contract (tests/rpn_train_ref.py) and, where recorded,
the reference's own building blocks (tests/golden/rpn_train.npz): integers, max_overlaps, gt_max, dx and dy bit for bit, dw and dh
within e_ref + 2 float32 ulps of log(float64(ratio)).  Every output -- and the workspace -- is pre-filled with 0xFF and followed by
guard words.  tests/README_rpn_train.md says what each case is for."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
import rpn_train_ref as rr

pytestmark = pytest.mark.gpu
GUARD = 64
OUT_NAMES = ("labels", "fg_index", "fg_targets", "fg_gt", "n_fg", "n_bg", "max_overlaps", "gt_max", "bbox_targets",
             "bbox_inside_weights", "bbox_outside_weights")


@pytest.fixture(scope="module")
def g():
    return golden("rpn_train")


def ff(shape, dtype):
    """a tensor of `shape` whose every byte is 0xFF, followed by GUARD words of 0xFF -> (the view, the whole allocation)"""
    n = int(np.prod(shape))
    full = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    return full[:n].view(dtype).reshape(shape), full


def levels_of(spec):
    from detectorch_amd.utils.rpn_targets import rpn_levels
    return rpn_levels([s[:3] for s in spec], [s[4] for s in spec], [s[3] for s in spec])


def outputs(levels, B, N, G, params, expanded=True, assignment=True):
    from detectorch_amd import hip, hip_rpn
    F = hip_rpn.fg_quota(params)
    f32, i32 = torch.float32, torch.int32
    shapes = dict(labels=((B, N), i32), fg_index=((B, F), i32), fg_targets=((B, F, 4), f32), fg_gt=((B, F), i32), n_fg=((B,), i32),
                  n_bg=((B,), i32), max_overlaps=((B, N), f32), gt_max=((B, G), f32), bbox_targets=((B, 4 * N), f32),
                  bbox_inside_weights=((B, 4 * N), f32), bbox_outside_weights=((B, 4 * N), f32))
    out, guards = {}, {}
    for k, (shape, dt) in shapes.items():
        skip = (k in ("max_overlaps", "gt_max") and not assignment) or (k.startswith("bbox_") and not expanded)
        out[k], guards[k] = (None, None) if skip else ff(shape, dt)
    need = hip_rpn.lib().dtc_rpn_targets_workspace_bytes(levels, len(levels), B, G)
    assert need > 0
    out["workspace"] = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")           # needs no initialisation
    return out, guards


def device_inputs(cases, G=None, nan_tail=True):
    """cases of one spec -> (gt_boxes [B,G,4], gt_is_crowd, gt_counts, im_scale, im_hw, rand_keys) on the device; rows past a case's
    own gt are NaN / garbage"""
    B = len(cases)
    G = max(len(c["gt_boxes"]) for c in cases) if G is None else G
    gt = np.full((B, G, 4), np.nan if nan_tail else 0.0, np.float32)
    crowd = np.full((B, G), 12345, np.int32)
    for b, c in enumerate(cases):
        n = len(c["gt_boxes"])
        gt[b, :n], crowd[b, :n] = c["gt_boxes"], c["is_crowd"]
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dt).contiguous()
    keys = np.stack([c["rand_keys"] for c in cases]).astype(np.uint32).view(np.int32)
    return (d(gt, torch.float32), d(crowd, torch.int32), d([c["count"] for c in cases], torch.int32),
            d([np.float32(c["im_scale"]) for c in cases], torch.float32), d([c["im_hw"] for c in cases], torch.float32),
            d(keys, torch.int32))


def run(cases, params, G=None, expanded=True, assignment=True, out=None):
    from detectorch_amd import hip_rpn
    spec = cases[0]["spec"]
    levels = levels_of(spec)
    N = rr.count_anchors(spec)
    ins = device_inputs(cases, G)
    prm = hip_rpn.rpn_train_params(**params)
    guards = None
    if out is None:
        out, guards = outputs(levels, len(cases), N, ins[0].shape[1], prm, expanded, assignment)
    hip_rpn.rpn_targets(levels, *ins, prm, out=out)
    torch.cuda.synchronize()
    if guards is not None:
        for k, full in guards.items():
            if full is not None:
                assert bool((full[-GUARD:] == -1).all()), "guard words after %s" % k
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items() if k != "workspace"}


def check(got, b, case, params, g=None, name=None, e_ref=None):
    """image b of `got` against the restatement of `case`; -> the largest dw / dh distance in ulps"""
    p = dict(rr.DEFAULTS, **params)
    m = rr.minibatch(case, p)
    for k in ("labels", "fg_index", "fg_gt"):
        assert np.array_equal(got[k][b], m[k]), k
    assert int(got["n_fg"][b]) == m["n_fg"] and int(got["n_bg"][b]) == m["n_bg"]
    if got["max_overlaps"] is not None:
        assert rr.same_bits(got["max_overlaps"][b], m["max_overlaps"])
        G = got["gt_max"].shape[1]
        assert rr.same_bits(got["gt_max"][b], np.r_[m["gt_max"], np.zeros(G - len(m["gt_max"]), np.float32)])
    t = got["fg_targets"][b]
    n = m["n_fg"]
    assert rr.same_bits(t[:, :2], m["fg_targets"][:, :2]) and not t[n:].any() and not np.signbit(t[n:]).any()
    u = float(rr.ulps_from(t[:n, 2:], m["want64"][:n]).max(initial=0.0))
    if got["bbox_targets"] is not None:                                   # the expanded blobs from the compact outputs
        bt, bi, bo = rr.expanded(case["spec"], got["labels"][b], got["fg_index"][b], t, n, m["n_bg"])
        assert rr.same_bits(got["bbox_targets"][b], bt) and rr.same_bits(got["bbox_inside_weights"][b], bi)
        assert rr.same_bits(got["bbox_outside_weights"][b], bo)
    if g is not None and name is not None:                                # the reference's own values where recorded
        N = len(m["labels"])
        rows = rr.sample_rows(name, N) if name in rr.SAMPLED_CASES else np.arange(N)
        ov = g[name + "_overlaps"]
        assert rr.same_bits(got["max_overlaps"][b][rows], ov.max(axis=1) if ov.shape[1] else np.zeros(len(rows), np.float32))
        assert rr.same_bits(t[:, :2], g[name + "_fg_targets"][:, :2])
    if e_ref is not None:
        print("dw / dh: %.3f ulps from log(float64(ratio)) (bound e_ref + 2 = %.3f)" % (u, e_ref + 2))
        assert u <= e_ref + 2
    return u


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------
def test_one_anchor(g):
    anchor = np.array([[0, 0, 15, 15]], np.float32)
    for gt, label in (([0, 0, 15, 15], 1), ([100, 100, 120, 120], 0)):
        case = dict(spec=[(1, 1, 1, 16.0, anchor)], gt_boxes=np.array([gt], np.float32), is_crowd=np.zeros(1, np.int32), count=1,
                    im_scale=1.0, im_hw=(64.0, 64.0), rand_keys=np.array([5], np.uint32))
        got = run([case], dict(batch_size_per_im=2))
        check(got, 0, case, dict(batch_size_per_im=2), e_ref=float(g["e_ref"]))
        assert got["labels"].tolist() == [[label]] and got["n_fg"][0] == label and got["n_bg"][0] == 1 - label
        assert got["fg_index"].tolist() == [[0 if label else -1]] and not got["fg_targets"].any()
        assert got["max_overlaps"][0, 0] == label


# ---- (b), (f) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rr.SIZE_CASES + ("fpn5", "c4", "fpn"))
def test_seeded_cases(g, name):
    case, params = rr.make_case(name), rr.CASES[name][5]
    got = run([case], params)
    check(got, 0, case, params, g, name, e_ref=float(g["e_ref"]))


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", sorted(rr.HAND_KEYS))
def test_hand_made_thresholds_ties_and_keys(g, keys):
    case = rr.hand_case(keys)
    got = run([case], rr.HAND_PARAMS)
    check(got, 0, case, rr.HAND_PARAMS, g, "hand" if keys == "random" else None, e_ref=float(g["e_ref"]))
    if keys == "equal":
        assert got["fg_index"][0].tolist() == [0, 2, 4, 7] and np.where(got["labels"][0] == 0)[0].tolist() == [5, 11, 12, 13]
    if keys == "extremes":
        assert got["fg_index"][0].tolist() == [0, 2, 4, 8]
    assert got["gt_max"][0, 6] == 0 and got["fg_gt"][0].max() <= 5


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", sorted(rr.STRADDLE_INSIDE))
def test_straddle(g, st):
    case, p = rr.straddle_case(st)
    params = dict(batch_size_per_im=8, straddle_thresh=st)
    got = run([case], params)
    check(got, 0, case, params, e_ref=float(g["e_ref"]))
    inside = np.array(rr.STRADDLE_INSIDE[st], bool)
    assert np.all(got["labels"][0][~inside] == -1) and not got["max_overlaps"][0][~inside].any()
    assert np.all(got["max_overlaps"][0][[0, 3]] == 1) and (got["max_overlaps"][0][6] == 1) == bool(inside[6])


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------
def test_gt_rows_and_counts(g):
    base, params = rr.make_case("n255"), rr.CASES["n255"][5]
    e_ref = float(g["e_ref"])
    rs = np.random.RandomState(3)
    many = rr.make_case("n1023")
    anchors = rr.anchors_of(many["spec"])
    big = anchors[rs.choice(len(anchors), 256, replace=False)] + rs.uniform(-3, 3, (256, 4)).astype(np.float32)
    big[:, 2:] = np.maximum(big[:, 2:], big[:, :2] + 1)
    variants = [
        (dict(base, count=0), params, None),                                                  # no gt
        (dict(base, is_crowd=np.ones(3, np.int32)), params, None),                            # crowd only
        (dict(base, count=-3), params, None), (dict(base, count=3 + 5), params, None),        # clamped counts
        (dict(base, count=2), params, 7),                                                     # NaN rows past the count
        (dict(many, gt_boxes=big, is_crowd=(rs.rand(256) < 0.1).astype(np.int32), count=256), rr.CASES["n1023"][5], None),   # 256 gt
    ]
    for case, prm, G in variants:
        got = run([case], prm, G=G)
        check(got, 0, case, prm, e_ref=e_ref)
    got = run([dict(base, count=0)], params)
    assert got["n_fg"][0] == 0 and got["n_bg"][0] == 8 and not got["max_overlaps"].any() and np.all(got["fg_index"] == -1)
    got = run([dict(base, is_crowd=np.ones(3, np.int32))], params)
    assert got["n_fg"][0] == 0 and not got["gt_max"].any()


def test_batch_of_three_equals_three_calls(g):
    base, params = rr.make_case("fpn5"), rr.CASES["fpn5"][5]
    rs = np.random.RandomState(4)
    cases = [base,
             dict(base, im_hw=(150.0, 256.0), im_scale=1.5, count=4, rand_keys=rs.randint(0, 2 ** 32, 12276, dtype=np.uint64).astype(np.uint32)),
             dict(base, im_hw=(192.0, 201.0), im_scale=1.7, count=6, rand_keys=rs.randint(0, 2 ** 32, 12276, dtype=np.uint64).astype(np.uint32))]
    got = run(cases, params)
    for b, c in enumerate(cases):
        check(got, b, c, params, e_ref=float(g["e_ref"]))
        one = run([c], params, G=6)
        for k in OUT_NAMES:
            assert rr.same_bits(got[k][b], one[k][0]), (b, k)
    assert len({got["labels"][b].tobytes() for b in range(3)}) == 3


# ---- (g) ------------------------------------------------------------------------------------------------------------------------------
def test_repeat_capture_and_inputs_rewritten_in_place(g):
    from detectorch_amd import hip_rpn
    name = "fpn5"
    case, params = rr.make_case(name), rr.CASES[name][5]
    spec = case["spec"]
    levels, N = levels_of(spec), rr.count_anchors(spec)
    prm = hip_rpn.rpn_train_params(**params)
    ins = device_inputs([case, case])
    snap = lambda o: {k: o[k].cpu().numpy().copy() for k in OUT_NAMES}
    eager = []
    for _ in range(2):
        out, _ = outputs(levels, 2, N, ins[0].shape[1], prm)
        hip_rpn.rpn_targets(levels, *ins, prm, out=out)
        torch.cuda.synchronize()
        eager.append(snap(out))
    out, _ = outputs(levels, 2, N, ins[0].shape[1], prm)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            hip_rpn.rpn_targets(levels, *ins, prm, out=out)
    replays = []
    for _ in range(2):
        for k in OUT_NAMES:
            out[k].view(torch.int32).fill_(-1)                                               # a replay over stale buffers is clean
        graph.replay()
        torch.cuda.synchronize()
        replays.append(snap(out))
    for other in (eager[1], replays[0], replays[1]):
        for k in OUT_NAMES:
            assert rr.same_bits(eager[0][k], other[k]), k
    # gt, im_hw and the keys rewritten in place: the replay gives the eager bits of the new values
    rs = np.random.RandomState(9)
    new = dict(case, gt_boxes=(case["gt_boxes"] + rs.uniform(-2, 2, case["gt_boxes"].shape)).astype(np.float32), im_hw=(180.0, 240.0),
               rand_keys=rs.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32))
    for dst, src in zip(ins, device_inputs([new, case])):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    replayed = snap(out)
    fresh = run([new, case], params)
    for k in OUT_NAMES:
        assert rr.same_bits(replayed[k], fresh[k]), k
    check(replayed, 0, new, params, e_ref=float(g["e_ref"]))
    assert not rr.same_bits(replayed["labels"][0], eager[0]["labels"][0])


def test_null_groups(g):
    case, params = rr.make_case("n257"), rr.CASES["n257"][5]
    full = run([case], params)
    for expanded, assignment in ((False, True), (True, False), (False, False)):
        got = run([case], params, expanded=expanded, assignment=assignment)
        for k in OUT_NAMES:
            assert got[k] is None or rr.same_bits(got[k], full[k]), k
    none = dict(params, fg_fraction=0.0)                                                      # F = 0: no fg rows at all
    got = run([case], none)
    check(got, 0, case, none)
    assert got["fg_index"].shape == (1, 0) and got["n_fg"][0] == 0 and got["n_bg"][0] == 8


def test_bad_argument_sets_write_nothing():
    from detectorch_amd import hip_rpn
    case, params = rr.make_case("n63"), rr.CASES["n63"][5]
    spec = case["spec"]
    levels, N = levels_of(spec), rr.count_anchors(spec)
    ins = device_inputs([case])
    L = hip_rpn.lib()
    bad = [(dict(batch_size_per_im=0), {}, -1), (dict(negative_overlap=0.9), {}, -1), (dict(batch_size_per_im=4097), {}, -4),
           ({}, dict(labels=None), -1), ({}, dict(bbox_targets=None), -1), ({}, dict(workspace_bytes=16), -3), ({}, dict(gt_counts=None), -1)]
    for kw, nulls, code in bad:
        prm = hip_rpn.rpn_train_params(**dict(params, **kw))
        out, guards = outputs(levels, 1, N, 3, hip_rpn.rpn_train_params(**params))
        args = dict(levels=levels, n_levels=1, batch=1, gt_boxes=ins[0], gt_is_crowd=ins[1], gt_counts=ins[2], gt_stride=3,
                    im_scale=ins[3], im_hw=ins[4], rand_keys=ins[5], params=prm, workspace=out["workspace"],
                    workspace_bytes=out["workspace"].numel(), stream=None, **{k: out[k] for k in OUT_NAMES})
        args.update(nulls)
        _, _, convert = hip_rpn.SIGNATURES["dtc_rpn_targets"]
        assert L.dtc_rpn_targets(*[c(args[n]) for n, c in convert]) == code, (kw, nulls)
        torch.cuda.synchronize()
        for k, full in guards.items():
            assert bool((full == -1).all()), (kw, nulls, k)
        assert bool((out["workspace"] == 0xFF).all())


# ---- (h) - (k): past the sizes and key patterns above (rr.TARGET_CASES; test_rpn_train_host.py asserts what each one reaches) --------
WORST_ULPS = {}


def run_case(g, name):
    """every image of rr.target_case(name) in ONE call against its restatement -> (outputs, cases, params)"""
    cases, params = rr.target_case(name)
    got = run(cases, params)
    for b, c in enumerate(cases):
        WORST_ULPS[name] = max(WORST_ULPS.get(name, 0.0), check(got, b, c, params, e_ref=float(g["e_ref"])))
    return got, cases, params


def key_order(case, idx):
    """the 52-bit keys of the anchors idx"""
    return (case["rand_keys"].astype(np.uint64)[idx] << np.uint64(20)) | idx.astype(np.uint64)


# ---- (h) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cluster_" + k for k in rr.CLUSTER_SETS] + ["c4_arange"])
def test_clustered_keys(g, name):
    got, (case,), _ = run_case(g, name)
    bg = np.where(got["labels"][0] == 0)[0]
    if name in ("cluster_arange", "c4_arange"):                                               # the first bg candidates in index order
        assert bg.max() < 2 * len(bg) + 200
    if name == "cluster_reversed":
        assert bg.min() > rr.count_anchors(case["spec"]) - 2 * len(bg) - 200


@pytest.mark.parametrize("name", sorted(rr.DIGIT_FIELDS))
def test_every_digit_decides(g, name):
    run_case(g, name)


def test_clustered_batch_of_three_equals_three_calls(g):
    got, cases, params = run_case(g, "cluster_b3")
    for b, c in enumerate(cases):
        one = run([c], params, G=3)
        for k in OUT_NAMES:
            assert rr.same_bits(got[k][b], one[k][0]), (b, k)
    assert len({got["labels"][b].tobytes() for b in range(3)}) == 3


# ---- (i) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.QUOTA_PARAMS))
def test_large_quotas_and_the_sort_branches(g, name):
    got, (case,), params = run_case(g, name)
    R, frac, thresh, count = rr.QUOTA_PARAMS[name]
    n, F = int(got["n_fg"][0]), int(frac * R)
    assert got["fg_index"].shape == (1, F) and n + int(got["n_bg"][0]) == (n if thresh == 0 else R)
    rows = got["fg_index"][0, :n]
    assert np.all(np.diff(key_order(case, rows).astype(np.int64)) > 0)                        # sampling order: ascending (key, index)
    assert n == F or thresh > 0                                                               # every anchor is fg: the quota is met
    if count == 0:
        assert np.all(got["fg_gt"] == -1) and not got["fg_targets"].any() and not got["bbox_targets"].any()
        assert int(got["bbox_inside_weights"].sum()) == 4 * n
    else:
        zero = got["max_overlaps"][0][rows] == 0                                              # fg whose best IoU is 0: the first gt
        assert got["fg_gt"][0, :n].min() >= 0 and zero.any() == (thresh == 0) and np.all(got["fg_gt"][0, :n][zero] == 0)


# ---- (j) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["switch_%d" % n for n in rr.SWITCH_SHAPES])
def test_group_switch_with_two_images(g, name):
    got, cases, _ = run_case(g, name)
    assert not rr.same_bits(got["labels"][0], got["labels"][1])


def test_two_to_the_twenty_anchors(g):
    got, (case,), _ = run_case(g, "full_2p20")
    assert got["labels"].shape == (1, 1 << 20)
    assert got["fg_index"][0].max() >= 1 << 19 and np.where(got["labels"][0] == 0)[0].min() >= 1 << 19


def test_batch_of_300(g):
    got, cases, _ = run_case(g, "batch_300")
    assert len(cases) == 300 and len({got["labels"][b].tobytes() for b in range(300)}) > 150


def test_print_the_largest_dw_dh_distances():
    print("largest dw / dh distance in ulps per case of (h) - (k): %s" % {k: round(v, 3) for k, v in WORST_ULPS.items()})
