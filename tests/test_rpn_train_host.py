"""RPN training without a GPU:
  * the numpy restatement (tests/rpn_train_ref.py) against the reference's own building blocks (tests/golden/rpn_train.npz, made by
    tests/golden/make_rpn_train_golden.py): anchors, integers, overlaps as float32 bits, dx and dy bit for bit, dw and dh within
    e_ref + 2 float32 ulps of log(float64(ratio)) -- the rule of tests/README_train_targets.md; the float64 loss yardsticks
    against torch's and the reference's own float64 chain;
  * every condition the cases of tests/README_rpn_train.md name actually occurs -- for the large and clustered cases (rr.TARGET_CASES,
    rr.LOSS_BIG_CASES) through rr.selection_profile, with the thresholds of the kernels read from the source text;
  * libdetectorch_rpn_hip.so exports exactly what include/detectorch_rpn_hip.h declares and hip_rpn.SIGNATURES binds it, parameter
    names in order; the other five libraries' export lists are unchanged;
  * the return codes of both entries on bad arguments, in the order shapes, limits, pointers, workspace (validation precedes every
    HIP call: taken in a child process that sees no device); workspace sizes against their restatement; CPU tensors raise;
  * the block constants of the tests are those of the source text.
Run as a script with --codes the module prints the return-code table as JSON (the child process of the test)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden
import rpn_train_ref as rr

sys.path.insert(0, GOLDEN)


@pytest.fixture(scope="module")
def g():
    return golden("rpn_train")


@pytest.fixture(scope="module")
def mb():
    return {c: rr.minibatch(rr.make_case(c), rr.params_of(c)) for c in rr.GOLDEN_CASES}


# ---- the restatement against the reference's building blocks ------------------------------------------------------------------------
@pytest.mark.parametrize("case", rr.GOLDEN_CASES)
def test_restatement_equals_reference(g, mb, case):
    c, m = rr.make_case(case), mb[case]
    N = rr.count_anchors(c["spec"])
    rows = rr.sample_rows(case, N) if case in rr.SAMPLED_CASES else np.arange(N)
    assert rr.same_bits(m["anchors"][rows], g[case + "_anchors"])
    n_g = c["count"]
    gt = (c["gt_boxes"][:n_g] * np.float32(c["im_scale"])).astype(np.float32)
    ok = c["is_crowd"][:n_g] == 0
    ov = np.zeros((N, int(ok.sum())), np.float32)
    ov[m["inside"]] = rr.bbox_overlaps(m["anchors"][m["inside"]], gt[ok])
    assert rr.same_bits(ov[rows], g[case + "_overlaps"])
    assert rr.same_bits(ov.max(axis=1), m["max_overlaps"]) and rr.same_bits(ov.max(axis=0), m["gt_max"][:n_g][ok])
    assert rr.same_bits(m["labels"].astype(np.int8), g[case + "_labels"])                     # the seeded cases are reproducible
    assert rr.same_bits(m["fg_index"], g[case + "_fg_index"]) and rr.same_bits(m["fg_gt"], g[case + "_fg_gt"])
    assert [m["n_fg"], m["n_bg"], int(m["fg"].sum()), int(m["bg"].sum())] == g[case + "_n"].tolist()
    want = g[case + "_fg_targets"]
    assert rr.same_bits(m["fg_targets"][:, :2], want[:, :2])                                  # dx, dy
    n = m["n_fg"]
    bound = float(g["e_ref"]) + 2.0
    assert rr.ulps_from(m["fg_targets"][:n, 2:], m["want64"][:n]).max(initial=0.0) <= bound
    assert rr.ulps_from(want[:n, 2:], m["want64"][:n]).max(initial=0.0) <= float(g["e_ref"])
    assert not m["fg_targets"][n:].any() and np.all(m["fg_index"][n:] == -1) and np.all(m["fg_gt"][n:] == -1)


@pytest.mark.parametrize("case", rr.LOSS_CASES)
def test_loss_yardstick_equals_reference(g, case):
    c = rr.make_loss_case(case)
    y = rr.y_of(c)
    # two float64 evaluations of the same sums in different orders: a few float64 roundings of at most 2 * 121 515 terms
    assert abs(y["loss_cls"] - float(g["loss_%s_cls" % case])) <= 1e-12 * max(1.0, y["loss_cls"])
    assert abs(y["loss_bbox"] - float(g["loss_%s_bbox" % case])) <= 1e-12 * max(1.0, y["loss_bbox"])
    keep = lambda a: a.ravel()[rr.sample_rows(case, a.size)]
    for mine, want in ((keep(y["grad_cls"][0]), g["loss_%s_grad_cls" % case]), (keep(y["grad_box"][0]), g["loss_%s_grad_box" % case])):
        assert np.array_equal(mine == 0, want == 0) and np.allclose(mine, want, rtol=1e-12, atol=0)
    b = rr.loss_bounds(y)
    # the float32 CPU reference stays within a quarter of every bound: the 32 eps arm governs, not 4 e_ref
    assert float(g["loss_%s_e_ref_cls" % case]) <= b["loss_cls"] / 4 and float(g["loss_%s_e_ref_box" % case]) <= b["loss_bbox"] / 4
    assert np.all(g["loss_%s_e_grad" % case] <= 0.25)


# ---- every condition the cases name occurs -------------------------------------------------------------------------------------------
def test_cases_are_the_engineered_ones(g, mb):
    assert float(g["e_ref"]) > 0
    assert [rr.count_anchors(rr.make_case(c)["spec"]) for c in rr.SIZE_CASES] == [63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
    assert rr.BLOCK == 256 and rr.SELECT_BLOCK == 1024                                         # block size - 1, the block size, + 1
    for c in rr.SIZE_CASES:
        assert mb[c]["n_fg"] >= 1 and mb[c]["n_bg"] >= 1, c
    # the five-level layout: both selections cut, and levels start off alignment
    spec, m = rr.make_case("fpn5")["spec"], mb["fpn5"]
    assert rr.count_anchors(spec) == 12276 and [(H, W) for _, H, W, _, _ in spec] == [(48, 64), (24, 32), (12, 16), (6, 8), (3, 4)]
    assert int(m["fg"].sum()) > 16 == m["n_fg"] and int(m["bg"].sum()) > 16 == m["n_bg"]
    assert any(o % 4 for o in rr.offsets(spec)[1:-1]) or any(o % 64 for o in rr.offsets(spec)[1:-1])
    # the defaults at real density
    assert rr.count_anchors(rr.make_case("c4")["spec"]) == 28500 and len(rr.make_case("c4")["gt_boxes"]) == 20
    assert 0 < mb["c4"]["n_fg"] < 128 and mb["c4"]["n_fg"] + mb["c4"]["n_bg"] == 256           # fewer fg than the quota: bg fills up
    assert rr.count_anchors(rr.make_case("fpn")["spec"]) == 121515 and len(rr.make_case("fpn")["gt_boxes"]) == 30
    assert int(mb["fpn"]["fg"].sum()) > 128 == mb["fpn"]["n_fg"] and int(mb["fpn"]["bg"].sum()) > 100000 and mb["fpn"]["n_bg"] == 128
    assert rr.make_case("c4")["is_crowd"].sum() == 2 and (mb["c4"]["gt_max"][:2] == 0).all()     # crowd rows take no part
    # anchors below positive_overlap that are fg because they are their gt's best (the large box of the seeded cases), some of them
    # below negative_overlap
    assert np.any(mb["c4"]["fg"] & (mb["c4"]["max_overlaps"] < 0.7)) and np.any(mb["fpn"]["fg"] & (mb["fpn"]["max_overlaps"] < 0.7))
    assert np.any(mb["n1024"]["fg"] & (mb["n1024"]["max_overlaps"] < 0.3))


@pytest.fixture(scope="module")
def profiles():
    """rr.selection_profile and the restatement of every image of every case of rr.TARGET_CASES"""
    out = {}
    for name in rr.TARGET_CASES:
        cases, params = rr.target_case(name)
        p = dict(rr.DEFAULTS, **params)
        ms = [rr.minibatch(c, p) for c in cases]
        out[name] = [(rr.selection_profile(c, p, m), m) for c, m in zip(cases, ms)]
    return out


def sort_branch(n):
    """the branch of block_bitonic_sort<1024> (csrc/block_sort.h) that sorts n taken fg keys"""
    np2 = 2
    while np2 < n:
        np2 *= 2
    per = (np2 + rr.SELECT_BLOCK - 1) // rr.SELECT_BLOCK
    return ("merge", np2) if per <= 1 and np2 >= 256 else ("network, %d per thread" % per, np2)


def test_large_and_clustered_cases_are_the_engineered_ones(profiles, mb):
    from detectorch_amd import hip_rpn
    src = lambda *parts: open(os.path.join(ROOT, "detectorch_amd", "csrc", *parts)).read()
    text = src("rpn_train", "rpn_train_common.h") + src("rpn_train", "rpn_targets.hip") + src("rpn_train", "rpn_loss.hip")
    const = lambda name, t=text: int(re.search(r"constexpr int %s = (\d+);" % name, t).group(1))
    # the points the cases are placed round, from the source text
    assert const("kRpnSelThreads") == rr.SELECT_BLOCK == 1024 and const("kRpnThreads") == rr.BLOCK == 256
    assert re.search(r"for \(int e = tid; e < n_c; e \+= kRpnSelThreads\)", text)                # rpn_threshold strides by its workgroup
    assert const("kRpnGroupPer") * const("kRpnThreads") == 2048 and re.search(r"constexpr int kRpnGroupPerFrom = 1 << 16;", text)
    assert const("kRpnLossMaxBlocks") * const("kLossThreads", src("loss", "loss_common.h")) == rr.LOSS_DENSE_ROUND == 131072
    assert hip_rpn.LOSS_BLOCK == 256 and hip_rpn.MAX_ANCHORS == 1 << 20 and hip_rpn.MAX_BATCH_PER_IM == 4096
    header = open(os.path.join(ROOT, "include", "detectorch_rpn_hip.h")).read()
    assert re.search(r"#define DTC_RPN_TRAIN_MAX_ANCHORS \(?1 << 20\)?", header) and re.search(r"#define DTC_RPN_TRAIN_MAX_BATCH_PER_IM 4096", header)
    assert re.search(r"if \(per <= 1 && n_pow2 >= 256\) block_merge_sort_e1<THREADS>", src("block_sort.h"))
    assert re.search(r"block_bitonic_sort<kRpnSelThreads>\(keys, np2\)", text)
    assert const("kRpnIdxBits") == 20 and const("kRpnDigitBits") == 11 and rr.KEY_FIELDS == ((44, 52), (33, 44), (22, 33), (11, 22), (0, 11))
    # what the earlier cases reach: a threshold bin of some hundred candidates, at most 128 fg to sort, anchor indices below 2^17
    old = {c: rr.selection_profile(rr.make_case(c), rr.params_of(c), mb[c]) for c in ("fpn5", "c4", "fpn")}
    assert max(p[s]["bin_population"] for p in old.values() for s in ("fg", "bg")) < 1024
    assert max(p["fg"]["taken"] for p in old.values()) == 128 and sort_branch(128) == ("network, 1 per thread", 128)
    assert max(p[s]["max_index"] for p in old.values() for s in ("fg", "bg")) < 1 << 17

    one = lambda name: profiles[name][0][0]
    # (h) clustered keys: the whole bg group in the threshold bin, more than one round of rpn_threshold's workgroup
    for k in ("arange", "constant", "reversed", "three"):
        p = one("cluster_" + k)
        assert rr.count_anchors(rr.target_case("cluster_" + k)[0][0]["spec"]) == 2560
        assert p["bg"]["cuts"] and p["bg"]["candidates"] > 2300 and p["bg"]["taken"] == 64 - p["fg"]["taken"] > 32
        assert p["bg"]["bin_population"] == p["bg"]["candidates"] > 2 * 1024, k
    assert one("cluster_constant")["bg"]["equal_rand_key"] and one("cluster_three")["bg"]["equal_rand_key"]
    keys = rr.target_case("cluster_own_bin")[0][0]["rand_keys"]
    assert len(set((keys >> 24).tolist())) == 256 and not (keys & 0xFFFFFF).any() and one("cluster_own_bin")["bg"]["bin_population"] <= 10
    assert one("c4_arange")["bg"]["bin_population"] == one("c4_arange")["bg"]["candidates"] > 3 * 4096
    # every field of the key decides once; in one case two anchors with one rand_key straddle the boundary
    for name, field in rr.DIGIT_FIELDS.items():
        assert one(name)["bg"]["cuts"] and one(name)["bg"]["field"] == field, name
    assert sorted(rr.DIGIT_FIELDS.values()) == sorted(rr.KEY_FIELDS)
    assert one("digit_index")["bg"]["equal_rand_key"] and not any(one(n)["bg"]["equal_rand_key"] for n in rr.DIGIT_FIELDS if n != "digit_index")
    assert all(one(n)["bg"]["bin_population"] > 2 * 1024 for n in rr.DIGIT_FIELDS if n != "digit_bin")
    b3 = rr.target_case("cluster_b3")[0]
    assert len(b3) == 3 and all(p["bg"]["bin_population"] > 2 * 1024 for p, _ in profiles["cluster_b3"])
    assert len({c["rand_keys"].tobytes() for c in b3}) == 3 and len({c["gt_boxes"].tobytes() for c in b3}) == 3
    # (i) every anchor fg: the quota is what is sorted -- the merge sort at 256, 512 and 1024 keys, two and four keys per thread,
    # counts that are no power of two just above each edge, fgkeys full
    taken = {n: one(n)["fg"]["taken"] for n in rr.QUOTA_PARAMS}
    assert taken == dict(quota_300=300, quota_600=600, quota_2048=2048, quota_4096=4096, quota_2050=2050, quota_1025=1025, quota_129=129,
                         quota_bg=taken["quota_bg"], quota_no_gt=4096, quota_arange=300)
    assert one("quota_arange")["fg"]["bin_population"] == 4608 > 4 * 1024                     # the fg half of the candidate list, strided
    assert [sort_branch(taken[n]) for n in ("quota_129", "quota_300", "quota_600", "quota_1025", "quota_2048", "quota_2050", "quota_4096")] == \
        [("merge", 256), ("merge", 512), ("merge", 1024), ("network, 2 per thread", 2048), ("network, 2 per thread", 2048),
         ("network, 4 per thread", 4096), ("network, 4 per thread", 4096)]
    for n in rr.QUOTA_PARAMS:
        (p, m), (case, prm) = profiles[n][0], (rr.target_case(n)[0][0], rr.target_case(n)[1])
        assert rr.count_anchors(case["spec"]) == 4608 and prm["straddle_thresh"] == -1.0 and m["inside"].all()
        if n != "quota_bg":
            assert p["fg"]["candidates"] == 4608 and p["fg"]["cuts"] and p["bg"]["candidates"] == 0
            assert np.any(m["max_overlaps"][m["fg_index"][:m["n_fg"]]] == 0)                   # fg whose best IoU is 0
            assert np.all(m["fg_gt"][:m["n_fg"]] >= 0) == (n != "quota_no_gt")
    assert rr.target_case("quota_no_gt")[0][0]["count"] == 0 and np.all(profiles["quota_no_gt"][0][1]["fg_gt"] == -1)
    p = one("quota_bg")                                                                       # fewer fg than F: the bg quota is R - n_fg
    assert p["fg"]["taken"] == p["fg"]["candidates"] < 4096 and p["bg"]["taken"] == 4096 - p["fg"]["taken"] > 3000 and p["bg"]["cuts"]
    # (j) round the switch of rpn_group to 2048 anchors per workgroup: the last workgroup is partial below and above it
    for n, shape in rr.SWITCH_SHAPES.items():
        cases = rr.target_case("switch_%d" % n)[0]
        assert rr.count_anchors(cases[0]["spec"]) == n == shape[0] * shape[1] * shape[2] and len(cases) == 2
        assert not np.array_equal(cases[0]["gt_boxes"], cases[1]["gt_boxes"]) and not np.array_equal(cases[0]["rand_keys"], cases[1]["rand_keys"])
        for p, m in profiles["switch_%d" % n]:
            assert p["fg"]["taken"] >= 1 and p["bg"]["cuts"] and p["fg"]["taken"] + p["bg"]["taken"] == 64
    assert sorted(rr.SWITCH_SHAPES) == [(1 << 16) - 1, 1 << 16, (1 << 16) + 1] and 65537 % 2048 == 1
    (p, m), case = profiles["full_2p20"][0], rr.target_case("full_2p20")[0][0]
    assert rr.count_anchors(case["spec"]) == 1 << 20 == hip_rpn.MAX_ANCHORS and case["spec"][0][0] == hip_rpn.MAX_ANCHORS_PER_CELL
    assert p["fg"]["max_index"] >= 1 << 19 and np.where(m["labels"] == 0)[0].min() >= 1 << 19   # index bits 17 - 19 in taken anchors
    assert p["bg"]["cuts"] and p["bg"]["equal_rand_key"] and p["bg"]["bin_population"] == p["bg"]["candidates"] > 10 ** 6
    assert m["fg_index"][:m["n_fg"]].min() < 1 << 19 and p["fg"]["taken"] + p["bg"]["taken"] == 256
    cases = rr.target_case("batch_300")[0]
    assert len(cases) == 300 > rr.BLOCK and sorted({c["count"] for c in cases}) == [0, 1, 2, 3]
    assert len({c["rand_keys"].tobytes() for c in cases}) == 300 and len({m["labels"].tobytes() for _, m in profiles["batch_300"]}) > 150
    # the losses: the dense pass starts over above 512 x 256 anchors, the rows above 256, the count above 256 images
    n_of = lambda name: rr.count_anchors(rr.big_loss_case(name)["spec"])
    assert [n_of("n%d" % n) for n in (131071, 131072, 131073)] == [131071, 131072, 131073]
    c = rr.big_loss_case("two_level")
    off = rr.offsets(c["spec"])
    assert len(c["spec"]) == 2 and off[1] > rr.LOSS_DENSE_ROUND
    for name in rr.LOSS_BIG_CASES:                                                            # no anchor has two counted rows
        c = rr.big_loss_case(name)
        B, F = c["fg_index"].shape
        for b in range(B):
            rows = c["fg_index"][b, :min(max(int(c["n_fg"][b]), 0), F)]
            rows = rows[(rows >= 0) & (rows < n_of(name))]
            assert len(set(rows.tolist())) == len(rows), name
            if name == "two_level":
                assert (rows >= off[1]).sum() == 4 and (rows < off[1]).sum() >= 5 and np.all(c["labels"][b, rows] == 1)
    c = rr.big_loss_case("rows_4096")
    assert c["fg_index"].shape == (2, hip_rpn.MAX_BATCH_PER_IM) and c["n_fg"].tolist() == [4096, 2500] and n_of("rows_4096") == 4608
    assert c["fg_index"][1, [5, 1000, 2499]].tolist() == [-1, 4608, 2 ** 30] and np.all(c["fg_index"][0] >= 0)
    past = c["fg_index"][1, 2500:]
    assert ((past >= 0) & (past < 4608)).sum() > 1500 and c["fg_targets"][1, 2500:].all() and not (c["labels"][1][past[:-3]] == 1).any()
    c = rr.big_loss_case("rows_300")
    assert c["fg_index"].shape == (3, 300) and 900 % 256 and c["n_fg"].tolist() == [300, 17, 300]   # the last counted row is row 899
    for B in (257, 600):
        c = rr.big_loss_case("batch_%d" % B)
        assert c["fg_index"].shape == (B, 2) and B > hip_rpn.LOSS_BLOCK and n_of("batch_%d" % B) == 4
        assert c["n_fg"].min() < 0 and c["n_fg"].max() > 2 and c["n_bg"].min() < 0 and c["n_bg"].max() > 0
        assert (c["n_fg"][256:] > 0).any() and (c["n_bg"][256:] > 0).any()                     # counts that matter past the first round


def test_hand_made_case_conditions(mb):
    m = mb["hand"]
    ov = rr.bbox_overlaps(rr.HAND_ANCHORS, rr.HAND_GT)
    assert ov[0, 0] == np.float32(0.5) and ov[1, 0] < np.float32(0.5) < ov[2, 0] and ov[2, 0] - ov[1, 0] < 2e-4
    assert ov[3, 1] == np.float32(0.25) and ov[5, 1] < np.float32(0.25) < ov[6, 1]
    assert m["fg"][0] and not m["fg"][1] and not m["bg"][1] and m["fg"][2]                     # 1/2: fg; below: ignored
    assert not m["fg"][3] and not m["bg"][3] and m["bg"][5] and not m["bg"][6] and not m["fg"][6]   # 1/4: not bg; below: bg
    assert ov[7, 2] == ov[8, 2] == m["gt_max"][2] < np.float32(0.5) and m["fg"][7] and m["fg"][8]   # two anchors tie: both fg
    assert m["arg"][9] == 3 and m["max_overlaps"][9] == 1                                      # identical gt: the first
    assert 0 < m["gt_max"][5] < np.float32(0.25) and m["fg"][10] and not m["bg"][10]           # a low-quality best anchor is fg, not bg
    assert m["gt_max"][6] == 0 and m["bg"][11:].all() and not m["fg"][11:].any()               # an untouched gt marks nothing
    assert int(m["fg"].sum()) == 7 > 4 and int(m["bg"].sum()) == 6 > 4                         # both selections cut
    eq = rr.minibatch(rr.hand_case("equal"), rr.params_of("hand"))
    assert eq["fg_index"].tolist() == [0, 2, 4, 7] and np.where(eq["labels"] == 0)[0].tolist() == [5, 11, 12, 13]   # index order
    ex = rr.minibatch(rr.hand_case("extremes"), rr.params_of("hand"))
    assert set(rr.hand_case("extremes")["rand_keys"].tolist()) == {0, 2 ** 32 - 1}
    assert ex["fg_index"].tolist() == [0, 2, 4, 8]                                             # key 0 first: the even anchors


def test_straddle_case_conditions():
    assert rr.STRADDLE_ANCHORS[1, 0] == 0 and np.signbit(rr.STRADDLE_ANCHORS[1, 0]) and rr.STRADDLE_ANCHORS[2, 0] < 0
    assert rr.STRADDLE_ANCHORS[3, 2] == 200 - 1 and rr.STRADDLE_ANCHORS[4, 2] == 200
    for st, want in rr.STRADDLE_INSIDE.items():
        c, p = rr.straddle_case(st)
        m = rr.minibatch(c, p)
        assert m["inside"].astype(int).tolist() == want, st
        assert np.all(m["labels"][~m["inside"]] == -1) and not m["max_overlaps"][~m["inside"]].any()


def test_expanded_blobs_of_the_restatement(mb):
    spec, m = rr.make_case("fpn5")["spec"], mb["fpn5"]
    bt, bi, bo = rr.expanded(spec, m["labels"], m["fg_index"], m["fg_targets"], m["n_fg"], m["n_bg"])
    assert int(bi.sum()) == 4 * m["n_fg"] and int((bo > 0).sum()) == 4 * (m["n_fg"] + m["n_bg"])
    assert np.all(bo[bo > 0] == np.float32(1) / np.float32(32)) and np.array_equal(bt != 0, (bi > 0) & (bt != 0))


# ---- the library: exports, binding, constants ------------------------------------------------------------------------------------------
def test_header_symbols_are_exported_and_bound():
    from make_native_host_codes import exports
    from test_binding_signatures_host import _struct_of, prototypes
    from detectorch_amd import hip_rpn
    L = hip_rpn.lib()
    protos = prototypes("detectorch_rpn_hip.h")
    names = ["dtc_rpn_loss", "dtc_rpn_loss_workspace_bytes", "dtc_rpn_targets", "dtc_rpn_targets_workspace_bytes",
             "dtc_rpn_train_target_arch"]
    assert sorted(protos) == names and exports(hip_rpn.LIB_PATH) == names and sorted(hip_rpn.SIGNATURES) == names
    for entry, (ret, params) in protos.items():
        row = hip_rpn.SIGNATURES[entry]
        assert row[0] == ret and [n for n, _ in row[1]] == [n for n, _ in params], entry
        for (name, got), (_, want) in zip(row[1], params):
            assert (got if isinstance(got, str) else _struct_of(got)) == want, (entry, name)
        assert getattr(L, entry).argtypes is not None or ret == "str"
    assert L.dtc_rpn_train_target_arch() == b"gfx950"
    assert C.sizeof(hip_rpn.RpnTrainLevel) == 304 and C.sizeof(hip_rpn.RpnTrainParams) == 32


def test_the_other_five_libraries_exports_unchanged():
    from make_native_host_codes import exports
    from test_binding_signatures_host import prototypes
    from detectorch_amd import build, hip, hip_grad, hip_loss, hip_optim, hip_train
    build.build()
    with open(os.path.join(GOLDEN, "native_host_codes.json")) as f:
        want = json.load(f)["exports"]
    assert exports(hip.LIB_PATH) == want and len(want) == 42
    for mod, header, count in ((hip_train, "detectorch_train_hip.h", 2), (hip_loss, "detectorch_loss_hip.h", 5),
                               (hip_grad, "detectorch_grad_hip.h", None), (hip_optim, "detectorch_optim_hip.h", None)):
        mod.lib()
        got = exports(mod.LIB_PATH)
        assert got == sorted(prototypes(header)) == sorted(mod.SIGNATURES), header
        assert count is None or len(got) == count
        assert not [n for n in got if "rpn" in n and "train" in n], header


def test_constants_are_those_of_the_source():
    from detectorch_amd import hip_rpn
    text = "".join(open(os.path.join(ROOT, "detectorch_amd", "csrc", "rpn_train", f)).read()
                   for f in ("rpn_train_common.h", "rpn_targets.hip", "rpn_loss.hip"))
    loss_common = open(os.path.join(ROOT, "detectorch_amd", "csrc", "loss", "loss_common.h")).read()
    const = lambda name, src=text: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert const("kRpnThreads") == hip_rpn.BLOCK == rr.BLOCK
    assert const("kRpnSelThreads") == hip_rpn.SELECT_BLOCK == rr.SELECT_BLOCK and const("kRpnDigitBins") == 1 << const("kRpnDigitBits")
    assert const("kLossThreads", loss_common) == hip_rpn.LOSS_BLOCK and const("kRpnLossMaxBlocks") == hip_rpn.LOSS_MAX_BLOCKS
    assert const("kRpnGroupPer") * rr.BLOCK == 2048 and rr.count_anchors(rr.make_case("fpn")["spec"]) >= 1 << 16 > 28500   # both forms of rpn_group run
    assert re.search(r"constexpr int kRpnGroupPerFrom = 1 << 16;", text)
    assert const("kRpnKeyBins") == 256 and 8 + 4 * const("kRpnDigitBits") == 32 + const("kRpnIdxBits") == 52 and 1 << 20 == hip_rpn.MAX_ANCHORS
    header = open(os.path.join(ROOT, "include", "detectorch_rpn_hip.h")).read()
    define = lambda name: re.search(r"#define %s \(?([\d <]+)\)?" % name, header).group(1).strip()
    assert int(define("DTC_RPN_TRAIN_MAX_LEVELS")) == hip_rpn.MAX_LEVELS and int(define("DTC_RPN_TRAIN_MAX_GT")) == hip_rpn.MAX_GT
    assert int(define("DTC_RPN_TRAIN_MAX_ANCHORS_PER_CELL")) == hip_rpn.MAX_ANCHORS_PER_CELL
    assert define("DTC_RPN_TRAIN_MAX_ANCHORS") == "1 << 20" and int(define("DTC_RPN_TRAIN_MAX_BATCH_PER_IM")) == hip_rpn.MAX_BATCH_PER_IM


def test_wrappers_raise_on_cpu_tensors():
    import torch
    from detectorch_amd import hip_rpn
    from detectorch_amd.model.loss import rpn_losses
    from detectorch_amd.utils.rpn_targets import rpn_levels, rpn_targets_batched
    spec = rr.single(1, 2, 2)
    levels = rpn_levels([s[:3] for s in spec], [s[4] for s in spec], [s[3] for s in spec])
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
    with pytest.raises(RuntimeError, match="GPU only"):
        rpn_targets_batched(levels, z(1, 2, 4), z(1, 2, dt=torch.int32), z(1, dt=torch.int32), z(1), z(1, 2),
                            rand_keys=z(1, 4, dt=torch.int32))
    blobs = dict(labels=z(1, 4, dt=torch.int32), fg_index=z(1, 2, dt=torch.int32), fg_targets=z(1, 2, 4), n_fg=z(1, dt=torch.int32),
                 n_bg=z(1, dt=torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        rpn_losses([z(1, 1, 2, 2)], [z(1, 4, 2, 2)], blobs)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip_rpn.rpn_loss(levels, blobs["labels"], blobs["fg_index"], blobs["fg_targets"], blobs["n_fg"], blobs["n_bg"])


# ---- workspace sizes -----------------------------------------------------------------------------------------------------------------
def _levels(hip_rpn, shapes, ptr=None):
    arr = (hip_rpn.RpnTrainLevel * len(shapes))()                              # (not make_levels: it refuses what these tests pass)
    for lv, (a, h, w) in zip(arr, shapes):
        lv.num_anchors, lv.height, lv.width, lv.feat_stride = a, h, w, 16.0
        lv.cls_logits = lv.bbox_pred = lv.grad_cls_logits = lv.grad_bbox_pred = ptr
        for q in range(64):
            lv.anchors[q] = 15.0 if q % 4 >= 2 else 0.0
    return arr


def _up(v, a=256):
    return (v + a - 1) // a * a


def targets_ws_bytes(B, G, N):
    """the carve of RpnTargetsWs: per-gt maxima, two 256-bin histograms and four counters per image (the zeroed part); the selection
    records; overlap and argmax per anchor; the candidate keys; the taken fg keys -- every block rounded up to 256 bytes"""
    return sum(_up(v) for v in (B * G * 4, B * 2 * 256 * 4, B * 16, B * 32, B * 16, B * N * 4, B * N * 4, B * N * 8, B * 4096 * 8))


def loss_ws_bytes(B, N):
    return 16 + B * min((N + 255) // 256, 512) * 8


def test_workspace_sizes():
    from detectorch_amd import hip_rpn
    L = hip_rpn.lib()
    tw = lambda shapes, B, G: L.dtc_rpn_targets_workspace_bytes(_levels(hip_rpn, shapes), len(shapes), B, G)
    lw = lambda shapes, B: L.dtc_rpn_loss_workspace_bytes(_levels(hip_rpn, shapes), len(shapes), B)
    for shapes, B, G in (([(1, 1, 1)], 1, 0), ([(3, 3, 7)], 2, 5), ([(15, 38, 50)], 8, 20), ([(3, 152, 200), (3, 76, 100)], 3, 256),
                         ([(16, 256, 256)], 1, 256)):
        N = sum(a * h * w for a, h, w in shapes)
        assert tw(shapes, B, G) == targets_ws_bytes(B, G, N) and lw(shapes, B) == loss_ws_bytes(B, N), (shapes, B, G)
    # monotone in each argument
    base = tw([(3, 10, 10)], 2, 8)
    assert tw([(3, 10, 11)], 2, 8) >= base and tw([(4, 10, 10)], 2, 8) >= base and tw([(3, 10, 10)], 3, 8) > base
    assert tw([(3, 10, 10)], 2, 200) > base and tw([(3, 10, 10), (3, 5, 5)], 2, 8) > base
    assert lw([(3, 10, 10)], 3) > lw([(3, 10, 10)], 2) and lw([(3, 100, 100)], 2) > lw([(3, 10, 10)], 2)
    assert lw([(16, 256, 256)], 2) == lw([(16, 200, 200)], 2)                                 # the dense pass has at most 512 workgroups
    # unsupported or malformed: 0
    assert tw([(17, 1, 1)], 1, 1) == 0 and tw([(16, 256, 257)], 1, 1) == 0 and tw([(1, 1, 1)], 1, 257) == 0 and tw([(1, 1, 1)], 0, 1) == 0
    assert tw([(1, 1, 1)] * 9, 1, 1) == 0 and tw([(1, 0, 1)], 1, 1) == 0 and lw([(1, 1, 1)], 0) == 0 and lw([(17, 1, 1)], 1) == 0


# ---- return codes ----------------------------------------------------------------------------------------------------------------------
BOGUS = 256                                                                  # a bogus, non-NULL, 16-byte aligned device pointer
T_ARGS = ("gt_boxes", "gt_is_crowd", "gt_counts", "im_scale", "im_hw", "rand_keys")
T_OUTS = ("labels", "fg_index", "fg_targets", "fg_gt", "n_fg", "n_bg", "max_overlaps", "gt_max", "bbox_targets", "bbox_inside_weights",
          "bbox_outside_weights")
L_ARGS = ("labels", "fg_index", "fg_targets", "n_fg", "n_bg", "upstream")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4

# label -> (keyword overrides of _targets, expected code)
T_CODES = {
    "ok": (dict(), 0), "batch -1": (dict(batch=-1), EINVAL), "G -1": (dict(G=-1), EINVAL), "params NULL": (dict(params=None), EINVAL),
    "levels NULL": (dict(levels=None), EINVAL), "n_levels 0": (dict(n_levels=0), EINVAL), "H 0": (dict(shapes=[(3, 0, 7)]), EINVAL),
    "stride 0": (dict(stride=0.0), EINVAL), "stride nan": (dict(stride=float("nan")), EINVAL),
    "batch_size_per_im 0": (dict(batch_size_per_im=0), EINVAL), "fg_fraction 1.5": (dict(fg_fraction=1.5), EINVAL),
    "positive nan": (dict(positive_overlap=float("nan")), EINVAL), "negative above positive": (dict(negative_overlap=0.8), EINVAL),
    "straddle inf": (dict(straddle_thresh=float("inf")), EINVAL),
    # shapes before limits
    "G 257 + H 0": (dict(G=257, shapes=[(3, 0, 7)]), EINVAL), "A 17 + fg_fraction 1.5": (dict(shapes=[(17, 1, 1)], fg_fraction=1.5), EINVAL),
    # limits before batch 0 and pointers
    "G 257": (dict(G=257), EUNSUPPORTED), "A 17": (dict(shapes=[(17, 1, 1)]), EUNSUPPORTED), "9 levels": (dict(shapes=[(1, 1, 1)] * 9), EUNSUPPORTED),
    "N 2^20 + 256": (dict(shapes=[(16, 256, 256), (1, 16, 16)]), EUNSUPPORTED), "N 2^20": (dict(shapes=[(16, 256, 256)], ws_bytes=0), EWORKSPACE),
    "batch_size_per_im 4097": (dict(batch_size_per_im=4097), EUNSUPPORTED), "G 257 + labels NULL": (dict(G=257, labels=None), EUNSUPPORTED),
    "batch 0 + every pointer NULL": (dict(batch=0, workspace=None, **{k: None for k in T_ARGS + T_OUTS}), 0),
    # pointers
    **{k + " NULL": ({k: None}, EINVAL) for k in T_ARGS + ("labels", "fg_index", "fg_targets", "fg_gt", "n_fg", "n_bg")},
    "G 0 + gt pointers NULL": (dict(G=0, gt_boxes=None, gt_is_crowd=None, gt_counts=None), 0),
    "F 0 + fg pointers NULL": (dict(fg_fraction=0.0, fg_index=None, fg_targets=None, fg_gt=None), 0),
    "bbox_targets alone NULL": (dict(bbox_targets=None), EINVAL), "expanded all NULL": (dict(bbox_targets=None, bbox_inside_weights=None,
                                                                                            bbox_outside_weights=None), 0),
    "max_overlaps NULL": (dict(max_overlaps=None), 0), "gt_max NULL": (dict(gt_max=None), 0),
    "gt_boxes misaligned": (dict(gt_boxes=BOGUS + 4), EINVAL), "fg_targets misaligned": (dict(fg_targets=BOGUS + 8), EINVAL),
    "workspace misaligned": (dict(workspace=BOGUS + 4), EINVAL),
    # pointers before workspace
    "workspace NULL": (dict(workspace=None), EWORKSPACE), "workspace one byte short": (dict(ws_short=1), EWORKSPACE),
    "workspace short + labels NULL": (dict(ws_short=1, labels=None), EINVAL),
}
L_CODES = {
    "batch 0": (dict(batch=0), EINVAL), "F -1": (dict(F=-1), EINVAL), "beta 0": (dict(beta=0.0), EINVAL), "beta nan": (dict(beta=float("nan")), EINVAL),
    "levels NULL": (dict(levels=None), EINVAL), "W 0": (dict(shapes=[(3, 3, 0)]), EINVAL),
    "A 17": (dict(shapes=[(17, 1, 1)]), EUNSUPPORTED), "F 4097": (dict(F=4097), EUNSUPPORTED), "A 17 + beta 0": (dict(shapes=[(17, 1, 1)], beta=0.0), EINVAL),
    "F 4097 + labels NULL": (dict(F=4097, labels=None), EUNSUPPORTED),
    **{k + " NULL": ({k: None}, EINVAL) for k in ("labels", "fg_index", "fg_targets", "n_fg", "n_bg", "losses", "n_valid")},
    "cls_logits NULL": (dict(null_maps=("cls_logits",)), EINVAL), "bbox_pred NULL": (dict(null_maps=("bbox_pred",)), EINVAL),
    "a gradient map missing in one level": (dict(shapes=[(3, 3, 7), (3, 2, 4)], null_maps=("grad_bbox_pred",), null_level=1), EINVAL),
    "workspace misaligned": (dict(workspace=BOGUS + 8), EINVAL),
    "workspace NULL": (dict(workspace=None), EWORKSPACE), "workspace one byte short": (dict(ws_short=1), EWORKSPACE),
    "workspace short + losses NULL": (dict(ws_short=1, losses=None), EINVAL),
}


def _targets(hip_rpn, batch=2, G=16, shapes=((3, 3, 7),), stride=16.0, params=True, ws_short=0, ws_bytes=None, **kw):
    shapes = list(shapes)
    levels = _levels(hip_rpn, shapes)
    for lv in levels:
        lv.feat_stride = stride
    n_levels = kw.pop("n_levels", len(shapes))
    levels = kw.pop("levels", levels)
    ptr = {k: kw.pop(k, BOGUS) for k in T_ARGS + T_OUTS + ("workspace",)}
    prm = hip_rpn.rpn_train_params(**kw) if params else None
    N = sum(a * h * w for a, h, w in shapes)
    need = targets_ws_bytes(max(batch, 0), max(G, 0), N) - ws_short if ws_bytes is None else ws_bytes
    v = lambda k: None if ptr[k] is None else C.c_void_p(ptr[k])
    return hip_rpn.lib().dtc_rpn_targets(levels, n_levels, batch, v("gt_boxes"), v("gt_is_crowd"), v("gt_counts"), G, v("im_scale"),
                                         v("im_hw"), v("rand_keys"), C.byref(prm) if prm is not None else None, v("workspace"), need,
                                         *[v(k) for k in T_OUTS], None)


def _loss(hip_rpn, batch=2, F=16, shapes=((3, 3, 7),), beta=1.0 / 9.0, ws_short=0, null_maps=(), null_level=0, **kw):
    shapes = list(shapes)
    levels = _levels(hip_rpn, shapes, BOGUS)
    for name in null_maps:
        setattr(levels[null_level], name, None)
    levels = kw.pop("levels", levels)
    ptr = {k: kw.pop(k, BOGUS) for k in L_ARGS + ("workspace", "losses", "n_valid")}
    assert not kw
    N = sum(a * h * w for a, h, w in shapes)
    v = lambda k: None if ptr[k] is None else C.c_void_p(ptr[k])
    return hip_rpn.lib().dtc_rpn_loss(levels, len(shapes), batch, v("labels"), v("fg_index"), v("fg_targets"), v("n_fg"), v("n_bg"), F,
                                      beta, v("upstream"), v("workspace"), loss_ws_bytes(max(batch, 0), N) - ws_short, v("losses"),
                                      v("n_valid"), None)


def test_return_codes_on_bad_arguments():
    """Only the rows that return an error, or return before the first launch, can be taken without a device: the rows whose expected
    code is DTC_OK with batch > 0 would launch; the NULL groups and F = 0 among them run on the GPU (tests/test_hip_rpn_targets.py)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--codes"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = json.loads(out.stdout.decode())
    assert got == {"targets": {k: v[1] for k, v in T_CODES.items() if _hostable(v)}, "loss": {k: v[1] for k, v in L_CODES.items()}}
    assert len(got["targets"]) >= 40 and len(got["loss"]) >= 20


def _hostable(row):
    return row[1] != 0 or row[0].get("batch") == 0


if __name__ == "__main__" and "--codes" in sys.argv:
    from detectorch_amd import hip_rpn as hr
    print(json.dumps({"targets": {k: _targets(hr, **kw) for k, (kw, code) in T_CODES.items() if _hostable((kw, code))},
                      "loss": {k: _loss(hr, **kw) for k, (kw, _) in L_CODES.items()}}))
