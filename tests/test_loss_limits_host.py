"""The cases of tests/loss_limit_cases.py without a GPU:
  * the float64 restatement (tests/loss_ref.py) against the reference's own functions on every recorded case
    (tests/golden/loss_limits.npz, made by tests/golden/make_loss_limits_golden.py) to a few float64 roundings, the seeded inputs by
    SHA-256;
  * what keeps tests/test_hip_loss_limits.py from passing emptily, asserted on the restatement and on the restated launch arithmetic
    alone: every case reaches the lane width, register slot, trip count, left-over or magnitude that its row in the table of
    tests/README_loss.md names."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
import loss_limit_cases as ll
import loss_ref as lr


@pytest.fixture(scope="module")
def g():
    return dict(golden("loss_limits"))


def _valid(c):
    return c["labels"] >= 0


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_the_table_is_recorded(g):
    assert set(ll.RECORDED) | set(ll.UNRECORDED) == set(ll.HEAD) and not set(ll.RECORDED) & set(ll.UNRECORDED)
    assert ll.UNRECORDED == ("tc324", "tc8", "mlogits", "b149", "b126", "b100", "b3e38")
    names = list(ll.RECORDED) + [ll.flat_name(s) for s in ll.FLAT]
    assert sorted(k[:-4] for k in g if k.endswith("_sha")) == sorted(names)
    size = lambda n: os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz"))
    assert 2 * size("loss_limits") < size("loss")


@pytest.mark.parametrize("name", ll.RECORDED)
def test_restatement_equals_reference(g, name):
    c, y = ll.case(name), ll.want(name)
    assert lr.same_bits(ll.head_digest(name), g[name + "_sha"])
    loss_cls, loss_bbox, acc, nv, e_cls, e_box = g[name + "_scalars"]
    assert y["n_valid"] == int(nv) and round(float(y["accuracy"]) * nv) == round(acc * nv)
    top = float(np.nanmax(np.abs(c["cls_score"])))
    assert abs(float(y["loss_cls"]) - loss_cls) <= 1e-12 * max(top, loss_cls)
    assert abs(float(y["loss_bbox"]) - loss_bbox) <= 1e-12 * loss_bbox
    if nv > 1:
        assert e_cls > 1e-12 * max(top, loss_cls)                            # e_ref is far above float64 rounding
    rows = ll.sample_rows(name)
    rows = np.arange(len(c["labels"])) if rows is None else rows
    assert (len(rows) < len(c["labels"])) == (len(c["labels"]) > 70 or c["cls_score"].shape[1] > 17)
    assert np.abs(y["grad_cls"][rows] - g[name + "_grad_cls"]).max() <= 1e-13 / nv
    assert not y["grad_cls"][~_valid(c)].any()
    if c["bbox_pred"] is not None:
        sel = np.take_along_axis(y["grad_box"], ll.selected(c)[:, None] + np.arange(4)[None, :], 1) * (ll.selected(c)[:, None] > 0)
        wanted = g[name + "_grad_box4"]
        assert np.abs(sel[rows] - wanted).max() <= 1e-13 * max(np.abs(wanted).max(), 1e-300)
        assert np.count_nonzero(y["grad_box"]) == np.count_nonzero(sel) and not y["grad_box"][~_valid(c)].any()
    else:
        assert name + "_grad_box4" not in g and loss_bbox == 0 and y["grad_box"] is None


@pytest.mark.parametrize("shape", sorted(ll.FLAT))
def test_flat_restatement_equals_reference(g, shape):
    c, name = ll.make_flat(shape), ll.flat_name(shape)
    assert lr.same_bits(ll.flat_digest(c), g[name + "_sha"])
    loss, grad = lr.smooth_l1(c["pred"], c["targets"], c["alpha_in"], c["alpha_out"], c["beta"])
    y, e_ref = g[name + "_scalars"]
    terms = float(np.abs(grad).sum())                                        # (the terms cancel: alpha_out takes both signs)
    assert abs(float(loss) - y) <= 1e-12 * max(abs(y), terms)
    assert np.abs(grad.reshape(-1)[ll.flat_sample(shape)] - g[name + "_grad"]).max() <= 1e-13 * np.abs(grad).max()
    sample = ll.flat_sample(shape)
    assert np.all(np.isin(np.arange(max(c["pred"].size - 8, 0), c["pred"].size), sample)) and np.all(grad != 0)


# ---- the launch arithmetic is the kernels' ------------------------------------------------------------------------------------------
def _source(*path):
    with open(os.path.join(ROOT, "detectorch_amd", "csrc", "loss", *path)) as f:
        return f.read()


def test_restated_launch_arithmetic_is_the_source():
    common, head, flat = _source("loss_common.h"), _source("fast_rcnn_loss.hip"), _source("smooth_l1.hip")
    const = lambda text, name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert (const(common, "kLossThreads"), const(common, "kLossMaxBlocks")) == (ll.THREADS, ll.MAX_BLOCKS) and ll.WAVES == ll.THREADS // 64
    assert "while (L < 64 && 4 * L < c) L <<= 1;" in head and "if (c <= 256)" in head
    assert "const int rows_per_block = 64 / p.L * dtc::kLossWaves;" in head
    assert "std::min(dtc::ceil_div(n, rows_per_block), dtc::kLossMaxBlocks)" in head
    assert "(total / 4 + dtc::kLossThreads - 1) / dtc::kLossThreads, 1), dtc::kLossMaxBlocks)" in flat
    assert [ll.lanes_per_row(c) for c in (2, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 1024)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64, 64]
    assert [ll.regs(c) for c in (2, 256, 257, 1024)] == [4, 4, 16, 16]
    assert all(ll.regs(c) * ll.lanes_per_row(c) >= c for c in range(2, 1025))      # every column has a register


# ---- 1, 2: the sweep -------------------------------------------------------------------------------------------------------------------
def test_sweep_takes_every_boundary_from_both_sides():
    assert set(ll.SWEEP_C) == set(ll.SWEEP_REACHES)
    for c, reach in ll.SWEEP_REACHES.items():
        assert (ll.lanes_per_row(c), ll.regs(c)) == reach, c
    L = ll.lanes_per_row
    for lo, hi in ((4, 5), (8, 9), (16, 17), (32, 33)):
        assert lo in ll.SWEEP_C and hi in ll.SWEEP_C and 2 * L(lo) == L(hi)
    assert (L(128), L(ll.WRAPS["r130"][0])) == (32, 64) and L(129) == 64          # 128 / 129: the sweep below, (130, 4099) above
    assert (ll.regs(256), ll.regs(257)) == (4, 16) and L(256) == L(257) == 64
    assert {L(c) for c in ll.SWEEP_C} == {1, 2, 4, 8, 16, 32, 64}
    assert ll.slots(1023) == 16 and 1023 - 15 * 64 == 63                          # the last slot of the E = 16 body: lane 63 masked


@pytest.mark.parametrize("name", ["s%d" % c for c in ll.SWEEP_C] + ["w%d" % c for c in ll.AGNOSTIC_C])
def test_sweep_case_covers_slots_lanes_and_rows(name):
    c, y = ll.case(name), ll.want(name)
    x, labels, pred, t5 = c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"]
    N, C = x.shape
    L, E = ll.lanes_per_row(C), ll.regs(C)
    assert N == 67 and pred.shape[1] == (8 if name[0] == "w" else 4 * C)
    valid = _valid(c)
    ok = valid & (labels < C)
    assert np.array_equal(~valid, np.arange(N) % 5 == 4)
    assert np.all(np.isnan(x[~valid])) and np.all(np.isnan(pred[~valid])) and np.all(np.isnan(t5[~valid]))
    assert np.all(np.isfinite(x[valid])) and np.all(np.isfinite(pred[valid])) and np.all(np.isfinite(t5[valid]))
    assert np.sum(labels == C) == 1 and np.sum(labels == C + 7) == 1 and y["n_valid"] == 54 == ok.sum() + 2
    # every register slot that holds a column, and the first and last lane of a row, is some valid row's label column
    slot, lane = labels[ok] // L, labels[ok] % L
    assert set(slot) == set(range(ll.slots(C))) and ll.slots(C) == min(E, -(-C // L))
    assert 0 in lane and L - 1 in lane
    # ... and the argmax lands in every slot, first and last lane too; about half the rows are hits
    am = lr.argmax_logits(x[ok])
    assert set(am // L) == set(range(ll.slots(C))) and 0 in am % L and L - 1 in am % L
    top2 = np.sort(x[ok], axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] >= 1.0
    assert clear.sum() == ok.sum() - 1 and not clear[list(np.where(ok)[0]).index(ll.ROW_TIE)]
    hits = int(np.sum(am == labels[ok]))
    assert 0.4 * ok.sum() <= hits <= 0.9 * ok.sum() and 0 < float(y["accuracy"]) < 1
    # the tie: two equal winners in different lanes, the lower index (the label) in the higher lane
    t = np.where(x[ll.ROW_TIE] == x[ll.ROW_TIE].max())[0]
    assert list(t) == [1, max(L, 2)] and labels[ll.ROW_TIE] == 1 and am[list(np.where(ok)[0]).index(ll.ROW_TIE)] == 1
    if L > 1:
        assert t[0] % L == 1 and t[1] % L == 0
    # box targets: keyed by the label on foreground rows; class C - 1; a background row that carries targets
    k = t5[valid, 0]
    fg = (labels[valid] > 0) & (labels[valid] < C)
    plain = fg & (np.where(valid)[0] != ll.ROW_LAST_CLASS)
    assert np.array_equal(k[plain], labels[valid][plain]) and t5[ll.ROW_LAST_CLASS, 0] == C - 1
    assert np.any((labels[valid] == 0) & (k > 0)) and np.any(k == 0) and np.any(k == 1) and np.any(k == C - 1)
    rows = np.where(valid)[0]
    assert np.array_equal(y["grad_box"][rows].any(axis=1), k > 0)
    if name[0] == "w":
        assert not y["grad_box"][:, :4].any() and y["grad_box"][rows[k == 1], 4:].all() and y["grad_box"][rows[k == C - 1], 4:].all()
    else:
        assert y["grad_box"][ll.ROW_LAST_CLASS, 4 * C - 4:].all()                  # the last 16 bytes of a row


def test_engineered_labels_at_1024_reach_the_columns_past_256():
    c = ll.case("s1024")
    ok = _valid(c) & (c["labels"] < 1024)
    assert np.sum(c["labels"][ok] >= 256) >= 30 and np.sum(lr.argmax_logits(c["cls_score"][ok]) >= 256) >= 30
    assert ll.AGNOSTIC_C == (3, 81, 257) and [ll.lanes_per_row(c) for c in ll.AGNOSTIC_C] == [1, 32, 64]


# ---- 3: the row loop ---------------------------------------------------------------------------------------------------------------------
def test_wrap_cases_wrap():
    want = {"r130": (130, 4099, 64, 4, 1024, 2), "r257": (257, 4101, 64, 4, 1024, 2), "r33": (33, 16387, 16, 16, 1024, 2),
            "r17": (17, 32771, 8, 32, 1024, 2), "ce257": (257, 65536, 64, 4, 1024, 16), "ce2": (2, 65536, 1, 256, 256, 1)}
    assert set(want) == set(ll.WRAPS)
    for name, (C, N, L, rpb, grid, trips) in want.items():
        assert ll.WRAPS[name][:2] == (C, N) and ll.WRAPS[name][3] == trips
        assert (ll.lanes_per_row(C), ll.rows_per_block(C), ll.grid(N, C), ll.trips(N, C)) == (L, rpb, grid, trips), name
        assert (N > 1024 * (64 // L) * 4) == (trips > 1)
    assert (ll.regs(257), ll.regs(130)) == (16, 4)
    for name in ("r130", "r257", "r33", "r17"):                              # the last trip's last workgroup is partly past N ...
        C, N = ll.WRAPS[name][:2]
        assert N % ll.rows_per_block(C) != 0
        if ll.lanes_per_row(C) < 64:                                         # ... and so is its last wavefront, where it holds > 1 row
            assert N % (64 // ll.lanes_per_row(C)) != 0


@pytest.mark.parametrize("name", ("r130", "r33", "ce2"))
def test_wrap_case_inputs(name):
    c = ll.case(name)
    C, N, box, _ = ll.WRAPS[name]
    valid = _valid(c)
    assert c["cls_score"].shape == (N, C) and 0.23 < np.mean(~valid) < 0.27
    assert np.all(np.isnan(c["cls_score"][~valid])) and np.all(np.isfinite(c["cls_score"][valid]))
    assert (c["bbox_pred"] is not None) == box
    second = np.arange(N) >= ll.grid(N, C) * ll.rows_per_block(C)            # rows of the second trip: valid ones among them
    if ll.trips(N, C) > 1:
        assert valid[second].any() and 0 < second.sum() < ll.rows_per_block(C)
    else:
        assert not second.any()


def test_one_valid_row_is_reached_on_the_second_trip():
    c, y = ll.case(ll.ONE_VALID), ll.want(ll.ONE_VALID)
    N, C = c["cls_score"].shape
    assert (N, C) == (4099, 130) and list(np.where(_valid(c))[0]) == [4098] and 4098 >= ll.grid(N, C) * ll.rows_per_block(C)
    assert y["n_valid"] == 1 and np.count_nonzero(y["grad_box"]) == 4
    row = lr.head(c["cls_score"][4098:], c["labels"][4098:], c["bbox_pred"][4098:], c["targets5"][4098:])
    assert float(row["loss_cls"]) == float(y["loss_cls"]) > 0 and float(row["loss_bbox"]) == float(y["loss_bbox"]) > 0


# ---- 4: target-class values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agnostic", (False, True))
def test_target_class_values(agnostic):
    c, off = ll.make_target_classes(agnostic)
    k = c["targets5"][:7, 0]
    assert k.dtype == np.float32 and np.signbit(k[0]) and k[0] == 0 and 0 < k[1] < np.finfo(np.float32).tiny
    assert k[2] == np.float32(0.999) and k[3] == 80.5 and np.isposinf(k[4]) and k[5] == 2.0 ** 24 and k[6] == 80
    assert c["bbox_pred"].shape[1] == (8 if agnostic else 324) and np.all(c["labels"][:7] >= 0)
    y = lr.head(c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"])
    assert list(y["grad_box"][:7].any(axis=1)) == [False] * 6 + [True]       # C - 1 is the only one with a box term
    y_off = lr.head(off["cls_score"], off["labels"], off["bbox_pred"], off["targets5"])
    # (loss_ref.head rescales by the count of rows it hands to smooth_l1, which differs between the two: a float64 rounding)
    assert abs(float(y["loss_bbox"]) - float(y_off["loss_bbox"])) <= 1e-15 * float(y["loss_bbox"])
    assert np.abs(y["grad_box"] - y_off["grad_box"]).max() <= 1e-15 * np.abs(y["grad_box"]).max()
    assert np.all(c["targets5"][:6, 1:] == 0.25) and not off["targets5"][:6].any()


# ---- 5: magnitudes --------------------------------------------------------------------------------------------------------------------------
def _finite_and_normal(loss, grads):
    with np.errstate(over="ignore"):
        assert np.isfinite(np.float32(loss))
    for gr in grads:
        nz = gr != 0
        assert np.all(np.isfinite(gr)) and (not nz.any() or np.abs(gr[nz]).min() >= 2.0 ** -100)


def test_magnitude_logits():
    c, y = ll.case("mlogits"), ll.want("mlogits")
    x, labels = c["cls_score"], c["labels"]
    rows = np.arange(len(labels))
    assert np.all(np.isfinite(x)) and ll.MAG_ROWS[:6] == ("low_label", "low_label2", "equal", "denormal", "onehot_hit", "onehot_miss")
    for r in (0, 1):
        assert set(np.unique(x[r])) == {-ll.BIG, ll.BIG} and x[r, labels[r]] == -ll.BIG
        assert np.isfinite(np.float32(x[r].max()) - np.float32(x[r, labels[r]]))      # 2e38 is still a float32
    assert np.all(x[2] == x[2, 0]) and np.all(x[3] > 0) and np.all(x[3] < np.finfo(np.float32).tiny)
    for r in (4, 5):
        assert np.sum(x[r] == ll.BIG) == 1 and np.sum(x[r] == -ll.BIG) == 80
    assert lr.argmax_logits(x)[4] == labels[4] and lr.argmax_logits(x)[5] != labels[5]
    # the softmax of a one-hot row is exactly one-hot: the label column's gradient is 0 on the hit and -1 / n_valid on the miss
    assert y["grad_cls"][4, labels[4]] == 0 and not y["grad_cls"][4].any()
    assert y["grad_cls"][5, labels[5]] == -1.0 / 8 and y["grad_cls"][5, 45] == 1.0 / 8 and np.count_nonzero(y["grad_cls"][5]) == 2
    _finite_and_normal(y["loss_cls"], [y["grad_cls"]])
    assert float(y["loss_cls"]) > 5e37


@pytest.mark.parametrize("name", sorted(ll.MAG_BETAS))
def test_magnitude_box(name):
    c, y = ll.case(name), ll.want(name)
    beta, res = ll.MAG_BETAS[name]
    assert c["beta"] == float(np.float32(beta)) > 0 and np.all(np.isfinite(c["bbox_pred"])) and np.all(np.isfinite(c["targets5"]))
    k = c["targets5"][:, 0].astype(int)
    x = np.concatenate([c["bbox_pred"][r, 4 * k[r]:4 * k[r] + 4].astype(np.float64) - c["targets5"][r, 1:] for r in range(8)])
    ax = np.abs(x)
    assert np.any(x == 0) and np.any(x > 0) and np.any(x < 0) and np.any(ax == c["beta"])
    assert np.any(ax > c["beta"]) and ax.max() >= 9e37                       # both arms
    if name != "b149":
        assert np.any((ax < c["beta"]) & (ax > 0))
    if name in ("b149", "b126"):
        assert np.any((ax > 0) & (ax < 1e-39))                               # a float32 denormal residual
    if name == "b3e38":
        assert ax.max() > 3.5e38                                             # past the float32 range: the difference exists in double only
    _finite_and_normal(y["loss_bbox"], [y["grad_box"]])
    bt, bi, bo = lr.expand(c["targets5"], 20)                                # the same numbers through the other entry
    loss, grad = lr.smooth_l1(c["bbox_pred"], bt, bi, bo, c["beta"])
    assert float(loss) == float(y["loss_bbox"]) and np.array_equal(grad, y["grad_box"])


def test_magnitude_alpha():
    c = ll.make_magnitude_alpha()
    assert {tuple(p) for p in np.stack([c["alpha_in"][:, 0], c["alpha_out"][:, 0]], 1)} == \
        {(np.float32(a), np.float32(b)) for a in (0.0, -1.5, 1e10) for b in (0.0, -1.0, 2.0 ** -20)}
    loss, grad = lr.smooth_l1(c["pred"], c["targets"], c["alpha_in"], c["alpha_out"], c["beta"])
    _finite_and_normal(loss, [grad])
    assert not grad[(c["alpha_in"] == 0) | (c["alpha_out"] == 0)].any() and np.count_nonzero(grad) >= 40
    x = (c["pred"].astype(np.float64) - c["targets"]) * c["alpha_in"]
    assert np.abs(x).max() >= 1e29 and np.any((np.abs(x) < 1) & (x != 0)) and float(loss) != 0


# ---- 6, 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_upstream_sets():
    assert ll.UPSTREAMS == ((0.0, 0.0), (-2.0, 0.25), (0.0, 3.0), (1.0, 0.0))


def test_flat_shapes_reach_their_left_over_and_wrap():
    issue = [(1, 1), (1, 2), (1, 3), (7, 1), (5, 1), (2, 3), (3, 2), (1025, 1024), (3, 349527), (1, 1048579)]
    assert list(ll.FLAT)[:len(issue)] == issue
    for (N, W), (left, wraps) in ll.FLAT.items():
        total = N * W
        assert total % 4 == left and ll.flat_wraps(total) == wraps, (N, W)
        assert ll.flat_blocks(total) == (1024 if total >= 4 * 256 * 1024 else max(-(-(total // 4) // 256), 1))
    assert [s for s in ll.FLAT if s[0] * s[1] < 4] == [(1, 1), (1, 2), (1, 3)]          # no 16-byte piece at all
    assert {ll.FLAT[s][0] for s in ll.FLAT if ll.FLAT[s][1]} == {0, 1, 3}                # wraps with left-overs 0, 1 and 3
    # (1, 1048579): one 16-byte piece for every thread of the full grid and none left for a second trip; 4 more elements wrap
    assert 1048579 // 4 == 1024 * 256 and not ll.flat_wraps(1048579) and ll.flat_wraps(1048583)


def test_the_two_arms_of_smooth_l1_agree_bit_for_bit_on_the_boundary():
    """Why `ax <= beta` against `ax < beta` cannot be seen in any output (the mutation run (e) of tests/README_loss.md): with
    |x| == beta, a float32 widened to double, 0.5 x^2 / beta and |x| - 0.5 beta are both exactly 0.5 beta (x^2 has at most 48
    significant bits) and x / beta is exactly sign(x): smooth-L1 and its derivative are continuous there, in double bit for bit."""
    rs = np.random.RandomState(6)
    beta = np.concatenate([rs.randint(1, 0x7F7FFFFF, 100000).astype(np.uint32).view(np.float32).astype(np.float64),
                           [ll.B149, ll.B126, ll.B100, float(np.float32(3e38)), 1.0, 0.5, float(np.float32(1.0 / 9.0))]])
    for x in (beta, -beta):
        assert np.array_equal(0.5 * x * x / beta, np.abs(x) - 0.5 * beta) and np.array_equal(x / beta, np.sign(x))
