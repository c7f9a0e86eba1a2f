"""The limit cases of the test-time-augmentation library without a GPU and without the library (the "Limits" section of
tests/README_tta.md): every case of tests/tta_limit_cases.py holds the condition it is named for, the vectorised expectations equal
the restatement on a sample, and the cases tell the mutants of the README's table from the contract."""
import re
import os

import numpy as np
import pytest

from conftest import ROOT
import tta_cases as tc
import tta_limit_cases as lc
import tta_ref as tr

f32 = np.float32


def define(name):
    header = open(os.path.join(ROOT, "include", "detectorch_aug_hip.h")).read()
    return eval(re.search(r"#define DTC_AUG_%s (\(?[\d <]+\)?)" % name, header).group(1))


def test_the_cases_stand_on_the_limits_of_the_header():
    assert (define("MAX_VIEWS"), define("MAX_ROIS"), define("MAX_ROWS"), define("MAX_CLASSES"), define("MAX_BATCH"), define("MAX_MASK")) == (
        8, 4096, 32768, 256, 65535, 64)
    assert max(c[2] for c in lc.MERGES) == define("MAX_CLASSES") + 1 and max(c[0] for c in lc.MERGES) == define("MAX_VIEWS")
    assert len(lc.ROWS_COUNTS) == 8 and max(lc.ROWS_COUNTS) == define("MAX_ROIS") and 8 * 4096 == define("MAX_ROWS")
    assert lc.NB == define("MAX_BATCH") and max(lc.SIZES) == define("MAX_MASK")
    assert lc.ROWS_B * lc.ROWS_MAX_OUT > 65535 and lc.ROWS_B * lc.ROWS_MAX_OUT <= define("MAX_MASK_ROWS")


@pytest.mark.parametrize("k", range(len(lc.MERGES)))
def test_merge_cases_hold_their_conditions(k):
    T, heurs, n_cls, R, counts, logits = lc.MERGES[k]
    views, im = lc.merge_case(T, R, n_cls, counts, logits)
    assert len(views) == T and views[0]["cls_score"].shape == (2, R, n_cls) and n_cls > 64       # more than one class per lane and slot
    assert [v["flipped"] for v in views] == [bool(f) for f in tc.FLIPS[:T]]
    ref = tr.merge_boxes(views, im, heurs[0], heurs[1], logits)
    live = ref["out_scores"][1, :ref["out_n"][1]]
    assert ref["out_n"].min() > 0 and np.isfinite(live).all() and np.isfinite(ref["out_boxes"]).all()
    assert np.abs(live.sum(axis=1) - 1).max() < 1e-4 and (live[:, 64:] > 0).any()                # probabilities; mass past class 63
    if T == 8 and heurs == ("AVG", "AVG"):                      # the mutant that adds the first four views only
        first4 = np.sum([tr.merge_boxes([v], im, logits=logits)["out_scores"][:, :R] for v in views[:4]], axis=0) / f32(8)
        assert not np.array_equal(first4, ref["out_scores"])
    if T == 8 and heurs[0] != heurs[1]:                         # each output by its own heuristic
        avg, ident = tr.merge_boxes(views, im, "AVG", "AVG", logits), tr.merge_boxes(views, im, "ID", "ID", logits)
        s, c = ("out_scores", "out_boxes") if heurs[0] == "AVG" else ("out_boxes", "out_scores")
        assert np.array_equal(ref[s], avg[s]) and np.array_equal(ref[c], ident[c]) and not np.array_equal(avg[c], ident[c])


def test_merge_rows_limit_holds_its_conditions():
    views, im = lc.merge_rows_limit()
    counts = [int(v["n_rois"][0]) for v in views]
    assert len(views) == 8 and views[0]["cls_score"].shape == (1, 4096, 2) and counts == list(lc.ROWS_COUNTS)
    assert sum(counts) % 4 and 0 in counts and 4096 in counts
    ref = tr.merge_boxes(views, im)
    assert ref["out_scores"].shape == (1, 32768, 2) and ref["out_n"][0] == sum(counts)
    src = ref["out_src"][0, :sum(counts)]
    assert src[0] == 0 and src[-1] == 7 * 4096 + 4095 and (np.diff(src) > 0).all() and not ((src >= 2 * 4096) & (src < 3 * 4096)).any()
    assert (ref["out_src"][0, sum(counts):] == -1).all() and not ref["out_boxes"][0, sum(counts):].any()


@pytest.mark.parametrize("logits", [False, True])
def test_merge_batch_formula_is_the_restatement_on_a_sample(logits):
    views, im, want = lc.merge_batch_limit(logits)
    assert views[0]["cls_score"].shape == (65535, 1, 2) and want["out_boxes"].shape == (65535, 1, 8)
    rows = np.r_[0:40, 65535 - 40:65535]
    sub = [{k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in views[0].items()}]
    ref = tr.merge_boxes(sub, im[rows], logits=logits)
    for k in ref:
        assert np.array_equal(ref[k], want[k][rows]) and ref[k].dtype == want[k].dtype, k
    assert set(want["out_n"].tolist()) == {0, 1} and len(np.unique(want["out_boxes"][:, 0, 4])) > 300      # chosen from b


@pytest.mark.parametrize("M,T", lc.COMBINES)
def test_combine_cases_hold_their_conditions(M, T):
    masks, flipped, cnt, mc = lc.combine_case(M, T, special=True)
    K = lc.channels(M)
    assert len(masks) == T and masks[0].shape == (12, K, M, M) and any(flipped) and not all(flipped)
    assert all(0 <= m.min() and m.max() <= 1 for m in masks) and all(np.isin(tc.SPECIAL, m).sum() >= min(3, M * M) for m in masks[:1])
    ref64 = tr.combine_masks64(masks, flipped, cnt, mc)
    lit = tr.combine_masks(masks, flipped, cnt, mc, "LOGIT_AVG", exact=False)
    assert np.isfinite(lit).all() and np.abs(lit.astype(np.float64) - ref64).max() > 0          # the tolerance of the GPU test
    if M > 1:                                                   # the flags matter: unflipped views give another answer
        assert not np.array_equal(tr.combine_masks(masks, flipped, cnt, None, "SOFT_AVG"), tr.combine_masks(masks, [0] * T, cnt, None, "SOFT_AVG"))
    if T == 8:
        assert not np.array_equal(tr.combine_masks(masks, flipped, cnt, None, "SOFT_MAX"), tr.combine_masks(masks[:4], flipped[:4], cnt, None, "SOFT_MAX"))


@pytest.mark.parametrize("where", lc.NAN_PLACES)
@pytest.mark.parametrize("M", [4, 7])
def test_nan_cases_hold_their_conditions(M, where):
    masks, flipped, cnt, place = lc.nan_case(M, where)
    assert flipped == (0, 1, 1) and sum(int(np.isnan(m).sum()) for m in masks) == 1
    ref = tr.combine_masks(masks, flipped, cnt, None, "SOFT_MAX")
    assert np.isnan(ref[place]) and np.isnan(ref).sum() == 1                                     # a NaN stays, at the mirrored place
    mutant = np.where(ref == 0, f32(0), lc.soft_max_without_the_nan_arm(masks, flipped))
    assert np.isnan(mutant[place]) == (where == "first_view")                                    # `v > a` alone loses a later NaN


def test_combine_rows_limit_holds_its_conditions():
    masks, flipped, cnt, mc = lc.combine_rows_limit()
    assert masks[0].shape == (66000, 1, 4, 4) and cnt.shape == (33000,) and cnt[:6].tolist() == [0, 1, 2, 0, 1, 2]
    ref = tr.combine_masks(masks, flipped, cnt, mc, "SOFT_AVG")
    assert ref[65536:].any() and not ref[0].any() and ref[2].any()                               # det_count 0; 1 with class 0
    rows = np.flatnonzero(ref.reshape(66000, -1).any(axis=1))
    want = [r for r in range(66000) if r % 2 < cnt[r // 2] and mc[r] == 0]
    assert rows.tolist() == want and rows.max() > 65535
