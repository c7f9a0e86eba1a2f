"""libdetectorch_aug_hip.so on the MI355X past where tests/test_hip_tta.py stops (-m gpu; the "Limits" section of
tests/README_tta.md): the cases of tests/tta_limit_cases.py against the restatement (tests/tta_ref.py), every output pre-filled with
NaN (0xFF bytes for integers).

REQUIRED AGREEMENT: the merge, SOFT_AVG and SOFT_MAX equal the restatement bit for bit (a NaN by its place).  LOGIT_AVG keeps the rule
of tests/test_hip_tta.py: within twice the largest distance of the float32 form numpy runs from the float64 form of the rule on the
same inputs, computed per case."""
import numpy as np
import pytest
import torch

import tta_limit_cases as lc
import tta_ref as tr
from test_hip_tta import aug, nan_filled, host, same_bits  # noqa: F401  (aug is a fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32


def cu(a):
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the cases are read-only


def run_merge(aug, views, im, sh, ch, logits):
    B, R, C = views[0]["cls_score"].shape
    out = nan_filled(aug.merge_outputs(B, aug.merge_rows(len(views), R, sh), C, "cuda"))
    dv = [{k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in view.items()} for view in views]
    aug.merge_boxes(dv, cu(im), sh, ch, logits, out=out)
    torch.cuda.synchronize()
    return host(out)


def check_merge(got, ref):
    for k in ("out_n", "out_src", "out_scores", "out_boxes"):   # NaN pre-fill: rows past out_n must read zero, out_src -1
        assert same_bits(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:5])


# ---- the merge -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(lc.MERGES)), ids=["T%d-%s-%s-c%d-%s" % (c[0], c[1][0], c[1][1], c[2], "logits" if c[5] else "probs")
                                                            for c in lc.MERGES])
def test_merge_limit_case(aug, k):
    T, heurs, n_cls, R, counts, logits = lc.MERGES[k]
    views, im = lc.merge_case(T, R, n_cls, counts, logits)
    ref = tr.merge_boxes(views, im, heurs[0], heurs[1], logits)
    check_merge(run_merge(aug, views, im, heurs[0], heurs[1], logits), ref)
    assert ref["out_n"].min() > 0


def test_merge_of_32768_rows(aug):
    views, im = lc.merge_rows_limit()
    ref = tr.merge_boxes(views, im)
    check_merge(run_merge(aug, views, im, "UNION", "UNION", False), ref)
    assert ref["out_n"][0] == sum(lc.ROWS_COUNTS) and ref["out_n"][0] % 4


@pytest.mark.parametrize("logits", [False, True])
def test_merge_of_65535_images(aug, logits):
    views, im, want = lc.merge_batch_limit(logits)
    check_merge(run_merge(aug, views, im, "UNION", "UNION", logits), want)


# ---- the combination -------------------------------------------------------------------------------------------------------------------------------
def run_combine(aug, masks, flipped, cnt, mc, heur):
    out = torch.full(masks[0].shape, float("nan"), device="cuda")
    aug.combine_masks([cu(m) for m in masks], flipped, cu(cnt), None if mc is None else cu(mc), heur, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_logit_avg(aug, masks, flipped, cnt, mc, label):
    ref64 = tr.combine_masks64(masks, flipped, cnt, mc)
    lit = tr.combine_masks(masks, flipped, cnt, mc, "LOGIT_AVG", exact=False)
    tol = 2 * np.abs(lit.astype(np.float64) - ref64).max()
    got = run_combine(aug, masks, flipped, cnt, mc, "LOGIT_AVG")
    dev = np.abs(got.astype(np.float64) - ref64).max()
    print("LOGIT_AVG %s: device %.3e, float32 form %.3e, tolerance %.3e" % (label, dev, tol / 2, tol))
    assert np.isfinite(got).all() and tol > 0 and dev <= tol
    assert same_bits(got == 0, ref64 == 0) and not np.signbit(got).any()


@pytest.mark.parametrize("with_class", [True, False])
@pytest.mark.parametrize("M,T", lc.COMBINES)
def test_soft_combinations_at_the_mask_sizes(aug, M, T, with_class):
    masks, flipped, cnt, mc = lc.combine_case(M, T)
    mc = mc if with_class else None
    for heur in ("SOFT_AVG", "SOFT_MAX"):
        assert same_bits(run_combine(aug, masks, flipped, cnt, mc, heur), tr.combine_masks(masks, flipped, cnt, mc, heur)), heur


@pytest.mark.parametrize("with_class", [True, False])
@pytest.mark.parametrize("M,T", lc.COMBINES)
def test_logit_avg_at_the_mask_sizes(aug, M, T, with_class):
    masks, flipped, cnt, mc = lc.combine_case(M, T, special=True)
    check_logit_avg(aug, masks, flipped, cnt, mc if with_class else None, "M=%d T=%d class=%d" % (M, T, with_class))


@pytest.mark.parametrize("where", lc.NAN_PLACES)
@pytest.mark.parametrize("M", [4, 7])
def test_a_nan_stays_under_soft_max(aug, M, where):
    masks, flipped, cnt, place = lc.nan_case(M, where)
    got, ref = run_combine(aug, masks, flipped, cnt, None, "SOFT_MAX"), tr.combine_masks(masks, flipped, cnt, None, "SOFT_MAX")
    assert np.isnan(got[place]) and same_bits(np.isnan(got), np.isnan(ref)) and same_bits(np.nan_to_num(got), np.nan_to_num(ref))


@pytest.mark.parametrize("with_class", [True, False])
def test_combination_of_66000_mask_rows(aug, with_class):
    masks, flipped, cnt, mc = lc.combine_rows_limit()
    mc = mc if with_class else None
    for heur in ("SOFT_AVG", "SOFT_MAX"):
        assert same_bits(run_combine(aug, masks, flipped, cnt, mc, heur), tr.combine_masks(masks, flipped, cnt, mc, heur)), heur
    check_logit_avg(aug, masks, flipped, cnt, mc, "66000 rows class=%d" % with_class)
