"""Inputs, oracle-side expectations and the branch table of the collect / distribute argument tests (test support, not a test
module): shared by tests/test_hip_collect_args.py (GPU), tests/test_collect_args_host.py, which pins on the oracle alone the
conditions the GPU tests rely on (so that none of them can pass emptily), and tests/golden/make_collect_levels_golden.py.
Everything here is numpy + the oracle.

Tie order is pinned to the project's canonical rule (csrc/block_sort.h: score descending, then concatenation index ascending)
through oracle.collect; the reference's torch.sort leaves it unspecified.  Level mapping and distribution are pinned to the
reference through tests/golden/collect_levels.npz."""
import numpy as np

from detectorch_amd import synth

# ---- fpn_collect_launch restated (csrc/fpn.hip) -----------------------------------------------------------------------------------
THREADS = 1024                                  # fpn.hip: kFpnThreads
FAST_MAX_TOP = 2048                             # fpn.hip: kFastMaxTop
ORDER_BUCKETS = 512                             # fpn.hip: kOrderBuckets
FAST_LDS_BUDGET = 150 * 1024                    # fpn.hip, fpn_collect_launch: `if (fsm <= 150 * 1024)`
GENERAL_LDS_LIMIT = 144 * 1024                  # fpn.hip: kFpnGeneralLdsLimit
GENERAL_STATIC_LDS = 4 * (2 * 9 + 8 * 16 + 8)   # fpn.hip: kFpnGeneralStaticLds (lvl_off, in_off, wave_cnt, lvl_run) = 616
MAX_TOP, MAX_ROWS = 16384, 16384                # fpn_collect_launch: post_nms_top_n; dtc_fpn_collect_distribute: n_max with scores
EUNSUPPORTED = -4


def next_pow2(n):
    p = 2
    while p < n:
        p <<= 1
    return p


def plan(L_in, in_stride, top_n, scores=True, sorted_=True, keep=False, roi_order=True, no_fast=False):
    """What fpn_collect_launch does with a shape that passed the entries' argument checks
    -> dict(kernel "fast1" | "fast2" | "general" | None (DTC_EUNSUPPORTED), lds = dynamic LDS bytes of the launch, branch)
    branch = "<kernel>:<collect>:<visiting order>":
      collect  merge (pairwise merge-path tree) | plain (rows in the given order: no scores, or one sorted list) |
               rank_merge (binary-search ranks of sorted lists) | key_sort (block_bitonic_sort of the keys) | no_scores
      order    bucket (fast kernel) | count (general, top_n <= 2048) | bitonic (general, top_n > 2048) | none (roi_order NULL)"""
    n_max = L_in * in_stride
    none = dict(kernel=None, lds=0, branch="unsupported")
    if scores and not keep and n_max > MAX_ROWS:                      # dtc_fpn_collect_distribute: `in_scores && n_max > 16384`
        return none
    smem = next_pow2(n_max) * 8 if scores else 16                    # fpn_collect_launch: `size_t smem = ...`
    if scores and sorted_:
        smem = top_n * 8 + n_max * 4 + 16                            # `if (in_scores && inputs_sorted) smem = ...`
    if roi_order:
        smem = max(smem, max(4, next_pow2(top_n)) * 8 * 2)           # `if (p.roi_order) { const size_t so = ...`
    if top_n > MAX_TOP:                                              # `if (post_nms_top_n > 16384)`
        return none
    fast = (top_n <= FAST_MAX_TOP and in_stride <= 1024 and n_max <= 8192 and (not scores or sorted_) and
            (not no_fast or keep))                                   # `const bool fast = ...`
    if fast:
        R = 1 if top_n <= THREADS else 2
        hdr = 2 * R * THREADS * 4 + 2 * ORDER_BUCKETS * 4            # fast_hdr_bytes(R)
        merge = scores and L_in > 1
        fsm = hdr + ((n_max + (L_in - 1) * top_n) * 8 if merge else 0) + (n_max * 4 if keep else 0) + 16    # `const size_t fsm = ...`
        if fsm <= FAST_LDS_BUDGET:
            return dict(kernel="fast%d" % R, lds=fsm,
                        branch="fast%d:%s:%s" % (R, "merge" if merge else "plain", "bucket" if roi_order else "none"))
    if keep:                                                         # `if (p.keep) return DTC_EUNSUPPORTED`
        return none
    if smem > GENERAL_LDS_LIMIT - GENERAL_STATIC_LDS:                # the host guard
        return none
    collect = "no_scores" if not scores else ("rank_merge" if sorted_ else "key_sort")
    order = "none" if not roi_order else ("count" if top_n <= 2048 else "bitonic")
    return dict(kernel="general", lds=smem, branch="general:%s:%s" % (collect, order))


def sort_keys_per_thread(n):
    """keys per thread of block_bitonic_sort<1024> over next_pow2(n) keys (block_sort.h)"""
    return max(1, next_pow2(n) // THREADS)


# ---- the case table ------------------------------------------------------------------------------------------------------------------
TIE_GENS = ("quant16", "const", "cut", "zeros")
K_RANGES = [(2, 5), (2, 6), (3, 5), (4, 4), (0, 7), (1, 8)]          # the fixture's ranges; the GPU tests run all but (2, 5)


def _c(L, P, top_n, branch, **kw):
    d = dict(L=L, P=P, top_n=top_n, branch=branch, scores=True, sorted_=True, keep=False, roi_order=True, no_fast=False)
    d.update(kw)
    return d


# test -> the shapes it runs and the branch each is meant to reach
CASES = {
    "ties_fast_merge": [_c(5, 200, 300, "fast1:merge:bucket"), _c(5, 600, 1500, "fast2:merge:bucket")],
    "ties_general_sorted": [_c(5, 200, 2049, "general:rank_merge:bitonic"), _c(3, 1025, 1000, "general:rank_merge:count")],
    "ties_general_unsorted": [_c(5, 200, 300, "general:key_sort:count", sorted_=False)],
    "list_count_sweep": ([_c(1, 128, 300, "fast1:plain:bucket")] +
                         [_c(L, 128, 300, "fast1:merge:bucket") for L in (2, 3, 4, 6, 7, 8)] +
                         [_c(8, 1024, 1000, "fast1:merge:bucket")]),
    "general_kernel_sizes": [_c(5, 1000, 3000, "general:rank_merge:bitonic"), _c(8, 1025, 2000, "general:rank_merge:count"),
                             _c(8, 1024, 2048, "general:rank_merge:count"),
                             _c(1, 2100, 2100, "general:no_scores:bitonic", scores=False),
                             _c(8, 2048, 1000, "general:key_sort:count", sorted_=False)],
    "visiting_order_above_2048": [_c(1, T, T, "general:no_scores:bitonic", scores=False) for T in (2049, 4096, 8192)],
    "level_ranges": [_c(5, 200, 300, "fast1:merge:bucket"), _c(5, 200, 2049, "general:rank_merge:bitonic"),
                     _c(1, 512, 512, "fast1:plain:bucket", scores=False)],
    "kept_form": [_c(L, 128, 300, "fast1:merge:bucket", keep=True) for L in (2, 3, 8)],
    "optional_outputs_null": [_c(5, 200, 300, "fast1:merge:bucket"), _c(5, 200, 300, "fast1:merge:none", roi_order=False),
                              _c(5, 200, 2049, "general:rank_merge:bitonic"),
                              _c(5, 200, 2049, "general:rank_merge:none", roi_order=False)],
    "general_kernel_knob": ([_c(5, 200, 300, "general:rank_merge:count", no_fast=True),
                             _c(5, 600, 1500, "general:rank_merge:count", no_fast=True),
                             _c(1, 128, 300, "general:rank_merge:count", no_fast=True)] +
                            [_c(L, 128, 300, "general:rank_merge:count", no_fast=True) for L in (2, 3, 4, 6, 7, 8)] +
                            [_c(8, 1024, 1000, "general:rank_merge:count", no_fast=True)]),
}
SWEEP_L = (1, 2, 3, 4, 6, 7, 8)
UNSORTED_TOTALS = (16384, 257, 1025, 2049, 4097, 0, 1, 2, 600)      # general_kernel_sizes, (8, 2048, 1000): rows per image
KEPT_K_STRIDE = 300

# the host guard: (entry arguments, passes validation?) -- the largest shapes the general kernel holds and the first it does not
GUARD_CASES = {
    "order, top_n 8192": (dict(L=1, P=8192, top_n=8192, scores=False), True),
    "order, top_n 8193": (dict(L=1, P=8193, top_n=8193, scores=False), False),
    "order, top_n 16384": (dict(L=1, P=16384, top_n=16384, scores=False), False),
    "no order, no scores, top_n 16384": (dict(L=1, P=16384, top_n=16384, scores=False, roi_order=False), True),
    "sorted, 16384 rows, top_n 8192": (dict(L=8, P=2048, top_n=8192), True),
    "sorted, no order, 16384 rows, top_n 10161": (dict(L=8, P=2048, top_n=10161, roi_order=False), True),
    "sorted, no order, 16384 rows, top_n 10162": (dict(L=8, P=2048, top_n=10162, roi_order=False), False),
    "sorted, no order, 16384 rows, top_n 16384": (dict(L=8, P=2048, top_n=16384, roi_order=False), False),
    "sorted, no order, 3938 rows, top_n 16384": (dict(L=2, P=1969, top_n=16384, roi_order=False), True),
    "sorted, no order, 3940 rows, top_n 16384": (dict(L=2, P=1970, top_n=16384, roi_order=False), False),
    "unsorted, no order, 16384 rows, top_n 16384": (dict(L=8, P=2048, top_n=16384, sorted_=False, roi_order=False), True),
    "unsorted, order, 16384 rows, top_n 8193": (dict(L=8, P=2048, top_n=8193, sorted_=False), False),
    "kept, merge buffers past the fast budget": (dict(L=8, P=1024, top_n=2048, keep=True), False),
    "kept, 8 x 1024 -> 1000 (keys + merge outputs + keep rows past the fast budget)": (dict(L=8, P=1024, top_n=1000, keep=True), False),
    "kept, 8 x 512 -> 1000": (dict(L=8, P=512, top_n=1000, keep=True), True),
}


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
def mixed_counts(seed, L, P, top_n):
    """[3, L] int32: image 0 has its last list full and the others well filled; image 1 an empty list and a single-row list (L permitting)
    next to well-filled ones; image 2 fewer rois than top_n (a few rows, empty lists)"""
    rs = synth.rng(61, seed)
    c = np.zeros((3, L), np.int32)
    c[0] = rs.randint(max(P // 2, 1), P + 1, L)
    c[0, 0] = rs.randint(max(P // 4, 1), max(P // 2, 1) + 1)          # shorter than top_n in every case: a constant score crosses lists
    c[0, L - 1] = P
    c[1] = rs.randint(max(P // 2, 1), P + 1, L)
    if L > 1:
        c[1, 1] = 0
    if L > 2:
        c[1, L - 1] = 1
    c[2, 0] = min(3, P, max(top_n - 1, 1))
    if L > 3:
        c[2, 3] = 1
    return c


def split_total(rs, total, L, P):
    """L list lengths <= P that sum to `total`, uneven, some of them zero where there is room"""
    c = np.zeros(L, np.int64)
    left = total
    for l in rs.permutation(L):
        take = min(P, left, int(rs.randint(0, max(2 * total // L, 1) + 2)))
        c[l] = take
        left -= take
    for l in range(L):
        take = min(P - c[l], left)
        c[l] += take
        left -= take
    assert left == 0 and c.sum() == total
    return c.astype(np.int32)


# ---- scores ----------------------------------------------------------------------------------------------------------------------------
def _free(rs, n, lo=0.0, hi=1.0):
    return synth.dedupe_scores(rs.uniform(lo, hi, n).astype(np.float32))


def _desc(a):
    return np.sort(a)[::-1]


def gen_scores(gen, rs, counts_b, top_n):
    """one image: list of L float32 arrays (counts_b[l] scores each), every list non-increasing"""
    L = len(counts_b)
    n = int(np.sum(counts_b))
    if gen == "free":
        flat = _free(rs, n)
        cut = np.concatenate([[0], np.cumsum(counts_b)])
        return [_desc(flat[cut[l]:cut[l + 1]]) for l in range(L)]
    if gen == "quant16":
        return [_desc((np.round(rs.uniform(0, 1, c) * 16) / 16).astype(np.float32)) for c in counts_b]
    if gen == "const":
        return [np.full(c, 0.5, np.float32) for c in counts_b]
    if gen == "zeros":
        # positive tie-free heads, then a tail of zeros that starts before rank top_n where the image has more rows than that;
        # every fifth zero is -0.0
        n_pos = min(int(0.6 * n), int(0.7 * top_n))
        out, left = [], n_pos
        flat = _free(rs, n, 0.1, 1.0)
        pos = 0
        for l, c in enumerate(counts_b):
            h = min(int(c), left if l == L - 1 else min(left, int(round(c * n_pos / max(n, 1)))))
            left -= h
            z = np.zeros(int(c) - h, np.float32)
            z[rs.permutation(z.size)[:z.size // 5]] = -0.0
            out.append(np.concatenate([_desc(flat[pos:pos + h]), z]).astype(np.float32))
            pos += h
        return out
    if gen == "cut":
        # `a` scores above 0.5 (tie-free), a run of `t` scores == 0.5 spread over the lists with >= 16 rows, the rest below (tie-free):
        # the run covers ranks [a, a + t); a + t / 2 = top_n where the image has more than top_n + t / 2 rows -- rank top_n falls inside
        # the run -- and the middle of the image otherwise
        big = [l for l in range(L) if counts_b[l] >= 16]
        if len(big) < 3:
            return gen_scores("quant16", rs, counts_b, top_n)
        tl = np.zeros(L, np.int64)
        for l in big:
            tl[l] = min(int(counts_b[l]) // 2, max(16, 48 // len(big) + 1))
        t = int(tl.sum())
        a = (top_n if n > top_n + t // 2 else n // 2) - t // 2
        if a < 0:
            return gen_scores("quant16", rs, counts_b, top_n)
        room = np.asarray(counts_b, np.int64) - tl
        al = np.zeros(L, np.int64)
        left = a
        for l in rs.permutation(L):                                   # heads: share `a` over the lists' room, unevenly
            al[l] = min(room[l], left, int(rs.randint(0, 2 * a // L + 2)))
            left -= al[l]
        for l in range(L):
            take = min(room[l] - al[l], left)
            al[l] += take
            left -= take
        assert left == 0
        out = []
        for l in range(L):
            below = int(counts_b[l] - tl[l] - al[l])
            out.append(np.concatenate([_desc(_free(rs, int(al[l]), 0.6, 1.0)), np.full(int(tl[l]), 0.5, np.float32),
                                       _desc(_free(rs, below, 0.0, 0.4))]).astype(np.float32))
        return out
    raise ValueError(gen)


GARBAGE_SCORE = np.float32(5.0)        # rows past a list's count: outranks every real score, so a row read past a count shows


def make_inputs(seed, L, P, top_n, gen, counts=None, shuffle=False, roi_kw=None):
    """-> (boxes [B, L, P, 4], scores [B, L, P], counts [B, L]).  Rows below the counts: synth.make_rois boxes (tied rows are
    distinguishable) and gen_scores scores, each list in descending order unless `shuffle` (rows permuted inside each list, boxes
    and scores together: inputs_sorted = 0).  Rows past the counts: other boxes, GARBAGE_SCORE."""
    if counts is None:
        counts = mixed_counts(seed, L, P, top_n)
    counts = np.asarray(counts, np.int32)
    B = counts.shape[0]
    rs = synth.rng(62, seed)
    boxes = np.stack([synth.make_rois(rs, L * P, **(roi_kw or {})).reshape(L, P, 4) for _ in range(B)])
    scores = np.full((B, L, P), GARBAGE_SCORE, np.float32)
    for b in range(B):
        sc = gen_scores(gen, rs, counts[b], top_n)
        for l in range(L):
            c = int(counts[b, l])
            assert sc[l].shape == (c,) and (c < 2 or np.all(sc[l][:-1] >= sc[l][1:]))
            scores[b, l, :c] = sc[l]
            if shuffle and c > 1:
                perm = rs.permutation(c)
                scores[b, l, :c] = scores[b, l, perm]
                boxes[b, l, :c] = boxes[b, l, perm]
    return boxes.astype(np.float32), scores, counts


def make_kept_inputs(seed, L, top_n, gen, keep_stride=128, k_stride=KEPT_K_STRIDE):
    """dtc_fpn_collect_distribute_kept: -> (sorted_boxes [B * L, k_stride, 4], sorted_scores [B * L, k_stride], keep [B * L, keep_stride]
    int32 with garbage past the counts, counts [B, L], and the gathered lists boxes [B, L, keep_stride, 4] / scores [B, L, keep_stride]
    whose rows below the counts are sorted[keep])"""
    counts = mixed_counts(seed, L, keep_stride, top_n)
    B = counts.shape[0]
    rs = synth.rng(63, seed)
    S = B * L
    sboxes = synth.make_rois(rs, S * k_stride).reshape(S, k_stride, 4)
    sscores = np.zeros((S, k_stride), np.float32)
    keep = rs.randint(-2 ** 31, 2 ** 31 - 1, (S, keep_stride)).astype(np.int32)
    gb = np.zeros((B, L, keep_stride, 4), np.float32)
    gs = np.full((B, L, keep_stride), GARBAGE_SCORE, np.float32)
    for b in range(B):
        full = gen_scores(gen, rs, np.full(L, k_stride), top_n)             # the whole pre-NMS segments, sorted
        for l in range(L):
            s_, c = b * L + l, int(counts[b, l])
            sscores[s_] = full[l]
            keep[s_, :c] = np.sort(rs.permutation(k_stride)[:c])           # ascending positions = score order
            gb[b, l, :c] = sboxes[s_, keep[s_, :c]]
            gs[b, l, :c] = sscores[s_, keep[s_, :c]]
    return sboxes.astype(np.float32), sscores, keep, counts, gb, gs


# ---- expectations -----------------------------------------------------------------------------------------------------------------------
def concat(boxes_b, scores_b, counts_b):
    L = len(counts_b)
    rc = np.concatenate([boxes_b[l, :counts_b[l]] for l in range(L)]).reshape(-1, 4)
    sc = None if scores_b is None else np.concatenate([scores_b[l, :counts_b[l]] for l in range(L)])
    return rc, sc


def expected(boxes, scores, counts, top_n, k_min, k_max):
    """Per image, from oracle.collect + oracle.distribute (which maps through oracle.map_rois_to_fpn_levels): list of
    dict(n_out, rois [n, 4], roi_scores [n] (None without scores), roi_levels [top_n] (level - k_min, -1 past n), idx_restore [n],
    level_counts [k_max - k_min + 1], rois_by_level [n, 4], src [n] = concatenation index of every output row).
    Without scores: the first rows of the lists as they are (list 0 when there is one list), at most top_n."""
    import oracle as orc
    out = []
    for b in range(boxes.shape[0]):
        rc, sc = concat(boxes[b], None if scores is None else scores[b], counts[b])
        if sc is None:
            m = min(rc.shape[0], top_n)
            top, tsc, src = rc[:m], None, np.arange(m)
        else:
            top, tsc, src = orc.collect(rc, sc, top_n)
        n = top.shape[0]
        outs, restore, lv = orc.distribute(top, k_min, k_max)
        assert np.array_equal(lv, orc.map_rois_to_fpn_levels(top, k_min, k_max))
        levels = np.full(top_n, -1, np.int32)
        levels[:n] = lv - k_min
        out.append(dict(n_out=n, rois=top, roi_scores=tsc, roi_levels=levels, idx_restore=restore.astype(np.int32),
                        level_counts=np.array([o.shape[0] for o in outs], np.int32),
                        rois_by_level=np.concatenate(outs).reshape(-1, 4) if n else np.zeros((0, 4), np.float32), src=src))
    return out


def list_of(src, counts_b):
    """the input list of every concatenation index"""
    return np.searchsorted(np.cumsum(counts_b), src, side="right")


def tie_stats(e, scores_cat, counts_b, top_n):
    """on one image's expectation: (pairs of equal-score rows that come from different lists inside the result,
    lists with a row tied with the score at the cut inside the result, lists with one outside it)"""
    lst = list_of(e["src"], counts_b)
    s = e["roi_scores"]
    pairs = 0
    for v in np.unique(s):                                       # rows i < j with equal scores and different lists (-0.0 == 0.0)
        per_list = np.bincount(lst[s == v])
        pairs += int((per_list.sum() ** 2 - (per_list ** 2).sum()) // 2)
    if e["n_out"] < top_n or scores_cat.shape[0] <= top_n:
        return pairs, set(), set()
    v = s[-1]
    all_lists = list_of(np.arange(scores_cat.shape[0]), counts_b)
    taken = np.zeros(scores_cat.shape[0], bool)
    taken[e["src"]] = True
    tied = scores_cat == v
    return pairs, set(all_lists[tied & taken].tolist()), set(all_lists[tied & ~taken].tolist())


# ---- level boundaries -------------------------------------------------------------------------------------------------------------------
BOUNDARY_J = tuple(range(-4, 5))
ULP_STEPS = (-8, -3, -2, -1, 1, 2, 3, 8)
BAND_FRACTIONS = (0.1, 0.25, 0.5, 0.75, 0.9, 1.1, 1.5, 3.0)        # of the 1e-6 the reference adds to sqrt(area) / 224 before log2


def boundary_boxes():
    """-> (boxes [n, 4] float32 at the origin, kind [n] of "exact" | "ulp" | "band" | "edge", j [n])
    exact: sqrt(area) / 224 == 2^j in float32 arithmetic (side 224 * 2^j: 14 ... 3584, every product exact);
    ulp:   the height a few float32 ulps either side of that side;
    band:  the height shortened so that sqrt(area) / 224 falls short of 2^j by BAND_FRACTIONS of 1e-6 (fractions < 1: the epsilon of
           multilevel_rois.py:51 lifts the box to the upper level; > 1: it does not);
    edge:  a 1 x 1 box, a box of width zero (area 0), a box whose float32 area overflows."""
    rows, kind, js = [], [], []

    def add(w, h, k, j):
        w, h = np.float32(w), np.float32(h)
        rows.append([0.0, 0.0, w - np.float32(1), h - np.float32(1)])
        kind.append(k); js.append(j)

    for j in BOUNDARY_J:
        s = np.float32(224.0 * 2.0 ** j)
        add(s, s, "exact", j)
        for k in ULP_STEPS:
            h = s
            for _ in range(abs(k)):
                h = np.nextafter(h, np.float32(np.inf if k > 0 else 0), dtype=np.float32)
            add(s, h, "ulp", j)
        for f in BAND_FRACTIONS:
            add(s, np.float32(float(s) * (1.0 - 2.0 * f * 1e-6 / 2.0 ** j)), "band", j)
    rows.append([5.0, 5.0, 5.0, 5.0]); kind.append("edge"); js.append(0)
    rows.append([5.0, 5.0, 4.0, 9.0]); kind.append("edge"); js.append(0)
    rows.append([0.0, 0.0, 3e19, 3e19]); kind.append("edge"); js.append(0)
    return np.array(rows, np.float32), np.array(kind), np.array(js, np.int32)


def level_boxes(seed=0):
    """the rows of test_level_ranges: the boundary boxes first, then 300 synth.make_rois boxes with sides 8 ... 6000 pixels on an
    8192 x 8192 frame, so that every level of every range of K_RANGES is populated"""
    bb, _, _ = boundary_boxes()
    more = synth.make_rois(synth.rng(64, seed), 300, im_h=8192, im_w=8192, min_side=8.0, max_side=6000.0)
    return np.vstack([bb, more]).astype(np.float32), bb.shape[0]


def level_inputs(L, P, top_n):
    """level_boxes() dealt over L lists of stride P with tie-free scores, every list sorted; the boundary rows hold the highest
    scores, so that all of them are collected when top_n cuts.  -> (boxes [2, L, P, 4], scores [2, L, P], counts [2, L], nb);
    image 1 holds the same rows in another deal"""
    rows, nb = level_boxes()
    n = rows.shape[0]
    assert n <= L * P and nb <= top_n
    boxes = np.zeros((2, L, P, 4), np.float32)
    scores = np.full((2, L, P), GARBAGE_SCORE, np.float32)
    counts = np.zeros((2, L), np.int32)
    for b in range(2):
        rs = synth.rng(65, b)
        sc = np.empty(n, np.float32)
        sc[:nb] = _free(rs, nb, 0.6, 1.0)
        sc[nb:] = _free(rs, n - nb, 0.0, 0.5)
        which = rs.randint(0, L, n)
        if L > 1:
            which[which == 1] = 0                                            # list 1 stays empty
        for l in range(L):
            idx = np.flatnonzero(which == l)
            idx = idx[np.argsort(-sc[idx], kind="stable")]
            assert idx.size <= P
            counts[b, l] = idx.size
            boxes[b, l, :idx.size] = rows[idx]
            scores[b, l, :idx.size] = sc[idx]
    return boxes, scores, counts, nb


# ---- the mask branch -------------------------------------------------------------------------------------------------------------------
MASK_R, MASK_D, MASK_NCLS = 300, 104, 81
MASK_IM = np.array([[8000.0, 8000.0], [8000.0, 8000.0]], np.float32)
MASK_SF = np.array([1.0, 1.0], np.float32)


def mask_branch_inputs():
    """dtc_postprocess_detections_fpn, B = 2, R = 300, 81 classes, scale 1, no suppression (nms_thresh 1.5 at the call), max_det 100:
    the first rows are the exact and band boundary boxes (j = -3 ... 4) with zero deltas -- decoding returns them bit for bit (box at
    the origin, scale 1, frame 8000 x 8000) -- and the highest scores, so they are among the 100 detections; the rest are
    synth.make_rois boxes with random deltas and lower scores.
    -> (rois5 [B, R, 5], cls [B, R, 81], deltas [B, R, 324], rows [nbnd, 4] the boundary boxes used)"""
    bb, kind, j = boundary_boxes()
    sel = ((kind == "exact") | (kind == "band")) & (j >= -3)
    rows = bb[sel]
    nbnd = rows.shape[0]
    assert nbnd <= 80
    B, R = 2, MASK_R
    rs = synth.rng(66, 0)
    rois5 = np.zeros((B, R, 5), np.float32)
    cls = np.zeros((B, R, MASK_NCLS), np.float32)
    deltas = (rs.standard_normal((B, R, 4 * MASK_NCLS)) * 0.1).astype(np.float32)
    for b in range(B):
        rois5[b, :, 0] = b
        rois5[b, :, 1:] = synth.make_rois(rs, R, im_h=4000, im_w=4000, min_side=8.0, max_side=3000.0)
        rois5[b, :nbnd, 1:] = rows if b == 0 else rows[::-1]
        deltas[b, :nbnd] = 0
        top = _free(rs, nbnd, 0.6, 0.95)
        low = _free(rs, R - nbnd, 0.06, 0.5)
        fg = rs.randint(1, MASK_NCLS, R)
        cls[b, np.arange(R), fg] = np.concatenate([top, low])
        cls[b, :, 0] = np.float32(1.0) - cls[b].sum(1)
    return rois5, cls, deltas, rows
