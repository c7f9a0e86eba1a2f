"""The limit cases of the flip entries (tests/flip_limit_cases.py) without a GPU and without the library: for every case THE CONDITION
IT IS NAMED FOR, computed from the restatement alone (tests/flip_ref.py), so that a case that drifts fails here and does not pass
vacuously on the GPU (tests/test_hip_flip_limits.py); and the sparse form flip_ref.flip_rle_sparse held to flip_ref.flip_rle_runs on
every run list of the two suites that can be decoded, and to answers written out by hand where none can."""
import numpy as np
import pytest

import flip_cases as fc
import flip_limit_cases as lc
import flip_ref as fr

CHUNK = lc.CHUNK


def group_starts(runs, h, w):
    """flip_ref.cut's pieces in input order -> (pieces, [piece starts a column group])"""
    pieces = fr.cut(runs, h, w)
    return pieces, [s % h == 0 for _, s, _ in pieces]


def run_chunks_without_a_group_start(runs, h, w):
    """the chunks of CHUNK input runs, other than the last, all of whose runs leave a piece and none of whose pieces starts a group"""
    starts = np.concatenate([[0], np.cumsum(np.asarray(runs, np.int64))])
    found = []
    for c in range((len(runs) - 1) // CHUNK):                  # not the last chunk: somebody must read what it carries
        ks = range(c * CHUNK, (c + 1) * CHUNK)
        if all(runs[k] > 0 and starts[k] % h != 0 and starts[k] // h == (starts[k + 1] - 1) // h for k in ks):
            found.append(c)
    return found


def piece_chunks_without_a_group_start(runs, h, w):
    """pass 2 walks the pieces backwards, output piece o = input piece T - 1 - o, and looks at piece T - o (or at the end, T): the
    chunks of CHUNK output pieces, other than the last, in which that piece never starts a group"""
    pieces, first = group_starts(runs, h, w)
    T = len(pieces)
    found = []
    for c in range((T - 1) // CHUNK):
        if all(T - o != T and not first[T - o] for o in range(c * CHUNK, (c + 1) * CHUNK)):
            found.append(c)
    return found


# ---- the sparse form -------------------------------------------------------------------------------------------------------------------------
def old_run_lists():
    rows = [(h, w, r) for _, h, w, r in fc.rle_rows()]
    rows.append(fc.BLOB_HW + (fc.blob_runs(),))
    m = np.random.RandomState(7).rand(401, 367) < 0.5           # test_flip_rle_more_than_65536_runs
    rows += [(401, 367, fr.encode(m)), (401, 367, [3 * 401 + 5, 2, 401 * 367 - 3 * 401 - 7])]
    rows += [(5, 7, r) for r in ([35], [0, 35], [4, 3, 0, 2, 26], [10, 5, 20], [0, 0, 4, 0, 0, 3, 0, 2, 6, 0, 20, 0], [7, 28])]
    rows += [(3, 4, r) for r in ([5, 2, 5], [12], [0, 12], [1, 11])]
    rows.append((5, 7, fr.encode(np.arange(35).reshape(7, 5).T % 3 == 0)))
    return rows


def new_run_lists():
    rows = list(lc.tall_column_rows()) + [z[:3] for z in lc.zero_run_rows()] + list(lc.GROWTH_ROWS) + list(lc.EDGE_ROWS)
    rows += [(7, 5, r) for r in lc.IM_SIZE_ROWS[0][1][:2]] + [(1, 1, [1]), (1, 1, [0, 1]), (0, 9, [0]), (0, 9, [0, 0]), (5, 7, [10, 5, 20])]
    c = lc.counts_case()
    rows += [(6, 8, c["runs"].view(np.uint32)[b, r, :c["n_runs"][b, r]].tolist()) for b in range(5) for r in range(5)]
    return rows


def test_sparse_form_equals_the_decoding_one_on_every_old_case():
    rows = old_run_lists()
    assert len(rows) >= 30 and max(len(r) for _, _, r in rows) > 65536
    for h, w, r in rows:
        assert fr.flip_rle_sparse(r, h, w) == fr.flip_rle_runs(r, h, w), (h, w, r[:8])


def test_sparse_form_equals_the_decoding_one_on_every_new_case():
    for h, w, r in new_run_lists():
        assert h * w <= lc.DENSE_PIXELS
        assert fr.flip_rle_sparse(r, h, w) == fr.flip_rle_runs(r, h, w), (h, w, r[:8])


def test_sparse_form_gives_the_answers_written_out_by_hand():
    """at 2^30 pixels nothing can be decoded: the expected lists of flip_limit_cases.PIXELS_2_30 were derived by hand"""
    assert lc.P30 == 1 << 30 and len(lc.PIXELS_2_30) >= 5
    for name, runs, want in lc.PIXELS_2_30:
        assert sum(runs) == sum(want) == lc.P30 and fr.flip_rle_sparse(runs, lc.S, lc.S) == want, name
        assert fr.flip_rle_sparse(want, lc.S, lc.S) == ([r for r in runs]), name               # and back
    # the same masks on a 4 x 4 image, where they can be decoded: the derivation itself
    assert fr.flip_rle_runs([1, 1, 14], 4, 4) == [13, 1, 2] and fr.flip_rle_runs([15, 1], 4, 4) == [3, 1, 12]
    assert fr.flip_rle_runs([12, 1, 3], 4, 4) == [0, 1, 15]
    assert fr.flip_rle_runs([4, 12, 1, 2, 13], 4, 8) == [13, 2, 1, 12, 4]   # columns 1 .. 3 and rows 1 .. 2 of column 4


def test_batched_restatement_takes_either_form():
    b = lc.rle_batches()["counts"][0]
    a = fr.flip_rle_batched(b["runs"], b["n_runs"], b["im_size"], b["flipped"], 64, b["counts"])
    s = fr.flip_rle_batched(b["runs"], b["n_runs"], b["im_size"], b["flipped"], 64, b["counts"], flip=fr.flip_rle_sparse)
    assert a[0] == s[0] and np.array_equal(a[1], s[1]) and np.array_equal(a[2], s[2])


# ---- dtc_flip_rle: the conditions --------------------------------------------------------------------------------------------------------------
def test_tall_column_has_whole_chunks_inside_one_column_group():
    rows = lc.tall_column_rows()
    assert len(rows[0][2]) == 605 and [r[:2] for r in rows] == [(600, 3), (1100, 2), (1100, 2)]
    for h, w, runs in rows:
        pieces, first = group_starts(runs, h, w)
        T = len(pieces)
        sizes = np.diff([i for i, f in enumerate(first) if f] + [T])
        assert sizes.max() > 2 * CHUNK, sizes.max()               # a column group of more than 512 pieces
        in_runs, in_pieces = run_chunks_without_a_group_start(runs, h, w), piece_chunks_without_a_group_start(runs, h, w)
        assert in_runs and in_pieces, (h, w, in_runs, in_pieces)
        # and the chunk behind each of them still has a piece of that group that is not its first: the carried value is read
        c = in_runs[0]
        starts = np.concatenate([[0], np.cumsum(runs)])
        k = (c + 1) * CHUNK
        assert starts[k] % h != 0 and starts[k] // h == starts[c * CHUNK] // h
        c = in_pieces[0]
        o = (c + 1) * CHUNK
        assert not any(first[T - o: T - c * CHUNK + 1])           # the first piece of the next chunk looks through the whole chunk for its group's end
    # the old cases have no such chunk
    for h, w, runs in old_run_lists():
        assert not run_chunks_without_a_group_start(runs, h, w) and not piece_chunks_without_a_group_start(runs, h, w), (h, w)


def test_zero_run_chunk_leaves_no_piece():
    (h0, w0, a, a0), (h1, w1, b, b0) = lc.zero_run_rows()
    assert a[4:604] == [0] * 600 and a[:4] == a0[:4] and a[604:] == a0[4:] and min(a0[1:]) > 0
    assert not any(a[CHUNK:2 * CHUNK]) and len(a) > 2 * CHUNK
    assert len(b0) > CHUNK and b[CHUNK:2 * CHUNK] == [0] * CHUNK and min(b[1:CHUNK]) > 0 and min(b[2 * CHUNK:]) > 0 and len(b) > 2 * CHUNK
    for h, w, spliced, plain in lc.zero_run_rows():
        assert sum(spliced) == sum(plain) == h * w and len(spliced) % 2 == len(plain) % 2
        assert fr.cut(spliced, h, w) != [] and len(fr.cut(spliced[CHUNK:2 * CHUNK], h, w)) == 0
        assert fr.flip_rle_sparse(spliced, h, w) == fr.flip_rle_runs(spliced, h, w) == fr.flip_rle_runs(plain, h, w)


def test_growth_is_past_two_and_a_half():
    needs = []
    for h, w, runs in lc.GROWTH_ROWS:
        assert sum(runs) == h * w
        needs.append(len(fr.flip_rle_runs(runs, h, w)))
        assert needs[-1] > 2.5 * len(runs)
    assert [len(r) for _, _, r in lc.GROWTH_ROWS] == [301, 306] and needs == [780, 826]
    rs, os_ = lc.GROWTH_STRIDES
    assert -(-max(needs) // CHUNK) > -(-max(len(r) for _, _, r in lc.GROWTH_ROWS) // CHUNK) and rs < min(needs) <= max(needs) <= os_
    batch, strides = lc.rle_batches()["growth"]
    assert batch["runs"].shape[2] == rs and strides == [os_, 780, 779, 826, 825]
    for out_stride in strides:
        _, out_n, need = lc.rle_expected("growth", out_stride)
        assert need.reshape(-1).tolist() == needs                # exact whether it fits or not
        assert out_n.reshape(-1).tolist() == [v if v <= out_stride else -1 for v in needs]


def test_chunk_edges_have_the_counts_they_are_named_for():
    one_row, three_rows, exact = lc.EDGE_ROWS[:5], lc.EDGE_ROWS[5:10], lc.EDGE_ROWS[10:]
    assert [len(r) for _, _, r in one_row] == list(lc.EDGE_COUNTS) == [len(r) for _, _, r in three_rows]
    for h, w, r in lc.EDGE_ROWS:
        assert sum(r) == h * w
    for h, w, r in one_row:
        assert len(fr.cut(r, h, w)) == len(r)
    for h, w, r in three_rows:
        assert h == 3 and len(fr.cut(r, h, w)) > len(r) + 50     # pieces != runs
    assert [len(fr.cut(r, h, w)) for h, w, r in exact] == list(lc.EDGE_PIECES) and [len(r) for _, _, r in exact] == [192, 384]


def test_pixels_2_30_fill_the_record():
    """h w = 2^30 exactly: the largest start, 2^30 - 1, shifted by 2 is the largest 32-bit record"""
    b, _ = lc.rle_batches()["pixels_2_30"]
    assert fr.side(b["im_size"][0, 0]) * fr.side(b["im_size"][0, 1]) == 1 << 30 and b["flipped"] == (1, 0)
    starts = [s for _, runs, _ in lc.PIXELS_2_30 for _, s, e in fr.cut(runs, lc.S, lc.S)]
    assert max(starts) == (1 << 30) - 1 and (max(starts) << 2 | 3) == (1 << 32) - 1
    lists, out_n, need = lc.rle_expected("pixels_2_30", 8)
    assert lists[0] == [p[2] for p in lc.PIXELS_2_30] and lists[1] == [p[1] for p in lc.PIXELS_2_30] and (out_n > 0).all()


def test_too_many_pixels_states():
    b, _ = lc.rle_batches()["too_many_pixels"]
    sides = [(fr.side(h), fr.side(w)) for h, w in b["im_size"]]
    assert sides == [(65536, 32768), (1 << 30, 1), (32768, 32769)]
    runs = b["runs"].view(np.uint32).astype(np.int64)
    for n, (h, w) in enumerate(sides):                            # each image: a list summing to the clipped and one to the true product
        sums = [int(runs[n, r, :b["n_runs"][n, r]].sum()) for r in range(3)]
        assert sums[0] == 1 << 30 and sums[1] == (h * w if n != 1 else 3000000000) and sums[2] in (1 << 30, h * w)
    lists, out_n, need = lc.rle_expected("too_many_pixels", 4)
    assert out_n[0].tolist() == out_n[2].tolist() == [-1, -1, -1] and not need[0].any() and not need[2].any()
    # (3e9, 1.5) is 2^30 x 1 after the side rule: 2^30 pixels are allowed, and a single column is its own mirror image.  Only the list
    # that sums to 3e9 is refused
    assert out_n[1].tolist() == [1, -1, 2] and need[1].tolist() == [1, 0, 2] and lists[1][0] == [1 << 30] and lists[1][2] == [5, (1 << 30) - 5]


def test_im_size_rules():
    b, _ = lc.rle_batches()["im_sizes"]
    assert [(fr.side(h), fr.side(w)) for h, w in b["im_size"]] == [(7, 5), (0, 9), (0, 9), (1, 1)] and np.isnan(b["im_size"][2, 0])
    lists, out_n, need = lc.rle_expected("im_sizes", 12)
    assert out_n[0, 0] > 1 and lists[0][1] == [35] and out_n[0, 2] == -1       # a 7 x 5 list; 36 does not sum to 35
    for n in (1, 2):                                             # no pixels: [0] -> [0], [5] -> -1, [0, 0] -> [0]
        assert lists[n][0] == [0] and out_n[n].tolist() == [1, -1, 1] and need[n].tolist() == [1, 0, 1] and lists[n][2] == [0]
    assert lists[3][0] == [1] and lists[3][1] == [0, 1] and out_n[3, 2] == -1


def test_wrapped_sums_are_right_modulo_2_32_only():
    h, w = lc.WRAPPED_HW
    for r in lc.WRAPPED_ROWS[:2]:
        assert sum(r) % 2 ** 32 == h * w and sum(r) != h * w and max(r) < 2 ** 32
    assert len(lc.WRAPPED_ROWS[2]) == 300 and sum(lc.WRAPPED_ROWS[2][:2]) > h * w and sum(lc.WRAPPED_ROWS[3]) == h * w
    b, _ = lc.rle_batches()["wrapped_sum"]
    assert b["runs"].view(np.uint32)[0, 0, 0] == 2 ** 32 - 1 and b["runs"][0, 0, 0] == -1           # the bits travel in int32
    lists, out_n, need = lc.rle_expected("wrapped_sum", 300)
    assert out_n[0].tolist() == [-1, -1, -1, 3] and need[0].tolist() == [0, 0, 0, 3]
    assert out_n[1].tolist() == [2, 3, 300, 3] and lists[1][2] == [2 ** 32 - 1] * 300            # not flipped: copied, whatever the sum


def test_counts_clamp():
    b, _ = lc.rle_batches()["counts"]
    assert b["counts"].tolist() == [-3, 0, 2, 5, 9] and b["runs"].shape[:2] == (5, 5) and set(b["flipped"]) == {0, 1}
    lists, out_n, need = lc.rle_expected("counts", 64)
    assert [sum(x is not None for x in per) for per in lists] == [0, 0, 2, 5, 5] and (out_n[2, :2] > 0).all() and not out_n[2, 2:].any()
    assert lists[3][0] == b["runs"][3, 0, :b["n_runs"][3, 0]].tolist() and lists[4][0] != b["runs"][4, 0, :b["n_runs"][4, 0]].tolist()


def test_padding_is_poisoned():
    for name, (b, _) in lc.rle_batches().items():
        runs, n = b["runs"].view(np.uint32), b["n_runs"]
        for i in range(n.shape[0]):
            for r in range(n.shape[1]):
                assert (runs[i, r, max(int(n[i, r]), 0):] == lc.POISON).all(), (name, i, r)
        assert not b["runs"].flags.writeable


# ---- boxes, polygons, prep -----------------------------------------------------------------------------------------------------------------
def test_box_cases_leave_block_zero():
    assert np.float32(2 ** 24 + 1) == 2 ** 24                  # the restatement's float32(w) and the kernel's (float)im_width are one number
    shapes = [c[0] for c in lc.BOX_CASES]
    assert shapes == [(2, 300, 12), (1, 1, 4096), (2, 70000, 4)]
    threads = [R * cols // 4 for _, R, cols in shapes]
    assert threads[0] == 900 and threads[0] % 256 and threads[1] == 1024 and -(-threads[2] // 256) == 274 and shapes[2][1] > 65535
    assert {w for c in lc.BOX_CASES for w in c[1]} >= {0, 1, 2 ** 24 + 1}
    for k, (shape, widths, calls) in enumerate(lc.BOX_CASES):
        b = lc.boxes(k)
        bits = b.view(np.uint32).reshape(-1, 4)
        for col in range(4):                                      # NaN with a payload, inf, -0.0 and denormals among x and among y
            have = set(bits[:, col].tolist())
            if shape[1] * shape[2] >= 1024:
                assert have >= set(lc.BOX_SPECIALS.view(np.uint32).tolist()), (k, col)
        assert any(cnt is not None and (min(cnt) < 0 or max(cnt) > shape[1]) for _, cnt in calls) or k == 1
        for flags, cnt in calls:
            want = fr.flip_boxes_batched(b, widths, flags, cnt)
            for i in range(shape[0]):                             # unflipped images and rows past the clamped count: bit copies
                n = shape[1] if cnt is None else min(max(cnt[i], 0), shape[1])
                n = n if flags[i] else 0
                assert want[i, n:].tobytes() == b[i, n:].tobytes() and want[i, :, 1::2].tobytes() == b[i, :, 1::2].tobytes()
                if n:
                    assert want[i, :n].tobytes() != b[i, :n].tobytes()
    assert fr.flip_boxes(np.array([[3, 0, 5, 0]], np.float32), 2 ** 24 + 1)[0].tolist() == [2 ** 24 - 6, 0, 2 ** 24 - 4, 0]


def test_polygon_cases_cross_the_block_border_and_meet_the_clamp():
    xy = lc.polygon_points()
    assert xy.shape == (3, 1000, 2) and lc.POLY_NP == 7 and (xy[:2, lc.POLY_X_AT, 0] == 639.49).all()
    assert np.float32(640 - 639.49 - 1) != np.float32(640) - np.float32(639.49) - np.float32(1)
    lasts = [v for last, _ in lc.POLY_CALLS for v in last]
    assert {1000, 257, -5, 2000} <= set(lasts) and any(0 in f for _, f in lc.POLY_CALLS)
    for last, flags in lc.POLY_CALLS:
        assert lc.polygon_ptr(last)[:, lc.POLY_NP].tolist() == list(last)
        w64, w32 = lc.polygons_expected(xy, last, flags)
        for b in range(3):
            n = min(max(last[b], 0), 1000) if flags[b] else 0
            assert w64[b, n:].tobytes() == xy[b, n:].tobytes() and w64[b, :, 1].tobytes() == xy[b, :, 1].tobytes()
            assert (w64[b, :n, 0] == lc.POLY_WIDTHS[b] - xy[b, :n, 0] - 1).all() and (n == 0 or (w64[b, :n, 0] != xy[b, :n, 0]).any())
        assert w32.dtype == np.float32 and w32.tobytes() == w64.astype(np.float32).tobytes()
    w64, w32 = lc.polygons_expected(xy, *lc.POLY_CALLS[0])
    assert w32[0, 255, 0] == np.float32(-0.49) and w32[1, 256, 0] == np.float32(-0.49) and w64[1, 257, 0] == xy[1, 257, 0]
    w64, _ = lc.polygons_expected(xy, *lc.POLY_CALLS[2])
    assert w64[0, 255, 0] != 639.49 and w64[0, 256, 0] == 639.49 and w64[1, 999, 0] != 639.49 and w64[2].tobytes() == xy[2].tobytes()


def test_prep_cases_are_wider_than_a_block():
    u8, f32 = lc.prep_images()
    assert u8.shape == f32.shape == (40, 301, 3) and u8.dtype == np.uint8 and f32.dtype == np.float32
    assert lc.PREP_TARGETS == ((40, 400), (20, 400), (80, 700)) and 301 > 256 and 301 % 2 == 1
    assert not np.array_equal(fr.flip_image(u8), u8)
