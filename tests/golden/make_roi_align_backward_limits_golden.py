"""Generate tests/golden/roi_align_backward_limits.npz from the REFERENCE ITSELF (build container only; needs the reference tree and g++).

    python tests/golden/make_roi_align_backward_limits_golden.py [reference root, default /root/reference]

The build of make_roi_align_backward_golden.py (the reference's unmodified lib/cppcuda/roi_align_backward_cpu.cpp, compiled where
it lies into a temporary directory that is deleted afterwards) run on the cases of tests/roi_align_backward_limit_cases.py.

Per case <c> of GOLDEN_CASES: <c>_digest (sha1 of the inputs, bad rows included) and <c>_L<l>, the float32 gradient of level l
[B, C', H, W]: the reference run on the rows of level l that the contract does not call bad (for those the reference indexes out
of range), every channel or, for the `channels` cases, the channels sample_channels() names.  4-column RoIs do not occur.
`nonfinite_top` is not recorded: the payload of the NaNs it produces is the compiler's choice; it rests on the restatement.
The file is written with fixed zip timestamps: a second run gives the same bytes.
"""
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import roi_align_backward_limit_cases as lc  # noqa: E402
import roi_align_backward_ref as rb  # noqa: E402
from make_roi_align_backward_golden import build_reference, run_reference, write_npz  # noqa: E402


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    tmp = tempfile.mkdtemp(prefix="roi_align_backward_limits_ref_")
    arrs = {}
    try:
        L = build_reference(ref_root, tmp)
        for name in lc.GOLDEN_CASES:
            c = lc.case(name)
            t0 = time.time()
            ch = lc.sample_channels(name, c["top"].shape[1])
            top = np.ascontiguousarray(c["top"][:, ch])
            levels = lc.levels_of(c)
            bad = set(lc.bad_rows_by_rule(c))
            assert bad == set(c["bad_rows"]), name
            for l, ((h, w), s) in enumerate(zip(c["shapes"], c["scales"])):
                rows = np.array([r for r in np.where(levels == l)[0] if r not in bad], np.int64)
                arrs["%s_L%d" % (name, l)] = run_reference(L, top[rows], c["rois"][rows], c["batch"], h, w, s, c["ratio"])
            arrs[name + "_digest"] = rb.digest(c)
            t1 = time.time()
            same = all(np.array_equal(arrs["%s_L%d" % (name, l)].view(np.uint32), r[0][:, ch].view(np.uint32))
                       for l, r in enumerate(lc.restatement(name)))
            print("%-24s top %-18s levels %d  reference %.2f s  restatement %.2f s  equal: %s"
                  % (name, top.shape, len(c["shapes"]), t1 - t0, time.time() - t1, same))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(HERE, "roi_align_backward_limits.npz")
    write_npz(path, arrs)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(arrs)))


if __name__ == "__main__":
    main()
