"""Generate tests/golden/mask_geometry_sizes.npz from the REFERENCE ITSELF (build container only; needs the reference tree +
`make -C oracle ref`), in the style of make_golden.py, which it leaves alone (mask_geometry.npz keeps M = 14 / 28).

    python tests/golden/make_mask_geometry_sizes.py

The reference's own expand_boxes (lib/utils/boxes.py:245-261, imported in place) + the int32 truncation of segm_results
(lib/utils/result_utils.py:182-184) for every mask side the paste kernel is tested at (tests/output_args_cases.py: MASK_SIDES,
M = 1 ... 62; the issue's M = 7 and 56 among them), on the boxes of tests/test_hip_mask_output_args.py's mask-side test plus 40
seeded ones.  Stored: ref_boxes [46, 4] float32 and exp_int_M<M> [46, 4] int32.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import output_args_cases as oc  # noqa: E402


def main():
    ns = rh.load_reference()
    ref_boxes = oc.geometry_boxes()
    arrs = {"ref_boxes": ref_boxes}
    for M in oc.MASK_SIDES:
        arrs["exp_int_M%d" % M] = ns.boxes.expand_boxes(ref_boxes, (M + 2.0) / M).astype(np.int32)
    path = os.path.join(HERE, "mask_geometry_sizes.npz")
    np.savez_compressed(path, **arrs)
    print("%-28s %7.1f KB  %s" % ("mask_geometry_sizes", os.path.getsize(path) / 1024.0, sorted(arrs)))


if __name__ == "__main__":
    main()
