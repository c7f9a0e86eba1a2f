"""Generate tests/golden/solver_lr.npz from the REFERENCE ITSELF (build container only; needs the reference tree).

    python tests/golden/make_solver_golden.py

lib/utils/solver.py is imported where it lies (by file path: it imports nothing) and its get_step_index and get_lr_at_iter are run
at the iterations around every edge of the schedule: the start and the end of the warm-up, the two decay steps, max_iter and
beyond.  Only results are stored, as data:
  iters [15] int64, step_index [15] int64, lr_linear [15] and lr_constant [15] float64 (warm_up_method 'linear', the default, and
  'constant'), unknown_method_error: the name of the exception an unknown warm_up_method raises while warming up (iteration 0),
  unknown_method_late: the float64 result with the same unknown method after the warm-up (iteration 500), where the reference does
  not look at it.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import ref_harness as rh  # noqa: E402

REF_SOLVER = os.path.join(rh.REF_ROOT, "lib", "utils", "solver.py")
ITERS = [0, 1, 249, 250, 499, 500, 501, 239999, 240000, 240001, 319999, 320000, 359999, 360000, 400000]


def main():
    spec = importlib.util.spec_from_file_location("reference_solver", REF_SOLVER)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    try:
        ref.get_lr_at_iter(0, warm_up_method='cosine')
        error = ""
    except Exception as e:                                   # noqa: BLE001 (whatever the reference raises is what is recorded)
        error = type(e).__name__
    np.savez(os.path.join(HERE, "solver_lr.npz"),
             iters=np.array(ITERS, np.int64),
             step_index=np.array([ref.get_step_index(i) for i in ITERS], np.int64),
             lr_linear=np.array([ref.get_lr_at_iter(i) for i in ITERS], np.float64),
             lr_constant=np.array([ref.get_lr_at_iter(i, warm_up_method='constant') for i in ITERS], np.float64),
             unknown_method_error=np.array(error),
             unknown_method_late=np.float64(ref.get_lr_at_iter(500, warm_up_method='cosine')))


if __name__ == "__main__":
    main()
