#!/bin/bash
# (the steps of this run that used builds or knobs removed since are cut: git show 7c22f5a:tools/r04/runs/gpu9.sh)
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT" || exit 1
timeout 900 python -m pytest tests/test_hip_fpn_det_mask.py tests/test_hip_pipeline.py tests/test_hip_detector.py -x -q 2>&1 | tail -3
bash tools/r04/runs/gpu8.sh 2>&1 | grep -E "det_candidates|det_finalize|default:"
