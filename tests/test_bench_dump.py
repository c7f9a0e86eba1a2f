"""bench.py --dump-outputs: what the timed path computed in its last step lands in DIR as float32 / float64 .npy files, 64 MB at
most, and the same arguments give the same files (the inputs are seeded), so that two builds can be compared output by output.
-m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--sustain-seconds", "0", "--no-cpu-baseline", "--no-modes", "--side-steps", "0", "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


@pytest.mark.parametrize("workload", ["cfg3", "cfg2"])
def test_dump_outputs_repeatable_and_bounded(tmp_path, workload):
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    wl = ("--workload", workload)
    out = _run(a, 5, wl)
    assert out["steps"] == 5
    _run(b, 3, wl)                            # last step on the same input set as 5 steps (two sets, taken in turn)
    _run(c, 4, wl)                            # last step on the other input set
    da, db, dc = _load(a), _load(b), _load(c)
    assert sorted(da) == sorted(db) == sorted(dc) and {"dets", "det_count", "rois", "n_rois", "box_feats_sample"} <= set(da)
    assert sum(os.path.getsize(os.path.join(a, k + ".npy")) for k in da) <= 64 << 20
    for k, v in da.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.array_equal(v, db[k]), k
    assert da["det_count"].min() > 0 and np.isfinite(da["box_feats_sample"]).all()
    assert not np.array_equal(da["dets"], dc["dets"])
