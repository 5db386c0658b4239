"""bench.py --dump-outputs: what the full loop's last timed step computed, as float32 / float64 .npy files of at most 64 MB.  The loop's
inputs are seeded and --steps is the exact number of timed steps, so two runs that take the same number of loop steps (warmup + timed)
must dump the same arrays bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(out, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--no-kernel-legs", "--no-cpu-baseline", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step_reproducibly(tmp_path):
    a = bench(tmp_path / "a", steps=7, warmup=2)
    b = bench(tmp_path / "b", steps=6, warmup=3)                 # the same 9 loop steps, split differently
    assert (a["steps"], b["steps"]) == (7, 6) and a["ms_per_step"] > 0 and b["ms_per_step"] > 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"actions.npy", "reward.npy", "terminal.npy", "frame.npy", "batch_index.npy", "loss.npy", "params.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64), n
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.isfinite(np.load(tmp_path / "a" / "params.npy")).all() and np.load(tmp_path / "a" / "loss.npy")[0] > 0
