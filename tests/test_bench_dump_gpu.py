"""bench.py --dump-outputs on the GPU: a plain one-GPU run writes the last timed
step's mask and counters as float .npy files equal to the CPU oracle's on the
same generated reads, identical from run to run, and its line carries no leg
that belongs to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# two batches, the second one short; steps > 1 so a step that did not reset would show
READS, BATCH, STEPS = 150_001, 100_000, 3


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--reads", str(READS), "--batch-reads", str(BATCH),
                        "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_dump_outputs_match_the_oracle_and_repeat(tmp_path):
    line = _bench(tmp_path / "a")
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    assert line["value"] > 0
    assert "cpu_baseline" not in line and "e2e" not in line
    assert sorted(os.listdir(tmp_path / "a")) == ["counters.npy", "mask.npy"]
    mask, ctr = np.load(tmp_path / "a" / "mask.npy"), np.load(tmp_path / "a" / "counters.npy")
    assert mask.dtype == np.float32 and ctr.dtype == np.float64

    # bench.py's C2: seed 2, 150 bp, the generator's 5 % / 5 % / 1 per 1024
    reads = O.synth(READS, seed=2, L=150, trunc_pct=5, bad_pct=5, n_per_1024=1)
    p = H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,")
    m_o, _, c_o = O.run(p, reads)
    assert np.array_equal(mask, m_o.astype(np.float32))
    assert np.array_equal(ctr, c_o.astype(np.float64))   # ONE step's counters: the last step's

    _bench(tmp_path / "b")
    for f in ("mask.npy", "counters.npy"):
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "a" / f))
